// e2e.hip -- End2End detection (Config.End2End, Data/Config.cs:239): the NMS-free post-process of Detect and the second
// BatchNorm running-statistics update of the aliased one2one towers.
//
// Restates (reference file:line under YoloSharp/):
//   Modules/Head.cs:117-127  postprocess: split boxes / scores, get_topk_index, gather the boxes, cat -> [B, k, 6]
//   Modules/Head.cs:321-339  Segment.postprocess: the same selection, plus the nm mask coefficients of the selected anchors -> [B, k, 6 + nm]
//   Modules/Head.cs:175-196  get_topk_index (agnostic_nms = false): k = min(max_det, A); stage 1 = the k anchors with the largest
//                            max-over-classes score; stage 2 = the k largest of the k * nc gathered scores, flattened;
//                            anchor = stage1[idx / nc], class = idx % nc
//   Utils/Ops.cs:258-267     non_max_suppression(end2end: true): rows with score > conf_thres, at most max_det
//   Modules/Head.cs:89-106   training forward: the one2one branch runs the SAME modules a second time (one2one_init copies references,
//                            :152-167), so every BatchNorm of the towers takes its momentum update twice with the same batch statistics
//
// Order.  ATen's topk leaves the order among equal values unspecified; this project's rule (as in the assigner, loss.hip) is
// (value descending, index ascending): in stage 1 the index is the anchor, in stage 2 the flattened [stage-1 rank][class] index.
// +0 and -0 are equal, NaN sorts first (ATen's topk treats NaN as the largest value).  The result is a pure function of the input:
// every selection compares 64-bit keys (ordered value bits << 32 | ~index) that are pairwise distinct, the only atomics are integer
// counters, and no float is ever added.
//
// Launches (ys_e2e_topk_launch): e2e_classmax_kernel, a wide grid that reads the [nc, A] class planes once, coalesced along A, and
// writes amax[B][A]; then e2e_topk_kernel, ONE workgroup per image, which selects twice with the same routine:
//   radix select -- four 8-bit passes over the ordered value bits with a 256-bin integer histogram in LDS find the k-th largest
//   value T and how many entries equal to T belong to the result; entries above T are appended in any order, the entries equal to T
//   in index order (a workgroup scan); the k keys are then ordered:
//     k <= E2E_RANK_MAX (2048; every max_det the reference uses): in LDS, by rank counting (k broadcast reads per thread, no barrier)
//     k >  E2E_RANK_MAX: the general path, a bitonic sort in a global workspace (k padded to a power of two)
// Values (amax, the k * nc gathered scores) stay in global memory (L2-resident: 33600 anchors are 134 KB per image, more than a
// workgroup's static LDS), so the kernel is correct for any A >= 1, nc >= 1, max_det >= 1 with k * nc < 2^30.
#include "ops_stage.h"

#define E2E_T 512            // threads of the per-image selection workgroup
#define E2E_RANK_MAX 2048    // keys ordered in LDS by rank counting (2 x 16 KB)
#define E2E_CM_T 256

typedef unsigned long long e2e_u64;

// order-preserving bits: larger value <=> larger key
__device__ inline unsigned e2e_key(float v) {
  if (v != v) return 0xFFFFFFFFu;
  if (v == 0.0f) return 0x80000000u;
  const unsigned u = ys_f2u(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ inline e2e_u64 e2e_comp(unsigned key, unsigned idx) { return ((e2e_u64)key << 32) | (e2e_u64)(~idx); }
__device__ inline unsigned e2e_comp_idx(e2e_u64 c) { return ~(unsigned)(c & 0xFFFFFFFFull); }

// ------------------------------------------------------------------ max over classes per anchor (scores.max(dim: -1), Head.cs:190)
__global__ void __launch_bounds__(E2E_CM_T)
e2e_classmax_kernel(const float* __restrict__ pred, int nc, int extra, int A, float* __restrict__ amax) {
  const int a = blockIdx.x * E2E_CM_T + threadIdx.x;
  const long b = blockIdx.y;
  if (a >= A) return;
  const float* p = pred + (b * (4 + nc + extra) + 4) * (long)A + a;
  float m = p[0];
#pragma unroll 8
  for (int c = 1; c < nc; c++) {
    const float v = p[(long)c * A];
    m = (v > m || v != v) ? v : m;          // NaN propagates, like amax
  }
  amax[b * A + a] = m;
}

// The k first entries of vals[0, N) in (value descending, index ascending) order, as keys in the returned array [0, k).
// buf: kp2 keys of work space (LDS when k <= E2E_RANK_MAX, else global); s_out: E2E_RANK_MAX keys of LDS.  1 <= k <= N.
__device__ inline const e2e_u64* e2e_select_sorted(const float* __restrict__ vals, int N, int k, e2e_u64* buf, e2e_u64* s_out, int kp2) {
  __shared__ unsigned s_hist[256];
  __shared__ unsigned s_digit;
  __shared__ int s_krem, s_cnt;
  __shared__ int s_wsum[E2E_T / 64];
  const int tid = threadIdx.x;
  unsigned prefix = 0u, mask = 0u;
  int krem = k;
  for (int shift = 24; shift >= 0; shift -= 8) {
    for (int i = tid; i < 256; i += E2E_T) s_hist[i] = 0u;
    __syncthreads();
    for (int i = tid; i < N; i += E2E_T) {
      const unsigned key = e2e_key(vals[i]);
      if ((key & mask) == prefix) atomicAdd(&s_hist[(key >> shift) & 255u], 1u);
    }
    __syncthreads();
    if (tid < 64) {     // wave 0: lane l owns bins [4 l, 4 l + 4); the bin in which the count from the top reaches krem
      int c[4], sum = 0;
#pragma unroll
      for (int j = 0; j < 4; j++) { c[j] = (int)s_hist[4 * tid + j]; sum += c[j]; }
      int incl = sum;
      for (int m = 1; m < 64; m <<= 1) { const int v = __shfl_down(incl, m); if (tid + m < 64) incl += v; }
      int above = incl - sum;
      if (above < krem && krem <= above + sum) {
#pragma unroll
        for (int j = 3; j >= 0; j--) {
          if (krem > above && krem <= above + c[j]) { s_digit = (unsigned)(4 * tid + j); s_krem = krem - above; }
          above += c[j];
        }
      }
    }
    __syncthreads();
    prefix |= s_digit << shift; mask |= 255u << shift; krem = s_krem;
  }
  // prefix = key of the k-th entry; krem of the entries equal to it belong to the result, the lowest indices first
  const int n_gt = k - krem;
  if (tid == 0) s_cnt = 0;
  for (int i = k + tid; i < kp2; i += E2E_T) buf[i] = 0ull;      // padding of the bitonic form: below every real key
  __syncthreads();
  const int chunk = (N + E2E_T - 1) / E2E_T;
  const int i0 = tid * chunk < N ? tid * chunk : N, i1 = i0 + chunk < N ? i0 + chunk : N;
  int neq = 0;
  for (int i = tid; i < N; i += E2E_T) {
    const unsigned key = e2e_key(vals[i]);
    if (key > prefix) buf[atomicAdd(&s_cnt, 1)] = e2e_comp(key, (unsigned)i);
  }
  for (int i = i0; i < i1; i++) neq += e2e_key(vals[i]) == prefix ? 1 : 0;
  int incl = neq;
  for (int m = 1; m < 64; m <<= 1) { const int v = __shfl_up(incl, m); if ((tid & 63) >= m) incl += v; }
  if ((tid & 63) == 63) s_wsum[tid >> 6] = incl;
  __syncthreads();
  int rank = incl - neq;
  for (int w = 0; w < (tid >> 6); w++) rank += s_wsum[w];
  if (neq > 0 && rank < krem)
    for (int i = i0; i < i1 && rank < krem; i++)
      if (e2e_key(vals[i]) == prefix) { buf[n_gt + rank] = e2e_comp(prefix, (unsigned)i); rank++; }
  __syncthreads();
  if (k <= E2E_RANK_MAX) {
    // rank counting: the keys are pairwise distinct, so the number of larger keys is the position
    for (int i = tid; i < k; i += E2E_T) {
      const e2e_u64 me = buf[i];
      int r = 0;
      for (int j = 0; j < k; j++) r += buf[j] > me ? 1 : 0;
      s_out[r] = me;
    }
    __syncthreads();
    return s_out;
  }
  for (int size = 2; size <= kp2; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int i = tid; i < (kp2 >> 1); i += E2E_T) {
        const int pos = 2 * i - (i & (stride - 1));
        const e2e_u64 x = buf[pos], y = buf[pos + stride];
        const bool desc = (pos & size) == 0;
        if (desc ? x < y : x > y) { buf[pos] = y; buf[pos + stride] = x; }
      }
      __syncthreads();
    }
  }
  return buf;
}

// ------------------------------------------------------------------ get_topk_index + gather (Head.cs:117-127, 175-196), one workgroup per image
__global__ void __launch_bounds__(E2E_T)
e2e_topk_kernel(const float* __restrict__ pred, int nc, int extra, int A, int k, int kp2, const float* __restrict__ amax, float* __restrict__ cand,
                int* __restrict__ stage1, e2e_u64* __restrict__ gsort, float* __restrict__ rows, long long* __restrict__ anchors) {
  __shared__ e2e_u64 s_buf[E2E_RANK_MAX];
  __shared__ e2e_u64 s_out[E2E_RANK_MAX];
  const int tid = threadIdx.x;
  const long b = blockIdx.x;
  const float* pb = pred + b * (4 + nc + extra) * (long)A;
  const int rl = 6 + extra;                       // row length: (box, score, class) + the `extra` trailing channels of the anchor
  e2e_u64* buf = k <= E2E_RANK_MAX ? s_buf : gsort + b * kp2;
  int* st1 = stage1 + b * k;
  const int N2 = k * nc;
  float* cd = cand + b * (long)N2;
  const e2e_u64* res = e2e_select_sorted(amax + b * A, A, k, buf, s_out, kp2);
  for (int r = tid; r < k; r += E2E_T) st1[r] = (int)e2e_comp_idx(res[r]);
  __syncthreads();
  // scores.gather(1, ori_index) flattened: entry j * nc + c = score of class c at the anchor of stage-1 rank j
  for (int i = tid; i < N2; i += E2E_T) {
    const int j = i / nc, c = i - j * nc;
    cd[i] = pb[(long)(4 + c) * A + st1[j]];
  }
  __syncthreads();
  res = e2e_select_sorted(cd, N2, k, buf, s_out, kp2);
  for (int r = tid; r < k; r += E2E_T) {
    const int i = (int)e2e_comp_idx(res[r]);
    const int j = i / nc, c = i - j * nc;
    const int a = st1[j];
    float* o = rows + (b * k + r) * rl;
    o[0] = pb[a]; o[1] = pb[(long)A + a]; o[2] = pb[2L * A + a]; o[3] = pb[3L * A + a];
    o[4] = cd[i]; o[5] = (float)c;
    anchors[b * k + r] = (long long)a;
  }
  if (extra > 0) {
    // Segment.postprocess (Head.cs:321-339): the nm mask coefficients gathered by the same anchor index (written above by this workgroup)
    __syncthreads();
    for (int i = tid; i < k * extra; i += E2E_T) {
      const int r = i / extra, j = i - r * extra;
      rows[(b * k + r) * rl + 6 + j] = pb[(long)(4 + nc + j) * A + (long)anchors[b * k + r]];
    }
  }
}

size_t ys_e2e_topk_ws_bytes(int B, int nc, int A, int max_det) {
  const long k = max_det < A ? max_det : A;
  long kp2 = 1; while (kp2 < k) kp2 <<= 1;
  size_t n = (size_t)B * A * 4 + (size_t)B * k * nc * 4 + (size_t)B * k * 4 + 256;      // + alignment of the sub-buffers
  if (k > E2E_RANK_MAX) n += (size_t)B * kp2 * 8;
  return n;
}

int ys_e2e_topk_launch(hipStream_t st, const float* pred, int B, int nc, int A, int max_det, void* ws, float* rows, long long* anchors, int extra) {
  if (B < 1 || nc < 1 || A < 1 || max_det < 1 || extra < 0) { ys_set_error("e2e top-k (ys_e2e_topk / ys_e2e_topk_ex): B=%d nc=%d A=%d max_det=%d extra=%d", B, nc, A, max_det, extra); return YS_ERR_INVALID_ARG; }
  const int k = max_det < A ? max_det : A;
  if ((long)k * nc >= (1L << 30) || B > 65535) { ys_set_error("e2e top-k (ys_e2e_topk / ys_e2e_topk_ex): k * nc = %ld candidates / batch %d out of range", (long)k * nc, B); return YS_ERR_UNSUPPORTED; }
  int kp2 = 1; while (kp2 < k) kp2 <<= 1;
  YsKprofScope prof(st, "e2e_topk");
  char* w = (char*)ws;
  float* amax = (float*)w; w += (size_t)B * A * 4;
  float* cand = (float*)w; w += (size_t)B * k * nc * 4;
  int* stage1 = (int*)w; w += (size_t)B * k * 4;
  w = (char*)ws + ((size_t)(w - (char*)ws) + 63) / 64 * 64;
  e2e_u64* gsort = (e2e_u64*)w;
  YS_LAUNCH(e2e_classmax_kernel, dim3(ys_cdiv(A, E2E_CM_T), B), E2E_CM_T, st, pred, nc, extra, A, amax);
  YS_LAUNCH(e2e_topk_kernel, B, E2E_T, st, pred, nc, extra, A, k, kp2, (const float*)amax, cand, stage1, gsort, rows, anchors);
  return YS_OK;
}

// ------------------------------------------------------------------ non_max_suppression(end2end: true) (Ops.cs:258-267)
// rows [B][k][row_len] (6, or 6 + nm for Segment rows) ordered by score: count[b] = the leading rows with score > conf_thres, at most max_det
__global__ void __launch_bounds__(256)
e2e_select_kernel(const float* __restrict__ rows, int k, int row_len, float conf, int max_det, int* __restrict__ count) {
  __shared__ int s_first;
  const long b = blockIdx.x;
  if (threadIdx.x == 0) s_first = k;
  __syncthreads();
  int first = k;                                  // first row that fails the test
  for (int r = threadIdx.x; r < k; r += 256)
    if (!(rows[(b * k + r) * row_len + 4] > conf)) { first = r; break; }
  if (first < k) atomicMin(&s_first, first);
  __syncthreads();
  if (threadIdx.x == 0) count[b] = s_first < max_det ? s_first : max_det;
}

int ys_e2e_select_launch(hipStream_t st, const float* rows, int B, int k, float conf, int max_det, int* count, int row_len) {
  if (B < 1 || k < 1 || max_det < 1 || row_len < 6) { ys_set_error("e2e select (ys_e2e_select / ys_e2e_select_ex): B=%d k=%d max_det=%d row length %d", B, k, max_det, row_len); return YS_ERR_INVALID_ARG; }
  YS_LAUNCH(e2e_select_kernel, B, 256, st, rows, k, row_len, conf, max_det, count);
  return YS_OK;
}

// ------------------------------------------------------------------ second running-statistics update of the aliased towers
// The one2one branch sees the same input values, weights and batch statistics s as the one2many branch (Head.cs:94-96), so each BatchNorm
// of the towers updates r1 = (1 - m) r0 + m s and then r2 = (1 - m) r1 + m s.  With r0 saved before the forward, m s = r1 - (1 - m) r0
// and r2 = r1 + (1 - m) (r1 - r0): no second pass over the activations.  st [n] = running_mean | running_var | num_batches_tracked
// regions of the tower units, snap = its copy from before the forward; is_count[i] != 0 marks a num_batches_tracked word (+ 1).
__global__ void __launch_bounds__(256)
e2e_bn_second_update_kernel(float* __restrict__ st, const float* __restrict__ snap, const unsigned char* __restrict__ is_count, long n, float momentum) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float r1 = st[i], r0 = snap[i];
  st[i] = is_count[i] ? r1 + (r1 - r0) : r1 + (1.0f - momentum) * (r1 - r0);
}

int ys_e2e_bn_second_update_launch(hipStream_t st, float* state, const float* snap, const unsigned char* is_count, long n, float momentum) {
  if (n > 0) YS_LAUNCH(e2e_bn_second_update_kernel, ys_cdiv(n, 256), 256, st, state, snap, is_count, n, momentum);
  return YS_OK;
}

// ---- C ABI: Detect.postprocess / get_topk_index (Modules/Head.cs:117-127, 175-196) on a [B, 4+nc, A] tensor and the thresholding of
//      Ops.non_max_suppression(end2end: true) (Utils/Ops.cs:258-267)
static int e2e_topk_impl(const char* fn, ys_ctx* ctx, const float* pred, int on_device, int batch, int nc, int extra, int anchors, int max_det, float* out_rows,
                         int64_t* out_anchor) {
  YS_REQUIRE(ctx && pred && out_rows && out_anchor, "%s: null argument", fn);
  YS_REQUIRE(batch > 0 && nc > 0 && extra >= 0 && anchors > 0 && max_det > 0, "%s: bad shape B=%d nc=%d extra=%d A=%d max_det=%d", fn, batch, nc, extra, anchors, max_det);
  YS_CHECK_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const size_t k = (size_t)(max_det < anchors ? max_det : anchors);
  const size_t n_pred = (size_t)batch * (4 + nc + extra) * anchors, n_rows = (size_t)batch * k * (6 + extra), n_anc = (size_t)batch * k;
  DevBuf dp, dr, da;
  YS_TRY(ys_ctx_reserve_ws(ctx, &ctx->e2e_ws, &ctx->e2e_ws_bytes, ys_e2e_topk_ws_bytes(batch, nc, anchors, max_det), fn));
  YsTimer timer(ctx, "e2e_topk");
  if (on_device) return ys_e2e_topk_launch(st, pred, batch, nc, anchors, max_det, ctx->e2e_ws, out_rows, (long long*)out_anchor, extra);
  YS_TRY(dp.alloc(n_pred * 4)); YS_TRY(dr.alloc(n_rows * 4)); YS_TRY(da.alloc(n_anc * 8));
  YS_TRY(h2d(st, dp.p, pred, n_pred * 4));
  YS_TRY(ys_e2e_topk_launch(st, (const float*)dp.p, batch, nc, anchors, max_det, ctx->e2e_ws, (float*)dr.p, (long long*)da.p, extra));
  YS_TRY(d2h(st, out_rows, dr.p, n_rows * 4));
  YS_TRY(d2h(st, out_anchor, da.p, n_anc * 8));
  YS_CHECK_HIP(hipStreamSynchronize(st));
  return YS_OK;
}

extern "C" int ys_e2e_topk(ys_ctx* ctx, const float* pred, int on_device, int batch, int nc, int anchors, int max_det, float* out_rows,
                           int64_t* out_anchor) {
  return e2e_topk_impl("ys_e2e_topk", ctx, pred, on_device, batch, nc, 0, anchors, max_det, out_rows, out_anchor);
}

extern "C" int ys_e2e_topk_ex(ys_ctx* ctx, const float* pred, int on_device, int batch, int nc, int extra, int anchors, int max_det, float* out_rows,
                              int64_t* out_anchor) {
  return e2e_topk_impl("ys_e2e_topk_ex", ctx, pred, on_device, batch, nc, extra, anchors, max_det, out_rows, out_anchor);
}

static int e2e_select_impl(const char* fn, ys_ctx* ctx, const float* rows, int on_device, int batch, int k, int row_len, float conf_thres, int max_det, int32_t* out_count) {
  YS_REQUIRE(ctx && rows && out_count, "%s: null argument", fn);
  // Ops.cs:248-251: ArgumentException for a threshold outside [0,1]
  YS_REQUIRE(conf_thres >= 0.f && conf_thres <= 1.f, "Invalid Confidence threshold %g, valid values are between 0.0 and 1.0", conf_thres);
  YS_REQUIRE(batch > 0 && k > 0 && max_det > 0 && row_len >= 6, "%s: bad shape B=%d k=%d max_det=%d row length %d", fn, batch, k, max_det, row_len);
  YS_CHECK_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  if (on_device) return ys_e2e_select_launch(st, rows, batch, k, conf_thres, max_det, out_count, row_len);
  DevBuf dr, dc;
  const size_t nb = (size_t)batch * k * row_len * 4;
  YS_TRY(dr.alloc(nb)); YS_TRY(dc.alloc((size_t)batch * 4));
  YS_TRY(h2d(st, dr.p, rows, nb));
  YS_TRY(ys_e2e_select_launch(st, (const float*)dr.p, batch, k, conf_thres, max_det, (int*)dc.p, row_len));
  YS_TRY(d2h(st, out_count, dc.p, (size_t)batch * 4));
  YS_CHECK_HIP(hipStreamSynchronize(st));
  return YS_OK;
}

extern "C" int ys_e2e_select(ys_ctx* ctx, const float* rows, int on_device, int batch, int k, float conf_thres, int max_det, int32_t* out_count) {
  return e2e_select_impl("ys_e2e_select", ctx, rows, on_device, batch, k, 6, conf_thres, max_det, out_count);
}

extern "C" int ys_e2e_select_ex(ys_ctx* ctx, const float* rows, int on_device, int batch, int k, int row_len, float conf_thres, int max_det, int32_t* out_count) {
  return e2e_select_impl("ys_e2e_select_ex", ctx, rows, on_device, batch, k, row_len, conf_thres, max_det, out_count);
}
