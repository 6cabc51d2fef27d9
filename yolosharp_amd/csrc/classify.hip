// classify.hip -- the Classify head's own device code (Modules/Head.cs:612-644, Utils/Loss.cs:1073-1091, Models/Classifier.cs:61-120).
//
//   pool forward   pooled[b][c] = mean_p act(y[b][p][c] * scale[c] + shift[c])    BN apply + SiLU + AdaptiveAvgPool2d(1) in ONE pass over
//                  the pre-BN output of the 1280-channel Conv (training: the activated map is never written); eval reads the map the
//                  convolution's folded-BN epilogue wrote and only averages it
//   pool backward  fused into that Conv unit's BN / SiLU backward: dz[b][p][c] = dpooled[b][c] / HW is never written -- the BN-backward
//                  reduction and apply passes take it from dpooled and produce the convolution's dy (run_conv_bwd, Conv unit pool_next)
//   cross entropy  one wave per row: max-subtracted log-sum-exp in fp32, loss_b = lse - x[label]; dlogits = (softmax - onehot) / B;
//                  the batch mean is a fixed-order reduction of the per-row losses (no float atomics: runs stay bit-reproducible).
//                  Without labels the same kernel writes the eval softmax.
//   top-k          one wave per row, k <= 16 passes of a wave arg-max over the entries below the previous pick in the order
//                  (score descending, index ascending): the reference's argsort(descending) with ties to the lower index.
// Every lane of a wave runs the same trip counts around the wave reductions (the interpreter build needs full waves there).
#include "ops_stage.h"
#include "bn_math.h"

#define CLS_THREADS 256
#define CLS_TOPK_MAX 16

// ---- pool forward: one thread per (image, EPL channels); 16-byte loads along the channels, pixels in order (fixed summation order)
template <class T, bool APPLY>
__global__ void __launch_bounds__(CLS_THREADS)
cls_pool_fwd_kernel(const T* __restrict__ x, int ldc, int coff, long bstride, int HW, int C, const float* __restrict__ scale,
                    const float* __restrict__ shift, int act, T* __restrict__ out, int ldo, int B) {
  constexpr int EPL = Elem<T>::EPL;
  const int vpr = C / EPL;
  const long t = (long)blockIdx.x * CLS_THREADS + threadIdx.x;
  if (t >= (long)B * vpr) return;
  const int b = (int)(t / vpr), c0 = (int)(t - (long)b * vpr) * EPL;
  float sc[EPL], sh[EPL], acc[EPL];
  for (int j = 0; j < EPL; j++) { acc[j] = 0.f; sc[j] = APPLY ? scale[c0 + j] : 1.f; sh[j] = APPLY ? shift[c0 + j] : 0.f; }
  const T* p = x + (long)b * bstride * ldc + coff + c0;
#pragma unroll 4
  for (int i = 0; i < HW; i++) {
    float f[EPL];
    ys_unpack<T>(*(const uint4*)(p + (long)i * ldc), f);
    for (int j = 0; j < EPL; j++) {
      acc[j] += APPLY ? bn_act1(f[j], sc[j], sh[j], act != 0) : f[j];
    }
  }
  const float inv = 1.0f / (float)HW;
  float o[EPL];
  for (int j = 0; j < EPL; j++) o[j] = acc[j] * inv;
  *(uint4*)(out + (long)b * ldo + c0) = ys_pack<T>(o);
}

int ys_cls_pool_fwd_launch(hipStream_t st, int dtype, const void* x, int ldc, int coff, long bstride, int B, int HW, int C,
                           const float* scale, const float* shift, int act, void* out, int ldo) {
  const int epl = dtype == YS_BF16 ? 8 : 4;
  if (C % epl || ldc % epl || coff % epl || ldo % epl) { ys_set_error("cls pool: C=%d ldc=%d coff=%d ldo=%d not multiples of %d", C, ldc, coff, ldo, epl); return YS_ERR_UNSUPPORTED; }
  YsKprofScope prof(st, "cls_pool");
  const long n = (long)B * (C / epl);
  const int grid = (int)((n + CLS_THREADS - 1) / CLS_THREADS);
  const bool apply = scale != nullptr;
  if (dtype == YS_BF16) {
    if (apply) YS_LAUNCH((cls_pool_fwd_kernel<bf16_t, true>), grid, CLS_THREADS, st, (const bf16_t*)x, ldc, coff, bstride, HW, C, scale, shift, act, (bf16_t*)out, ldo, B);
    else YS_LAUNCH((cls_pool_fwd_kernel<bf16_t, false>), grid, CLS_THREADS, st, (const bf16_t*)x, ldc, coff, bstride, HW, C, scale, shift, act, (bf16_t*)out, ldo, B);
  } else {
    if (apply) YS_LAUNCH((cls_pool_fwd_kernel<float, true>), grid, CLS_THREADS, st, (const float*)x, ldc, coff, bstride, HW, C, scale, shift, act, (float*)out, ldo, B);
    else YS_LAUNCH((cls_pool_fwd_kernel<float, false>), grid, CLS_THREADS, st, (const float*)x, ldc, coff, bstride, HW, C, scale, shift, act, (float*)out, ldo, B);
  }
  return YS_OK;
}

// ---- pool backward fused into the Conv unit's BN / SiLU backward.  dz[b][p][c] = dpooled[b][c] / HW is the same at every pixel of an
// image, so it is never written: the reduction pass takes it from dpooled (one thread per (image, EPL channels), pixels in order -> the
// partial rows [B][2][C] bn_bwd_finalize reads, nblk = B), and the apply pass writes the convolution's dy from it.  The arithmetic of
// chan_reduce_kernel / bn_bwd_apply_kernel (batchnorm.hip; bn_math.h) with dz = dpooled / HW kept in fp32.
template <class T, bool ACT>
__global__ void __launch_bounds__(CLS_THREADS)
cls_bn_bwd_reduce_kernel(const T* __restrict__ dp, int ldp, const T* __restrict__ y, int B, int HW, int C, const float* __restrict__ scale,
                         const float* __restrict__ shift, float* __restrict__ partial) {
  constexpr int EPL = Elem<T>::EPL;
  const int vpr = C / EPL;
  const long t = (long)blockIdx.x * CLS_THREADS + threadIdx.x;
  if (t >= (long)B * vpr) return;
  const int b = (int)(t / vpr), c = (int)(t - (long)b * vpr) * EPL;
  float g[EPL], sc[EPL], sh[EPL], a1[EPL], a2[EPL];
  ys_unpack<T>(*(const uint4*)(dp + (long)b * ldp + c), g);
  const float inv = 1.0f / (float)HW;
  for (int e = 0; e < EPL; e++) { g[e] *= inv; sc[e] = scale[c + e]; sh[e] = shift[c + e]; a1[e] = 0.f; a2[e] = 0.f; }
  const T* yp = y + (long)b * HW * C + c;
#pragma unroll 4
  for (int i = 0; i < HW; i++) {
    float f[EPL];
    ys_unpack<T>(*(const uint4*)(yp + (long)i * C), f);
    for (int e = 0; e < EPL; e++) {
      const float du = bn_du1(g[e], f[e], sc[e], sh[e], ACT);
      a1[e] += du;
      a2[e] += du * f[e];
    }
  }
  for (int e = 0; e < EPL; e++) { partial[((long)b * 2 + 0) * C + c + e] = a1[e]; partial[((long)b * 2 + 1) * C + c + e] = a2[e]; }
}

template <class T, bool ACT>
__global__ void __launch_bounds__(CLS_THREADS)
cls_bn_bwd_apply_kernel(const T* __restrict__ dp, int ldp, const T* __restrict__ y, long rows, int HW, int C, const float* __restrict__ scale,
                        const float* __restrict__ shift, const float* __restrict__ k2, const float* __restrict__ k3, T* __restrict__ dy) {
  constexpr int EPL = Elem<T>::EPL;
  const int vpr = C / EPL;
  const long t = (long)blockIdx.x * CLS_THREADS + threadIdx.x;
  if (t >= rows * vpr) return;
  const long row = t / vpr;
  const int c = (int)(t - row * vpr) * EPL;
  const long b = row / HW;
  float g[EPL], f[EPL];
  ys_unpack<T>(*(const uint4*)(dp + b * ldp + c), g);
  ys_unpack<T>(*(const uint4*)(y + row * C + c), f);
  const float inv = 1.0f / (float)HW;
  for (int e = 0; e < EPL; e++) {
    const float sc = scale[c + e];
    f[e] = bn_dy1(bn_du1(g[e] * inv, f[e], sc, shift[c + e], ACT), f[e], sc, k2[c + e], k3[c + e]);
  }
  *(uint4*)(dy + row * C + c) = ys_pack<T>(f);
}

int ys_cls_bn_bwd_reduce_launch(hipStream_t st, int dtype, const void* dpooled, int ldp, const void* y, int B, int HW, int C, const float* scale,
                                const float* shift, int act, float* partial) {
  const int epl = dtype == YS_BF16 ? 8 : 4;
  if (C % epl || ldp % epl) { ys_set_error("cls BN backward: C=%d ldp=%d not multiples of %d", C, ldp, epl); return YS_ERR_UNSUPPORTED; }
  YsKprofScope prof(st, "cls_pool_bwd");
  const long n = (long)B * (C / epl);
  const int grid = (int)((n + CLS_THREADS - 1) / CLS_THREADS);
  YS_DISPATCH_T_ACT(dtype, act, YS_LAUNCH((cls_bn_bwd_reduce_kernel<TT, AF>), grid, CLS_THREADS, st, (const TT*)dpooled, ldp, (const TT*)y, B, HW, C, scale, shift, partial));
  return YS_OK;
}

int ys_cls_bn_bwd_apply_launch(hipStream_t st, int dtype, const void* dpooled, int ldp, const void* y, int B, int HW, int C, const float* scale,
                               const float* shift, const float* k2, const float* k3, int act, void* dy) {
  const int epl = dtype == YS_BF16 ? 8 : 4;
  if (C % epl || ldp % epl) { ys_set_error("cls BN backward: C=%d ldp=%d not multiples of %d", C, ldp, epl); return YS_ERR_UNSUPPORTED; }
  YsKprofScope prof(st, "cls_pool_bwd");
  const long rows = (long)B * HW;
  const long n = rows * (C / epl);
  const int grid = (int)((n + CLS_THREADS - 1) / CLS_THREADS);
  YS_DISPATCH_T_ACT(dtype, act, YS_LAUNCH((cls_bn_bwd_apply_kernel<TT, AF>), grid, CLS_THREADS, st, (const TT*)dpooled, ldp, (const TT*)y, rows, HW, C, scale, shift, k2, k3, (TT*)dy));
  return YS_OK;
}

// ---- softmax / cross entropy: one wave per row (4 rows per workgroup)
template <class T>
__global__ void __launch_bounds__(CLS_THREADS)
cls_xent_kernel(const T* __restrict__ logits, int ld, int B, int nc, const float* __restrict__ labels, T* __restrict__ dlogits,
                float* __restrict__ probs, float* __restrict__ row_loss) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * (CLS_THREADS / 64) + (threadIdx.x >> 6);
  if (b >= B) return;                                            // whole waves leave together
  const T* x = logits + (long)b * ld;
  float mx = -INFINITY;
  for (int j = lane; j < nc; j += 64) mx = fmaxf(mx, Elem<T>::to_f(x[j]));
  mx = ys_wave_max(mx);
  float s = 0.f;
  for (int j = lane; j < nc; j += 64) s += expf(Elem<T>::to_f(x[j]) - mx);
  s = ys_wave_sum(s);
  const float inv = 1.0f / s;
  if (probs)
    for (int j = lane; j < nc; j += 64) probs[(long)b * nc + j] = expf(Elem<T>::to_f(x[j]) - mx) * inv;
  if (!labels) return;
  const float lf = labels[b];
  const bool ok = lf >= 0.f && lf < (float)nc && lf == floorf(lf);
  const int lab = ok ? (int)lf : -1;
  if (lane == 0) {
    row_loss[b] = ok ? (logf(s) + mx) - Elem<T>::to_f(x[lab]) : 0.f;   // lse - x[label]
    row_loss[B + b] = ok ? 0.f : 1.f;                                   // invalid-label flag (read back by ys_loss_read_items)
  }
  const float rb = 1.0f / (float)B;
  T* d = dlogits + (long)b * ld;
  for (int j = lane; j < ld; j += 64) {
    float g = 0.f;
    if (j < nc) g = (expf(Elem<T>::to_f(x[j]) - mx) * inv - (j == lab ? 1.f : 0.f)) * rb;
    d[j] = Elem<T>::from_f(g);                                      // pad channels: 0
  }
}

// mean over the batch in one workgroup: fixed strided order per thread, fixed tree, double accumulation
__global__ void __launch_bounds__(CLS_THREADS)
cls_xent_finalize_kernel(const float* __restrict__ row_loss, int B, float* __restrict__ scalars) {
  __shared__ double s_l[CLS_THREADS], s_f[CLS_THREADS];
  const int tid = threadIdx.x;
  double l = 0.0, f = 0.0;
  for (int i = tid; i < B; i += CLS_THREADS) { l += (double)row_loss[i]; f += (double)row_loss[B + i]; }
  s_l[tid] = l; s_f[tid] = f;
  __syncthreads();
  for (int st = CLS_THREADS / 2; st > 0; st >>= 1) {
    if (tid < st) { s_l[tid] += s_l[tid + st]; s_f[tid] += s_f[tid + st]; }
    __syncthreads();
  }
  if (tid == 0) {
    const float mean = (float)(s_l[0] / (double)B);
    scalars[1] = mean;                 // the criterion's one item (Loss.cs:1086)
    scalars[4] = mean;                 // the scalar backward() differentiates: the mean itself (not * B, unlike the detection losses)
    scalars[14] = (float)s_f[0];       // rows whose label lies outside [0, nc)
    scalars[15] = 0.f;                 // (label-capacity word of the detection losses: unused)
  }
}

int ys_cls_xent_launch(hipStream_t st, int dtype, const void* logits, int ld, int B, int nc, const float* labels, void* dlogits,
                       float* probs, float* row_loss, float* scalars) {
  if (nc < 1 || ld < nc || B < 1) { ys_set_error("cls cross entropy: B=%d nc=%d ld=%d", B, nc, ld); return YS_ERR_INVALID_ARG; }
  YsKprofScope prof(st, labels ? "cls_xent" : "cls_softmax");
  const int grid = (B + CLS_THREADS / 64 - 1) / (CLS_THREADS / 64);
  if (dtype == YS_BF16) YS_LAUNCH(cls_xent_kernel<bf16_t>, grid, CLS_THREADS, st, (const bf16_t*)logits, ld, B, nc, labels, (bf16_t*)dlogits, probs, row_loss);
  else YS_LAUNCH(cls_xent_kernel<float>, grid, CLS_THREADS, st, (const float*)logits, ld, B, nc, labels, (float*)dlogits, probs, row_loss);
  if (labels) YS_LAUNCH(cls_xent_finalize_kernel, 1, CLS_THREADS, st, row_loss, B, scalars);
  return YS_OK;
}

// ---- top-k: one wave per row
__global__ void __launch_bounds__(CLS_THREADS)
cls_topk_kernel(const float* __restrict__ x, int rows, int cols, int k, int32_t* __restrict__ idx) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * (CLS_THREADS / 64) + (threadIdx.x >> 6);
  if (r >= rows) return;
  const float* p = x + (long)r * cols;
  float lv = INFINITY; int li = -1;                              // last pick: entries after it in (score desc, index asc) order remain
  for (int q = 0; q < k; q++) {
    float bv = -INFINITY; int bi = 0x7fffffff;
    for (int j = lane; j < cols; j += 64) {
      const float v = p[j];
      const bool below = v < lv || (v == lv && j > li);
      if (below && (v > bv || (v == bv && j < bi))) { bv = v; bi = j; }
    }
    for (int m = 32; m >= 1; m >>= 1) {
      const float ov = __shfl_xor(bv, m);
      const int oi = __shfl_xor(bi, m);
      if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
    }
    if (lane == 0) idx[(long)r * k + q] = bi == 0x7fffffff ? -1 : bi;   // -1: fewer than k comparable (non-NaN) entries
    lv = bv; li = bi;
  }
}

int ys_cls_topk_launch(hipStream_t st, const float* x, int rows, int cols, int k, int32_t* idx) {
  if (rows < 0 || cols < 1 || k < 1 || k > CLS_TOPK_MAX || k > cols) { ys_set_error("ys_cls_topk: rows=%d cols=%d k=%d (1 <= k <= min(16, cols))", rows, cols, k); return YS_ERR_INVALID_ARG; }
  if (rows == 0) return YS_OK;
  YsKprofScope prof(st, "cls_topk");
  const int grid = (rows + CLS_THREADS / 64 - 1) / (CLS_THREADS / 64);
  YS_LAUNCH(cls_topk_kernel, grid, CLS_THREADS, st, x, rows, cols, k, idx);
  return YS_OK;
}

// ---- C ABI: ys_cls_topk (Classifier.Val's argsort, Models/Classifier.cs:95-100)
extern "C" int ys_cls_topk(ys_ctx* ctx, const float* scores, int on_device, int rows, int cols, int k, int32_t* idx) {
  YS_REQUIRE(ctx && scores && idx, "ys_cls_topk: null argument");
  YS_REQUIRE(rows >= 0 && cols >= 1 && k >= 1 && k <= CLS_TOPK_MAX && k <= cols, "ys_cls_topk: rows=%d cols=%d k=%d (1 <= k <= min(16, cols))", rows, cols, k);
  if (rows == 0) return YS_OK;
  YS_CHECK_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  if (on_device) return ys_cls_topk_launch(st, scores, rows, cols, k, idx);
  DevBuf ds, di;
  YS_TRY(ds.alloc((size_t)rows * cols * 4));
  YS_TRY(di.alloc((size_t)rows * k * 4));
  YS_TRY(h2d(st, ds.p, scores, (size_t)rows * cols * 4));
  YS_TRY(ys_cls_topk_launch(st, (const float*)ds.p, rows, cols, k, (int32_t*)di.p));
  YS_TRY(d2h(st, idx, di.p, (size_t)rows * k * 4));
  YS_CHECK_HIP(hipStreamSynchronize(st));
  return YS_OK;
}
