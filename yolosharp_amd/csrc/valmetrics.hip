// valmetrics.hip -- the per-image part of Detector.Val (Models/Detector.cs:103-120) on the device:
//   GT boxes = bboxes[batch_idx == b] * (W, H, W, H) -> xyxy          (Ops.xywh2xyxy, Utils/Ops.cs:68-81)
//   iou      = Metrics.box_iou(gt, pred[:, 0:4])                       (Utils/Metrics.cs:16-34, eps 1e-7)
//   correct  = match_predictions(pred[:, 5], cls, iou)                 (Models/YoloBaseTaskModel.cs:377-446)
// The reference walks images on the host and de-duplicates matches with per-element .item() loops
// (GetUniqueByColumn, :422-444); here one workgroup owns an image and nothing leaves the device.
//
// match_predictions, restated.  For a threshold t the reference takes all (label, detection) pairs with
// iou * (class match) >= t, orders them by IoU descending, keeps the FIRST pair of every detection (result ordered by
// detection index, since torch.unique sorts), then the first pair of every label in THAT order.  Hence:
//   best(d)  = the class-matching label with the largest IoU for detection d (independent of t),
//   label l is credited to the smallest d with best(d) == l and iou(best(d), d) >= t,   correct[d][t] = 1 for those d.
// Equal IoUs are ordered by the sort implementation upstream (unpinned); here the lower label index wins.
// The three stages -- gather the image's labels, best label per detection, credit per (label, threshold) -- are stated once (vm_gather_labels, VmBest,
// vm_credit) and called by the four matching kernels, which differ in the metric only: box IoU (val_match_kernel), probiou (val_match_rot_kernel), box IoU
// and OKS (val_match_pose_kernel), a supplied matrix (match_iou_kernel).
// Compiled with -ffp-contract=off: the IoU arithmetic is the reference's operation order in plain fp32.
#include "ops_stage.h"
#include "probiou.h"

#define VM_THREADS 256
#define VM_NT 10          // IoU thresholds linspace(0.5, 0.95, 10)

struct VmThr { float t[VM_NT]; };

__device__ inline float vm_iou(float a1x, float a1y, float a2x, float a2y, float b1x, float b1y, float b2x, float b2y, float eps) {
  // inter = (min(a2, b2) - max(a1, b1)).clamp(0).prod ; iou = inter / (area1 + area2 - inter + eps)
  float iw = fminf(a2x, b2x) - fmaxf(a1x, b1x);
  float ih = fminf(a2y, b2y) - fmaxf(a1y, b1y);
  iw = iw < 0.f ? 0.f : iw;
  ih = ih < 0.f ? 0.f : ih;
  const float inter = iw * ih;
  const float area1 = (a2x - a1x) * (a2y - a1y), area2 = (b2x - b1x) * (b2y - b1y);
  return inter / (area1 + area2 - inter + eps);
}

__global__ void __launch_bounds__(VM_THREADS)
box_iou_kernel(const float* __restrict__ b1, int n, const float* __restrict__ b2, int m, float eps, float* __restrict__ out) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)n * m) return;
  const int r = (int)(i / m), c = (int)(i - (long)r * m);
  out[i] = vm_iou(b1[4 * r], b1[4 * r + 1], b1[4 * r + 2], b1[4 * r + 3], b2[4 * c], b2[4 * c + 1], b2[4 * c + 2], b2[4 * c + 3], eps);
}

// Metrics.kpt_iou (Metrics.cs:186-212): OKS of ground-truth keypoints kpt1 [n][K][3] (x, y, visibility) against predictions
// kpt2 [m][K][D]; area [n]; sigma = OKS sigmas when K == 17, else 1/K.  One thread per (gt, prediction) pair.
struct KptSigma { float s[64]; };
// one (gt, prediction) pair: g [K][3], p [K][D], area of the gt.  Shared by kpt_iou_kernel and val_match_pose_kernel, so both evaluate the same operations.
__device__ inline float vm_oks(const float* __restrict__ g, const float* __restrict__ p, float area, int K, int D, const KptSigma& sg, float eps) {
  const float ar = area + eps;
  float acc = 0.f, cnt = 0.f;
  for (int k = 0; k < K; k++) {
    const float dx = g[3 * k] - p[D * k], dy = g[3 * k + 1] - p[D * k + 1];
    const float s2 = 2.0f * sg.s[k];
    const float e = (dx * dx + dy * dy) / (s2 * s2 * ar * 2.0f);
    const float mk = g[3 * k + 2] != 0.f ? 1.f : 0.f;
    acc += expf(-e) * mk;
    cnt += mk;
  }
  return acc / (cnt + eps);
}
__global__ void __launch_bounds__(VM_THREADS)
kpt_iou_kernel(const float* __restrict__ k1, int n, const float* __restrict__ k2, int m, const float* __restrict__ area, int K, int D,
               KptSigma sg, float eps, float* __restrict__ out) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)n * m) return;
  const int r = (int)(i / m), c = (int)(i - (long)r * m);
  out[i] = vm_oks(k1 + (long)r * K * 3, k2 + (long)c * K * D, area[r], K, D, sg, eps);
}

// ---- match_predictions' shared stages.  ws_lab [B][n_labels] (an image can hold all labels of the batch), ws_best [B][max_det][2 per metric],
// correct [B][max_det][10].
__device__ inline int vm_count(int count, int max_det) { return count < max_det ? (count > 0 ? count : 0) : max_det; }
__device__ inline void vm_clear(unsigned char* __restrict__ cor, int n) {
  for (int i = threadIdx.x; i < n; i += VM_THREADS) cor[i] = 0;
}
// stage 1: the labels of image b in collate order (boolean-mask indexing keeps the order, Detector.cs:110-112); *s_nl = their number, valid after the
// caller's barrier
__device__ inline void vm_gather_labels(const float* __restrict__ batch_idx, int n_labels, int b, int* __restrict__ lab, int* s_nl) {
  if (threadIdx.x != 0) return;
  int k = 0;
  for (int j = 0; j < n_labels; j++)
    if ((int)batch_idx[j] == b) lab[k++] = j;
  *s_nl = k;
}
// stage 2: the class-matching label with the largest metric; the lower label index wins among equals
struct VmBest {
  float v = -1.f; int k = -1;
  __device__ void offer(float metric, int label) { if (metric > v) { v = metric; k = label; } }
  __device__ void store(float* __restrict__ best) const { best[0] = v; best[1] = (float)k; }
};
// stage 3: every (metric, label, threshold): the first detection that chose this label and clears the threshold.  A `best` row holds NM (value, label) pairs
template <int NM>
__device__ inline void vm_credit(const float* __restrict__ best, int L, int D, const VmThr& thr, unsigned char* __restrict__ cor0, unsigned char* __restrict__ cor1) {
  for (int e = threadIdx.x; e < NM * L * VM_NT; e += VM_THREADS) {
    const int mt = NM > 1 ? e / (L * VM_NT) : 0, r = e - mt * L * VM_NT;
    const int k = r / VM_NT, ti = r - k * VM_NT;
    const float t = thr.t[ti];
    unsigned char* cor = mt ? cor1 : cor0;
    for (int d = 0; d < D; d++)
      if ((int)best[2 * (NM * d + mt) + 1] == k && best[2 * (NM * d + mt)] >= t) { cor[d * VM_NT + ti] = 1; break; }
  }
}

// The per-image part of Detector.Val for a whole batch: one workgroup per image
__global__ void __launch_bounds__(VM_THREADS)
val_match_kernel(const float* __restrict__ rows, const int* __restrict__ count, int max_det, int row_stride,
                 const float* __restrict__ batch_idx, const float* __restrict__ cls, const float* __restrict__ bboxes, int n_labels,
                 float img_w, float img_h, VmThr thr, int* __restrict__ ws_lab, float* __restrict__ ws_best, unsigned char* __restrict__ correct) {
  __shared__ int s_nl;
  const int b = blockIdx.x, tid = threadIdx.x;
  int* lab = ws_lab + (long)b * n_labels;
  float* best = ws_best + (long)b * max_det * 2;
  unsigned char* cor = correct + (long)b * max_det * VM_NT;
  const int D = vm_count(count[b], max_det);
  vm_clear(cor, max_det * VM_NT);
  vm_gather_labels(batch_idx, n_labels, b, lab, &s_nl);
  __syncthreads();
  const int L = s_nl;
  for (int d = tid; d < D; d += VM_THREADS) {
    const float* pr = rows + ((long)b * max_det + d) * row_stride;
    const float px1 = pr[0], py1 = pr[1], px2 = pr[2], py2 = pr[3], pc = pr[5];
    VmBest bi;
    for (int k = 0; k < L; k++) {
      const int j = lab[k];
      if (cls[j] != pc) continue;
      const float cx = bboxes[4 * j] * img_w, cy = bboxes[4 * j + 1] * img_h, w = bboxes[4 * j + 2] * img_w, h = bboxes[4 * j + 3] * img_h;
      bi.offer(vm_iou(cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2, px1, py1, px2, py2, 1e-7f), k);
    }
    bi.store(best + 2 * d);
  }
  __syncthreads();
  vm_credit<1>(best, L, D, thr, cor, nullptr);
}

// The per-image part of Obber.Val (Models/Obber.cs:102-114) for a whole batch: val_match_kernel with Metrics.batch_probiou in place of box_iou.  GT =
// bboxes[batch_idx == b] as (cx W, cy H, w W, h H, angle) in collate order, prediction d = rows[b][d] columns 0..3 + column angle_col; obb1 = GT, obb2 =
// prediction (Obber.cs:112).  nms_obb_cov / nms_probiou are probiou_kernel's (probiou.h), so `correct` equals ys_batch_probiou + ys_match_predictions per
// image bit for bit.  Each label's covariance terms are computed once into ws_gt [n_labels][5], indexed by the LABEL (a pure function of the label, and a
// label belongs to one image: no two workgroups write one word).
__global__ void __launch_bounds__(VM_THREADS)
val_match_rot_kernel(const float* __restrict__ rows, const int* __restrict__ count, int max_det, int row_stride, int angle_col,
                     const float* __restrict__ batch_idx, const float* __restrict__ cls, const float* __restrict__ bboxes, int n_labels,
                     float img_w, float img_h, VmThr thr, int* __restrict__ ws_lab, float* __restrict__ ws_gt, float* __restrict__ ws_best,
                     unsigned char* __restrict__ correct) {
  __shared__ int s_nl;
  const int b = blockIdx.x, tid = threadIdx.x;
  int* lab = ws_lab + (long)b * n_labels;
  float* best = ws_best + (long)b * max_det * 2;
  unsigned char* cor = correct + (long)b * max_det * VM_NT;
  const int D = vm_count(count[b], max_det);
  vm_clear(cor, max_det * VM_NT);
  vm_gather_labels(batch_idx, n_labels, b, lab, &s_nl);
  __syncthreads();
  const int L = s_nl;
  for (int k = tid; k < L; k += VM_THREADS) {
    const int j = lab[k];
    const float g[5] = {bboxes[5 * j] * img_w, bboxes[5 * j + 1] * img_h, bboxes[5 * j + 2] * img_w, bboxes[5 * j + 3] * img_h, bboxes[5 * j + 4]};
    float a, bq, c;
    nms_obb_cov(g, a, bq, c);
    float* gt = ws_gt + 5L * j;
    gt[0] = g[0]; gt[1] = g[1]; gt[2] = a; gt[3] = bq; gt[4] = c;
  }
  __syncthreads();
  for (int d = tid; d < D; d += VM_THREADS) {
    const float* pr = rows + ((long)b * max_det + d) * row_stride;
    const float p[5] = {pr[0], pr[1], pr[2], pr[3], pr[angle_col]};
    const float pc = pr[5];
    float a2, b2, c2;
    nms_obb_cov(p, a2, b2, c2);
    VmBest bi;
    for (int k = 0; k < L; k++) {
      const long j = lab[k];
      if (cls[j] != pc) continue;
      const float* g = ws_gt + 5 * j;
      bi.offer(nms_probiou(g[0], g[1], g[2], g[3], g[4], p[0], p[1], a2, b2, c2, 1e-7f), k);
    }
    bi.store(best + 2 * d);
  }
  __syncthreads();
  vm_credit<1>(best, L, D, thr, cor, nullptr);
}

// The per-image part of PoseDetector.Val (Models/PoseDetector.cs:131-165) for a whole batch: val_match_kernel with two metrics.  Computed once per label,
// what :140-156 compute per image: the xyxy box of bboxes * (W, H, W, H), area = (x2 - x1) * (y2 - y1) * 0.53f and the keypoints * (W, H, 1) with the
// "seen" column of ones for 2-column labels, in workspaces indexed by the label like ws_gt above (ws_gt [n_labels][5], ws_kp [n_labels][K][3]).
// Per detection: the best class-matching label by vm_iou and the best by vm_oks, in a ws_best row of four.  Same operations as ys_box_iou / ys_kpt_iou +
// ys_match_predictions per image, so both outputs equal that path bit for bit.
__global__ void __launch_bounds__(VM_THREADS)
val_match_pose_kernel(const float* __restrict__ rows, const int* __restrict__ count, int max_det, int row_stride, int kpt_col, int K, int D,
                      const float* __restrict__ batch_idx, const float* __restrict__ cls, const float* __restrict__ bboxes,
                      const float* __restrict__ keypoints /*[n_labels][K][LD]*/, int LD, int n_labels, float img_w, float img_h, VmThr thr, KptSigma sg,
                      int* __restrict__ ws_lab, float* __restrict__ ws_gt, float* __restrict__ ws_kp, float* __restrict__ ws_best,
                      unsigned char* __restrict__ correct_box, unsigned char* __restrict__ correct_pose) {
  __shared__ int s_nl;
  const int b = blockIdx.x, tid = threadIdx.x;
  int* lab = ws_lab + (long)b * n_labels;
  float* best = ws_best + (long)b * max_det * 4;
  unsigned char* cob = correct_box + (long)b * max_det * VM_NT;
  unsigned char* cop = correct_pose + (long)b * max_det * VM_NT;
  const int Dn = vm_count(count[b], max_det);
  vm_clear(cob, max_det * VM_NT);
  vm_clear(cop, max_det * VM_NT);
  vm_gather_labels(batch_idx, n_labels, b, lab, &s_nl);
  __syncthreads();
  const int L = s_nl;
  for (int k = tid; k < L; k += VM_THREADS) {                    // PoseDetector.cs:140, 148, 156
    const int j = lab[k];
    const float cx = bboxes[4 * j] * img_w, cy = bboxes[4 * j + 1] * img_h, w = bboxes[4 * j + 2] * img_w, h = bboxes[4 * j + 3] * img_h;
    const float x1 = cx - w / 2, y1 = cy - h / 2, x2 = cx + w / 2, y2 = cy + h / 2;
    float* g = ws_gt + 5L * j;
    g[0] = x1; g[1] = y1; g[2] = x2; g[3] = y2; g[4] = (x2 - x1) * (y2 - y1) * 0.53f;
  }
  for (int e = tid; e < L * K; e += VM_THREADS) {                // PoseDetector.cs:141-153
    const int k = e / K, q = e - k * K;
    const long j = lab[k];
    const float* src = keypoints + (j * K + q) * LD;
    float* dst = ws_kp + (j * K + q) * 3;
    dst[0] = src[0] * img_w; dst[1] = src[1] * img_h; dst[2] = LD == 3 ? src[2] : 1.0f;      // (w, h, 1): the third factor is exact
  }
  __syncthreads();
  for (int d = tid; d < Dn; d += VM_THREADS) {
    const float* pr = rows + ((long)b * max_det + d) * row_stride;
    const float px1 = pr[0], py1 = pr[1], px2 = pr[2], py2 = pr[3], pc = pr[5];
    VmBest bi, bo;
    for (int k = 0; k < L; k++) {
      const long j = lab[k];
      if (cls[j] != pc) continue;
      const float* g = ws_gt + 5 * j;
      bi.offer(vm_iou(g[0], g[1], g[2], g[3], px1, py1, px2, py2, 1e-7f), k);
      bo.offer(vm_oks(ws_kp + j * K * 3, pr + kpt_col, g[4], K, D, sg, 1e-7f), k);
    }
    bi.store(best + 4 * d);
    bo.store(best + 4 * d + 2);
  }
  __syncthreads();
  vm_credit<2>(best, L, Dn, thr, cob, cop);
}

// Metrics.mask_iou (Utils/Metrics.cs:120-125) as Segmenter.Val calls it (Models/Segmenter.cs:131-143): mask1[k] = (gt_ids == k + 1)
// from the overlap-encoded id map, mask2[j] = the 0/1 masks of Ops.process_mask.  The reference's float matmul of 0/1 values is
// an exact integer count (npix < 2^24), so  iou = inter / ((area1 + area2 - inter) + eps)  is reproduced bit for bit.
// One workgroup per predicted mask; LDS histograms over the label ids (dynamic LDS: 2 * nl ints).
__global__ void __launch_bounds__(VM_THREADS)
mask_iou_kernel(const float* __restrict__ gt_ids, int nl, const unsigned char* __restrict__ pm, int n, int npix, float eps,
                float* __restrict__ iou /*[nl][n]*/) {
  YS_DYN_LDS(lds);
  int* s_hist = (int*)lds;                 // [0, nl): |mask1[k]|, [nl, 2 nl): |mask1[k] & mask2[j]|
  __shared__ int s_area2;
  const int j = blockIdx.x, tid = threadIdx.x;
  for (int i = tid; i < 2 * nl; i += VM_THREADS) s_hist[i] = 0;
  if (tid == 0) s_area2 = 0;
  __syncthreads();
  const unsigned char* m2 = pm + (long)j * npix;
  int a2 = 0;
  for (int p = tid; p < npix; p += VM_THREADS) {
    const float idf = gt_ids[p];
    const int id = (int)idf;
    const bool lab = id >= 1 && id <= nl && (float)id == idf;       // (batch_mask == index) is an exact float comparison
    const bool on = m2[p] != 0;
    if (on) a2++;
    if (lab) {
      atomicAdd(&s_hist[id - 1], 1);
      if (on) atomicAdd(&s_hist[nl + id - 1], 1);
    }
  }
  atomicAdd(&s_area2, a2);
  __syncthreads();
  for (int k = tid; k < nl; k += VM_THREADS) {
    const float inter = (float)s_hist[nl + k];
    const float uni = ((float)s_hist[k] + (float)s_area2) - inter;
    iou[(long)k * n + j] = inter / (uni + eps);
  }
}

// match_predictions (Models/YoloBaseTaskModel.cs:377-446) on a caller-supplied IoU matrix [L][D]: stages 2 and 3 (one workgroup).
__global__ void __launch_bounds__(VM_THREADS)
match_iou_kernel(const float* __restrict__ pred_cls, int D, const float* __restrict__ true_cls, int L, const float* __restrict__ iou,
                 VmThr thr, float* __restrict__ best /*[D][2]*/, unsigned char* __restrict__ cor /*[D][10]*/) {
  vm_clear(cor, D * VM_NT);
  for (int d = threadIdx.x; d < D; d += VM_THREADS) {
    const float pc = pred_cls[d];
    VmBest bi;
    for (int k = 0; k < L; k++)
      if (true_cls[k] == pc) bi.offer(iou[(long)k * D + d], k);
    bi.store(best + 2 * d);
  }
  __syncthreads();
  vm_credit<1>(best, L, D, thr, cor, nullptr);
}

// torch.linspace(0.5, 0.95, 10) in fp32 (ATen: step = (end-start)/(steps-1); first half start + step*i, second half
// end - step*(steps-1-i))
static VmThr vm_thresholds() {
  VmThr t;
  const float start = 0.5f, end = 0.95f;
  const float step = (end - start) / (float)(VM_NT - 1);
  for (int i = 0; i < VM_NT; i++) t.t[i] = i < VM_NT / 2 ? start + step * (float)i : end - step * (float)(VM_NT - 1 - i);
  return t;
}

// Staging of the validation entry points: device pointers are used as they are, host arrays are copied to scratch that lives as long as the stage.
// rc: the first failure (its error text is set); finish() copies the outputs back and waits for the stream whenever scratch is in use.
namespace {
struct VmStage {
  const char* who; hipStream_t st; bool on_device; int rc = YS_OK;
  struct Back { void* host; const void* dev; size_t bytes; };
  std::vector<void*> tmp; std::vector<Back> back;
  VmStage(const char* w, ys_ctx* ctx, int od) : who(w), st(ctx->stream), on_device(od != 0) {}
  ~VmStage() { for (void* p : tmp) (void)hipFree(p); }
  void* alloc(size_t bytes) {
    void* p = nullptr;
    if (rc != YS_OK) return nullptr;
    if (hipMalloc(&p, bytes ? bytes : 4) != hipSuccess) { ys_set_error("%s: out of device memory", who); rc = YS_ERR_OOM; return nullptr; }
    tmp.push_back(p);
    return p;
  }
  const void* in(const void* host, size_t bytes) {
    if (on_device || !host) return host;
    void* d = alloc(bytes);
    if (d && bytes) rc = h2d(st, d, host, bytes);
    return d;
  }
  void* out(void* host, size_t bytes) {
    if (on_device) return host;
    void* d = alloc(bytes);
    back.push_back(Back{host, d, bytes});
    return d;
  }
  int finish() {
    YS_CHECK_HIP(hipGetLastError());
    for (const Back& o : back) YS_TRY(d2h(st, o.host, o.dev, o.bytes));
    if (!tmp.empty()) YS_CHECK_HIP(hipStreamSynchronize(st));      // the scratch is released when the stage goes out of scope
    return YS_OK;
  }
};
}  // namespace

extern "C" {

int ys_box_iou(ys_ctx* ctx, const float* box1, int n, const float* box2, int m, float eps, int on_device, float* iou) {
  YS_REQUIRE(ctx && iou && n >= 0 && m >= 0, "ys_box_iou: bad argument");
  if ((long)n * m == 0) return YS_OK;
  YS_REQUIRE(box1 && box2, "ys_box_iou: null boxes");
  YS_CHECK_HIP(hipSetDevice(ctx->device));
  VmStage sg("ys_box_iou", ctx, on_device);
  const float* d1 = (const float*)sg.in(box1, (size_t)n * 16);
  const float* d2 = (const float*)sg.in(box2, (size_t)m * 16);
  float* d_iou = (float*)sg.out(iou, (size_t)n * m * 4);
  YS_TRY(sg.rc);
  YS_LAUNCH(box_iou_kernel, ys_cdiv((long)n * m, VM_THREADS), VM_THREADS, sg.st, d1, n, d2, m, eps, d_iou);
  return sg.finish();
}

int ys_mask_iou(ys_ctx* ctx, const float* gt_ids, int nl, const uint8_t* pred_masks, int n, int npix, float eps, int on_device, float* iou) {
  YS_REQUIRE(ctx && iou && nl >= 0 && n >= 0 && npix > 0, "ys_mask_iou: bad argument");
  if ((long)nl * n == 0) return YS_OK;
  YS_REQUIRE(gt_ids && pred_masks, "ys_mask_iou: null masks");
  YS_REQUIRE(npix < (1 << 24), "ys_mask_iou: %d pixels exceed the exact-integer range of the fp32 reference", npix);
  YS_REQUIRE(nl <= 8192, "ys_mask_iou: %d labels exceed the LDS histogram capacity (8192)", nl);
  YS_CHECK_HIP(hipSetDevice(ctx->device));
  VmStage sg("ys_mask_iou", ctx, on_device);
  const float* d_ids = (const float*)sg.in(gt_ids, (size_t)npix * 4);
  const unsigned char* d_pm = (const unsigned char*)sg.in(pred_masks, (size_t)n * npix);
  float* d_iou = (float*)sg.out(iou, (size_t)nl * n * 4);
  YS_TRY(sg.rc);
  YS_LAUNCH_LDS(mask_iou_kernel, n, VM_THREADS, (size_t)2 * nl * sizeof(int) + 16, sg.st, d_ids, nl, d_pm, n, npix, eps, d_iou);
  return sg.finish();
}

// OKS_SIGMA (PoseDetector.cs:12-19) when K == 17, else 1 / K (Metrics.cs:205)
static KptSigma vm_sigmas(int kpt_num) {
  static const float oks[17] = {0.026f, 0.025f, 0.025f, 0.035f, 0.035f, 0.079f, 0.079f, 0.072f, 0.072f, 0.062f, 0.062f, 0.107f, 0.107f,
                                0.087f, 0.087f, 0.089f, 0.089f};
  KptSigma ks{};
  for (int k = 0; k < kpt_num; k++) ks.s[k] = kpt_num == 17 ? oks[k] : 1.0f / (float)kpt_num;
  return ks;
}

int ys_kpt_iou(ys_ctx* ctx, const float* kpt1, int n, const float* kpt2, int m, const float* area, int kpt_num, int kpt_dim, float eps,
               int on_device, float* iou) {
  YS_REQUIRE(ctx && iou && n >= 0 && m >= 0, "ys_kpt_iou: bad argument");
  YS_REQUIRE(kpt_num > 0 && kpt_num <= 64 && (kpt_dim == 2 || kpt_dim == 3), "ys_kpt_iou: %d keypoints of dim %d", kpt_num, kpt_dim);
  if ((long)n * m == 0) return YS_OK;
  YS_REQUIRE(kpt1 && kpt2 && area, "ys_kpt_iou: null argument");
  YS_CHECK_HIP(hipSetDevice(ctx->device));
  VmStage sg("ys_kpt_iou", ctx, on_device);
  const float* d1 = (const float*)sg.in(kpt1, (size_t)n * kpt_num * 3 * 4);
  const float* d2 = (const float*)sg.in(kpt2, (size_t)m * kpt_num * kpt_dim * 4);
  const float* da = (const float*)sg.in(area, (size_t)n * 4);
  float* d_iou = (float*)sg.out(iou, (size_t)n * m * 4);
  YS_TRY(sg.rc);
  YS_LAUNCH(kpt_iou_kernel, ys_cdiv((long)n * m, VM_THREADS), VM_THREADS, sg.st, d1, n, d2, m, da, kpt_num, kpt_dim, vm_sigmas(kpt_num), eps, d_iou);
  return sg.finish();
}

int ys_match_predictions(ys_ctx* ctx, const float* pred_cls, int n, const float* true_cls, int nl, const float* iou, int on_device,
                         uint8_t* correct) {
  YS_REQUIRE(ctx && n >= 0 && nl >= 0, "ys_match_predictions: bad argument");
  if (n == 0) return YS_OK;
  YS_REQUIRE(pred_cls && correct && (nl == 0 || (true_cls && iou)), "ys_match_predictions: null argument");
  YS_CHECK_HIP(hipSetDevice(ctx->device));
  VmStage sg("ys_match_predictions", ctx, on_device);
  const float* d_pc = (const float*)sg.in(pred_cls, (size_t)n * 4);
  const float* d_tc = (const float*)sg.in(true_cls, (size_t)nl * 4);
  const float* d_iou = (const float*)sg.in(iou, (size_t)nl * n * 4);
  unsigned char* d_cor = (unsigned char*)sg.out(correct, (size_t)n * VM_NT);
  float* d_best = (float*)sg.alloc((size_t)n * 8);
  YS_TRY(sg.rc);
  YS_LAUNCH(match_iou_kernel, 1, VM_THREADS, sg.st, d_pc, n, d_tc, nl, d_iou, vm_thresholds(), d_best, d_cor);
  return sg.finish();
}

// what the three batched entry points stage alike: rows [batch][max_det][row_stride], count [batch], the label arrays (bboxes of box_cols columns), and the
// scratch ws_lab [batch][n_labels] / ws_best [batch][max_det][2 per metric]
namespace {
struct VmBatch {
  const float *rows, *bi, *cl, *bb; const int* cnt; int* lab; float* best; size_t ncor;
  VmBatch(VmStage& sg, const float* rows_, const int32_t* count, int batch, int max_det, int row_stride, const float* batch_idx, const float* cls,
          const float* bboxes, int box_cols, int n_labels, int metrics) {
    ncor = (size_t)batch * max_det * VM_NT;
    lab = (int*)sg.alloc((size_t)batch * n_labels * 4);
    best = (float*)sg.alloc((size_t)batch * max_det * 8 * metrics);
    rows = (const float*)sg.in(rows_, (size_t)batch * max_det * row_stride * 4);
    cnt = (const int*)sg.in(count, (size_t)batch * 4);
    bi = (const float*)sg.in(batch_idx, (size_t)n_labels * 4);
    cl = (const float*)sg.in(cls, (size_t)n_labels * 4);
    bb = (const float*)sg.in(bboxes, (size_t)n_labels * box_cols * 4);
  }
};
}  // namespace

int ys_val_match_batched(ys_ctx* ctx, const float* rows, const int32_t* count, int on_device, int batch, int max_det, int row_stride,
                         const float* batch_idx, const float* cls, const float* bboxes, int n_labels, float img_w, float img_h,
                         uint8_t* correct) {
  YS_REQUIRE(ctx && rows && count && correct, "ys_val_match_batched: null argument");
  YS_REQUIRE(batch > 0 && max_det > 0 && row_stride >= 6 && n_labels >= 0, "ys_val_match_batched: bad shape");
  YS_REQUIRE(n_labels == 0 || (batch_idx && cls && bboxes), "ys_val_match_batched: null label arrays");
  YS_CHECK_HIP(hipSetDevice(ctx->device));
  VmStage sg("ys_val_match_batched", ctx, on_device);
  const VmBatch v(sg, rows, count, batch, max_det, row_stride, batch_idx, cls, bboxes, 4, n_labels, 1);
  unsigned char* d_cor = (unsigned char*)sg.out(correct, v.ncor);
  YS_TRY(sg.rc);
  YS_LAUNCH(val_match_kernel, batch, VM_THREADS, sg.st, v.rows, v.cnt, max_det, row_stride, v.bi, v.cl, v.bb, n_labels, img_w, img_h, vm_thresholds(),
            v.lab, v.best, d_cor);
  return sg.finish();
}

// Obber.Val's per-image part (Models/Obber.cs:102-114) for a batch: val_match_rot_kernel above
int ys_val_match_rotated_batched(ys_ctx* ctx, const float* rows, const int32_t* count, int on_device, int batch, int max_det, int row_stride,
                                 int angle_col, const float* batch_idx, const float* cls, const float* bboxes, int n_labels, float img_w,
                                 float img_h, uint8_t* correct) {
  YS_REQUIRE(ctx && rows && count && correct, "ys_val_match_rotated_batched: null argument");
  YS_REQUIRE(batch > 0 && max_det > 0 && row_stride >= 7 && n_labels >= 0, "ys_val_match_rotated_batched: bad shape");
  YS_REQUIRE(angle_col >= 6 && angle_col < row_stride, "ys_val_match_rotated_batched: angle column %d outside [6, %d)", angle_col, row_stride);
  YS_REQUIRE(n_labels == 0 || (batch_idx && cls && bboxes), "ys_val_match_rotated_batched: null label arrays");
  YS_CHECK_HIP(hipSetDevice(ctx->device));
  VmStage sg("ys_val_match_rotated_batched", ctx, on_device);
  const VmBatch v(sg, rows, count, batch, max_det, row_stride, batch_idx, cls, bboxes, 5, n_labels, 1);
  float* d_gt = (float*)sg.alloc((size_t)n_labels * 20);
  unsigned char* d_cor = (unsigned char*)sg.out(correct, v.ncor);
  YS_TRY(sg.rc);
  YS_LAUNCH(val_match_rot_kernel, batch, VM_THREADS, sg.st, v.rows, v.cnt, max_det, row_stride, angle_col, v.bi, v.cl, v.bb, n_labels, img_w, img_h,
            vm_thresholds(), v.lab, d_gt, v.best, d_cor);
  return sg.finish();
}

// PoseDetector.Val's per-image part (Models/PoseDetector.cs:131-165) for a batch: val_match_pose_kernel above
int ys_val_match_pose_batched(ys_ctx* ctx, const float* rows, const int32_t* count, int on_device, int batch, int max_det, int row_stride,
                              int kpt_col, int kpt_num, int kpt_dim, const float* batch_idx, const float* cls, const float* bboxes,
                              const float* keypoints, int label_kpt_dim, int n_labels, float img_w, float img_h, uint8_t* correct_box,
                              uint8_t* correct_pose) {
  YS_REQUIRE(ctx && rows && count && correct_box && correct_pose, "ys_val_match_pose_batched: null argument");
  YS_REQUIRE(batch > 0 && max_det > 0 && n_labels >= 0, "ys_val_match_pose_batched: bad shape");
  YS_REQUIRE(kpt_num > 0 && kpt_num <= 64 && (kpt_dim == 2 || kpt_dim == 3) && (label_kpt_dim == 2 || label_kpt_dim == 3),
             "ys_val_match_pose_batched: %d keypoints of dim %d, labels of dim %d", kpt_num, kpt_dim, label_kpt_dim);
  YS_REQUIRE(kpt_col >= 6 && kpt_col + kpt_num * kpt_dim <= row_stride, "ys_val_match_pose_batched: keypoint columns [%d, %d) outside a row of [6, %d)", kpt_col,
             kpt_col + kpt_num * kpt_dim, row_stride);
  YS_REQUIRE(n_labels == 0 || (batch_idx && cls && bboxes && keypoints), "ys_val_match_pose_batched: null label arrays");
  YS_CHECK_HIP(hipSetDevice(ctx->device));
  VmStage sg("ys_val_match_pose_batched", ctx, on_device);
  const VmBatch v(sg, rows, count, batch, max_det, row_stride, batch_idx, cls, bboxes, 4, n_labels, 2);
  const size_t nkp = (size_t)n_labels * kpt_num;
  float* d_gt = (float*)sg.alloc((size_t)n_labels * 20);
  float* d_kp = (float*)sg.alloc(nkp * 12);
  const float* d_kl = (const float*)sg.in(keypoints, nkp * label_kpt_dim * 4);
  unsigned char* d_cb = (unsigned char*)sg.out(correct_box, v.ncor);
  unsigned char* d_cp = (unsigned char*)sg.out(correct_pose, v.ncor);
  YS_TRY(sg.rc);
  YS_LAUNCH(val_match_pose_kernel, batch, VM_THREADS, sg.st, v.rows, v.cnt, max_det, row_stride, kpt_col, kpt_num, kpt_dim, v.bi, v.cl, v.bb, d_kl,
            label_kpt_dim, n_labels, img_w, img_h, vm_thresholds(), vm_sigmas(kpt_num), v.lab, d_gt, d_kp, v.best, d_cb, d_cp);
  return sg.finish();
}

}  // extern "C"
