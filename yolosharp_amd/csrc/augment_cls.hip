// augment_cls.hip -- the classification training and validation input on the device: ClassificationDataset's chain with Auto_Augment = None
// (Data/ClassificationDataset.cs:90-131, GetTensor :70-88) as ONE fused gather per batch: no cropped, resized or uint8 intermediate image exists -- and
// with AutoAugment / RandAugment rows the same chain around the operator slots of augment_aa.hip (the last paragraph below).
//
//   train: RandomResizedCrop(imgsz, scale, ratio) (:95) -> RandomHorizontalFlip (:98) -> RandomVerticalFlip (:102) -> RandomErasing (:120, the
//          reference's own class :166-226) -> ColorJitter(vgain, vgain, sgain, hgain) (:122) -> mul(1 / 255.0f) (:79)
//   val:   Resize(imgsz) (:126) -> CenterCrop(imgsz) (:127) -> mul(1 / 255.0f)
//   label: the source's class id, one per image (:80-83), fp32 (what ys_loss_classify(..., on_device = 1) reads)
//
// Geometry: one mapping serves both.  The flips are folded into the output coordinate, y' = flip_ud ? s - 1 - y : y (x' likewise), and
//   out[y][x] = src[top + min(floor((y' + oy) * ((float)ch / (float)oh)), ch - 1)][left + min(floor((x' + ox) * ((float)cw / (float)ow)), cw - 1)]
// -- the project's nearest rule (ATen legacy nearest in fp32, the one aug_letterbox_kernel uses) on the crop window (top, left, ch, cw) of the source
// resized to (oh, ow), of which the s x s window at (oy, ox) is taken.  Train: oh = ow = s, oy = ox = 0.  Val: the window is the whole source,
// (oh, ow) the resized size and (oy, ox) the centre-crop offset.
//
// Erase: in the OUTPUT frame -- after the flips, in front of the jitter -- a pixel with er_y <= y < er_y + er_h and er_x <= x < er_x + er_w takes one
// noise byte per channel.  The reference writes torch.empty(c, h, w).normal_(), a float tensor, into the uint8 image: ATen's CPU cast truncates toward
// zero and wraps mod 256 (-1.3 -> 255, -2.7 -> 254, 0.7 -> 0, 1.9 -> 1).  The byte is drawn from exactly that distribution, (uint8)(int64)z with
// z ~ N(0, 1), by integer thresholds on one 32-bit word, without a transcendental: value k = 0 covers (-1, 1), k > 0 covers [k, k + 1), k < 0 covers
// (k - 1, k]; the table holds k = -6 .. 6 (DEVIATION: the tails beyond +-7, mass 2.6e-12, fold into +-6) as round(2^32 * cumulative probability),
// computed in float64 from erf; the last threshold is 2^32 (every word is below it).  The word is a counter-based function of (er_seed, c, y, x), so the
// result does not depend on the launch shape:
//   u = mix32(mix32(er_seed ^ (c * 0x9e3779b9u)) + (y * s + x))        c = the channel, (y, x) = the output pixel, all in uint32 arithmetic
//   mix32(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16
//   k = -6 + the number of thresholds T[0..11] with u >= T[i];  byte = k & 255
//
// Jitter: the three bytes go through the image's ys_aug_jitter row (aug_jitter.h, the arithmetic of the other gather kernels), then
// (float)byte * (1 / 255.0f).  jitter == NULL: none (the val chain).  Contrast -- the classification chain always has it: the reference passes vgain as
// contrast -- needs the mean of the gray image in its state in front of the contrast op over the s x s OUTPUT, so a batch with contrast rows takes
// two launches like ys_color_jitter:
//   aug_cls_gray_sum_kernel   replays gather + erase + the ops ahead of contrast and adds the gray bytes into sums[b]: a reduction in LDS, one integer
//                             atomic per workgroup (any order gives the same sum).  Images whose row has no contrast leave at once.
//   aug_cls_apply_kernel      the whole chain with mean = (float)sum / (float)(s * s): for s * s <= 65536 (s = 224 included) torch.mean's value bit
//                             for bit; above that the deviation ys_color_jitter documents carries over.  One thread of each image also writes
//                             out_cls[b] = src_cls[items[b].src].
// A thread takes four consecutive output x of one row and writes three 16-byte stores (s % 4 == 0 and an aligned base; scalar stores otherwise), as
// aug_letterbox_kernel does; blockIdx.z is the image.
// A refused item or jitter row (aug_cls_item_ok; aug_jitter_state == 0) gives the all-114 image, not jittered, and class -1.
//
// Auto_Augment = AutoAugment / RandAugment (:105-116; ys_augment_classify_aa with rows): the two operator slots stand between the flips and the erase and
// need the whole image (histograms, means, warps, a stencil), so that chain has intermediates -- the plain one keeps none:
//   aug_cls_stage_kernel          crop + flips of every image as uint8 [B, 3, s, s] in the context's workspace (a quarter of the output's bytes)
//   augment_aa.hip                slot 0 into a second such image, slot 1 back into the first (a statistics and an apply launch each)
//   aug_cls_gray_sum_kernel<true> / aug_cls_apply_kernel<true>   the two launches above with the staged bytes in place of the source gather (STAGED): the
//                                 erase rectangle, the noise, the jitter and the stores are the same code.  A refused ys_aa_row refuses the image too.
#include "ys_internal.h"
#include "ys_kernels.h"
#include "aug_jitter.h"
#include "aug_aa.h"
#include <cmath>

#define AUGC_T 256

// an item the kernels can run (include/yolosharp_hip.h lists the same rules)
__host__ __device__ inline int aug_cls_item_ok(const ys_cls_item& it, const ys_aug_src* srcs, int n_src, int s) {
  if (it.src < 0 || it.src >= n_src) return 0;
  const ys_aug_src& sr = srcs[it.src];
  if (sr.h < 1 || sr.w < 1 || sr.img_off < 0) return 0;
  if (it.ch < 1 || it.cw < 1 || it.top < 0 || it.left < 0 || (long long)it.top + it.ch > sr.h || (long long)it.left + it.cw > sr.w) return 0;
  if (it.oh < 1 || it.ow < 1 || it.oy < 0 || it.ox < 0 || (long long)it.oy + s > it.oh || (long long)it.ox + s > it.ow) return 0;
  if ((it.flip_lr != 0 && it.flip_lr != 1) || (it.flip_ud != 0 && it.flip_ud != 1)) return 0;
  if (it.er_y == 0 && it.er_x == 0 && it.er_h == 0 && it.er_w == 0) return 1;                    // no erase
  if (it.er_h < 1 || it.er_w < 1 || it.er_y < 0 || it.er_x < 0 || (long long)it.er_y + it.er_h > s || (long long)it.er_x + it.er_w > s) return 0;
  return 1;
}

__device__ __forceinline__ unsigned aug_cls_mix32(unsigned x) {
  x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
  return x;
}

// (uint8)(int64)z, z ~ N(0, 1), from the word of (seed, c, pixel index y * s + x): the byte as a whole number in fp32
__device__ __forceinline__ float aug_cls_noise(unsigned seed, unsigned c, unsigned pix) {
  // round(2^32 * Phi(k)) for k = -6 .. -1, 1 .. 6 (float64, from erf); the thirteenth, 2^32, is above every word
  constexpr unsigned T[12] = {0x00000004u, 0x000004cfu, 0x0002135bu, 0x00587788u, 0x05d2f3e1u, 0x289da177u,
                              0xd7625e89u, 0xfa2d0c1fu, 0xffa78878u, 0xfffdeca5u, 0xfffffb31u, 0xfffffffcu};
  const unsigned u = aug_cls_mix32(aug_cls_mix32(seed ^ (c * 0x9e3779b9u)) + pix);
  int k = -6;
#pragma unroll
  for (int i = 0; i < 12; i++) k += u >= T[i] ? 1 : 0;
  return (float)(k & 255);
}

// what a thread needs of a valid item, wave-uniform
struct AugClsGeom {
  const unsigned char* base;          // the source's first plane at (top, left)
  long long plane;                    // H * W
  int W, ch, cw, oy, ox, flr, fud, er_y0, er_y1, er_x0, er_x1;
  unsigned seed;
  float sy, sx;
};

__device__ __forceinline__ AugClsGeom aug_cls_geom(const unsigned char* __restrict__ arena, const ys_aug_src& sr, const ys_cls_item& it) {
  AugClsGeom g;
  g.base = arena + sr.img_off + (long long)it.top * sr.w + it.left;
  g.plane = (long long)sr.h * sr.w;
  g.W = sr.w; g.ch = it.ch; g.cw = it.cw; g.oy = it.oy; g.ox = it.ox; g.flr = it.flip_lr; g.fud = it.flip_ud;
  g.er_y0 = it.er_y; g.er_y1 = it.er_y + it.er_h; g.er_x0 = it.er_x; g.er_x1 = it.er_x + it.er_w;      // an empty rectangle when there is no erase
  g.seed = it.er_seed;
  g.sy = (float)it.ch / (float)it.oh; g.sx = (float)it.cw / (float)it.ow;
  return g;
}

// the quad's four pixels at (x0 .. x0 + 3, y) after gather and erase: three bytes each as fp32; positions at or past s stay 114 and are never stored.
// STAGED: the bytes outside the erase rectangle come from `staged`, the image's uint8 [3, s, s] planes (crop and flips done, the AutoAugment slots run)
template <bool STAGED>
__device__ __forceinline__ void aug_cls_quad(const AugClsGeom& g, const unsigned char* __restrict__ staged, int s, int x0, int y, AugPx& p0, AugPx& p1,
                                             AugPx& p2, AugPx& p3) {
  float v[3][4];
  const unsigned char* __restrict__ row;
  if (STAGED) {
    row = staged + (long long)y * s;
  } else {
    const int ly = g.fud ? s - 1 - y : y;
    int iy = (int)floorf((float)(ly + g.oy) * g.sy);
    iy = iy < g.ch - 1 ? iy : g.ch - 1;
    row = g.base + (long long)iy * g.W;
  }
  const bool er_row = y >= g.er_y0 && y < g.er_y1;
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const int x = x0 + j;
    v[0][j] = 114.0f; v[1][j] = 114.0f; v[2][j] = 114.0f;
    if (x < s) {
      if (er_row && x >= g.er_x0 && x < g.er_x1) {
        const unsigned pix = (unsigned)y * (unsigned)s + (unsigned)x;
#pragma unroll
        for (int c = 0; c < 3; c++) v[c][j] = aug_cls_noise(g.seed, (unsigned)c, pix);
      } else if (STAGED) {
#pragma unroll
        for (int c = 0; c < 3; c++) v[c][j] = (float)row[(long long)c * s * s + x];
      } else {
        const int lx = g.flr ? s - 1 - x : x;
        int ix = (int)floorf((float)(lx + g.ox) * g.sx);
        ix = ix < g.cw - 1 ? ix : g.cw - 1;
#pragma unroll
        for (int c = 0; c < 3; c++) v[c][j] = (float)row[c * g.plane + ix];
      }
    }
  }
  p0.c0 = v[0][0]; p0.c1 = v[1][0]; p0.c2 = v[2][0]; p1.c0 = v[0][1]; p1.c1 = v[1][1]; p1.c2 = v[2][1];
  p2.c0 = v[0][2]; p2.c1 = v[1][2]; p2.c2 = v[2][2]; p3.c0 = v[0][3]; p3.c1 = v[1][3]; p3.c2 = v[2][3];
}

// AutoAugment, launch 1: crop + flips of every image as uint8 [B, 3, s, s] -- what the slots read; no erase, no jitter.  A refused item stages 114
__global__ void __launch_bounds__(AUGC_T)
aug_cls_stage_kernel(const unsigned char* __restrict__ arena, const ys_aug_src* __restrict__ srcs, int n_src, const ys_cls_item* __restrict__ items, int s,
                     int vec, unsigned char* __restrict__ staged) {
  const ys_cls_item& it = items[blockIdx.z];
  const int qpr = (s + 3) >> 2;
  const unsigned i = blockIdx.x * AUGC_T + threadIdx.x;
  if (i >= (unsigned)qpr * (unsigned)s) return;
  const int y = (int)(i / (unsigned)qpr), x0 = (int)(i - (unsigned)y * (unsigned)qpr) * 4;
  AugPx p[4];
  p[0].c0 = p[0].c1 = p[0].c2 = 114.0f; p[1] = p[0]; p[2] = p[0]; p[3] = p[0];
  if (aug_cls_item_ok(it, srcs, n_src, s)) {
    AugClsGeom g = aug_cls_geom(arena, srcs[it.src], it);
    g.er_y0 = g.er_y1 = g.er_x0 = g.er_x1 = 0;                 // the erase comes after the slots
    aug_cls_quad<false>(g, nullptr, s, x0, y, p[0], p[1], p[2], p[3]);
  }
  const long long plane = (long long)s * s;
  unsigned char* dst = staged + (long long)blockIdx.z * 3 * plane + (long long)y * s + x0;
  if (vec) {
    *(unsigned*)dst = (unsigned)p[0].c0 | ((unsigned)p[1].c0 << 8) | ((unsigned)p[2].c0 << 16) | ((unsigned)p[3].c0 << 24);
    *(unsigned*)(dst + plane) = (unsigned)p[0].c1 | ((unsigned)p[1].c1 << 8) | ((unsigned)p[2].c1 << 16) | ((unsigned)p[3].c1 << 24);
    *(unsigned*)(dst + 2 * plane) = (unsigned)p[0].c2 | ((unsigned)p[1].c2 << 8) | ((unsigned)p[2].c2 << 16) | ((unsigned)p[3].c2 << 24);
  } else {
    for (int j = 0; j < 4 && x0 + j < s; j++) {
      dst[j] = (unsigned char)p[j].c0; dst[plane + j] = (unsigned char)p[j].c1; dst[2 * plane + j] = (unsigned char)p[j].c2;
    }
  }
}

// contrast, launch 1 of 2: sums[b] += the gray bytes of output image b in its state in front of the contrast op.  STAGED (the AutoAugment chain): the
// bytes come from `staged` and a refused ys_aa_row refuses the image
template <bool STAGED>
__global__ void __launch_bounds__(AUGC_T)
aug_cls_gray_sum_kernel(const unsigned char* __restrict__ arena, const ys_aug_src* __restrict__ srcs, int n_src, const ys_cls_item* __restrict__ items,
                        const ys_aug_jitter* __restrict__ jitter, int s, unsigned long long* __restrict__ sums, const unsigned char* __restrict__ staged,
                        const ys_aa_row* __restrict__ aa) {
  __shared__ unsigned s_red[AUGC_T];
  const ys_aug_jitter* __restrict__ J = jitter + blockIdx.z;
  if (aug_jitter_state(*J) != 2) return;                  // wave-uniform, block-uniform
  const ys_cls_item& it = items[blockIdx.z];
  if (!aug_cls_item_ok(it, srcs, n_src, s)) return;
  if (STAGED && !aug_aa_row_ok(aa[blockIdx.z])) return;
  const int qpr = (s + 3) >> 2;
  const unsigned i = blockIdx.x * AUGC_T + threadIdx.x;
  unsigned sum = 0;
  if (i < (unsigned)qpr * (unsigned)s) {
    const int y = (int)(i / (unsigned)qpr), x0 = (int)(i - (unsigned)y * (unsigned)qpr) * 4;
    const AugClsGeom g = aug_cls_geom(arena, srcs[it.src], it);
    AugPx p0, p1, p2, p3;
    aug_cls_quad<STAGED>(g, STAGED ? staged + (long long)blockIdx.z * 3 * s * s : nullptr, s, x0, y, p0, p1, p2, p3);
    aug_jitter_quad(J, 0.0f, true, p0, p1, p2, p3);
    sum = (unsigned)aug_jit_gray(p0);
    if (x0 + 1 < s) sum += (unsigned)aug_jit_gray(p1);
    if (x0 + 2 < s) sum += (unsigned)aug_jit_gray(p2);
    if (x0 + 3 < s) sum += (unsigned)aug_jit_gray(p3);
  }
  s_red[threadIdx.x] = sum;
  __syncthreads();
  for (int d = AUGC_T / 2; d > 0; d >>= 1) {
    if ((int)threadIdx.x < d) s_red[threadIdx.x] += s_red[threadIdx.x + d];
    __syncthreads();
  }
  if (threadIdx.x == 0) atomicAdd(&sums[blockIdx.z], (unsigned long long)s_red[0]);
}

// launch 2 of 2 (the only one for a batch without contrast rows): the whole chain, the fp32 image and the image's class id
template <bool STAGED>
__global__ void __launch_bounds__(AUGC_T)
aug_cls_apply_kernel(const unsigned char* __restrict__ arena, const ys_aug_src* __restrict__ srcs, int n_src, const float* __restrict__ src_cls,
                     const ys_cls_item* __restrict__ items, const ys_aug_jitter* __restrict__ jitter, int s, int vec,
                     const unsigned long long* __restrict__ sums, float* __restrict__ images, float* __restrict__ out_cls,
                     const unsigned char* __restrict__ staged, const ys_aa_row* __restrict__ aa) {
  // wave-uniform: the item, its jitter row and whether the image is refused
  const ys_cls_item& it = items[blockIdx.z];
  const ys_aug_jitter* __restrict__ J = jitter ? jitter + blockIdx.z : nullptr;
  const int jstate = J ? aug_jitter_state(*J) : 1;
  const bool ok = jstate != 0 && aug_cls_item_ok(it, srcs, n_src, s) && (!STAGED || aug_aa_row_ok(aa[blockIdx.z]));
  if (blockIdx.x == 0 && threadIdx.x == 0) out_cls[blockIdx.z] = ok ? src_cls[it.src] : -1.0f;
  const int qpr = (s + 3) >> 2;
  const unsigned i = blockIdx.x * AUGC_T + threadIdx.x;
  if (i >= (unsigned)qpr * (unsigned)s) return;
  const int y = (int)(i / (unsigned)qpr), x0 = (int)(i - (unsigned)y * (unsigned)qpr) * 4;
  AugPx p0, p1, p2, p3;
  if (ok) {
    const AugClsGeom g = aug_cls_geom(arena, srcs[it.src], it);
    aug_cls_quad<STAGED>(g, STAGED ? staged + (long long)blockIdx.z * 3 * s * s : nullptr, s, x0, y, p0, p1, p2, p3);
    if (J) {
      const float mean = jstate == 2 ? (float)sums[blockIdx.z] / (float)((long long)s * s) : 0.0f;
      aug_jitter_quad(J, mean, false, p0, p1, p2, p3);
    }
  } else {
    p0.c0 = p0.c1 = p0.c2 = 114.0f; p1 = p0; p2 = p0; p3 = p0;
  }
  const float q = 1 / 255.0f;                             // mul(1 / 255.0f), ClassificationDataset.cs:79: a multiply, bit-exact per byte
  p0.c0 *= q; p0.c1 *= q; p0.c2 *= q; p1.c0 *= q; p1.c1 *= q; p1.c2 *= q; p2.c0 *= q; p2.c1 *= q; p2.c2 *= q; p3.c0 *= q; p3.c1 *= q; p3.c2 *= q;
  const long long plane = (long long)s * s;
  float* dst = images + (long long)blockIdx.z * 3 * plane + (long long)y * s + x0;
  if (vec) {
    ys_st16(dst, make_uint4(ys_f2u(p0.c0), ys_f2u(p1.c0), ys_f2u(p2.c0), ys_f2u(p3.c0)));
    ys_st16(dst + plane, make_uint4(ys_f2u(p0.c1), ys_f2u(p1.c1), ys_f2u(p2.c1), ys_f2u(p3.c1)));
    ys_st16(dst + 2 * plane, make_uint4(ys_f2u(p0.c2), ys_f2u(p1.c2), ys_f2u(p2.c2), ys_f2u(p3.c2)));
  } else {
    if (x0 < s) { dst[0] = p0.c0; dst[plane] = p0.c1; dst[2 * plane] = p0.c2; }
    if (x0 + 1 < s) { dst[1] = p1.c0; dst[plane + 1] = p1.c1; dst[2 * plane + 1] = p1.c2; }
    if (x0 + 2 < s) { dst[2] = p2.c0; dst[plane + 2] = p2.c1; dst[2 * plane + 2] = p2.c2; }
    if (x0 + 3 < s) { dst[3] = p3.c0; dst[plane + 3] = p3.c1; dst[2 * plane + 3] = p3.c2; }
  }
}

// ---------------------------------------------------------------------------------------------------------------- launchers
int ys_aug_cls_item_ok_host(const ys_cls_item* it, const ys_aug_src* srcs, int n_src, int s) { return aug_cls_item_ok(*it, srcs, n_src, s); }

// sums: B 64-bit counters, zeroed by the caller when with_contrast (read and written only where a row runs contrast); with_contrast = 0 skips the reduction
int ys_aug_classify_launch(hipStream_t st, const unsigned char* arena, const ys_aug_src* srcs, int n_src, const float* src_cls, const ys_cls_item* items,
                           int B, int s, const ys_aug_jitter* jitter, int with_contrast, void* sums, float* images, float* out_cls) {
  const long quads = (long)((s + 3) / 4) * s;
  const dim3 grid(ys_cdiv(quads, AUGC_T), 1, B);
  const unsigned char* no_stage = nullptr;
  const ys_aa_row* no_aa = nullptr;
  if (jitter && with_contrast)
    YS_LAUNCH(aug_cls_gray_sum_kernel<false>, grid, AUGC_T, st, arena, srcs, n_src, items, jitter, s, (unsigned long long*)sums, no_stage, no_aa);
  YS_LAUNCH(aug_cls_apply_kernel<false>, grid, AUGC_T, st, arena, srcs, n_src, src_cls, items, jitter, s, (s % 4 == 0 && ((size_t)images & 15) == 0) ? 1 : 0,
            (const unsigned long long*)sums, images, out_cls, no_stage, no_aa);
  return YS_OK;
}

// the chain with the AutoAugment / RandAugment slots between the flips and the erase: crop + flips staged as uint8 (stage_a), slot 0 into stage_b, slot 1 back
// into stage_a (augment_aa.hip), then the two launches above on the staged bytes -- seven launches at most.  stage_a / stage_b: B * 3 * s * s bytes each,
// 4-byte aligned; aa_stats: ys_aa_stats_bytes(B) zeroed bytes; stats_mask: ys_aa_slots_launch
int ys_aug_classify_aa_launch(hipStream_t st, const unsigned char* arena, const ys_aug_src* srcs, int n_src, const float* src_cls, const ys_cls_item* items,
                              int B, int s, const ys_aa_row* aa, int stats_mask, void* aa_stats, unsigned char* stage_a, unsigned char* stage_b,
                              const ys_aug_jitter* jitter, int with_contrast, void* sums, float* images, float* out_cls) {
  const long quads = (long)((s + 3) / 4) * s;
  const dim3 grid(ys_cdiv(quads, AUGC_T), 1, B);
  YS_LAUNCH(aug_cls_stage_kernel, grid, AUGC_T, st, arena, srcs, n_src, items, s, (s % 4 == 0 && ((size_t)stage_a & 3) == 0) ? 1 : 0, stage_a);
  YS_TRY(ys_aa_slots_launch(st, stage_a, stage_b, stage_a, aa, B, s, s, stats_mask, aa_stats));
  const unsigned char* staged = stage_a;
  if (jitter && with_contrast)
    YS_LAUNCH(aug_cls_gray_sum_kernel<true>, grid, AUGC_T, st, arena, srcs, n_src, items, jitter, s, (unsigned long long*)sums, staged, aa);
  YS_LAUNCH(aug_cls_apply_kernel<true>, grid, AUGC_T, st, arena, srcs, n_src, src_cls, items, jitter, s, (s % 4 == 0 && ((size_t)images & 15) == 0) ? 1 : 0,
            (const unsigned long long*)sums, images, out_cls, staged, aa);
  return YS_OK;
}
