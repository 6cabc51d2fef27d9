// augment_aa.hip -- the fourteen operators of torchvision's AutoAugment / RandAugment on uint8 planes [B, 3, H, W]: the transform ClassificationDataset puts
// between its flips and RandomErasing when Config.Auto_Augment is AutoAugment, the reference's default (Data/ClassificationDataset.cs:105-116,
// Data/Config.cs:228), or RandAugment.  What is restated is torchvision's public tensor / uint8 path with nearest interpolation and fill = None (transforms/
// _functional_tensor.py, autoaugment.py _apply_op); TorchVision.NET is not in the reference tree, parity with it is UNPINNED.  The draws (policy, probabilities,
// signs, magnitudes, the inverse affine matrix) stay on the host: an image brings one ys_aa_row = two slots of (op id, argument, theta).
//
// A slot is two launches over the batch, blockIdx.z = the image, the row wave-uniform:
//   aug_aa_stats_kernel   only for Contrast, AutoContrast and Equalize rows (the others leave at once): the gray sum, or the three 256-bin histograms built
//                         in LDS and flushed with integer atomics into the image's zeroed AaStats row -- any order gives the same row.  A thread takes
//                         AA_CHUNK quads of four consecutive bytes per plane; a quad of four equal bytes is ONE LDS atomic, which keeps a flat image from
//                         serialising every add of a wave on one address.
//   aug_aa_apply_kernel   reads the slot's INPUT image and writes its output (never in place: the warps and the stencil read neighbours).  AutoContrast's
//                         bounds and Equalize's table are rebuilt per workgroup from the 3 KB histogram (a 256-wide scan).  A thread takes four consecutive
//                         x of one row; one 4-byte store per plane where W % 4 == 0 and the bases are aligned, byte stores otherwise.
// Arithmetic (every fp32 step rounded on its own: this unit is compiled without contraction; hipcc's fp32 division is correctly rounded):
//   affine 0-4   r[0..2] = theta[0..2] / (0.5f w), r[3..5] = theta[3..5] / (0.5f h); bx = (float)x + (-w 0.5f + 0.5f), by likewise; gx = (bx r0 + by r1) + r2,
//                gy = (bx r3 + by r4) + r5; ux = ((gx + 1) w - 1) / 2; ix = nearbyint(ux) (half to even); in[iy][ix] inside the image, 0 outside --
//                _gen_affine_grid + grid_sample(nearest, zeros, align_corners = False)
//   blends 5-8   aug_jitter.h's blend with the other image 0 (Brightness), gray (Color), the mean of gray over the slot's input (Contrast), or the 3 x 3
//                filter [[1,1,1],[1,5,1],[1,1,1]] / 13 rounded to nearest on the interior and the input on the border (Sharpness; h <= 2 or w <= 2: unchanged).
//                The filter's sum S is an integer and S / 13 is never within 1 / 26 of a half: the byte is (S + 6) / 13 in integers
//   9 Posterize  v & -(1 << (8 - bits))        10 Solarize  (float)v >= threshold ? 255 - v : v        13 Invert  255 - v
//   11 AutoContrast  per channel: scale = (1.0f / (max - min)) * 255.0f -- torch evaluates a Python number over a tensor as reciprocal() * number, two
//                roundings, and 255 / 179 shows the difference -- (min, scale) = (0, 1) where max == min; trunc(clamp(((float)v - min) * scale, 0, 255))
//   12 Equalize  per channel, integers: step = (N - hist[last non-empty bin]) / 255; step == 0: unchanged; lut[0] = 0,
//                lut[v] = min((cumsum_inclusive[v - 1] + step / 2) / step, 255)
// An invalid row (aug_aa.h) writes the all-114 image in both slots.
#include "ys_internal.h"
#include "ys_kernels.h"
#include "aug_jitter.h"
#include "aug_aa.h"
#include <cmath>

#define AA_T 256
#define AA_CHUNK 8                      // quads per thread of the statistics launch: 8192 bytes of each plane per workgroup, one flush of <= 768 atomics

// four consecutive bytes of a plane at p (vec: one aligned 4-byte load; else `valid` of them, the rest 0)
__device__ __forceinline__ void aa_ld4(const unsigned char* __restrict__ p, int vec, int valid, unsigned v[4]) {
  if (vec) {
    const unsigned u = *(const unsigned*)p;
    v[0] = u & 255u; v[1] = (u >> 8) & 255u; v[2] = (u >> 16) & 255u; v[3] = u >> 24;
  } else {
#pragma unroll
    for (int j = 0; j < 4; j++) v[j] = j < valid ? (unsigned)p[j] : 0u;
  }
}

__device__ __forceinline__ void aa_st4(unsigned char* __restrict__ p, int vec, int valid, const unsigned v[4]) {
  if (vec) {
    *(unsigned*)p = v[0] | (v[1] << 8) | (v[2] << 16) | (v[3] << 24);
  } else {
#pragma unroll
    for (int j = 0; j < 4; j++)
      if (j < valid) p[j] = (unsigned char)v[j];
  }
}

// launch 1 of a slot: the statistics of the images whose row needs them.  n = H * W; a plane is walked as a flat array
__global__ void __launch_bounds__(AA_T)
aug_aa_stats_kernel(const unsigned char* __restrict__ in, const ys_aa_row* __restrict__ rows, int slot, long long n, int vec, AaStats* __restrict__ stats) {
  __shared__ unsigned s_hist[3 * 256];
  const ys_aa_row& R = rows[blockIdx.z];
  const int op = R.op[slot];
  if (!aug_aa_needs_stats(op) || !aug_aa_row_ok(R)) return;          // block-uniform
  const unsigned char* __restrict__ img = in + (long long)blockIdx.z * 3 * n;
  AaStats* __restrict__ S = stats + blockIdx.z;
  const long long q0 = (long long)blockIdx.x * AA_CHUNK * AA_T + threadIdx.x;
  if (op == AA_CONTRAST) {
    unsigned sum = 0;                                                 // <= 8 * 4 * 255 per thread, 2.1e6 per workgroup
    for (int k = 0; k < AA_CHUNK; k++) {
      const long long i = (q0 + (long long)k * AA_T) * 4;
      if (i >= n) break;
      const int valid = n - i < 4 ? (int)(n - i) : 4;
      unsigned r[4], g[4], b[4];
      aa_ld4(img + i, vec, valid, r); aa_ld4(img + n + i, vec, valid, g); aa_ld4(img + 2 * n + i, vec, valid, b);
#pragma unroll
      for (int j = 0; j < 4; j++) {
        AugPx px; px.c0 = (float)r[j]; px.c1 = (float)g[j]; px.c2 = (float)b[j];
        if (j < valid) sum += (unsigned)aug_jit_gray(px);
      }
    }
    s_hist[threadIdx.x] = sum;
    __syncthreads();
    for (int d = AA_T / 2; d > 0; d >>= 1) {
      if ((int)threadIdx.x < d) s_hist[threadIdx.x] += s_hist[threadIdx.x + d];
      __syncthreads();
    }
    if (threadIdx.x == 0) atomicAdd(&S->gray, (unsigned long long)s_hist[0]);
    return;
  }
  for (int t = threadIdx.x; t < 3 * 256; t += AA_T) s_hist[t] = 0;
  __syncthreads();
  for (int k = 0; k < AA_CHUNK; k++) {
    const long long i = (q0 + (long long)k * AA_T) * 4;
    if (i >= n) break;
    const int valid = n - i < 4 ? (int)(n - i) : 4;
#pragma unroll
    for (int c = 0; c < 3; c++) {
      unsigned v[4];
      aa_ld4(img + c * n + i, vec, valid, v);
      unsigned* h = s_hist + c * 256;
      if (valid == 4 && v[0] == v[1] && v[0] == v[2] && v[0] == v[3]) {
        atomicAdd(&h[v[0]], 4u);
      } else {
#pragma unroll
        for (int j = 0; j < 4; j++)
          if (j < valid) atomicAdd(&h[v[j]], 1u);
      }
    }
  }
  __syncthreads();
  unsigned* gh = &S->hist[0][0];
  for (int t = threadIdx.x; t < 3 * 256; t += AA_T)
    if (s_hist[t]) atomicAdd(&gh[t], s_hist[t]);
}

// one byte of the slot's input at (iy, ix) given as fp32 whole numbers after nearbyint, 0 outside the image (NaN compares false: outside)
__device__ __forceinline__ unsigned aa_fetch(const unsigned char* __restrict__ plane, int W, float fx, float fy, float wm1, float hm1) {
  if (!(fx >= 0.0f && fx <= wm1 && fy >= 0.0f && fy <= hm1)) return 0u;
  return (unsigned)plane[(long long)(int)fy * W + (int)fx];
}

// launch 2 of a slot: out = op(in) for every image
__global__ void __launch_bounds__(AA_T)
aug_aa_apply_kernel(const unsigned char* __restrict__ in, unsigned char* __restrict__ out, const ys_aa_row* __restrict__ rows, int slot, int H, int W, int vec,
                    const AaStats* __restrict__ stats) {
  __shared__ unsigned s_cum[3][256];
  __shared__ unsigned char s_lut[3][256];
  __shared__ int s_lo[3], s_hi[3];
  // wave-uniform, block-uniform: the row, its op
  const ys_aa_row& R = rows[blockIdx.z];
  const int op = aug_aa_row_ok(R) ? R.op[slot] : -2;
  const float arg = R.arg[slot];
  const long long n = (long long)H * W;
  const unsigned char* __restrict__ src = in + (long long)blockIdx.z * 3 * n;
  unsigned char* __restrict__ dst = out + (long long)blockIdx.z * 3 * n;
  const int t = threadIdx.x;

  if (op == AA_AUTOCONTRAST || op == AA_EQUALIZE) {                   // the tables from the image's histograms
    const AaStats* __restrict__ S = stats + blockIdx.z;
    if (t < 3) { s_lo[t] = 255; s_hi[t] = 0; }
#pragma unroll
    for (int c = 0; c < 3; c++) s_cum[c][t] = S->hist[c][t];
    __syncthreads();
#pragma unroll
    for (int c = 0; c < 3; c++)
      if (s_cum[c][t]) { atomicMin(&s_lo[c], t); atomicMax(&s_hi[c], t); }
    __syncthreads();
    if (op == AA_EQUALIZE) {
      for (int d = 1; d < 256; d <<= 1) {                             // inclusive scan of the three histograms
        unsigned a[3];
#pragma unroll
        for (int c = 0; c < 3; c++) a[c] = t >= d ? s_cum[c][t - d] : 0u;
        __syncthreads();
#pragma unroll
        for (int c = 0; c < 3; c++) s_cum[c][t] += a[c];
        __syncthreads();
      }
#pragma unroll
      for (int c = 0; c < 3; c++) {
        const int hi = s_hi[c];
        const unsigned last = s_cum[c][hi] - (hi > 0 ? s_cum[c][hi - 1] : 0u);
        const unsigned step = ((unsigned)n - last) / 255u;
        unsigned l = (unsigned)t;
        if (step) {
          l = t == 0 ? 0u : (s_cum[c][t - 1] + step / 2u) / step;
          l = l < 255u ? l : 255u;
        }
        s_lut[c][t] = (unsigned char)l;
      }
      __syncthreads();
    }
  }

  const int qpr = (W + 3) >> 2;
  const unsigned i = blockIdx.x * AA_T + threadIdx.x;
  if (i >= (unsigned)qpr * (unsigned)H) return;
  const int y = (int)(i / (unsigned)qpr), x0 = (int)(i - (unsigned)y * (unsigned)qpr) * 4;
  const int valid = W - x0 < 4 ? W - x0 : 4;
  const long long at = (long long)y * W + x0;
  unsigned o[3][4];

  if (op >= AA_SHEAR_X && op <= AA_ROTATE) {
    const float* __restrict__ th = R.theta[slot];
    const float w = (float)W, h = (float)H, hw = 0.5f * w, hh = 0.5f * h;
    const float r0 = th[0] / hw, r1 = th[1] / hw, r2 = th[2] / hw, r3 = th[3] / hh, r4 = th[4] / hh, r5 = th[5] / hh;
    const float by = (float)y + (-h * 0.5f + 0.5f), ox = -w * 0.5f + 0.5f;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const float bx = (float)(x0 + j) + ox;
      const float gx = (bx * r0 + by * r1) + r2, gy = (bx * r3 + by * r4) + r5;
      const float fx = nearbyintf(((gx + 1.0f) * w - 1.0f) / 2.0f), fy = nearbyintf(((gy + 1.0f) * h - 1.0f) / 2.0f);
#pragma unroll
      for (int c = 0; c < 3; c++) o[c][j] = aa_fetch(src + c * n, W, fx, fy, w - 1.0f, h - 1.0f);
    }
  } else if (op == -2) {
#pragma unroll
    for (int c = 0; c < 3; c++) { o[c][0] = 114u; o[c][1] = 114u; o[c][2] = 114u; o[c][3] = 114u; }
  } else {
#pragma unroll
    for (int c = 0; c < 3; c++) aa_ld4(src + c * n + at, vec, valid, o[c]);
    if (op >= AA_BRIGHTNESS && op <= AA_SHARPNESS) {
      const float f = arg, g = 1.0f - f;
      if (op != AA_SHARPNESS || (H > 2 && W > 2)) {
        float other[3][4];                                            // the image blended against
        if (op == AA_SHARPNESS) {
          const bool yin = y >= 1 && y < H - 1;
#pragma unroll
          for (int c = 0; c < 3; c++) {
            const unsigned char* __restrict__ p = src + c * n;
            unsigned col[6] = {0u, 0u, 0u, 0u, 0u, 0u};               // the 3-row sums of columns x0 - 1 .. x0 + 4
            if (yin) {
#pragma unroll
              for (int k = 0; k < 6; k++) {
                const int x = x0 - 1 + k;
                if (x >= 0 && x < W) col[k] = (unsigned)p[at - W - 1 + k] + (unsigned)p[at - 1 + k] + (unsigned)p[at + W - 1 + k];
              }
            }
#pragma unroll
            for (int j = 0; j < 4; j++) {
              const int x = x0 + j;
              const bool inner = yin && x >= 1 && x < W - 1;
              const unsigned sum = col[j] + col[j + 1] + col[j + 2] + 4u * o[c][j];
              other[c][j] = inner ? (float)((sum + 6u) / 13u) : (float)o[c][j];
            }
          }
        } else {
          const float mean = op == AA_CONTRAST ? (float)stats[blockIdx.z].gray / (float)n : 0.0f;
#pragma unroll
          for (int j = 0; j < 4; j++) {
            AugPx px; px.c0 = (float)o[0][j]; px.c1 = (float)o[1][j]; px.c2 = (float)o[2][j];
            const float v = op == AA_COLOR ? aug_jit_gray(px) : mean;   // Brightness: mean is 0
            other[0][j] = v; other[1][j] = v; other[2][j] = v;
          }
        }
#pragma unroll
        for (int c = 0; c < 3; c++)
#pragma unroll
          for (int j = 0; j < 4; j++) o[c][j] = (unsigned)aug_jit_blend((float)o[c][j], other[c][j], f, g);
      }
    } else if (op == AA_POSTERIZE) {
      const unsigned mask = (unsigned)(-(1 << (8 - (int)arg))) & 255u;
#pragma unroll
      for (int c = 0; c < 3; c++)
#pragma unroll
        for (int j = 0; j < 4; j++) o[c][j] &= mask;
    } else if (op == AA_SOLARIZE) {
#pragma unroll
      for (int c = 0; c < 3; c++)
#pragma unroll
        for (int j = 0; j < 4; j++) o[c][j] = (float)o[c][j] >= arg ? 255u - o[c][j] : o[c][j];
    } else if (op == AA_INVERT) {
#pragma unroll
      for (int c = 0; c < 3; c++)
#pragma unroll
        for (int j = 0; j < 4; j++) o[c][j] = 255u - o[c][j];
    } else if (op == AA_AUTOCONTRAST) {
#pragma unroll
      for (int c = 0; c < 3; c++) {
        const int lo = s_lo[c], hi = s_hi[c];
        const float mn = hi == lo ? 0.0f : (float)lo, scale = hi == lo ? 1.0f : (1.0f / ((float)hi - (float)lo)) * 255.0f;
#pragma unroll
        for (int j = 0; j < 4; j++) o[c][j] = (unsigned)truncf(fminf(fmaxf(((float)o[c][j] - mn) * scale, 0.0f), 255.0f));
      }
    } else if (op == AA_EQUALIZE) {
#pragma unroll
      for (int c = 0; c < 3; c++)
#pragma unroll
        for (int j = 0; j < 4; j++) o[c][j] = s_lut[c][o[c][j]];
    }                                                                 // AA_NONE: the copy
  }
#pragma unroll
  for (int c = 0; c < 3; c++) aa_st4(dst + c * n + at, vec, valid, o[c]);
}

// ---------------------------------------------------------------------------------------------------------------- launchers
int ys_aa_row_ok_host(const ys_aa_row* row) { return aug_aa_row_ok(*row); }
int ys_aa_row_needs_stats_host(const ys_aa_row* row, int slot) { return aug_aa_needs_stats(row->op[slot]); }
size_t ys_aa_stats_bytes(int B) { return (size_t)2 * B * sizeof(AaStats); }

// in -> slot 0 -> mid -> slot 1 -> out, all uint8 [B, 3, H, W]; mid differs from in and out (out may be in).  stats: ys_aa_stats_bytes(B) zeroed bytes;
// stats_mask bit k = slot k's statistics launch runs (a host that read the rows clears the bit of a slot no row of which needs it)
int ys_aa_slots_launch(hipStream_t st, const unsigned char* in, unsigned char* mid, unsigned char* out, const ys_aa_row* rows, int B, int H, int W,
                       int stats_mask, void* stats) {
  const long long n = (long long)H * W;
  const dim3 sgrid(ys_cdiv(ys_cdiv(n, 4), (long)AA_CHUNK * AA_T), 1, B), agrid(ys_cdiv((long)((W + 3) / 4) * H, AA_T), 1, B);
  const unsigned char* src[2] = {in, mid};
  unsigned char* dst[2] = {mid, out};
  for (int k = 0; k < 2; k++) {
    AaStats* S = (AaStats*)stats + (size_t)k * B;
    const int aligned = (((size_t)src[k] | (size_t)dst[k]) & 3) == 0;
    if ((stats_mask >> k) & 1) YS_LAUNCH(aug_aa_stats_kernel, sgrid, AA_T, st, src[k], rows, k, n, (aligned && n % 4 == 0) ? 1 : 0, S);
    YS_LAUNCH(aug_aa_apply_kernel, agrid, AA_T, st, src[k], dst[k], rows, k, H, W, (aligned && W % 4 == 0) ? 1 : 0, (const AaStats*)S);
  }
  return YS_OK;
}
