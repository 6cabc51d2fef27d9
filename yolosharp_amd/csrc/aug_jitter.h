// aug_jitter.h -- the ColorJitter device functions the gather kernels of augment.hip and augment_cls.hip run in their epilogue, and ys_color_jitter on its own.
// Device code of units compiled without contraction (build.py NO_CONTRACT): every step below is one rounded fp32 operation.
#pragma once
#include "ys_internal.h"
#include "ys_kernels.h"
#include <cmath>

// ---------------------------------------------------------------------------------------------------------------- ColorJitter (RandomHSV)
// RandomHSV (Data/Augment.cs:968-987) is torchvision ColorJitter(brightness 0.4, contrast 0, saturation 0.7, hue 0.015) on the uint8 image, the last
// transform of both training chains (Data/YoloDataset.cs:86, :416).  TorchVision.NET is not part of the reference tree: what is restated here is
// torchvision's public uint8 algorithm (transforms/_functional_tensor.py: _blend, rgb_to_grayscale, adjust_hue, _rgb2hsv, _hsv2rgb,
// convert_image_dtype); parity with TorchVision.NET is UNPINNED.  Every op ends in a byte (truncation BETWEEN the ops), every step is one rounded fp32
// operation (this file is compiled without contraction), hipcc's fp32 division is correctly rounded: the result is bit-exact against an fp32
// restatement (tests/color_jitter_ref.py).
//   blend(a, b, f) = trunc(clamp(f * a + (1 - f) * b, 0, 255)); 1.0 - f is formed in double there and then rounded: for an fp32 f that IS 1.0f - f
//   gray = trunc((0.2989f r + 0.587f g) + 0.114f b)
//   op 0 brightness blend(c, 0, f) | op 1 contrast blend(c, mean of gray over the image, f) | op 2 saturation blend(c, gray, f) | op 3 hue (below)
// A row is per image, so the order and the factors are wave-uniform: scalar loads, one uniform branch per slot.  The slots are the OUTER loop and a
// thread's four pixels the inner, unrolled one: each op's code exists once per pixel, and the four independent chains hide the latency of the
// divisions (hue: 3 by 255, 4 in rgb2hsv, 1 by 6 per pixel, each ~10 VALU instructions with one quarter-rate v_rcp_f32).
struct AugPx { float c0, c1, c2; };                       // one pixel: three bytes as fp32 (whole numbers), or the final [0, 1] values

// 0 = invalid, 1 = valid, 2 = valid and runs contrast (ids in {-1, 0..3}, none twice; factors 0..2 finite and >= 0; hue in [-0.5, 0.5])
__host__ __device__ inline int aug_jitter_state(const ys_aug_jitter& J) {
  int seen = 0;
  for (int k = 0; k < 4; k++) {
    const int id = J.order[k];
    if (id == -1) continue;
    if (id < 0 || id > 3 || ((seen >> id) & 1)) return 0;
    seen |= 1 << id;
  }
  for (int k = 0; k < 3; k++)
    if (!(J.factor[k] >= 0.0f && J.factor[k] <= 3.402823466e38f)) return 0;
  if (!(J.factor[3] >= -0.5f && J.factor[3] <= 0.5f)) return 0;
  return (seen & 2) ? 2 : 1;
}

__device__ __forceinline__ float aug_jit_blend(float a, float b, float f, float g) {
  const float v = f * a + g * b;
  return truncf(fminf(fmaxf(v, 0.0f), 255.0f));
}

__device__ __forceinline__ float aug_jit_gray(const AugPx& p) { return truncf((0.2989f * p.c0 + 0.587f * p.c1) + 0.114f * p.c2); }

// adjust_hue on a byte pixel: / 255, _rgb2hsv, (h + f) mod 1, _hsv2rgb, trunc(v * 255.999f).  Selects where torchvision multiplies by masks: the terms
// it masks out are finite, so they add +-0 and the sum is the selected term.  fmod(x, 1) = x - trunc(x) (exact below 2^23).
__device__ __forceinline__ void aug_jit_hue(float f, AugPx& px) {
  const float r = px.c0 / 255.0f, g = px.c1 / 255.0f, b = px.c2 / 255.0f;
  const float maxc = fmaxf(fmaxf(r, g), b), minc = fminf(fminf(r, g), b);
  const bool eqc = maxc == minc;
  const float cr = maxc - minc;
  const float s = cr / (eqc ? 1.0f : maxc);
  const float d = eqc ? 1.0f : cr;
  const float rc = (maxc - r) / d, gc = (maxc - g) / d, bc = (maxc - b) / d;
  float h = maxc == r ? bc - gc : (maxc == g ? (2.0f + rc) - bc : (4.0f + gc) - rc);
  h = h / 6.0f + 1.0f;                                     // in [5/6, 11/6]
  h = h - truncf(h);                                       // fmod(.., 1)
  h = h + f;
  h = h - truncf(h);                                       // the Python-style remainder: fmod, then + 1 where the result is negative
  h = h < 0.0f ? h + 1.0f : h;                             // (can round to exactly 1: i = 6 below)
  const float h6 = h * 6.0f, fi = floorf(h6), ff = h6 - fi;
  int i = (int)fi;
  i = i >= 6 ? i - 6 : i;
  const float v = maxc;
  const float p = fminf(fmaxf(v * (1.0f - s), 0.0f), 1.0f);
  const float q = fminf(fmaxf(v * (1.0f - s * ff), 0.0f), 1.0f);
  const float t = fminf(fmaxf(v * (1.0f - (s * (1.0f - ff))), 0.0f), 1.0f);
  const float R = i == 0 ? v : (i == 1 ? q : (i == 2 ? p : (i == 3 ? p : (i == 4 ? t : v))));
  const float G = i == 0 ? t : (i == 1 ? v : (i == 2 ? v : (i == 3 ? q : p)));
  const float B = i == 0 ? p : (i == 1 ? p : (i == 2 ? t : (i == 3 ? v : (i == 4 ? v : q))));
  px.c0 = truncf(R * 255.999f); px.c1 = truncf(G * 255.999f); px.c2 = truncf(B * 255.999f);   // convert_image_dtype: max + 1 - 1e-3, truncated
}

// the ops of one VALID row on a thread's four pixels, in the row's order; until_contrast: stop in front of op 1 (the reduction's replay)
__device__ __forceinline__ void aug_jitter_quad(const ys_aug_jitter* __restrict__ J, float mean, bool until_contrast, AugPx& p0, AugPx& p1, AugPx& p2,
                                                AugPx& p3) {
#pragma unroll 1
  for (int k = 0; k < 4; k++) {
    const int id = J->order[k];                            // wave-uniform
    if (id < 0) continue;
    if (id == 1 && until_contrast) break;
    const float f = J->factor[id];
    if (id == 3) {
      aug_jit_hue(f, p0); aug_jit_hue(f, p1); aug_jit_hue(f, p2); aug_jit_hue(f, p3);
    } else {
      const float g = 1.0f - f;
      float o0 = 0.0f, o1 = 0.0f, o2 = 0.0f, o3 = 0.0f;
      if (id == 2) { o0 = aug_jit_gray(p0); o1 = aug_jit_gray(p1); o2 = aug_jit_gray(p2); o3 = aug_jit_gray(p3); }
      else if (id == 1) { o0 = mean; o1 = mean; o2 = mean; o3 = mean; }
      p0.c0 = aug_jit_blend(p0.c0, o0, f, g); p0.c1 = aug_jit_blend(p0.c1, o0, f, g); p0.c2 = aug_jit_blend(p0.c2, o0, f, g);
      p1.c0 = aug_jit_blend(p1.c0, o1, f, g); p1.c1 = aug_jit_blend(p1.c1, o1, f, g); p1.c2 = aug_jit_blend(p1.c2, o1, f, g);
      p2.c0 = aug_jit_blend(p2.c0, o2, f, g); p2.c1 = aug_jit_blend(p2.c1, o2, f, g); p2.c2 = aug_jit_blend(p2.c2, o2, f, g);
      p3.c0 = aug_jit_blend(p3.c0, o3, f, g); p3.c1 = aug_jit_blend(p3.c1, o3, f, g); p3.c2 = aug_jit_blend(p3.c2, o3, f, g);
    }
  }
}
