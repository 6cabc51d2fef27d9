// aug_aa.h -- what augment_aa.hip (the AutoAugment / RandAugment operators) and augment_cls.hip (the classification chain that runs them between its flips
// and its erase) share: the op ids of a ys_aa_row, the rule that makes a row valid, and the per-image statistics row of a slot.
#pragma once
#include "ys_internal.h"
#include "ys_kernels.h"

// torchvision's _augmentation_space order; -1 = nothing (the slot's probability draw failed, or RandAugment's Identity)
enum { AA_NONE = -1, AA_SHEAR_X = 0, AA_SHEAR_Y = 1, AA_TRANSLATE_X = 2, AA_TRANSLATE_Y = 3, AA_ROTATE = 4, AA_BRIGHTNESS = 5, AA_COLOR = 6, AA_CONTRAST = 7,
       AA_SHARPNESS = 8, AA_POSTERIZE = 9, AA_SOLARIZE = 10, AA_AUTOCONTRAST = 11, AA_EQUALIZE = 12, AA_INVERT = 13 };

// what a slot's statistics launch leaves for its apply launch: the 256-bin histogram of each channel (AutoContrast, Equalize) and the sum of the gray
// bytes (Contrast) of the image in its state in front of the slot.  Zeroed by the caller; integer atomics, so any arrival order gives the same row.
struct AaStats { unsigned hist[3][256]; unsigned long long gray; };

__host__ __device__ inline int aug_aa_finite(float v) { return v >= -3.402823466e38f && v <= 3.402823466e38f; }

// op ids in -1 .. 13, every arg and theta entry finite, Posterize bits in 0 .. 8 (include/yolosharp_hip.h lists the same rules)
__host__ __device__ inline int aug_aa_row_ok(const ys_aa_row& r) {
  for (int k = 0; k < 2; k++) {
    if (r.op[k] < AA_NONE || r.op[k] > AA_INVERT || !aug_aa_finite(r.arg[k])) return 0;
    for (int i = 0; i < 6; i++)
      if (!aug_aa_finite(r.theta[k][i])) return 0;
    if (r.op[k] == AA_POSTERIZE && !(r.arg[k] >= 0.0f && r.arg[k] <= 8.0f)) return 0;
  }
  return 1;
}

__host__ __device__ inline int aug_aa_needs_stats(int op) { return op == AA_CONTRAST || op == AA_AUTOCONTRAST || op == AA_EQUALIZE; }
