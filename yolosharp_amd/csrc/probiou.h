// probiou.h -- Metrics.batch_probiou's two device functions, shared by nms.hip (nms_rot_removed_kernel, probiou_kernel) and valmetrics.hip
// (val_match_rot_kernel).  Both units are compiled with -ffp-contract=off (build.py NO_CONTRACT), so these round identically in either:
// val_match_rot_kernel's `correct` equals ys_batch_probiou + ys_match_predictions per image bit for bit.  A unit that includes this header belongs in
// that set.
#pragma once
#include "ys_hip.h"

// Metrics.batch_probiou (Metrics.cs:223-258), operation for operation in fp32: box 1 = (x1, y1, a1, b1, c1), box 2 likewise
__device__ inline float nms_probiou(float x1, float y1, float a1, float b1, float c1, float x2, float y2, float a2, float b2, float c2, float eps) {
  const float sa = a1 + a2, sb = b1 + b2, sc = c1 + c2;
  const float dy = y1 - y2, dx = x1 - x2;
  const float det = sa * sb - sc * sc;
  const float t1 = ((sa * (dy * dy) + sb * (dx * dx)) / (det + eps)) * 0.25f;
  const float t2 = ((sc * (x2 - x1) * dy) / (det + eps)) * 0.5f;
  const float d1 = fmaxf(a1 * b1 - c1 * c1, 0.f), d2 = fmaxf(a2 * b2 - c2 * c2, 0.f);
  const float t3 = logf(det / (4.0f * sqrtf(d1 * d2) + eps) + eps) * 0.5f;
  float bd = t1 + t2 + t3;
  bd = fminf(fmaxf(bd, eps), 100.0f);
  const float hd = sqrtf(1.0f - expf(-bd) + eps);
  return 1.0f - hd;
}

// covariance terms of an oriented box (cx, cy, w, h, angle) -- _get_covariance_matrix (Metrics.cs:260-276), operation for operation in fp32
__device__ inline void nms_obb_cov(const float* q, float& a, float& b, float& c) {
  const float ga = q[2] * q[2] / 12.0f, gb = q[3] * q[3] / 12.0f;
  const float cs = cosf(q[4]), sn = sinf(q[4]);
  const float cos2 = cs * cs, sin2 = sn * sn;
  a = ga * cos2 + gb * sin2; b = ga * sin2 + gb * cos2; c = (ga - gb) * cs * sn;
}
