// bn_math.h -- the arithmetic of BatchNorm2d(eps 1e-3, momentum 0.03) + SiLU training (Modules/Convs.cs:36-62), each statement once.
// batchnorm.hip (single, grouped, q8 and finalize-inside-apply kernels) and classify.hip (the pool-fused forms) are launch shapes around
// these functions: "same arithmetic, same order, bit-identical" between them holds because there is one copy.  Everything is
// __forceinline__, so a kernel compiles to what it was with the expressions written out in place.
#pragma once
#include "ys_kernels.h"

// ------------------------------------------------------------------ block reduction helper (double)
// two sums at once: wave shuffles, then one LDS exchange of the NT/64 wave totals combined in a fixed order (the LDS
// tree above costs 9 barriers per value -- most of a ~5 us finalize kernel)
template <int NT>
__device__ __forceinline__ void block_sum2_d(double& a, double& b, double* sbuf) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) { a += __shfl_down(a, off); b += __shfl_down(b, off); }
  if (lane == 0) { sbuf[2 * wave] = a; sbuf[2 * wave + 1] = b; }
  __syncthreads();
  double ta = 0.0, tb = 0.0;
#pragma unroll
  for (int w = 0; w < NT / 64; w++) { ta += sbuf[2 * w]; tb += sbuf[2 * w + 1]; }
  a = ta; b = tb;
}
// one workgroup per channel: deterministic sum of the partial rows [nblk][2][C] of channel c in double (TWO = false: first sum only)
template <int NT, bool TWO = true>
__device__ __forceinline__ void bn_partial_sum(const float* partial, int nblk, int C, int c, double& s1, double& s2, double* sbuf) {
  s1 = 0.0; s2 = 0.0;
  for (int k = threadIdx.x; k < nblk; k += NT) {
    s1 += (double)partial[((long)k * 2 + 0) * C + c];
    if (TWO) s2 += (double)partial[((long)k * 2 + 1) * C + c];
  }
  block_sum2_d<NT>(s1, s2, sbuf);
}
// The partial rows of a channel come from the source that covers it (FinSrc): one source = the channel-reduction pass; several =
// the dgrad launches whose epilogues produced the sums (fused BN-backward reduction, BnRedSeg), each with its own row count.
__device__ __forceinline__ const float* bn_fin_src_pick(const FinSrc& src, int c, int& nblk) {
  const float* partial = src.p[0]; nblk = src.nblk[0];
#pragma unroll
  for (int k = 1; k < YS_BNRED_MAXSEG; k++) if (k < src.n && c >= src.c1[k - 1]) { partial = src.p[k]; nblk = src.nblk[k]; }
  return partial;
}

// ------------------------------------------------------------------ per-channel coefficients
// sum of one channel's fixed-point accumulator copies (ys_stat_acc_add); poisoned: a producer workgroup saw a non-finite / out-of-range partial
__device__ __forceinline__ bool bn_acc_sums(const unsigned long long* acc, int C, int c, double& s1, double& s2) {
  long long a1 = 0, a2 = 0;
  bool poisoned = false;
#pragma unroll
  for (int s = 0; s < YS_STAT_SHARDS; s++) {
    const unsigned long long w2 = acc[((long)s * C + c) * 2 + 1];
    poisoned |= (w2 >> 62) != 0;
    a1 += (long long)acc[((long)s * C + c) * 2 + 0];
    a2 += (long long)w2;
  }
  s1 = (double)a1 * (1.0 / (double)YS_STAT_FIX); s2 = (double)a2 * (1.0 / (double)YS_STAT_FIX);
  return poisoned;
}
struct BnFwdCoef { double mean, var; float rstd, scale, shift; };
// forward: (sum y, sum y^2) over `count` values -> batch statistics and z = y * scale + shift; a poisoned channel gets NaN statistics
__device__ __forceinline__ BnFwdCoef bn_fwd_coeffs(double s1, double s2, double count, float eps, float g, float bt, bool poisoned = false) {
  BnFwdCoef k;
  k.mean = s1 / count;
  k.var = s2 / count - k.mean * k.mean;   // biased (torch BatchNorm2d training normalisation)
  if (k.var < 0.0) k.var = 0.0;
  if (poisoned) { k.mean = __builtin_nan(""); k.var = k.mean; }
  k.rstd = (float)(1.0 / sqrt(k.var + (double)eps));
  k.scale = g * k.rstd;
  k.shift = bt - (float)k.mean * g * k.rstd;
  return k;
}
// running stats: momentum 0.03, unbiased variance (Convs.cs:41-42,48).  PRE: the caller fetched the values before the step
// (rm0 / rv0 / nbt0) ahead of its reduction; otherwise they are read here
template <bool PRE>
__device__ __forceinline__ void bn_running_update(const BnFwdCoef& k, double count, float momentum, int c, float* run_mean, float* run_var, float* nbt,
                                                  float rm0 = 0.f, float rv0 = 0.f, float nbt0 = 0.f) {
  const double unb = count > 1.0 ? k.var * count / (count - 1.0) : k.var;
  run_mean[c] = (1.0f - momentum) * (PRE ? rm0 : run_mean[c]) + momentum * (float)k.mean;
  run_var[c] = (1.0f - momentum) * (PRE ? rv0 : run_var[c]) + momentum * (float)unb;
  if (c == 0 && nbt) nbt[0] = (PRE ? nbt0 : nbt[0]) + 1.0f;
}
struct BnBwdCoef { float dgamma, dbeta, k2, k3; };
// backward: (sum du, sum du*y) -> the dgamma / dbeta increments and the coefficients of dy = scale*du - k2 - y*k3
__device__ __forceinline__ BnBwdCoef bn_bwd_coeffs(double s1, double s2, double count, float sc, float mu, float rs) {
  BnBwdCoef k;
  s2 = (double)rs * (s2 - (double)mu * s1);   // sum(du * xhat) from sum(du * y) (chan_reduce_kernel)
  k.dgamma = (float)s2;  // dgamma += sum(du * xhat)
  k.dbeta = (float)s1;   // dbeta  += sum(du)
  // dy = gamma*rstd*(du - m1 - xhat*m2) = scale*du - k2 - y*k3  (m1 = mean(du), m2 = mean(du*xhat))
  const float m1 = (float)(s1 / count), m2 = (float)(s2 / count);
  k.k2 = sc * (m1 - mu * rs * m2);
  k.k3 = sc * rs * m2;
  return k;
}

// ------------------------------------------------------------------ per-element forms
// `act` is a compile-time constant at every call site that sits in an unrolled element loop (see chan_reduce_kernel)
__device__ __forceinline__ float bn_act1(float y, float sc, float sh, bool act) {
  float u = y * sc + sh;
  if (act) u = ys_silu(u);
  return u;
}
__device__ __forceinline__ float bn_du1(float g, float y, float sc, float sh, bool act) {
  const float u = y * sc + sh;
  return act ? g * ys_silu_grad(u) : g;
}
__device__ __forceinline__ float bn_dy1(float du, float y, float sc, float k2, float k3) { return sc * du - k2 - y * k3; }

// ------------------------------------------------------------------ one 16-byte vector (EPL elements of T)
// f <- act(f * sc + sh) (+ r when res); returns max |f|
template <class T, bool ACT>
__device__ __forceinline__ float bn_apply_vec(float* f, const float* sc, const float* sh, bool res, const float* r) {
  float mx = 0.f;
#pragma unroll
  for (int e = 0; e < Elem<T>::EPL; e++) {
    float u = bn_act1(f[e], sc[e], sh[e], ACT);
    if (res) u += r[e];
    f[e] = u;
    mx = fmaxf(mx, fabsf(u));
  }
  return mx;
}
// f (the raw conv output y) <- dy for the output gradient g; returns max |dy|
template <class T, bool ACT>
__device__ __forceinline__ float bn_bwd_vec(const float* g, float* f, const float* sc, const float* sh, const float* k2, const float* k3) {
  float mx = 0.f;
#pragma unroll
  for (int e = 0; e < Elem<T>::EPL; e++) {
    f[e] = bn_dy1(bn_du1(g[e], f[e], sc[e], sh[e], ACT), f[e], sc[e], k2[e], k3[e]);
    mx = fmaxf(mx, fabsf(f[e]));
  }
  return mx;
}
// d(residual input) += dz: the Bottleneck shortcut's share; `old` is the vector loaded from rp
template <class T>
__device__ __forceinline__ void bn_rg_add(T* rp, const uint4& old, const float* g) {
  float o[Elem<T>::EPL];
  ys_unpack<T>(old, o);
#pragma unroll
  for (int e = 0; e < Elem<T>::EPL; e++) o[e] += g[e];
  ys_st16(rp, ys_pack<T>(o));
}
