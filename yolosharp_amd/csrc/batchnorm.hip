// batchnorm.hip -- the BatchNorm2d(eps 1e-3, momentum 0.03) + SiLU training passes around the convolutions (gfx950; Modules/Convs.cs:36-62).
//   forward   statistics finalize, eval coefficients, apply (+ fp8 image: q8), finalize-inside-apply
//   backward  per-channel reductions over rows (also the plain column sums of the bias gradients), finalize, apply (+ q8)
//   grouped   the same passes for several independent Conv units in one launch
// The arithmetic is bn_math.h; a kernel here is the launch shape (indexing, loads, stores) around it.  Each single / grouped pair is one
// body and two thin __global__ wrappers.  All tensors are [rows][ldc] views with a channel offset; one thread moves 16 bytes (8 bf16 / 4 f32).
#include "ys_internal.h"
#include "bn_math.h"

#define EW_THREADS 256

// ------------------------------------------------------------------ BN forward finalize
// one workgroup per channel: deterministic sum of the conv epilogue's partials in double
__device__ __forceinline__ void bn_finalize_body(const float* partial, int nblk, int C, int c, double count, const float* gamma,
                                                 const float* beta, float eps, float momentum, float* run_mean,
                                                 float* run_var, float* nbt, float* scale,
                                                 float* shift, float* mean_o, float* rstd_o) {
  __shared__ double sbuf[EW_THREADS];
  // per-channel operands of the tail are fetched first: their latency overlaps the partial loads instead of forming a second
  // dependent round trip after the reduction
  float g = 0.f, bt = 0.f, rm0 = 0.f, rv0 = 0.f, nbt0 = 0.f;
  if (threadIdx.x == 0) { g = gamma[c]; bt = beta[c]; rm0 = run_mean[c]; rv0 = run_var[c]; if (c == 0 && nbt) nbt0 = nbt[0]; }
  double s1, s2;
  bn_partial_sum<EW_THREADS>(partial, nblk, C, c, s1, s2, sbuf);
  if (threadIdx.x == 0) {
    const BnFwdCoef k = bn_fwd_coeffs(s1, s2, count, eps, g, bt);
    scale[c] = k.scale;
    shift[c] = k.shift;
    mean_o[c] = (float)k.mean;
    rstd_o[c] = k.rstd;
    bn_running_update<true>(k, count, momentum, c, run_mean, run_var, nbt, rm0, rv0, nbt0);
  }
}
__global__ void __launch_bounds__(EW_THREADS)
bn_finalize_kernel(const float* __restrict__ partial, int nblk, int C, double count, const float* __restrict__ gamma,
                   const float* __restrict__ beta, float eps, float momentum, float* __restrict__ run_mean,
                   float* __restrict__ run_var, float* __restrict__ nbt, float* __restrict__ scale,
                   float* __restrict__ shift, float* __restrict__ mean_o, float* __restrict__ rstd_o) {
  bn_finalize_body(partial, nblk, C, blockIdx.x, count, gamma, beta, eps, momentum, run_mean, run_var, nbt, scale, shift, mean_o, rstd_o);
}
int ys_bn_finalize_launch(hipStream_t st, const float* partial, int nblk, int C, long count, const float* gamma,
                          const float* beta, float eps, float momentum, float* run_mean, float* run_var, float* nbt,
                          float* scale, float* shift, float* mean, float* rstd) {
  YS_LAUNCH(bn_finalize_kernel, C, EW_THREADS, st, partial, nblk, C, (double)count, gamma, beta, eps, momentum,
            run_mean, run_var, nbt, scale, shift, mean, rstd);
  return YS_OK;
}

__global__ void __launch_bounds__(EW_THREADS)
bn_eval_coeffs_kernel(int C, const float* __restrict__ gamma, const float* __restrict__ beta,
                      const float* __restrict__ rm, const float* __restrict__ rv, float eps,
                      float* __restrict__ scale, float* __restrict__ shift) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const float rstd = 1.0f / sqrtf(rv[c] + eps);
  scale[c] = gamma[c] * rstd;
  shift[c] = beta[c] - rm[c] * gamma[c] * rstd;
}
int ys_bn_eval_coeffs_launch(hipStream_t st, int C, const float* gamma, const float* beta, const float* rm,
                             const float* rv, float eps, float* scale, float* shift) {
  YS_LAUNCH(bn_eval_coeffs_kernel, ys_cdiv(C, EW_THREADS), EW_THREADS, st, C, gamma, beta, rm, rv, eps, scale, shift);
  return YS_OK;
}

// ------------------------------------------------------------------ BN + act apply (training forward, pass 2)
// one vector of the pass: f <- act(y[row][c ..] * scale + shift) (+ residual view); returns max |f|
template <class T, bool ACT>
__device__ __forceinline__ float bn_act_apply_vec(const T* y, long row, int c, int C, const float* scale, const float* shift, const T* res, int res_ldc,
                                                  int res_coff, float* f) {
  constexpr int EPL = Elem<T>::EPL;
  float r[EPL], sc[EPL], sh[EPL];
  ys_unpack<T>(ys_ld16(y + row * C + c), f);
  if (res) ys_unpack<T>(ys_ld16(res + row * res_ldc + res_coff + c), r);
  ys_ldcoef<EPL>(scale + c, sc);
  ys_ldcoef<EPL>(shift + c, sh);
  return bn_apply_vec<T, ACT>(f, sc, sh, res != nullptr, r);
}
// ACT is a template parameter: a run-time flag inside the unrolled element loop splits it into basic blocks (see chan_reduce);
// rows * CG < 2^31 (every graph here) takes 32-bit index arithmetic instead of a ~80-instruction 64-bit division.
template <class T, bool ACT>
__global__ void __launch_bounds__(EW_THREADS)
bn_act_apply_kernel(const T* __restrict__ y, long rows, int C, const float* __restrict__ scale,
                    const float* __restrict__ shift, const T* __restrict__ res, int res_ldc, int res_coff,
                    T* __restrict__ z, int z_ldc, int z_coff, int small, unsigned* __restrict__ amax) {
  constexpr int EPL = Elem<T>::EPL;
  const int CG = C / EPL;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  float mx = 0.f;
  if (i < rows * CG) {
    long row; int c;
    if (small) { const unsigned iu = (unsigned)i, r = iu / (unsigned)CG; row = r; c = (int)(iu - r * (unsigned)CG) * EPL; }
    else { row = i / CG; c = (int)(i - row * CG) * EPL; }
    float f[EPL];
    mx = bn_act_apply_vec<T, ACT>(y, row, c, C, scale, shift, res, res_ldc, res_coff, f);
    ys_st16(z + row * z_ldc + z_coff + c, ys_pack<T>(f));
  }
  // fp8 mode: amax(|z|) of the tensor this pass writes feeds the NEXT step's activation scale (delayed scaling, f8.hip); the
  // maximum of non-negative floats is order-independent, so the atomic keeps the step deterministic
  if (amax) ys_amax_update(amax, mx);
}
// (row, channel vector) of a grid-stride pass over rows x CG vectors.  The thread's first vector is divided once; every further trip adds the launch-constant
// stride as (quotient, remainder) of CG with a carry, so no division is left inside the loop (it was a 64-bit division by a run-time value per 16-byte vector).
// I = unsigned where rows * CG < 2^31 (the launcher's `small`; i + stride stays below 2^32: the bounded grid's stride is 2^19 vectors), long otherwise.
template <class I>
struct EwWalk {
  I i, n, row, step, qs;
  int cv, rs, CG;
  __device__ EwWalk(long rows, int CG_) : CG(CG_) {
    n = (I)(rows * CG_);
    i = (I)blockIdx.x * (I)EW_THREADS + (I)threadIdx.x;
    step = (I)gridDim.x * (I)EW_THREADS;
    row = i / (I)CG_; cv = (int)(i - row * (I)CG_);
    qs = step / (I)CG_; rs = (int)(step - qs * (I)CG_);
  }
  __device__ bool more() const { return i < n; }
  __device__ void next() {
    i += step; row += qs; cv += rs;
    if (cv >= CG) { cv -= CG; row += 1; }
  }
};
// amax bookkeeping of a grid-stride pass: workgroup maximum through LDS, then ONE slot update per workgroup
__device__ inline void ys_amax_update_wg(unsigned* slots, float mx) {
  __shared__ float s_wmax[EW_THREADS / 64];
  mx = ys_wave_max(mx);
  if ((threadIdx.x & 63) == 0) s_wmax[threadIdx.x >> 6] = mx;
  __syncthreads();
  if (threadIdx.x == 0) {
    float v = s_wmax[0];
    for (int w = 1; w < EW_THREADS / 64; w++) v = fmaxf(v, s_wmax[w]);
    if (v > 0.f) {
      unsigned* slot = slots + (blockIdx.x & (YS_AMAX_WAYS - 1));
      const unsigned cur = *(volatile unsigned*)slot;
      if (ys_f2u(v) > cur) atomicMax(slot, ys_f2u(v));
    }
  }
}
// the fp8 image of a vector the pass just stored as `pk`: the stored (bf16-rounded) value is quantised -- what every other reader of the
// tensor sees; mx = max(mx, |values|)
template <int BF8>
__device__ __forceinline__ void bn_q8_store(const uint4& pk, float qs, unsigned char* q8p, float& mx) {
  float f[8];
  ys_unpack<bf16_t>(pk, f);
#pragma unroll
  for (int e = 0; e < 8; e++) { mx = fmaxf(mx, fabsf(f[e])); f[e] *= qs; }
  *(uint2*)q8p = ys_pack_f8x8<BF8>(f);
}

// fp8 mode, bf16 storage: the same pass also writes the e4m3 image (dense [rows][C], the consumer's delayed activation scale) of the
// tensor it produces and records amax(|z|) -- used when the next convolution of the schedule reads exactly this
// view and will run the fp8 blocked-GEMM kernel (Bottleneck cv1 -> cv2), instead of a quantisation pass over z.  Grid-stride with a
// bounded grid: one amax atomic per workgroup.
template <bool ACT>
__global__ void __launch_bounds__(EW_THREADS)
bn_act_apply_q8_kernel(const bf16_t* __restrict__ y, long rows, int C, const float* __restrict__ scale, const float* __restrict__ shift,
                       const bf16_t* __restrict__ res, int res_ldc, int res_coff, bf16_t* __restrict__ z, int z_ldc, int z_coff,
                       unsigned char* __restrict__ q8, const float* __restrict__ qscale, int small, unsigned* __restrict__ amax) {
  const int CG = C / 8;
  const float qs = qscale[0];
  float mx = 0.f;
  auto pass = [&](auto w) {
    for (; w.more(); w.next()) {
      const long row = (long)w.row; const int c = w.cv * 8;
      float f[8], r[8], sc[8], sh[8];             // loaded here, not through bn_act_apply_vec: with the arrays inside the helper this loop zero-fills r per trip (+1..3 VGPRs)
      ys_unpack<bf16_t>(ys_ld16(y + row * C + c), f);
      if (res) ys_unpack<bf16_t>(ys_ld16(res + row * res_ldc + res_coff + c), r);
      ys_ldcoef<8>(scale + c, sc);
      ys_ldcoef<8>(shift + c, sh);
      bn_apply_vec<bf16_t, ACT>(f, sc, sh, res != nullptr, r);
      const uint4 pk = ys_pack<bf16_t>(f);
      ys_st16(z + row * z_ldc + z_coff + c, pk);
      bn_q8_store<0>(pk, qs, q8 + row * C + c, mx);
    }
  };
  if (small) pass(EwWalk<unsigned>(rows, CG)); else pass(EwWalk<long>(rows, CG));
  if (amax) ys_amax_update_wg(amax, mx);
}
// bounded grid of the grid-stride passes: `per` vectors per thread, at most 2048 workgroups
static int bounded_grid(long n, long per) {
  const long gcap = 2048;
  long g = ys_cdiv(n, EW_THREADS * per); if (g > gcap) g = gcap; if (g < 1) g = 1;
  return (int)g;
}
int ys_bn_act_apply_q8_launch(hipStream_t st, const void* y, long rows, int C, const float* scale, const float* shift, int act,
                              const void* res, int res_ldc, int res_coff, void* z, int z_ldc, int z_coff, void* q8,
                              const float* qscale, unsigned* amax) {
  const long n = rows * (C / 8);
  const int g = bounded_grid(n, 4);
  const int small = n < (1L << 31) ? 1 : 0;
  YS_DISPATCH_ACT(act, YS_LAUNCH((bn_act_apply_q8_kernel<AF>), g, EW_THREADS, st, (const bf16_t*)y, rows, C, scale, shift, (const bf16_t*)res,
                                 res_ldc, res_coff, (bf16_t*)z, z_ldc, z_coff, (unsigned char*)q8, qscale, small, amax));
  return YS_OK;
}

int ys_bn_act_apply_launch(hipStream_t st, int dtype, const void* y, long rows, int C, const float* scale,
                           const float* shift, int act, const void* res, int res_ldc, int res_coff, void* z,
                           int z_ldc, int z_coff, unsigned* amax) {
  const int epl = dtype == YS_BF16 ? 8 : 4;
  const long n = rows * (C / epl);
  const int small = n < (1L << 31) ? 1 : 0;
  YS_DISPATCH_T_ACT(dtype, act, YS_LAUNCH((bn_act_apply_kernel<TT, AF>), ys_cdiv(n, EW_THREADS), EW_THREADS, st, (const TT*)y, rows, C, scale, shift,
                                          (const TT*)res, res_ldc, res_coff, (TT*)z, z_ldc, z_coff, small, amax));
  return YS_OK;
}

// ------------------------------------------------------------------ BN finalize + apply in one pass (round 5)
// The convolution left the unit's batch statistics as fixed-point integer sums (ys_stat_acc_add: 64-bit atomics, YS_STAT_SHARDS copies).  Every workgroup adds the
// copies and does bn_finalize_kernel's arithmetic for all C channels itself (same integers in, same double arithmetic: the same coefficients in every workgroup, no
// hand-off between workgroups) into LDS; workgroup 0 also stores scale / shift / mean / rstd for the backward pass and updates the running statistics.  Grid-stride
// with a bounded grid so that the C-channel prologue is paid ~2 thousand times per launch, not once per 256 vectors.  The separate bn_finalize launch (4.9 us + a
// kernel boundary, 45 per YOLOv8n step) goes.
template <class T, bool ACT>
__global__ void __launch_bounds__(EW_THREADS)
bn_fin_apply_kernel(const T* __restrict__ y, long rows, int C, BnAccFin f, const T* __restrict__ res, int res_ldc, int res_coff,
                    T* __restrict__ z, int z_ldc, int z_coff, int small) {
  constexpr int EPL = Elem<T>::EPL;
  YS_DYN_LDS(lds);
  float* s_sc = (float*)lds;                   // [C] scale, [C] shift
  float* s_sh = s_sc + C;
  for (int c = threadIdx.x; c < C; c += EW_THREADS) {
    double s1, s2;
    const bool poisoned = bn_acc_sums(f.acc, C, c, s1, s2);
    const BnFwdCoef k = bn_fwd_coeffs(s1, s2, f.count, f.eps, f.gamma[c], f.beta[c], poisoned);
    s_sc[c] = k.scale; s_sh[c] = k.shift;
    if (blockIdx.x == 0) {
      f.scale[c] = k.scale; f.shift[c] = k.shift; f.mean[c] = (float)k.mean; f.rstd[c] = k.rstd;
      bn_running_update<false>(k, f.count, f.momentum, c, f.run_mean, f.run_var, f.nbt);
    }
  }
  __syncthreads();
  const int CG = C / EPL;
  auto pass = [&](auto w) {
    for (; w.more(); w.next()) {
      const long row = (long)w.row; const int c = w.cv * EPL;
      float v[EPL], r[EPL];
      ys_unpack<T>(ys_ld16(y + row * C + c), v);
      if (res) ys_unpack<T>(ys_ld16(res + row * res_ldc + res_coff + c), r);
      bn_apply_vec<T, ACT>(v, s_sc + c, s_sh + c, res != nullptr, r);
      ys_st16(z + row * z_ldc + z_coff + c, ys_pack<T>(v));
    }
  };
  if (small) pass(EwWalk<unsigned>(rows, CG)); else pass(EwWalk<long>(rows, CG));
}
int ys_bn_fin_apply_launch(hipStream_t st, int dtype, const void* y, long rows, int C, const BnAccFin& f, int act, const void* res, int res_ldc, int res_coff,
                           void* z, int z_ldc, int z_coff) {
  const long n = rows * (C / (dtype == YS_BF16 ? 8 : 4));
  const int g = bounded_grid(n, 2);
  const int small = n < (1L << 31) ? 1 : 0;
  const size_t lds = (size_t)2 * C * sizeof(float);
  YS_DISPATCH_T_ACT(dtype, act, YS_LAUNCH_LDS((bn_fin_apply_kernel<TT, AF>), g, EW_THREADS, lds, st, (const TT*)y, rows, C, f, (const TT*)res, res_ldc,
                                              res_coff, (TT*)z, z_ldc, z_coff, small));
  return YS_OK;
}

// ------------------------------------------------------------------ per-channel reductions over rows
// thread t owns channel vector cv = t % CG and row lane t / CG; workgroup blk owns a contiguous row range.
// MODE 0: BN backward (sum du, sum du*xhat), optional res_grad += dz.   MODE 1: plain column sum.
constexpr int CR_U = 2;   // rows per software-pipelined trip of chan_reduce_kernel
template <class T, int MODE, bool RG = false, bool ACT = false>
__global__ void __launch_bounds__(EW_THREADS)
chan_reduce_kernel(const T* __restrict__ dz, int dz_ldc, int dz_coff, const T* __restrict__ y, long rows, int C,
                   const float* __restrict__ scale, const float* __restrict__ shift, const float* __restrict__ mean,
                   const float* __restrict__ rstd, int act, T* __restrict__ rg, int rg_ldc, int rg_coff,
                   float* __restrict__ partial, long rpb, long bstride) {
  constexpr int EPL = Elem<T>::EPL;
  constexpr int NV = MODE == 1 ? EPL : 2 * EPL;          // running sums per thread
  __shared__ float sAcc[NV][EW_THREADS];                 // [value][thread]: conflict-free for consecutive threads
  const int CG = C / EPL;
  const int RP = EW_THREADS / CG;  // rows per pass
  const int tid = threadIdx.x;
  const int cv = tid % CG, rl = tid / CG;
  const int c = cv * EPL;
  const long rows_per_blk = (rows + gridDim.x - 1) / gridDim.x;
  const long r0 = (long)blockIdx.x * rows_per_blk;
  long r1 = r0 + rows_per_blk;
  if (r1 > rows) r1 = rows;
  float a1[EPL], a2[EPL];
#pragma unroll
  for (int e = 0; e < EPL; e++) { a1[e] = 0.f; a2[e] = 0.f; }
  if (rl < RP) {
    // the second BN-backward sum is accumulated against the raw conv output (sum du*y); chan_finalize turns it into
    // sum du*xhat = rstd * (sum du*y - mean * sum du) in double.  Keeping mean / rstd out of the loop saves 16 VGPRs per
    // thread (occupancy 3 -> 5 waves per SIMD), which is what this latency-bound pass needs.
    float sc[EPL], sh[EPL];
    if (MODE == 0) { ys_ldcoef<EPL>(scale + c, sc); ys_ldcoef<EPL>(shift + c, sh); }
    // Software-pipelined over trips of U rows: the loads of trip t+1 are issued before the arithmetic of trip t.  The SiLU
    // derivative is ~18 VALU issue slots per element, i.e. about as long as the HBM latency of a trip; without the
    // prefetch every wave of a SIMD alternates in step between "all waiting" and "all computing" and the two never overlap.
    constexpr int U = CR_U;
    const bool dense = MODE != 1 || rpb == rows;         // no per-image row stride (always for the BN passes): skip the 64-bit division
    const long step = (long)RP * U;
    auto issue = [&](long rowb, uint4 (&gv)[U], uint4 (&fv)[U], uint4 (&ov)[U]) {
#pragma unroll
      for (int k = 0; k < U; k++) {
        // rows past the end are clamped to the last row and ignored by consume(): loads inside exec-masked branches make the
        // compiler fall back to s_waitcnt vmcnt(0) at the join, which would wait for the prefetch as well
        long row = rowb + (long)k * RP;
        row = row < r1 ? row : r1 - 1;
        long zrow = row;
        if (!dense) { const long zb = row / rpb; zrow = zb * bstride + (row - zb * rpb); }   // dz rows strided per image (head outputs)
        gv[k] = ys_ld16(dz + zrow * dz_ldc + dz_coff + c);
        if (MODE == 0) {
          fv[k] = ys_ld16(y + row * C + c);
          if (RG) ov[k] = ys_ld16(rg + row * rg_ldc + rg_coff + c);
        } else { fv[k] = ys_zero16(); }
        if (!RG) ov[k] = ys_zero16();
      }
    };
    auto consume = [&](long rowb, const uint4 (&gv)[U], const uint4 (&fv)[U], const uint4 (&ov)[U]) {
#pragma unroll
      for (int k = 0; k < U; k++) {
        const long row = rowb + (long)k * RP;
        if (row >= r1) continue;
        float g[EPL];
        ys_unpack<T>(gv[k], g);
        if (MODE == 0) {
          float f[EPL];
          ys_unpack<T>(fv[k], f);
          if (RG) bn_rg_add<T>(rg + row * rg_ldc + rg_coff + c, ov[k], g);
#pragma unroll
          for (int e = 0; e < EPL; e++) {
            const float du = bn_du1(g[e], f[e], sc[e], sh[e], ACT);   // compile-time: a run-time flag here splits the unrolled
            a1[e] += du;                                            // elements into basic blocks and serialises the exp/rcp chains
            a2[e] += du * f[e];
          }
        } else if (MODE == 2) {
#pragma unroll
          for (int e = 0; e < EPL; e++) { a1[e] += g[e]; a2[e] += g[e] * g[e]; }
        } else {
#pragma unroll
          for (int e = 0; e < EPL; e++) a1[e] += g[e];
        }
      }
    };
    uint4 gA[U], fA[U], oA[U], gB[U], fB[U], oB[U];
    long rowb = r0 + rl;
    if (rowb < r1) {
      issue(rowb, gA, fA, oA);
      while (true) {                                     // two trips per iteration: the buffers alternate without dynamic indexing
        issue(rowb + step, gB, fB, oB);                  // (unconditional: past the end it re-reads the last row)
        consume(rowb, gA, fA, oA);
        rowb += step;
        if (rowb >= r1) break;
        issue(rowb + step, gA, fA, oA);
        consume(rowb, gB, fB, oB);
        rowb += step;
        if (rowb >= r1) break;
      }
    }
  }
  // workgroup reduction over the RP row lanes: pairwise halving with every thread taking part (the previous form -- CG threads
  // each walking RP rows -- was a serial chain of up to 2048 LDS reads per workgroup for the 16-channel layers)
#pragma unroll
  for (int e = 0; e < EPL; e++) { sAcc[e][tid] = a1[e]; if (MODE != 1) sAcc[EPL + e][tid] = a2[e]; }
  __syncthreads();
  for (int n = RP; n > 1;) {
    const int half = (n + 1) >> 1;
    if (rl + half < n) {
#pragma unroll
      for (int v = 0; v < NV; v++) sAcc[v][tid] += sAcc[v][tid + half * CG];
    }
    __syncthreads();
    n = half;
  }
  if (tid < CG) {
#pragma unroll
    for (int e = 0; e < EPL; e++) {
      partial[((long)blockIdx.x * 2 + 0) * C + c + e] = sAcc[e][tid];
      partial[((long)blockIdx.x * 2 + 1) * C + c + e] = MODE != 1 ? sAcc[(MODE != 1 ? EPL : 0) + e][tid] : 0.f;
    }
  }
}

static int reduce_blocks(long rows, int C, int epl) {
  const int cg = C / epl;
  const int rp = EW_THREADS / cg;
  // prefer 16 row passes per workgroup, but keep >= 512 workgroups (2 per CU) while a workgroup still has a few trips of
  // work; at most 768 (3 per CU, one resident round at 4-5 waves per SIMD): more partial rows only lengthen the finalize
  // kernel and add a ragged second round (measured: 2048 -> 12.86, 1024 -> 12.77, 768/512 -> 12.75 ms/step)
  const long maxnb = 768, minnb = 512;
  long passes = 16;
  while (passes > 4 && (rows + (long)rp * passes - 1) / ((long)rp * passes) < minnb) passes >>= 1;
  long nb = (rows + (long)rp * passes - 1) / ((long)rp * passes);
  if (nb > maxnb) nb = maxnb;
  if (nb < 1) nb = 1;
  return (int)nb;
}
int ys_colsum_blocks(long rows, int C, int dtype) { return reduce_blocks(rows, C, dtype == YS_BF16 ? 8 : 4); }

int ys_bn_bwd_reduce_launch(hipStream_t st, int dtype, const void* dz, int dz_ldc, int dz_coff, const void* y, long rows,
                            int C, const float* scale, const float* shift, const float* mean, const float* rstd,
                            int act, void* res_grad, int rg_ldc, int rg_coff, float* partial, int* nblk_out) {
  const int epl = dtype == YS_BF16 ? 8 : 4;
  if (C % epl || C / epl > EW_THREADS) { ys_set_error("bn_bwd: unsupported channel count %d", C); return YS_ERR_UNSUPPORTED; }
  const int nb = reduce_blocks(rows, C, epl);
  *nblk_out = nb;
#define CR_LAUNCH(RGF) \
  YS_DISPATCH_T_ACT(dtype, act, YS_LAUNCH((chan_reduce_kernel<TT, 0, RGF, AF>), nb, EW_THREADS, st, (const TT*)dz, dz_ldc, dz_coff, (const TT*)y, rows, C, scale, shift, \
                                          mean, rstd, act, (TT*)res_grad, rg_ldc, rg_coff, partial, rows, rows))
  if (res_grad) CR_LAUNCH(true); else CR_LAUNCH(false);
#undef CR_LAUNCH
  return YS_OK;
}

// the plain reductions (MODE 1 column sum, MODE 2 sum and sum of squares) of a [rows][ldc] view: no BN operands
template <class T, int MODE>
static void chan_reduce_plain(hipStream_t st, int nb, const void* x, int ldc, int coff, long rows, int C, float* partial, long rpb, long bstride) {
  const float* nof = nullptr;
  YS_LAUNCH((chan_reduce_kernel<T, MODE>), nb, EW_THREADS, st, (const T*)x, ldc, coff, (const T*)nullptr, rows, C, nof, nof, nof, nof, 0, (T*)nullptr, 0, 0, partial, rpb, bstride);
}
// per-channel (sum, sum of squares) partials of a dense [rows][C] tensor (BN statistics of depthwise conv outputs)
int ys_chan_stats_launch(hipStream_t st, int dtype, const void* y, long rows, int C, float* partial, int* nblk_out) {
  const int epl = dtype == YS_BF16 ? 8 : 4;
  if (C % epl || C / epl > EW_THREADS) { ys_set_error("chan_stats: unsupported channel count %d", C); return YS_ERR_UNSUPPORTED; }
  const int nb = reduce_blocks(rows, C, epl);
  *nblk_out = nb;
  if (dtype == YS_BF16) chan_reduce_plain<bf16_t, 2>(st, nb, y, C, 0, rows, C, partial, rows, rows);
  else chan_reduce_plain<float, 2>(st, nb, y, C, 0, rows, C, partial, rows, rows);
  return YS_OK;
}

// one workgroup per channel: sums partials; MODE 0 -> BN grads + coefficients, MODE 1 -> bias grad.
template <int MODE>
__device__ __forceinline__ void chan_finalize_body(const FinSrc& src, int C, int c, double count, float* g0,
                                                   float* g1, float* c1, float* c2,
                                                   const float* scale, const float* mean, const float* rstd) {
  __shared__ double sbuf[EW_THREADS];
  int nblk;
  const float* partial = bn_fin_src_pick(src, c, nblk);
  float sc = 0.f, mu = 0.f, rs = 0.f, g0p = 0.f, g1p = 0.f;   // tail operands first (see bn_finalize_kernel)
  if (threadIdx.x == 0) {
    g0p = g0[c];
    if (MODE == 0) { sc = scale[c]; mu = mean[c]; rs = rstd[c]; g1p = g1[c]; }
  }
  double s1, s2;
  bn_partial_sum<EW_THREADS, MODE == 0>(partial, nblk, C, c, s1, s2, sbuf);
  if (threadIdx.x == 0) {
    if (MODE == 0) {
      const BnBwdCoef k = bn_bwd_coeffs(s1, s2, count, sc, mu, rs);
      g0[c] = g0p + k.dgamma;
      g1[c] = g1p + k.dbeta;
      c1[c] = k.k2;
      c2[c] = k.k3;
    } else {
      g0[c] = g0p + (float)s1;
    }
  }
}
template <int MODE>
__global__ void __launch_bounds__(EW_THREADS)
chan_finalize_kernel(FinSrc src, int C, double count, float* __restrict__ g0,
                     float* __restrict__ g1, float* __restrict__ c1, float* __restrict__ c2,
                     const float* __restrict__ scale, const float* __restrict__ mean, const float* __restrict__ rstd) {
  chan_finalize_body<MODE>(src, C, blockIdx.x, count, g0, g1, c1, c2, scale, mean, rstd);
}
int ys_bn_bwd_finalize_src_launch(hipStream_t st, const FinSrc& src, int C, long count, float* dgamma, float* dbeta, float* c1,
                                  float* c2, const float* scale, const float* mean, const float* rstd) {
  YS_LAUNCH((chan_finalize_kernel<0>), C, EW_THREADS, st, src, C, (double)count, dgamma, dbeta, c1, c2, scale, mean, rstd);
  return YS_OK;
}
int ys_bn_bwd_finalize_launch(hipStream_t st, const float* partial, int nblk, int C, long count, float* dgamma,
                              float* dbeta, float* c1, float* c2, const float* scale, const float* mean, const float* rstd) {
  FinSrc src{}; src.n = 1; src.p[0] = partial; src.nblk[0] = nblk; src.c1[0] = C;
  return ys_bn_bwd_finalize_src_launch(st, src, C, count, dgamma, dbeta, c1, c2, scale, mean, rstd);
}

int ys_colsum_launch(hipStream_t st, int dtype, const void* x, int ldc, int coff, long rows, long rows_per_b,
                     long bstride, int C, float* partial, float* grad) {
  const int epl = dtype == YS_BF16 ? 8 : 4;
  const int Cp = (C + epl - 1) / epl * epl;  // padded channels of the view are zero
  if (Cp / epl > EW_THREADS) { ys_set_error("colsum: unsupported channel count %d", C); return YS_ERR_UNSUPPORTED; }
  const int nb = reduce_blocks(rows, Cp, epl);
  if (dtype == YS_BF16) chan_reduce_plain<bf16_t, 1>(st, nb, x, ldc, coff, rows, Cp, partial, rows_per_b, bstride);
  else chan_reduce_plain<float, 1>(st, nb, x, ldc, coff, rows, Cp, partial, rows_per_b, bstride);
  // partial rows are Cp wide; finalize only the C real channels
  FinSrc src{}; src.n = 1; src.p[0] = partial; src.nblk[0] = nb; src.c1[0] = Cp;
  YS_LAUNCH((chan_finalize_kernel<1>), C, EW_THREADS, st, src, Cp, 1.0, grad, (float*)nullptr, (float*)nullptr, (float*)nullptr, (const float*)nullptr, (const float*)nullptr, (const float*)nullptr);
  return YS_OK;
}

// ------------------------------------------------------------------ BN backward apply (pass 2)
// one vector of the pass: f <- dy[row][c ..] from dz and the raw conv output y; rg: also rg[view] += dz; returns max |dy|
template <class T, bool ACT>
__device__ __forceinline__ float bn_bwd_apply_vec(const T* dz, int dz_ldc, int dz_coff, const T* y, long row, int c, int C,
                                                  const float* scale, const float* shift, const float* k2,
                                                  const float* k3, T* rg, int rg_ldc, int rg_coff, float* f) {
  constexpr int EPL = Elem<T>::EPL;
  float g[EPL], sc[EPL], sh[EPL], a2[EPL], a3[EPL];
  ys_unpack<T>(ys_ld16(dz + row * dz_ldc + dz_coff + c), g);
  ys_unpack<T>(ys_ld16(y + row * C + c), f);
  if (rg) {     // d(residual input) += dz: the Bottleneck shortcut's share, done here when the reduction pass that used to carry it is fused away
    T* rp = rg + row * rg_ldc + rg_coff + c;
    bn_rg_add<T>(rp, ys_ld16(rp), g);
  }
  ys_ldcoef<EPL>(scale + c, sc); ys_ldcoef<EPL>(shift + c, sh); ys_ldcoef<EPL>(k2 + c, a2); ys_ldcoef<EPL>(k3 + c, a3);
  return bn_bwd_vec<T, ACT>(g, f, sc, sh, a2, a3);
}
template <class T, bool ACT>
__global__ void __launch_bounds__(EW_THREADS)
bn_bwd_apply_kernel(const T* __restrict__ dz, int dz_ldc, int dz_coff, const T* __restrict__ y, long rows, int C,
                    const float* __restrict__ scale, const float* __restrict__ shift, const float* __restrict__ k2,
                    const float* __restrict__ k3, T* __restrict__ dy, int small, unsigned* __restrict__ amax,
                    T* __restrict__ rg, int rg_ldc, int rg_coff) {
  constexpr int EPL = Elem<T>::EPL;
  const int CG = C / EPL;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  float mx = 0.f;
  if (i < rows * CG) {
    long row; int c;
    if (small) { const unsigned iu = (unsigned)i, r = iu / (unsigned)CG; row = r; c = (int)(iu - r * (unsigned)CG) * EPL; }
    else { row = i / CG; c = (int)(i - row * CG) * EPL; }
    float f[EPL];
    mx = bn_bwd_apply_vec<T, ACT>(dz, dz_ldc, dz_coff, y, row, c, C, scale, shift, k2, k3, rg, rg_ldc, rg_coff, f);
    ys_st16(dy + row * C + c, ys_pack<T>(f));
  }
  if (amax) ys_amax_update(amax, mx);          // fp8 mode: amax(|dy|) for the next step's gradient scale (f8.hip)
}
// fp8 mode, bf16 storage: the same pass also writes the e5m2 image of dy (dense [rows][C], scaled by the layer's delayed gradient
// scale) that the fp8 dgrad kernel consumes, and records amax(|dy|) for the next step's scale -- instead of a separate quantisation
// pass over dy (f8_quant_view_kernel: 2 B read + 1 B written per element and layer).  Grid-stride with a bounded grid so that the
// amax bookkeeping is one atomic per workgroup (one-shot waves each paying a dependent global round trip were measured 5x slower).
template <bool ACT>
__global__ void __launch_bounds__(EW_THREADS)
bn_bwd_apply_q8_kernel(const bf16_t* __restrict__ dz, int dz_ldc, int dz_coff, const bf16_t* __restrict__ y, long rows, int C,
                       const float* __restrict__ scale, const float* __restrict__ shift, const float* __restrict__ k2,
                       const float* __restrict__ k3, bf16_t* __restrict__ dy, unsigned char* __restrict__ q8,
                       const float* __restrict__ qscale, int small, unsigned* __restrict__ amax, bf16_t* __restrict__ rg, int rg_ldc, int rg_coff) {
  const int CG = C / 8;
  const float qs = qscale[0];
  float mx = 0.f;
  auto pass = [&](auto w) {
    for (; w.more(); w.next()) {
      const long row = (long)w.row; const int c = w.cv * 8;
      float f[8];
      bn_bwd_apply_vec<bf16_t, ACT>(dz, dz_ldc, dz_coff, y, row, c, C, scale, shift, k2, k3, rg, rg_ldc, rg_coff, f);
      const uint4 pk = ys_pack<bf16_t>(f);
      ys_st16(dy + row * C + c, pk);
      bn_q8_store<1>(pk, qs, q8 + row * C + c, mx);   // quantise what the bf16 consumers (wgrad) see: the rounded value
    }
  };
  if (small) pass(EwWalk<unsigned>(rows, CG)); else pass(EwWalk<long>(rows, CG));
  if (amax) ys_amax_update_wg(amax, mx);
}
int ys_bn_bwd_apply_q8_launch(hipStream_t st, const void* dz, int dz_ldc, int dz_coff, const void* y, long rows, int C,
                              const float* scale, const float* shift, const float* k2, const float* k3, int act, void* dy,
                              void* q8, const float* qscale, unsigned* amax, void* rg, int rg_ldc, int rg_coff) {
  const long n = rows * (C / 8);
  const int g = bounded_grid(n, 4);
  const int small = n < (1L << 31) ? 1 : 0;
  YS_DISPATCH_ACT(act, YS_LAUNCH((bn_bwd_apply_q8_kernel<AF>), g, EW_THREADS, st, (const bf16_t*)dz, dz_ldc, dz_coff, (const bf16_t*)y, rows, C, scale, shift,
                                 k2, k3, (bf16_t*)dy, (unsigned char*)q8, qscale, small, amax, (bf16_t*)rg, rg_ldc, rg_coff));
  return YS_OK;
}

int ys_bn_bwd_apply_launch(hipStream_t st, int dtype, const void* dz, int dz_ldc, int dz_coff, const void* y, long rows,
                           int C, const float* scale, const float* shift, const float* k2, const float* k3, int act, void* dy,
                           unsigned* amax, void* rg, int rg_ldc, int rg_coff) {
  const int epl = dtype == YS_BF16 ? 8 : 4;
  const long n = rows * (C / epl);
  const int small = n < (1L << 31) ? 1 : 0;
  YS_DISPATCH_T_ACT(dtype, act, YS_LAUNCH((bn_bwd_apply_kernel<TT, AF>), ys_cdiv(n, EW_THREADS), EW_THREADS, st, (const TT*)dz, dz_ldc, dz_coff, (const TT*)y,
                                          rows, C, scale, shift, k2, k3, (TT*)dy, small, amax, (TT*)rg, rg_ldc, rg_coff));
  return YS_OK;
}

// ------------------------------------------------------------------ grouped (multi-problem) BatchNorm passes
// The BN passes of INDEPENDENT Conv units that the planner runs side by side (the tower layers of the three pyramid levels of a
// head, model.hip run_conv_fwd_group / run_conv_bwd_group) as one launch each: workgroups [end[i-1], end[i]) serve problem i.  The
// P4 / P5 instances are 5-14 us launch-latency-bound kernels on their own; each kernel runs the body of its single-problem kernel
// above on the problem its workgroup serves (bit-identical results).
template <class G> __device__ inline int ys_ew_group_pick(const G& g, int bx, int& start) {
  int pi = 0;
#pragma unroll
  for (int k = 0; k + 1 < YS_EW_GROUP_MAX; k++) pi += (int)(k + 1 < g.n && bx >= g.end[k]);
  start = pi ? g.end[pi - 1] : 0;
  return pi;
}
// host side: grp.p / grp.end from the problem list, blocks(problem) workgroups each (< 0: refused); the launch's grid size in *total
template <class G, class P, class F>
static int group_fill(G& grp, const P* probs, int n, const char* what, F blocks, int* total) {
  if (n < 1 || n > YS_EW_GROUP_MAX) { ys_set_error("%s group: %d problems", what, n); return YS_ERR_INVALID_ARG; }
  grp.n = n;
  long end = 0;
  for (int i = 0; i < n; i++) {
    const long nb = blocks(probs[i]);
    if (nb < 0) { ys_set_error("%s group: problem too large", what); return YS_ERR_UNSUPPORTED; }
    grp.p[i] = probs[i]; end += nb; grp.end[i] = (int)end;
  }
  for (int i = n; i < YS_EW_GROUP_MAX; i++) grp.end[i] = (int)end;
  *total = (int)end;
  return YS_OK;
}
// workgroups of an elementwise problem of `rows` x C: one vector per thread, rows * CG < 2^31 (the grouped kernels index in 32 bits)
static long apply_blocks(long rows, int C, int epl) {
  const long nn = rows * (C / epl);
  return nn >= (1L << 31) ? -1 : ys_cdiv(nn, EW_THREADS);
}

__global__ void __launch_bounds__(EW_THREADS)
bn_finalize_group_kernel(BnFinGroup grp, float eps, float momentum) {
  int start;
  const BnFinProb& p = grp.p[ys_ew_group_pick(grp, (int)blockIdx.x, start)];
  bn_finalize_body(p.partial, p.nblk, p.C, (int)blockIdx.x - start, p.count, p.gamma, p.beta, eps, momentum, p.run_mean, p.run_var, p.nbt, p.scale,
                   p.shift, p.mean, p.rstd);
}
int ys_bn_finalize_group_launch(hipStream_t st, const BnFinProb* probs, int n, float eps, float momentum) {
  BnFinGroup grp{};
  int total;
  YS_TRY(group_fill(grp, probs, n, "bn finalize", [](const BnFinProb& p) { return (long)p.C; }, &total));
  YS_LAUNCH(bn_finalize_group_kernel, total, EW_THREADS, st, grp, eps, momentum);
  return YS_OK;
}

template <class T, bool ACT>
__global__ void __launch_bounds__(EW_THREADS)
bn_act_apply_group_kernel(BnApplyGroup grp) {
  constexpr int EPL = Elem<T>::EPL;
  int start;
  const BnApplyProb& p = grp.p[ys_ew_group_pick(grp, (int)blockIdx.x, start)];
  const int C = p.C, CG = C / EPL;
  const unsigned iu = (unsigned)((int)blockIdx.x - start) * (unsigned)EW_THREADS + threadIdx.x;     // rows * CG < 2^31 (checked by the launcher)
  if ((long)iu < p.rows * CG) {
    const unsigned r = iu / (unsigned)CG;
    const long row = r; const int c = (int)(iu - r * (unsigned)CG) * EPL;
    const T* __restrict__ y = (const T*)p.y; const T* __restrict__ res = (const T*)p.res; T* __restrict__ z = (T*)p.z;
    float f[EPL];
    bn_act_apply_vec<T, ACT>(y, row, c, C, p.scale, p.shift, res, p.res_ldc, p.res_coff, f);
    ys_st16(z + row * p.z_ldc + p.z_coff + c, ys_pack<T>(f));
  }
}
int ys_bn_act_apply_group_launch(hipStream_t st, int dtype, const BnApplyProb* probs, int n, int act) {
  const int epl = dtype == YS_BF16 ? 8 : 4;
  BnApplyGroup grp{};
  int total;
  YS_TRY(group_fill(grp, probs, n, "bn apply", [epl](const BnApplyProb& p) { return apply_blocks(p.rows, p.C, epl); }, &total));
  YS_DISPATCH_T_ACT(dtype, act, YS_LAUNCH((bn_act_apply_group_kernel<TT, AF>), total, EW_THREADS, st, grp));
  return YS_OK;
}

// MODE 0 (BN backward) of chan_finalize_kernel for several units at once
__global__ void __launch_bounds__(EW_THREADS)
chan_finalize_group_kernel(ChanFinGroup grp) {
  int start;
  const ChanFinProb& p = grp.p[ys_ew_group_pick(grp, (int)blockIdx.x, start)];
  chan_finalize_body<0>(p.src, p.C, (int)blockIdx.x - start, p.count, p.g0, p.g1, p.c1, p.c2, p.scale, p.mean, p.rstd);
}
int ys_bn_bwd_finalize_group_launch(hipStream_t st, const ChanFinProb* probs, int n) {
  ChanFinGroup grp{};
  int total;
  YS_TRY(group_fill(grp, probs, n, "bn backward finalize", [](const ChanFinProb& p) { return (long)p.C; }, &total));
  YS_LAUNCH(chan_finalize_group_kernel, total, EW_THREADS, st, grp);
  return YS_OK;
}

template <class T, bool ACT>
__global__ void __launch_bounds__(EW_THREADS)
bn_bwd_apply_group_kernel(BnBwdGroup grp) {
  constexpr int EPL = Elem<T>::EPL;
  int start;
  const BnBwdProb& p = grp.p[ys_ew_group_pick(grp, (int)blockIdx.x, start)];
  const int C = p.C, CG = C / EPL;
  const unsigned iu = (unsigned)((int)blockIdx.x - start) * (unsigned)EW_THREADS + threadIdx.x;
  if ((long)iu < p.rows * CG) {
    const unsigned r = iu / (unsigned)CG;
    const long row = r; const int c = (int)(iu - r * (unsigned)CG) * EPL;
    const T* __restrict__ dz = (const T*)p.dz; const T* __restrict__ y = (const T*)p.y; T* __restrict__ dy = (T*)p.dy; T* __restrict__ rg = (T*)p.rg;
    float f[EPL];
    bn_bwd_apply_vec<T, ACT>(dz, p.dz_ldc, p.dz_coff, y, row, c, C, p.scale, p.shift, p.k2, p.k3, rg, p.rg_ldc, p.rg_coff, f);
    ys_st16(dy + row * C + c, ys_pack<T>(f));
  }
}
int ys_bn_bwd_apply_group_launch(hipStream_t st, int dtype, const BnBwdProb* probs, int n, int act) {
  const int epl = dtype == YS_BF16 ? 8 : 4;
  BnBwdGroup grp{};
  int total;
  YS_TRY(group_fill(grp, probs, n, "bn backward apply", [epl](const BnBwdProb& p) { return apply_blocks(p.rows, p.C, epl); }, &total));
  YS_DISPATCH_T_ACT(dtype, act, YS_LAUNCH((bn_bwd_apply_group_kernel<TT, AF>), total, EW_THREADS, st, grp));
  return YS_OK;
}
