// conv.hip -- NHWC implicit-GEMM convolution for gfx950 (CDNA4), forward / dgrad / wgrad.
//
// Replaces the arithmetic of torch.nn.Conv2d inside Modules/Convs.cs:36-62 (Conv = conv2d, bias=False,
// p = k/2) and the plain biased Conv2d heads of Modules/Head.cs:47-50, plus their autograd
// (Amp.cs:348,370).  k in {1,3}, stride in {1,2}, groups = 1.
//
// Layout: activations NHWC (channel stride `ldc`, channel offset `coff` so producers write straight
// into concat buffers and chunk() is a view); weights [Cout][kh][kw][Cin] (K-contiguous per cout).
// GEMM view per launch:  D[cout][pixel] = sum_k W[cout][k] * X[pixel][k],  k = (kh,kw,ci).
// MFMA orientation is "weights as the row operand": a lane ends up with 4 consecutive output
// channels of ONE pixel -> 8-byte (bf16) / 16-byte (f32) NHWC stores, and BN batch statistics
// reduce across lanes with 4 xor-shuffles.
//   T = bf16_t : v_mfma_f32_16x16x32_bf16, one 16-byte fragment load feeds one MFMA (K = 32)
//   T = float  : v_mfma_f32_16x16x4_f32 x4 (exact f32 fma chain) -- the parity path
// Activations stream HBM -> VGPR fragments directly (no reuse across waves: waves split pixels);
// the weight tile of the current tap is staged in LDS once per workgroup and shared by 4 waves.
//
// The same kernel computes dgrad:  ih*DIV = oh*SA + kh - PAD  describes both the forward gather
// (SA = stride, DIV = 1, PAD = k/2) and the input-gradient gather of a strided conv
// (SA = 1, DIV = stride, PAD = k-1-k/2, spatially flipped + transposed weights).
//
// This unit holds the two dtype-generic kernels (direct-fragment and chunked 3x3 patch) with their launchers, and the ROUTE: which of them,
// of conv_p2_kernel (conv_p2.h) and of conv_gemm_kernel / conv_halo_kernel (conv_gemm.hip) runs a convolution -- decided once, in conv_route.
#include "conv_p2.h"
#include <atomic>
#include <cstdlib>

// ------------------------------------------------------------------ shared epilogue
// Lane (li,q) holds acc[mf][nf][r] = D[channel n0+nf*16+4q+r][pixel mf*16+li].  Per pixel fragment the wave rounds its
// 16 x BN tile to T into a wave-private LDS slice and writes it back out as full 16-byte vectors, consecutive lanes
// covering consecutive channels of one pixel row (whole 64-256 B rows per pixel instead of 8-byte fragments); the
// residual add (eval Bottleneck) and gradient accumulation (dgrad into an already written view) happen on that
// wide path.  BN batch statistics are taken from the rounded values in the fragment layout.
template <class T, int MR, int NR, int NW>
__device__ inline void conv_epilogue(const ConvArgs& a, f32x4 (&acc)[MR][NR], const long (&orow)[MR], const bool (&mv)[MR],
                                     int n0, T* wst, float* sStat, long stat_row) {
  constexpr int EPL = Elem<T>::EPL;
  constexpr int BN = NR * 16;
  constexpr int BNP = BN + EPL;        // staging row pitch (elements), rows stay 16-byte aligned
  constexpr int VPP = BN / EPL;        // 16-byte vectors per pixel
  constexpr int NIT = (16 * VPP + 63) / 64;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, q = lane >> 4;
  const bool do_stats = a.stats != nullptr;
  float s1[NR][4], s2[NR][4];
#pragma unroll
  for (int nf = 0; nf < NR; nf++)
#pragma unroll
    for (int r = 0; r < 4; r++) { s1[nf][r] = 0.f; s2[nf][r] = 0.f; }
  char* yb = (char*)a.y;
  const char* rb = (const char*)a.res;
#pragma unroll
  for (int mf = 0; mf < MR; mf++) {
#pragma unroll
    for (int nf = 0; nf < NR; nf++) {
      const int c = n0 + nf * 16 + 4 * q;
      float v[4];
#pragma unroll
      for (int r = 0; r < 4; r++) v[r] = acc[mf][nf][r];
      if (a.scale || a.shift) {
#pragma unroll
        for (int r = 0; r < 4; r++) {
          const int cc = (c + r) < a.Cout ? (c + r) : 0;
          const float sc = a.scale ? a.scale[cc] : 1.0f;
          const float sh = a.shift ? a.shift[cc] : 0.0f;
          v[r] = v[r] * sc + sh;
          if (a.act) v[r] = ys_silu(v[r]);
        }
      }
      T o[4];
#pragma unroll
      for (int r = 0; r < 4; r++) {
        if (c + r >= a.Cout) v[r] = 0.f;     // padded channels of the output row stay zero
        o[r] = Elem<T>::from_f(v[r]);
      }
      if (do_stats && mv[mf]) {
#pragma unroll
        for (int r = 0; r < 4; r++) {
          const float f = Elem<T>::to_f(o[r]);
          s1[nf][r] += f;
          s2[nf][r] += f * f;
        }
      }
      T* wp = wst + li * BNP + nf * 16 + 4 * q;
      if (sizeof(T) == 2) {
        uint2 pk;
        pk.x = ys_pack_bf16x2(v[0], v[1]);
        pk.y = ys_pack_bf16x2(v[2], v[3]);
        *(uint2*)wp = pk;
      } else {
        *(uint4*)wp = make_uint4(ys_f2u(v[0]), ys_f2u(v[1]), ys_f2u(v[2]), ys_f2u(v[3]));
      }
    }
    ys_wave_sync();
    const unsigned rlo = (unsigned)(unsigned long)orow[mf], rhi = (unsigned)((unsigned long)orow[mf] >> 32);
    const int mvi = mv[mf] ? 1 : 0;
#pragma unroll
    for (int it = 0; it < NIT; it++) {
      const int vv = lane + 64 * it;
      const int px = vv < 16 * VPP ? vv / VPP : 0;
      const int cv = vv - px * VPP;
      const unsigned plo = __shfl(rlo, px), phi = __shfl(rhi, px);
      const int pok = __shfl(mvi, px);
      const int c = n0 + cv * EPL;
      if (vv < 16 * VPP && pok && c < a.Cout) {
        const long row = (long)(((unsigned long)phi << 32) | plo);
        uint4 val = *(const uint4*)(wst + px * BNP + cv * EPL);
        T* yp = (T*)(yb + (row * a.out_ldc + a.out_coff + c) * (long)sizeof(T));
        if (rb || a.accumulate) {
          float f[EPL], g[EPL];
          ys_unpack<T>(val, f);
          if (rb) {
            ys_unpack<T>(ys_ld16(rb + (row * a.res_ldc + a.res_coff + c) * (long)sizeof(T)), g);
#pragma unroll
            for (int e = 0; e < EPL; e++) f[e] += g[e];
          }
          if (a.accumulate) {
            ys_unpack<T>(ys_ld16(yp), g);
#pragma unroll
            for (int e = 0; e < EPL; e++) f[e] += g[e];
          }
          val = ys_pack<T>(f);
        }
        ys_st16(yp, val);
      }
    }
    ys_wave_sync();
  }
  if (do_stats) {
#pragma unroll
    for (int nf = 0; nf < NR; nf++)
#pragma unroll
      for (int r = 0; r < 4; r++) {
        float x1 = s1[nf][r], x2 = s2[nf][r];
        for (int msk = 1; msk <= 8; msk <<= 1) {
          x1 += __shfl_xor(x1, msk);
          x2 += __shfl_xor(x2, msk);
        }
        if (li == 0) {
          sStat[((wave * BN) + nf * 16 + 4 * q + r) * 2 + 0] = x1;
          sStat[((wave * BN) + nf * 16 + 4 * q + r) * 2 + 1] = x2;
        }
      }
    __syncthreads();
    if (tid < BN && n0 + tid < a.Cout) {
      float t1 = 0.f, t2 = 0.f;
      for (int w = 0; w < NW; w++) { t1 += sStat[(w * BN + tid) * 2 + 0]; t2 += sStat[(w * BN + tid) * 2 + 1]; }
      if (a.stat_acc) { ys_stat_acc_add(a.stat_acc, stat_row, a.Cout, n0 + tid, 0, t1); ys_stat_acc_add(a.stat_acc, stat_row, a.Cout, n0 + tid, 1, t2); }
      else {
        a.stats[(stat_row * 2 + 0) * a.Cout + n0 + tid] = t1;
        a.stats[(stat_row * 2 + 1) * a.Cout + n0 + tid] = t2;
      }
    }
  }
}

template <class T, int MR, int NR>
__global__ void __launch_bounds__(256)
conv_igemm_kernel(ConvArgs a) {
  constexpr int EPL = Elem<T>::EPL;
  constexpr int BN = NR * 16;
  constexpr int LDS_UNITS = NR <= 2 ? 1024 : 3072;      // 16 / 48 KiB of staged weights
  constexpr int PITCH = ((LDS_UNITS / BN) - 1) | 1;     // odd row pitch in 16-byte units (bank spread)
  constexpr int GSTEPS = PITCH / 4;                     // k-steps whose weights fit in LDS at once
  __shared__ uint4 sW[BN * PITCH];
  __shared__ float sStat[4][BN][2];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int li = lane & 15;
  const int q = lane >> 4;
  const int m0 = blockIdx.x * (4 * MR * 16) + wave * (MR * 16);
  const int n0 = blockIdx.y * BN;
  const int HWo = a.Hout * a.Wout;
  const char* xb = (const char*)a.x;
  const char* wb = (const char*)a.w;
  const int taps = a.KH * a.KW;
  const int Ktot = taps * a.Cin;
  const int cu = a.Cin / EPL;        // 16-byte units per tap
  const int spt = (cu + 3) >> 2;     // k-steps per tap (4 units each, tail predicated off)
  const int total = taps * spt;

  // per m-fragment pixel coordinates of this lane's column (pixel j = li)
  int pb[MR], poh[MR], pow_[MR];
  bool pv[MR];
#pragma unroll
  for (int mf = 0; mf < MR; mf++) {
    const int m = m0 + mf * 16 + li;
    pv[mf] = m < a.M;
    const int mm = pv[mf] ? m : 0;
    const int b = mm / HWo;
    const int r = mm - b * HWo;
    pb[mf] = b;
    poh[mf] = r / a.Wout;
    pow_[mf] = r - poh[mf] * a.Wout;
  }

  f32x4 acc[MR][NR];
#pragma unroll
  for (int mf = 0; mf < MR; mf++)
#pragma unroll
    for (int nf = 0; nf < NR; nf++) acc[mf][nf] = f32x4_zero();

  // ---- activation stream: software-pipelined one k-step ahead (HBM/L2 -> VGPR fragments)
  const char* px[MR];
  bool pvt[MR];
  auto set_tap = [&](int kh, int kw) {
#pragma unroll
    for (int mf = 0; mf < MR; mf++) {
      const int ihn = poh[mf] * a.SA + kh - a.PAD;
      const int iwn = pow_[mf] * a.SA + kw - a.PAD - a.pad_w_delta;
      const int ih = ihn >> a.DIVS, iw = iwn >> a.DIVS;
      const bool ok = pv[mf] && ihn >= 0 && iwn >= 0 && ((ihn | iwn) & a.DIVM) == 0 && ih < a.Hin && iw < a.Win;
      pvt[mf] = ok;
      const long pix = ok ? ((long)pb[mf] * a.in_bstride + (long)ih * a.Win + iw) : 0;
      px[mf] = xb + (pix * a.in_ldc + a.in_coff) * (long)sizeof(T);
    }
  };
  // Loads are issued unconditionally (padding pixels point at pixel 0, a channel tail re-reads channel 0) and masked when the
  // fragment is consumed: a load under an exec mask makes the compiler wait with vmcnt(0) BEFORE the MFMAs of the current step,
  // which serialises the one-step-ahead prefetch with the arithmetic it is meant to hide behind.
  auto load_step = [&](uint4* xf, int s) -> unsigned {
    const int c = (4 * s + q) * EPL;
    const bool cok = c < a.Cin;
    const long cb = (long)(cok ? c : 0) * (long)sizeof(T);
    unsigned okm = 0;
#pragma unroll
    for (int mf = 0; mf < MR; mf++) {
      xf[mf] = ys_ld16(px[mf] + cb);
      okm |= (pvt[mf] && cok) ? (1u << mf) : 0u;
    }
    return okm;
  };
  uint4 xc[MR], xn[MR];
  int ltap = 0, ls = 0, lkh = 0, lkw = 0;   // position of the NEXT load
  set_tap(0, 0);
  {
    const unsigned m0k = load_step(xc, 0);
#pragma unroll
    for (int mf = 0; mf < MR; mf++) if (!((m0k >> mf) & 1u)) xc[mf] = ys_zero16();
  }
  int lt = 0;                                // k-step index inside the staged weight group
  for (int t = 0; t < total; t++) {
    // advance the load position and prefetch step t+1
    ls++;
    if (ls == spt) {
      ls = 0; ltap++; lkw++;
      if (lkw == a.KW) { lkw = 0; lkh++; }
      if (ltap < taps) set_tap(lkh, lkw);
    }
    const unsigned nmask = load_step(xn, ls);   // (past the last step: a harmless re-read)
    if (lt == 0) {
      // stage the weights of k-steps [t, t+GSTEPS) for this workgroup's BN output channels
      __syncthreads();
      const int gs = (total - t) < GSTEPS ? (total - t) : GSTEPS;
      const int gu = gs * 4;
      for (int idx = tid; idx < BN * gu; idx += 256) {
        const int n = idx / gu, lu = idx - n * gu;
        const int tt = t + (lu >> 2);
        const int tp = tt / spt;
        const int c = (((tt - tp * spt) << 2) + (lu & 3)) * EPL;
        uint4 v = ys_zero16();
        if (n0 + n < a.Cout && c < a.Cin)
          v = ys_ld16(wb + ((long)(n0 + n) * Ktot + (long)tp * a.Cin + c) * (long)sizeof(T));
        sW[n * PITCH + lu] = v;
      }
      __syncthreads();
    }
    const int u = 4 * lt + q;
#pragma unroll
    for (int nf = 0; nf < NR; nf++) {
      const uint4 wf = sW[(nf * 16 + li) * PITCH + u];
#pragma unroll
      for (int mf = 0; mf < MR; mf++) acc[mf][nf] = ys_mma<T>(wf, xc[mf], acc[mf][nf]);
    }
#pragma unroll
    for (int mf = 0; mf < MR; mf++) xc[mf] = ((nmask >> mf) & 1u) ? xn[mf] : ys_zero16();
    lt++;
    if (lt == GSTEPS) lt = 0;
  }

  // ------------------------------------------------------------------ epilogue (weights in LDS are dead: reuse as staging)
  __syncthreads();
  long orow[MR];
  bool mvv[MR];
#pragma unroll
  for (int mf = 0; mf < MR; mf++) {
    const int m = m0 + mf * 16 + li;
    mvv[mf] = m < a.M;
    const int mm = mvv[mf] ? m : 0;
    const int bb = mm / HWo;
    const int rr = mm - bb * HWo;
    orow[mf] = a.out_rh ? (long)bb * a.out_bstride + (long)(rr / a.Wout) * a.out_rh + (long)(rr % a.Wout) * a.out_rw + a.out_r0
                        : (long)bb * a.out_bstride + rr;
  }
  T* wst = (T*)sW + wave * (16 * (BN + EPL));
  conv_epilogue<T, MR, NR, 4>(a, acc, orow, mvv, n0, wst, &sStat[0][0][0], (long)blockIdx.x);
}

// ===================================================================================== 3x3: LDS patch kernel
// 3x3 convolutions (forward s1/s2 and dgrad s1/s2) re-use every input pixel up to 9 times.  Instead of fetching the
// operand fragments of each tap from L1/L2 (latency- and TA-bound), one workgroup owns a 2-D output tile TH x TW
// (<= 64*MR pixels) and stages, per 32-channel (bf16) / 16-channel (f32) chunk, the input PATCH = tile + halo once
// in LDS ([PH][PW] pixels x 4 sixteen-byte units, pitch 5 units) together with the chunk's weights of all 9 taps
// ([BN][9*4] units, pitch 37).  All global loads of a chunk are issued back-to-back by the 256 threads (deep
// memory-level parallelism), then the 9 taps x MR x NR MFMAs run from LDS only.  Zero padding and stride-2 dgrad
// holes are handled by zero-filled patch pixels / predicated fragments.
#define PATCH_UNITS 1664
#define C3_THREADS 512
// Persistent variant: grid.x workgroups (about one per CU) walk the tiles; when the weights of this workgroup's BN
// output channels fit in LDS for the whole K range (wres) they are staged ONCE per workgroup, otherwise per chunk.
// The global loads of the next (tile, chunk) are issued into registers before the MFMAs of the current one.
template <class T, int MR, int NR>
__global__ void __launch_bounds__(C3_THREADS)
conv3x3_tile_kernel(ConvArgs a, int ntiles, int nchunks, int wres, int wpitch, int patch_units) {
  constexpr int EPL = Elem<T>::EPL;
  constexpr int BN = NR * 16;
  constexpr int PP = 5;                                     // patch pixel pitch: 4 units + 1
  constexpr int PATCH_DATA = (PATCH_UNITS / PP) * 4;          // data units of the largest patch (pitch 5 holds 4)
  constexpr int NPU = (PATCH_DATA + C3_THREADS - 1) / C3_THREADS;    // patch units fetched per thread
  constexpr int NWU = (BN * 36 + C3_THREADS - 1) / C3_THREADS;       // weight units per thread (non-resident mode)
  YS_DYN_LDS(lds);
  uint4* sW = lds;                                          // [BN][wpitch]
  uint4* sP = lds + BN * wpitch;                            // [PATCH_UNITS]
  float* sStat = (float*)(sP + patch_units);                // [8][BN][2]

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, q = lane >> 4;
  const int n0 = blockIdx.y * BN;
  const char* xb = (const char*)a.x;
  const char* wb = (const char*)a.w;
  const int Ktot = 9 * a.Cin;

  if (wres) {
    const int per_row = nchunks * 36;
    for (int idx = tid; idx < BN * per_row; idx += C3_THREADS) {
      const int n = idx / per_row, cu = idx - n * per_row;
      const int chunk = cu / 36, tu = cu - chunk * 36;
      const int ch = chunk * 4 * EPL + (tu & 3) * EPL;
      uint4 v = ys_zero16();
      if (n0 + n < a.Cout && ch < a.Cin)
        v = ys_ld16(wb + ((long)(n0 + n) * Ktot + (long)(tu >> 2) * a.Cin + ch) * (long)sizeof(T));
      sW[n * wpitch + cu] = v;
    }
  }

  // All loads of a fetch are issued unconditionally (clamped to a valid address) and masked when the registers are written to
  // LDS: loads under exec masks make the compiler wait for them with vmcnt(0) before the MFMAs they are meant to overlap.
  uint4 rp[NPU], rw[NWU];
  unsigned pmask = 0, wmask = 0;
  const long safe_x = (long)a.in_coff * (long)sizeof(T);
  auto fetch = [&](int tile, int chunk) {
    int t = tile;
    const int txi = t % a.tiles_x; t /= a.tiles_x;
    const int tyi = t % a.tiles_y;
    const int b = t / a.tiles_y;
    const int oy0 = tyi * a.TH, ox0 = txi * a.TW;
    const int iy_lo = (oy0 * a.SA - a.PAD) >> a.DIVS, ix_lo = (ox0 * a.SA - a.PAD) >> a.DIVS;
    const int iy_hi = ((oy0 + a.TH - 1) * a.SA + 2 - a.PAD) >> a.DIVS, ix_hi = ((ox0 + a.TW - 1) * a.SA + 2 - a.PAD) >> a.DIVS;
    const int PH = iy_hi - iy_lo + 1, PW = ix_hi - ix_lo + 1;
    const int npatch = PH * PW * 4;
    const int c0 = chunk * 4 * EPL;
    pmask = 0;
#pragma unroll
    for (int k = 0; k < NPU; k++) {
      const int idx = tid + C3_THREADS * k;
      const int pix = idx >> 2, u = idx & 3;
      const int r = pix / PW, cc = pix - r * PW;
      const int iy = iy_lo + r, ix = ix_lo + cc;
      const int ch = c0 + u * EPL;
      const bool ok = (bool)((int)(idx < npatch) & (int)((unsigned)iy < (unsigned)a.Hin) & (int)((unsigned)ix < (unsigned)a.Win) &
                             (int)(ch < a.Cin) & (int)!(a.dbg & 1));
      long off = ((((long)b * a.in_bstride + (long)iy * a.Win + ix) * a.in_ldc) + a.in_coff + ch) * (long)sizeof(T);
      off = ok ? off : safe_x;
      rp[k] = ys_ld16(xb + off);
      pmask |= (unsigned)ok << k;
    }
    if (!wres) {
      wmask = 0;
#pragma unroll
      for (int k = 0; k < NWU; k++) {
        const int idx = tid + C3_THREADS * k;
        const int n = idx / 36, tu = idx - n * 36;
        const int ch = c0 + (tu & 3) * EPL;
        const bool ok = (bool)((int)(idx < BN * 36) & (int)(n0 + n < a.Cout) & (int)(ch < a.Cin));
        long off = ((long)(n0 + n) * Ktot + (long)(tu >> 2) * a.Cin + ch) * (long)sizeof(T);
        off = ok ? off : 0;
        rw[k] = ys_ld16(wb + off);
        wmask |= (unsigned)ok << k;
      }
    }
  };

  int tile = blockIdx.x, chunk = 0;
  if (tile < ntiles) fetch(tile, 0);
  // geometry of the tile being computed
  int b = 0, oy0 = 0, ox0 = 0, iy_lo = 0, ix_lo = 0, PW = 1;
  int poy[MR], pox[MR];
  bool pv[MR];
  f32x4 acc[MR][NR];
  while (tile < ntiles) {
    __syncthreads();                       // every wave finished reading the previous chunk
#pragma unroll
    for (int k = 0; k < NPU; k++) {
      const int idx = tid + C3_THREADS * k;
      if (idx < PATCH_DATA) sP[(idx >> 2) * PP + (idx & 3)] = ((pmask >> k) & 1u) ? rp[k] : ys_zero16();
    }
    if (!wres) {
#pragma unroll
      for (int k = 0; k < NWU; k++) {
        const int idx = tid + C3_THREADS * k;
        if (idx < BN * 36) { const int n = idx / 36; sW[n * wpitch + (idx - n * 36)] = ((wmask >> k) & 1u) ? rw[k] : ys_zero16(); }
      }
    }
    __syncthreads();
    // ---- prefetch the next (tile, chunk); past the end it re-fetches the current one (unconditional, see above)
    int ntile = tile, nchunk = chunk + 1;
    if (nchunk == nchunks) { nchunk = 0; ntile = tile + gridDim.x; }
    {
      const bool more = ntile < ntiles;
      fetch(more ? ntile : tile, more ? nchunk : chunk);
    }
    // ---- compute this chunk from LDS
    if (chunk == 0) {
      int t = tile;
      const int txi = t % a.tiles_x; t /= a.tiles_x;
      const int tyi = t % a.tiles_y;
      b = t / a.tiles_y;
      oy0 = tyi * a.TH; ox0 = txi * a.TW;
      iy_lo = (oy0 * a.SA - a.PAD) >> a.DIVS; ix_lo = (ox0 * a.SA - a.PAD) >> a.DIVS;
      const int ix_hi = ((ox0 + a.TW - 1) * a.SA + 2 - a.PAD) >> a.DIVS;
      PW = ix_hi - ix_lo + 1;
#pragma unroll
      for (int mf = 0; mf < MR; mf++) {
        const int p = wave * (MR * 16) + mf * 16 + li;
        const int ty = p / a.TW, tx = p - ty * a.TW;
        poy[mf] = oy0 + ty; pox[mf] = ox0 + tx;
        pv[mf] = p < a.TH * a.TW && poy[mf] < a.Hout && pox[mf] < a.Wout;
#pragma unroll
        for (int nf = 0; nf < NR; nf++) acc[mf][nf] = f32x4_zero();
      }
    }
    const int wbase = wres ? chunk * 36 : 0;
    if (!(a.dbg & 2))
#pragma unroll
    for (int kh = 0; kh < 3; kh++) {
#pragma unroll
      for (int kw = 0; kw < 3; kw++) {
        uint4 xf[MR];
#pragma unroll
        for (int mf = 0; mf < MR; mf++) {
          const int ihn = poy[mf] * a.SA + kh - a.PAD, iwn = pox[mf] * a.SA + kw - a.PAD;
          const bool ok = pv[mf] && ((ihn | iwn) & a.DIVM) == 0;
          const int r = (ihn >> a.DIVS) - iy_lo, cc = (iwn >> a.DIVS) - ix_lo;
          xf[mf] = ys_zero16();
          if (ok) xf[mf] = sP[(r * PW + cc) * PP + q];
        }
#pragma unroll
        for (int nf = 0; nf < NR; nf++) {
          const uint4 wf = sW[(nf * 16 + li) * wpitch + wbase + (kh * 3 + kw) * 4 + q];
#pragma unroll
          for (int mf = 0; mf < MR; mf++) acc[mf][nf] = ys_mma<T>(wf, xf[mf], acc[mf][nf]);
        }
      }
    }
    if (chunk == nchunks - 1 && !(a.dbg & 4)) {
      // ---------------------------------------------------------------- epilogue (patch region becomes the staging area)
      __syncthreads();
      long orow[MR];
#pragma unroll
      for (int mf = 0; mf < MR; mf++) orow[mf] = (long)b * a.out_bstride + (pv[mf] ? ((long)poy[mf] * a.Wout + pox[mf]) : 0);
      T* wst = (T*)sP + wave * (16 * (BN + EPL));
      conv_epilogue<T, MR, NR, C3_THREADS / 64>(a, acc, orow, pv, n0, wst, sStat, (long)tile);
    }  // last chunk of the tile
    tile = ntile; chunk = nchunk;
  }
}

// host-side tile choice for the patch kernel: largest pixel tile (64*MR) whose patch fits PATCH_UNITS, shaped to
// minimise (patch pixels loaded) + (idle tile pixels), keeping a few workgroups per CU
struct TileChoice { int mr, th, tw, tx, ty; };
static TileChoice conv3x3_pick_tile(const ConvArgs& a, int nr) {
  const int gy = ys_cdiv(a.Cout, nr * 16);
  const int div = a.DIVM + 1;
  TileChoice best{0, 0, 0, 0, 0};
  for (int mr = 2; mr >= 1; mr >>= 1) {
    const int npx = 128 * mr;   // 8 waves x MR fragments x 16 pixels
    double best_cost = 1e30;
    TileChoice cur{0, 0, 0, 0, 0};
    for (int tw = 1; tw <= npx && tw <= a.Wout; tw++) {
      const int th_max = (npx / tw) < a.Hout ? (npx / tw) : a.Hout;
      for (int th = th_max; th >= 1; th--) {
        const int ph = div == 1 ? (th - 1) * a.SA + 3 : (th + 1) / 2 + 2, pw = div == 1 ? (tw - 1) * a.SA + 3 : (tw + 1) / 2 + 2;
        if ((long)ph * pw * 5 > PATCH_UNITS) continue;
        const int tx = ys_cdiv(a.Wout, tw), ty = ys_cdiv(a.Hout, th);
        const double cost = (double)tx * ty * ((double)ph * pw + 0.5 * npx);
        if (cost < best_cost) { best_cost = cost; cur = TileChoice{mr, th, tw, tx, ty}; }
      }
    }
    if (cur.mr == 0) continue;
    if (best.mr == 0) best = cur;
    if ((long)cur.tx * cur.ty * a.B * gy >= 512) return cur;   // enough tiles to feed every CU: take the largest
    best = cur;                                                // otherwise keep shrinking
  }
  return best;
}
struct C3Plan { int nr, wres, nchunks, wpitch, patch_units; size_t lds_bytes; };
static C3Plan conv3x3_plan(const ConvArgs& a, int epl) {
  const int nfr = (a.Cout + 15) / 16;
  const int nchunks = (a.Cin + 4 * epl - 1) / (4 * epl);
  C3Plan p{};
  p.nchunks = nchunks;
  const int es = epl == 8 ? 2 : 4;
  auto patch_units_for = [&](int nr) {   // patch region doubles as the epilogue staging area (8 waves x 16 x (BN+EPL) elements)
    const int need = (8 * 16 * (nr * 16 + epl) * es + 15) / 16;
    return need > PATCH_UNITS ? need : PATCH_UNITS;
  };
  for (int nr = nfr < 5 ? nfr : 5; nr >= 1; nr--) {       // weights of all chunks resident in LDS?
    const size_t fixed = (size_t)patch_units_for(nr) * 16;
    const size_t bytes = (size_t)nr * 16 * (nchunks * 36 + 1) * 16 + fixed + (size_t)nr * 16 * 64;
    if (bytes <= 144 * 1024 && (nr == nfr || nr * 2 >= (nfr < 5 ? nfr : 5))) {   // do not shrink NR below half for residency
      p.nr = nr; p.wres = 1; p.wpitch = nchunks * 36 + 1; p.lds_bytes = bytes; p.patch_units = patch_units_for(nr);
      return p;
    }
  }
  p.nr = nfr <= 5 ? nfr : (nfr % 5 == 0 ? 5 : 4);
  p.wres = 0; p.wpitch = 37; p.patch_units = patch_units_for(p.nr);
  p.lds_bytes = (size_t)p.nr * 16 * 37 * 16 + (size_t)p.patch_units * 16 + (size_t)p.nr * 16 * 64;
  return p;
}
// stride-2 forward convs have a 4x larger input patch per output pixel: their tiles would be patch-limited to ~64 pixels,
// so they stay on the direct-fragment kernel; stride-1 forward and all dgrads (SA == 1) use the LDS patch kernel
static bool conv_use_patch(const ConvArgs& a) { return a.KH == 3 && a.KW == 3 && a.SA == 1; }

template <class T, int MR, int NR>
static void conv_launch_t(hipStream_t st, const ConvArgs& a) {
  dim3 grid(ys_cdiv(a.M, 4 * MR * 16), ys_cdiv(a.Cout, NR * 16));
  char lab[128] = "";
  if (ys_kprof_enabled()) snprintf(lab, sizeof(lab), "direct k%d s%d div%d cin%d cout%d M%d acc%d mr%d nr%d", a.KH, a.SA, a.DIVM + 1, a.Cin, a.Cout, a.M, a.accumulate, MR, NR);
  YsKprofScope prof(st, "conv_igemm", lab);
  YS_LAUNCH((conv_igemm_kernel<T, MR, NR>), grid, 256, st, a);
}

// Tile selection.  NR = output-channel fragments per workgroup (all of Cout when it fits, so activations are read
// once); MR = pixel fragments per wave: 2 (occupancy: three workgroups per CU overlap each other's load and
// epilogue phases; larger MR measured slower), 1 on small feature maps (20x20, 40x40 at the deep end of the net)
// so that the grid still covers the 256 CUs a few times.
static int conv_pick_nr(int cout, int M = 1 << 30) {
  const int nfr = (cout + 15) / 16;
  if (nfr <= 6) return nfr;
  // small feature maps: narrower column tiles give the chip more workgroups (Cin = 128 -> 256 stride-2 layer at 20x20: 119 -> 83 us)
  const int smallm = 30000;
  if (M <= smallm && nfr % 4 == 0) return 4;
  if (nfr % 8 == 0 || nfr > 10) return 8;
  if (nfr % 5 == 0) return 5;
  return 4;
}
static int conv_pick_mr(int M, int cout) {
  const int nr = conv_pick_nr(cout, M);
  const int gy = ys_cdiv(cout, nr * 16);
  int mr = 2;   // measured: 2 fragments per wave (<= ~130 registers, 3 workgroups per CU) beats 4-8 fragments at 2 per CU
  while (mr > 1 && (long)ys_cdiv(M, 64 * mr) * gy < 768) mr >>= 1;
  return mr;
}

template <class T, int MR, int NR>
static int conv3x3_launch_t(hipStream_t st, ConvArgs a, const TileChoice& t, const C3Plan& p) {
  a.TH = t.th; a.TW = t.tw; a.tiles_x = t.tx; a.tiles_y = t.ty;
#ifdef YS_P2_ABLATE
  a.dbg = (int)YS_OPT_INT("DBG", 0);
#endif
  const int ntiles = t.tx * t.ty * a.B;
  const int gy = ys_cdiv(a.Cout, NR * 16);
  const int per_cu = p.lds_bytes <= 76 * 1024 ? 2 : 1;
  int gx = (ys_cu_count() * per_cu + gy - 1) / gy;
  if (gx > ntiles) gx = ntiles;
  static std::atomic<unsigned> attr_done{0};      // per device: the attribute belongs to the device's code object
  int dev_id = 0;
  (void)hipGetDevice(&dev_id);
  if (!(attr_done.load(std::memory_order_relaxed) & (1u << (dev_id & 31)))) {
    hipFuncSetAttribute((const void*)conv3x3_tile_kernel<T, MR, NR>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    attr_done.fetch_or(1u << (dev_id & 31), std::memory_order_relaxed);
  }
  char lab[160] = "";
  if (ys_kprof_enabled()) snprintf(lab, sizeof(lab), "patch k3 s%d div%d cin%d cout%d M%d acc%d mr%d nr%d tile%dx%d grid%dx%d lds%d", a.SA, a.DIVM + 1, a.Cin, a.Cout, a.M, a.accumulate, MR, NR, a.TH, a.TW, gx, gy, (int)p.lds_bytes);
  YsKprofScope prof(st, "conv_igemm", lab);
  YS_LAUNCH_LDS((conv3x3_tile_kernel<T, MR, NR>), dim3(gx, gy), C3_THREADS, p.lds_bytes, st, a, ntiles, p.nchunks, p.wres, p.wpitch, p.patch_units);
  return YS_OK;
}

// the chunked 3x3 kernel's tile: the same for both dtypes (its tile count is the statistics grid); NR only enters through the workgroup-count heuristic
static TileChoice conv3x3_tile(const ConvArgs& a) { return conv3x3_pick_tile(a, conv3x3_plan(a, 8).nr); }

// variant dispatch of the chunked 3x3 patch kernel / the direct-fragment kernel
template <class T>
static int conv3x3_dispatch(hipStream_t st, const ConvArgs& a) {
  const C3Plan p = conv3x3_plan(a, Elem<T>::EPL);
  const TileChoice t = conv3x3_tile(a);
  if (t.mr == 0) { ys_set_error("conv3x3: no tile fits"); return YS_ERR_UNSUPPORTED; }
#define C3(M_, N_) if (t.mr == M_ && p.nr == N_) return conv3x3_launch_t<T, M_, N_>(st, a, t, p);
  C3(1, 1) C3(2, 1) C3(1, 2) C3(2, 2) C3(1, 3) C3(2, 3) C3(1, 4) C3(2, 4) C3(1, 5) C3(2, 5)
#undef C3
  ys_set_error("conv3x3: no kernel for tile MR=%d NR=%d", t.mr, p.nr);
  return YS_ERR_UNSUPPORTED;
}
template <class T>
static int conv_generic_dispatch(hipStream_t st, const ConvArgs& a) {
  const int nr = conv_pick_nr(a.Cout, a.M), mr = conv_pick_mr(a.M, a.Cout);
#define CV(M_, N_) if (mr == M_ && nr == N_) { conv_launch_t<T, M_, N_>(st, a); return YS_OK; }
  CV(1, 1) CV(2, 1) CV(4, 1) CV(8, 1)
  CV(1, 2) CV(2, 2) CV(4, 2) CV(8, 2)
  CV(1, 3) CV(2, 3) CV(4, 3)
  CV(1, 4) CV(2, 4) CV(4, 4)
  CV(1, 5) CV(2, 5)
  CV(1, 6) CV(2, 6)
  CV(1, 8) CV(2, 8)
#undef CV
  ys_set_error("conv: no kernel for tile MR=%d NR=%d", mr, nr);
  return YS_ERR_UNSUPPORTED;
}

// ===================================================================================== the route
// Which kernels run a convolution is decided HERE and nowhere else.  ys_conv_launch executes a route; the queries at the end of the file (statistics
// rows, BN-backward partial rows, fp8 image wanted, P2 channel tiles) read one -- so the memory their answers size is the memory the launch writes.
enum ConvKind { CONV_GEMM, CONV_P2, CONV_PATCH3X3, CONV_GENERIC };
struct ConvLeaf {
  ConvKind kind;
  ConvArgs a;      // effective arguments: f8 cleared where fp8 is declined or has no plan, x8 set where the quantised image is used, phase geometry for a phase
  P2Plan p2;       // CONV_P2 outside a grouped launch
  int rows;        // statistics / BN-backward partial rows the launch writes: one per workgroup (per tile for the chunked 3x3 kernel)
  bool bnred;      // the kernel variant carries the fused BN-backward reduction (conv_epi.h)
};
struct ConvRoute {
  bool quantise_first;   // ys_f8_quant_view_launch of the input view into a.q8 before the leaves, which read it as x8 (that pass records amax)
  bool grouped;          // the leaves are the four phases of a stride-2 dgrad as ONE conv_p2_group_kernel grid (their own plans are the group's business)
  int n;                 // 1, or the non-empty phases of a stride-2 dgrad in launch order
  ConvLeaf leaf[4];
};

// fp8 pays where the quantisation pass of the input is amortised over several taps: measured on YOLOv8x 1280 (config 5), every 1x1
// layer is faster on the bf16 kernels once that pass is counted (e.g. 1280 -> 320 @ 160x160: 480 us bf16 vs 306 + 393 us), every
// 3x3 layer is 1.3-1.5x faster in fp8.  YS_F8_MIN_TAPS overrides (the tests run 1x1 layers in fp8 too).
static bool conv_f8_declined(const ConvArgs& a) {
  const int min_taps = (int)YS_OPT_INT("F8_MIN_TAPS", 4);
  return a.f8 && !a.x8 && a.KH * a.KW < min_taps;
}
// an fp8 request that could read a dense fp8 image of its input if one were made: none is there yet, and the images of the batch are contiguous in the view
static bool conv_f8_image_possible(const ConvArgs& a) { return a.f8 && !a.x8 && a.in_bstride == (long)a.Hin * a.Win; }

// ---- stride-2 3x3 dgrad as four phase convolutions (bf16).  dx[ih, iw] only receives the taps whose parity matches
// (ih, iw): phase (a, b) = (ih & 1, iw & 1) is a stride-1 correlation of dy with KH_a x KW_b taps (1 if the parity is 0,
// else 2: row offsets {0, +1} <-> kh = {2, 0}) written to the rows 2i+a / columns 2j+b of dx.  9/4 taps per output pixel
// instead of 9 with 3/4 of them predicated off.  The dgrad weights of such a layer are laid out phase-major by the weight
// prep: [phase][Cin_real][taps_p][Cout_pad], phases in the order (0,0) (0,1) (1,0) (1,1) -> tap offsets 0, 1, 3, 5.
bool ys_conv_dgrad_uses_phases(int dtype, int k, int stride) { return dtype == YS_BF16 && k == 3 && stride == 2; }

// arguments of phase ph of a stride-2 3x3 dgrad; false when the phase has no output pixels
static bool conv_dgrad_s2_phase_args(const ConvArgs& a, int ph, ConvArgs& q) {
  static const int toff[4] = {0, 1, 3, 5};
  const int Hx = a.Hout, Wx = a.Wout;                     // dx grid (the layer's input)
  const int pa = ph >> 1, pb = ph & 1;
  q = a;
  q.KH = pa ? 2 : 1; q.KW = pb ? 2 : 1;
  q.SA = 1; q.DIVS = 0; q.DIVM = 0; q.PAD = 0;
  q.Hout = (Hx - pa + 1) / 2; q.Wout = (Wx - pb + 1) / 2;
  if (q.Hout <= 0 || q.Wout <= 0) return false;
  q.M = a.B * q.Hout * q.Wout;
  q.w = (const char*)a.w + (size_t)toff[ph] * a.Cout * a.Cin * 2;   // [phase][Cout = layer Cin_real][taps_p][Cin = layer Cout_pad]
  if (a.w8) q.w8 = (const char*)a.w8 + (size_t)toff[ph] * a.Cout * a.Cin;
  q.out_rh = 2 * Wx; q.out_rw = 2; q.out_r0 = (long)pa * Wx + pb;
  return true;
}

// One convolution -- a layer, or one phase of a stride-2 dgrad -- to its kernel.  bf16 storage: an fp8 request runs the blocked-GEMM kernel on the fp8
// image, else the P2 kernel's fp8 mode, else (no fp8 plan for this shape) it is a bf16 launch with the same result type; bf16: the blocked GEMM of the
// wide layers, else P2.  What neither takes, and every f32 layer, runs the chunked 3x3 patch kernel or the direct-fragment kernel.
static ConvLeaf conv_route_leaf(const ConvArgs& a, int dtype) {
  ConvLeaf l{};
  l.a = a;
  if (dtype == YS_BF16) {
    if (l.a.f8) {
      if (l.a.x8 && (l.rows = ys_conv_gemm_rows(l.a)) != 0) { l.kind = CONV_GEMM; l.bnred = l.a.f8 == 2; return l; }   // only the e5m2-input (dgrad) form of the fp8 GEMM kernel carries the fused reduction
      l.p2 = ys_conv_p2_plan(l.a);
      if (l.p2.ok) { l.kind = CONV_P2; l.rows = l.p2.gx; l.bnred = false; return l; }                                    // conv_p2_kernel<F8> has none
      l.a.f8 = 0;
    }
    if ((l.rows = ys_conv_gemm_rows(l.a)) != 0) { l.kind = CONV_GEMM; l.bnred = true; return l; }
    l.p2 = ys_conv_p2_plan(l.a);
    if (l.p2.ok) { l.kind = CONV_P2; l.rows = l.p2.gx; l.bnred = true; return l; }   // one row per (persistent) workgroup
  }
  if (conv_use_patch(l.a)) {
    const TileChoice t = conv3x3_tile(l.a);
    l.kind = CONV_PATCH3X3; l.rows = t.tx * t.ty * l.a.B;
    return l;
  }
  l.kind = CONV_GENERIC; l.rows = ys_cdiv(l.a.M, 64 * conv_pick_mr(l.a.M, l.a.Cout));
  return l;
}

// the phases of a stride-2 3x3 dgrad (bf16 storage)
static void conv_route_phases(ConvRoute& r, const ConvArgs& a) {
  // The four phases as ONE persistent grid (conv_p2_group_kernel) when every phase is a bf16 patch-kernel launch of one variant: they read the
  // same dy tiles -- side by side on an XCD the second to fourth read hit its L2 -- and three launches' fixed costs go.  The 2x2-tap phase
  // first: the group runs on the variant of its first largest member, and that phase has the largest patch.
  if (!a.f8) {
    ConvArgs qs[4];
    int n = 0, rows[4];
    for (int ph = 3; ph >= 0; ph--) if (conv_dgrad_s2_phase_args(a, ph, qs[n])) n++; else break;
    if (n == 4 && ys_conv_p2_group_launch(nullptr, qs, 4, nullptr, rows, true) == YS_OK) {
      r.grouped = true;
      for (int i = 0, row0 = a.red_row0; i < 4; row0 += rows[i++]) {
        ConvLeaf& l = r.leaf[r.n++];
        l.kind = CONV_P2; l.a = qs[i]; l.a.red_row0 = row0; l.rows = rows[i]; l.bnred = true;
      }
      return;
    }
  }
  int row0 = a.red_row0;
  for (int ph = 0; ph < 4; ph++) {
    ConvArgs q;
    if (!conv_dgrad_s2_phase_args(a, ph, q)) continue;
    q.red_row0 = row0;                                                // the phases write disjoint pixels of dx: their partial rows stack
    const ConvLeaf& l = r.leaf[r.n++] = conv_route_leaf(q, YS_BF16);
    if (l.kind == CONV_GEMM || l.kind == CONV_P2) row0 += l.rows;     // (the other two kernels have no fused reduction: such a route answers 0 rows)
  }
}

static ConvRoute conv_route(const ConvArgs& a0, int dtype) {
  ConvRoute r{};
  ConvArgs a = a0;
  if (dtype != YS_BF16) { r.leaf[r.n++] = conv_route_leaf(a, dtype); return r; }
  if (conv_f8_declined(a)) a.f8 = 0;
  // fp8 on the blocked-GEMM kernel: its operand tiles reach LDS by DMA, so the input view is quantised into the caller's scratch first (one pass
  // that also records amax(|input|) for the next step's scale) -- when the layer, or a phase of its stride-2 dgrad, will run that kernel.  Routed
  // as if the image were there: x8 only ever selects that kernel, so without such a leaf the route is the one of the arguments as they came.
  const bool lent = a.q8 && conv_f8_image_possible(a);
  if (lent) a.x8 = a.q8;
  if (ys_conv_dgrad_uses_phases(dtype, a.KH, a.DIVM + 1) && a.KW == a.KH) conv_route_phases(r, a);
  else r.leaf[r.n++] = conv_route_leaf(a, dtype);
  if (lent) {
    for (int i = 0; i < r.n; i++) r.quantise_first |= r.leaf[i].kind == CONV_GEMM && r.leaf[i].a.f8;
    for (int i = 0; i < r.n; i++) { if (r.quantise_first) r.leaf[i].a.amax = nullptr; else r.leaf[i].a.x8 = nullptr; }   // (amax: recorded by the quantisation pass)
  }
  return r;
}

static int conv_leaf_launch(hipStream_t st, int dtype, const ConvLeaf& l) {
  const bool bf16 = dtype == YS_BF16;
  switch (l.kind) {
    case CONV_GEMM: return ys_conv_gemm_launch(st, l.a);
    case CONV_P2: return ys_conv_p2_dispatch(st, l.a, l.p2);
    case CONV_PATCH3X3: return bf16 ? conv3x3_dispatch<bf16_t>(st, l.a) : conv3x3_dispatch<float>(st, l.a);
    default: return bf16 ? conv_generic_dispatch<bf16_t>(st, l.a) : conv_generic_dispatch<float>(st, l.a);
  }
}

int ys_conv_launch(hipStream_t st, int dtype, const ConvArgs& a) {
  const int epl = dtype == YS_BF16 ? 8 : 4;
  if (a.Cin % epl || a.in_ldc % epl || a.in_coff % epl) {
    ys_set_error("conv: Cin/ldc/coff (%d,%d,%d) must be multiples of %d", a.Cin, a.in_ldc, a.in_coff, epl);
    return YS_ERR_INVALID_ARG;
  }
  const ConvRoute r = conv_route(a, dtype);
  if (r.quantise_first) {
    const int rc = ys_f8_quant_view_launch(st, a.f8 == 2 ? 1 : 0, a.x, (long)a.B * a.Hin * a.Win, a.Cin, a.in_ldc, a.in_coff, a.qscale, a.q8, a.amax);
    if (rc != YS_OK) return rc;
  }
  if (r.grouped) {
    ConvArgs qs[4];
    int rows[4];
    for (int i = 0; i < r.n; i++) qs[i] = r.leaf[i].a;
    return ys_conv_p2_group_launch(st, qs, r.n, nullptr, rows);
  }
  for (int i = 0; i < r.n; i++) {
    const int rc = conv_leaf_launch(st, dtype, r.leaf[i]);
    if (rc != YS_OK) return rc;
  }
  return YS_OK;
}

// ---- what a launch of `a` will do, read from its route (prototypes and contracts: ys_kernels.h)
int ys_conv_grid_m(const ConvArgs& a, int dtype) {
  const ConvRoute r = conv_route(a, dtype);
  int rows = 0;
  for (int i = 0; i < r.n; i++) rows += r.leaf[i].rows;
  return rows;
}

int ys_conv_bnred_rows(const ConvArgs& a, int dtype) {
  const ConvRoute r = conv_route(a, dtype);
  int rows = 0;
  for (int i = 0; i < r.n; i++) { if (!r.leaf[i].bnred) return 0; rows += r.leaf[i].rows; }
  return rows;
}

bool ys_conv_wants_x8(const ConvArgs& a) {
  if (!conv_f8_image_possible(a)) return false;
  ConvArgs b = a; b.x8 = a.x;                 // any non-null pointer: the plans only test for presence
  const ConvRoute r = conv_route(b, YS_BF16);
  for (int i = 0; i < r.n; i++) if (r.leaf[i].kind == CONV_GEMM && r.leaf[i].a.f8) return true;
  return false;
}

// channel tiles (gridDim.y) of the conv_p2_kernel launch a bf16 forward convolution gets when it runs that kernel in bf16; 0 = another kernel runs it
int ys_conv_is_p2(const ConvArgs& a) {
  const ConvRoute r = conv_route(a, YS_BF16);
  return r.n == 1 && r.leaf[0].kind == CONV_P2 && !r.leaf[0].a.f8 ? r.leaf[0].p2.gy : 0;
}
