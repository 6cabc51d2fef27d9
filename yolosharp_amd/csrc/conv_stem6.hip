// conv_stem6.hip -- the first convolution of the YOLOv5u graph (model.0 = Conv(3, c, k = 6, s = 2, p = 2): Models/Yolo.cs:163, Modules/Convs.cs:36-62) read
// STRAIGHT from the image tensor the reference hands over: fp32 NCHW [B][3][H][W], gfx950 (CDNA4).  The 6x6 sibling of conv_stem.hip, with the same contract:
// the forward and the weight gradient stage their input patch from the fp32 planes themselves (rounded to bf16 on the way into LDS, the rounding the packed
// NHWC copy has), so the layer needs no packed copy of the image.  It moves the bytes of the 3x3 stem (B = 64 at 640 x 640: 315 MB read + 210 MB written
// forward, 315 + 210 MB read backward) for 4x its arithmetic (23 GFLOP): still HBM-bound by two orders of magnitude.
//
// GEMM view: K = 3 * 6 * 6 = 108 padded to 128, k = c * 36 + kh * 6 + kw (kw fastest: an even k and its odd neighbour are two ADJACENT input columns),
//   forward   D[cout][pixel] = sum_k W[cout][k] X[pixel][k]            four v_mfma_f32_16x16x32_bf16 per 16 pixels x 16 output channels
//   wgrad     D[cout][k]     = sum_pixels dy[pixel][cout] X[pixel][k]   seven 16-column blocks of k (112), K = 32 consecutive pixels of one output row
// A workgroup tile is 8 x 32 output pixels; its input patch is rows 2 oy0 - 2 .. + 19, columns 2 ox0 - 2 .. + 67 of the three planes.  2 ox0 - 2 is even and
// 2 ox0 a multiple of 64: a patch row is [2 halo | 64 aligned | 2 halo] columns.
#include "ys_internal.h"
#include "ys_kernels.h"
#include <atomic>
#include <cstdlib>

#define S6_TH 8
#define S6_TW 32
#define S6_PH (2 * S6_TH + 4)          // 20 input rows
#define S6_PW (2 * S6_TW + 4)          // 68 input columns
#define S6_ROWS (3 * S6_PH)            // 60 patch rows (plane, row)
#define S6_NPATCH (S6_ROWS * S6_PW)    // 4080
#define S6_THREADS 256
#define S6_NLD ((S6_NPATCH + S6_THREADS - 1) / S6_THREADS)   // patch values per thread, element form (16)
// vector form: per patch row the float2 of columns 0, 1 (the left halo) and seventeen aligned float4 of columns 2 .. 69 (66, 67 = the right halo; 68, 69 are
// fetched with them and never read)
#define S6_VPR 17
#define S6_NVEC (S6_ROWS * S6_VPR)     // 1020
#define S6_NVL ((S6_NVEC + S6_THREADS - 1) / S6_THREADS)     // 4 per thread
#define S6_KB 7                        // 16-column blocks of k in the weight gradient

struct Stem6FwdArgs {
  const float* x;            // [B][3][H][W] fp32
  const bf16_t* wf;          // forward weight shadow [Cout][36][8] (channels 3..7 zero)
  bf16_t* y;                 // [B][out_bstride][out_ldc] + out_coff
  float* stats;              // training: one row [2][Cout] per workgroup (sum, sum of squares of the bf16-rounded outputs)
  unsigned long long* stat_acc;   // ... or, when set, fixed-point integer accumulators (ys_kernels.h ys_stat_acc_add)
  const float* scale;        // eval: BatchNorm folded to scale / shift (+ SiLU when act)
  const float* shift;
  int B, H, W, Hout, Wout, Cout, out_ldc, out_coff, act;
  long out_bstride;          // rows per image of the output buffer
  int tiles_x, tiles_y, ntiles;
};

// fp32 image patch of the tile whose first input row / column are (iy0, ix0) -> registers (all loads in flight), zero outside the image
__device__ inline void s6_patch_fetch(const float* __restrict__ x, int b, int iy0, int ix0, int H, int W, float (&v)[S6_NLD]) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int k = 0; k < S6_NLD; k++) {
    const int e = tid + S6_THREADS * k;
    const int row = e / S6_PW, col = e - row * S6_PW;
    const int c = row / S6_PH, r = row - c * S6_PH;
    const int iy = iy0 + r, ix = ix0 + col;
    const bool ok = (bool)((int)(e < S6_NPATCH) & (int)((unsigned)iy < (unsigned)H) & (int)((unsigned)ix < (unsigned)W));
    const long off = ok ? (((long)b * 3 + c) * H + iy) * (long)W + ix : 0;
    const float f = x[off];
    v[k] = ok ? f : 0.f;
  }
}

// The same patch as 16-byte vectors (W % 4 == 0 and a 16-byte aligned image: ix0 + 2 is a multiple of 64, so every float4 is aligned and lies inside the row or
// outside it as a whole; ix0 is even, so the float2 of the left halo is 8-byte aligned).  Vector u = tid + 256 k: patch row u / 17, columns 2 + 4 (u % 17) .. + 3.
struct S6PatchV { float4 v[S6_NVL]; float2 h; };
__device__ inline void s6_patch_fetch_v(const float* __restrict__ x, int b, int iy0, int ix0, int H, int W, S6PatchV& p) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int k = 0; k < S6_NVL; k++) {
    const int u = tid + S6_THREADS * k;
    const int row = u / S6_VPR, j = u - row * S6_VPR;
    const int c = row / S6_PH, r = row - c * S6_PH;
    const int iy = iy0 + r, ix = ix0 + 2 + 4 * j;
    const bool ok = (bool)((int)(u < S6_NVEC) & (int)((unsigned)iy < (unsigned)H) & (int)(ix + 3 < W));
    const long off = ok ? (((long)b * 3 + c) * H + iy) * (long)W + ix : 0;
    const float4 f = *(const float4*)(x + off);
    p.v[k] = ok ? f : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  {
    const int row = tid < S6_ROWS ? tid : 0;
    const int c = row / S6_PH, r = row - c * S6_PH;
    const int iy = iy0 + r;
    const bool ok = (bool)((int)(tid < S6_ROWS) & (int)((unsigned)iy < (unsigned)H) & (int)(ix0 >= 0));
    const long off = ok ? (((long)b * 3 + c) * H + iy) * (long)W + ix0 : 0;
    const float2 f = *(const float2*)(x + off);
    p.h = ok ? f : make_float2(0.f, 0.f);
  }
}

__device__ inline void s6_tile_origin(int tile, int tiles_x, int tiles_y, int& b, int& oy0, int& ox0) {
  const int tx = tile % tiles_x, trem = tile / tiles_x;
  b = trem / tiles_y; oy0 = (trem % tiles_y) * S6_TH; ox0 = tx * S6_TW;
}

// ------------------------------------------------------------------------------------------------------------------ forward
// LDS patch: planar bf16 [60][72].  Lane (li, q) of a pixel fragment supplies, in K-step s, the K values k = 32 s + 8 q .. + 7 of pixel li: four (even k, odd k)
// pairs, each ONE aligned 4-byte LDS read (patch column 2 ox + kw with kw even; the row pitch is even).  k >= 108 has zero weights and re-reads k = 0.
template <int NR, int EVAL, int VEC>
__global__ void __launch_bounds__(S6_THREADS)
stem6_fwd_kernel(Stem6FwdArgs a) {
  constexpr int PWP = 72;
  __shared__ unsigned sPw[S6_ROWS * PWP / 2];
  __shared__ float sStat[4][NR * 16][2];
  unsigned short* sP = (unsigned short*)sPw;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, q = lane >> 4;

  // weight fragments (rows = output channels) and this lane's patch offsets: both tile-independent
  uint4 wfr[NR][4];
  int offp[16];
#pragma unroll
  for (int i = 0; i < 16; i++) {
    const int k = (i >> 2) * 32 + q * 8 + (i & 3) * 2;
    const int c = k / 36, tap = k - c * 36;
    const int kh = tap / 6, kw = tap - kh * 6;
    offp[i] = k < 108 ? (c * S6_PH + kh) * PWP + kw : 0;
  }
#pragma unroll
  for (int nf = 0; nf < NR; nf++)
#pragma unroll
    for (int s = 0; s < 4; s++) {
      unsigned short e[8];
#pragma unroll
      for (int j = 0; j < 8; j++) {
        const int k = s * 32 + q * 8 + j;
        const int c = k / 36, tap = k - c * 36;
        const int co = nf * 16 + li;
        const bool ok = (bool)((int)(k < 108) & (int)(co < a.Cout));
        const unsigned short w = a.wf[ok ? ((long)co * 36 + tap) * 8 + c : 0].v;
        e[j] = ok ? w : (unsigned short)0;
      }
      wfr[nf][s] = make_uint4((unsigned)e[0] | ((unsigned)e[1] << 16), (unsigned)e[2] | ((unsigned)e[3] << 16),
                              (unsigned)e[4] | ((unsigned)e[5] << 16), (unsigned)e[6] | ((unsigned)e[7] << 16));
    }
  float sc[NR][4], sh[NR][4];
  if (EVAL) {
#pragma unroll
    for (int nf = 0; nf < NR; nf++)
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int c = nf * 16 + q * 4 + r;
        sc[nf][r] = c < a.Cout ? a.scale[c] : 0.f;
        sh[nf][r] = c < a.Cout ? a.shift[c] : 0.f;
      }
  }
  float st1[NR][4], st2[NR][4];
#pragma unroll
  for (int nf = 0; nf < NR; nf++)
#pragma unroll
    for (int r = 0; r < 4; r++) { st1[nf][r] = 0.f; st2[nf][r] = 0.f; }

  // VEC: the NEXT tile's patch is requested as soon as the current one sits in LDS (as in stem_fwd_kernel: a workgroup's loads stay in flight all the time)
  S6PatchV pv;
  if (VEC && (int)blockIdx.x < a.ntiles) {
    int b, oy0, ox0;
    s6_tile_origin(blockIdx.x, a.tiles_x, a.tiles_y, b, oy0, ox0);
    s6_patch_fetch_v(a.x, b, 2 * oy0 - 2, 2 * ox0 - 2, a.H, a.W, pv);
  }
  for (int tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
    int b, oy0, ox0;
    s6_tile_origin(tile, a.tiles_x, a.tiles_y, b, oy0, ox0);
    if (VEC) {
      __syncthreads();                        // the previous tile's fragments are read
#pragma unroll
      for (int k = 0; k < S6_NVL; k++) {
        const int u = tid + S6_THREADS * k;
        if (u < S6_NVEC) {
          const int row = u / S6_VPR, j = u - row * S6_VPR;
          unsigned* d = sPw + row * (PWP / 2) + 1 + 2 * j;      // columns 2 + 4 j .. + 3: two aligned pairs
          d[0] = ys_pack_bf16x2(pv.v[k].x, pv.v[k].y);
          d[1] = ys_pack_bf16x2(pv.v[k].z, pv.v[k].w);
        }
      }
      if (tid < S6_ROWS) sPw[tid * (PWP / 2)] = ys_pack_bf16x2(pv.h.x, pv.h.y);
      const int nt = tile + gridDim.x;
      if (nt < a.ntiles) {
        int nb, noy0, nox0;
        s6_tile_origin(nt, a.tiles_x, a.tiles_y, nb, noy0, nox0);
        s6_patch_fetch_v(a.x, nb, 2 * noy0 - 2, 2 * nox0 - 2, a.H, a.W, pv);
      }
    } else {
      float v[S6_NLD];
      s6_patch_fetch(a.x, b, 2 * oy0 - 2, 2 * ox0 - 2, a.H, a.W, v);
      __syncthreads();                        // the previous tile's fragments are read
#pragma unroll
      for (int k = 0; k < S6_NLD; k++) {
        const int e = tid + S6_THREADS * k;
        if (e < S6_NPATCH) {
          const int row = e / S6_PW, col = e - row * S6_PW;
          sP[row * PWP + col] = Elem<bf16_t>::from_f(v[k]).v;
        }
      }
    }
    __syncthreads();                          // the patch is complete
#pragma unroll
    for (int mf = 0; mf < 4; mf++) {
      const int oyl = 2 * wave + (mf >> 1), oxl = (mf & 1) * 16 + li;
      const unsigned short* pp = sP + (2 * oyl) * PWP + 2 * oxl;
      uint4 xf[4];
#pragma unroll
      for (int s = 0; s < 4; s++)
        xf[s] = make_uint4(*(const unsigned*)(pp + offp[4 * s]), *(const unsigned*)(pp + offp[4 * s + 1]),
                           *(const unsigned*)(pp + offp[4 * s + 2]), *(const unsigned*)(pp + offp[4 * s + 3]));
      const int oy = oy0 + oyl, ox = ox0 + oxl;
      const bool valid = (bool)((int)(oy < a.Hout) & (int)(ox < a.Wout));
      bf16_t* yp = a.y + (((long)b * a.out_bstride + (long)(valid ? oy : 0) * a.Wout + (valid ? ox : 0)) * a.out_ldc + a.out_coff + q * 4);
#pragma unroll
      for (int nf = 0; nf < NR; nf++) {
        f32x4 d = f32x4_zero();
#pragma unroll
        for (int s = 0; s < 4; s++) d = ys_mma<bf16_t>(wfr[nf][s], xf[s], d);
        uint2 pk;
        pk.x = ys_pack_bf16x2(d[0], d[1]);
        pk.y = ys_pack_bf16x2(d[2], d[3]);
        // everything downstream sees the bf16-rounded output: statistics (training) and the folded BatchNorm (eval) use it too
        float f[4] = {ys_u2f(pk.x << 16), ys_u2f(pk.x & 0xffff0000u), ys_u2f(pk.y << 16), ys_u2f(pk.y & 0xffff0000u)};
        if (EVAL) {
#pragma unroll
          for (int r = 0; r < 4; r++) { f[r] = f[r] * sc[nf][r] + sh[nf][r]; }
          if (a.act) {
#pragma unroll
            for (int r = 0; r < 4; r++) f[r] = ys_silu(f[r]);
          }
          pk.x = ys_pack_bf16x2(f[0], f[1]);
          pk.y = ys_pack_bf16x2(f[2], f[3]);
        } else if (valid) {
#pragma unroll
          for (int r = 0; r < 4; r++) { st1[nf][r] += f[r]; st2[nf][r] += f[r] * f[r]; }
        }
        if (valid && nf * 16 + q * 4 < a.Cout) *(uint2*)(yp + nf * 16) = pk;
      }
    }
  }
  if (!EVAL && a.stats) {
    // one statistics row per workgroup: the 16 pixel lanes of a quarter, then the four waves in a fixed order
#pragma unroll
    for (int nf = 0; nf < NR; nf++)
#pragma unroll
      for (int r = 0; r < 4; r++) {
        float s1 = st1[nf][r], s2 = st2[nf][r];
#pragma unroll
        for (int msk = 1; msk < 16; msk <<= 1) { s1 += __shfl_xor(s1, msk); s2 += __shfl_xor(s2, msk); }
        if (li == 0) { sStat[wave][nf * 16 + q * 4 + r][0] = s1; sStat[wave][nf * 16 + q * 4 + r][1] = s2; }
      }
    __syncthreads();
    if (tid < NR * 16 && tid < a.Cout) {
      const float s1 = (sStat[0][tid][0] + sStat[1][tid][0]) + (sStat[2][tid][0] + sStat[3][tid][0]);
      const float s2 = (sStat[0][tid][1] + sStat[1][tid][1]) + (sStat[2][tid][1] + sStat[3][tid][1]);
      if (a.stat_acc) { ys_stat_acc_add(a.stat_acc, (long)blockIdx.x, a.Cout, tid, 0, s1); ys_stat_acc_add(a.stat_acc, (long)blockIdx.x, a.Cout, tid, 1, s2); }
      else {
        a.stats[((long)blockIdx.x * 2 + 0) * a.Cout + tid] = s1;
        a.stats[((long)blockIdx.x * 2 + 1) * a.Cout + tid] = s2;
      }
    }
  }
}

bool ys_stem6_eligible(int dtype, int cin, int cout, int k, int s, int pad) {
  return dtype == YS_BF16 && cin == 3 && k == 6 && s == 2 && pad == 2 && cout % 16 == 0 && cout >= 16 && cout <= 80;
}

static int s6_hout(int H) { return (H - 2) / 2 + 1; }                                    // (H + 2 * 2 - 6) / 2 + 1
static int s6_grid(long ntiles) { return (int)(ntiles < 2048 ? ntiles : 2048); }         // rows of the statistics region

int ys_stem6_fwd_rows(int B, int Hout, int Wout) {
  return s6_grid((long)B * ys_cdiv(Hout, S6_TH) * ys_cdiv(Wout, S6_TW));
}

// training (stats != nullptr): raw bf16 output + one statistics row per workgroup (*rows); eval: scale / shift (+ SiLU) applied
int ys_stem6_fwd_launch(hipStream_t st, const float* x, int B, int H, int W, const void* wf, int Cout, void* y, int out_ldc, int out_coff,
                        long out_bstride, float* stats, const float* scale, const float* shift, int act, int* rows, unsigned long long* stat_acc) {
  Stem6FwdArgs a{};
  a.x = x; a.wf = (const bf16_t*)wf; a.y = (bf16_t*)y; a.stats = stats; a.stat_acc = stat_acc; a.scale = scale; a.shift = shift; a.act = act;
  a.B = B; a.H = H; a.W = W; a.Hout = s6_hout(H); a.Wout = s6_hout(W); a.Cout = Cout;
  a.out_ldc = out_ldc; a.out_coff = out_coff; a.out_bstride = out_bstride;
  if (B < 1 || H < 2 || W < 2 || (long)B * 3 * H * W >= (1L << 31) || (out_ldc & 3) || (out_coff & 3)) { ys_set_error("stem6 conv: unsupported view"); return YS_ERR_UNSUPPORTED; }
  a.tiles_x = ys_cdiv(a.Wout, S6_TW); a.tiles_y = ys_cdiv(a.Hout, S6_TH); a.ntiles = B * a.tiles_x * a.tiles_y;
  const int grid = s6_grid(a.ntiles);
  if (rows) *rows = grid;
  const int nr = Cout / 16;
  const bool eval = stats == nullptr;
  if (eval && (!scale || !shift)) { ys_set_error("stem6 conv: eval launch without BatchNorm coefficients"); return YS_ERR_INVALID_ARG; }
  if (Cout % 16 || nr < 1 || nr > 5) { ys_set_error("stem6 conv: %d output channels", Cout); return YS_ERR_UNSUPPORTED; }
  char lab[160] = "";
  if (ys_kprof_enabled()) snprintf(lab, sizeof(lab), "stem6 k66 s2 div1 cin3 cout%d M%ld acc0 tile%dx%d grid%dx1", Cout, (long)B * a.Hout * a.Wout, S6_TH, S6_TW, grid);
  YsKprofScope prof(st, "stem6", lab);           // a class of its own: tests count the launches that took this route
  const bool vec = (W & 3) == 0 && ((size_t)x & 15) == 0;       // aligned float4 rows
#define S6_F(N_) if (nr == N_) { \
    if (eval) { if (vec) YS_LAUNCH((stem6_fwd_kernel<N_, 1, 1>), grid, S6_THREADS, st, a); else YS_LAUNCH((stem6_fwd_kernel<N_, 1, 0>), grid, S6_THREADS, st, a); } \
    else { if (vec) YS_LAUNCH((stem6_fwd_kernel<N_, 0, 1>), grid, S6_THREADS, st, a); else YS_LAUNCH((stem6_fwd_kernel<N_, 0, 0>), grid, S6_THREADS, st, a); } \
    return YS_OK; }
  S6_F(1) S6_F(2) S6_F(3) S6_F(4) S6_F(5)
#undef S6_F
  return YS_ERR_UNSUPPORTED;
}

// ------------------------------------------------------------------------------------------------------------------ weight gradient
// dW[cout][k] = sum over output pixels of dy[pixel][cout] * x[c][2 oy + kh - 2][2 ox + kw - 2].  The MFMA's K dimension is 32 consecutive pixels of one output
// row, so both operands want eight CONSECUTIVE pixels per lane:
//  * x: patch column 2 ox + kw of consecutive ox is a unit-stride run of the column-parity plane kw & 1, starting at entry ox + (kw >> 1).  Each parity plane is
//    kept three times, shifted by 0 / 1 / 2 entries, so that every 16-byte fragment read starts at entry 8 q of its copy: six planes [60][40] bf16, plane
//    (parity, shift) entry i = patch column 2 (i + shift) + parity.
//  * dy: the tile's rows [256 pixels][Cout] sit in LDS as they are in memory; a lane gathers its output channel's eight pixels.
// A workgroup accumulates its tiles in registers and leaves ONE partial slab [Cout][36][8] (the generic kernel's split layout, so the batched split reduction
// of the backward segment takes it as it is).
struct Stem6WgArgs {
  const float* x;
  const bf16_t* dy;          // [B][dy_bstride][dy_ldc] + dy_coff
  float* partial;            // [gridDim.x][Cout][36][8]
  int B, H, W, Hout, Wout, Cout, dy_ldc, dy_coff;
  long dy_bstride;
  int tiles_x, tiles_y, ntiles;
};

template <int NR, int VEC>
__global__ void __launch_bounds__(S6_THREADS)
stem6_wgrad_kernel(Stem6WgArgs a) {
  constexpr int PL = 40;                                // plane row pitch (entries): a multiple of 8 -> aligned 16-byte reads
  constexpr int PLANE = S6_ROWS * PL;                   // 2400 entries = 4800 bytes
  constexpr int DP = NR * 16 + 2;                       // dy row pitch in LDS (entries)
  // one (dynamic: 37 - 69 KB) LDS block of stem6_wgrad_lds(NR) bytes: the six planes, then the dy rows.  After the last tile its head becomes the cross-wave
  // reduction scratch [4][7][64][4] floats (28672 bytes <= the planes' 28800)
  constexpr int X_BYTES = 6 * PLANE * 2, RED_BYTES = 4 * S6_KB * 64 * 16;
  static_assert(RED_BYTES <= X_BYTES, "reduction scratch must fit the planes");
  YS_DYN_LDS(sMem);
  unsigned short* sX = (unsigned short*)sMem;           // plane (parity, shift) at sX + (parity * 3 + shift) * PLANE
  unsigned short* sDy = sX + 6 * PLANE;                 // 6 * PLANE * 2 bytes is a multiple of 16
  float* sRed = (float*)sMem;                           // [wave][kb][lane][4]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, q = lane >> 4;

  // this lane's column of the B operand: k = kb * 16 + li -> (c, kh, kw) -> plane copy and row offset; k >= 108: a zero fragment
  int boff[S6_KB];
#pragma unroll
  for (int kb = 0; kb < S6_KB; kb++) {
    const int k = kb * 16 + li;
    const int c = k / 36, tap = k - c * 36;
    const int kh = tap / 6, kw = tap - kh * 6;
    boff[kb] = k < 108 ? ((kw & 1) * 3 + (kw >> 1)) * PLANE + (c * S6_PH + kh) * PL : -1;
  }
  f32x4 acc[NR][S6_KB];
#pragma unroll
  for (int nf = 0; nf < NR; nf++)
#pragma unroll
    for (int kb = 0; kb < S6_KB; kb++) acc[nf][kb] = f32x4_zero();

  // one patch value into the three shifted copies of its parity plane (entries that fall before a copy's start do not exist)
  auto put = [&](int row, int col, unsigned short h) {
    unsigned short* p = sX + (col & 1) * 3 * PLANE + row * PL + (col >> 1);
    p[0] = h;
    if (col >= 2) p[PLANE - 1] = h;
    if (col >= 4) p[2 * PLANE - 2] = h;
  };

  // dy rows of a tile: 256 pixels x NR*16 channels, 16-byte units (8 channels), zero outside the image
  constexpr int DU = S6_TH * S6_TW * NR * 2;      // 16-byte units of the tile
  constexpr int NDU = (DU + S6_THREADS - 1) / S6_THREADS;
  float v[S6_NLD];                            // (the form not taken is dead code: VEC is a template parameter)
  S6PatchV pv;
  uint4 dv[NDU];
  auto fetch_tile = [&](int t) {              // everything tile t needs from memory, all loads back to back
    int b, oy0, ox0;
    s6_tile_origin(t, a.tiles_x, a.tiles_y, b, oy0, ox0);
    if (VEC) s6_patch_fetch_v(a.x, b, 2 * oy0 - 2, 2 * ox0 - 2, a.H, a.W, pv);
    else s6_patch_fetch(a.x, b, 2 * oy0 - 2, 2 * ox0 - 2, a.H, a.W, v);
#pragma unroll
    for (int k = 0; k < NDU; k++) {
      const int u = tid + S6_THREADS * k;
      const int px = u / (NR * 2), cu = u - px * (NR * 2);
      const int oyl = px / S6_TW, oxl = px - oyl * S6_TW;
      const int oy = oy0 + oyl, ox = ox0 + oxl;
      const bool ok = (bool)((int)(u < DU) & (int)(oy < a.Hout) & (int)(ox < a.Wout) & (int)(cu * 8 < a.Cout));
      const long off = ok ? (((long)b * a.dy_bstride + (long)oy * a.Wout + ox) * a.dy_ldc + a.dy_coff + cu * 8) : 0;
      const uint4 t4 = *(const uint4*)(a.dy + off);
      dv[k] = ok ? t4 : ys_zero16();
    }
  };
  // the NEXT tile's operands are requested as soon as the current ones sit in LDS (as in stem_wgrad_kernel)
  if ((int)blockIdx.x < a.ntiles) fetch_tile(blockIdx.x);
  for (int tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
    __syncthreads();                          // barrier A: every wave is through the previous tile's fragment reads before the planes / dy rows are overwritten
    if (VEC) {
#pragma unroll
      for (int k = 0; k < S6_NVL; k++) {
        const int u = tid + S6_THREADS * k;
        if (u < S6_NVEC) {
          const int row = u / S6_VPR, col = 2 + 4 * (u - row * S6_VPR);
          put(row, col, Elem<bf16_t>::from_f(pv.v[k].x).v); put(row, col + 1, Elem<bf16_t>::from_f(pv.v[k].y).v);
          put(row, col + 2, Elem<bf16_t>::from_f(pv.v[k].z).v); put(row, col + 3, Elem<bf16_t>::from_f(pv.v[k].w).v);
        }
      }
      if (tid < S6_ROWS) { put(tid, 0, Elem<bf16_t>::from_f(pv.h.x).v); put(tid, 1, Elem<bf16_t>::from_f(pv.h.y).v); }
    } else {
#pragma unroll
      for (int k = 0; k < S6_NLD; k++) {
        const int e = tid + S6_THREADS * k;
        if (e < S6_NPATCH) { const int row = e / S6_PW; put(row, e - row * S6_PW, Elem<bf16_t>::from_f(v[k]).v); }
      }
    }
#pragma unroll
    for (int k = 0; k < NDU; k++) {
      const int u = tid + S6_THREADS * k;
      if (u < DU) {
        const int px = u / (NR * 2), cu = u - px * (NR * 2);
        unsigned* d = (unsigned*)(sDy + px * DP + cu * 8);     // DP is even: 4-byte aligned
        d[0] = dv[k].x; d[1] = dv[k].y; d[2] = dv[k].z; d[3] = dv[k].w;
      }
    }
    if (tile + (int)gridDim.x < a.ntiles) fetch_tile(tile + gridDim.x);
    __syncthreads();                          // barrier B: planes and dy rows of this tile are complete
    // wave w: output rows 2w, 2w + 1 of the tile; one K = 32 step per row
#pragma unroll
    for (int rr = 0; rr < 2; rr++) {
      const int oyl = 2 * wave + rr;
      uint4 xf[S6_KB];
#pragma unroll
      for (int kb = 0; kb < S6_KB; kb++) {
        const uint4 t = *(const uint4*)(sX + (boff[kb] < 0 ? 0 : boff[kb]) + (2 * oyl) * PL + q * 8);
        xf[kb] = boff[kb] < 0 ? ys_zero16() : t;
      }
#pragma unroll
      for (int nf = 0; nf < NR; nf++) {
        const unsigned short* dp = sDy + (oyl * S6_TW + q * 8) * DP + nf * 16 + li;
        unsigned short e[8];
#pragma unroll
        for (int j = 0; j < 8; j++) e[j] = dp[j * DP];
        const uint4 df = make_uint4((unsigned)e[0] | ((unsigned)e[1] << 16), (unsigned)e[2] | ((unsigned)e[3] << 16),
                                    (unsigned)e[4] | ((unsigned)e[5] << 16), (unsigned)e[6] | ((unsigned)e[7] << 16));
#pragma unroll
        for (int kb = 0; kb < S6_KB; kb++) acc[nf][kb] = ys_mma<bf16_t>(df, xf[kb], acc[nf][kb]);
      }
    }
  }
  // The four waves' accumulators, summed in a fixed order -> this workgroup's slab, sixteen output channels (one nf) at a time.  Lane (li, q) holds
  // D[cout = nf * 16 + 4q + r][k = kb * 16 + li].  The scratch aliases the planes:
  //   barrier C (top of each round) -- round 0: every wave is through its last fragment reads of the tile loop before the planes are overwritten (the race class of
  //     the 3x3 kernel's round 5); later rounds: every thread is through the previous round's scratch reads before the next sums are written;
  //   barrier D -- the four waves' sums of this round are in the scratch before any thread adds them up.
  float* slab = a.partial + (long)blockIdx.x * a.Cout * 288;
#pragma unroll
  for (int nf = 0; nf < NR; nf++) {
    __syncthreads();                          // barrier C
#pragma unroll
    for (int kb = 0; kb < S6_KB; kb++)
#pragma unroll
      for (int r = 0; r < 4; r++) sRed[((wave * S6_KB + kb) * 64 + lane) * 4 + r] = acc[nf][kb][r];
    __syncthreads();                          // barrier D
    for (int o = tid; o < 16 * 288; o += S6_THREADS) {
      const int cl = o / 288, rem = o - cl * 288;
      const int tap = rem >> 3, c = rem & 7;
      const int co = nf * 16 + cl;
      float s = 0.f;
      if (c < 3) {
        const int k = c * 36 + tap;
        const int kb = k >> 4, l = (k & 15) + 16 * (cl >> 2), r = cl & 3;
        const float* p = sRed + ((long)kb * 64 + l) * 4 + r;
        constexpr int WS = S6_KB * 64 * 4;        // one wave's sums
        s = (p[0] + p[WS]) + (p[2 * WS] + p[3 * WS]);
      }
      if (co < a.Cout) slab[(long)co * 288 + rem] = s;
    }
  }
}

static size_t stem6_wgrad_lds(int nr) { return (size_t)6 * S6_ROWS * 40 * 2 + (size_t)S6_TH * S6_TW * (nr * 16 + 2) * 2; }

template <int NR, int VEC>
static void stem6_wgrad_launch_t(hipStream_t st, int grid, const Stem6WgArgs& a) {
  const size_t lds = stem6_wgrad_lds(NR);
#ifndef YS_EMU_BUILD
  if (lds > 64 * 1024) {       // Cout = 80: above the default dynamic-LDS limit.  Per device: the attribute belongs to the device's code object
    static std::atomic<unsigned> attr_done{0};
    int dev_id = 0;
    (void)hipGetDevice(&dev_id);
    if (!(attr_done.load(std::memory_order_relaxed) & (1u << (dev_id & 31)))) {
      hipFuncSetAttribute((const void*)stem6_wgrad_kernel<NR, VEC>, hipFuncAttributeMaxDynamicSharedMemorySize, 80 * 1024);
      attr_done.fetch_or(1u << (dev_id & 31), std::memory_order_relaxed);
    }
  }
#endif
  YS_LAUNCH_LDS((stem6_wgrad_kernel<NR, VEC>), grid, S6_THREADS, lds, st, a);
}

// partial slabs the weight-gradient launch wants for this shape (it never writes more than the caller's max_splits)
int ys_stem6_wgrad_splits(int B, int H, int W) {
  const long ntiles = (long)B * ys_cdiv(s6_hout(H), S6_TH) * ys_cdiv(s6_hout(W), S6_TW);
  return (int)(ntiles < 1024 ? ntiles : 1024);
}

// writes min(max_splits, 1024, tiles) partial slabs [Cout][36][8] into `partial`; *used = the number written
int ys_stem6_wgrad_launch(hipStream_t st, const float* x, int B, int H, int W, const void* dy, int dy_ldc, int dy_coff, long dy_bstride,
                          int Cout, float* partial, int max_splits, int* used) {
  Stem6WgArgs a{};
  a.x = x; a.dy = (const bf16_t*)dy; a.partial = partial;
  a.B = B; a.H = H; a.W = W; a.Hout = s6_hout(H); a.Wout = s6_hout(W); a.Cout = Cout;
  a.dy_ldc = dy_ldc; a.dy_coff = dy_coff; a.dy_bstride = dy_bstride;
  if (B < 1 || H < 2 || W < 2 || (long)B * 3 * H * W >= (1L << 31) || (dy_ldc & 7) || (dy_coff & 7) || max_splits < 1) { ys_set_error("stem6 wgrad: unsupported view"); return YS_ERR_UNSUPPORTED; }
  a.tiles_x = ys_cdiv(a.Wout, S6_TW); a.tiles_y = ys_cdiv(a.Hout, S6_TH); a.ntiles = B * a.tiles_x * a.tiles_y;
  int grid = ys_stem6_wgrad_splits(B, H, W);
  if (grid > max_splits) grid = max_splits;
  if (used) *used = grid;
  const int nr = Cout / 16;
  if (Cout % 16 || nr < 1 || nr > 5) { ys_set_error("stem6 wgrad: %d output channels", Cout); return YS_ERR_UNSUPPORTED; }
  char lab[160] = "";
  if (ys_kprof_enabled()) snprintf(lab, sizeof(lab), "wstem6 k6 s2 cin3 cout%d M%ld tile%dx%d grid%dx1", Cout, (long)B * a.Hout * a.Wout, S6_TH, S6_TW, grid);
  YsKprofScope prof(st, "stem6_wg", lab);        // a class of its own, like "stem6"
  const bool vec = (W & 3) == 0 && ((size_t)x & 15) == 0;
#define S6_W(N_) if (nr == N_) { if (vec) stem6_wgrad_launch_t<N_, 1>(st, grid, a); else stem6_wgrad_launch_t<N_, 0>(st, grid, a); return YS_OK; }
  S6_W(1) S6_W(2) S6_W(3) S6_W(4) S6_W(5)
#undef S6_W
  return YS_ERR_UNSUPPORTED;
}
