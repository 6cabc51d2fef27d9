// conv_p2.h -- conv_p2_kernel / conv_p2_group_kernel, the whole-Cin LDS patch convolution of the bf16 path ("P2"): the device side, the host plan
// record and the functions its translation units share.  conv_p2_plan.hip plans (no kernels); conv_p2.hip (plain bf16) and conv_p2_f8.hip (fp8, and bf16 with
// the fused BN-backward reduction) hold the single-launch instances (conv_p2_launch.h); conv_p2_group.hip the grouped ones; conv.hip routes to them (conv_route).
#pragma once
#include "ys_internal.h"
#include "ys_kernels.h"

// ===================================================================================== 3x3, bf16: whole-Cin LDS patch ("P2")
// Round-1 follow-up of the chunked patch kernel (conv.hip conv3x3_tile_kernel) for bf16 (the f32 parity path keeps the chunked kernel).  Differences:
//  * the patch holds ALL input channels of the tile (+halo) in natural NHWC rows, so a tile needs one load phase and one
//    barrier pair instead of two barriers per 32-channel chunk;
//  * K runs over (tap, channel) in steps of 32 regardless of Cin (Cin = 16 packs two taps into one MFMA); the LDS offset
//    of every (K-step, q) fragment is tile-independent and comes from a small table built once per workgroup, and each
//    lane's pixel offsets are computed once per kernel -> the inner loop is 1 table read + adds + ds_read_b128 + MFMA;
//  * small weight sets stay resident (persistent grid); large ones stream through a double-buffered LDS ring, one barrier
//    per K-group, so the footprint stays <= ~75 KB and two workgroups share a CU (one loads while the other computes);
//  * 256 threads, <= 128 VGPRs: register pressure no longer caps occupancy.
// Handles forward (stride 1 and 2) and stride-1 dgrad (same gather, flipped weights); DIV = 2 dgrads stay on the old path.
#include "conv_epi.h"
constexpr int YS_EPI_BATCH_P2 = 4;   // store-loop iterations whose accumulate operands p2_epilogue requests ahead (BMAX): what the register budget affords

// ablation switches (YS_DBG bits) cost scalar checks in the hot loops: compiled in only for triage builds (-DYS_P2_ABLATE)
#ifdef YS_P2_ABLATE
#define P2_DBG(bit) ((a.dbg & (bit)) != 0)
#else
#define P2_DBG(bit) false
#endif
constexpr int P2_KG = 2;   // K-steps (32 K each) per streamed weight group
#define P2_NPU 12          // max patch units (16 B) a thread keeps in flight: 12 x 256 x 16 B = 48 KB per workgroup (small layers: 6)
struct P2Tag0 { static constexpr int value = 0; };
struct P2Tag1 { static constexpr int value = 1; };
// K-steps per register group of the pipelined K loop: enough MFMAs per group (>= 8) to cover an LDS round trip
// G K-steps share one LDS wait: about 16 MFMAs per group, so that a group's MFMA time matches the LDS round trip the SIMD's other
// waves have to cover -- bounded by the fragment registers a group keeps live, 4 * G * (MR + NR): <= 64 in the 256-register
// variants, <= 32 in the `tight` ones (compiled for three waves per SIMD, 168 registers).  G is 1, 2 or 4 (one table read).
__host__ __device__ constexpr int p2_reg_group(int mr, int nr, bool tight = false) {
  const int want = mr * nr >= 10 ? 1 : (mr * nr >= 6 ? 2 : 4);
  const int cap = (tight ? 8 : 16) / (mr + nr);
  const int g = want < cap ? want : cap;
  return g >= 4 ? 4 : (g >= 2 ? 2 : 1);
}
struct P2Args {
  int TH, TW, tiles_x, tiles_y, ntiles, PH, PW;
  int ppb;       // patch pixel pitch (bytes)
  int prb;       // patch row pitch (bytes) = PW * ppb + row padding (p2_pick_rowpad)
  int wpitch;    // weight row pitch in LDS (16-byte units)
  int nsteps;    // K-steps (32 K each) = ceil(KH*KW*Cin / 32)
  int nsp;       // row length of the q-major offset table [4][nsp]: nsteps rounded up to 4, plus slack for the pipelined over-read
  int kg;        // K-steps per streamed weight group
  int off_w, off_p, off_stat;   // LDS byte offsets (offset table sits at 0)
  unsigned xbytes;              // bytes of the input view from its first channel to the end of the last image (descriptor range, < 2^31)
};

// F8 = 1: fp8 mode.  Global activations stay bf16 (same HBM bytes); the patch is quantised to fp8 (e4m3, or e5m2 for a
// gradient input) with a per-tensor scale as it is written to LDS, the weights arrive pre-quantised (e4m3), and the K loop
// runs v_mfma_scale_f32_16x16x128_f8f6f4 with unit block scales: 128 K per instruction at twice the bf16 MFMA rate, and half
// the LDS bytes per K (the K loop of this kernel is LDS-bandwidth-bound for small register tiles).  A K-step is then 128 K =
// four 32-channel pieces (one per lane quarter); Cin % 32 == 0.  The fp32 accumulators are scaled back in the epilogue.
// RED = 1: dgrad launches that also take the BN-backward sums of the producers whose gradient they complete (conv_epi.h, BnRedSeg)
// The kernel body takes its workgroup index and grid size as arguments (vbx of vgx): conv_p2_kernel passes blockIdx.x / gridDim.x,
// conv_p2_group_kernel (below) the workgroup's index inside the problem its blockIdx.x range belongs to.
template <int MR, int NR, int WRES, int NPU, int NT, int F8, int RED = 0>
__device__ __forceinline__ void conv_p2_body(const ConvArgs& a, const P2Args& g, const int* __restrict__ tab, const int vbx, const int vgx) {
  typedef bf16_t T;
  constexpr int WES = F8 ? 1 : 2;             // bytes per weight element
  constexpr int UPS = F8 ? 8 : 4;             // 16-byte LDS units per weight row and K-step
  if (P2_DBG(64)) return;                     // ablation: launch + dispatch cost only
  constexpr int BN = NR * 16;
  constexpr int NWV = NT / 64;
#ifdef YS_P2_TIMELINE
  // s_memtime stamps of wave 0 / lane 0 of every 37th workgroup: [slot 0] entry, [1] prologue issued, then per tile
  // (top, patch in LDS, MFMA loop done, epilogue done), last = exit.  64 slots per recorded workgroup.
  int tl_n = 0;
  unsigned long long* tl_p = (a.tl && (vbx % 37) == 0 && blockIdx.y == 0 && threadIdx.x == 0) ? a.tl + (vbx / 37) * 64 : nullptr;
#define TL_STAMP() do { if (tl_p && tl_n < 63) tl_p[1 + tl_n++] = __builtin_readcyclecounter(); } while (0)
#ifdef YS_P2_TIMELINE_FINE
#define TL_STAMP2() TL_STAMP()
#else
#define TL_STAMP2() ((void)0)
#endif
#else
#define TL_STAMP() ((void)0)
#define TL_STAMP2() ((void)0)
#endif
  TL_STAMP();
  constexpr int NWU = WRES ? 1 : (BN * P2_KG * UPS + NT - 1) / NT;   // streamed weight units per thread
  YS_DYN_LDS(lds);
  char* lb = (char*)lds;
  int* sOff = (int*)lb;                       // [nsteps][4]
  uint4* sW = (uint4*)(lb + g.off_w);         // WRES: [BN][wpitch]; else [2][BN][wpitch]
  char* sPb = lb + g.off_p;                   // [PH*PW][ppb]
  float* sStat = (float*)(lb + g.off_stat);   // [NWV][BN][2]

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, q = lane >> 4;
  const int n0 = blockIdx.y * BN;
  const char* xb = (const char*)a.x;
  const char* wb = (const char*)(F8 ? a.w8 : a.w);
  const int taps = a.KH * a.KW;
  const int Ktot = taps * a.Cin;
  const int cu = a.Cin >> 3;                  // 16-byte units per patch pixel in GLOBAL memory (bf16)
  const float qs = F8 ? a.qscale[0] : 1.0f;   // quantisation multiplier of the input tensor
  float amx = 0.f;                            // fp8: running amax(|input|) of what this thread stages (next step's scale)
  const int npatch = g.PH * g.PW * cu;

  // ---- tile-independent tables, computed once per layer geometry on the host (p2_tables): per-(quarter, K-step) patch
  // offsets (q-major so that a lane fetches the offsets of consecutive K-steps with one LDS read), per-thread pixel offsets,
  // per-thread patch unit descriptors
  // the offset table goes global -> LDS by DMA as well (nsp 16-byte units, <= 2 requests): the copy through registers made every
  // workgroup wait out one L2 round trip before it could even request its patch
  {
    const ys_rsrc_t rsT = ys_make_rsrc(tab, (unsigned)g.nsp * 16u);
    if (tid < g.nsp) ys_bufld_lds16(rsT, (unsigned)tid * 16u, 0u, lb + wave * 1024);
  }
  const int* tpx = tab + g.nsp * 4;
  int pixbase[MR], pty[MR], ptx[MR], prow[MR];
#pragma unroll
  for (int mf = 0; mf < MR; mf++) {
    pixbase[mf] = tpx[(mf * 4 + 0) * NT + tid];
    pty[mf] = tpx[(mf * 4 + 1) * NT + tid];
    ptx[mf] = tpx[(mf * 4 + 2) * NT + tid];
    prow[mf] = tpx[(mf * 4 + 3) * NT + tid];    // output row of the lane's pixel relative to the tile's first pixel (epilogue)
  }
  constexpr int KG = P2_KG;                    // K-steps per streamed weight group
  constexpr int GU = KG * UPS;                 // 16-byte units per weight row and group
  constexpr bool TIGHT = NT == 256 && NPU <= 6 && MR * NR <= 8 && !F8;                    // 168-register variants
  constexpr int G0 = F8 ? 1 : p2_reg_group(MR, NR, TIGHT);   // fp8: one K-step is already 128 K (32-byte fragments)
  // streamed bf16 weights by DMA leave the dgrad variants (no bias / BatchNorm / residual epilogue paths) room for both K-steps of a weight
  // group per LDS wait: with two waves per SIMD the one-step form is a chain of two LDS round trips per 10-16 MFMAs
  constexpr bool DMAW_G2 = !WRES && !F8 && NT == 256 && RED != 0 && MR * NR <= 12;   // (4 x 4: spills)
  constexpr int G = DMAW_G2 ? KG : ((WRES || G0 < KG) ? G0 : KG);   // K-steps per register group of the K loop
  const int ngroups = WRES ? 1 : (g.nsteps + KG - 1) / KG;
  // (Two round-4 alternatives for the streamed weights, both built, measured on the same box in alternation and dropped, profiles/README.md: weights fetched
  // through registers THREE groups ahead with the next patch requested after the K loop -- grouped head launches 1.00 -> 0.96 ms, plain launches 2.96 -> 3.00,
  // step 9.75 = 9.75: the K loop of the streamed layers is bound by its LDS round trips per K-step, not by the weight fetch; and the dgrad variants' next patch
  // requested inside the epilogue to pay for two K-steps per LDS wait on the 2 x 5 tile -- grouped head launches 0.68 -> 0.67 ms, step 9.51 = 9.51.)
  // DMAW (round 4): streamed bf16 weights by LDS DMA.  A weight group (KG = 2 K-steps = 64 K = 128 bytes per output channel) is BN rows of
  // eight 16-byte units; a wave instruction moves eight rows (1 KB), lane l -> row l / 8, LDS unit l % 8, which holds the row's logical unit
  // (l % 8) ^ ((row / 2) % 8) -- the blocked-GEMM kernel's swizzle: the K loop's fragment reads (16 rows x 4 units) are conflict-free.  Three
  // slots: at group g the workgroup waits for its own requests of g (issued two groups earlier), meets at ONE barrier, requests g + 2 into
  // the slot group g - 1 was read from, and multiplies.  The register form costs 12 registers, three ds_write_b128 and -- the expensive
  // part -- a wait for loads issued only one group (~1 thousand cycles) earlier, per thread and group.
  constexpr bool DMAW = !WRES && !F8 && NT == 256;
  static_assert(!DMAW || (KG == 2 && UPS == 4), "the DMA weight ring hard-codes 128-byte rows per group (two K-steps of four 16-byte units): offsets, slot stride and the host plan's wbytes");
  constexpr int NBP = BN / 8;                  // 1 KB requests per weight group
  constexpr int NPW = (NBP + NWV - 1) / NWV;   // ... per wave (the last round may be partial)
  uint4 rwA[NWU];
  // this thread's (row, unit-in-group) of the streamed weight tile never changes: keep the row's byte offset (32 bits, through a buffer
  // descriptor of the weight shadow: a unit past the row's real K, a row past Cout or an idle thread carries the out-of-range offset and
  // arrives as zeros -- no 64-bit row pointers to keep (they were spilled next to three register sets), no select after the load)
  const ys_rsrcv_t rsWv = ys_make_rsrcv(wb, (unsigned)((long)a.Cout * Ktot * WES));
  unsigned wro[NWU];
  int wun[NWU];
#pragma unroll
  for (int k = 0; k < NWU; k++) {
    const int idx = tid + NT * k;
    const int n = idx / GU;
    wun[k] = (idx < BN * GU && n0 + n < a.Cout) ? idx - n * GU : -1;
    wro[k] = (unsigned)((long)(n0 + (wun[k] >= 0 ? n : 0)) * Ktot * WES);
  }
  auto wfetch = [&](uint4 (&rw)[NWU], int grp) {   // global -> registers: weights of K-steps [grp*KG, grp*KG + KG); unconditional loads
#pragma unroll
    for (int k = 0; k < NWU; k++) {
      const int u = grp * GU + wun[k];
      const bool ok = (bool)((int)(wun[k] >= 0) & (int)(u * (16 / WES) < Ktot) & (int)!P2_DBG(16));
      rw[k] = ys_bufld16(rsWv, ok ? wro[k] + (unsigned)u * 16u : YS_BUF_OOB);
    }
  };
  auto wstore = [&](const uint4 (&rw)[NWU], int buf) {
#pragma unroll
    for (int k = 0; k < NWU; k++) {
      const int idx = tid + NT * k;
      if (idx < BN * GU) { const int n = idx / GU; sW[(buf * BN + n) * g.wpitch + (idx - n * GU)] = rw[k]; }
    }
  };

#ifdef YS_EMU_BUILD
  const int wvu = wave;
#else
  const int wvu = __builtin_amdgcn_readfirstlane(wave);
#endif
  const int nmine = DMAW ? (NBP - wvu + NWV - 1) / NWV : 0;     // requests of this wave per weight group
  const int kunits = Ktot >> 3;
  const ys_rsrc_t rsWd = ys_make_rsrc(wb, (unsigned)((long)a.Cout * Ktot * WES));
  unsigned dro[DMAW ? NPW : 1];
  int dun[DMAW ? NPW : 1];
  if constexpr (DMAW) {
#pragma unroll
    for (int j = 0; j < NPW; j++) {
      const int row = (wvu + NWV * j) * 8 + (lane >> 3);
      dun[j] = (lane & 7) ^ ((row >> 1) & 7);
      dro[j] = (row < BN && n0 + row < a.Cout) ? (unsigned)((long)(n0 + row) * Ktot * 2) + (unsigned)dun[j] * 16u : YS_BUF_OOB;
    }
  }
  auto wdma = [&](int grp, int slot) {           // weight group grp -> ring slot; units past the row's real K, rows past Cout: zeros
    if constexpr (DMAW) {
#pragma unroll
      for (int j = 0; j < NPW; j++)
        if (wvu + NWV * j < NBP) {
          const bool ok = (bool)((int)(grp * 8 + dun[j] < kunits) & (int)!P2_DBG(16));
          ys_bufld_lds16(rsWd, ok ? dro[j] : YS_BUF_OOB, (unsigned)grp * 128u, (char*)sW + slot * (BN * 128) + (wvu + NWV * j) * 1024);
        }
    }
  };
  const int wko0 = (q ^ ((li >> 1) & 3)) * 16 + ((((li >> 1) & 7) >> 2) << 6);   // ring slot: byte offset of (K-step 0, quarter q) in this lane's rows

  // ---- patch of a tile: global -> registers (all loads back-to-back); the NEXT tile's patch is in flight while the
  // current one is consumed, so every resident workgroup always has a whole patch outstanding (HBM needs ~40 KB per CU
  // in flight to reach its bandwidth).  Per patch unit a thread keeps two tile-independent words: the element offset from
  // the tile's patch origin in global memory, and (row, column, LDS slot) packed -- so a tile costs an add, two compares
  // and a shift per unit instead of divisions and multiplies.
  uint4 rp[NPU];
  unsigned pdesc[NPU];                      // patch row (9 bits) | patch column (10) | LDS offset / 16 (13)
  int goff[NPU];                            // (row * Win + column) * in_ldc + unit * 8
  {
    const int* tpd = tpx + MR * 4 * NT;
#pragma unroll
    for (int k = 0; k < NPU; k++) {
      pdesc[k] = (unsigned)tpd[(2 * k + 0) * NT + tid];
      goff[k] = tpd[(2 * k + 1) * NT + tid];
    }
  }
  // Tile order.  Workgroup i runs on XCD i % 8 (round-robin dispatch); when the grid is a multiple of 8 each XCD walks its own
  // contiguous eighth of the tile list, so the tiles resident on an XCD at any time are spatial neighbours and their shared
  // halo rows hit that XCD's L2.  Otherwise plain interleaving.  Tile coordinates advance incrementally (no per-tile divisions).
  const bool xcd_order = (vgx & 7) == 0 && !P2_DBG(32);
  const int t_per_xcd = (g.ntiles + 7) >> 3;
  const int t_step = xcd_order ? (vgx >> 3) : vgx;
  const int t_first = xcd_order ? (vbx & 7) * t_per_xcd + (vbx >> 3) : vbx;
  const int t_end = xcd_order ? (((vbx & 7) + 1) * t_per_xcd < g.ntiles ? ((vbx & 7) + 1) * t_per_xcd : g.ntiles) : g.ntiles;
  int stx, sty, sb;
  {
    const int G = t_step;
    stx = G % g.tiles_x; const int rem = G / g.tiles_x;
    sty = rem % g.tiles_y; sb = rem / g.tiles_y;
  }
  auto advance = [&](int& txi, int& tyi, int& b) {
    txi += stx; if (txi >= g.tiles_x) { txi -= g.tiles_x; tyi++; }
    tyi += sty; if (tyi >= g.tiles_y) { tyi -= g.tiles_y; b++; }
    b += sb;
  };
  // Every unit issues its load unconditionally (loads inside exec-masked branches make the compiler lose count of what is in
  // flight and fall back to s_waitcnt vmcnt(0) BEFORE the MFMA loop, i.e. no overlap).  The loads go through a buffer descriptor
  // of the input view: a unit that is unused or falls into the zero padding gets the out-of-range offset and the hardware
  // returns zeros -- one 32-bit add and one select per unit instead of a 64-bit address, a 64-bit select against a safe address
  // and a second select when the patch is written to LDS.
  const ys_rsrcv_t rsP = ys_make_rsrcv(xb + (long)a.in_coff * 2L, g.xbytes);
  auto pfetch = [&](int txi, int tyi, int b) -> unsigned {
    const int iy0 = tyi * g.TH * a.SA - a.PAD, ix0 = txi * g.TW * a.SA - a.PAD;
    const int toff = (int)((((long)b * a.in_bstride + (long)iy0 * a.Win + ix0) * a.in_ldc) * 2L);   // may be negative for a tile on the border: only valid units use it
    unsigned okm = 0;
#pragma unroll
    for (int k = 0; k < NPU; k++) {
      unsigned d = pdesc[k];
      int go = goff[k];
#ifndef YS_EMU_BUILD
      asm volatile("" : "+v"(d), "+v"(go));
#endif
      // branch-free validity (bitwise, not short-circuit): unit in use, row and column inside the image
      const unsigned iy = (unsigned)(iy0 + (int)(d >> 23)), ix = (unsigned)(ix0 + (int)((d >> 13) & 1023u));
      const bool ok = (bool)((int)(d != 0xffffffffu) & (int)(iy < (unsigned)a.Hin) & (int)(ix < (unsigned)a.Win) & (int)!P2_DBG(1));
      rp[k] = ys_bufld16(rsP, ok ? (unsigned)(toff + go * 2) : YS_BUF_OOB);
      okm |= (unsigned)ok << k;
    }
    return okm;
  };
  int txi, tyi, b;
  {
    int t = t_first;
    txi = t % g.tiles_x; t /= g.tiles_x;
    tyi = t % g.tiles_y; b = t / g.tiles_y;
  }
  int ntx = txi, nty = tyi, nb = b;
  unsigned okm_next = 0;
  TL_STAMP();                                            // tables requested
  if (t_first < t_end) okm_next = pfetch(txi, tyi, b);   // the first patch is in flight while the weights are staged
  TL_STAMP();                                            // first patch requested
  if (WRES) {
    // resident weights: rows padded with zeros to a multiple of 4 K-steps (the pipelined K loop runs whole register groups).
    // LDS DMA (buffer_load ... lds, 1 KB per wave instruction): all of a wave's requests are in flight at once and no VGPR is
    // touched.  The register form -- eight loads, then eight LDS stores, per round -- was 4-8 thousand cycles of every workgroup's
    // ~10 thousand cycle prologue (s_memtime stamps, round 3).  LDS slot j of the weight region is (row j / wpitch, unit j % wpitch);
    // units past the real K (zero padding of the row, the pitch's spare slots) and rows past Cout carry the out-of-range offset =
    // zeros.  The region is rounded up to whole 1 KB requests by the plan.
    const int per_row = ((g.nsteps + 3) & ~3) * UPS;
    const int nslots = BN * g.wpitch;
    const ys_rsrc_t rsW = ys_make_rsrc(wb, (unsigned)((long)a.Cout * Ktot * WES));
    int n = tid / g.wpitch, u = tid - n * g.wpitch;
    const int dn = NT / g.wpitch, du = NT - dn * g.wpitch;       // one round of the workgroup = NT slots further
    char* dst = (char*)sW + wave * 1024;
    for (int j = wave * 64; j < nslots; j += NT) {
      const bool ok = (bool)((int)(u < per_row) & (int)(u * (16 / WES) < Ktot) & (int)(n0 + n < a.Cout) & (int)!P2_DBG(16));
      ys_bufld_lds16(rsW, ok ? (unsigned)((long)(n0 + n) * Ktot * WES) + (unsigned)u * 16u : YS_BUF_OOB, 0u, dst);
      dst += NT * 16;
      n += dn; u += du;
      if (u >= g.wpitch) { u -= g.wpitch; n++; }
    }
  }
  TL_STAMP();
  if (P2_DBG(128)) return;                     // ablation: prologue only (tables, resident weights, first patch fetch)
  float st1[8], st2[8];                        // BN statistics of this workgroup's tiles (per-lane column sums)
#pragma unroll
  for (int e = 0; e < 8; e++) { st1[e] = 0.f; st2[e] = 0.f; }

  // Counted waits (round 4).  vmcnt counts loads AND stores on this part and retires them in issue order.  The tile loop used to open
  // with s_waitcnt vmcnt(0): besides the prefetched patch that also drained the previous tile's output stores, which a CU retires at
  // 7-10 bytes per clock -- about two thousand cycles for a 16 KB tile, every tile, with nothing of this workgroup overlapping it (the
  // "patch in LDS" phase of the round-3 stamps: 3.4-3.6 thousand cycles whatever the epilogue form).  The patch loads are issued BEFORE
  // the epilogue, so "at most NST operations outstanding", NST = the epilogue's store instructions per wave (a static count: the stores
  // are unconditional, masked lanes carry the out-of-range offset), means the patch has landed while the stores keep draining under the
  // LDS writes, the next prefetch and the K loop.  Anything else the epilogue issued (accumulate / residual / y loads) only makes the
  // number outstanding larger, i.e. the wait longer -- never too short.  The weight / table DMA (inline asm, invisible to the
  // compiler) is waited for once, in front of the loop.  This relies on loads and stores retiring in issue order on the shared counter -- what hipcc's own
  // wait insertion assumes on gfx9-family parts.  (Suspected and withdrawn once in round 4 when the config-5 determinism test failed with it; the bisection,
  // profiles/README.md, cleared it: the cause was packed-FP32 statistics, and with -fno-slp-vectorize the combination is stable in 8 / 8 model-level rounds.)
  constexpr int NST = p2_epi_stores(MR, NR);
  YS_WAIT_VM0();
  for (int tile = t_first; tile < t_end; tile += t_step) {
    const int oy0 = tyi * g.TH, ox0 = txi * g.TW;
    TL_STAMP();
    ys_wait_vm<NST>();                        // this tile's patch has landed (the previous tile's stores may still be in flight)
    TL_STAMP2();
    ys_barrier_lds();                         // previous tile's epilogue staging (patch region) and tables are settled
    TL_STAMP2();
    if (!WRES && !DMAW) wfetch(rwA, 0);
#pragma unroll
    for (int k = 0; k < NPU; k++) {
      unsigned d = pdesc[k];
#ifndef YS_EMU_BUILD
      asm volatile("" : "+v"(d));
#endif
      if (F8) {
        if (d != 0xffffffffu && !P2_DBG(8)) {
          uint2 v8; v8.x = 0u; v8.y = 0u;
          if ((okm_next >> k) & 1u) {
            float f[8];
            ys_unpack<T>(rp[k], f);
#pragma unroll
            for (int e = 0; e < 8; e++) { amx = fmaxf(amx, fabsf(f[e])); f[e] *= qs; }
            v8 = a.f8 == 2 ? ys_pack_f8x8<1>(f) : ys_pack_f8x8<0>(f);
          }
          *(uint2*)(sPb + ((d & 8191u) << 3)) = v8;
        }
      } else {
        if (d != 0xffffffffu && !P2_DBG(8)) *(uint4*)(sPb + ((d & 8191u) << 4)) = rp[k];     // padding units arrived as zeros
      }
    }
    if (!WRES && !DMAW) wstore(rwA, 0);
    ys_barrier_lds();
    TL_STAMP();
    advance(ntx, nty, nb);
    // everything older (the patch just consumed, the previous epilogue's conditional loads / stores) has already been waited
    // for above; saying so explicitly resets the compiler's "may still be in flight" state for the accumulator registers
    ys_wait_vm<NST>();                        // (without it -- the epilogue's stores are unconditional now -- the class is 3 % slower: 5.10 -> 5.25 ms)
    const bool more = tile + t_step < t_end;
    if constexpr (DMAW) { wdma(0, 0); if (ngroups > 1) wdma(1, 1); }   // BEFORE the patch requests: the first groups' waits then leave the patch in flight
    if (more) okm_next = pfetch(ntx, nty, nb);

    // resident weights: the accumulators start as the first K-step's products (MFMA with a zero C operand -- an inline constant, no
    // registers cleared: 4 * MR * NR v_mov per tile in a kernel whose busiest pipe is the VALU); streamed weights enter the K loop
    // once per weight group and keep the cleared accumulators
    f32x4 acc[MR][NR];
    if (!WRES || F8) {                        // (fp8 variants keep the cleared accumulators: peeling their 128-deep first group costs them registers)
#pragma unroll
      for (int mf = 0; mf < MR; mf++)
#pragma unroll
        for (int nf = 0; nf < NR; nf++) acc[mf][nf] = f32x4_zero();
    }

    // ---- K loop in register groups of G K-steps.  The one-step-at-a-time form (table read -> wait -> operand reads -> wait ->
    // MFMAs) cost ~350 cycles per K-step whatever the number of MFMAs in it (s_memtime stamps: 90-180 cycles per MFMA against 16
    // of issue time): two dependent LDS round trips per step with only 2-3 waves per SIMD to cover them.  Now one LDS wait serves
    // G steps (about 16 MFMAs), and the next group's table entries are fetched while the MFMAs issue, so the chain per group is
    // one round trip + the MFMAs -- which the SIMD's other waves overlap.  (Double-buffered fragment sets cost 50-100 registers
    // and spilled in most variants.)  Reads past the last real step land in valid LDS; their weights are zero.
    constexpr int FU = F8 ? 2 : 1;             // 16-byte reads per fragment
    struct Frags { uint4 w[G][NR][FU]; uint4 x[G][MR][FU]; };
    auto read_offs = [&](int (&off)[G], int s) {
      const int* pq = sOff + q * g.nsp + s;
      if (G == 4) { const uint4 v = *(const uint4*)pq; off[0] = (int)v.x; off[G > 1 ? 1 : 0] = (int)v.y; off[G > 2 ? 2 : 0] = (int)v.z; off[G > 3 ? 3 : 0] = (int)v.w; }
      else if (G == 2) { const uint2 v = *(const uint2*)pq; off[0] = (int)v.x; off[G > 1 ? 1 : 0] = (int)v.y; }
      else off[0] = pq[0];
    };
    // ng register groups starting at table step sbase, weight units from 0 in wbuf
    auto kloop = [&](const uint4* wbuf, int sbase, int ng, auto bf8_tag) {
      constexpr int B_BF8 = decltype(bf8_tag)::value;
      if (P2_DBG(2)) {                          // ablation build only: no K loop, defined accumulators
        if (WRES && !F8) {
#pragma unroll
          for (int mf = 0; mf < MR; mf++)
#pragma unroll
            for (int nf = 0; nf < NR; nf++) acc[mf][nf] = f32x4_zero();
        }
        return;
      }
      int off[G];
      read_offs(off, sbase);
      auto group = [&](const int gi, auto first_tag) {
        constexpr bool FIRST = decltype(first_tag)::value != 0;   // the tile's first group: C = 0 for its first K-step
        Frags f;
#pragma unroll
        for (int gs = 0; gs < G; gs++) {
#pragma unroll
          for (int nf = 0; nf < NR; nf++)
#pragma unroll
            for (int h = 0; h < FU; h++) {
              if constexpr (DMAW) f.w[gs][nf][h] = *(const uint4*)((const char*)wbuf + (nf * 16 + li) * 128 + (wko0 ^ (((gi * G + gs) & 1) << 6)));
              else f.w[gs][nf][h] = wbuf[(nf * 16 + li) * g.wpitch + ((gi * G + gs) * 4 + q) * FU + h];
            }
#pragma unroll
          for (int mf = 0; mf < MR; mf++)
#pragma unroll
            for (int h = 0; h < FU; h++) f.x[gs][mf][h] = *(const uint4*)(sPb + pixbase[mf] + off[gs] + h * 16);
        }
        read_offs(off, sbase + (gi + 1) * G);
        YS_SCHED_FENCE();                        // every read of the group is issued before its first MFMA
#pragma unroll
        for (int gs = 0; gs < G; gs++)
#pragma unroll
          for (int nf = 0; nf < NR; nf++)
#pragma unroll
            for (int mf = 0; mf < MR; mf++) {
              const f32x4 c0 = (FIRST && gs == 0) ? f32x4_zero() : acc[mf][nf];
              if (F8) acc[mf][nf] = mfma_scale_16x16x128_f8<B_BF8>(f.w[gs][nf][0], f.w[gs][nf][FU - 1], f.x[gs][mf][0], f.x[gs][mf][FU - 1], c0);
              else acc[mf][nf] = ys_mma<T>(f.w[gs][nf][0], f.x[gs][mf][0], c0);
            }
      };
      int gi0 = 0;
      if (WRES && !F8) { group(0, P2Tag1{}); gi0 = 1; }
#pragma unroll 1
      for (int gi = gi0; gi < ng; gi++) group(gi, P2Tag0{});
    };
    const bool in_bf8 = F8 && a.f8 == 2;      // uniform: the input operand is a gradient quantised to e5m2
    if (WRES) {
      if (in_bf8) kloop(sW, 0, (g.nsteps + G - 1) / G, P2Tag1{}); else kloop(sW, 0, (g.nsteps + G - 1) / G, P2Tag0{});
    } else if constexpr (DMAW) {
      constexpr int NGS = KG / G;
      // Counted waits: vmcnt(N) with N = the requests of THIS wave known to be younger than group grp's -- group grp + 1's (issued one
      // iteration earlier) and, for the first two groups, the next tile's patch (NPU unconditional loads issued after the prologue's two
      // groups).  Anything else in flight (older stores, spills) only makes the wait stricter.
      int slot = 0;
#pragma unroll 1
      for (int grp = 0; grp < ngroups; grp++) {
        ys_wait_vm_dyn((grp + 1 < ngroups ? nmine : 0) + ((grp < 2 && more) ? NPU : 0));
        if (grp < 3) TL_STAMP2();
        ys_barrier_lds();                       // group grp is in LDS for every wave; nobody still reads the slot of group grp - 1
        if (grp < 3) TL_STAMP2();
        int s2 = slot + 2; if (s2 >= 3) s2 -= 3;
        if (grp + 2 < ngroups) wdma(grp + 2, s2);
        if (in_bf8) kloop(sW + slot * (BN * 8), grp * KG, NGS, P2Tag1{}); else kloop(sW + slot * (BN * 8), grp * KG, NGS, P2Tag0{});
        if (grp < 3) TL_STAMP2();
        slot = slot == 2 ? 0 : slot + 1;
      }
      ys_barrier_lds();                         // every wave finished reading the patch: it becomes the staging area
    } else {
      constexpr int NGS = KG / G;               // register groups per streamed weight slot
#pragma unroll 1
      for (int grp = 0; grp < ngroups; grp++) {
        wfetch(rwA, grp + 1);                   // unconditional (past the end: zeros); lands during this group's MFMAs
        if (grp < 3) TL_STAMP2();               // (fine timeline: weight fetch issued / K-steps done / weights stored / barrier passed, first three groups)
        if (in_bf8) kloop(sW + (grp & 1) * BN * g.wpitch, grp * KG, NGS, P2Tag1{}); else kloop(sW + (grp & 1) * BN * g.wpitch, grp * KG, NGS, P2Tag0{});
        if (grp < 3) TL_STAMP2();
        wstore(rwA, (grp + 1) & 1);
        if (grp < 3) TL_STAMP2();
        ys_barrier_lds();
        if (grp < 3) TL_STAMP2();
      }
    }
    if (WRES) ys_barrier_lds();               // every wave finished reading the patch: it becomes the staging area
    TL_STAMP();

    // output rows: tile base (scalar) + the lane's table entry -- the 64-bit per-lane form cost ~1-1.5 thousand cycles per tile
    // (s_memtime stamps, round 3); every row index / byte offset of a P2 launch fits 31 bits (conv_p2_plan)
    const int rh = a.out_rh ? a.out_rh : a.Wout, rw = a.out_rh ? a.out_rw : 1;
    const int tbase = b * (int)a.out_bstride + oy0 * rh + ox0 * rw + (int)a.out_r0;
    int orow[MR];
    bool pv[MR];
#pragma unroll
    for (int mf = 0; mf < MR; mf++) {
      pv[mf] = (bool)((int)(pty[mf] < g.TH) & (int)(oy0 + pty[mf] < a.Hout) & (int)(ox0 + ptx[mf] < a.Wout));
      orow[mf] = tbase + prow[mf];
    }
    char* stg = sPb + wave * (16 * MR * (BN + 8) * 2 + 16 * MR * 16);
    if (F8) {                                 // back to real units: 1 / (input scale * weight scale)
      const float dq = a.deq[0];
#pragma unroll
      for (int mf = 0; mf < MR; mf++)
#pragma unroll
        for (int nf = 0; nf < NR; nf++)
#pragma unroll
          for (int r = 0; r < 4; r++) acc[mf][nf][r] *= dq;
    }
#ifdef YS_P2_TIMELINE
    if (!P2_DBG(4)) p2_epilogue<MR, NR, RED, YS_EPI_BATCH_P2>(a, acc, orow, pv, n0, stg, st1, st2, [&]() { TL_STAMP(); });
#else
    if (!P2_DBG(4)) p2_epilogue<MR, NR, RED, YS_EPI_BATCH_P2>(a, acc, orow, pv, n0, stg, st1, st2);
#endif
    TL_STAMP();
    txi = ntx; tyi = nty; b = nb;
  }
  YS_WAIT_VM0();                               // a workgroup without tiles still has its table / weight DMA in flight: it must land before the LDS is released
  if (RED ? a.nred > 0 : a.stats != nullptr) p2_stats_flush<NR, NWV>(a, n0, st1, st2, (float*)sPb, (long)vbx);
  if (F8 && a.amax && blockIdx.y == 0) ys_amax_update(a.amax, amx);
  TL_STAMP();
#ifdef YS_P2_TIMELINE
  if (tl_p) tl_p[0] = (unsigned long long)tl_n;
#endif
}

template <int MR, int NR, int WRES, int NPU, int NT, int F8, int RED = 0>
__global__ void __launch_bounds__(NT, (NT == 512 ? 4 : (NPU <= 6 && MR * NR <= 8 && !F8 ? 3 : 2)))   // TIGHT variants: 3 waves / SIMD
conv_p2_kernel(ConvArgs a, P2Args g, const int* __restrict__ tab) {
  conv_p2_body<MR, NR, WRES, NPU, NT, F8, RED>(a, g, tab, (int)blockIdx.x, (int)gridDim.x);
}

// ---- grouped (multi-problem) launch.  Several INDEPENDENT convolutions that share a kernel variant -- the tower layers of the three
// pyramid levels of Detect / Segment (Head.cs:81-82: the same module applied to x[0], x[1], x[2] with per-level weights) -- run as ONE
// persistent grid: workgroups [end[i-1], end[i]) belong to problem i and see themselves as workgroup vbx of a grid of end[i] - end[i-1].
// The P4 / P5 launches of a YOLOv8n step are 100-400 tiles each, i.e. one latency-bound round of workgroups (12-27 us against a byte
// floor of 1-4 us); inside the P3 level's grid they are just more tiles.  Side streams were measured twice (-5 %: co-running persistent
// grids take each other's workgroup slots); one grid with a static split does not have that problem.  Range starts and sizes are
// multiples of 8 whenever a problem has >= 8 workgroups, so workgroup vbx still runs on XCD vbx % 8 (the tile order relies on it).
struct P2Prob { ConvArgs a; P2Args g; const int* tab; };
struct P2Group { int n; int end[YS_GROUP_MAX]; P2Prob p[YS_GROUP_MAX]; };
template <int MR, int NR, int WRES, int NPU, int NT, int RED>
__global__ void __launch_bounds__(NT, (NT == 512 ? 4 : (NPU <= 6 && MR * NR <= 8 ? 3 : 2)))
conv_p2_group_kernel(P2Group grp) {
  const int bx = (int)blockIdx.x;
  int pi = 0;
#pragma unroll
  for (int k = 0; k + 1 < YS_GROUP_MAX; k++) pi += (int)(k + 1 < grp.n && bx >= grp.end[k]);
  const int start = pi ? grp.end[pi - 1] : 0;
  const P2Prob& pr = grp.p[pi];
  // The problem's arguments are copied into registers once (round 4).  Read in place -- a dynamically indexed slot of the kernel-argument
  // segment -- hipcc re-loads fields where they are used: 81-109 s_load instructions per variant against 36-44 in conv_p2_kernel, many
  // of them inside the K loop, and every one is followed by s_waitcnt lgkmcnt(0), which drains the wave's LDS reads as well (the
  // counter is shared): per-launch records put the grouped 80 -> 80 tower layer at 228 us for 1.31x the pixels of a 113 us single launch.
  const ConvArgs a = pr.a;
  const P2Args g = pr.g;
  const int* const tab = pr.tab;
  conv_p2_body<MR, NR, WRES, NPU, NT, 0, RED>(a, g, tab, bx - start, grp.end[pi] - start);
}

// ------------------------------------------------------------------ host side
struct P2Plan { int ok, mr, nr, wres, npu, nt, gx, gy, per_cu; size_t lds; P2Args g; };
// conv_p2_plan.hip.  force_mr / force_npu / force_nr (0 = free) and want_full = false: grouped launches need every problem on the kernel variant
// of the group's largest problem, and a small member does not have to fill the chip by itself
P2Plan ys_conv_p2_plan(const ConvArgs& a, int force_mr = 0, int force_npu = 0, bool want_full = true, int force_nr = 0);
// tile-independent index tables of a planned launch, cached on the device per layer geometry; null = out of memory
const int* ys_p2_tables(const ConvArgs& a, const P2Plan& p);
// conv_p2.hip: variant dispatch of one planned launch -- its own plain bf16 instances, or those of conv_p2_f8.hip (a.f8, or a.nred > 0)
int ys_conv_p2_dispatch(hipStream_t st, const ConvArgs& a, const P2Plan& p);
int ys_conv_p2_dispatch_f8_red(hipStream_t st, const ConvArgs& a, const P2Plan& p);
