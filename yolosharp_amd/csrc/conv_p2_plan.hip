// conv_p2_plan.hip -- host side of conv_p2_kernel (conv_p2.h): the LDS bank model, the plan (tile, weight residency, LDS layout, grid) and the
// cached index tables.  No kernels: an edit here recompiles in seconds.
#include "conv_p2.h"
#include <map>
#include <mutex>
#include <vector>


// ---- LDS bank model of the K loop's ds_read_b128 fragment reads (MI355X: a wave's b128 read is served in four fixed 16-lane groups
// over 64 four-byte banks, i.e. 16 slots of 16 bytes; lanes of a group that hit the same slot at different addresses serialise).
// Lane (li, q) of a patch fragment reads pixel(li) * ppb + q * 16 (+ a tap / channel offset common to the wave), and each group holds
// eight lanes of quarter q and eight of quarter q + 1.  With an ODD number of slots per pixel (the round-1/2 rule) the eight pixels of
// one quarter and the eight of the next always collide pairwise: every fragment read cost 8 LDS cycles instead of 4 (measured:
// SQ_LDS_BANK_CONFLICT = 44 % of LDS-active cycles).  A pitch of 2 (mod 4) slots puts the pixels of a quarter on even slots and the
// next quarter's on odd ones -> conflict-free for 16 consecutive pixels; a tile row shorter than 16 pixels needs the row pitch
// adjusted as well, which p2_pick_rowpad searches with this model.  Returns the mean LDS cycles per fragment read (4 = conflict-free).
static double p2_read_cycles(int cin, int kh, int kw, int sa, int th, int tw, int mr, int nwv, int ppb, int prb) {
  static const int grp[2][16] = {{0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27}, {4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31}};
  const int ktot = kh * kw * cin;
  const int nsteps = cin >= 16 ? 1 : (ktot + 31) / 32;   // cin >= 16: the quarters of a lane group share a tap, so every K-step adds one constant to all lanes -> same pattern
  long tot = 0, n = 0;
  for (int wave = 0; wave < nwv; wave++)
    for (int mf = 0; mf < mr; mf++) {
      int pb[16];
      for (int li = 0; li < 16; li++) {
        const int px = wave * mr * 16 + mf * 16 + li;
        int ty = px / tw, tx = px - ty * tw;
        if (ty >= th) { ty = 0; tx = 0; }
        pb[li] = ty * sa * prb + tx * sa * ppb;
      }
      for (int st = 0; st < nsteps; st++) {
        int qo[4];
        for (int q = 0; q < 4; q++) {
          int k0 = st * 32 + q * 8; if (k0 >= ktot) k0 = 0;
          const int tap = k0 / cin, ch = k0 - tap * cin;
          const int a = tap / kw, b = tap - a * kw;
          qo[q] = a * prb + b * ppb + ch * 2;
        }
        for (int half = 0; half < 2; half++)
          for (int g = 0; g < 2; g++) {
            int addr[16], mx = 1;
            for (int i = 0; i < 16; i++) { const int l = grp[g][i] + half * 32; addr[i] = pb[l & 15] + qo[l >> 4]; }
            for (int i = 0; i < 16; i++) {
              int c = 1;
              for (int j = 0; j < i; j++) if (addr[j] == addr[i]) { c = 0; break; }       // identical addresses broadcast
              if (!c) continue;
              for (int j = i + 1; j < 16; j++) {
                if (((addr[j] >> 4) & 15) != ((addr[i] >> 4) & 15) || addr[j] == addr[i]) continue;
                bool dup = false;
                for (int k = i + 1; k < j; k++) if (addr[k] == addr[j]) { dup = true; break; }
                if (!dup) c++;
              }
              if (c > mx) mx = c;
            }
            tot += mx;
          }
        n++;
      }
    }
  return n ? (double)tot / (double)n : 4.0;
}
// pixel pitch of the bf16 patch: stride 1 -> smallest slot count >= Cin / 8 that is 2 (mod 4); stride 2 (lanes two pixels apart) -> odd.
// (Round 3 measured the odd rule everywhere as the slower alternative.)
static int p2_pixel_pitch(int cin, int sa) {
  const int cu = cin / 8;
  if (sa != 1) return cin * 2 + ((cu & 1) ? 32 : 16);
  int p = cu;
  while ((p & 3) != 2) p++;
  return p * 16;
}
// row padding (in 16-byte slots, 0..15) of the patch that minimises the modelled read cycles of the chosen tile within `room` bytes
static int p2_pick_rowpad(int cin, int kh, int kw, int sa, int th, int tw, int mr, int nwv, int ppb, int pw, int ph, size_t room) {
  static std::map<std::vector<int>, int> cache;
  static std::mutex mu;
  const std::vector<int> key = {cin, kh, kw, sa, th, tw, mr, nwv, ppb, pw, ph, (int)(room / (16 * (size_t)(ph > 0 ? ph : 1)) > 15 ? 15 : (int)(room / (16 * (size_t)(ph > 0 ? ph : 1))))};
  std::lock_guard<std::mutex> lock(mu);
  auto it = cache.find(key);
  if (it != cache.end()) return it->second;
  double best = p2_read_cycles(cin, kh, kw, sa, th, tw, mr, nwv, ppb, pw * ppb);
  int pad = 0;
  for (int r = 1; r < 16 && best > 4.0 + 1e-9; r++) {
    if ((size_t)ph * r * 16 > room) break;
    const double c = p2_read_cycles(cin, kh, kw, sa, th, tw, mr, nwv, ppb, pw * ppb + r * 16);
    if (c < best - 1e-9) { best = c; pad = r; }
  }
  cache[key] = pad;
  return pad;
}

// fp8 variants whose 32-byte fragments fit the 256-register budget without spilling (hipcc -Rpass-analysis=kernel-resource-usage)
static bool p2_f8_tile_ok(int mr, int nr, int wres, int npu) {
  if (wres) return npu == 6 ? !(mr == 4 && nr == 4) : (mr * nr <= 8 && !(mr == 2 && nr == 5));
  return npu == 6 ? (mr * nr <= 6 || (mr == 4 && nr == 2)) && !(mr == 1 && nr == 5) : (mr * nr <= 4 && mr + nr <= 5);
}
// plan sweep (tools/dev/r06/p2_sweep.py through ys_debug_p2_force): a register-tile height, a tile width and an output-channel split imposed on every plan of the
// process; 0 = the cost model's own choice.  Triage library only (-DYS_TRIAGE, `build.py triage`): unsynchronised process-global state; the product sees constants.
#ifdef YS_TRIAGE
static int g_p2_force_mr = 0, g_p2_force_tw = 0, g_p2_force_nr = 0;
extern "C" __attribute__((visibility("default"))) int ys_debug_p2_force(int mr, int tw, int nr) { g_p2_force_mr = mr; g_p2_force_tw = tw; g_p2_force_nr = nr; return 0; }
#else
constexpr int g_p2_force_mr = 0, g_p2_force_tw = 0, g_p2_force_nr = 0;
#endif
P2Plan ys_conv_p2_plan(const ConvArgs& a, int force_mr, int force_npu, bool want_full, int force_nr) {
  P2Plan p{};
  if (g_p2_force_mr && !force_mr) force_mr = g_p2_force_mr;
  if (g_p2_force_nr && !force_nr) force_nr = g_p2_force_nr;
  // 3x3 forward / stride-1 dgrad, 1x1 forward / dgrad, and the 1x1 .. 2x2 phase convolutions of a stride-2 dgrad (strided
  // output-row map)
  const bool k3 = a.KH == 3 && a.KW == 3 && a.out_rh == 0;
  const bool phase = a.KH >= 1 && a.KH <= 2 && a.KW >= 1 && a.KW <= 2 && a.SA == 1 && a.out_rh != 0 && a.PAD == 0;
  // 1x1 layers use the same kernel (patch = tile, no halo): measured 4 % faster per step than the direct-fragment kernel
  const bool k1 = a.KH == 1 && a.KW == 1 && a.PAD == 0 && a.SA == 1 && a.out_rh == 0;
  if (!((k3 || phase || k1) && a.DIVM == 0 && (a.SA == 1 || a.SA == 2) && a.pad_w_delta == 0)) return p;
  if (a.Cin % 8) return p;
  long xbytes_l;
  {
    const long pix = (long)(a.B - 1) * a.in_bstride + (long)a.Hin * a.Win;
    xbytes_l = (pix * a.in_ldc - a.in_coff) * 2L;
    if (xbytes_l <= 0 || xbytes_l >= (1L << 31)) return p;     // 32-bit descriptor offsets (larger views: the round-1 kernels)
    if ((long)a.B * a.out_bstride * a.out_ldc * 2L >= (1L << 31)) return p;                      // the epilogue's store offsets
  }
  const bool f8 = a.f8 != 0;
  // fp8 pays where the K loop dominates (LDS / MFMA bound layers); the HBM-bound small-channel layers gain nothing from it and pay
  // the on-the-fly quantisation (measured: 32-channel layers 1.6x slower in fp8) -> they keep the bf16 kernel
  const int f8_min_cin = (int)YS_OPT_INT("F8_MIN_CIN", 128);
  if (f8 && (a.Cin % 32 || a.Cin < f8_min_cin || !a.w8 || !a.qscale || !a.deq)) return p;
  const int ups = f8 ? 8 : 4;                        // 16-byte LDS units per weight row and K-step
  const int nfr = (a.Cout + 15) / 16;
  int nr = nfr <= 4 ? nfr : (nfr % 5 == 0 ? 5 : 4);
  const int cu = a.Cin / 8;
  P2Args g{};
  g.xbytes = (unsigned)xbytes_l;
  g.ppb = f8 ? a.Cin + (((a.Cin / 16) & 1) ? 32 : 16) : p2_pixel_pitch(a.Cin, a.SA);   // bf16: bank-model rule (p2_pixel_pitch); fp8: odd number of 16-byte slots per pixel
  const int taps = a.KH * a.KW;
  g.nsteps = f8 ? (taps * a.Cin + 127) / 128 : (taps * a.Cin + 31) / 32;
  // resident up to 40 KB (measured: 20 KB 14.52, 40 KB 14.48, 80 KB 14.96 ms/step -- larger resident sets cost the second
  // workgroup per CU)
  // rows padded to 4 K-steps; fp8: 52 KB (the streamed fp8 variants are limited to small register tiles; YOLOv8x 1280 step 165.3 -> 161.7 ms)
  const size_t wresmax = f8 ? 52 * 1024 : 44 * 1024;
  // Streamed weights cost one L2 round trip per K-group on the critical path of every tile.  When half the output channels
  // would make the weight set resident, split the channels over two workgroup columns instead (the patch is then read
  // twice, from L2).
  const double tileconst = 3000.0;
  const int nsteps4 = (g.nsteps + 3) & ~3;           // resident weight rows are zero-padded to whole register groups (<= 4 K-steps)
  // weight rows: 16 consecutive rows per fragment read, same lane-group structure as the patch -> a pitch of 2 (mod 4) slots is
  // conflict-free (the odd pitch was 2-way); fp8 rows (two reads per fragment, quarters two slots apart) keep the odd pitch
  auto wp = [&](int units) { if (f8) return units | 1; int p = units; while ((p & 3) != 2) p++; return p; };
  g.nsp = nsteps4 + 12;                              // + slack: the pipelined loop reads table entries up to two groups ahead
  if ((size_t)nr * 16 * wp(nsteps4 * ups) * 16 > wresmax && nr % 2 == 0 &&   // (measured 13.00 -> 12.86 ms/step)
      (size_t)(nr / 2) * 16 * wp(nsteps4 * ups) * 16 <= wresmax && nfr % (nr / 2) == 0)
    nr /= 2;
  if (f8 && (size_t)nr * 16 * wp(nsteps4 * ups) * 16 > wresmax && nr > 2) nr = 2;   // streamed fp8 weights: small register tiles only
  if (force_nr && force_nr <= nr && nfr % force_nr == 0) nr = force_nr;   // grouped launch: the output-channel split of the group's first member (never wider than this problem's own choice)
  const int bn = nr * 16;
  const size_t wres_bytes = (size_t)bn * wp(nsteps4 * ups) * 16;
  const int wres = wres_bytes <= wresmax ? 1 : 0;
  g.kg = wres ? g.nsteps : P2_KG;     // conv_p2_kernel::KG
  if (!wres && g.kg > g.nsteps) g.kg = g.nsteps;
  g.wpitch = wres ? wp(nsteps4 * ups) : wp(g.kg * ups);
  const bool dmaw = !wres && !f8;   // conv_p2_body::DMAW (every streamed bf16 variant has 256 threads): three ring slots of bn 128-byte rows
  const size_t wbytes = wres ? (wres_bytes + 1023) / 1024 * 1024 : (dmaw ? (size_t)3 * bn * 128 : (size_t)2 * bn * g.wpitch * 16);   // resident set: whole 1 KB LDS-DMA requests
  const size_t tab = ((size_t)g.nsp * 16 + 15) / 16 * 16;
  const int gy = ys_cdiv(a.Cout, bn);
  // 3x3 layers with >= 256 input channels do not fit a useful whole-Cin patch (<= 64-pixel tiles, the full weight set streamed
  // per tile): the chunked round-1 kernel handles them better (YOLOv11m-seg step 65.9 -> 63.4 ms)
  const int maxcin3 = 255;
  if (k3 && a.SA == 1 && a.Cin > (f8 ? 640 : maxcin3)) return p;   // an fp8 patch pixel is half the bytes
  for (size_t budget = (wres && wres_bytes > 52 * 1024 ? 152 : 76) * 1024; budget <= 152 * 1024 && !p.ok; budget *= 2) {   // two workgroups per CU; one if nothing else fits
  // tile = (4 waves x 16*mr pixels, th x tw): minimise the bytes a layer moves through the CU (patch incl. halo, streamed
  // weights, output) plus a per-tile constant; among shapes that give the chip >= 512 workgroups when the layer is large
  // enough.  (512-thread workgroups -- 8 waves x 2 fragments, same LDS footprint -- were measured 13 % slower: the 128-register
  // budget of 4 waves/SIMD spills for >= 48 output channels.)
  double best = 1e30; bool best_full = false;
  {
    const int nt = 256, nwv = nt / 64;
    const size_t stat = (size_t)nwv * bn * 2 * 4;
    const int npu_max = P2_NPU;
    for (int mr = (nr <= 4 ? 4 : 2); mr >= 1; mr >>= 1) {
      if (force_mr && mr != force_mr) continue;
      const int npx = 16 * nwv * mr;
      const size_t stage = (size_t)nwv * (16 * mr * (bn + 8) * 2 + 16 * mr * 16);
      for (int tw = 1; tw <= npx && tw <= a.Wout; tw++) {
        if (g_p2_force_tw && tw != g_p2_force_tw) continue;
        int th = npx / tw; if (th > a.Hout) th = a.Hout;
        const int ph = (th - 1) * a.SA + a.KH, pw = (tw - 1) * a.SA + a.KW;
        size_t pbytes = (size_t)ph * pw * g.ppb; if (pbytes < stage) pbytes = stage;
        if (pbytes < (size_t)17 * nt * 4) pbytes = (size_t)17 * nt * 4;   // statistics scratch of p2_stats_flush ([16][NT] lane sums + [P][2 BN] partials)
        const size_t lds = tab + wbytes + pbytes + stat;
        if (f8 && !p2_f8_tile_ok(mr, nr, wres, ph * pw * cu <= 6 * 256 ? 6 : 12)) continue;
        if (lds > budget || ph * pw * cu > npu_max * nt || (size_t)ph * pw * g.ppb > (size_t)8192 * (f8 ? 8 : 16)) continue;   // 13-bit LDS slot field
        if (force_npu == 6 && ph * pw * cu > 6 * nt) continue;
        const int tx = ys_cdiv(a.Wout, tw), ty = ys_cdiv(a.Hout, th);
        const long ntiles = (long)tx * ty * a.B;
        const double per_tile = (double)ph * pw * a.Cin + (wres ? 0.0 : 0.5 * bn * (double)taps * a.Cin) + 1.0 * npx * (a.Cin + bn) + tileconst;
        // Round 6 (plan sweep on the MI355X, tools/dev/r06/p2_sweep.py): the byte model above prefers the largest tile, but a plan of the three-workgroups-per-CU class
        // (6-unit patch, register tile of <= 8 MFMAs, <= 50 KB of LDS: conv_p2_kernel's TIGHT variants) beats a cheaper-looking two-per-CU plan by more than the
        // bytes say -- 1x1 64 -> 64 at M = 409600: 4 x 4 tiles 37.0 us, 1 x 4 tiles 28.2 us; 3x3 s2 16 -> 32 at M = 1.6 M: 68.0 -> 59.0 us.  The class gets a discount.
        const bool cls3 = !f8 && nt == 256 && mr * nr <= 8 && ph * pw * cu <= 6 * nt && lds <= (size_t)50 * 1024;
        const double cost = (double)tx * ty * per_tile * (cls3 ? 0.75 : 1.0);   // (0.85 / 0.75 / 0.65 / 0.55 measured alike end to end: conv_p2 time 2.16 -> 2.11 ms per config-2 step, config 3 1.44 -> 1.40, config 4 3.27 -> 3.16)
        const bool full = !want_full || ntiles * gy >= 512;   // (a small member of a grouped launch does not have to fill the chip by itself: cheapest tiles)
        if ((full && !best_full) || (full == best_full && cost < best)) {
          best = cost; best_full = full;
          P2Args cur = g;
          cur.TH = th; cur.TW = tw; cur.tiles_x = tx; cur.tiles_y = ty; cur.PH = ph; cur.PW = pw; cur.ntiles = (int)ntiles;
          cur.off_w = (int)tab; cur.off_p = (int)(tab + wbytes); cur.off_stat = (int)(lds - stat);
          p.ok = 1; p.mr = mr; p.nr = nr; p.wres = wres; p.g = cur; p.lds = lds; p.gy = gy; p.nt = nt;
          p.npu = ph * pw * cu <= 6 * 256 ? 6 : 12;
          if (force_npu) p.npu = force_npu;
        }
      }
    }
  }
  }
  if (!p.ok) return p;
  if ((long)p.g.ntiles > 2L * ys_cdiv(a.M, 64)) { p.ok = 0; return p; }   // stats workspace bound (plan.hip allocate: stat_max)
  // three workgroups per CU (TIGHT register variants) when three footprints fit the 160 KB
  const size_t lds3 = (size_t)50 * 1024;
  p.g.prb = p.g.PW * p.g.ppb;
  if (!f8) {
    // row padding of the patch (bank model, p2_pick_rowpad) inside the occupancy class the tile search settled on
    const int nwv = p.nt / 64;
    const size_t stat = (size_t)nwv * bn * 2 * 4, stage = (size_t)nwv * (16 * p.mr * (bn + 8) * 2 + 16 * p.mr * 16);
    size_t floor_b = stage > (size_t)17 * p.nt * 4 ? stage : (size_t)17 * p.nt * 4;
    const size_t pb0 = (size_t)p.g.PH * p.g.prb;
    const size_t cap = (p.lds <= lds3 && p.npu == 6 && p.mr * p.nr <= 8) ? lds3 : (p.lds <= 76 * 1024 ? 76 * 1024 : 152 * 1024);
    const size_t base = p.lds - (pb0 > floor_b ? pb0 : floor_b);           // tables + weights + statistics
    size_t room = cap > base + pb0 ? cap - base - pb0 : 0;
    if (pb0 + room > (size_t)8192 * 16) room = (size_t)8192 * 16 > pb0 ? (size_t)8192 * 16 - pb0 : 0;   // 13-bit LDS slot field
    const int pad = p2_pick_rowpad(a.Cin, a.KH, a.KW, a.SA, p.g.TH, p.g.TW, p.mr, nwv, p.g.ppb, p.g.PW, p.g.PH, room);
    p.g.prb += pad * 16;
    const size_t pb1 = (size_t)p.g.PH * p.g.prb;
    p.lds = base + (pb1 > floor_b ? pb1 : floor_b);
    p.g.off_stat = (int)(p.lds - stat);
  }
  // three per CU needs the TIGHT register variant too (conv_p2_kernel's launch bounds: NPU <= 6, MR * NR <= 8, bf16 -- 168 registers): the
  // 4 x 3, 2 x 5 and 4 x 4 tiles compile to 189-236 registers, i.e. two waves per SIMD, and a 768-workgroup grid of theirs left 256
  // workgroups waiting for a slot (round 4: the same pathology as the grouped launches' rounding)
  const bool tight_regs = p.npu == 6 && p.mr * p.nr <= 8 && !f8;
  const int per_cu = (p.lds <= lds3 && tight_regs) ? 3 : (p.lds <= 76 * 1024 ? 2 : 1);
  p.per_cu = per_cu;
  // (measured, round 4: a 168-register variant that LDS limits to two workgroups per CU anyway is NOT better off on the 12-unit variant of the
  // same tile with 2-4 K-steps per LDS wait: config 2 patch-kernel time 2.58 -> 2.65 ms, config 5 6.8 -> 6.9 -- the K loop of these tiles is
  // bound by LDS read bandwidth / issue, not by the exposed wait)
  long gx = ((long)ys_cu_count() * per_cu) / p.gy;            // persistent grid: the next tile's patch is prefetched
  if (gx > p.g.ntiles) gx = p.g.ntiles;
  if (gx < 1) gx = 1;
  p.gx = (int)gx;
  return p;
}

// Tile-independent index tables of a P2 launch (see conv_p2_kernel), built on the host once per layer geometry and cached
// on the device for the life of the process (a few KB per distinct layer shape).
const int* ys_p2_tables(const ConvArgs& a, const P2Plan& p) {
  static std::map<std::vector<int>, int*> cache;
  static std::mutex cache_mu;                   // distinct ys_ctx may launch from different threads
  std::lock_guard<std::mutex> lock(cache_mu);
  int dev = 0;
  hipGetDevice(&dev);
  const P2Args& g = p.g;
  const bool f8 = a.f8 != 0;
  const int rh = a.out_rh ? a.out_rh : a.Wout, rw = a.out_rh ? a.out_rw : 1;
  std::vector<int> key = {dev, a.Cin, a.KH, a.KW, a.SA, a.Win, a.in_ldc, g.TH, g.TW, g.PH, g.PW, g.ppb, g.prb, g.nsteps, g.nsp, p.mr, p.npu, p.nt, (int)f8, rh, rw};
  auto it = cache.find(key);
  if (it != cache.end()) return it->second;
  const int NT = p.nt;
  const int cu = a.Cin / 8, Ktot = a.KH * a.KW * a.Cin, npatch = g.PH * g.PW * cu;
  std::vector<int> h((size_t)g.nsp * 4 + (size_t)p.mr * 4 * NT + (size_t)p.npu * 2 * NT, 0);
  for (int qq = 0; qq < 4; qq++)            // q-major: [quarter][K-step]; steps past the last real one keep offset 0 (their weights are zero)
    for (int st = 0; st < g.nsteps; st++) {
      const int kp = f8 ? 32 : 8;             // channels per (K-step, quarter) piece
      const int k0 = st * 4 * kp + qq * kp;
      if (k0 < Ktot) {
        const int tap = k0 / a.Cin, ch = k0 - tap * a.Cin;
        const int kh = tap / a.KW, kw = tap - kh * a.KW;
        h[(size_t)qq * g.nsp + st] = kh * g.prb + kw * g.ppb + ch * (f8 ? 1 : 2);
      }
    }
  int* tpx = h.data() + g.nsp * 4;
  for (int tid = 0; tid < NT; tid++) {
    const int wave = tid >> 6, li = tid & 15;
    for (int mf = 0; mf < p.mr; mf++) {
      const int px = wave * (p.mr * 16) + mf * 16 + li;
      int ty = px / g.TW, tx = px - ty * g.TW;
      if (ty >= g.TH) { ty = g.TH; tx = 0; }    // idle lane of a ragged tile: marked by ty == TH, reads pixel (0,0)
      tpx[(mf * 4 + 0) * NT + tid] = ty < g.TH ? (ty * a.SA) * g.prb + (tx * a.SA) * g.ppb : 0;
      tpx[(mf * 4 + 1) * NT + tid] = ty;
      tpx[(mf * 4 + 2) * NT + tid] = tx;
      tpx[(mf * 4 + 3) * NT + tid] = ty < g.TH ? ty * rh + tx * rw : 0;
    }
  }
  int* tpd = tpx + p.mr * 4 * NT;
  for (int tid = 0; tid < NT; tid++)
    for (int k = 0; k < p.npu; k++) {
      const int idx = tid + NT * k;
      unsigned d = 0xffffffffu; int go = 0;
      if (idx < npatch) {
        const int pix = idx / cu, u = idx - pix * cu;
        const int r = pix / g.PW, cc = pix - r * g.PW;
        d = ((unsigned)r << 23) | ((unsigned)cc << 13) | (f8 ? (unsigned)((r * g.prb + cc * g.ppb + u * 8) >> 3) : (unsigned)((r * g.prb + cc * g.ppb + u * 16) >> 4));
        go = (r * a.Win + cc) * a.in_ldc + u * 8;
      }
      tpd[(2 * k + 0) * NT + tid] = (int)d;
      tpd[(2 * k + 1) * NT + tid] = go;
    }
  int* dptr = nullptr;
  if (hipMalloc(&dptr, h.size() * sizeof(int)) != hipSuccess) return nullptr;
  if (hipMemcpy(dptr, h.data(), h.size() * sizeof(int), hipMemcpyHostToDevice) != hipSuccess) { hipFree(dptr); return nullptr; }
  cache[key] = dptr;
  return dptr;
}

// Development aid (tools/dev/p2_plans.py, triage library only): the P2 plan of a forward convolution geometry as text -- no device needed.
#ifdef YS_TRIAGE
extern "C" __attribute__((visibility("default"))) int ys_debug_p2_plan(int B, int Hin, int Win, int Cin, int Cout, int k, int s, int in_ldc, char* buf, int cap) {
  ConvArgs a{};
  a.B = B; a.Hin = Hin; a.Win = Win; a.Cin = Cin; a.Cout = Cout; a.KH = a.KW = k; a.SA = s; a.PAD = k / 2;
  a.Hout = (Hin + 2 * (k / 2) - k) / s + 1; a.Wout = (Win + 2 * (k / 2) - k) / s + 1;
  a.in_ldc = in_ldc; a.in_bstride = (long)Hin * Win; a.out_ldc = Cout; a.out_bstride = (long)a.Hout * a.Wout; a.M = B * a.Hout * a.Wout;
  if (ys_conv_gemm_rows(a)) { snprintf(buf, cap, "gemm"); return 2; }
  const P2Plan p = ys_conv_p2_plan(a);
  if (!p.ok) { snprintf(buf, cap, "none"); return 0; }
  const double cyc = p2_read_cycles(a.Cin, a.KH, a.KW, a.SA, p.g.TH, p.g.TW, p.mr, p.nt / 64, p.g.ppb, p.g.prb);
  snprintf(buf, cap, "mr%d nr%d wres%d npu%d tile%dx%d grid%dx%d lds%zu ppb%d prb%d(pad%d) wpitch%d readcyc%.2f", p.mr, p.nr, p.wres, p.npu, p.g.TH, p.g.TW,
           p.gx, p.gy, p.lds, p.g.ppb, p.g.prb, (p.g.prb - p.g.PW * p.g.ppb) / 16, p.g.wpitch, cyc);
  return 1;
}
#endif
