// conv_p2_group.hip -- conv_p2_group_kernel (conv_p2.h): several independent P2 convolutions of one kernel variant as one persistent grid
#include "conv_p2.h"
#include <atomic>
#include <cstdlib>

// ---- grouped launch of n <= YS_GROUP_MAX independent P2 convolutions on one kernel variant (conv_p2_group_kernel).  Returns YS_OK
// and the statistics rows (= workgroups) each problem got in rows[], or YS_ERR_UNSUPPORTED when the problems cannot share a variant
// (the caller then launches them one by one).  row_cap[i] > 0 bounds problem i's workgroups (partial-row regions sized elsewhere).
template <int MR, int NR, int WRES, int NPU, int NT, int RED>
static int conv_p2_group_launch_t(hipStream_t st, const ConvArgs* a, const P2Plan* p, int n, const int* gxs, size_t lds) {
#ifdef YS_P2_ABLATE
  const int dbg = (int)YS_OPT_INT("DBG", 0);
#else
  const int dbg = 0;
#endif
  static std::atomic<unsigned> attr_done{0};
  int dev_id = 0;
  (void)hipGetDevice(&dev_id);
  if (!(attr_done.load(std::memory_order_relaxed) & (1u << (dev_id & 31)))) {
    hipFuncSetAttribute((const void*)conv_p2_group_kernel<MR, NR, WRES, NPU, NT, RED>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    attr_done.fetch_or(1u << (dev_id & 31), std::memory_order_relaxed);
  }
  P2Group grp{};
  grp.n = n;
  int total = 0;
  char lab[320] = "";
  for (int i = 0; i < n; i++) {
    P2Prob& pr = grp.p[i];
    pr.a = a[i]; pr.a.dbg = dbg; pr.g = p[i].g;
    pr.a.red_koff = (int)(offsetof(P2Group, p) + (size_t)i * sizeof(P2Prob) + offsetof(P2Prob, a) + offsetof(ConvArgs, red));
    pr.tab = ys_p2_tables(a[i], p[i]);
    if (!pr.tab) { ys_set_error("conv p2: cannot allocate the index tables"); return YS_ERR_OOM; }
    total += gxs[i];
    grp.end[i] = total;
  }
  for (int i = n; i < YS_GROUP_MAX; i++) grp.end[i] = total;
  if (ys_kprof_enabled()) {
    int o = snprintf(lab, sizeof(lab), "p2grp%d k%d s%d div1 cin%d cout%d M", n, a[0].KH * 10 + a[0].KW, a[0].SA, a[0].Cin, a[0].Cout);
    long Msum = 0;
    for (int i = 0; i < n; i++) Msum += a[i].M;
    o += snprintf(lab + o, sizeof(lab) - o, "%ld acc%d nt%d mr%d nr%d wres%d npu%d tile%dx%d grid%dx%d lds%d", Msum, a[0].accumulate, NT, MR, NR, WRES, NPU, p[0].g.TH, p[0].g.TW, total, p[0].gy, (int)lds);
    for (int i = 0; i < n && o < (int)sizeof(lab) - 24; i++) o += snprintf(lab + o, sizeof(lab) - o, " [%dx%d t%d g%d]", p[i].g.TH, p[i].g.TW, p[i].g.ntiles, gxs[i]);
  }
  YsKprofScope prof(st, "conv_igemm", lab);
  YS_LAUNCH_LDS((conv_p2_group_kernel<MR, NR, WRES, NPU, NT, RED>), dim3(total, p[0].gy), NT, lds, st, grp);
  return YS_OK;
}

// variant dispatch of a grouped launch (n >= 1 problems already planned on ONE variant; gxs = workgroups per problem)
static int conv_p2_group_dispatch(hipStream_t st, const ConvArgs* a, const P2Plan* p, int n, const int* gxs, size_t lds) {
  const bool red = a[0].nred > 0;
#define P2GF(M_, N_, R_) { \
    if (p[0].wres) return p[0].npu == 6 ? conv_p2_group_launch_t<M_, N_, 1, 6, 256, R_>(st, a, p, n, gxs, lds) : conv_p2_group_launch_t<M_, N_, 1, 12, 256, R_>(st, a, p, n, gxs, lds); \
    return p[0].npu == 6 ? conv_p2_group_launch_t<M_, N_, 0, 6, 256, R_>(st, a, p, n, gxs, lds) : conv_p2_group_launch_t<M_, N_, 0, 12, 256, R_>(st, a, p, n, gxs, lds); }
#define P2G(M_, N_) if (p[0].mr == M_ && p[0].nr == N_) { if (red) P2GF(M_, N_, 1) else P2GF(M_, N_, 0) }
#ifdef YS_P2_ONE
  P2G(YS_P2_ONE_M, YS_P2_ONE_N)
#else
  P2G(1, 1) P2G(2, 1) P2G(4, 1) P2G(1, 2) P2G(2, 2) P2G(4, 2) P2G(1, 3) P2G(2, 3) P2G(4, 3) P2G(1, 4) P2G(2, 4) P2G(4, 4) P2G(1, 5) P2G(2, 5)
#endif
#undef P2G
#undef P2GF
  ys_set_error("conv p2 group: no kernel for MR=%d NR=%d", p[0].mr, p[0].nr);
  return YS_ERR_UNSUPPORTED;
}

int ys_conv_p2_group_launch(hipStream_t st, const ConvArgs* a, int n, const int* row_cap, int* rows, bool plan_only) {
  const bool off = YS_OPT_INT("GROUP", 1) == 0;
  if (off || n < 2 || n > YS_GROUP_MAX) return YS_ERR_UNSUPPORTED;
  P2Plan p[YS_GROUP_MAX];
  int big = 0;
  for (int i = 0; i < n; i++) {
    const ConvArgs& x = a[i];
    // (measured, round 4: the stride-2 dgrad phases of the 128- and 256-channel layers, which the blocked-GEMM kernel takes one by one, run as one
    // patch-kernel grid within noise of the four GEMM launches: 9.01-9.02 -> 8.92-9.00 ms/step; they stay on the GEMM kernel)
    if (x.f8 || ys_conv_gemm_rows(x)) return YS_ERR_UNSUPPORTED;
    if (ys_conv_dgrad_uses_phases(YS_BF16, x.KH, x.DIVM + 1) && x.KW == x.KH) return YS_ERR_UNSUPPORTED;
    if (x.Cin != a[0].Cin || x.Cout != a[0].Cout || x.SA != a[0].SA || x.PAD != a[0].PAD ||   // (kernel sizes may differ: the four phases of a stride-2 dgrad)
        (x.nred > 0) != (a[0].nred > 0) || (x.accumulate != 0) != (a[0].accumulate != 0) || (x.stats != nullptr) != (a[0].stats != nullptr)) return YS_ERR_UNSUPPORTED;
    if (x.M > a[big].M) big = i;
  }
  p[big] = ys_conv_p2_plan(a[big]);
  if (!p[big].ok) return YS_ERR_UNSUPPORTED;
  for (int i = 0; i < n; i++) {
    if (i == big) continue;
    p[i] = ys_conv_p2_plan(a[i], p[big].mr, p[big].npu, false, p[big].nr);
    if (!p[i].ok || p[i].nr != p[big].nr || p[i].wres != p[big].wres || p[i].nt != p[big].nt || p[i].gy != p[big].gy) return YS_ERR_UNSUPPORTED;
  }
  // one persistent grid: the slots of the largest LDS footprint's occupancy class, split in proportion to the tile counts
  size_t lds = 0; int per_cu = 3;
  long tiles = 0;
  for (int i = 0; i < n; i++) { lds = lds > p[i].lds ? lds : p[i].lds; per_cu = per_cu < p[i].per_cu ? per_cu : p[i].per_cu; tiles += p[i].g.ntiles; }
  const long slots = ((long)ys_cu_count() * per_cu) / p[0].gy > 0 ? ((long)ys_cu_count() * per_cu) / p[0].gy : 1;
  int gxs[YS_GROUP_MAX];
  long used = 0;
  for (int i = 0; i < n; i++) {
    long gx = (slots * p[i].g.ntiles + tiles / 2) / tiles;
    if (gx >= 8) gx = (gx + 4) / 8 * 8;          // multiples of 8: workgroup vbx keeps running on XCD vbx % 8
    if (gx < 1) gx = 1;
    if (gx > p[i].g.ntiles) gx = p[i].g.ntiles;
    if (row_cap && row_cap[i] > 0 && gx > row_cap[i]) gx = row_cap[i];
    gxs[i] = (int)gx; used += gx;
  }
  // The grid must FIT: rounding every range up to a multiple of 8 made it 520-528 workgroups for 512 slots (776 for 768) on the Detect
  // towers -- the last 8 wait for a slot, start when the first workgroups leave and then walk their whole tile share alone (round 4,
  // per-launch records: the grouped 80 -> 80 layer 215 us against 174 us for its three levels launched one by one).  Take the excess
  // from the largest ranges, 8 at a time (1 at a time below 16).
  while (used > slots) {
    int big = 0;
    for (int i = 1; i < n; i++) if (gxs[i] > gxs[big]) big = i;
    const int dec = gxs[big] >= 16 ? 8 : 1;
    if (gxs[big] - dec < 1) break;
    gxs[big] -= dec; used -= dec;
  }
  // a range that is not a multiple of 8 shifts the XCD phase of the ranges behind it: order the problems so that only the last may be ragged
  // (ranges of >= 8 workgroups are multiples of 8 unless a cap cut them; a shifted phase only costs L2 locality, never correctness)
  for (int i = 0; i < n; i++) if (rows) rows[i] = gxs[i];
  if (plan_only) return YS_OK;
  return conv_p2_group_dispatch(st, a, p, n, gxs, lds);
}
