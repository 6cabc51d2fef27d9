// conv_p2_launch.h -- launcher of conv_p2_kernel (conv_p2.h) and the pieces of its register-tile dispatch.  The 168 single-launch kernels compiled for
// 101 s as one unit, so two units instantiate them: conv_p2.hip the plain bf16 variant <F8 = 0, RED = 0>, conv_p2_f8.hip the fp8 variant <1, 0> and
// the bf16 variant with the fused BN-backward reduction <0, 1>.  (The fp8 kernels stay beside a bf16 variant on purpose: compiled in a unit of
// their own, hipcc schedules a dozen scalar instructions of their prologue in another order.)
#pragma once
#include "conv_p2.h"
#include "conv_tl.h"
#include <atomic>
#include <cstdlib>

template <int MR, int NR, int WRES, int NPU, int NT, int F8, int RED = 0>
static int conv_p2_launch_t(hipStream_t st, ConvArgs a, const P2Plan& p) {
#ifdef YS_P2_ABLATE
  a.dbg = (int)YS_OPT_INT("DBG", 0);   // ablation switches (triage build only: build.py p2ablate)
#endif
  a.red_koff = (int)offsetof(ConvArgs, red);       // ConvArgs is the kernel's first argument (conv_epi.h ys_red_table)
  static std::atomic<unsigned> attr_done{0};      // per device: the attribute belongs to the device's code object
  int dev_id = 0;
  (void)hipGetDevice(&dev_id);
  if (!(attr_done.load(std::memory_order_relaxed) & (1u << (dev_id & 31)))) {
    hipFuncSetAttribute((const void*)conv_p2_kernel<MR, NR, WRES, NPU, NT, F8, RED>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    attr_done.fetch_or(1u << (dev_id & 31), std::memory_order_relaxed);
  }
  char lab[192] = "";
  if (ys_kprof_enabled()) snprintf(lab, sizeof(lab), F8 ? "p2f8 k%d s%d div1 cin%d cout%d M%d acc%d nt%d mr%d nr%d wres%d npu%d tile%dx%d grid%dx%d lds%d" : "p2 k%d s%d div1 cin%d cout%d M%d acc%d nt%d mr%d nr%d wres%d npu%d tile%dx%d grid%dx%d lds%d", a.KH * 10 + a.KW, a.SA, a.Cin, a.Cout, a.M, a.accumulate, NT, MR, NR, WRES, NPU, p.g.TH, p.g.TW, p.gx, p.gy, (int)p.lds);
  YsKprofScope prof(st, "conv_igemm", lab);
  const int* tab = ys_p2_tables(a, p);
  if (!tab) { ys_set_error("conv p2: cannot allocate the index tables"); return YS_ERR_OOM; }
#ifdef YS_P2_TIMELINE
  const char* tl_path = ys_tl_begin(st, a);
#endif
  YS_LAUNCH_LDS((conv_p2_kernel<MR, NR, WRES, NPU, NT, F8, RED>), dim3(p.gx, p.gy), NT, p.lds, st, a, p.g, tab);
#ifdef YS_P2_TIMELINE
  ys_tl_dump(st, tl_path, a, p.gx, "# k%d%d s%d cin%d cout%d M%d mr%d nr%d wres%d npu%d tile%dx%d grid%dx%d lds%d ntiles%d nsteps%d", a.KH, a.KW, a.SA, a.Cin, a.Cout, a.M, MR, NR, WRES, NPU, p.g.TH, p.g.TW, p.gx, p.gy, (int)p.lds, p.g.ntiles, p.g.nsteps);
#endif
  return YS_OK;
}

// the launch of register tile M_ x N_ in variant <F_, R_>: resident or streamed weights, 6 or 12 patch units per thread
#define P2F(M_, N_, F_, R_) { \
    if (p.wres) return p.npu == 6 ? conv_p2_launch_t<M_, N_, 1, 6, 256, F_, R_>(st, a, p) : conv_p2_launch_t<M_, N_, 1, 12, 256, F_, R_>(st, a, p); \
    return p.npu == 6 ? conv_p2_launch_t<M_, N_, 0, 6, 256, F_, R_>(st, a, p) : conv_p2_launch_t<M_, N_, 0, 12, 256, F_, R_>(st, a, p); }
// every register tile through the unit's P2(M_, N_)
#ifdef YS_P2_ONE          // compile-time triage: a single register tile (seconds instead of minutes per resource-usage experiment)
#ifndef YS_P2_ONE_M
#define YS_P2_ONE_M 1
#define YS_P2_ONE_N 5
#endif
#define P2_TILES P2(YS_P2_ONE_M, YS_P2_ONE_N)
#else
#define P2_TILES P2(1, 1) P2(2, 1) P2(4, 1) P2(1, 2) P2(2, 2) P2(4, 2) P2(1, 3) P2(2, 3) P2(4, 3) P2(1, 4) P2(2, 4) P2(4, 4) P2(1, 5) P2(2, 5)
#endif
