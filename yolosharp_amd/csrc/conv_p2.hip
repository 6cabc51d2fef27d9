// conv_p2.hip -- conv_p2_kernel (conv_p2.h): the plain bf16 instances, and the variant dispatch of a single launch
#include "conv_p2_launch.h"

// (Single launches through conv_p2_group_kernel with one problem -- arguments read from the kernel-argument segment instead of held in scalar registers --
// were built and measured in round 4 as no faster; the switch is gone.)
int ys_conv_p2_dispatch(hipStream_t st, const ConvArgs& a, const P2Plan& p) {
  if (a.f8 && a.nred > 0) { ys_set_error("conv p2: the fused BN-backward reduction has no fp8 variant"); return YS_ERR_UNSUPPORTED; }
  if (a.f8 || a.nred > 0) return ys_conv_p2_dispatch_f8_red(st, a, p);
#define P2(M_, N_) if (p.mr == M_ && p.nr == N_) P2F(M_, N_, 0, 0)
  P2_TILES
#undef P2
  ys_set_error("conv p2: no kernel for NT=%d MR=%d NR=%d", p.nt, p.mr, p.nr);
  return YS_ERR_UNSUPPORTED;
}
