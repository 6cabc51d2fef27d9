// conv_p2_f8.hip -- conv_p2_kernel (conv_p2.h): the fp8 instances (a.f8) and the bf16 dgrad instances with the fused BN-backward reduction (a.nred > 0)
#include "conv_p2_launch.h"

int ys_conv_p2_dispatch_f8_red(hipStream_t st, const ConvArgs& a, const P2Plan& p) {
#define P2(M_, N_) if (p.mr == M_ && p.nr == N_) { if (a.f8) P2F(M_, N_, 1, 0) else P2F(M_, N_, 0, 1) }
  P2_TILES
#undef P2
  ys_set_error("conv p2: no kernel for NT=%d MR=%d NR=%d", p.nt, p.mr, p.nr);
  return YS_ERR_UNSUPPORTED;
}
