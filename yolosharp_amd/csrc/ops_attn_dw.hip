// ops_attn_dw.hip -- per-kernel test entries of the C ABI on the YOLOv11-only operators (attn_dw.hip), one call per kernel family.  Host arrays in and out,
// nothing a training step calls.  The operands sit inside WIDER NHWC device buffers, as in the model's shared activation buffers; everything outside the
// views is a sentinel that must survive the call.
#include "ops_stage.h"

namespace {
struct AttnBufs {
  PadView qkv, ao;
  DevBuf P;
  size_t pp = 0;     // elements of a [B*heads][N][N] matrix
};

int attn_args(const char* who, ys_ctx* ctx, int dtype, const float* qkv, int B, int N, int heads, int kd, int hd, int ldq_pad, int ldo_pad) {
  YS_REQUIRE(ctx && qkv, "%s: null argument", who);
  YS_REQUIRE(dtype == YS_F32 || dtype == YS_BF16, "%s: bad dtype %d", who, dtype);
  YS_REQUIRE(B >= 1 && heads >= 1 && ldq_pad >= 0 && ldo_pad >= 0, "%s: B=%d heads=%d ldq_pad=%d ldo_pad=%d", who, B, heads, ldq_pad, ldo_pad);
  YS_TRY(ys_attn_supported(N, kd, hd));           // the launchers' own refusal, before anything is staged
  YS_REQUIRE((2 * kd + hd) % ys_epl(dtype) == 0 && hd % ys_epl(dtype) == 0, "%s: kd=%d hd=%d: channel counts must be multiples of %d", who, kd, hd, ys_epl(dtype));
  return YS_OK;
}

// qkv staged into its padded view, ao / P pre-filled, ys_attn_fwd_launch
int attn_forward_staged(hipStream_t st, int dtype, const float* qkv, int B, int N, int heads, int kd, int hd, int ldq_pad, int ldo_pad, AttnBufs& b) {
  const int Cq = heads * (2 * kd + hd), Co = heads * hd;
  b.pp = (size_t)B * heads * N * N;
  YS_TRY(b.qkv.alloc(st, dtype, (long)B * N, Cq, Cq + ldq_pad, 0));
  YS_TRY(b.ao.alloc(st, dtype, (long)B * N, Co, Co + ldo_pad, 0));
  YS_TRY(alloc_filled(b.P, (b.pp + kGuardFloats) * 4, st));
  YS_TRY(b.qkv.stage(st, qkv, B));
  return ys_attn_fwd_launch(st, dtype, b.qkv.p, b.qkv.ld, B, N, heads, kd, hd, b.ao.p, b.ao.ld, (float*)b.P.p);
}
}  // namespace

extern "C" int ys_attn_fwd(ys_ctx* ctx, int dtype, const float* qkv, int B, int N, int heads, int kd, int hd, int ldq_pad, int ldo_pad,
                           float* ao, float* P, int32_t* view_intact) {
  YS_TRY(attn_args("ys_attn_fwd", ctx, dtype, qkv, B, N, heads, kd, hd, ldq_pad, ldo_pad));
  YS_REQUIRE(ao, "ys_attn_fwd: null argument");
  YS_CHECK_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  AttnBufs b;
  YS_TRY(attn_forward_staged(st, dtype, qkv, B, N, heads, kd, hd, ldq_pad, ldo_pad, b));
  YS_TRY(b.ao.fetch(st, ao, B));
  if (P) YS_TRY(d2h(st, P, b.P.p, b.pp * 4));
  int ok = 1;
  YS_TRY(b.ao.check(st, &ok));
  YS_TRY(b.qkv.check(st, &ok));
  YS_TRY(check_guard(st, b.P.p, b.pp * 4, &ok));
  YS_CHECK_HIP(hipStreamSynchronize(st));
  YS_CHECK_HIP(hipGetLastError());
  if (view_intact) *view_intact = ok;
  return YS_OK;
}

extern "C" int ys_attn_bwd(ys_ctx* ctx, int dtype, const float* qkv, int B, int N, int heads, int kd, int hd, int ldq_pad, int ldo_pad,
                           const float* dao, const float* dv_in, float* dqkv, int32_t* view_intact) {
  YS_TRY(attn_args("ys_attn_bwd", ctx, dtype, qkv, B, N, heads, kd, hd, ldq_pad, ldo_pad));
  YS_REQUIRE(dao && dqkv, "ys_attn_bwd: null argument");
  YS_CHECK_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  AttnBufs b;
  YS_TRY(attn_forward_staged(st, dtype, qkv, B, N, heads, kd, hd, ldq_pad, ldo_pad, b));
  const int Cq = b.qkv.C, Co = b.ao.C;
  PadView ddao, dgrad;
  DevBuf dS;
  YS_TRY(ddao.alloc(st, dtype, b.ao.rows, Co, b.ao.ld, 0));
  YS_TRY(dgrad.alloc(st, dtype, b.qkv.rows, Cq, b.qkv.ld, 0));
  YS_TRY(alloc_filled(dS, (b.pp + kGuardFloats) * 4, st));
  YS_TRY(ddao.stage(st, dao, B));
  // the gradient buffer on entry: dv_in in the v slices (the kernels add to it); the q / k slices hold the sentinel value, so an
  // element the kernels fail to write shows in the result
  const int hs = 2 * kd + hd;
  std::vector<float> init((size_t)b.qkv.rows * Cq);
  const float sent = ys_u2f(0x01010101u * (unsigned)kSentinelByte);
  for (int bi = 0; bi < B; bi++)
    for (int c = 0; c < Cq; c++) {
      const int h = c / hs, j = c - h * hs;
      float* dst = init.data() + ((size_t)bi * Cq + c) * N;
      const float* src = (j >= 2 * kd && dv_in) ? dv_in + ((size_t)bi * Co + h * hd + (j - 2 * kd)) * N : nullptr;
      for (int n = 0; n < N; n++) dst[n] = j < 2 * kd ? sent : (src ? src[n] : 0.f);
    }
  YS_TRY(dgrad.stage(st, init.data(), B));
  YS_TRY(ys_attn_bwd_launch(st, dtype, b.qkv.p, b.qkv.ld, B, N, heads, kd, hd, ddao.p, ddao.ld, (const float*)b.P.p, (float*)dS.p, dgrad.p));
  YS_TRY(dgrad.fetch(st, dqkv, B));
  int ok = 1;
  YS_TRY(dgrad.check(st, &ok));
  YS_TRY(ddao.check(st, &ok));
  YS_TRY(b.qkv.check(st, &ok));
  YS_TRY(b.ao.check(st, &ok));
  YS_TRY(check_guard(st, b.P.p, b.pp * 4, &ok));
  YS_TRY(check_guard(st, dS.p, b.pp * 4, &ok));
  YS_CHECK_HIP(hipStreamSynchronize(st));
  YS_CHECK_HIP(hipGetLastError());
  if (view_intact) *view_intact = ok;
  return YS_OK;
}

namespace {
int dwconv_args(const char* who, ys_ctx* ctx, int dtype, const float* x, int B, int C, int H, int W, const float* w, int x_ldc, int x_coff,
                int o_ldc, int o_coff) {
  YS_REQUIRE(ctx && x && w, "%s: null argument", who);
  YS_REQUIRE(dtype == YS_F32 || dtype == YS_BF16, "%s: bad dtype %d", who, dtype);
  YS_REQUIRE(B >= 1 && C >= 1 && H >= 1 && W >= 1, "%s: B=%d C=%d H=%d W=%d", who, B, C, H, W);
  YS_TRY(ys_dwconv_supported(dtype, C));
  YS_TRY(view_on_grid(who, dtype, C, x_ldc, x_coff));
  return view_on_grid(who, dtype, C, o_ldc, o_coff);
}
// [C][1][3][3] host -> tap-major [9][C] device
int dw_weights(hipStream_t st, const float* w, int C, DevBuf& d) {
  std::vector<float> wt((size_t)9 * C);
  for (int c = 0; c < C; c++)
    for (int t = 0; t < 9; t++) wt[(size_t)t * C + c] = w[(size_t)c * 9 + t];
  YS_TRY(d.alloc(wt.size() * 4));
  YS_TRY(h2d(st, d.p, wt.data(), wt.size() * 4));
  YS_CHECK_HIP(hipStreamSynchronize(st));
  return YS_OK;
}
}  // namespace

extern "C" int ys_dwconv3x3_fwd(ys_ctx* ctx, int dtype, const float* x, int B, int C, int H, int W, const float* w,
                                int x_ldc, int x_coff, int y_ldc, int y_coff, float* y, int32_t* view_intact) {
  YS_TRY(dwconv_args("ys_dwconv3x3_fwd", ctx, dtype, x, B, C, H, W, w, x_ldc, x_coff, y_ldc, y_coff));
  YS_REQUIRE(y, "ys_dwconv3x3_fwd: null argument");
  YS_CHECK_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const long rows = (long)B * H * W;
  PadView vx, vy;
  DevBuf dw;
  YS_TRY(vx.alloc(st, dtype, rows, C, x_ldc, x_coff));
  YS_TRY(vy.alloc(st, dtype, rows, C, y_ldc, y_coff));
  YS_TRY(vx.stage(st, x, B));
  YS_TRY(dw_weights(st, w, C, dw));
  YS_TRY(ys_dwconv_launch(st, dtype, 0, vx.p, x_ldc, x_coff, B, H, W, C, (const float*)dw.p, vy.p, y_ldc, y_coff, 0));
  YS_TRY(vy.fetch(st, y, B));
  int ok = 1;
  YS_TRY(vy.check(st, &ok));
  YS_TRY(vx.check(st, &ok));
  YS_CHECK_HIP(hipGetLastError());
  if (view_intact) *view_intact = ok;
  return YS_OK;
}

extern "C" int ys_dwconv3x3_bwd(ys_ctx* ctx, int dtype, const float* x, int B, int C, int H, int W, const float* w, const float* dy,
                                int x_ldc, int x_coff, int dx_ldc, int dx_coff, int accumulate, float* dx, float* dw,
                                int32_t* view_intact) {
  YS_TRY(dwconv_args("ys_dwconv3x3_bwd", ctx, dtype, x, B, C, H, W, w, x_ldc, x_coff, dx_ldc, dx_coff));
  YS_REQUIRE(dy && (dx || dw), "ys_dwconv3x3_bwd: null argument");
  if (dw) YS_TRY(ys_dwconv_wgrad_supported(dtype, C));
  YS_CHECK_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const long rows = (long)B * H * W;
  PadView vx, vdx;
  DevBuf bdy, bw, bpart, bgrad;
  YS_TRY(vx.alloc(st, dtype, rows, C, x_ldc, x_coff));
  YS_TRY(bdy.alloc((size_t)rows * C * ys_es(dtype)));           // the incoming gradient is dense in the model too (the depthwise layer's own buffer)
  YS_TRY(vx.stage(st, x, B));
  YS_TRY(stage_view(st, dtype, dy, B, C, (long)H * W, bdy.p, C, 0));
  int ok = 1;
  if (dx) {
    YS_TRY(vdx.alloc(st, dtype, rows, C, dx_ldc, dx_coff));      // without `accumulate` the view itself starts as the sentinel: an unwritten element shows
    if (accumulate) YS_TRY(vdx.stage(st, dx, B));
    YS_TRY(dw_weights(st, w, C, bw));
    YS_TRY(ys_dwconv_launch(st, dtype, 1, bdy.p, C, 0, B, H, W, C, (const float*)bw.p, vdx.p, dx_ldc, dx_coff, accumulate ? 1 : 0));
    YS_TRY(vdx.fetch(st, dx, B));
    YS_TRY(vdx.check(st, &ok));
  }
  if (dw) {
    const size_t np = (size_t)ys_dwconv_wgrad_blocks(rows, C, dtype) * 9 * C;
    YS_TRY(alloc_filled(bpart, (np + kGuardFloats) * 4, st));
    YS_TRY(bgrad.alloc((size_t)9 * C * 4));
    YS_CHECK_HIP(hipMemsetAsync(bgrad.p, 0, (size_t)9 * C * 4, st));
    YS_TRY(ys_dwconv_wgrad_launch(st, dtype, vx.p, x_ldc, x_coff, bdy.p, B, H, W, C, (float*)bpart.p, (float*)bgrad.p));
    std::vector<float> g((size_t)9 * C);
    YS_TRY(d2h(st, g.data(), bgrad.p, g.size() * 4));
    YS_CHECK_HIP(hipStreamSynchronize(st));
    for (int c = 0; c < C; c++)
      for (int t = 0; t < 9; t++) dw[(size_t)c * 9 + t] = g[(size_t)t * C + c];
    YS_TRY(check_guard(st, bpart.p, np * 4, &ok));
  }
  YS_TRY(vx.check(st, &ok));
  YS_CHECK_HIP(hipStreamSynchronize(st));
  YS_CHECK_HIP(hipGetLastError());
  if (view_intact) *view_intact = ok;
  return YS_OK;
}
