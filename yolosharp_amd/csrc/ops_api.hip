// ops_api.hip -- per-operator entry points of the C ABI (unit parity; a TorchSharp-free Conv wrapper).
#include "ys_internal.h"
#include "ys_kernels.h"
#include <cstring>
#include <vector>

namespace {
struct DevBuf {
  void* p = nullptr;
  ~DevBuf() { if (p) hipFree(p); }
  int alloc(size_t n) { hipError_t e = hipMalloc(&p, n ? n : 16); return e == hipSuccess ? YS_OK : YS_ERR_OOM; }
};
}  // namespace

// stat_mode 0: the convolution writes one statistics row per workgroup row, ys_bn_finalize_launch + ys_bn_act_apply_launch.
// stat_mode 1: what run_conv_fwd does for a model with BN_ATOMIC = 1 -- the epilogues add their sums into zeroed fixed-point accumulators
// (ConvArgs::stat_acc, a.stats stays the take-statistics flag) and ys_bn_fin_apply_launch finalizes from them inside the apply pass.
static int conv_bn_act_fwd_impl(ys_ctx* ctx, int dtype, const float* x_nchw, int B, int Cin, int H, int W,
                                const float* w_oihw, int Cout, int k, int stride, const float* bn_gamma,
                                const float* bn_beta, float* bn_mean, float* bn_var, const float* bias,
                                int act_silu, int training, int stat_mode, float* y_nchw, float* y_raw, float* coef, int32_t* stat_rows,
                                float prev_amax = 0.f, float* f8_scales = nullptr, float* f8_amax = nullptr) {
  YS_REQUIRE(ctx && x_nchw && w_oihw && y_nchw, "ys_conv_bn_act_fwd: null argument");
  YS_REQUIRE(dtype == YS_F32 || dtype == YS_BF16 || dtype == YS_FP8, "ys_conv_bn_act_fwd: bad dtype %d", dtype);
  YS_REQUIRE((k == 1 || k == 3) && (stride == 1 || stride == 2), "ys_conv_bn_act_fwd: k=%d stride=%d unsupported", k, stride);
  YS_REQUIRE(stat_mode == 0 || stat_mode == 1, "ys_conv_bn_act_fwd: stat_mode %d", stat_mode);
  YS_REQUIRE(!(stat_mode == 1 && dtype == YS_FP8), "ys_conv_bn_act_fwd: the fp8 mode keeps statistics rows (stat_mode 0)");
  YS_REQUIRE(!(y_raw || coef || stat_rows) || (bn_gamma && training), "ys_conv_bn_act_fwd: y_raw / coef / stat_rows exist for training-mode BatchNorm only");
  // YS_FP8: bf16 storage; the convolution runs the fp8 MFMA kernel with CURRENT per-tensor scales of this call's own tensors
  // (s_w = 448 / amax|W|, s_x = 0.5 * 448 / amax|bf16(x)|, the recipe of f8.hip) when Cin % 32 == 0, else the bf16 kernel
  const bool want_f8 = dtype == YS_FP8;
  if (want_f8) dtype = YS_BF16;
  const bool has_bn = bn_gamma != nullptr;
  YS_REQUIRE(!has_bn || (bn_beta && bn_mean && bn_var), "ys_conv_bn_act_fwd: incomplete BN arguments");
  YS_CHECK_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const int epl = dtype == YS_BF16 ? 8 : 4;
  const size_t es = dtype == YS_BF16 ? 2 : 4;
  const int cpad = (Cin + epl - 1) / epl * epl;
  const int pad = k / 2;
  const int Ho = (H + 2 * pad - k) / stride + 1, Wo = (W + 2 * pad - k) / stride + 1;
  const int taps = k * k;
  const long M = (long)B * Ho * Wo;
  const int cout_ld = (Cout + epl - 1) / epl * epl;

  // host: OIHW -> [Cout][taps][Cin]
  std::vector<float> wint((size_t)Cout * taps * Cin);
  for (int co = 0; co < Cout; co++)
    for (int ci = 0; ci < Cin; ci++)
      for (int t = 0; t < taps; t++) wint[((size_t)co * taps + t) * Cin + ci] = w_oihw[((size_t)co * Cin + ci) * taps + t];

  DevBuf dx, dxn, dwm, dwf, dy, dz, dstat, dacc, dpar, dout;
  YS_TRY(dx.alloc((size_t)B * Cin * H * W * 4));
  YS_TRY(dxn.alloc((size_t)B * H * W * cpad * es));
  YS_TRY(dwm.alloc(wint.size() * 4));
  YS_TRY(dwf.alloc((size_t)Cout * taps * cpad * es));
  YS_TRY(dy.alloc((size_t)M * cout_ld * es));
  YS_TRY(dz.alloc((size_t)M * cout_ld * es));
  YS_TRY(dout.alloc((size_t)M * Cout * 4));
  YS_CHECK_HIP(hipMemsetAsync(dy.p, 0, (size_t)M * cout_ld * es, st));
  YS_CHECK_HIP(hipMemsetAsync(dz.p, 0, (size_t)M * cout_ld * es, st));
  YS_CHECK_HIP(hipMemcpyAsync(dx.p, x_nchw, (size_t)B * Cin * H * W * 4, hipMemcpyHostToDevice, st));
  YS_CHECK_HIP(hipMemcpyAsync(dwm.p, wint.data(), wint.size() * 4, hipMemcpyHostToDevice, st));
  YS_TRY(ys_pack_input_launch(st, dtype, (const float*)dx.p, B, Cin, H, W, cpad, dxn.p));
  YS_TRY(ys_weight_prep_launch(st, dtype, (const float*)dwm.p, Cout, taps, Cin, cpad, cout_ld, dwf.p, nullptr, 0));

  // per-channel parameter block: gamma, beta, rmean, rvar, scale, shift, mean, rstd, bias, nbt
  YS_TRY(dpar.alloc((size_t)Cout * 10 * 4));
  float* par = (float*)dpar.p;
  float *g = par, *bt = par + Cout, *rm = par + 2 * Cout, *rv = par + 3 * Cout, *sc = par + 4 * Cout, *sh = par + 5 * Cout,
        *mu = par + 6 * Cout, *rs = par + 7 * Cout, *bs = par + 8 * Cout, *nbt = par + 9 * Cout;
  if (has_bn) {
    YS_CHECK_HIP(hipMemcpyAsync(g, bn_gamma, Cout * 4, hipMemcpyHostToDevice, st));
    YS_CHECK_HIP(hipMemcpyAsync(bt, bn_beta, Cout * 4, hipMemcpyHostToDevice, st));
    YS_CHECK_HIP(hipMemcpyAsync(rm, bn_mean, Cout * 4, hipMemcpyHostToDevice, st));
    YS_CHECK_HIP(hipMemcpyAsync(rv, bn_var, Cout * 4, hipMemcpyHostToDevice, st));
  }
  if (bias) YS_CHECK_HIP(hipMemcpyAsync(bs, bias, Cout * 4, hipMemcpyHostToDevice, st));
  YS_CHECK_HIP(hipMemsetAsync(nbt, 0, Cout * 4, st));

  ConvArgs a{};
  a.x = dxn.p; a.w = dwf.p;
  DevBuf dw8, dq, dq8;
  if (want_f8 && Cin % 32 == 0) {
    YS_TRY(dw8.alloc((size_t)Cout * taps * cpad));
    YS_TRY(dq8.alloc((size_t)B * H * W * cpad));   // fp8 image of the input for the blocked-GEMM kernel (quantised by ys_conv_launch)
    YS_TRY(dq.alloc(1024));                     // floats: [0] amax_w, [16..80) amax_x ways, [96..160) amax_dy ways, [200..204) scales
    YS_CHECK_HIP(hipMemsetAsync(dq.p, 0, 1024, st));
    float* qf = (float*)dq.p;
    F8Layer hl{0, (long)Cout * taps * Cin};
    F8Conv hc{0};
    DevBuf dl, dc;
    YS_TRY(dl.alloc(sizeof hl)); YS_TRY(dc.alloc(sizeof hc));
    YS_CHECK_HIP(hipMemcpyAsync(dl.p, &hl, sizeof hl, hipMemcpyHostToDevice, st));
    YS_CHECK_HIP(hipMemcpyAsync(dc.p, &hc, sizeof hc, hipMemcpyHostToDevice, st));
    YS_TRY(ys_f8_weight_amax_launch(st, (const float*)dwm.p, (const F8Layer*)dl.p, 1, qf));
    // delayed scaling (ys_conv_f8_fwd): the caller's amax of an EARLIER step stands in the slot instead of this input's own
    if (prev_amax > 0.f) YS_CHECK_HIP(hipMemcpyAsync(qf + 16, &prev_amax, 4, hipMemcpyHostToDevice, st));
    else YS_TRY(ys_f8_view_amax_launch(st, dxn.p, (long)B * H * W, cpad, cpad, 0, (unsigned*)(qf + 16)));
    YS_TRY(ys_f8_scales_launch(st, (const F8Conv*)dc.p, 1, qf, (unsigned*)(qf + 16), (unsigned*)(qf + 96), qf + 200));
    YS_TRY(ys_f8_quant_weights_launch(st, dwf.p, (long)Cout * taps * cpad, qf, dw8.p));
    YS_CHECK_HIP(hipStreamSynchronize(st));     // hl / hc / dl / dc are temporaries of this scope
    a.f8 = 1; a.w8 = dw8.p; a.qscale = qf + 200; a.deq = qf + 201; a.q8 = dq8.p;
    if (f8_amax) a.amax = (unsigned*)(qf + 16);   // the slots the scales launch just cleared: the launch records amax(|input|) as a model's step does
  }
  a.B = B; a.Hin = H; a.Win = W; a.Cin = cpad; a.Hout = Ho; a.Wout = Wo; a.Cout = Cout; a.KH = k; a.KW = k;
  a.SA = stride; a.DIVS = 0; a.DIVM = 0; a.PAD = pad;
  a.in_ldc = cpad; a.in_coff = 0; a.in_bstride = (long)H * W;
  a.out_ldc = cout_ld; a.out_coff = 0; a.out_bstride = (long)Ho * Wo;
  a.vec_ok = 1; a.M = (int)M;
  const void* result = nullptr;
  if (has_bn && training) {
    YS_REQUIRE(Cout % epl == 0, "ys_conv_bn_act_fwd: training BN needs Cout %% %d == 0", epl);
    const int gm = ys_conv_grid_m(a, dtype);
    YS_TRY(dstat.alloc((size_t)gm * 2 * Cout * 4));
    a.y = dy.p; a.stats = (float*)dstat.p;
    if (stat_mode == 1) {
      const size_t accb = (size_t)YS_STAT_SHARDS * Cout * 2 * sizeof(unsigned long long);
      YS_TRY(dacc.alloc(accb));
      YS_CHECK_HIP(hipMemsetAsync(dacc.p, 0, accb, st));      // one clear per forward, as ys_model_forward does for every unit
      a.stat_acc = (unsigned long long*)dacc.p;
      YS_TRY(ys_conv_launch(st, dtype, a));
      BnAccFin f{};
      f.acc = (const unsigned long long*)dacc.p; f.count = (double)M;
      f.gamma = g; f.beta = bt; f.run_mean = rm; f.run_var = rv; f.nbt = nbt;
      f.scale = sc; f.shift = sh; f.mean = mu; f.rstd = rs; f.eps = 1e-3f; f.momentum = 0.03f;
      YS_TRY(ys_bn_fin_apply_launch(st, dtype, dy.p, M, Cout, f, act_silu, nullptr, 0, 0, dz.p, cout_ld, 0));
    } else {
      YS_TRY(ys_conv_launch(st, dtype, a));
      YS_TRY(ys_bn_finalize_launch(st, (const float*)dstat.p, gm, Cout, M, g, bt, 1e-3f, 0.03f, rm, rv, nbt, sc, sh, mu, rs));
      YS_TRY(ys_bn_act_apply_launch(st, dtype, dy.p, M, Cout, sc, sh, act_silu, nullptr, 0, 0, dz.p, cout_ld, 0));
    }
    result = dz.p;
    if (stat_rows) *stat_rows = gm;
    if (coef) YS_CHECK_HIP(hipMemcpyAsync(coef, sc, (size_t)4 * Cout * 4, hipMemcpyDeviceToHost, st));      // scale, shift, mean, rstd are adjacent in the parameter block
    if (y_raw) {
      YS_TRY(ys_unpack_nchw_launch(st, dtype, dy.p, cout_ld, 0, B, Cout, (long)Ho * Wo, (float*)dout.p));
      YS_CHECK_HIP(hipMemcpyAsync(y_raw, dout.p, (size_t)M * Cout * 4, hipMemcpyDeviceToHost, st));
    }
    YS_CHECK_HIP(hipMemcpyAsync(bn_mean, rm, Cout * 4, hipMemcpyDeviceToHost, st));
    YS_CHECK_HIP(hipMemcpyAsync(bn_var, rv, Cout * 4, hipMemcpyDeviceToHost, st));
  } else {
    if (has_bn) {
      YS_TRY(ys_bn_eval_coeffs_launch(st, Cout, g, bt, rm, rv, 1e-3f, sc, sh));
      a.scale = sc; a.shift = sh;
    } else if (bias) {
      a.shift = bs;
    }
    a.act = act_silu && (a.scale || a.shift) ? 1 : 0;
    YS_REQUIRE(!(act_silu && !a.scale && !a.shift), "ys_conv_bn_act_fwd: activation without BN/bias is not a reference configuration");
    a.y = dz.p;
    YS_TRY(ys_conv_launch(st, dtype, a));
    result = dz.p;
  }
  YS_TRY(ys_unpack_nchw_launch(st, dtype, result, cout_ld, 0, B, Cout, (long)Ho * Wo, (float*)dout.p));
  YS_CHECK_HIP(hipMemcpyAsync(y_nchw, dout.p, (size_t)M * Cout * 4, hipMemcpyDeviceToHost, st));
  if (a.f8 && f8_scales) YS_CHECK_HIP(hipMemcpyAsync(f8_scales, (const float*)dq.p + 200, 16, hipMemcpyDeviceToHost, st));
  float ways[YS_AMAX_WAYS] = {};
  if (a.f8 && f8_amax) YS_CHECK_HIP(hipMemcpyAsync(ways, (const float*)dq.p + 16, sizeof ways, hipMemcpyDeviceToHost, st));
  YS_CHECK_HIP(hipStreamSynchronize(st));
  YS_CHECK_HIP(hipGetLastError());
  if (f8_amax) { float m = 0.f; for (float v : ways) m = v > m ? v : m; *f8_amax = m; }
  return YS_OK;
}

extern "C" int ys_conv_f8_fwd(ys_ctx* ctx, const float* x_nchw, int B, int Cin, int H, int W, const float* w_oihw, int Cout, int k, int stride,
                              const float* bn_gamma, const float* bn_beta, float* bn_mean, float* bn_var, const float* bias, int act_silu, int training,
                              float prev_amax, float* y_nchw, float* y_raw, float* coef, int32_t* stat_rows, float* scales, float* amax) {
  YS_REQUIRE(scales && amax, "ys_conv_f8_fwd: null argument");
  YS_REQUIRE(Cin >= 32 && Cin % 32 == 0, "ys_conv_f8_fwd: Cin=%d (the fp8 kernels take multiples of 32 input channels)", Cin);
  YS_REQUIRE(prev_amax >= 0.f && prev_amax < __builtin_inff(), "ys_conv_f8_fwd: prev_amax must be finite and >= 0");
  return conv_bn_act_fwd_impl(ctx, YS_FP8, x_nchw, B, Cin, H, W, w_oihw, Cout, k, stride, bn_gamma, bn_beta, bn_mean, bn_var, bias, act_silu, training, 0,
                              y_nchw, y_raw, coef, stat_rows, prev_amax, scales, amax);
}

extern "C" int ys_conv_bn_act_fwd(ys_ctx* ctx, int dtype, const float* x_nchw, int B, int Cin, int H, int W,
                                  const float* w_oihw, int Cout, int k, int stride, const float* bn_gamma,
                                  const float* bn_beta, float* bn_mean, float* bn_var, const float* bias,
                                  int act_silu, int training, float* y_nchw) {
  return conv_bn_act_fwd_impl(ctx, dtype, x_nchw, B, Cin, H, W, w_oihw, Cout, k, stride, bn_gamma, bn_beta, bn_mean, bn_var, bias, act_silu, training, 0,
                              y_nchw, nullptr, nullptr, nullptr);
}

extern "C" int ys_conv_bn_act_fwd_ex(ys_ctx* ctx, int dtype, const float* x_nchw, int B, int Cin, int H, int W,
                                     const float* w_oihw, int Cout, int k, int stride, const float* bn_gamma,
                                     const float* bn_beta, float* bn_mean, float* bn_var, const float* bias,
                                     int act_silu, int training, int stat_mode, float* y_nchw, float* y_raw, float* coef, int32_t* stat_rows) {
  return conv_bn_act_fwd_impl(ctx, dtype, x_nchw, B, Cin, H, W, w_oihw, Cout, k, stride, bn_gamma, bn_beta, bn_mean, bn_var, bias, act_silu, training,
                              training && bn_gamma ? stat_mode : 0, y_nchw, y_raw, coef, stat_rows);
}

// Gradients of y = conv2d(x, w, stride, padding=k/2) given dy (autograd of torch.nn.Conv2d, reached from
// Amp.cs:348,370): dx [B,Cin,H,W] (may be null) and dw [Cout,Cin,k,k], all fp32 NCHW/OIHW host arrays.
// dw_oihw == nullptr (ys_conv_f8_dgrad): the input gradient alone, x_nchw unused
static int conv_bwd_impl(ys_ctx* ctx, int dtype, const float* x_nchw, int B, int Cin, int H, int W,
                         const float* w_oihw, int Cout, int k, int stride, const float* dy_nchw,
                         float* dx_nchw, float* dw_oihw, float prev_amax, float* f8_scales, float* f8_amax) {
  YS_REQUIRE(ctx && w_oihw && dy_nchw && (dw_oihw ? x_nchw != nullptr : dx_nchw != nullptr), "ys_conv_bwd: null argument");
  YS_REQUIRE(dtype == YS_F32 || dtype == YS_BF16 || dtype == YS_FP8, "ys_conv_bwd: bad dtype %d", dtype);
  const bool want_f8 = dtype == YS_FP8;           // dgrad on the fp8 kernel (dy -> e5m2, weights -> e4m3, current scales); wgrad stays bf16
  if (want_f8) dtype = YS_BF16;
  YS_REQUIRE((k == 1 || k == 3) && (stride == 1 || stride == 2), "ys_conv_bwd: k=%d stride=%d unsupported", k, stride);
  YS_CHECK_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const int epl = dtype == YS_BF16 ? 8 : 4;
  const size_t es = dtype == YS_BF16 ? 2 : 4;
  const int cpad = (Cin + epl - 1) / epl * epl, copad = (Cout + epl - 1) / epl * epl;
  const int pad = k / 2, taps = k * k;
  const int Ho = (H + 2 * pad - k) / stride + 1, Wo = (W + 2 * pad - k) / stride + 1;
  const long M = (long)B * Ho * Wo;
  std::vector<float> wint((size_t)Cout * taps * Cin);
  for (int co = 0; co < Cout; co++)
    for (int ci = 0; ci < Cin; ci++)
      for (int t = 0; t < taps; t++) wint[((size_t)co * taps + t) * Cin + ci] = w_oihw[((size_t)co * Cin + ci) * taps + t];
  DevBuf dx, dxn, ddy, ddyn, dwm, dwf, dwd, dgx, dgxo, dgw, dpart;
  YS_TRY(dx.alloc((size_t)B * Cin * H * W * 4));
  YS_TRY(dxn.alloc((size_t)B * H * W * cpad * es));
  YS_TRY(ddy.alloc((size_t)M * Cout * 4));
  YS_TRY(ddyn.alloc((size_t)M * copad * es));
  YS_TRY(dwm.alloc(wint.size() * 4));
  YS_TRY(dwf.alloc((size_t)Cout * taps * cpad * es));
  YS_TRY(dwd.alloc((size_t)Cin * taps * copad * es));
  YS_TRY(dgx.alloc((size_t)B * H * W * cpad * es));
  YS_TRY(dgxo.alloc((size_t)B * Cin * H * W * 4));
  YS_TRY(dgw.alloc(wint.size() * 4));
  YS_CHECK_HIP(hipMemsetAsync(dgx.p, 0, (size_t)B * H * W * cpad * es, st));
  YS_CHECK_HIP(hipMemsetAsync(dgw.p, 0, wint.size() * 4, st));
  if (dw_oihw) YS_CHECK_HIP(hipMemcpyAsync(dx.p, x_nchw, (size_t)B * Cin * H * W * 4, hipMemcpyHostToDevice, st));
  YS_CHECK_HIP(hipMemcpyAsync(ddy.p, dy_nchw, (size_t)M * Cout * 4, hipMemcpyHostToDevice, st));
  YS_CHECK_HIP(hipMemcpyAsync(dwm.p, wint.data(), wint.size() * 4, hipMemcpyHostToDevice, st));
  if (dw_oihw) YS_TRY(ys_pack_input_launch(st, dtype, (const float*)dx.p, B, Cin, H, W, cpad, dxn.p));
  YS_TRY(ys_pack_input_launch(st, dtype, (const float*)ddy.p, B, Cout, Ho, Wo, copad, ddyn.p));
  YS_TRY(ys_weight_prep_launch(st, dtype, (const float*)dwm.p, Cout, taps, Cin, cpad, copad, dwf.p, dwd.p, ys_conv_dgrad_uses_phases(dtype, k, stride) ? 1 : 0));
  std::vector<float> gw(dw_oihw ? wint.size() : 0);
  if (dw_oihw) {
    WgradArgs wa{};
    wa.x = dxn.p; wa.dy = ddyn.p;
    wa.B = B; wa.Hin = H; wa.Win = W; wa.Cin = cpad; wa.Hout = Ho; wa.Wout = Wo; wa.Cout = Cout; wa.KH = wa.KW = k;
    wa.stride = stride; wa.pad = pad; wa.in_ldc = cpad; wa.in_coff = 0; wa.in_bstride = (long)H * W;
    wa.dy_ldc = copad; wa.dy_coff = 0; wa.dy_bstride = (long)Ho * Wo; wa.M = (int)M;
    const int splits = ys_wgrad_splits(wa, dtype);
    YS_TRY(dpart.alloc((size_t)splits * Cout * taps * cpad * 4));
    wa.partial = (float*)dpart.p;
    YS_TRY(ys_wgrad_launch(st, dtype, wa, splits, Cin, (float*)dgw.p));
    YS_CHECK_HIP(hipMemcpyAsync(gw.data(), dgw.p, gw.size() * 4, hipMemcpyDeviceToHost, st));
  }
  float ways[YS_AMAX_WAYS] = {};
  if (dx_nchw) {
    ConvArgs a{};
    a.x = ddyn.p; a.w = dwd.p; a.y = dgx.p;
    DevBuf dw8, dq, dq8;
    if (want_f8 && Cout % 32 == 0) {
      YS_TRY(dw8.alloc((size_t)Cin * taps * copad));
      YS_TRY(dq8.alloc((size_t)M * copad));
      YS_TRY(dq.alloc(1024));
      YS_CHECK_HIP(hipMemsetAsync(dq.p, 0, 1024, st));
      float* qf = (float*)dq.p;
      F8Layer hl{0, (long)Cout * taps * Cin};
      F8Conv hc{0};
      DevBuf dl, dc;
      YS_TRY(dl.alloc(sizeof hl)); YS_TRY(dc.alloc(sizeof hc));
      YS_CHECK_HIP(hipMemcpyAsync(dl.p, &hl, sizeof hl, hipMemcpyHostToDevice, st));
      YS_CHECK_HIP(hipMemcpyAsync(dc.p, &hc, sizeof hc, hipMemcpyHostToDevice, st));
      YS_TRY(ys_f8_weight_amax_launch(st, (const float*)dwm.p, (const F8Layer*)dl.p, 1, qf));
      if (prev_amax > 0.f) YS_CHECK_HIP(hipMemcpyAsync(qf + 96, &prev_amax, 4, hipMemcpyHostToDevice, st));     // delayed scaling: see conv_bn_act_fwd_impl
      else YS_TRY(ys_f8_view_amax_launch(st, ddyn.p, M, copad, copad, 0, (unsigned*)(qf + 96)));
      YS_TRY(ys_f8_scales_launch(st, (const F8Conv*)dc.p, 1, qf, (unsigned*)(qf + 16), (unsigned*)(qf + 96), qf + 200));
      YS_TRY(ys_f8_quant_weights_launch(st, dwd.p, (long)Cin * taps * copad, qf, dw8.p));
      YS_CHECK_HIP(hipStreamSynchronize(st));
      a.f8 = 2; a.w8 = dw8.p; a.qscale = qf + 202; a.deq = qf + 203; a.q8 = dq8.p;
      if (f8_amax) a.amax = (unsigned*)(qf + 96);
    }
    a.B = B; a.Hin = Ho; a.Win = Wo; a.Cin = copad; a.Hout = H; a.Wout = W; a.Cout = Cin; a.KH = a.KW = k;
    a.SA = 1; a.DIVS = stride == 2 ? 1 : 0; a.DIVM = stride - 1; a.PAD = k - 1 - pad;
    a.in_ldc = copad; a.in_coff = 0; a.in_bstride = (long)Ho * Wo;
    a.out_ldc = cpad; a.out_coff = 0; a.out_bstride = (long)H * W; a.vec_ok = 1; a.M = B * H * W;
    YS_TRY(ys_conv_launch(st, dtype, a));
    YS_TRY(ys_unpack_nchw_launch(st, dtype, dgx.p, cpad, 0, B, Cin, (long)H * W, (float*)dgxo.p));
    YS_CHECK_HIP(hipMemcpyAsync(dx_nchw, dgxo.p, (size_t)B * Cin * H * W * 4, hipMemcpyDeviceToHost, st));
    if (a.f8 && f8_scales) YS_CHECK_HIP(hipMemcpyAsync(f8_scales, (const float*)dq.p + 200, 16, hipMemcpyDeviceToHost, st));
    if (a.f8 && f8_amax) YS_CHECK_HIP(hipMemcpyAsync(ways, (const float*)dq.p + 96, sizeof ways, hipMemcpyDeviceToHost, st));
    YS_CHECK_HIP(hipStreamSynchronize(st));     // dw8 / dq / dq8 are temporaries of this scope
  }
  YS_CHECK_HIP(hipStreamSynchronize(st));
  if (dw_oihw)
    for (int co = 0; co < Cout; co++)
      for (int ci = 0; ci < Cin; ci++)
        for (int t = 0; t < taps; t++) dw_oihw[((size_t)co * Cin + ci) * taps + t] = gw[((size_t)co * taps + t) * Cin + ci];
  YS_CHECK_HIP(hipGetLastError());
  if (f8_amax) { float m = 0.f; for (float v : ways) m = v > m ? v : m; *f8_amax = m; }
  return YS_OK;
}

extern "C" int ys_conv_bwd(ys_ctx* ctx, int dtype, const float* x_nchw, int B, int Cin, int H, int W,
                           const float* w_oihw, int Cout, int k, int stride, const float* dy_nchw,
                           float* dx_nchw, float* dw_oihw) {
  YS_REQUIRE(x_nchw && dw_oihw, "ys_conv_bwd: null argument");
  return conv_bwd_impl(ctx, dtype, x_nchw, B, Cin, H, W, w_oihw, Cout, k, stride, dy_nchw, dx_nchw, dw_oihw, 0.f, nullptr, nullptr);
}

extern "C" int ys_conv_f8_dgrad(ys_ctx* ctx, int B, int Cin, int H, int W, const float* w_oihw, int Cout, int k, int stride, const float* dy_nchw,
                                float prev_amax, float* dx_nchw, float* scales, float* amax) {
  YS_REQUIRE(dx_nchw && scales && amax, "ys_conv_f8_dgrad: null argument");
  YS_REQUIRE(Cout >= 32 && Cout % 32 == 0, "ys_conv_f8_dgrad: Cout=%d (the fp8 kernels take multiples of 32 gradient channels)", Cout);
  YS_REQUIRE(prev_amax >= 0.f && prev_amax < __builtin_inff(), "ys_conv_f8_dgrad: prev_amax must be finite and >= 0");
  return conv_bwd_impl(ctx, YS_FP8, nullptr, B, Cin, H, W, w_oihw, Cout, k, stride, dy_nchw, dx_nchw, nullptr, prev_amax, scales, amax);
}

// ------------------------------------------------------------------ YOLOv11-only operators (attn_dw.hip), one call per kernel family
// The operands sit inside WIDER NHWC device buffers, as in the model's shared activation buffers; everything outside the views is a
// sentinel that must survive the call.
namespace {
constexpr int kSentinelByte = 0x4E;          // bf16 0x4E4E = fp32 0x4E4E4E4E = 8.65e8: finite, and ruinous when a kernel reads it as data
constexpr size_t kGuardFloats = 64;          // sentinel floats behind the [B*heads][N][N] matrices
inline int ys_epl(int dtype) { return dtype == YS_BF16 ? 8 : 4; }
inline size_t ys_es(int dtype) { return dtype == YS_BF16 ? 2 : 4; }

int alloc_filled(DevBuf& b, size_t bytes, hipStream_t st) {
  YS_TRY(b.alloc(bytes));
  YS_CHECK_HIP(hipMemsetAsync(b.p, kSentinelByte, bytes ? bytes : 16, st));
  return YS_OK;
}

// fp32 NCHW host tensor [B][C][rpb] -> channels [coff, coff + C) of the pre-filled [B*rpb][ld] device buffer `wide`
int stage_view(hipStream_t st, int dtype, const float* host, int B, int C, long rpb, void* wide, int ld, int coff) {
  const int epl = ys_epl(dtype);
  const size_t es = ys_es(dtype);
  const long rows = (long)B * rpb;
  DevBuf d32, compact;
  YS_TRY(d32.alloc((size_t)rows * C * 4));
  YS_TRY(compact.alloc((size_t)rows * C * es));
  YS_CHECK_HIP(hipMemcpyAsync(d32.p, host, (size_t)rows * C * 4, hipMemcpyHostToDevice, st));
  YS_TRY(ys_pack_input_launch(st, dtype, (const float*)d32.p, B, C, 1, (int)rpb, C, compact.p));
  if (ld % epl == 0 && coff % epl == 0) {
    YS_TRY(ys_copy_view_launch(st, dtype, compact.p, C, 0, rows, C, wide, ld, coff, 0));
  } else {
    // a pitch off the 16-byte grid (the scalar attention kernels accept it; ys_copy_view_launch moves 16-byte vectors): rows placed by the host
    std::vector<char> hc((size_t)rows * C * es), hw((size_t)rows * ld * es);
    YS_CHECK_HIP(hipMemcpyAsync(hc.data(), compact.p, hc.size(), hipMemcpyDeviceToHost, st));
    YS_CHECK_HIP(hipMemcpyAsync(hw.data(), wide, hw.size(), hipMemcpyDeviceToHost, st));
    YS_CHECK_HIP(hipStreamSynchronize(st));
    for (long r = 0; r < rows; r++) memcpy(hw.data() + ((size_t)r * ld + coff) * es, hc.data() + (size_t)r * C * es, (size_t)C * es);
    YS_CHECK_HIP(hipMemcpyAsync(wide, hw.data(), hw.size(), hipMemcpyHostToDevice, st));
  }
  YS_CHECK_HIP(hipStreamSynchronize(st));      // d32 / compact are temporaries of this scope
  return YS_OK;
}

// channels [coff, coff + C) of a [B*rpb][ld] device buffer -> fp32 NCHW host tensor
int fetch_view(hipStream_t st, int dtype, const void* wide, int ld, int coff, int B, int C, long rpb, float* host) {
  DevBuf d32;
  const size_t n = (size_t)B * C * rpb;
  YS_TRY(d32.alloc(n * 4));
  YS_TRY(ys_unpack_nchw_launch(st, dtype, wide, ld, coff, B, C, rpb, (float*)d32.p));
  YS_CHECK_HIP(hipMemcpyAsync(host, d32.p, n * 4, hipMemcpyDeviceToHost, st));
  YS_CHECK_HIP(hipStreamSynchronize(st));
  return YS_OK;
}

// *ok &= every byte of the [rows][ld] buffer outside channels [coff, coff + C) is still the sentinel
int check_sentinel(hipStream_t st, const void* wide, long rows, int ld, int coff, int C, size_t es, int* ok) {
  if (ld == C) return YS_OK;
  std::vector<unsigned char> h((size_t)rows * ld * es);
  YS_CHECK_HIP(hipMemcpyAsync(h.data(), wide, h.size(), hipMemcpyDeviceToHost, st));
  YS_CHECK_HIP(hipStreamSynchronize(st));
  const size_t lo = (size_t)coff * es, hi = (size_t)(coff + C) * es, pitch = (size_t)ld * es;
  for (long r = 0; r < rows; r++)
    for (size_t i = 0; i < pitch; i++) {
      if (i == lo) i = hi;
      if (i < pitch && h[(size_t)r * pitch + i] != kSentinelByte) { *ok = 0; return YS_OK; }
    }
  return YS_OK;
}
// ... and the kGuardFloats behind the `n` floats of a workspace matrix
int check_guard(hipStream_t st, const void* base, size_t n, int* ok) {
  unsigned char h[kGuardFloats * 4];
  YS_CHECK_HIP(hipMemcpyAsync(h, (const float*)base + n, sizeof h, hipMemcpyDeviceToHost, st));
  YS_CHECK_HIP(hipStreamSynchronize(st));
  for (size_t i = 0; i < sizeof h; i++)
    if (h[i] != kSentinelByte) *ok = 0;
  return YS_OK;
}

struct AttnBufs {
  DevBuf qkv, ao, P;
  int Cq = 0, Co = 0, ldq = 0, ldo = 0;
  long rows = 0;
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
  const size_t es = ys_es(dtype);
  b.Cq = heads * (2 * kd + hd); b.Co = heads * hd; b.ldq = b.Cq + ldq_pad; b.ldo = b.Co + ldo_pad;
  b.rows = (long)B * N; b.pp = (size_t)B * heads * N * N;
  YS_TRY(alloc_filled(b.qkv, (size_t)b.rows * b.ldq * es, st));
  YS_TRY(alloc_filled(b.ao, (size_t)b.rows * b.ldo * es, st));
  YS_TRY(alloc_filled(b.P, (b.pp + kGuardFloats) * 4, st));
  YS_TRY(stage_view(st, dtype, qkv, B, b.Cq, N, b.qkv.p, b.ldq, 0));
  return ys_attn_fwd_launch(st, dtype, b.qkv.p, b.ldq, B, N, heads, kd, hd, b.ao.p, b.ldo, (float*)b.P.p);
}
}  // namespace

extern "C" int ys_attn_fwd(ys_ctx* ctx, int dtype, const float* qkv, int B, int N, int heads, int kd, int hd, int ldq_pad, int ldo_pad,
                           float* ao, float* P, int32_t* view_intact) {
  YS_TRY(attn_args("ys_attn_fwd", ctx, dtype, qkv, B, N, heads, kd, hd, ldq_pad, ldo_pad));
  YS_REQUIRE(ao, "ys_attn_fwd: null argument");
  YS_CHECK_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const size_t es = ys_es(dtype);
  AttnBufs b;
  YS_TRY(attn_forward_staged(st, dtype, qkv, B, N, heads, kd, hd, ldq_pad, ldo_pad, b));
  YS_TRY(fetch_view(st, dtype, b.ao.p, b.ldo, 0, B, b.Co, N, ao));
  if (P) YS_CHECK_HIP(hipMemcpyAsync(P, b.P.p, b.pp * 4, hipMemcpyDeviceToHost, st));
  int ok = 1;
  YS_TRY(check_sentinel(st, b.ao.p, b.rows, b.ldo, 0, b.Co, es, &ok));
  YS_TRY(check_sentinel(st, b.qkv.p, b.rows, b.ldq, 0, b.Cq, es, &ok));
  YS_TRY(check_guard(st, b.P.p, b.pp, &ok));
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
  const size_t es = ys_es(dtype);
  AttnBufs b;
  YS_TRY(attn_forward_staged(st, dtype, qkv, B, N, heads, kd, hd, ldq_pad, ldo_pad, b));
  DevBuf ddao, dgrad, dS;
  YS_TRY(alloc_filled(ddao, (size_t)b.rows * b.ldo * es, st));
  YS_TRY(alloc_filled(dgrad, (size_t)b.rows * b.ldq * es, st));
  YS_TRY(alloc_filled(dS, (b.pp + kGuardFloats) * 4, st));
  YS_TRY(stage_view(st, dtype, dao, B, b.Co, N, ddao.p, b.ldo, 0));
  // the gradient buffer on entry: dv_in in the v slices (the kernels add to it); the q / k slices hold the sentinel value, so an
  // element the kernels fail to write shows in the result
  const int hs = 2 * kd + hd;
  std::vector<float> init((size_t)b.rows * b.Cq);
  float sent; { sent = ys_u2f(0x01010101u * (unsigned)kSentinelByte); }
  for (int bi = 0; bi < B; bi++)
    for (int c = 0; c < b.Cq; c++) {
      const int h = c / hs, j = c - h * hs;
      float* dst = init.data() + ((size_t)bi * b.Cq + c) * N;
      const float* src = (j >= 2 * kd && dv_in) ? dv_in + ((size_t)bi * b.Co + h * hd + (j - 2 * kd)) * N : nullptr;
      for (int n = 0; n < N; n++) dst[n] = j < 2 * kd ? sent : (src ? src[n] : 0.f);
    }
  YS_TRY(stage_view(st, dtype, init.data(), B, b.Cq, N, dgrad.p, b.ldq, 0));
  YS_TRY(ys_attn_bwd_launch(st, dtype, b.qkv.p, b.ldq, B, N, heads, kd, hd, ddao.p, b.ldo, (const float*)b.P.p, (float*)dS.p, dgrad.p));
  YS_TRY(fetch_view(st, dtype, dgrad.p, b.ldq, 0, B, b.Cq, N, dqkv));
  int ok = 1;
  YS_TRY(check_sentinel(st, dgrad.p, b.rows, b.ldq, 0, b.Cq, es, &ok));
  YS_TRY(check_sentinel(st, ddao.p, b.rows, b.ldo, 0, b.Co, es, &ok));
  YS_TRY(check_sentinel(st, b.qkv.p, b.rows, b.ldq, 0, b.Cq, es, &ok));
  YS_TRY(check_sentinel(st, b.ao.p, b.rows, b.ldo, 0, b.Co, es, &ok));
  YS_TRY(check_guard(st, b.P.p, b.pp, &ok));
  YS_TRY(check_guard(st, dS.p, b.pp, &ok));
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
  const int epl = ys_epl(dtype);
  YS_REQUIRE(x_coff >= 0 && o_coff >= 0 && x_ldc >= x_coff + C && o_ldc >= o_coff + C && x_ldc % epl == 0 && x_coff % epl == 0 && o_ldc % epl == 0 && o_coff % epl == 0,
             "%s: views (ldc %d coff %d), (ldc %d coff %d) must hold C=%d channels on the %d-element vector grid", who, x_ldc, x_coff, o_ldc, o_coff, C, epl);
  return YS_OK;
}
// [C][1][3][3] host -> tap-major [9][C] device
int dw_weights(hipStream_t st, const float* w, int C, DevBuf& d) {
  std::vector<float> wt((size_t)9 * C);
  for (int c = 0; c < C; c++)
    for (int t = 0; t < 9; t++) wt[(size_t)t * C + c] = w[(size_t)c * 9 + t];
  YS_TRY(d.alloc(wt.size() * 4));
  YS_CHECK_HIP(hipMemcpyAsync(d.p, wt.data(), wt.size() * 4, hipMemcpyHostToDevice, st));
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
  const size_t es = ys_es(dtype);
  const long rows = (long)B * H * W;
  DevBuf dx, dy, dw;
  YS_TRY(alloc_filled(dx, (size_t)rows * x_ldc * es, st));
  YS_TRY(alloc_filled(dy, (size_t)rows * y_ldc * es, st));
  YS_TRY(stage_view(st, dtype, x, B, C, (long)H * W, dx.p, x_ldc, x_coff));
  YS_TRY(dw_weights(st, w, C, dw));
  YS_TRY(ys_dwconv_launch(st, dtype, 0, dx.p, x_ldc, x_coff, B, H, W, C, (const float*)dw.p, dy.p, y_ldc, y_coff, 0));
  YS_TRY(fetch_view(st, dtype, dy.p, y_ldc, y_coff, B, C, (long)H * W, y));
  int ok = 1;
  YS_TRY(check_sentinel(st, dy.p, rows, y_ldc, y_coff, C, es, &ok));
  YS_TRY(check_sentinel(st, dx.p, rows, x_ldc, x_coff, C, es, &ok));
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
  const size_t es = ys_es(dtype);
  const long rows = (long)B * H * W;
  DevBuf bx, bdy, bdx, bw, bpart, bgrad;
  YS_TRY(alloc_filled(bx, (size_t)rows * x_ldc * es, st));
  YS_TRY(bdy.alloc((size_t)rows * C * es));           // the incoming gradient is dense in the model too (the depthwise layer's own buffer)
  YS_TRY(stage_view(st, dtype, x, B, C, (long)H * W, bx.p, x_ldc, x_coff));
  YS_TRY(stage_view(st, dtype, dy, B, C, (long)H * W, bdy.p, C, 0));
  int ok = 1;
  if (dx) {
    YS_TRY(alloc_filled(bdx, (size_t)rows * dx_ldc * es, st));      // without `accumulate` the view itself starts as the sentinel: an unwritten element shows
    if (accumulate) YS_TRY(stage_view(st, dtype, dx, B, C, (long)H * W, bdx.p, dx_ldc, dx_coff));
    YS_TRY(dw_weights(st, w, C, bw));
    YS_TRY(ys_dwconv_launch(st, dtype, 1, bdy.p, C, 0, B, H, W, C, (const float*)bw.p, bdx.p, dx_ldc, dx_coff, accumulate ? 1 : 0));
    YS_TRY(fetch_view(st, dtype, bdx.p, dx_ldc, dx_coff, B, C, (long)H * W, dx));
    YS_TRY(check_sentinel(st, bdx.p, rows, dx_ldc, dx_coff, C, es, &ok));
  }
  if (dw) {
    const size_t np = (size_t)ys_dwconv_wgrad_blocks(rows, C, dtype) * 9 * C;
    YS_TRY(alloc_filled(bpart, (np + kGuardFloats) * 4, st));
    YS_TRY(bgrad.alloc((size_t)9 * C * 4));
    YS_CHECK_HIP(hipMemsetAsync(bgrad.p, 0, (size_t)9 * C * 4, st));
    YS_TRY(ys_dwconv_wgrad_launch(st, dtype, bx.p, x_ldc, x_coff, bdy.p, B, H, W, C, (float*)bpart.p, (float*)bgrad.p));
    std::vector<float> g((size_t)9 * C);
    YS_CHECK_HIP(hipMemcpyAsync(g.data(), bgrad.p, g.size() * 4, hipMemcpyDeviceToHost, st));
    YS_CHECK_HIP(hipStreamSynchronize(st));
    for (int c = 0; c < C; c++)
      for (int t = 0; t < 9; t++) dw[(size_t)c * 9 + t] = g[(size_t)t * C + c];
    YS_TRY(check_guard(st, bpart.p, np, &ok));
  }
  YS_TRY(check_sentinel(st, bx.p, rows, x_ldc, x_coff, C, es, &ok));
  YS_CHECK_HIP(hipStreamSynchronize(st));
  YS_CHECK_HIP(hipGetLastError());
  if (view_intact) *view_intact = ok;
  return YS_OK;
}

// ------------------------------------------------------------------ BatchNorm training kernels of batchnorm.hip, one call per launch sequence
// Host tensors are channel-major [C][rows] (NCHW with B = 1).  y / dy are dense [rows][C] on the device as in the model (a unit's own buffers); z, res, dz and
// rg sit inside sentinel-padded views; partial-row workspaces and dy carry a sentinel guard behind them.
namespace {
constexpr int kEwMaxVec = 256;               // vectors per row the channel-reduction launchers take (EW_THREADS of batchnorm.hip)

// ys_stat_acc_add on test-supplied partial rows [P][2][C]: one thread per (row, which, channel) -- the device function every convolution epilogue calls
__global__ void __launch_bounds__(256)
stat_acc_push_kernel(const float* __restrict__ partial, int P, int C, unsigned long long* __restrict__ acc) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)P * 2 * C) return;
  const long row = i / (2L * C);
  const int which = (int)((i / C) & 1), c = (int)(i % C);
  ys_stat_acc_add(acc, row, C, c, which, partial[i]);
}

// *ok &= every byte of the [rows][ld] buffer outside the nv channel ranges v[k] = {coff, C} is still the sentinel
int check_sentinel_views(hipStream_t st, const void* wide, long rows, int ld, const int (*v)[2], int nv, size_t es, int* ok) {
  std::vector<unsigned char> h((size_t)rows * ld * es);
  YS_CHECK_HIP(hipMemcpyAsync(h.data(), wide, h.size(), hipMemcpyDeviceToHost, st));
  YS_CHECK_HIP(hipStreamSynchronize(st));
  const size_t pitch = (size_t)ld * es;
  for (long r = 0; r < rows; r++)
    for (int c = 0; c < ld; c++) {
      bool in = false;
      for (int k = 0; k < nv; k++) in |= c >= v[k][0] && c < v[k][0] + v[k][1];
      if (in) continue;
      for (size_t b = 0; b < es; b++)
        if (h[(size_t)r * pitch + (size_t)c * es + b] != kSentinelByte) { *ok = 0; return YS_OK; }
    }
  return YS_OK;
}

int view_ok(const char* who, int dtype, int C, int pad, int coff) {
  const int epl = ys_epl(dtype);
  YS_REQUIRE(pad >= 0 && coff >= 0 && pad % epl == 0 && coff % epl == 0, "%s: view (pad %d, coff %d) must sit on the %d-element vector grid (C = %d)", who, pad, coff, epl, C);
  return YS_OK;
}
int h2d(hipStream_t st, void* d, const void* h, size_t bytes) { YS_CHECK_HIP(hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, st)); return YS_OK; }
int d2h(hipStream_t st, void* h, const void* d, size_t bytes) { YS_CHECK_HIP(hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, st)); return YS_OK; }

struct BnFwdBufs {
  DevBuf y, z, res, par, part, acc;
  int ldz = 0, ldr = 0, nblk = 0;
  size_t npart = 0;
  float *g, *bt, *rm, *rv, *sc, *sh, *mu, *rs, *nbt;
  const void* resp = nullptr;
};
struct BnBwdBufs {
  DevBuf dz, y, rg, dy, par, part, srcp[YS_BNRED_MAXSEG];
  int ldd = 0, ldg = 0, nblk = 0;
  size_t npart = 0;
  float *sc, *sh, *mu, *rs, *dg, *db, *k2, *k3;
};
}  // namespace

extern "C" int ys_bn_train_fwd(ys_ctx* ctx, int dtype, int mode, int act, int n, ys_bn_fwd_case* cases) {
  YS_REQUIRE(ctx && cases, "ys_bn_train_fwd: null argument");
  YS_REQUIRE(dtype == YS_F32 || dtype == YS_BF16, "ys_bn_train_fwd: bad dtype %d", dtype);
  YS_REQUIRE(mode >= 0 && mode <= 2 && n >= 1 && (mode == 2 || n == 1), "ys_bn_train_fwd: mode %d with %d problems", mode, n);
  YS_CHECK_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const int epl = ys_epl(dtype);
  const size_t es = ys_es(dtype);
  if (n > YS_EW_GROUP_MAX) {                  // the grouped launcher's own refusal, before anything is staged
    std::vector<BnFinProb> none((size_t)n);
    return ys_bn_finalize_group_launch(st, none.data(), n, 1e-3f, 0.03f);
  }
  for (int i = 0; i < n; i++) {
    const ys_bn_fwd_case& c = cases[i];
    YS_REQUIRE(c.y && c.gamma && c.beta && c.run_mean && c.run_var && c.z && c.coef, "ys_bn_train_fwd: problem %d: null argument", i);
    YS_REQUIRE(c.rows >= 1 && c.C >= epl && c.C % epl == 0, "ys_bn_train_fwd: problem %d: rows=%d C=%d (C must be a multiple of %d)", i, c.rows, c.C, epl);
    YS_TRY(view_ok("ys_bn_train_fwd z", dtype, c.C, c.z_pad, c.z_coff));
    if (c.res) YS_TRY(view_ok("ys_bn_train_fwd res", dtype, c.C, c.res_pad, c.res_coff));
    YS_REQUIRE(!(c.res && c.res_shares_z) || c.res_coff + c.C <= c.z_coff || c.z_coff + c.C <= c.res_coff, "ys_bn_train_fwd: problem %d: res and z views overlap", i);
    YS_REQUIRE(mode != 1 || (c.partial && c.P >= 1), "ys_bn_train_fwd: mode 1 needs partial rows");
    // ys_chan_stats_launch's limit (one workgroup row holds every vector of a pixel), checked here so that nothing is staged or launched first
    if (mode != 1 && c.C / epl > kEwMaxVec) { ys_set_error("chan_stats: unsupported channel count %d", c.C); return YS_ERR_UNSUPPORTED; }
  }
  BnFwdBufs bufs[YS_EW_GROUP_MAX];
  for (int i = 0; i < n; i++) {
    ys_bn_fwd_case& c = cases[i];
    BnFwdBufs& b = bufs[i];
    const int C = c.C; const long rows = c.rows;
    const bool shared = c.res && c.res_shares_z;
    b.ldz = c.z_coff + C + c.z_pad;
    if (shared && c.res_coff + C + c.z_pad > b.ldz) b.ldz = c.res_coff + C + c.z_pad;
    YS_TRY(alloc_filled(b.z, (size_t)rows * b.ldz * es, st));
    if (c.res) {
      b.ldr = shared ? b.ldz : c.res_coff + C + c.res_pad;
      if (!shared) YS_TRY(alloc_filled(b.res, (size_t)rows * b.ldr * es, st));
      b.resp = shared ? b.z.p : b.res.p;
      YS_TRY(stage_view(st, dtype, c.res, 1, C, rows, (void*)b.resp, b.ldr, c.res_coff));
    }
    YS_TRY(b.y.alloc((size_t)rows * C * es));
    YS_TRY(stage_view(st, dtype, c.y, 1, C, rows, b.y.p, C, 0));
    YS_TRY(b.par.alloc((size_t)9 * C * 4));
    float* par = (float*)b.par.p;
    b.g = par; b.bt = par + C; b.rm = par + 2 * C; b.rv = par + 3 * C; b.sc = par + 4 * C; b.sh = par + 5 * C; b.mu = par + 6 * C; b.rs = par + 7 * C;
    b.nbt = c.nbt ? par + 8 * C : nullptr;
    YS_CHECK_HIP(hipMemsetAsync(par, 0, (size_t)9 * C * 4, st));
    YS_TRY(h2d(st, b.g, c.gamma, (size_t)C * 4)); YS_TRY(h2d(st, b.bt, c.beta, (size_t)C * 4));
    YS_TRY(h2d(st, b.rm, c.run_mean, (size_t)C * 4)); YS_TRY(h2d(st, b.rv, c.run_var, (size_t)C * 4));
    if (c.nbt) YS_TRY(h2d(st, b.nbt, c.nbt, 4));
    if (mode == 1) {
      const size_t accb = (size_t)YS_STAT_SHARDS * C * 2 * sizeof(unsigned long long), np = (size_t)c.P * 2 * C;
      YS_TRY(b.part.alloc(np * 4));
      YS_TRY(h2d(st, b.part.p, c.partial, np * 4));
      YS_TRY(alloc_filled(b.acc, accb + kGuardFloats * 4, st));
      YS_CHECK_HIP(hipMemsetAsync(b.acc.p, 0, accb, st));
      const float* rows_p = (const float*)b.part.p;        // plain values: the interpreter build's launch captures its arguments by copy
      unsigned long long* acc_p = (unsigned long long*)b.acc.p;
      const int P = c.P;
      YS_LAUNCH(stat_acc_push_kernel, ys_cdiv((long)np, 256), 256, st, rows_p, P, C, acc_p);
      BnAccFin f{};
      f.acc = (const unsigned long long*)b.acc.p; f.count = (double)rows;
      f.gamma = b.g; f.beta = b.bt; f.run_mean = b.rm; f.run_var = b.rv; f.nbt = b.nbt;
      f.scale = b.sc; f.shift = b.sh; f.mean = b.mu; f.rstd = b.rs; f.eps = 1e-3f; f.momentum = 0.03f;
      YS_TRY(ys_bn_fin_apply_launch(st, dtype, b.y.p, rows, C, f, act, b.resp, b.ldr, c.res_coff, b.z.p, b.ldz, c.z_coff));
    } else {
      b.npart = (size_t)ys_colsum_blocks(rows, C, dtype) * 2 * C;
      YS_TRY(alloc_filled(b.part, (b.npart + kGuardFloats) * 4, st));
      YS_TRY(ys_chan_stats_launch(st, dtype, b.y.p, rows, C, (float*)b.part.p, &b.nblk));
      YS_REQUIRE((size_t)b.nblk * 2 * C == b.npart, "ys_bn_train_fwd: the launcher wrote %d partial rows, %zu were reserved", b.nblk, b.npart / (2 * (size_t)C));
      if (mode == 0) {
        YS_TRY(ys_bn_finalize_launch(st, (const float*)b.part.p, b.nblk, C, rows, b.g, b.bt, 1e-3f, 0.03f, b.rm, b.rv, b.nbt, b.sc, b.sh, b.mu, b.rs));
        YS_TRY(ys_bn_act_apply_launch(st, dtype, b.y.p, rows, C, b.sc, b.sh, act, b.resp, b.ldr, c.res_coff, b.z.p, b.ldz, c.z_coff));
      }
    }
  }
  if (mode == 2) {
    BnFinProb fp[YS_EW_GROUP_MAX]; BnApplyProb ap[YS_EW_GROUP_MAX];
    for (int i = 0; i < n; i++) {
      const BnFwdBufs& b = bufs[i];
      fp[i] = BnFinProb{(const float*)b.part.p, b.nblk, cases[i].C, (double)cases[i].rows, b.g, b.bt, b.rm, b.rv, b.nbt, b.sc, b.sh, b.mu, b.rs};
      ap[i] = BnApplyProb{b.y.p, (long)cases[i].rows, cases[i].C, b.sc, b.sh, b.resp, b.ldr, cases[i].res_coff, b.z.p, b.ldz, cases[i].z_coff};
    }
    YS_TRY(ys_bn_finalize_group_launch(st, fp, n, 1e-3f, 0.03f));
    YS_TRY(ys_bn_act_apply_group_launch(st, dtype, ap, n, act));
  }
  for (int i = 0; i < n; i++) {
    ys_bn_fwd_case& c = cases[i];
    BnFwdBufs& b = bufs[i];
    const int C = c.C; const long rows = c.rows;
    YS_TRY(fetch_view(st, dtype, b.z.p, b.ldz, c.z_coff, 1, C, rows, c.z));
    YS_TRY(d2h(st, c.coef, b.sc, (size_t)4 * C * 4));
    YS_TRY(d2h(st, c.run_mean, b.rm, (size_t)C * 4)); YS_TRY(d2h(st, c.run_var, b.rv, (size_t)C * 4));
    if (c.nbt) YS_TRY(d2h(st, c.nbt, b.nbt, 4));
    c.nblk = b.nblk;
    if (c.part_out && mode != 1) YS_TRY(d2h(st, c.part_out, b.part.p, b.npart * 4));
    if (c.acc_out && mode == 1) YS_TRY(d2h(st, c.acc_out, b.acc.p, (size_t)YS_STAT_SHARDS * C * 2 * sizeof(unsigned long long)));
    int ok = 1;
    const int views[2][2] = {{c.z_coff, C}, {c.res_coff, C}};
    YS_TRY(check_sentinel_views(st, b.z.p, rows, b.ldz, views, c.res && c.res_shares_z ? 2 : 1, es, &ok));
    if (b.res.p) YS_TRY(check_sentinel(st, b.res.p, rows, b.ldr, c.res_coff, C, es, &ok));
    if (mode == 1) YS_TRY(check_guard(st, b.acc.p, (size_t)YS_STAT_SHARDS * C * 4, &ok));
    else YS_TRY(check_guard(st, b.part.p, b.npart, &ok));
    YS_CHECK_HIP(hipStreamSynchronize(st));
    c.view_intact = ok;
  }
  YS_CHECK_HIP(hipGetLastError());
  return YS_OK;
}

extern "C" int ys_bn_train_bwd(ys_ctx* ctx, int dtype, int mode, int act, int n, ys_bn_bwd_case* cases) {
  YS_REQUIRE(ctx && cases, "ys_bn_train_bwd: null argument");
  YS_REQUIRE(dtype == YS_F32 || dtype == YS_BF16, "ys_bn_train_bwd: bad dtype %d", dtype);
  YS_REQUIRE(mode >= 0 && mode <= 3 && n >= 1 && (mode == 2 || n == 1), "ys_bn_train_bwd: mode %d with %d problems", mode, n);
  YS_CHECK_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const int epl = ys_epl(dtype);
  const size_t es = ys_es(dtype);
  if (n > YS_EW_GROUP_MAX) {
    std::vector<ChanFinProb> none((size_t)n);
    return ys_bn_bwd_finalize_group_launch(st, none.data(), n);
  }
  for (int i = 0; i < n; i++) {
    const ys_bn_bwd_case& c = cases[i];
    YS_REQUIRE(c.coef && c.dgamma && c.dbeta && c.k23, "ys_bn_train_bwd: problem %d: null argument", i);
    YS_REQUIRE(c.rows >= 1 && c.C >= epl && c.C % epl == 0, "ys_bn_train_bwd: problem %d: rows=%d C=%d (C must be a multiple of %d)", i, c.rows, c.C, epl);
    if (mode == 3) {
      YS_REQUIRE(c.nsrc >= 1 && c.nsrc <= YS_BNRED_MAXSEG, "ys_bn_train_bwd: %d partial-row sources", c.nsrc);
      for (int k = 0; k < c.nsrc; k++) YS_REQUIRE(c.src_part[k] && c.src_nblk[k] >= 1, "ys_bn_train_bwd: source %d is empty", k);
      continue;
    }
    YS_REQUIRE(c.dz && c.y && c.dy, "ys_bn_train_bwd: problem %d: null argument", i);
    YS_TRY(view_ok("ys_bn_train_bwd dz", dtype, c.C, c.dz_pad, c.dz_coff));
    if (c.rg) YS_TRY(view_ok("ys_bn_train_bwd rg", dtype, c.C, c.rg_pad, c.rg_coff));
    if (c.C / epl > kEwMaxVec) { ys_set_error("bn_bwd: unsupported channel count %d", c.C); return YS_ERR_UNSUPPORTED; }   // ys_bn_bwd_reduce_launch's limit, before anything is staged
  }
  BnBwdBufs bufs[YS_EW_GROUP_MAX];
  for (int i = 0; i < n; i++) {
    ys_bn_bwd_case& c = cases[i];
    BnBwdBufs& b = bufs[i];
    const int C = c.C; const long rows = c.rows;
    YS_TRY(b.par.alloc((size_t)8 * C * 4));
    float* par = (float*)b.par.p;
    b.sc = par; b.sh = par + C; b.mu = par + 2 * C; b.rs = par + 3 * C; b.dg = par + 4 * C; b.db = par + 5 * C; b.k2 = par + 6 * C; b.k3 = par + 7 * C;
    YS_CHECK_HIP(hipMemsetAsync(par, kSentinelByte, (size_t)8 * C * 4, st));        // k2 / k3 start as the sentinel: an unwritten coefficient shows
    YS_TRY(h2d(st, b.sc, c.coef, (size_t)4 * C * 4));
    YS_TRY(h2d(st, b.dg, c.dgamma, (size_t)C * 4)); YS_TRY(h2d(st, b.db, c.dbeta, (size_t)C * 4));
    if (mode == 3) {
      FinSrc src{};
      src.n = c.nsrc;
      for (int k = 0; k < c.nsrc; k++) {
        const size_t nb = (size_t)c.src_nblk[k] * 2 * C * 4;
        YS_TRY(b.srcp[k].alloc(nb));
        YS_TRY(h2d(st, b.srcp[k].p, c.src_part[k], nb));
        src.p[k] = (const float*)b.srcp[k].p; src.nblk[k] = c.src_nblk[k]; src.c1[k] = c.src_c1[k];
      }
      YS_TRY(ys_bn_bwd_finalize_src_launch(st, src, C, rows, b.dg, b.db, b.k2, b.k3, b.sc, b.mu, b.rs));
      continue;
    }
    b.ldd = c.dz_coff + C + c.dz_pad;
    YS_TRY(alloc_filled(b.dz, (size_t)rows * b.ldd * es, st));
    YS_TRY(stage_view(st, dtype, c.dz, 1, C, rows, b.dz.p, b.ldd, c.dz_coff));
    YS_TRY(b.y.alloc((size_t)rows * C * es));
    YS_TRY(stage_view(st, dtype, c.y, 1, C, rows, b.y.p, C, 0));
    if (c.rg) {
      b.ldg = c.rg_coff + C + c.rg_pad;
      YS_TRY(alloc_filled(b.rg, (size_t)rows * b.ldg * es, st));
      YS_TRY(stage_view(st, dtype, c.rg, 1, C, rows, b.rg.p, b.ldg, c.rg_coff));
    }
    YS_TRY(alloc_filled(b.dy, (size_t)rows * C * es + kGuardFloats * 4, st));
    b.npart = (size_t)ys_colsum_blocks(rows, C, dtype) * 2 * C;
    YS_TRY(alloc_filled(b.part, (b.npart + kGuardFloats) * 4, st));
    YS_TRY(ys_bn_bwd_reduce_launch(st, dtype, b.dz.p, b.ldd, c.dz_coff, b.y.p, rows, C, b.sc, b.sh, b.mu, b.rs, act, mode == 0 ? b.rg.p : nullptr, b.ldg, c.rg_coff,
                                   (float*)b.part.p, &b.nblk));
    YS_REQUIRE((size_t)b.nblk * 2 * C == b.npart, "ys_bn_train_bwd: the launcher wrote %d partial rows, %zu were reserved", b.nblk, b.npart / (2 * (size_t)C));
    if (mode == 2) continue;
    YS_TRY(ys_bn_bwd_finalize_launch(st, (const float*)b.part.p, b.nblk, C, rows, b.dg, b.db, b.k2, b.k3, b.sc, b.mu, b.rs));
    YS_TRY(ys_bn_bwd_apply_launch(st, dtype, b.dz.p, b.ldd, c.dz_coff, b.y.p, rows, C, b.sc, b.sh, b.k2, b.k3, act, b.dy.p, nullptr, mode == 1 ? b.rg.p : nullptr,
                                  b.ldg, c.rg_coff));
  }
  if (mode == 2) {
    ChanFinProb fp[YS_EW_GROUP_MAX]; BnBwdProb bp[YS_EW_GROUP_MAX];
    for (int i = 0; i < n; i++) {
      const BnBwdBufs& b = bufs[i];
      FinSrc src{}; src.n = 1; src.p[0] = (const float*)b.part.p; src.nblk[0] = b.nblk; src.c1[0] = cases[i].C;
      fp[i] = ChanFinProb{src, cases[i].C, (double)cases[i].rows, b.dg, b.db, b.k2, b.k3, b.sc, b.mu, b.rs};
      bp[i] = BnBwdProb{b.dz.p, b.ldd, cases[i].dz_coff, b.y.p, (long)cases[i].rows, cases[i].C, b.sc, b.sh, b.k2, b.k3, b.dy.p, b.rg.p, b.ldg, cases[i].rg_coff};
    }
    YS_TRY(ys_bn_bwd_finalize_group_launch(st, fp, n));
    YS_TRY(ys_bn_bwd_apply_group_launch(st, dtype, bp, n, act));
  }
  for (int i = 0; i < n; i++) {
    ys_bn_bwd_case& c = cases[i];
    BnBwdBufs& b = bufs[i];
    const int C = c.C; const long rows = c.rows;
    YS_TRY(d2h(st, c.dgamma, b.dg, (size_t)C * 4)); YS_TRY(d2h(st, c.dbeta, b.db, (size_t)C * 4));
    YS_TRY(d2h(st, c.k23, b.k2, (size_t)2 * C * 4));
    int ok = 1;
    if (mode != 3) {
      YS_TRY(fetch_view(st, dtype, b.dy.p, C, 0, 1, C, rows, c.dy));
      if (c.rg) YS_TRY(fetch_view(st, dtype, b.rg.p, b.ldg, c.rg_coff, 1, C, rows, c.rg));
      c.nblk = b.nblk;
      if (c.part_out) YS_TRY(d2h(st, c.part_out, b.part.p, b.npart * 4));
      YS_TRY(check_sentinel(st, b.dz.p, rows, b.ldd, c.dz_coff, C, es, &ok));
      if (c.rg) YS_TRY(check_sentinel(st, b.rg.p, rows, b.ldg, c.rg_coff, C, es, &ok));
      YS_TRY(check_guard(st, b.part.p, b.npart, &ok));
      YS_TRY(check_guard(st, b.dy.p, (size_t)rows * C * es / 4, &ok));
    }
    YS_CHECK_HIP(hipStreamSynchronize(st));
    c.view_intact = ok;
  }
  YS_CHECK_HIP(hipGetLastError());
  return YS_OK;
}

// grad[C] += column sums of x [B][C][rows_per_b] (chan_reduce_kernel MODE 1 + chan_finalize_kernel MODE 1, the bias gradients): the view starts at channel coff
// of a [B * bstride][coff + Cp + ld_pad] buffer, Cp = C rounded up to the vector width over ZEROED padding channels; images are bstride >= rows_per_b rows apart
// and the rows between them hold the sentinel.
extern "C" int ys_colsum(ys_ctx* ctx, int dtype, const float* x, int B, int C, int rows_per_b, int bstride, int ld_pad, int coff, float* grad,
                         int32_t* view_intact) {
  YS_REQUIRE(ctx && x && grad, "ys_colsum: null argument");
  YS_REQUIRE(dtype == YS_F32 || dtype == YS_BF16, "ys_colsum: bad dtype %d", dtype);
  YS_REQUIRE(B >= 1 && C >= 1 && rows_per_b >= 1 && bstride >= rows_per_b, "ys_colsum: B=%d C=%d rows_per_b=%d bstride=%d", B, C, rows_per_b, bstride);
  YS_TRY(view_ok("ys_colsum", dtype, C, ld_pad, coff));
  const int epl = ys_epl(dtype);
  const size_t es = ys_es(dtype);
  const int Cp = (C + epl - 1) / epl * epl, ld = coff + Cp + ld_pad;
  if (Cp / epl > kEwMaxVec) { ys_set_error("colsum: unsupported channel count %d", C); return YS_ERR_UNSUPPORTED; }    // ys_colsum_launch's limit, before anything is staged
  YS_CHECK_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const long rows = (long)B * rows_per_b, brows = (long)B * bstride;
  DevBuf dx, dpart, dgrad;
  YS_TRY(alloc_filled(dx, (size_t)brows * ld * es, st));
  std::vector<float> hp((size_t)Cp * rows_per_b, 0.f);
  for (int b = 0; b < B; b++) {
    memcpy(hp.data(), x + (size_t)b * C * rows_per_b, (size_t)C * rows_per_b * 4);
    YS_TRY(stage_view(st, dtype, hp.data(), 1, Cp, rows_per_b, (char*)dx.p + (size_t)b * bstride * ld * es, ld, coff));
  }
  const size_t np = (size_t)ys_colsum_blocks(rows, Cp, dtype) * 2 * Cp;
  YS_TRY(alloc_filled(dpart, (np + kGuardFloats) * 4, st));
  YS_TRY(alloc_filled(dgrad, ((size_t)C + kGuardFloats) * 4, st));
  YS_TRY(h2d(st, dgrad.p, grad, (size_t)C * 4));
  YS_TRY(ys_colsum_launch(st, dtype, dx.p, ld, coff, rows, rows_per_b, bstride, C, (float*)dpart.p, (float*)dgrad.p));
  YS_TRY(d2h(st, grad, dgrad.p, (size_t)C * 4));
  int ok = 1;
  YS_TRY(check_guard(st, dpart.p, np, &ok));
  YS_TRY(check_guard(st, dgrad.p, (size_t)C, &ok));
  YS_CHECK_HIP(hipStreamSynchronize(st));
  YS_CHECK_HIP(hipGetLastError());
  if (view_intact) *view_intact = ok;
  return YS_OK;
}

// Nearest 2x up-sample of src [B][C][H*W] into dst [B][C][4*H*W] (backward = 0), or its gradient: src [B][C][4*H*W] summed 2 x 2 into dst [B][C][H*W]
// (backward = 1; with accumulate != 0 dst holds the gradient already in the buffer and receives dst_in + sum, one rounding).  Both operands in padded views.
extern "C" int ys_upsample2x(ys_ctx* ctx, int dtype, int backward, const float* src, int B, int H, int W, int C, int s_ldc, int s_coff, int d_ldc, int d_coff,
                             int accumulate, float* dst, int32_t* view_intact) {
  YS_REQUIRE(ctx && src && dst, "ys_upsample2x: null argument");
  YS_REQUIRE(dtype == YS_F32 || dtype == YS_BF16, "ys_upsample2x: bad dtype %d", dtype);
  const int epl = ys_epl(dtype);
  const size_t es = ys_es(dtype);
  YS_REQUIRE(B >= 1 && H >= 1 && W >= 1 && C >= epl && C % epl == 0, "ys_upsample2x: B=%d H=%d W=%d C=%d", B, H, W, C);
  YS_REQUIRE(s_coff >= 0 && d_coff >= 0 && s_ldc >= s_coff + C && d_ldc >= d_coff + C && s_ldc % epl == 0 && s_coff % epl == 0 && d_ldc % epl == 0 && d_coff % epl == 0,
             "ys_upsample2x: views (ldc %d coff %d), (ldc %d coff %d) must hold C=%d channels on the %d-element vector grid", s_ldc, s_coff, d_ldc, d_coff, C, epl);
  YS_REQUIRE(!accumulate || backward, "ys_upsample2x: only the backward pass accumulates");
  YS_CHECK_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const long small = (long)H * W, big = 4 * small;
  const long srpb = backward ? big : small, drpb = backward ? small : big;
  DevBuf ds, dd;
  YS_TRY(alloc_filled(ds, (size_t)B * srpb * s_ldc * es, st));
  YS_TRY(alloc_filled(dd, (size_t)B * drpb * d_ldc * es, st));
  YS_TRY(stage_view(st, dtype, src, B, C, srpb, ds.p, s_ldc, s_coff));
  if (accumulate) YS_TRY(stage_view(st, dtype, dst, B, C, drpb, dd.p, d_ldc, d_coff));
  if (backward) YS_TRY(ys_upsample2x_bwd_launch(st, dtype, ds.p, s_ldc, s_coff, B, H, W, C, dd.p, d_ldc, d_coff, accumulate ? 1 : 0));
  else YS_TRY(ys_upsample2x_fwd_launch(st, dtype, ds.p, s_ldc, s_coff, B, H, W, C, dd.p, d_ldc, d_coff));
  YS_TRY(fetch_view(st, dtype, dd.p, d_ldc, d_coff, B, C, drpb, dst));
  int ok = 1;
  YS_TRY(check_sentinel(st, dd.p, (long)B * drpb, d_ldc, d_coff, C, es, &ok));
  YS_TRY(check_sentinel(st, ds.p, (long)B * srpb, s_ldc, s_coff, C, es, &ok));
  YS_CHECK_HIP(hipGetLastError());
  if (view_intact) *view_intact = ok;
  return YS_OK;
}

// dst view (+)= src view (copy_view_kernel): src, dst [C][rows]; with accumulate != 0 dst holds the destination's content on entry
extern "C" int ys_copy_view(ys_ctx* ctx, int dtype, const float* src, int rows, int C, int s_ldc, int s_coff, int d_ldc, int d_coff, int accumulate, float* dst,
                            int32_t* view_intact) {
  YS_REQUIRE(ctx && src && dst, "ys_copy_view: null argument");
  YS_REQUIRE(dtype == YS_F32 || dtype == YS_BF16, "ys_copy_view: bad dtype %d", dtype);
  const int epl = ys_epl(dtype);
  const size_t es = ys_es(dtype);
  YS_REQUIRE(rows >= 1 && C >= epl && C % epl == 0, "ys_copy_view: rows=%d C=%d", rows, C);
  YS_REQUIRE(s_coff >= 0 && d_coff >= 0 && s_ldc >= s_coff + C && d_ldc >= d_coff + C && s_ldc % epl == 0 && s_coff % epl == 0 && d_ldc % epl == 0 && d_coff % epl == 0,
             "ys_copy_view: views (ldc %d coff %d), (ldc %d coff %d) must hold C=%d channels on the %d-element vector grid", s_ldc, s_coff, d_ldc, d_coff, C, epl);
  YS_CHECK_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  DevBuf ds, dd;
  YS_TRY(alloc_filled(ds, (size_t)rows * s_ldc * es, st));
  YS_TRY(alloc_filled(dd, (size_t)rows * d_ldc * es, st));
  YS_TRY(stage_view(st, dtype, src, 1, C, rows, ds.p, s_ldc, s_coff));
  if (accumulate) YS_TRY(stage_view(st, dtype, dst, 1, C, rows, dd.p, d_ldc, d_coff));
  YS_TRY(ys_copy_view_launch(st, dtype, ds.p, s_ldc, s_coff, rows, C, dd.p, d_ldc, d_coff, accumulate ? 1 : 0));
  YS_TRY(fetch_view(st, dtype, dd.p, d_ldc, d_coff, 1, C, rows, dst));
  int ok = 1;
  YS_TRY(check_sentinel(st, dd.p, rows, d_ldc, d_coff, C, es, &ok));
  YS_TRY(check_sentinel(st, ds.p, rows, s_ldc, s_coff, C, es, &ok));
  YS_CHECK_HIP(hipGetLastError());
  if (view_intact) *view_intact = ok;
  return YS_OK;
}

// ------------------------------------------------------------------ scaling machinery of the fp8 path (f8.hip) and the quantising BatchNorm passes, one call per kernel
namespace {
// the YS_AMAX_WAYS slots of one tensor, zeroed, with a sentinel guard behind them
int alloc_slots(DevBuf& b, hipStream_t st) {
  YS_TRY(alloc_filled(b, (YS_AMAX_WAYS + kGuardFloats) * 4, st));
  YS_CHECK_HIP(hipMemsetAsync(b.p, 0, YS_AMAX_WAYS * 4, st));
  return YS_OK;
}
// slots -> host (optional), *amax = their maximum, guard checked
int fetch_slots(hipStream_t st, const DevBuf& b, float* slots, float* amax, int* ok) {
  float h[YS_AMAX_WAYS];
  YS_TRY(d2h(st, h, b.p, sizeof h));
  YS_TRY(check_guard(st, b.p, YS_AMAX_WAYS, ok));      // synchronizes
  float m = 0.f;
  for (int i = 0; i < YS_AMAX_WAYS; i++) { if (slots) slots[i] = h[i]; m = h[i] > m ? h[i] : m; }
  *amax = m;
  return YS_OK;
}
// *ok &= the kGuardFloats * 4 bytes behind the n bytes of an fp8 image are still the sentinel
int check_guard_bytes(hipStream_t st, const void* base, size_t n, int* ok) {
  unsigned char h[kGuardFloats * 4];
  YS_TRY(d2h(st, h, (const char*)base + n, sizeof h));
  YS_CHECK_HIP(hipStreamSynchronize(st));
  for (size_t i = 0; i < sizeof h; i++)
    if (h[i] != kSentinelByte) *ok = 0;
  return YS_OK;
}
int scalar_to_device(hipStream_t st, DevBuf& b, float v) {
  YS_TRY(b.alloc(16));
  YS_TRY(h2d(st, b.p, &v, 4));
  YS_CHECK_HIP(hipStreamSynchronize(st));     // v is the caller's local
  return YS_OK;
}
}  // namespace

extern "C" int ys_f8_quant(ys_ctx* ctx, int kind, const float* x, int rows, int C, int coff, int pad, float qscale, uint8_t* q8, float* amax, float* slots,
                           int32_t* view_intact) {
  YS_REQUIRE(ctx && x && amax, "ys_f8_quant: null argument");
  YS_REQUIRE(kind >= 0 && kind <= 3, "ys_f8_quant: kind %d", kind);
  YS_REQUIRE(kind == 2 || q8, "ys_f8_quant: null argument");
  YS_REQUIRE(rows >= 1 && C >= 1 && coff >= 0 && pad >= 0, "ys_f8_quant: rows=%d C=%d coff=%d pad=%d", rows, C, coff, pad);
  const bool flat = kind == 3;
  const int vec = kind == 2 ? 8 : 16;          // elements per thread and trip of the view kernels
  YS_REQUIRE(flat ? (coff == 0 && pad == 0) : (C % vec == 0 && coff % 8 == 0 && pad % 8 == 0),
             "ys_f8_quant: kind %d: view (C %d, coff %d, pad %d) must sit on the %d-element grid (the weight form is dense)", kind, C, coff, pad, vec);
  YS_CHECK_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const size_t n = (size_t)rows * C;
  const int ld = coff + C + pad;
  // bf16 on the host (exact for values that are bf16 already), the rest of the buffer the sentinel
  std::vector<unsigned short> h((size_t)rows * ld, (unsigned short)(kSentinelByte * 0x0101));
  for (int r = 0; r < rows; r++)
    for (int c = 0; c < C; c++) h[(size_t)r * ld + coff + c] = f32_to_bf16_bits(x[(size_t)r * C + c]);
  DevBuf dx, dq, ds, dsc;
  YS_TRY(dx.alloc(h.size() * 2));
  YS_TRY(h2d(st, dx.p, h.data(), h.size() * 2));
  YS_TRY(alloc_filled(dq, n + kGuardFloats * 4, st));
  YS_TRY(alloc_slots(ds, st));
  YS_TRY(scalar_to_device(st, dsc, qscale));
  if (kind == 2) YS_TRY(ys_f8_view_amax_launch(st, dx.p, rows, C, ld, coff, (unsigned*)ds.p));
  else if (kind == 3) YS_TRY(ys_f8_quant_weights_launch(st, dx.p, (long)n, (const float*)dsc.p, dq.p));
  else YS_TRY(ys_f8_quant_view_launch(st, kind, dx.p, rows, C, ld, coff, (const float*)dsc.p, dq.p, (unsigned*)ds.p));
  if (q8 && kind != 2) YS_TRY(d2h(st, q8, dq.p, n));
  int ok = 1;
  YS_TRY(fetch_slots(st, ds, slots, amax, &ok));
  YS_TRY(check_guard_bytes(st, dq.p, n, &ok));
  if (kind == 2) YS_TRY(check_guard_bytes(st, dq.p, 0, &ok));          // the amax pass writes no image
  YS_TRY(check_sentinel(st, dx.p, rows, ld, coff, C, 2, &ok));
  YS_CHECK_HIP(hipStreamSynchronize(st));
  YS_CHECK_HIP(hipGetLastError());
  if (view_intact) *view_intact = ok;
  return YS_OK;
}

extern "C" int ys_f8_amax_ways(void) { return YS_AMAX_WAYS; }

extern "C" int ys_f8_scales(ys_ctx* ctx, const float* params, int64_t n_params, const int64_t* layer_off, const int64_t* layer_count, int n_layers,
                            const int32_t* conv_layer, int n_convs, float* amax_x, float* amax_dy, float* scales, float* amax_w) {
  YS_REQUIRE(ctx && params && layer_off && layer_count && conv_layer && amax_x && amax_dy && scales && amax_w, "ys_f8_scales: null argument");
  YS_REQUIRE(n_params >= 1 && n_layers >= 1 && n_convs >= 1, "ys_f8_scales: n_params=%lld n_layers=%d n_convs=%d", (long long)n_params, n_layers, n_convs);
  std::vector<F8Layer> hl((size_t)n_layers);
  std::vector<F8Conv> hc((size_t)n_convs);
  for (int l = 0; l < n_layers; l++) {
    YS_REQUIRE(layer_off[l] >= 0 && layer_count[l] >= 0 && layer_off[l] + layer_count[l] <= n_params, "ys_f8_scales: layer %d lies outside the parameter array", l);
    hl[l] = F8Layer{(long)layer_off[l], (long)layer_count[l]};
  }
  for (int c = 0; c < n_convs; c++) {
    YS_REQUIRE(conv_layer[c] >= 0 && conv_layer[c] < n_layers, "ys_f8_scales: convolution %d names layer %d", c, conv_layer[c]);
    hc[c] = F8Conv{conv_layer[c]};
  }
  YS_CHECK_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const size_t nslot = (size_t)n_convs * YS_AMAX_WAYS;
  DevBuf dp, dl, dc, daw, dax, dag, dsc;
  YS_TRY(dp.alloc((size_t)n_params * 4)); YS_TRY(dl.alloc(hl.size() * sizeof(F8Layer))); YS_TRY(dc.alloc(hc.size() * sizeof(F8Conv)));
  YS_TRY(alloc_filled(daw, ((size_t)n_layers + kGuardFloats) * 4, st));
  YS_TRY(alloc_filled(dax, (nslot + kGuardFloats) * 4, st)); YS_TRY(alloc_filled(dag, (nslot + kGuardFloats) * 4, st));
  YS_TRY(alloc_filled(dsc, ((size_t)n_convs * 4 + kGuardFloats) * 4, st));
  YS_TRY(h2d(st, dp.p, params, (size_t)n_params * 4));
  YS_TRY(h2d(st, dl.p, hl.data(), hl.size() * sizeof(F8Layer))); YS_TRY(h2d(st, dc.p, hc.data(), hc.size() * sizeof(F8Conv)));
  YS_TRY(h2d(st, dax.p, amax_x, nslot * 4)); YS_TRY(h2d(st, dag.p, amax_dy, nslot * 4));
  YS_TRY(h2d(st, dsc.p, scales, (size_t)n_convs * 16));
  YS_TRY(ys_f8_weight_amax_launch(st, (const float*)dp.p, (const F8Layer*)dl.p, n_layers, (float*)daw.p));
  YS_TRY(ys_f8_scales_launch(st, (const F8Conv*)dc.p, n_convs, (const float*)daw.p, (unsigned*)dax.p, (unsigned*)dag.p, (float*)dsc.p));
  YS_TRY(d2h(st, amax_w, daw.p, (size_t)n_layers * 4));
  YS_TRY(d2h(st, amax_x, dax.p, nslot * 4)); YS_TRY(d2h(st, amax_dy, dag.p, nslot * 4));
  YS_TRY(d2h(st, scales, dsc.p, (size_t)n_convs * 16));
  int ok = 1;
  YS_TRY(check_guard(st, daw.p, (size_t)n_layers, &ok)); YS_TRY(check_guard(st, dax.p, nslot, &ok)); YS_TRY(check_guard(st, dag.p, nslot, &ok));
  YS_TRY(check_guard(st, dsc.p, (size_t)n_convs * 4, &ok));
  YS_CHECK_HIP(hipStreamSynchronize(st));
  YS_CHECK_HIP(hipGetLastError());
  YS_REQUIRE(ok, "ys_f8_scales: a kernel wrote behind its arrays");
  return YS_OK;
}

extern "C" int ys_bn_apply_q8_fwd(ys_ctx* ctx, int act, const float* y, int rows, int C, const float* scale, const float* shift, const float* res, int res_pad,
                                  int res_coff, int z_pad, int z_coff, int res_shares_z, float qscale, float* z, uint8_t* q8, float* amax, int32_t* view_intact) {
  YS_REQUIRE(ctx && y && scale && shift && z && q8 && amax, "ys_bn_apply_q8_fwd: null argument");
  YS_REQUIRE(rows >= 1 && C >= 8 && C % 8 == 0, "ys_bn_apply_q8_fwd: rows=%d C=%d (C must be a multiple of 8)", rows, C);
  YS_TRY(view_ok("ys_bn_apply_q8_fwd z", YS_BF16, C, z_pad, z_coff));
  if (res) YS_TRY(view_ok("ys_bn_apply_q8_fwd res", YS_BF16, C, res_pad, res_coff));
  const bool shared = res && res_shares_z;
  YS_REQUIRE(!shared || res_coff + C <= z_coff || z_coff + C <= res_coff, "ys_bn_apply_q8_fwd: res and z views overlap");
  YS_CHECK_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const int dtype = YS_BF16;
  const size_t n = (size_t)rows * C;
  int ldz = z_coff + C + z_pad, ldr = 0;
  if (shared && res_coff + C + z_pad > ldz) ldz = res_coff + C + z_pad;
  DevBuf dy, dz, dres, dpar, dq, ds, dsc;
  YS_TRY(alloc_filled(dz, (size_t)rows * ldz * 2, st));
  const void* resp = nullptr;
  if (res) {
    ldr = shared ? ldz : res_coff + C + res_pad;
    if (!shared) YS_TRY(alloc_filled(dres, (size_t)rows * ldr * 2, st));
    resp = shared ? dz.p : dres.p;
    YS_TRY(stage_view(st, dtype, res, 1, C, rows, (void*)resp, ldr, res_coff));
  }
  YS_TRY(dy.alloc(n * 2));
  YS_TRY(stage_view(st, dtype, y, 1, C, rows, dy.p, C, 0));
  YS_TRY(dpar.alloc((size_t)2 * C * 4));
  YS_TRY(h2d(st, dpar.p, scale, (size_t)C * 4)); YS_TRY(h2d(st, (float*)dpar.p + C, shift, (size_t)C * 4));
  YS_TRY(alloc_filled(dq, n + kGuardFloats * 4, st));
  YS_TRY(alloc_slots(ds, st));
  YS_TRY(scalar_to_device(st, dsc, qscale));
  YS_TRY(ys_bn_act_apply_q8_launch(st, dy.p, rows, C, (const float*)dpar.p, (const float*)dpar.p + C, act, resp, ldr, res_coff, dz.p, ldz, z_coff, dq.p,
                                   (const float*)dsc.p, (unsigned*)ds.p));
  YS_TRY(fetch_view(st, dtype, dz.p, ldz, z_coff, 1, C, rows, z));
  YS_TRY(d2h(st, q8, dq.p, n));
  int ok = 1;
  YS_TRY(fetch_slots(st, ds, nullptr, amax, &ok));
  YS_TRY(check_guard_bytes(st, dq.p, n, &ok));
  const int views[2][2] = {{z_coff, C}, {res_coff, C}};
  YS_TRY(check_sentinel_views(st, dz.p, rows, ldz, views, shared ? 2 : 1, 2, &ok));
  if (dres.p) YS_TRY(check_sentinel(st, dres.p, rows, ldr, res_coff, C, 2, &ok));
  YS_CHECK_HIP(hipStreamSynchronize(st));
  YS_CHECK_HIP(hipGetLastError());
  if (view_intact) *view_intact = ok;
  return YS_OK;
}

extern "C" int ys_bn_apply_q8_bwd(ys_ctx* ctx, int act, const float* dz, const float* y, int rows, int C, const float* coef, int dz_pad, int dz_coff, float* rg,
                                  int rg_pad, int rg_coff, float qscale, float* dy, uint8_t* q8, float* amax, int32_t* view_intact) {
  YS_REQUIRE(ctx && dz && y && coef && dy && q8 && amax, "ys_bn_apply_q8_bwd: null argument");
  YS_REQUIRE(rows >= 1 && C >= 8 && C % 8 == 0, "ys_bn_apply_q8_bwd: rows=%d C=%d (C must be a multiple of 8)", rows, C);
  YS_TRY(view_ok("ys_bn_apply_q8_bwd dz", YS_BF16, C, dz_pad, dz_coff));
  if (rg) YS_TRY(view_ok("ys_bn_apply_q8_bwd rg", YS_BF16, C, rg_pad, rg_coff));
  YS_CHECK_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const int dtype = YS_BF16;
  const size_t n = (size_t)rows * C;
  const int ldd = dz_coff + C + dz_pad, ldg = rg ? rg_coff + C + rg_pad : 0;
  DevBuf ddz, dyb, drg, ddy, dpar, dq, ds, dsc;
  YS_TRY(alloc_filled(ddz, (size_t)rows * ldd * 2, st));
  YS_TRY(stage_view(st, dtype, dz, 1, C, rows, ddz.p, ldd, dz_coff));
  YS_TRY(dyb.alloc(n * 2));
  YS_TRY(stage_view(st, dtype, y, 1, C, rows, dyb.p, C, 0));
  if (rg) {
    YS_TRY(alloc_filled(drg, (size_t)rows * ldg * 2, st));
    YS_TRY(stage_view(st, dtype, rg, 1, C, rows, drg.p, ldg, rg_coff));
  }
  YS_TRY(alloc_filled(ddy, n * 2 + kGuardFloats * 4, st));
  YS_TRY(dpar.alloc((size_t)4 * C * 4));
  YS_TRY(h2d(st, dpar.p, coef, (size_t)4 * C * 4));
  const float* par = (const float*)dpar.p;
  YS_TRY(alloc_filled(dq, n + kGuardFloats * 4, st));
  YS_TRY(alloc_slots(ds, st));
  YS_TRY(scalar_to_device(st, dsc, qscale));
  YS_TRY(ys_bn_bwd_apply_q8_launch(st, ddz.p, ldd, dz_coff, dyb.p, rows, C, par, par + C, par + 2 * C, par + 3 * C, act, ddy.p, dq.p, (const float*)dsc.p,
                                   (unsigned*)ds.p, drg.p, ldg, rg_coff));
  YS_TRY(fetch_view(st, dtype, ddy.p, C, 0, 1, C, rows, dy));
  if (rg) YS_TRY(fetch_view(st, dtype, drg.p, ldg, rg_coff, 1, C, rows, rg));
  YS_TRY(d2h(st, q8, dq.p, n));
  int ok = 1;
  YS_TRY(fetch_slots(st, ds, nullptr, amax, &ok));
  YS_TRY(check_guard_bytes(st, dq.p, n, &ok));
  YS_TRY(check_guard_bytes(st, ddy.p, n * 2, &ok));
  YS_TRY(check_sentinel(st, ddz.p, rows, ldd, dz_coff, C, 2, &ok));
  if (rg) YS_TRY(check_sentinel(st, drg.p, rows, ldg, rg_coff, C, 2, &ok));
  YS_CHECK_HIP(hipStreamSynchronize(st));
  YS_CHECK_HIP(hipGetLastError());
  if (view_intact) *view_intact = ok;
  return YS_OK;
}

// ---- End2End post-process (e2e.hip): Detect.postprocess / get_topk_index (Modules/Head.cs:117-127, 175-196) on a [B, 4+nc, A] tensor and the
//      thresholding of Ops.non_max_suppression(end2end: true) (Utils/Ops.cs:258-267)
static int e2e_topk_impl(const char* fn, ys_ctx* ctx, const float* pred, int on_device, int batch, int nc, int extra, int anchors, int max_det, float* out_rows,
                         int64_t* out_anchor) {
  YS_REQUIRE(ctx && pred && out_rows && out_anchor, "%s: null argument", fn);
  YS_REQUIRE(batch > 0 && nc > 0 && extra >= 0 && anchors > 0 && max_det > 0, "%s: bad shape B=%d nc=%d extra=%d A=%d max_det=%d", fn, batch, nc, extra, anchors, max_det);
  YS_CHECK_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const size_t k = (size_t)(max_det < anchors ? max_det : anchors);
  const size_t n_pred = (size_t)batch * (4 + nc + extra) * anchors, n_rows = (size_t)batch * k * (6 + extra), n_anc = (size_t)batch * k;
  DevBuf dp, dr, da;
  const size_t need = ys_e2e_topk_ws_bytes(batch, nc, anchors, max_det);
  if (need > ctx->e2e_ws_bytes) {               // the context keeps the workspace (like the NMS one): device-resident calls stay asynchronous
    if (ctx->e2e_ws) { YS_CHECK_HIP(hipStreamSynchronize(st)); YS_CHECK_HIP(hipFree(ctx->e2e_ws)); ctx->e2e_ws = nullptr; ctx->e2e_ws_bytes = 0; }
    if (hipMalloc(&ctx->e2e_ws, need) != hipSuccess) { ys_set_error("%s: out of device memory (%zu bytes)", fn, need); return YS_ERR_OOM; }
    ctx->e2e_ws_bytes = need;
  }
  YsTimer timer(ctx, "e2e_topk");
  if (on_device) return ys_e2e_topk_launch(st, pred, batch, nc, anchors, max_det, ctx->e2e_ws, out_rows, (long long*)out_anchor, extra);
  YS_TRY(dp.alloc(n_pred * 4)); YS_TRY(dr.alloc(n_rows * 4)); YS_TRY(da.alloc(n_anc * 8));
  YS_CHECK_HIP(hipMemcpyAsync(dp.p, pred, n_pred * 4, hipMemcpyHostToDevice, st));
  YS_TRY(ys_e2e_topk_launch(st, (const float*)dp.p, batch, nc, anchors, max_det, ctx->e2e_ws, (float*)dr.p, (long long*)da.p, extra));
  YS_CHECK_HIP(hipMemcpyAsync(out_rows, dr.p, n_rows * 4, hipMemcpyDeviceToHost, st));
  YS_CHECK_HIP(hipMemcpyAsync(out_anchor, da.p, n_anc * 8, hipMemcpyDeviceToHost, st));
  YS_CHECK_HIP(hipStreamSynchronize(st));
  return YS_OK;
}

extern "C" int ys_e2e_topk(ys_ctx* ctx, const float* pred, int on_device, int batch, int nc, int anchors, int max_det, float* out_rows,
                           int64_t* out_anchor) {
  return e2e_topk_impl("ys_e2e_topk", ctx, pred, on_device, batch, nc, 0, anchors, max_det, out_rows, out_anchor);
}

extern "C" int ys_e2e_topk_ex(ys_ctx* ctx, const float* pred, int on_device, int batch, int nc, int extra, int anchors, int max_det, float* out_rows,
                              int64_t* out_anchor) {
  return e2e_topk_impl("ys_e2e_topk_ex", ctx, pred, on_device, batch, nc, extra, anchors, max_det, out_rows, out_anchor);
}

static int e2e_select_impl(const char* fn, ys_ctx* ctx, const float* rows, int on_device, int batch, int k, int row_len, float conf_thres, int max_det, int32_t* out_count) {
  YS_REQUIRE(ctx && rows && out_count, "%s: null argument", fn);
  // Ops.cs:248-251: ArgumentException for a threshold outside [0,1]
  YS_REQUIRE(conf_thres >= 0.f && conf_thres <= 1.f, "Invalid Confidence threshold %g, valid values are between 0.0 and 1.0", conf_thres);
  YS_REQUIRE(batch > 0 && k > 0 && max_det > 0 && row_len >= 6, "%s: bad shape B=%d k=%d max_det=%d row length %d", fn, batch, k, max_det, row_len);
  YS_CHECK_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  if (on_device) return ys_e2e_select_launch(st, rows, batch, k, conf_thres, max_det, out_count, row_len);
  DevBuf dr, dc;
  const size_t nb = (size_t)batch * k * row_len * 4;
  YS_TRY(dr.alloc(nb)); YS_TRY(dc.alloc((size_t)batch * 4));
  YS_CHECK_HIP(hipMemcpyAsync(dr.p, rows, nb, hipMemcpyHostToDevice, st));
  YS_TRY(ys_e2e_select_launch(st, (const float*)dr.p, batch, k, conf_thres, max_det, (int*)dc.p, row_len));
  YS_CHECK_HIP(hipMemcpyAsync(out_count, dc.p, (size_t)batch * 4, hipMemcpyDeviceToHost, st));
  YS_CHECK_HIP(hipStreamSynchronize(st));
  return YS_OK;
}

extern "C" int ys_e2e_select(ys_ctx* ctx, const float* rows, int on_device, int batch, int k, float conf_thres, int max_det, int32_t* out_count) {
  return e2e_select_impl("ys_e2e_select", ctx, rows, on_device, batch, k, 6, conf_thres, max_det, out_count);
}

extern "C" int ys_e2e_select_ex(ys_ctx* ctx, const float* rows, int on_device, int batch, int k, int row_len, float conf_thres, int max_det, int32_t* out_count) {
  return e2e_select_impl("ys_e2e_select_ex", ctx, rows, on_device, batch, k, row_len, conf_thres, max_det, out_count);
}

// ---- the assigner's second stage on its own (loss.hip tal_keep_best_kernel, the kernel the End2End Segment criterion runs; Utils/Tal.cs:242-250)
extern "C" int ys_tal_keep_best(ys_ctx* ctx, const float* align, uint8_t* mask_pos, const int32_t* gt_count, int on_device, int batch, int boxes, int anchors) {
  YS_REQUIRE(ctx && align && mask_pos && gt_count, "ys_tal_keep_best: null argument");
  YS_REQUIRE(batch > 0 && boxes > 0 && anchors > 0, "ys_tal_keep_best: bad shape B=%d G=%d A=%d", batch, boxes, anchors);
  YS_CHECK_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const size_t n = (size_t)batch * boxes * anchors;
  TalKeepArgs k{};
  k.B = batch; k.G = boxes; k.A = anchors;
  if (on_device) {      // the caller vouches for 0 <= gt_count[b] <= boxes
    k.align = align; k.mpos = mask_pos; k.gt_count = gt_count;
    return ys_tal_keep_best_launch(st, k);
  }
  for (int b = 0; b < batch; b++) YS_REQUIRE(gt_count[b] >= 0 && gt_count[b] <= boxes, "ys_tal_keep_best: gt_count[%d] = %d outside [0, %d]", b, gt_count[b], boxes);
  DevBuf da, dm, dc;
  YS_TRY(da.alloc(n * 4)); YS_TRY(dm.alloc(n)); YS_TRY(dc.alloc((size_t)batch * 4));
  YS_CHECK_HIP(hipMemcpyAsync(da.p, align, n * 4, hipMemcpyHostToDevice, st));
  YS_CHECK_HIP(hipMemcpyAsync(dm.p, mask_pos, n, hipMemcpyHostToDevice, st));
  YS_CHECK_HIP(hipMemcpyAsync(dc.p, gt_count, (size_t)batch * 4, hipMemcpyHostToDevice, st));
  k.align = (const float*)da.p; k.mpos = (unsigned char*)dm.p; k.gt_count = (const int*)dc.p;
  YS_TRY(ys_tal_keep_best_launch(st, k));
  YS_CHECK_HIP(hipMemcpyAsync(mask_pos, dm.p, n, hipMemcpyDeviceToHost, st));
  YS_CHECK_HIP(hipStreamSynchronize(st));
  return YS_OK;
}

// ---- training input on the device (augment.hip): Mosaic4 + RandomPerspective + flips + Normalize + collate (Data/Augment.cs:158-274, 315-695, 860-966;
//      Data/YoloDataset.cs:102-151; Data/YoloDataLoader.cs:18-44)
namespace {
int aug_reserve_ws(ys_ctx* ctx, int batch) {
  const size_t need = ys_aug_ws_bytes(batch);
  if (need <= ctx->aug_ws_bytes) return YS_OK;
  if (ctx->aug_ws) { YS_CHECK_HIP(hipStreamSynchronize(ctx->stream)); YS_CHECK_HIP(hipFree(ctx->aug_ws)); ctx->aug_ws = nullptr; ctx->aug_ws_bytes = 0; }
  if (hipMalloc(&ctx->aug_ws, need) != hipSuccess) { ys_set_error("ys_augment: out of device memory (%zu bytes)", need); return YS_ERR_OOM; }
  ctx->aug_ws_bytes = need;
  return YS_OK;
}
// the part of the arena the sources name (what a host-pointer call uploads)
size_t aug_arena_bytes(const ys_aug_src* srcs, int n_src) {
  size_t bytes = 0;
  for (int k = 0; k < n_src; k++) {
    const ys_aug_src& sr = srcs[k];
    if (sr.img_off >= 0 && sr.h > 0 && sr.w > 0) { const size_t e = (size_t)sr.img_off + (size_t)3 * sr.h * sr.w; bytes = e > bytes ? e : bytes; }
    if (sr.mask_off >= 0 && sr.mh > 0 && sr.mw > 0) { const size_t e = (size_t)sr.mask_off + (size_t)sr.mh * sr.mw; bytes = e > bytes ? e : bytes; }
  }
  return bytes;
}
// the checks a host-resident item table allows (include/yolosharp_hip.h); n_src < 0: unknown, only src >= 0 is checked
int aug_check_items(const char* fn, const ys_aug_item* items, int batch, const ys_aug_src* srcs, int n_src, int s, int perspective) {
  for (int b = 0; b < batch; b++) {
    const ys_aug_item& it = items[b];
    for (int i = 0; i < 4; i++)
      if (n_src < 0) YS_REQUIRE(it.src[i] >= 0, "%s: item %d: src[%d] = %d is negative", fn, b, i, it.src[i]);
      else YS_REQUIRE(it.src[i] >= 0 && it.src[i] < n_src, "%s: item %d: src[%d] = %d is outside [0, %d)", fn, b, i, it.src[i], n_src);
    YS_REQUIRE(it.xc >= 0 && it.xc <= 2 * s && it.yc >= 0 && it.yc <= 2 * s, "%s: item %d: centre (%d, %d) is outside [0, %d]", fn, b, it.xc, it.yc, 2 * s);
    int mx = 0;
    for (int i = 0; i < 4; i++) mx = it.src[i] > mx ? it.src[i] : mx;
    for (int i = 0; i < 4; i++)
      YS_REQUIRE(srcs[it.src[i]].h > 0 && srcs[it.src[i]].w > 0 && srcs[it.src[i]].img_off >= 0, "%s: source %d has no image", fn, it.src[i]);
    YS_REQUIRE(ys_aug_item_ok_host(&it, srcs, mx + 1, s, perspective), "%s: item %d: M is singular", fn, b);
  }
  return YS_OK;
}
}  // namespace

namespace {
// the checks a host-resident jitter table allows: every row valid (YS_ERR_INVALID_ARG); allow_contrast = 0: no row runs contrast (YS_ERR_UNSUPPORTED).
// *any_contrast (may be NULL) = some row runs it
int aug_check_jitter(const char* fn, const ys_aug_jitter* rows, int batch, int allow_contrast, int* any_contrast) {
  int any = 0;
  for (int b = 0; b < batch; b++) {
    const ys_aug_jitter& J = rows[b];
    const int state = ys_aug_jitter_state_host(&J);
    YS_REQUIRE(state != 0, "%s: jitter row %d is invalid: order (%d, %d, %d, %d) must hold ids in {-1, 0..3} with none twice, factors (%g, %g, %g) must be "
               "finite and >= 0, hue %g in [-0.5, 0.5]", fn, b, J.order[0], J.order[1], J.order[2], J.order[3], (double)J.factor[0], (double)J.factor[1],
               (double)J.factor[2], (double)J.factor[3]);
    if (state == 2 && !allow_contrast) {
      ys_set_error("%s: jitter row %d runs contrast: the fused entries have no image mean (ys_color_jitter does)", fn, b);
      return YS_ERR_UNSUPPORTED;
    }
    any |= state == 2;
  }
  if (any_contrast) *any_contrast = any;
  return YS_OK;
}

int aug_mosaic_impl(const char* fn, ys_ctx* ctx, const uint8_t* arena, const ys_aug_src* srcs, int n_src, const ys_aug_item* items, int batch, int on_device,
                    int imgsz, int mask_ratio, int perspective, const ys_aug_jitter* jitter, float* images, float* masks) {
  YS_REQUIRE(ctx && arena && srcs && items && images, "%s: null argument", fn);
  YS_REQUIRE(batch > 0 && batch <= 65535 && n_src > 0, "%s: bad shape batch=%d (1..65535) n_src=%d", fn, batch, n_src);
  YS_REQUIRE(imgsz >= 2 && imgsz % 2 == 0 && imgsz <= 16384, "%s: imgsz %d must be even and in [2, 16384]", fn, imgsz);
  if (masks) YS_REQUIRE(mask_ratio >= 1 && imgsz % mask_ratio == 0 && 2 * imgsz / mask_ratio >= 2, "%s: mask_ratio %d does not divide imgsz %d", fn, mask_ratio, imgsz);
  const int r = masks ? mask_ratio : 1;
  YS_CHECK_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  YS_TRY(aug_reserve_ws(ctx, batch));
  YsTimer timer(ctx, "augment");
  if (on_device) return ys_aug_mosaic_launch(st, arena, srcs, n_src, items, batch, imgsz, r, perspective != 0, jitter, ctx->aug_ws, images, masks);
  YS_TRY(aug_check_items(fn, items, batch, srcs, n_src, imgsz, perspective != 0));
  if (jitter) YS_TRY(aug_check_jitter(fn, jitter, batch, 0, nullptr));
  const size_t arena_bytes = aug_arena_bytes(srcs, n_src);
  const size_t n_img = (size_t)batch * 3 * imgsz * imgsz, n_msk = masks ? (size_t)batch * (imgsz / r) * (imgsz / r) : 0;
  DevBuf da, ds, di, dj, dimg, dm;
  YS_TRY(da.alloc(arena_bytes)); YS_TRY(ds.alloc((size_t)n_src * sizeof(ys_aug_src))); YS_TRY(di.alloc((size_t)batch * sizeof(ys_aug_item)));
  YS_TRY(dimg.alloc(n_img * 4)); YS_TRY(dm.alloc(n_msk * 4));
  YS_CHECK_HIP(hipMemcpyAsync(da.p, arena, arena_bytes, hipMemcpyHostToDevice, st));
  YS_CHECK_HIP(hipMemcpyAsync(ds.p, srcs, (size_t)n_src * sizeof(ys_aug_src), hipMemcpyHostToDevice, st));
  YS_CHECK_HIP(hipMemcpyAsync(di.p, items, (size_t)batch * sizeof(ys_aug_item), hipMemcpyHostToDevice, st));
  if (jitter) {
    YS_TRY(dj.alloc((size_t)batch * sizeof(ys_aug_jitter)));
    YS_CHECK_HIP(hipMemcpyAsync(dj.p, jitter, (size_t)batch * sizeof(ys_aug_jitter), hipMemcpyHostToDevice, st));
  }
  YS_TRY(ys_aug_mosaic_launch(st, (const unsigned char*)da.p, (const ys_aug_src*)ds.p, n_src, (const ys_aug_item*)di.p, batch, imgsz, r, perspective != 0,
                              jitter ? (const ys_aug_jitter*)dj.p : nullptr, ctx->aug_ws, (float*)dimg.p, masks ? (float*)dm.p : nullptr));
  YS_CHECK_HIP(hipMemcpyAsync(images, dimg.p, n_img * 4, hipMemcpyDeviceToHost, st));
  if (masks) YS_CHECK_HIP(hipMemcpyAsync(masks, dm.p, n_msk * 4, hipMemcpyDeviceToHost, st));
  YS_CHECK_HIP(hipStreamSynchronize(st));
  return YS_OK;
}
}  // namespace

extern "C" int ys_augment_mosaic(ys_ctx* ctx, const uint8_t* arena, const ys_aug_src* srcs, int n_src, const ys_aug_item* items, int batch,
                                 int on_device, int imgsz, int mask_ratio, int perspective, float* images, float* masks) {
  return aug_mosaic_impl("ys_augment_mosaic", ctx, arena, srcs, n_src, items, batch, on_device, imgsz, mask_ratio, perspective, nullptr, images, masks);
}

// the same with the ColorJitter (RandomHSV, Data/Augment.cs:968-987) rows of the batch in the warp kernel's epilogue; jitter == NULL is the entry above
extern "C" int ys_augment_mosaic_jitter(ys_ctx* ctx, const uint8_t* arena, const ys_aug_src* srcs, int n_src, const ys_aug_item* items, int batch,
                                        int on_device, int imgsz, int mask_ratio, int perspective, const ys_aug_jitter* jitter, float* images,
                                        float* masks) {
  return aug_mosaic_impl("ys_augment_mosaic_jitter", ctx, arena, srcs, n_src, items, batch, on_device, imgsz, mask_ratio, perspective, jitter, images, masks);
}

namespace {
// ys_augment_labels (corners == NULL) and ys_augment_labels_obb (corners [n, 4, 2] in place of the keypoints, out_bboxes [capacity, 5], flags 0)
int aug_labels_impl(const char* fn, ys_ctx* ctx, const ys_aug_src* srcs, const int32_t* lab_off, const float* cls, const float* boxes, const float* keypoints,
                    int kpt_num, int kpt_dim, const float* corners, int obb, const ys_aug_item* items, int batch, int on_device, int imgsz, int perspective,
                    int flags, int capacity, float* out_batch_idx, float* out_cls, float* out_bboxes, float* out_keypoints, int32_t* out_count) {
  YS_REQUIRE(ctx && srcs && lab_off && cls && boxes && items && out_batch_idx && out_cls && out_bboxes && out_count && (!obb || corners), "%s: null argument", fn);
  YS_REQUIRE(batch > 0 && batch <= 65535 && capacity > 0, "%s: bad shape batch=%d (1..65535) capacity=%d", fn, batch, capacity);
  YS_REQUIRE(imgsz >= 2 && imgsz % 2 == 0 && imgsz <= 16384, "%s: imgsz %d must be even and in [2, 16384]", fn, imgsz);
  YS_REQUIRE((keypoints != nullptr) == (out_keypoints != nullptr), "%s: keypoints and out_keypoints go together", fn);
  if (keypoints) {
    YS_REQUIRE(kpt_dim == 3, "%s: kpt_dim %d: only (x, y, visibility) keypoints are supported (apply_keypoints reads column 2)", fn, kpt_dim);
    YS_REQUIRE(kpt_num > 0, "%s: kpt_num %d", fn, kpt_num);
  }
  if (obb) YS_REQUIRE(flags == 0, "%s: flags 0x%x: the box-flip switches have nothing to act on, flags must be 0", fn, flags);
  else YS_REQUIRE((flags & ~YS_AUG_SORT_FLIPPED) == 0, "%s: unknown flags 0x%x", fn, flags);
  // the per-label table beside the boxes: K keypoints of 3 floats, or 4 corners of 2; the width of an output box row
  const int K = keypoints ? kpt_num : 0;
  const size_t xf = obb ? 8 : (size_t)K * 3, bw = obb ? 5 : 4;
  const float* extra = obb ? corners : keypoints;
  YS_CHECK_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  YS_TRY(aug_reserve_ws(ctx, batch));
  YsTimer timer(ctx, "augment_labels");
  if (on_device)    // the source count is not part of the signature: lab_off has one entry per source and one more, device items are the caller's responsibility
    return ys_aug_labels_launch(st, srcs, 0x7fffffff, lab_off, cls, boxes, extra, K, items, batch, imgsz, perspective != 0, flags, capacity, ctx->aug_ws,
                                out_batch_idx, out_cls, out_bboxes, out_keypoints, out_count, obb);
  YS_TRY(aug_check_items(fn, items, batch, srcs, -1, imgsz, perspective != 0));
  int n_src = 0;
  for (int b = 0; b < batch; b++) for (int i = 0; i < 4; i++) n_src = items[b].src[i] + 1 > n_src ? items[b].src[i] + 1 : n_src;
  size_t n_lab = 0;
  for (int b = 0; b < batch; b++) {
    long sum = 0;
    for (int i = 0; i < 4; i++) {
      const int k = items[b].src[i];
      YS_REQUIRE(lab_off[k] >= 0 && lab_off[k + 1] >= lab_off[k], "%s: lab_off is not non-decreasing at source %d", fn, k);
      sum += lab_off[k + 1] - lab_off[k];
      n_lab = (size_t)lab_off[k + 1] > n_lab ? (size_t)lab_off[k + 1] : n_lab;
    }
    YS_REQUIRE(sum <= capacity, "%s: item %d carries %ld labels over its four tiles, capacity is %d", fn, b, sum, capacity);
  }
  const size_t cap = (size_t)capacity;
  DevBuf ds, dl, dc, db, dk, di, obi, ocl, obx, okp, ocn;
  YS_TRY(ds.alloc((size_t)n_src * sizeof(ys_aug_src))); YS_TRY(dl.alloc((size_t)(n_src + 1) * 4)); YS_TRY(dc.alloc(n_lab * 4)); YS_TRY(db.alloc(n_lab * 16));
  YS_TRY(dk.alloc(n_lab * xf * 4)); YS_TRY(di.alloc((size_t)batch * sizeof(ys_aug_item)));
  YS_TRY(obi.alloc(cap * 4)); YS_TRY(ocl.alloc(cap * 4)); YS_TRY(obx.alloc(cap * bw * 4)); YS_TRY(okp.alloc(cap * K * 12)); YS_TRY(ocn.alloc(4));
  YS_CHECK_HIP(hipMemcpyAsync(ds.p, srcs, (size_t)n_src * sizeof(ys_aug_src), hipMemcpyHostToDevice, st));
  YS_CHECK_HIP(hipMemcpyAsync(dl.p, lab_off, (size_t)(n_src + 1) * 4, hipMemcpyHostToDevice, st));
  if (n_lab) {
    YS_CHECK_HIP(hipMemcpyAsync(dc.p, cls, n_lab * 4, hipMemcpyHostToDevice, st));
    YS_CHECK_HIP(hipMemcpyAsync(db.p, boxes, n_lab * 16, hipMemcpyHostToDevice, st));
    if (xf) YS_CHECK_HIP(hipMemcpyAsync(dk.p, extra, n_lab * xf * 4, hipMemcpyHostToDevice, st));
  }
  YS_CHECK_HIP(hipMemcpyAsync(di.p, items, (size_t)batch * sizeof(ys_aug_item), hipMemcpyHostToDevice, st));
  YS_TRY(ys_aug_labels_launch(st, (const ys_aug_src*)ds.p, n_src, (const int*)dl.p, (const float*)dc.p, (const float*)db.p, xf ? (const float*)dk.p : nullptr, K,
                              (const ys_aug_item*)di.p, batch, imgsz, perspective != 0, flags, capacity, ctx->aug_ws, (float*)obi.p, (float*)ocl.p, (float*)obx.p,
                              K ? (float*)okp.p : nullptr, (int*)ocn.p, obb));
  YS_CHECK_HIP(hipMemcpyAsync(out_batch_idx, obi.p, cap * 4, hipMemcpyDeviceToHost, st));
  YS_CHECK_HIP(hipMemcpyAsync(out_cls, ocl.p, cap * 4, hipMemcpyDeviceToHost, st));
  YS_CHECK_HIP(hipMemcpyAsync(out_bboxes, obx.p, cap * bw * 4, hipMemcpyDeviceToHost, st));
  if (K) YS_CHECK_HIP(hipMemcpyAsync(out_keypoints, okp.p, cap * K * 12, hipMemcpyDeviceToHost, st));
  YS_CHECK_HIP(hipMemcpyAsync(out_count, ocn.p, 4, hipMemcpyDeviceToHost, st));
  YS_CHECK_HIP(hipStreamSynchronize(st));
  return YS_OK;
}
}  // namespace

extern "C" int ys_augment_labels(ys_ctx* ctx, const ys_aug_src* srcs, const int32_t* lab_off, const float* cls, const float* boxes,
                                 const float* keypoints, int kpt_num, int kpt_dim, const ys_aug_item* items, int batch, int on_device,
                                 int imgsz, int perspective, int flags, int capacity, float* out_batch_idx, float* out_cls, float* out_bboxes,
                                 float* out_keypoints, int32_t* out_count) {
  return aug_labels_impl("ys_augment_labels", ctx, srcs, lab_off, cls, boxes, keypoints, kpt_num, kpt_dim, nullptr, 0, items, batch, on_device, imgsz, perspective,
                         flags, capacity, out_batch_idx, out_cls, out_bboxes, out_keypoints, out_count);
}

// OBB corner labels (Data/YoloDataset.cs:110-129, 216-244): the corners through the chain, the minimum-area rectangle, rows of 5
extern "C" int ys_augment_labels_obb(ys_ctx* ctx, const ys_aug_src* srcs, const int32_t* lab_off, const float* cls, const float* boxes,
                                     const float* corners, const ys_aug_item* items, int batch, int on_device, int imgsz, int perspective, int flags,
                                     int capacity, float* out_batch_idx, float* out_cls, float* out_bboxes, int32_t* out_count) {
  return aug_labels_impl("ys_augment_labels_obb", ctx, srcs, lab_off, cls, boxes, nullptr, 0, 3, corners, 1, items, batch, on_device, imgsz, perspective, flags,
                         capacity, out_batch_idx, out_cls, out_bboxes, nullptr, out_count);
}

// the rectangle on its own: corners [n, 4, 2] -> out [n, 5] = cx, cy, w, h in the corners' units, angle in radians; n == 0 does nothing
extern "C" int ys_xyxyxyxy2xywhr(ys_ctx* ctx, const float* corners, int n, int on_device, float* out) {
  YS_REQUIRE(ctx && n >= 0 && (n == 0 || (corners && out)), "ys_xyxyxyxy2xywhr: null argument or n = %d < 0", n);
  if (n == 0) return YS_OK;
  YS_CHECK_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  YsTimer timer(ctx, "xyxyxyxy2xywhr");
  if (on_device) return ys_xyxyxyxy2xywhr_launch(st, corners, n, out);
  DevBuf dc, dout;
  YS_TRY(dc.alloc((size_t)n * 32)); YS_TRY(dout.alloc((size_t)n * 20));
  YS_CHECK_HIP(hipMemcpyAsync(dc.p, corners, (size_t)n * 32, hipMemcpyHostToDevice, st));
  YS_TRY(ys_xyxyxyxy2xywhr_launch(st, (const float*)dc.p, n, (float*)dout.p));
  YS_CHECK_HIP(hipMemcpyAsync(out, dout.p, (size_t)n * 20, hipMemcpyDeviceToHost, st));
  YS_CHECK_HIP(hipStreamSynchronize(st));
  return YS_OK;
}

// ---- the LetterBox (close-mosaic) branch of the training input (Data/YoloDataset.cs:378-429; Data/Augment.cs:698-778, 860-966)
namespace {
int aug_check_letterbox_items(const char* fn, const ys_aug_item* items, int batch, const ys_aug_src* srcs, int n_src) {
  for (int b = 0; b < batch; b++) {
    const int k = items[b].src[0];
    YS_REQUIRE(k >= 0 && k < n_src, "%s: item %d: src[0] = %d is outside [0, %d)", fn, b, k, n_src);
    YS_REQUIRE(ys_aug_letterbox_src_host(&items[b], srcs, n_src) == k, "%s: source %d has no image", fn, k);
  }
  return YS_OK;
}

int aug_letterbox_impl(const char* fn, ys_ctx* ctx, const uint8_t* arena, const ys_aug_src* srcs, int n_src, const ys_aug_item* items, int batch,
                       int on_device, int imgsz, int mask_ratio, const ys_aug_jitter* jitter, float* images, float* masks) {
  YS_REQUIRE(ctx && arena && srcs && items && images, "%s: null argument", fn);
  YS_REQUIRE(batch > 0 && batch <= 65535 && n_src > 0, "%s: bad shape batch=%d (1..65535) n_src=%d", fn, batch, n_src);
  YS_REQUIRE(imgsz >= 2 && imgsz % 2 == 0 && imgsz <= 16384, "%s: imgsz %d must be even and in [2, 16384]", fn, imgsz);
  if (masks) YS_REQUIRE(mask_ratio >= 1 && imgsz % mask_ratio == 0, "%s: mask_ratio %d does not divide imgsz %d", fn, mask_ratio, imgsz);
  const int r = masks ? mask_ratio : 1;
  YS_CHECK_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  YsTimer timer(ctx, "augment_letterbox");
  if (on_device) return ys_aug_letterbox_launch(st, arena, srcs, n_src, items, batch, imgsz, r, jitter, images, masks);
  YS_TRY(aug_check_letterbox_items(fn, items, batch, srcs, n_src));
  if (jitter) YS_TRY(aug_check_jitter(fn, jitter, batch, 0, nullptr));
  const size_t arena_bytes = aug_arena_bytes(srcs, n_src);
  const size_t n_img = (size_t)batch * 3 * imgsz * imgsz, n_msk = masks ? (size_t)batch * (imgsz / r) * (imgsz / r) : 0;
  DevBuf da, ds, di, dj, dimg, dm;
  YS_TRY(da.alloc(arena_bytes)); YS_TRY(ds.alloc((size_t)n_src * sizeof(ys_aug_src))); YS_TRY(di.alloc((size_t)batch * sizeof(ys_aug_item)));
  YS_TRY(dimg.alloc(n_img * 4)); YS_TRY(dm.alloc(n_msk * 4));
  YS_CHECK_HIP(hipMemcpyAsync(da.p, arena, arena_bytes, hipMemcpyHostToDevice, st));
  YS_CHECK_HIP(hipMemcpyAsync(ds.p, srcs, (size_t)n_src * sizeof(ys_aug_src), hipMemcpyHostToDevice, st));
  YS_CHECK_HIP(hipMemcpyAsync(di.p, items, (size_t)batch * sizeof(ys_aug_item), hipMemcpyHostToDevice, st));
  if (jitter) {
    YS_TRY(dj.alloc((size_t)batch * sizeof(ys_aug_jitter)));
    YS_CHECK_HIP(hipMemcpyAsync(dj.p, jitter, (size_t)batch * sizeof(ys_aug_jitter), hipMemcpyHostToDevice, st));
  }
  YS_TRY(ys_aug_letterbox_launch(st, (const unsigned char*)da.p, (const ys_aug_src*)ds.p, n_src, (const ys_aug_item*)di.p, batch, imgsz, r,
                                 jitter ? (const ys_aug_jitter*)dj.p : nullptr, (float*)dimg.p, masks ? (float*)dm.p : nullptr));
  YS_CHECK_HIP(hipMemcpyAsync(images, dimg.p, n_img * 4, hipMemcpyDeviceToHost, st));
  if (masks) YS_CHECK_HIP(hipMemcpyAsync(masks, dm.p, n_msk * 4, hipMemcpyDeviceToHost, st));
  YS_CHECK_HIP(hipStreamSynchronize(st));
  return YS_OK;
}
}  // namespace

extern "C" int ys_augment_letterbox(ys_ctx* ctx, const uint8_t* arena, const ys_aug_src* srcs, int n_src, const ys_aug_item* items, int batch,
                                    int on_device, int imgsz, int mask_ratio, float* images, float* masks) {
  return aug_letterbox_impl("ys_augment_letterbox", ctx, arena, srcs, n_src, items, batch, on_device, imgsz, mask_ratio, nullptr, images, masks);
}

// the same with the batch's ColorJitter rows in the image kernel's epilogue; jitter == NULL is the entry above
extern "C" int ys_augment_letterbox_jitter(ys_ctx* ctx, const uint8_t* arena, const ys_aug_src* srcs, int n_src, const ys_aug_item* items, int batch,
                                           int on_device, int imgsz, int mask_ratio, const ys_aug_jitter* jitter, float* images, float* masks) {
  return aug_letterbox_impl("ys_augment_letterbox_jitter", ctx, arena, srcs, n_src, items, batch, on_device, imgsz, mask_ratio, jitter, images, masks);
}

// ---- ColorJitter on its own (augment.hip; Data/Augment.cs:968-987, Data/ClassificationDataset.cs:122): all four ops, uint8 or fp32 * (1 / 255.0f) out
extern "C" int ys_color_jitter(ys_ctx* ctx, const uint8_t* src, const ys_aug_jitter* jitter, int batch, int h, int w, int on_device, void* dst,
                               int dst_is_float) {
  YS_REQUIRE(ctx && src && jitter && dst, "ys_color_jitter: null argument");
  YS_REQUIRE(batch > 0 && batch <= 65535 && h > 0 && w > 0 && h <= 16384 && w <= 16384, "ys_color_jitter: bad shape batch=%d (1..65535) h=%d w=%d (1..16384)",
             batch, h, w);
  YS_CHECK_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  YS_TRY(aug_reserve_ws(ctx, batch));                      // the per-image gray sums live in the augmenter's workspace (8 bytes per image)
  YsTimer timer(ctx, "color_jitter");
  const long long n = (long long)h * w;
  if (on_device) {                                         // the host cannot read the rows: the reduction runs and leaves at once where a row has no contrast
    YS_CHECK_HIP(hipMemsetAsync(ctx->aug_ws, 0, (size_t)batch * 8, st));
    return ys_color_jitter_launch(st, src, jitter, batch, n, 1, ctx->aug_ws, dst, dst_is_float != 0);
  }
  int contrast = 0;
  YS_TRY(aug_check_jitter("ys_color_jitter", jitter, batch, 1, &contrast));
  const size_t n_px = (size_t)batch * 3 * (size_t)n, out_bytes = n_px * (dst_is_float ? 4 : 1);
  DevBuf dsrc, dj, dout;
  YS_TRY(dsrc.alloc(n_px)); YS_TRY(dj.alloc((size_t)batch * sizeof(ys_aug_jitter))); YS_TRY(dout.alloc(out_bytes));
  YS_CHECK_HIP(hipMemcpyAsync(dsrc.p, src, n_px, hipMemcpyHostToDevice, st));
  YS_CHECK_HIP(hipMemcpyAsync(dj.p, jitter, (size_t)batch * sizeof(ys_aug_jitter), hipMemcpyHostToDevice, st));
  if (contrast) YS_CHECK_HIP(hipMemsetAsync(ctx->aug_ws, 0, (size_t)batch * 8, st));
  YS_TRY(ys_color_jitter_launch(st, (const unsigned char*)dsrc.p, (const ys_aug_jitter*)dj.p, batch, n, contrast, ctx->aug_ws, dout.p, dst_is_float != 0));
  YS_CHECK_HIP(hipMemcpyAsync(dst, dout.p, out_bytes, hipMemcpyDeviceToHost, st));
  YS_CHECK_HIP(hipStreamSynchronize(st));
  return YS_OK;
}

namespace {
// ys_augment_letterbox_labels (corners == NULL) and ys_augment_letterbox_labels_obb, like aug_labels_impl
int aug_letterbox_labels_impl(const char* fn, ys_ctx* ctx, const ys_aug_src* srcs, int n_src, const int32_t* lab_off, const float* cls, const float* boxes,
                              const float* keypoints, int kpt_num, int kpt_dim, const float* corners, int obb, const ys_aug_item* items, int batch,
                              int on_device, int imgsz, int flags, int capacity, float* out_batch_idx, float* out_cls, float* out_bboxes, float* out_keypoints,
                              int32_t* out_count) {
  YS_REQUIRE(ctx && srcs && lab_off && cls && boxes && items && out_batch_idx && out_cls && out_bboxes && out_count && (!obb || corners), "%s: null argument", fn);
  YS_REQUIRE(batch > 0 && batch <= 65535 && capacity > 0 && n_src > 0, "%s: bad shape batch=%d (1..65535) capacity=%d n_src=%d", fn, batch, capacity, n_src);
  YS_REQUIRE(imgsz >= 2 && imgsz % 2 == 0 && imgsz <= 16384, "%s: imgsz %d must be even and in [2, 16384]", fn, imgsz);
  YS_REQUIRE((keypoints != nullptr) == (out_keypoints != nullptr), "%s: keypoints and out_keypoints go together", fn);
  if (keypoints) {
    YS_REQUIRE(kpt_dim == 3, "%s: kpt_dim %d: only (x, y, visibility) keypoints are supported", fn, kpt_dim);
    YS_REQUIRE(kpt_num > 0, "%s: kpt_num %d", fn, kpt_num);
  }
  if (obb) YS_REQUIRE(flags == 0, "%s: flags 0x%x: the box-flip switches have nothing to act on, flags must be 0", fn, flags);
  else YS_REQUIRE((flags & ~(YS_AUG_SORT_FLIPPED | YS_AUG_FLIP_KEEP_SIZE)) == 0, "%s: unknown flags 0x%x", fn, flags);
  const int K = keypoints ? kpt_num : 0;
  const size_t xf = obb ? 8 : (size_t)K * 3, bw = obb ? 5 : 4;
  const float* extra = obb ? corners : keypoints;
  YS_CHECK_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  YS_TRY(aug_reserve_ws(ctx, batch));
  YsTimer timer(ctx, "augment_letterbox_labels");
  if (on_device)
    return ys_aug_letterbox_labels_launch(st, srcs, n_src, lab_off, cls, boxes, extra, K, items, batch, imgsz, flags, capacity, ctx->aug_ws, out_batch_idx,
                                          out_cls, out_bboxes, out_keypoints, out_count, obb);
  YS_TRY(aug_check_letterbox_items(fn, items, batch, srcs, n_src));
  for (int k = 0; k < n_src; k++)
    YS_REQUIRE(lab_off[k] >= 0 && lab_off[k + 1] >= lab_off[k], "%s: lab_off is not non-decreasing at source %d", fn, k);
  long total = 0;
  for (int b = 0; b < batch; b++) total += lab_off[items[b].src[0] + 1] - lab_off[items[b].src[0]];
  YS_REQUIRE(total <= capacity, "%s: the batch carries %ld labels, capacity is %d", fn, total, capacity);
  const size_t cap = (size_t)capacity, n_lab = (size_t)lab_off[n_src];
  DevBuf ds, dl, dc, db, dk, di, obi, ocl, obx, okp, ocn;
  YS_TRY(ds.alloc((size_t)n_src * sizeof(ys_aug_src))); YS_TRY(dl.alloc((size_t)(n_src + 1) * 4)); YS_TRY(dc.alloc(n_lab * 4)); YS_TRY(db.alloc(n_lab * 16));
  YS_TRY(dk.alloc(n_lab * xf * 4)); YS_TRY(di.alloc((size_t)batch * sizeof(ys_aug_item)));
  YS_TRY(obi.alloc(cap * 4)); YS_TRY(ocl.alloc(cap * 4)); YS_TRY(obx.alloc(cap * bw * 4)); YS_TRY(okp.alloc(cap * K * 12)); YS_TRY(ocn.alloc(4));
  YS_CHECK_HIP(hipMemcpyAsync(ds.p, srcs, (size_t)n_src * sizeof(ys_aug_src), hipMemcpyHostToDevice, st));
  YS_CHECK_HIP(hipMemcpyAsync(dl.p, lab_off, (size_t)(n_src + 1) * 4, hipMemcpyHostToDevice, st));
  if (n_lab) {
    YS_CHECK_HIP(hipMemcpyAsync(dc.p, cls, n_lab * 4, hipMemcpyHostToDevice, st));
    YS_CHECK_HIP(hipMemcpyAsync(db.p, boxes, n_lab * 16, hipMemcpyHostToDevice, st));
    if (xf) YS_CHECK_HIP(hipMemcpyAsync(dk.p, extra, n_lab * xf * 4, hipMemcpyHostToDevice, st));
  }
  YS_CHECK_HIP(hipMemcpyAsync(di.p, items, (size_t)batch * sizeof(ys_aug_item), hipMemcpyHostToDevice, st));
  YS_TRY(ys_aug_letterbox_labels_launch(st, (const ys_aug_src*)ds.p, n_src, (const int*)dl.p, (const float*)dc.p, (const float*)db.p,
                                        xf ? (const float*)dk.p : nullptr, K, (const ys_aug_item*)di.p, batch, imgsz, flags, capacity, ctx->aug_ws, (float*)obi.p,
                                        (float*)ocl.p, (float*)obx.p, K ? (float*)okp.p : nullptr, (int*)ocn.p, obb));
  YS_CHECK_HIP(hipMemcpyAsync(out_batch_idx, obi.p, cap * 4, hipMemcpyDeviceToHost, st));
  YS_CHECK_HIP(hipMemcpyAsync(out_cls, ocl.p, cap * 4, hipMemcpyDeviceToHost, st));
  YS_CHECK_HIP(hipMemcpyAsync(out_bboxes, obx.p, cap * bw * 4, hipMemcpyDeviceToHost, st));
  if (K) YS_CHECK_HIP(hipMemcpyAsync(out_keypoints, okp.p, cap * K * 12, hipMemcpyDeviceToHost, st));
  YS_CHECK_HIP(hipMemcpyAsync(out_count, ocn.p, 4, hipMemcpyDeviceToHost, st));
  YS_CHECK_HIP(hipStreamSynchronize(st));
  return YS_OK;
}
}  // namespace

extern "C" int ys_augment_letterbox_labels(ys_ctx* ctx, const ys_aug_src* srcs, int n_src, const int32_t* lab_off, const float* cls, const float* boxes,
                                           const float* keypoints, int kpt_num, int kpt_dim, const ys_aug_item* items, int batch, int on_device,
                                           int imgsz, int flags, int capacity, float* out_batch_idx, float* out_cls, float* out_bboxes,
                                           float* out_keypoints, int32_t* out_count) {
  return aug_letterbox_labels_impl("ys_augment_letterbox_labels", ctx, srcs, n_src, lab_off, cls, boxes, keypoints, kpt_num, kpt_dim, nullptr, 0, items, batch,
                                   on_device, imgsz, flags, capacity, out_batch_idx, out_cls, out_bboxes, out_keypoints, out_count);
}

extern "C" int ys_augment_letterbox_labels_obb(ys_ctx* ctx, const ys_aug_src* srcs, int n_src, const int32_t* lab_off, const float* cls, const float* boxes,
                                               const float* corners, const ys_aug_item* items, int batch, int on_device, int imgsz, int flags, int capacity,
                                               float* out_batch_idx, float* out_cls, float* out_bboxes, int32_t* out_count) {
  return aug_letterbox_labels_impl("ys_augment_letterbox_labels_obb", ctx, srcs, n_src, lab_off, cls, boxes, nullptr, 0, 3, corners, 1, items, batch, on_device,
                                   imgsz, flags, capacity, out_batch_idx, out_cls, out_bboxes, nullptr, out_count);
}
