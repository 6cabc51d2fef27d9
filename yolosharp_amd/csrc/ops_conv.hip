// ops_conv.hip -- per-operator entry points of the C ABI on the convolution kernels (unit parity; a TorchSharp-free Conv wrapper) and on the scaling
// machinery of the fp8 path (f8.hip), one call per kernel.  Host arrays in and out: test and parity entries, nothing a training step calls.
#include "ops_stage.h"

namespace {
// OIHW <-> [Cout][taps][Cin]
void weight_interleave(const float* src, int Cout, int Cin, int taps, bool back, float* dst) {
  for (int co = 0; co < Cout; co++)
    for (int ci = 0; ci < Cin; ci++)
      for (int t = 0; t < taps; t++) {
        const size_t oihw = ((size_t)co * Cin + ci) * taps + t, tapmajor = ((size_t)co * taps + t) * Cin + ci;
        if (back) dst[oihw] = src[tapmajor]; else dst[tapmajor] = src[oihw];
      }
}
std::vector<float> weights_to_tap_major(const float* w_oihw, int Cout, int Cin, int taps) {
  std::vector<float> wint((size_t)Cout * taps * Cin);
  weight_interleave(w_oihw, Cout, Cin, taps, false, wint.data());
  return wint;
}
void weights_to_oihw(const std::vector<float>& wint, int Cout, int Cin, int taps, float* w_oihw) { weight_interleave(wint.data(), Cout, Cin, taps, true, w_oihw); }

// The fp8 set-up of one convolution with CURRENT per-tensor scales of its own tensors, for both directions.  q, 1024 bytes of floats: [0] amax_w,
// [16..80) amax_x ways, [96..160) amax_dy ways, [200..204) scales.  dir 1 (forward): the operand is the packed input, its ways at 16, scales 200 / 201;
// dir 2 (dgrad): the operand is the packed output gradient, its ways at 96, scales 202 / 203.
struct F8Scratch { DevBuf w8, q, q8; };
constexpr int kF8Scales = 200;
inline int f8_ways_slot(int dir) { return dir == 1 ? 16 : 96; }

// w32: the n_w fp32 weights; wprep: the n_wq prepared bf16 weights the kernel of this direction reads; operand: [rows][ld] bf16.  record_amax: the launch records
// amax(|operand|) into the slots the scales launch just cleared, as a model's step does
int f8_setup(hipStream_t st, int dir, const float* w32, long n_w, const void* wprep, long n_wq, const void* operand, long rows, int ld, float prev_amax,
             bool record_amax, F8Scratch& s, ConvArgs& a) {
  YS_TRY(s.w8.alloc((size_t)n_wq));
  YS_TRY(s.q8.alloc((size_t)rows * ld));       // fp8 image of the operand for the blocked-GEMM kernel (quantised by ys_conv_launch)
  YS_TRY(s.q.alloc(1024));
  YS_CHECK_HIP(hipMemsetAsync(s.q.p, 0, 1024, st));
  float* qf = (float*)s.q.p;
  unsigned* ways = (unsigned*)(qf + f8_ways_slot(dir));
  F8Layer hl{0, n_w};
  F8Conv hc{0};
  DevBuf dl, dc;
  YS_TRY(dl.alloc(sizeof hl)); YS_TRY(dc.alloc(sizeof hc));
  YS_TRY(h2d(st, dl.p, &hl, sizeof hl));
  YS_TRY(h2d(st, dc.p, &hc, sizeof hc));
  YS_TRY(ys_f8_weight_amax_launch(st, w32, (const F8Layer*)dl.p, 1, qf));
  // delayed scaling (ys_conv_f8_fwd / ys_conv_f8_dgrad): the caller's amax of an EARLIER step stands in the slot instead of this operand's own
  if (prev_amax > 0.f) YS_TRY(h2d(st, ways, &prev_amax, 4));
  else YS_TRY(ys_f8_view_amax_launch(st, operand, rows, ld, ld, 0, ways));
  YS_TRY(ys_f8_scales_launch(st, (const F8Conv*)dc.p, 1, qf, (unsigned*)(qf + 16), (unsigned*)(qf + 96), qf + kF8Scales));
  YS_TRY(ys_f8_quant_weights_launch(st, wprep, n_wq, qf, s.w8.p));
  YS_CHECK_HIP(hipStreamSynchronize(st));     // hl / hc / dl / dc / prev_amax are temporaries of this scope
  const int sc = kF8Scales + 2 * (dir - 1);
  a.f8 = dir; a.w8 = s.w8.p; a.qscale = qf + sc; a.deq = qf + sc + 1; a.q8 = s.q8.p;
  if (record_amax) a.amax = ways;
  return YS_OK;
}
// the four scales and the amax ways the launch recorded, each where the caller asked for it
int f8_fetch(hipStream_t st, int dir, const F8Scratch& s, float* f8_scales, float* ways) {
  if (f8_scales) YS_TRY(d2h(st, f8_scales, (const float*)s.q.p + kF8Scales, 16));
  if (ways) YS_TRY(d2h(st, ways, (const float*)s.q.p + f8_ways_slot(dir), YS_AMAX_WAYS * 4));
  return YS_OK;
}
float max_way(const float* ways) { float m = 0.f; for (int i = 0; i < YS_AMAX_WAYS; i++) m = ways[i] > m ? ways[i] : m; return m; }
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
  const int epl = ys_epl(dtype);
  const size_t es = ys_es(dtype);
  const int cpad = ys_round_up(Cin, epl), cout_ld = ys_round_up(Cout, epl);
  const int pad = k / 2, taps = k * k;
  const int Ho = (H + 2 * pad - k) / stride + 1, Wo = (W + 2 * pad - k) / stride + 1;
  const long M = (long)B * Ho * Wo;
  const size_t cb = (size_t)Cout * 4;
  const std::vector<float> wint = weights_to_tap_major(w_oihw, Cout, Cin, taps);

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
  YS_TRY(h2d(st, dx.p, x_nchw, (size_t)B * Cin * H * W * 4));
  YS_TRY(h2d(st, dwm.p, wint.data(), wint.size() * 4));
  YS_TRY(ys_pack_input_launch(st, dtype, (const float*)dx.p, B, Cin, H, W, cpad, dxn.p));
  YS_TRY(ys_weight_prep_launch(st, dtype, (const float*)dwm.p, Cout, taps, Cin, cpad, cout_ld, dwf.p, nullptr, 0));

  // per-channel parameter block: gamma, beta, rmean, rvar, scale, shift, mean, rstd, bias, nbt
  YS_TRY(dpar.alloc((size_t)Cout * 10 * 4));
  float* par = (float*)dpar.p;
  float *g = par, *bt = par + Cout, *rm = par + 2 * Cout, *rv = par + 3 * Cout, *sc = par + 4 * Cout, *sh = par + 5 * Cout,
        *mu = par + 6 * Cout, *rs = par + 7 * Cout, *bs = par + 8 * Cout, *nbt = par + 9 * Cout;
  if (has_bn) {
    YS_TRY(h2d(st, g, bn_gamma, cb)); YS_TRY(h2d(st, bt, bn_beta, cb));
    YS_TRY(h2d(st, rm, bn_mean, cb)); YS_TRY(h2d(st, rv, bn_var, cb));
  }
  if (bias) YS_TRY(h2d(st, bs, bias, cb));
  YS_CHECK_HIP(hipMemsetAsync(nbt, 0, cb, st));

  ConvArgs a{};
  a.x = dxn.p; a.w = dwf.p;
  F8Scratch f8;
  if (want_f8 && Cin % 32 == 0)
    YS_TRY(f8_setup(st, 1, (const float*)dwm.p, (long)Cout * taps * Cin, dwf.p, (long)Cout * taps * cpad, dxn.p, (long)B * H * W, cpad, prev_amax, f8_amax != nullptr, f8, a));
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
    if (coef) YS_TRY(d2h(st, coef, sc, 4 * cb));      // scale, shift, mean, rstd are adjacent in the parameter block
    if (y_raw) {
      YS_TRY(ys_unpack_nchw_launch(st, dtype, dy.p, cout_ld, 0, B, Cout, (long)Ho * Wo, (float*)dout.p));
      YS_TRY(d2h(st, y_raw, dout.p, (size_t)M * Cout * 4));
    }
    YS_TRY(d2h(st, bn_mean, rm, cb));
    YS_TRY(d2h(st, bn_var, rv, cb));
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
  YS_TRY(d2h(st, y_nchw, dout.p, (size_t)M * Cout * 4));
  float ways[YS_AMAX_WAYS] = {};
  if (a.f8) YS_TRY(f8_fetch(st, 1, f8, f8_scales, f8_amax ? ways : nullptr));
  YS_CHECK_HIP(hipStreamSynchronize(st));
  YS_CHECK_HIP(hipGetLastError());
  if (f8_amax) *f8_amax = max_way(ways);
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
  const int epl = ys_epl(dtype);
  const size_t es = ys_es(dtype);
  const int cpad = ys_round_up(Cin, epl), copad = ys_round_up(Cout, epl);
  const int pad = k / 2, taps = k * k;
  const int Ho = (H + 2 * pad - k) / stride + 1, Wo = (W + 2 * pad - k) / stride + 1;
  const long M = (long)B * Ho * Wo;
  const std::vector<float> wint = weights_to_tap_major(w_oihw, Cout, Cin, taps);
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
  if (dw_oihw) YS_TRY(h2d(st, dx.p, x_nchw, (size_t)B * Cin * H * W * 4));
  YS_TRY(h2d(st, ddy.p, dy_nchw, (size_t)M * Cout * 4));
  YS_TRY(h2d(st, dwm.p, wint.data(), wint.size() * 4));
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
    YS_TRY(d2h(st, gw.data(), dgw.p, gw.size() * 4));
  }
  float ways[YS_AMAX_WAYS] = {};
  if (dx_nchw) {
    ConvArgs a{};
    a.x = ddyn.p; a.w = dwd.p; a.y = dgx.p;
    F8Scratch f8;
    if (want_f8 && Cout % 32 == 0)
      YS_TRY(f8_setup(st, 2, (const float*)dwm.p, (long)Cout * taps * Cin, dwd.p, (long)Cin * taps * copad, ddyn.p, M, copad, prev_amax, f8_amax != nullptr, f8, a));
    a.B = B; a.Hin = Ho; a.Win = Wo; a.Cin = copad; a.Hout = H; a.Wout = W; a.Cout = Cin; a.KH = a.KW = k;
    a.SA = 1; a.DIVS = stride == 2 ? 1 : 0; a.DIVM = stride - 1; a.PAD = k - 1 - pad;
    a.in_ldc = copad; a.in_coff = 0; a.in_bstride = (long)Ho * Wo;
    a.out_ldc = cpad; a.out_coff = 0; a.out_bstride = (long)H * W; a.vec_ok = 1; a.M = B * H * W;
    YS_TRY(ys_conv_launch(st, dtype, a));
    YS_TRY(ys_unpack_nchw_launch(st, dtype, dgx.p, cpad, 0, B, Cin, (long)H * W, (float*)dgxo.p));
    YS_TRY(d2h(st, dx_nchw, dgxo.p, (size_t)B * Cin * H * W * 4));
    if (a.f8) YS_TRY(f8_fetch(st, 2, f8, f8_scales, f8_amax ? ways : nullptr));
    YS_CHECK_HIP(hipStreamSynchronize(st));     // the F8Scratch buffers are temporaries of this scope
  }
  YS_CHECK_HIP(hipStreamSynchronize(st));
  if (dw_oihw) weights_to_oihw(gw, Cout, Cin, taps, dw_oihw);
  YS_CHECK_HIP(hipGetLastError());
  if (f8_amax) *f8_amax = max_way(ways);
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

// ---- Yolov5u's stem Conv(3, Cout, 6, 2, 2) on the kernels of conv_stem6.hip alone (a model's bf16 model.0): the image stays fp32 NCHW on the device, the
// weights go through the model's weight prep ([Cout][36][8] bf16), the outputs sit in sentinel-guarded buffers
static int stem6_stage(hipStream_t st, const float* x_nchw, int B, int H, int W, DevBuf& dx) {
  YS_TRY(dx.alloc((size_t)B * 3 * H * W * 4));
  return h2d(st, dx.p, x_nchw, (size_t)B * 3 * H * W * 4);
}

extern "C" int ys_stem6_fwd(ys_ctx* ctx, const float* x_nchw, int B, int H, int W, const float* w_oihw, int Cout, int stat_mode,
                            const float* scale, const float* shift, int act, float* y_nchw, double* stats) {
  YS_REQUIRE(ctx && x_nchw && w_oihw && y_nchw, "ys_stem6_fwd: null argument");
  YS_REQUIRE(stat_mode == 0 || stat_mode == 1, "ys_stem6_fwd: stat_mode %d", stat_mode);
  const bool train = scale == nullptr;
  YS_REQUIRE(train ? stats != nullptr : shift != nullptr, "ys_stem6_fwd: %s", train ? "the training form returns stats" : "eval needs scale and shift");
  if (!ys_stem6_eligible(YS_BF16, 3, Cout, 6, 2, 2) || B < 1 || H < 2 || W < 2 || (long)B * 3 * H * W >= (1L << 31)) {
    ys_set_error("ys_stem6_fwd: the 6x6 stem kernels take Cout in {16, 32, 48, 64, 80} and images of at least 2 x 2 (Cout %d, B %d, %d x %d)", Cout, B, H, W);
    return YS_ERR_UNSUPPORTED;
  }
  YS_CHECK_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const int Ho = (H - 2) / 2 + 1, Wo = (W - 2) / 2 + 1;
  const long M = (long)B * Ho * Wo;
  const std::vector<float> wint = weights_to_tap_major(w_oihw, Cout, 3, 36);
  DevBuf dx, dwm, dwf, dy, dout, dstat, dacc, dpar;
  YS_TRY(stem6_stage(st, x_nchw, B, H, W, dx));
  YS_TRY(dwm.alloc(wint.size() * 4));
  YS_TRY(dwf.alloc((size_t)Cout * 36 * 8 * 2));
  YS_TRY(h2d(st, dwm.p, wint.data(), wint.size() * 4));
  YS_TRY(ys_weight_prep_launch(st, YS_BF16, (const float*)dwm.p, Cout, 36, 3, 8, Cout, dwf.p, nullptr, 0));
  const size_t yb = (size_t)M * Cout * 2;
  YS_TRY(alloc_filled(dy, yb + kGuardFloats * 4, st));
  YS_TRY(dout.alloc((size_t)M * Cout * 4));
  int rows = ys_stem6_fwd_rows(B, Ho, Wo), ok = 1;
  const size_t accb = (size_t)YS_STAT_SHARDS * Cout * 2 * sizeof(unsigned long long), rowb = (size_t)rows * 2 * Cout * 4;
  if (train) {
    YS_TRY(alloc_filled(dstat, rowb + kGuardFloats * 4, st));
    if (stat_mode == 1) { YS_TRY(dacc.alloc(accb)); YS_CHECK_HIP(hipMemsetAsync(dacc.p, 0, accb, st)); }
    YS_TRY(ys_stem6_fwd_launch(st, (const float*)dx.p, B, H, W, dwf.p, Cout, dy.p, Cout, 0, (long)Ho * Wo, (float*)dstat.p, nullptr, nullptr, 0, &rows,
                               stat_mode == 1 ? (unsigned long long*)dacc.p : nullptr));
    if (stat_mode == 1) {
      std::vector<long long> h((size_t)YS_STAT_SHARDS * Cout * 2);
      YS_TRY(d2h(st, h.data(), dacc.p, accb));
      YS_CHECK_HIP(hipStreamSynchronize(st));
      for (int c = 0; c < Cout; c++)
        for (int w = 0; w < 2; w++) {
          long long s = 0;
          for (int sh = 0; sh < YS_STAT_SHARDS; sh++) s += h[((size_t)sh * Cout + c) * 2 + w];
          stats[(size_t)w * Cout + c] = (double)s / (double)YS_STAT_FIX;
        }
    } else {
      std::vector<float> h((size_t)rows * 2 * Cout);
      YS_TRY(d2h(st, h.data(), dstat.p, rowb));
      YS_CHECK_HIP(hipStreamSynchronize(st));
      for (int i = 0; i < 2 * Cout; i++) stats[i] = 0.0;
      for (int r = 0; r < rows; r++) for (int i = 0; i < 2 * Cout; i++) stats[i] += (double)h[(size_t)r * 2 * Cout + i];
    }
    YS_TRY(check_guard(st, dstat.p, rowb, &ok));
  } else {
    YS_TRY(dpar.alloc((size_t)Cout * 2 * 4));
    YS_TRY(h2d(st, dpar.p, scale, (size_t)Cout * 4));
    YS_TRY(h2d(st, (float*)dpar.p + Cout, shift, (size_t)Cout * 4));
    YS_TRY(ys_stem6_fwd_launch(st, (const float*)dx.p, B, H, W, dwf.p, Cout, dy.p, Cout, 0, (long)Ho * Wo, nullptr, (const float*)dpar.p, (const float*)dpar.p + Cout,
                               act ? 1 : 0, nullptr, nullptr));
  }
  YS_TRY(ys_unpack_nchw_launch(st, YS_BF16, dy.p, Cout, 0, B, Cout, (long)Ho * Wo, (float*)dout.p));
  YS_TRY(d2h(st, y_nchw, dout.p, (size_t)M * Cout * 4));
  YS_TRY(check_guard(st, dy.p, yb, &ok));
  YS_CHECK_HIP(hipStreamSynchronize(st));
  YS_CHECK_HIP(hipGetLastError());
  YS_REQUIRE(ok, "ys_stem6_fwd: the kernel wrote behind its arrays");
  return YS_OK;
}

extern "C" int ys_stem6_wgrad(ys_ctx* ctx, const float* x_nchw, int B, int H, int W, const float* dy_nchw, int Cout, float* dw_oihw) {
  YS_REQUIRE(ctx && x_nchw && dy_nchw && dw_oihw, "ys_stem6_wgrad: null argument");
  if (!ys_stem6_eligible(YS_BF16, 3, Cout, 6, 2, 2) || B < 1 || H < 2 || W < 2 || (long)B * 3 * H * W >= (1L << 31)) {
    ys_set_error("ys_stem6_wgrad: the 6x6 stem kernels take Cout in {16, 32, 48, 64, 80} and images of at least 2 x 2 (Cout %d, B %d, %d x %d)", Cout, B, H, W);
    return YS_ERR_UNSUPPORTED;
  }
  YS_CHECK_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const int Ho = (H - 2) / 2 + 1, Wo = (W - 2) / 2 + 1;
  const long M = (long)B * Ho * Wo, n = (long)Cout * 36 * 8;
  DevBuf dx, ddy, ddyn, dpart, dgw, ddesc;
  YS_TRY(stem6_stage(st, x_nchw, B, H, W, dx));
  YS_TRY(ddy.alloc((size_t)M * Cout * 4));
  YS_TRY(ddyn.alloc((size_t)M * Cout * 2));
  YS_TRY(h2d(st, ddy.p, dy_nchw, (size_t)M * Cout * 4));
  YS_TRY(ys_pack_input_launch(st, YS_BF16, (const float*)ddy.p, B, Cout, Ho, Wo, Cout, ddyn.p));
  const int splits = ys_stem6_wgrad_splits(B, H, W);
  const size_t pb = (size_t)splits * n * 4;
  YS_TRY(alloc_filled(dpart, pb + kGuardFloats * 4, st));
  YS_TRY(dgw.alloc((size_t)Cout * 36 * 3 * 4));
  YS_CHECK_HIP(hipMemsetAsync(dgw.p, 0, (size_t)Cout * 36 * 3 * 4, st));
  int used = 0, ok = 1;
  YS_TRY(ys_stem6_wgrad_launch(st, (const float*)dx.p, B, H, W, ddyn.p, Cout, 0, (long)Ho * Wo, Cout, (float*)dpart.p, splits, &used));
  // the split reduction of a backward segment (model.hip reduce_range), with this layer as its only descriptor
  WgRedDesc d{};
  d.partial = (const float*)dpart.p; d.grad = (float*)dgw.p; d.n = n; d.blk0 = 0; d.splits = used; d.cin_pad = 8; d.cin_real = 3;
  YS_TRY(ddesc.alloc(sizeof d));
  YS_TRY(h2d(st, ddesc.p, &d, sizeof d));
  YS_TRY(ys_wgrad_reduce_batched_launch(st, (const WgRedDesc*)ddesc.p, 1, (n + YS_WGRED_OUT_PER_BLOCK - 1) / YS_WGRED_OUT_PER_BLOCK));
  std::vector<float> gw((size_t)Cout * 36 * 3);
  YS_TRY(d2h(st, gw.data(), dgw.p, gw.size() * 4));
  YS_TRY(check_guard(st, dpart.p, pb, &ok));
  YS_CHECK_HIP(hipStreamSynchronize(st));
  YS_CHECK_HIP(hipGetLastError());
  YS_REQUIRE(ok, "ys_stem6_wgrad: the kernel wrote behind its arrays");
  weights_to_oihw(gw, Cout, 3, 36, dw_oihw);
  return YS_OK;
}

// ---- scaling machinery of the fp8 path (f8.hip), one call per kernel
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
  YS_TRY(check_guard(st, dq.p, n, &ok));
  if (kind == 2) YS_TRY(check_guard(st, dq.p, 0, &ok));          // the amax pass writes no image
  const int view[1][2] = {{coff, C}};
  if (ld != C) YS_TRY(check_sentinel(st, dx.p, rows, ld, 2, view, 1, &ok));
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
  const size_t gb = kGuardFloats * 4, lb = (size_t)n_layers * 4, slotb = (size_t)n_convs * YS_AMAX_WAYS * 4, scb = (size_t)n_convs * 16;
  DevBuf dp, dl, dc, daw, dax, dag, dsc;
  YS_TRY(dp.alloc((size_t)n_params * 4)); YS_TRY(dl.alloc(hl.size() * sizeof(F8Layer))); YS_TRY(dc.alloc(hc.size() * sizeof(F8Conv)));
  YS_TRY(alloc_filled(daw, lb + gb, st));
  YS_TRY(alloc_filled(dax, slotb + gb, st)); YS_TRY(alloc_filled(dag, slotb + gb, st));
  YS_TRY(alloc_filled(dsc, scb + gb, st));
  YS_TRY(h2d(st, dp.p, params, (size_t)n_params * 4));
  YS_TRY(h2d(st, dl.p, hl.data(), hl.size() * sizeof(F8Layer))); YS_TRY(h2d(st, dc.p, hc.data(), hc.size() * sizeof(F8Conv)));
  YS_TRY(h2d(st, dax.p, amax_x, slotb)); YS_TRY(h2d(st, dag.p, amax_dy, slotb));
  YS_TRY(h2d(st, dsc.p, scales, scb));
  YS_TRY(ys_f8_weight_amax_launch(st, (const float*)dp.p, (const F8Layer*)dl.p, n_layers, (float*)daw.p));
  YS_TRY(ys_f8_scales_launch(st, (const F8Conv*)dc.p, n_convs, (const float*)daw.p, (unsigned*)dax.p, (unsigned*)dag.p, (float*)dsc.p));
  YS_TRY(d2h(st, amax_w, daw.p, lb));
  YS_TRY(d2h(st, amax_x, dax.p, slotb)); YS_TRY(d2h(st, amax_dy, dag.p, slotb));
  YS_TRY(d2h(st, scales, dsc.p, scb));
  int ok = 1;
  YS_TRY(check_guard(st, daw.p, lb, &ok)); YS_TRY(check_guard(st, dax.p, slotb, &ok)); YS_TRY(check_guard(st, dag.p, slotb, &ok));
  YS_TRY(check_guard(st, dsc.p, scb, &ok));
  YS_CHECK_HIP(hipStreamSynchronize(st));
  YS_CHECK_HIP(hipGetLastError());
  YS_REQUIRE(ok, "ys_f8_scales: a kernel wrote behind its arrays");
  return YS_OK;
}
