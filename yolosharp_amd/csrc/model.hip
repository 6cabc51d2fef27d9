// model.hip -- the step behind ys_model_forward / ys_model_backward* / ys_block_* / ys_head_* (the handle: ys_model.h; the graph it walks: graph.hip; the
// layout, allocations and plans it follows: plan.hip; the entry points: model_api.hip; the criterion: criterion.hip).
//
// Forward and backward live in ONE unit: they share fwd_args / dgrad_args, the BatchNorm operand helpers and the weight-gradient stream state.
// Training forward keeps the raw conv output y per Conv unit (BN backward needs it); backward walks the op
// list in reverse, gradient buffers mirror activation buffers, "first writer writes, later writers accumulate".
#include "ys_model.h"
#include <cstring>
#include <algorithm>

namespace ysm {

// ---- operands of Conv unit c that several launches share: its coefficient rows (scale, shift, mean, rstd, c1, c2) and its pre-BN output
static float* chan_ptr(ys_model* m, const ConvL& c, int which) { return m->chan + c.ch_off + (long)which * ((c.cout + 3) / 4 * 4); }
static char* y_ptr(const ys_model* m, const ConvL& c) { return (char*)m->y_all + (size_t)c.y_off * m->es; }
// the shortcut view its BN / SiLU apply pass adds (null without one)
struct ResView { const void* p = nullptr; int ldc = 0, coff = 0; };
static ResView res_view(const ys_model* m, const ConvL& c) {
  if (!c.has_res) return ResView{};
  return ResView{m->bufs[c.res.buf].act, m->bufs[c.res.buf].ldc, c.res.coff};
}
// everything a training-mode BatchNorm finalize reads and writes, over `nblk` statistics rows at `partial`
static BnFinProb bn_fin(ys_model* m, const ConvL& c, const float* partial, int nblk, long count) {
  return BnFinProb{partial, nblk, c.cout, (double)count, m->params + c.g_off, m->params + c.b_off, m->state + c.rm_off, m->state + c.rv_off,
                   m->state + c.nbt_off, chan_ptr(m, c, 0), chan_ptr(m, c, 1), chan_ptr(m, c, 2), chan_ptr(m, c, 3)};
}
static int bn_finalize(ys_model* m, const ConvL& c, const float* partial, int nblk, long count) {
  const BnFinProb p = bn_fin(m, c, partial, nblk, count);
  return ys_bn_finalize_launch(m->ctx->stream, partial, nblk, c.cout, count, p.gamma, p.beta, BN_EPS, BN_MOMENTUM, p.run_mean, p.run_var, p.nbt,
                               p.scale, p.shift, p.mean, p.rstd);
}

// ------------------------------------------------------------------ forward
// depthwise Conv unit: y = dwconv(x) (dense), then BN statistics / apply exactly like the dense path
static int run_dwconv_fwd(ys_model* m, const ConvL& c, int B) {
  hipStream_t st = m->ctx->stream;
  const Buf& ib = m->bufs[c.in.buf];
  const Buf& ob = m->bufs[c.out.buf];
  const long M = (long)B * c.Hout * c.Wout;
  void* y = y_ptr(m, c);
  YS_TRY(ys_dwconv_launch(st, m->dtype, 0, ib.act, ib.ldc, c.in.coff, B, c.Hin, c.Win, c.cout, m->params + c.w_off, y, c.cout, 0, 0));
  if (m->training) {
    int nblk = 0;
    YS_TRY(ys_chan_stats_launch(st, m->dtype, y, M, c.cout, m->stat_partial, &nblk));
    YS_TRY(bn_finalize(m, c, m->stat_partial, nblk, M));
  }
  const ResView r = res_view(m, c);
  YS_TRY(ys_bn_act_apply_launch(st, m->dtype, y, M, c.cout, chan_ptr(m, c, 0), chan_ptr(m, c, 1), c.act ? 1 : 0, r.p, r.ldc, r.coff,
                                ob.act, ob.ldc, c.out.coff));
  return YS_OK;
}

// ConvTranspose2d(k=2, s=2, bias): out[b, 2h+dh, 2w+dw, :] = W[dh,dw] x[b,h,w,:] + bias  -> four 1x1 GEMMs with a strided output map
static int run_convT_fwd(ys_model* m, const ConvL& c, int B) {
  hipStream_t st = m->ctx->stream;
  const Buf& ib = m->bufs[c.in.buf];
  const Buf& ob = m->bufs[c.out.buf];
  for (int ph = 0; ph < 4; ph++) {
    const int dh = ph >> 1, dw = ph & 1;
    ConvArgs a{};
    a.x = ib.act; a.w = (char*)m->wf_all + (size_t)(c.wf_off + (long)ph * c.cout * c.cin_pad) * m->es; a.y = ob.act;
    a.B = B; a.Hin = c.Hin; a.Win = c.Win; a.Cin = c.cin_pad; a.Hout = c.Hin; a.Wout = c.Win; a.Cout = c.cout; a.KH = a.KW = 1;
    a.SA = 1; a.PAD = 0;
    a.in_ldc = ib.ldc; a.in_coff = c.in.coff; a.in_bstride = ib.rows_per_b;
    a.out_ldc = ob.ldc; a.out_coff = c.out.coff; a.out_bstride = ob.rows_per_b;
    a.out_rh = 4 * c.Win; a.out_rw = 2; a.out_r0 = (long)dh * 2 * c.Win + dw;
    a.vec_ok = (ob.ldc % 4 == 0 && c.out.coff % 4 == 0) ? 1 : 0;
    a.shift = m->params + c.g_off;
    a.M = B * c.Hin * c.Win;
    YS_TRY(ys_conv_launch(st, m->dtype, a));
  }
  return YS_OK;
}

// geometry / operand part of the forward convolution arguments of layer c
static ConvArgs fwd_args(ys_model* m, const ConvL& c, int B) {
  const Buf& ib = m->bufs[c.in.buf];
  ConvArgs a{};
  a.x = ib.act; a.w = (char*)m->wf_all + (size_t)c.wf_off * m->es;
  a.B = B; a.Hin = c.Hin; a.Win = c.Win; a.Cin = c.cin_pad; a.Hout = c.Hout; a.Wout = c.Wout; a.Cout = c.cout; a.KH = a.KW = c.k;
  a.SA = c.s; a.DIVS = 0; a.DIVM = 0; a.PAD = c.pad;
  a.in_ldc = ib.ldc; a.in_coff = c.in.coff; a.in_bstride = ib.rows_per_b;
  a.M = B * c.Hout * c.Wout;
  return a;
}

// finalize-inside-apply operands of BatchNorm unit c (ys_bn_fin_apply_launch): its accumulators + everything bn_finalize_kernel reads and writes
static BnAccFin bn_acc_fin(ys_model* m, const ConvL& c, long count) {
  const BnFinProb p = bn_fin(m, c, nullptr, 0, count);
  BnAccFin f{};
  f.acc = m->stat_acc_all + c.acc_off; f.count = p.count;
  f.gamma = p.gamma; f.beta = p.beta; f.run_mean = p.run_mean; f.run_var = p.run_var; f.nbt = p.nbt;
  f.scale = p.scale; f.shift = p.shift; f.mean = p.mean; f.rstd = p.rstd;
  f.eps = BN_EPS; f.momentum = BN_MOMENTUM;
  return f;
}

// where the convolution of unit c writes: a training-mode BN unit's pre-BN output y, else the output view with the epilogue's BN coefficients / bias
static void fwd_out_operands(ys_model* m, const ConvL& c, ConvArgs& a) {
  const Buf& ob = m->bufs[c.out.buf];
  if (c.bn && m->training) {
    a.y = y_ptr(m, c); a.out_ldc = c.cout; a.out_coff = 0; a.out_bstride = (long)c.Hout * c.Wout; a.vec_ok = (c.cout % 4 == 0);
    return;
  }
  a.y = view_ptr(m, ob.act, ob, c.out_rowoff);
  a.out_ldc = ob.ldc; a.out_coff = c.out.coff; a.out_bstride = ob.rows_per_b; a.vec_ok = (ob.ldc % 4 == 0 && c.out.coff % 4 == 0) ? 1 : 0;
  if (c.bn) {
    const ResView r = res_view(m, c);
    a.scale = chan_ptr(m, c, 0); a.shift = chan_ptr(m, c, 1); a.act = c.act ? 1 : 0; a.res = r.p; a.res_ldc = r.ldc; a.res_coff = r.coff;
  } else {
    a.shift = m->params + c.g_off;  // conv bias
  }
}
// fp8 forward of unit c: its e4m3 forward weights and activation scale pair
static void f8_fwd_operands(const ys_model* m, const ConvL& c, ConvArgs& a) {
  a.f8 = 1; a.w8 = m->wf8_all + c.wf_off; a.qscale = m->f8_scales + 4L * c.idx; a.deq = m->f8_scales + 4L * c.idx + 1;
}

// `next`: the convolution that runs right after this one, when it reads exactly the view this one writes (else null)
static int run_conv_fwd(ys_model* m, const ConvL& c, int B, const ConvL* next = nullptr) {
  if (c.dw) return run_dwconv_fwd(m, c, B);
  if (c.ct) return run_convT_fwd(m, c, B);
  hipStream_t st = m->ctx->stream;
  float* stat_partial = m->stat_partial;
  const Buf& ib = m->bufs[c.in.buf];
  const Buf& ob = m->bufs[c.out.buf];
  if (c.first && m->in_f32) {      // model.0 straight from the fp32 image planes (conv_stem.hip)
    const long Ms = (long)B * c.Hout * c.Wout;
    const void* wf = (char*)m->wf_all + (size_t)c.wf_off * m->es;
    const auto stem_fwd = c.k == 6 ? ys_stem6_fwd_launch : ys_stem_fwd_launch;      // Yolov5u's 6x6 stem (conv_stem6.hip): the same contract
    if (m->training) {
      void* y = y_ptr(m, c);
      int gm = 0;
      const bool atomic = m->bn_atomic && c.acc_off >= 0;
      YS_TRY(stem_fwd(st, m->in_f32, B, c.Hin, c.Win, wf, c.cout, y, c.cout, 0, (long)c.Hout * c.Wout, stat_partial, nullptr, nullptr, 0, &gm,
                                atomic ? m->stat_acc_all + c.acc_off : nullptr));
      if (atomic) {
        YS_TRY(ys_bn_fin_apply_launch(st, m->dtype, y, Ms, c.cout, bn_acc_fin(m, c, Ms), c.act ? 1 : 0, nullptr, 0, 0, ob.act, ob.ldc, c.out.coff));
      } else {
        YS_TRY(bn_finalize(m, c, stat_partial, gm, Ms));
        YS_TRY(ys_bn_act_apply_launch(st, m->dtype, y, Ms, c.cout, chan_ptr(m, c, 0), chan_ptr(m, c, 1), c.act ? 1 : 0, nullptr, 0, 0,
                                      ob.act, ob.ldc, c.out.coff, nullptr));
      }
    } else {
      YS_TRY(stem_fwd(st, m->in_f32, B, c.Hin, c.Win, wf, c.cout, ob.act, ob.ldc, c.out.coff, ob.rows_per_b, nullptr,
                      chan_ptr(m, c, 0), chan_ptr(m, c, 1), c.act ? 1 : 0, nullptr, nullptr));
    }
    return YS_OK;
  }
  ConvArgs a = fwd_args(m, c, B);
  const long M = a.M;
  if (m->f8 && c.f8_fwd) {
    unsigned* slots = m->amax_act + (size_t)c.idx * YS_AMAX_WAYS;
    if (m->f8_sx_valid) {   // fp8 MFMA kernel where one is planned (ys_conv_launch falls back to bf16 otherwise); it records amax(|x|) itself
      f8_fwd_operands(m, c, a); a.amax = slots;
      a.q8 = m->q8;
      if (m->q8_fwd_ready == c.idx) { a.x8 = m->q8; a.amax = nullptr; }   // image and maximum written by the producer's BN / SiLU pass
    } else {                // first pass: no scale yet -> bf16 kernels, and a bootstrap pass records the input maximum
      YS_TRY(ys_f8_view_amax_launch(st, ib.act, (long)B * c.Hin * c.Win, c.cin_pad, ib.ldc, c.in.coff, slots));
    }
  }
  fwd_out_operands(m, c, a);
  if (!(c.bn && m->training)) return ys_conv_launch(st, m->dtype, a);
  void* y = a.y;
  a.stats = stat_partial;
  // Classify's Conv unit: statistics rows + bn_finalize here, the BN + SiLU apply inside the pool op (OP_POOL) -- no activated map
  const bool atomic = m->bn_atomic && c.acc_off >= 0 && !a.f8 && !c.pool_next;
  if (atomic) a.stat_acc = m->stat_acc_all + c.acc_off;
  YS_TRY(ys_conv_launch(st, m->dtype, a));
  const ResView r = res_view(m, c);
  if (atomic)   // the statistics left the convolution already reduced (integer sums): finalize + BN + SiLU in ONE pass, no bn_finalize launch
    return ys_bn_fin_apply_launch(st, m->dtype, y, M, c.cout, bn_acc_fin(m, c, M), c.act ? 1 : 0, r.p, r.ldc, r.coff, ob.act, ob.ldc, c.out.coff);
  YS_TRY(bn_finalize(m, c, stat_partial, ys_conv_grid_m(a, m->dtype), M));
  if (c.pool_next) return YS_OK;
  // fp8 mode: the next convolution of the schedule reads exactly this output and will run the fp8 blocked-GEMM kernel -> this pass also writes
  // the e4m3 image it consumes (the consumer's delayed scale) into the scratch and records its maximum
  bool q8_out = false;
  if (next && m->f8 && m->f8_sx_valid && next->f8_fwd && m->q8 && m->dtype == YS_BF16 && !next->dw && !next->ct) {
    ConvArgs q = fwd_args(m, *next, B);
    f8_fwd_operands(m, *next, q);
    q8_out = ys_conv_wants_x8(q);
  }
  if (q8_out) {
    YS_TRY(ys_bn_act_apply_q8_launch(st, y, M, c.cout, chan_ptr(m, c, 0), chan_ptr(m, c, 1), c.act ? 1 : 0, r.p, r.ldc, r.coff, ob.act, ob.ldc,
                                     c.out.coff, m->q8, m->f8_scales + 4L * next->idx, m->amax_act + (size_t)next->idx * YS_AMAX_WAYS));
    m->q8_fwd_ready = next->idx;
    return YS_OK;
  }
  return ys_bn_act_apply_launch(st, m->dtype, y, M, c.cout, chan_ptr(m, c, 0), chan_ptr(m, c, 1), c.act ? 1 : 0, r.p, r.ldc, r.coff,
                                ob.act, ob.ldc, c.out.coff, nullptr);
}

// ---- grouped forward of n independent Conv units / plain convolutions of one head stage (ConvL::group): one grouped convolution
// launch when the problems share a kernel variant (same channels and taps: the .1 / .2 tower layers of the three levels), else one
// launch each; then ONE BatchNorm finalize and ONE BN + SiLU apply launch for the whole stage.  Same arithmetic as run_conv_fwd.
static int run_conv_fwd_group(ys_model* m, ConvL* const* cs, int n, int B) {
  hipStream_t st = m->ctx->stream;
  bool ok = n >= 2 && n <= YS_GROUP_MAX && !m->f8;
  for (int i = 0; i < n && ok; i++) {
    const ConvL& c = *cs[i];
    ok = !c.dw && !c.ct && !c.has_res && c.gstat_off >= 0 && c.bn == cs[0]->bn && c.act == cs[0]->act;
  }
  if (!ok) { for (int i = 0; i < n; i++) YS_TRY(run_conv_fwd(m, *cs[i], B)); return YS_OK; }
  ConvArgs a[YS_GROUP_MAX];
  int rows[YS_GROUP_MAX] = {0, 0, 0}, cap[YS_GROUP_MAX] = {0, 0, 0};
  const bool bn_train = cs[0]->bn && m->training;
  for (int i = 0; i < n; i++) {
    a[i] = fwd_args(m, *cs[i], B);
    fwd_out_operands(m, *cs[i], a[i]);
    if (bn_train) a[i].stats = m->stat_group + cs[i]->gstat_off;
    // a unit's statistics region holds 2 * ceil(M / 64) rows (plan.hip allocate).  A map smaller than one pixel tile has one tile per IMAGE -- three images of
    // a 3 x 5 map are 3 tiles for M = 45 -- so the persistent grid is held to the rows there are: its workgroups walk the tiles between them
    cap[i] = (int)(2 * ys_cdiv((long)a[i].M, 64));
  }
  int rc = m->dtype == YS_BF16 ? ys_conv_p2_group_launch(st, a, n, bn_train ? cap : nullptr, rows) : YS_ERR_UNSUPPORTED;
  if (rc == YS_ERR_UNSUPPORTED) {
    for (int i = 0; i < n; i++) rows[i] = ys_conv_grid_m(a[i], m->dtype);
    bool fits = true;
    for (int i = 0; i < n; i++) fits = fits && (!bn_train || rows[i] <= cap[i]);
    if (!fits) { for (int i = 0; i < n; i++) YS_TRY(run_conv_fwd(m, *cs[i], B)); return YS_OK; }     // (single launches cannot be capped: the shared statistics scratch)
    for (int i = 0; i < n; i++) YS_TRY(ys_conv_launch(st, m->dtype, a[i]));
  } else if (rc != YS_OK) return rc;
  if (!bn_train) return YS_OK;
  BnFinProb fp[YS_GROUP_MAX];
  BnApplyProb ap[YS_GROUP_MAX];
  for (int i = 0; i < n; i++) {
    const ConvL& c = *cs[i];
    const Buf& ob = m->bufs[c.out.buf];
    fp[i] = bn_fin(m, c, m->stat_group + c.gstat_off, rows[i], a[i].M);
    ap[i] = BnApplyProb{a[i].y, a[i].M, c.cout, chan_ptr(m, c, 0), chan_ptr(m, c, 1), nullptr, 0, 0, ob.act, ob.ldc, c.out.coff};
  }
  YS_TRY(ys_bn_finalize_group_launch(st, fp, n, BN_EPS, BN_MOMENTUM));
  YS_TRY(ys_bn_act_apply_group_launch(st, m->dtype, ap, n, cs[0]->act ? 1 : 0));
  return YS_OK;
}

// SPPF: ops [i0, i0 + 2] are three max-pools chained through the slices of one concat buffer, and the one-launch form takes the view (elementwise.hip)
static bool sppf_chain(const ys_model* m, int i0, int* coff) {
  if (!m->sppf_fuse || i0 < 0 || i0 + 2 >= (int)m->ops.size()) return false;
  const Op& o0 = m->ops[i0];
  for (int k = 0; k < 3; k++) {
    const Op& o = m->ops[i0 + k];
    if (o.type != OP_MAXPOOL || o.in.buf != o0.in.buf || o.out.buf != o0.in.buf || o.in.C != o0.in.C || o.out.C != o0.in.C || o.H != o0.H || o.W != o0.W ||
        o.seg != o0.seg) return false;
    if (k > 0 && o.in.coff != m->ops[i0 + k - 1].out.coff) return false;
    coff[k] = o.in.coff; coff[k + 1] = o.out.coff;
  }
  for (int i = 0; i < 4; i++) for (int j = i + 1; j < 4; j++) if (abs(coff[i] - coff[j]) < o0.in.C) return false;   // four distinct slices
  unsigned char* am[3];
  for (int k = 0; k < 3; k++) am[k] = m->argmax + m->ops[i0 + k].aux_off;
  return ys_sppf_pool3_ok(m->dtype, o0.H, o0.W, o0.in.C, m->bufs[o0.in.buf].ldc, coff, am) != 0;
}

// the units of the head-stage group (ConvL::group) op i belongs to, in forward order: the run of consecutive ops of that group from i on in direction
// `step` (+1: i is its first op, -1: its last).  Returns their count (<= YS_GROUP_MAX)
static int group_run(ys_model* m, int i, int step, ConvL** gc) {
  const int gid = m->convs[m->ops[i].conv].group;
  int gn = 0;
  for (int j = i; j >= 0 && j < (int)m->ops.size() && gn < YS_GROUP_MAX && m->ops[j].type == OP_CONV && m->convs[m->ops[j].conv].group == gid; j += step) gn++;
  for (int k = 0; k < gn; k++) gc[k] = &m->convs[m->ops[(step > 0 ? i : i - gn + 1) + k].conv];
  return gn;
}

int forward_impl(ys_model* m, int B) {
  hipStream_t st = m->ctx->stream;
  YS_TRY(join_wgrad_stream(m));              // asynchronous segment ends: the previous step's weight-gradient kernels still read activations / dy slots
  YS_TRY(prep_weights(m));
  if (m->training && m->bn_atomic) YS_CHECK_HIP(hipMemsetAsync(m->stat_acc_all, 0, (size_t)m->n_stat_acc * 8, st));   // every unit's statistics accumulators: one clear per forward
  if (m->f8)   // delayed scaling: this pass quantises with the maxima the previous passes recorded (consumed and cleared here)
    YS_TRY(ys_f8_scales_launch(st, m->f8_convs, m->n_f8_convs, m->amax_w, m->amax_act, m->amax_dy, m->f8_scales));
  if (m->f8 && m->f8_bwd_done) m->f8_sg_valid = true;
  if (!m->training && m->eval_coeffs_dirty) {
    for (auto& c : m->convs)
      if (c.bn) YS_TRY(ys_bn_eval_coeffs_launch(st, c.cout, m->params + c.g_off, m->params + c.b_off, m->state + c.rm_off,
                                                m->state + c.rv_off, BN_EPS, chan_ptr(m, c, 0), chan_ptr(m, c, 1)));
    m->eval_coeffs_dirty = false;
  }
  m->q8_fwd_ready = -1;
  const bool e2e_stats = m->e2e && m->training && m->n_hstate > 0;
  if (e2e_stats) {
    long so = 0;
    for (int r = 0; r < m->n_hstate_rng; r++) {
      YS_CHECK_HIP(hipMemcpyAsync(m->hstate_snap + so, m->state + m->hstate_rng[r].off, (size_t)m->hstate_rng[r].count * 4, hipMemcpyDeviceToDevice, st));
      so += m->hstate_rng[r].count;
    }
  }
  for (size_t oi = 0; oi < m->ops.size(); oi++) {
    const Op& op = m->ops[oi];
    const Buf& ib = m->bufs[op.in.buf];
    const Buf& ob = m->bufs[op.out.buf];
    if (op.type == OP_CONV && m->convs[op.conv].group >= 0) {
      // a head stage: the consecutive ops of one group run as grouped launches
      ConvL* gc[YS_GROUP_MAX];
      const int gn = group_run(m, (int)oi, +1, gc);
      YS_TRY(run_conv_fwd_group(m, gc, gn, B));
      oi += gn - 1;
      continue;
    }
    if (op.type == OP_CONV) {
      const ConvL& cc = m->convs[op.conv];
      const ConvL* next = nullptr;               // the very next op, if it is a convolution reading exactly what this one writes
      if (oi + 1 < m->ops.size() && m->ops[oi + 1].type == OP_CONV) {
        const ConvL& nc = m->convs[m->ops[oi + 1].conv];
        if (nc.in.buf == cc.out.buf && nc.in.coff == cc.out.coff && nc.in.C == cc.out.C && nc.cin_pad == cc.cout && nc.cin == cc.cout &&
            nc.Hin == cc.Hout && nc.Win == cc.Wout) next = &nc;
      }
      YS_TRY(run_conv_fwd(m, cc, B, next));
    } else if (int pc[4]; op.type == OP_MAXPOOL && sppf_chain(m, (int)oi, pc)) {
      unsigned char* am[3];
      for (int k = 0; k < 3; k++) am[k] = m->training ? m->argmax + m->ops[oi + k].aux_off : nullptr;
      YS_TRY(ys_sppf_pool3_fwd_launch(st, m->dtype, ib.act, ib.ldc, pc, B, op.H, op.W, op.in.C, am));
      oi += 2;
    } else if (op.type == OP_MAXPOOL) {
      YS_TRY(ys_maxpool5_fwd_launch(st, m->dtype, ib.act, ib.ldc, op.in.coff, B, op.H, op.W, op.in.C, ob.act, ob.ldc,
                                    op.out.coff, m->training ? m->argmax + op.aux_off : nullptr));
    } else if (op.type == OP_UPSAMPLE) {
      YS_TRY(ys_upsample2x_fwd_launch(st, m->dtype, ib.act, ib.ldc, op.in.coff, B, op.H, op.W, op.in.C, ob.act, ob.ldc, op.out.coff));
    } else if (op.type == OP_ATTN) {
      YS_TRY(ys_attn_fwd_launch(st, m->dtype, ib.act, ib.ldc, B, op.H * op.W, op.heads, op.kd, op.hd, ob.act, ob.ldc, m->attn_ws + op.aux_off));
    } else if (op.type == OP_VCOPY) {
      YS_TRY(ys_attn_v_copy_launch(st, m->dtype, ib.act, ob.act, (long)B * op.H * op.W, ib.ldc, op.heads, op.kd, op.hd, ob.ldc, 0));
    } else if (op.type == OP_COPY) {
      YS_TRY(ys_copy_view_launch(st, m->dtype, ib.act, ib.ldc, op.in.coff, (long)B * op.H * op.W, op.in.C, ob.act, ob.ldc, op.out.coff, 0));
    } else if (op.type == OP_POOL) {
      // AdaptiveAvgPool2d(1) + flatten (Head.cs:637): training applies the Conv unit's batch-statistics BN + SiLU to its pre-BN output y on
      // the way; eval averages the map the folded-BN epilogue wrote
      const ConvL& c = m->convs[op.conv];
      const int HW = op.H * op.W;
      if (m->training)
        YS_TRY(ys_cls_pool_fwd_launch(st, m->dtype, y_ptr(m, c), c.cout, 0, HW, B, HW, c.cout, chan_ptr(m, c, 0),
                                      chan_ptr(m, c, 1), c.act ? 1 : 0, ob.act, ob.ldc));
      else
        YS_TRY(ys_cls_pool_fwd_launch(st, m->dtype, ib.act, ib.ldc, op.in.coff, ib.rows_per_b, B, HW, op.in.C, nullptr, nullptr, 0, ob.act, ob.ldc));
    }
  }
  if (!m->training && m->cls)   // Classify eval: inference["cls"] = softmax(logits, 1) (Head.cs:640)
    YS_TRY(ys_cls_xent_launch(st, m->dtype, m->bufs[m->logit_buf].act, m->ld_cls, B, m->d.nc, nullptr, nullptr, m->pred, nullptr, nullptr));
  if (m->f8) m->f8_sx_valid = true;        // every fp8 candidate has recorded an input maximum (bootstrap pass or its own kernel)
  if (e2e_stats) {   // the one2one branch runs the same tower modules again on the same values: their running statistics move twice (e2e.hip)
    long so = 0;
    for (int r = 0; r < m->n_hstate_rng; r++) {
      YS_TRY(ys_e2e_bn_second_update_launch(st, m->state + m->hstate_rng[r].off, m->hstate_snap + so, m->hstate_count + so, m->hstate_rng[r].count, BN_MOMENTUM));
      so += m->hstate_rng[r].count;
    }
  }
  if (!m->training && m->pd_buf >= 0) YS_TRY(eval_tail(m, B));
  YS_CHECK_HIP(hipGetLastError());
  return YS_OK;
}

// The tail of an eval forward of a detection-family model: the head buffers of B images -> `pred` (and, End2End, "det").  forward_impl ends with it;
// ys_model_decode_preds runs it alone on head buffers a caller supplied (ys_model_set_preds)
int eval_tail(ys_model* m, int B) {
  hipStream_t st = m->ctx->stream;
  YS_TRY(ys_detect_decode_launch(st, m->dtype, m->bufs[m->pd_buf].act, m->ld_pd, m->bufs[m->ps_buf].act, m->ld_ps, B, m->A,
                                 m->d.nc, m->d.reg_max, m->nl, m->lvl_off, m->lvl_w, m->lvl_stride, m->pred, 4 + m->d.nc + m->nm,
                                 m->xkind >= 2 ? m->bufs[m->mc_buf].act : nullptr, m->ld_mc, m->xkind, m->nm, m->kdim, m->e2e && m->xkind != 2 ? 1 : 0));
  if (m->segment)   // Segment._inference: cat(preds, mask_coefficient) (Head.cs:309-313), raw coefficients
    YS_TRY(ys_unpack_nchw_strided_launch(st, m->dtype, m->bufs[m->mc_buf].act, m->ld_mc, 0, B, m->nm, m->A, m->pred,
                                         (long)(4 + m->d.nc + m->nm) * m->A, (long)(4 + m->d.nc) * m->A));
  if (m->e2e)   // Detect.postprocess on the one2one branch (same values as the one2many branch): [B][k][6] (Head.cs:107-127).  Segment.postprocess (Head.cs:321-339):
                // the same selection, the nm coefficients gathered by the same anchor index: [B][k][6 + nm]; Obb.postprocess (Head.cs:439-452): the angle channel
                // rides the same way, rows (cx, cy, w, h, score, class, angle); Pose.postprocess (Head.cs:550-563): the nk decoded keypoint values, rows
                // (x1, y1, x2, y2, score, class, keypoints) -- the decode above wrote xyxy (Detect.decode_bboxes, Head.cs:201).  A Detect model has nm = 0
    YS_TRY(ys_e2e_topk_launch(st, m->pred, B, m->d.nc, m->A, m->max_det, m->det_ws, m->det_rows, m->det_anchor, m->nm));
  return YS_OK;
}

// ------------------------------------------------------------------ backward
// returns 0 = first writer (overwrite), 1 = accumulate; -1 = inconsistent slice state
static int grad_mode(ys_model* m, const View& v) {
  Buf& b = m->bufs[v.buf];
  int nw = 0;
  for (int c = v.coff; c < v.coff + v.C; c++) nw += b.gw[c] ? 1 : 0;
  if (nw != 0 && nw != v.C) return -1;
  for (int c = v.coff; c < v.coff + v.C; c++) b.gw[c] = 1;
  return nw ? 1 : 0;
}
// grad_mode into *mode, or the error every writer reports: "backward: inconsistent <what> state at <where>"
static int claim_grad(ys_model* m, const View& v, int* mode, const std::string& where, const char* what = "gradient slice") {
  *mode = grad_mode(m, v);
  if (*mode < 0) { ys_set_error("backward: inconsistent %s state at %s", what, where.c_str()); return YS_ERR_STATE; }
  return YS_OK;
}
// End2End, one2one pass: the branch reads x.detach() (Head.cs:94) -- a unit that reads a feature map gets parameter gradients only
static bool reads_detached_map(const ys_model* m, const ConvL& c) {
  return m->e2e_pass && (c.in.buf == m->det_in[0] || c.in.buf == m->det_in[1] || c.in.buf == m->det_in[2]);
}

// input-gradient convolution of layer c (gather form with flipped / transposed weights) reading dy as a [M][dy_ldc] view
ConvArgs dgrad_args(ys_model* m, const ConvL& c, int B, const void* dy, int dy_ldc, int dy_coff, long dy_bstride) {
  const Buf& ib = m->bufs[c.in.buf];
  ConvArgs a{};
  a.x = dy; a.w = (char*)m->wd_all + (size_t)c.wd_off * m->es;
  a.y = ib.grad;
  a.B = B; a.Hin = c.Hout; a.Win = c.Wout; a.Cin = c.cout_ld; a.Hout = c.Hin; a.Wout = c.Win; a.Cout = c.cin_pad; a.KH = a.KW = c.k;
  a.SA = 1; a.DIVS = c.s == 2 ? 1 : 0; a.DIVM = c.s - 1; a.PAD = c.k - 1 - c.pad;
  a.in_ldc = dy_ldc; a.in_coff = dy_coff; a.in_bstride = dy_bstride;
  a.out_ldc = ib.ldc; a.out_coff = c.in.coff; a.out_bstride = ib.rows_per_b;
  a.vec_ok = (ib.ldc % 4 == 0 && c.in.coff % 4 == 0) ? 1 : 0;
  a.M = B * c.Hin * c.Win;
  return a;
}
void f8_dgrad_operands(const ys_model* m, const ConvL& c, ConvArgs& a) {
  a.f8 = 2; a.w8 = m->wd8_all + c.wd_off; a.qscale = m->f8_scales + 4L * c.idx + 2; a.deq = m->f8_scales + 4L * c.idx + 3;
}

// weight gradient of one convolution on stream `sw` (split partials into the layer's own region when the reduction is deferred)
static int launch_wgrad(ys_model* m, ConvL& c, int B, const void* dy, int dy_ldc, int dy_coff, long dy_bstride, hipStream_t sw, bool bnb = false) {
  WgradArgs a = wgrad_args(m, c, B, dy_ldc, dy_coff, dy_bstride);
  a.x = m->bufs[c.in.buf].act; a.dy = dy; a.partial = m->wg_partial;
  int splits = ys_wgrad_splits(a, m->dtype);
  const bool defer = c.wgp_off >= 0;
  const bool stem = c.first && m->in_f32 && defer;     // model.0: x is the fp32 image itself (conv_stem.hip); slabs in the generic split layout
  int used = 0;
  if (stem) {
    // bnb: dy is the gradient of the unit's output and the kernel runs the BatchNorm backward itself (run_conv_bwd: stem_fused)
    const StemBnb sb{y_ptr(m, c), chan_ptr(m, c, 0), chan_ptr(m, c, 1), chan_ptr(m, c, 4), chan_ptr(m, c, 5), c.act ? 1 : 0};
    a.partial = m->wg_partial + c.wgp_off;
    if (c.k == 6) {          // Yolov5u's 6x6 stem (conv_stem6.hip) has no fused form: stem_bnb_planned answers false for it
      if (bnb) { ys_set_error("backward: %s was queued without its dy", c.name.c_str()); return YS_ERR_STATE; }
      YS_TRY(ys_stem6_wgrad_launch(sw, m->in_f32, B, c.Hin, c.Win, dy, dy_ldc, dy_coff, dy_bstride, c.cout, a.partial, c.wgp_splits, &used));
    } else
    YS_TRY(ys_stem_wgrad_launch(sw, m->in_f32, B, c.Hin, c.Win, dy, dy_ldc, dy_coff, dy_bstride, c.cout, a.partial, c.wgp_splits, &used,
                                bnb ? &sb : nullptr));
  } else {
    if (bnb) { ys_set_error("backward: %s was queued without its dy", c.name.c_str()); return YS_ERR_STATE; }
    if (defer) { a.partial = m->wg_partial + c.wgp_off; if (splits > c.wgp_splits) splits = c.wgp_splits; }   // own region (sized at max_batch)
    else if ((long)splits * c.cout * c.k * c.k * c.cin_pad > m->n_wgp) { ys_set_error("wgrad workspace too small"); return YS_ERR_STATE; }
    YS_TRY(ys_wgrad_launch(sw, m->dtype, a, splits, c.cin, m->grads + c.w_off, defer ? &used : nullptr));
  }
  if (defer) {   // what the batched split reduction of the segment will read (backward_range: reduce_range)
    WgRedDesc& d = m->red_host[c.red_slot];
    d.partial = a.partial; d.grad = m->grads + c.w_off; d.n = (long)c.cout * c.k * c.k * c.cin_pad; d.splits = used;
    d.cin_pad = c.cin_pad; d.cin_real = c.cin;
    YS_REQUIRE((c.cin_pad & 3) == 0, "wgrad reduce: input channel pitch must be a multiple of 4");
  }
  return YS_OK;
}

// Hand the queued weight-gradient launches to the second stream behind ONE event (everything they read -- their units' dy, written by bn_bwd_apply launches
// already issued on the main stream -- is complete there once the event fires).  Without the second stream nothing is ever queued.
static int flush_wgrads(ys_model* m, int B) {
  if (m->pend_wg.empty()) return YS_OK;
  hipStream_t sw = m->ctx->stream;
  if (m->overlap) {
    hipEvent_t ev = m->ev_hand[m->hand_next];
    m->hand_next = (m->hand_next + 1) % (ys_model::N_HAND + 1);
    YS_CHECK_HIP(hipEventRecord(ev, m->ctx->stream));
    YS_CHECK_HIP(hipStreamWaitEvent(m->st2, ev, 0));
    sw = m->st2;
    m->st2_dirty = true;
  }
  for (const auto& p : m->pend_wg) YS_TRY(launch_wgrad(m, m->convs[p.conv], B, p.dy, p.ldc, p.coff, p.bstride, sw, p.bnb));
  m->pend_wg.clear(); m->pend_mb = 0.0;
  return YS_OK;
}
// queue layer c's weight gradient; flush when the batch is full: 6 launches or 40 megabytes of (input + dy) tensors (
// the P1 / P2 / P3 layers, whose kernels run 50-150 us, go over one or two at a time -- the bubble is small next to them and the second stream should not start
// them late; the P4 / P5 layers, 15-30 us each, go over in fours to sixes)
static int queue_wgrad(ys_model* m, ConvL& c, int B, const void* dy, int ldc, int coff, long bstride, bool bnb = false) {
  if (!m->overlap) return launch_wgrad(m, c, B, dy, ldc, coff, bstride, m->ctx->stream, bnb);
  if (c.first && m->hold_stem) {               // everything queued so far goes now; the stem's own launch waits for the segment end
    YS_TRY(flush_wgrads(m, B));
    m->pend_wg.push_back(ys_model::PendWg{c.idx, dy, ldc, coff, bstride, bnb});
    return YS_OK;
  }
  m->pend_wg.push_back(ys_model::PendWg{c.idx, dy, ldc, coff, bstride, bnb});
  m->pend_mb += ((double)B * c.Hout * c.Wout * c.cout + (double)B * c.Hin * c.Win * c.cin_pad) * m->es * 1e-6;
  // (measured on config 2, same box, two rounds each: one per launch 8.71 / 8.71 ms, 4 / 24 MB 8.74 / 8.72, 6 / 40 MB 8.65 / 8.66, 12 / 80 MB 8.81 / 8.75, 8 / 200 MB 8.84 / 8.81,
  // everything in one batch per segment 8.93 / 8.87; round 5's ring + per-launch events 8.79 / 8.73)
  if (m->pend_wg.size() >= 6 || m->pend_mb >= 40.0) return flush_wgrads(m, B);
  return YS_OK;
}

static int run_convT_bwd(ys_model* m, const ConvL& c, int B) {
  hipStream_t st = m->ctx->stream;
  YS_TRY(flush_wgrads(m, B));            // queued weight gradients go first: this path drains the second stream and then uses the shared workspace
  if (m->overlap && m->st2_dirty) {      // this path uses the shared wgrad workspace on `st`: drain the weight-gradient stream first
    YS_CHECK_HIP(hipEventRecord(m->ev_join, m->st2));
    YS_CHECK_HIP(hipStreamWaitEvent(st, m->ev_join, 0));
    m->st2_dirty = false;
  }
  const Buf& ib = m->bufs[c.in.buf];
  const Buf& ob = m->bufs[c.out.buf];
  const long Mup = (long)B * c.Hout * c.Wout;
  YS_TRY(ys_colsum_launch(st, m->dtype, ob.grad, ob.ldc, c.out.coff, Mup, Mup, Mup, c.cout, m->stat_partial, m->grads + c.g_off));
  int mode0 = 0;
  YS_TRY(claim_grad(m, c.in, &mode0, c.name));
  for (int ph = 0; ph < 4; ph++) {
    const int dh = ph >> 1, dw = ph & 1;
    WgradArgs wa = wgrad_args(m, c, B, ob.ldc, c.out.coff, ob.rows_per_b, ph);
    wa.x = ib.act; wa.dy = ob.grad; wa.partial = m->wg_partial;
    const int splits = ys_wgrad_splits(wa, m->dtype);
    if ((long)splits * c.cout * c.cin_pad > m->n_wgp) { ys_set_error("wgrad workspace too small"); return YS_ERR_STATE; }
    YS_TRY(ys_wgrad_launch(st, m->dtype, wa, splits, c.cin, m->grads + c.w_off + (long)ph * c.cout * c.cin));
    // dx[h,w] (+)= W[dh,dw]^T dy[2h+dh, 2w+dw]: 1x1 gather with stride 2 and offsets (dh, dw)
    ConvArgs a{};
    a.x = ob.grad; a.w = (char*)m->wd_all + (size_t)(c.wd_off + (long)ph * c.cin * c.cout_ld) * m->es; a.y = ib.grad;
    a.B = B; a.Hin = c.Hout; a.Win = c.Wout; a.Cin = c.cout_ld; a.Hout = c.Hin; a.Wout = c.Win; a.Cout = c.cin; a.KH = a.KW = 1;
    a.SA = 2; a.PAD = -dh; a.pad_w_delta = dh - dw;
    a.in_ldc = ob.ldc; a.in_coff = c.out.coff; a.in_bstride = ob.rows_per_b;
    a.out_ldc = ib.ldc; a.out_coff = c.in.coff; a.out_bstride = ib.rows_per_b;
    a.vec_ok = (ib.ldc % 4 == 0 && c.in.coff % 4 == 0) ? 1 : 0;
    a.accumulate = (ph == 0) ? mode0 : 1;
    a.M = B * c.Hin * c.Win;
    YS_TRY(ys_conv_launch(st, m->dtype, a));
  }
  if (m->overlap) {                      // later weight-gradient launches must not overtake this layer's use of the workspace
    YS_CHECK_HIP(hipEventRecord(m->ev_hand[ys_model::N_HAND], st));
    YS_CHECK_HIP(hipStreamWaitEvent(m->st2, m->ev_hand[ys_model::N_HAND], 0));
  }
  return YS_OK;
}

// the BN-backward segments of the producers whose dz this dgrad launch completes (c.feeds) -> a.red[]; `rows` = partial rows it will write
static void attach_bnred_feeds(ys_model* m, ConvL& c, ConvArgs& a, int rows) {
  a.nred = (int)c.feeds.size(); a.red_row0 = 0;
  for (int k = 0; k < a.nred; k++) {
    ConvL::RedFeed& f = c.feeds[k];
    ConvL& l = m->convs[f.prod];
    BnRedSeg& sg = a.red[k];
    sg.y = y_ptr(m, l); sg.scale = chan_ptr(m, l, 0); sg.shift = chan_ptr(m, l, 1);
    sg.part = m->bnred_part + f.part_off; sg.c0 = f.c0; sg.c1 = f.c1; sg.yc0 = f.yc0; sg.C = l.cout; sg.act = l.act ? 1 : 0;
    f.rows = rows;
    l.red_seen++;
  }
}
// ... when the rows that launch will write fit every feed's planned capacity (else its producers run their own reduction pass)
static void attach_bnred_feeds_if_fit(ys_model* m, ConvL& c, ConvArgs& a) {
  a.nred = 0;
  if (c.feeds.empty()) return;
  const int rows = ys_conv_bnred_rows(a, m->dtype);
  bool fits = rows > 0;
  for (auto& f : c.feeds) fits = fits && rows <= f.rows_cap;
  if (fits) attach_bnred_feeds(m, c, a, rows);
}
// producer side: every source of unit c's BN-backward sums was attached in this backward pass / where they lie
static bool bnred_ready(const ConvL& c) { return c.red_ok && c.red_seen == (int)c.red_src.size() && !c.red_src.empty(); }
static FinSrc bnred_src(const ys_model* m, const ConvL& c) {
  FinSrc src{};
  src.n = (int)c.red_src.size();
  for (int k = 0; k < src.n; k++) {
    const ConvL::RedFeed& f = m->convs[c.red_src[k].cons].feeds[c.red_src[k].feed];
    src.p[k] = m->bnred_part + f.part_off; src.nblk[k] = f.rows; src.c1[k] = f.yc0 + (f.c1 - f.c0);
  }
  return src;
}
// BN-backward finalize of unit c over `count` rows: dgamma / dbeta into the gradients, the apply pass's coefficients c1 / c2 into its scratch rows
static ChanFinProb bn_bwd_fin(ys_model* m, const ConvL& c, const FinSrc& src, long count) {
  return ChanFinProb{src, c.cout, (double)count, m->grads + c.g_off, m->grads + c.b_off, chan_ptr(m, c, 4), chan_ptr(m, c, 5), chan_ptr(m, c, 0), chan_ptr(m, c, 2), chan_ptr(m, c, 3)};
}
static int bn_bwd_finalize(ys_model* m, const ConvL& c, int nblk, long count) {     // sums from nblk rows of stat_partial
  const ChanFinProb p = bn_bwd_fin(m, c, FinSrc{}, count);
  return ys_bn_bwd_finalize_launch(m->ctx->stream, m->stat_partial, nblk, c.cout, count, p.g0, p.g1, p.c1, p.c2, p.scale, p.mean, p.rstd);
}

static int run_conv_bwd(ys_model* m, ConvL& c, int B) {
  if (c.ct) return run_convT_bwd(m, c, B);
  hipStream_t st = m->ctx->stream;
  const Buf& ib = m->bufs[c.in.buf];
  const Buf& ob = m->bufs[c.out.buf];
  const long M = (long)B * c.Hout * c.Wout;
  const void* dy = nullptr; int dy_ldc = 0, dy_coff = 0; long dy_bstride = (long)c.Hout * c.Wout;
  bool dy_q8 = false;                       // m->q8 already holds the e5m2 image of dy (written by the BN backward pass)
  bool stem_scratch = false;                // model.0 planned for the fused form in a step that cannot take it: its dy sits in dy_scratch
  bool stem_fused = false;                  // dy is not materialised: the stem's weight-gradient kernel forms it from dz and y
  if (c.bn) {
    const void* y = y_ptr(m, c);
    void* rg = nullptr; int rgl = 0, rgc = 0;
    if (c.has_res) {
      // d(residual input) += dz.  First contribution to that view: plain copy; later ones accumulate inside the reduce pass.
      Buf& rb = m->bufs[c.res.buf];
      int rmode = 0;
      YS_TRY(claim_grad(m, c.res, &rmode, c.name, "residual gradient"));
      if (rmode == 0) {
        YS_TRY(ys_copy_view_launch(st, m->dtype, ob.grad, ob.ldc, c.out.coff, M, c.cout, rb.grad, rb.ldc, c.res.coff, 0));
      } else {
        rg = rb.grad; rgl = rb.ldc; rgc = c.res.coff;
      }
    }
    // sum(du), sum(du * y): from the epilogues of the dgrad launches that completed dz (fused BN-backward reduction), else a pass of its own
    const bool fused = bnred_ready(c);
    if (c.pool_next) {   // Classify: dz = dpooled / HW (OP_POOL) is never materialised -- reduction and apply read the pooled gradient
      const Buf& pb = m->bufs[m->pool_buf];
      const int HW = c.Hout * c.Wout;
      if ((long)B * 2 * c.cout > m->n_stat) { ys_set_error("backward: batch %d too large for the Classify statistics rows", B); return YS_ERR_STATE; }
      YS_TRY(ys_cls_bn_bwd_reduce_launch(st, m->dtype, pb.grad, pb.ldc, y, B, HW, c.cout, chan_ptr(m, c, 0), chan_ptr(m, c, 1), c.act ? 1 : 0,
                                         m->stat_partial));
      YS_TRY(bn_bwd_finalize(m, c, B, M));
      void* dyb = (m->overlap && c.dy_own) ? c.dy_own : m->dy_scratch;
      YS_TRY(ys_cls_bn_bwd_apply_launch(st, m->dtype, pb.grad, pb.ldc, y, B, HW, c.cout, chan_ptr(m, c, 0), chan_ptr(m, c, 1), chan_ptr(m, c, 4),
                                        chan_ptr(m, c, 5), c.act ? 1 : 0, dyb));
      dy = dyb; dy_ldc = c.cout; dy_coff = 0;
    } else {
    c.red_seen = 0;
    void* rg_apply = nullptr;                    // the shortcut's residual-gradient accumulation rides on the reduction pass; without one, on the apply pass
    if (fused) {
      const ChanFinProb p = bn_bwd_fin(m, c, bnred_src(m, c), M);
      YS_TRY(ys_bn_bwd_finalize_src_launch(st, p.src, c.cout, M, p.g0, p.g1, p.c1, p.c2, p.scale, p.mean, p.rstd));
      rg_apply = rg;
    } else {
      int nblk = 0;
      YS_TRY(ys_bn_bwd_reduce_launch(st, m->dtype, ob.grad, ob.ldc, c.out.coff, y, M, c.cout, chan_ptr(m, c, 0), chan_ptr(m, c, 1),
                                     chan_ptr(m, c, 2), chan_ptr(m, c, 3), c.act ? 1 : 0, rg, rgl, rgc, m->stat_partial, &nblk));
      YS_TRY(bn_bwd_finalize(m, c, nblk, M));
    }
    // model.0 read from the fp32 image: no apply pass -- its weight-gradient kernel takes dz, y and the coefficient rows the finalize above just wrote
    stem_fused = c.idx == 0 && m->in_f32 && c.wgp_off >= 0 && stem_bnb_planned(m);
    // planned fused (no dy buffer of its own), but this step's forward packed its input (ys_model_forward_u8): dy goes to the shared scratch buffer.  model.0 is the
    // last unit of the backward, nothing writes that buffer after it, and the next backward joins the second stream before it starts (ys_model_backward).
    stem_scratch = !stem_fused && m->overlap && c.idx == 0 && !c.dy_own && !c.dw && stem_bnb_planned(m);
    void* dyb = m->dy_scratch;
    if (m->overlap && !c.dw && c.dy_own) dyb = c.dy_own;   // the unit's own buffer: its weight gradient reads it later, from the second stream (queue_wgrad)
    // fp8 mode: when this layer's dgrad will run the fp8 blocked-GEMM kernel, the same pass writes the e5m2 image of dy it consumes
    // (and records amax(|dy|)) -- no separate quantisation pass over dy
    if (m->f8 && c.f8_bwd && m->f8_sg_valid && !c.first && !c.dw && m->q8 && m->dtype == YS_BF16 && c.cout_ld == c.cout) {
      ConvArgs q = dgrad_args(m, c, B, dyb, c.cout, 0, (long)c.Hout * c.Wout);
      f8_dgrad_operands(m, c, q);
      dy_q8 = ys_conv_wants_x8(q);
    }
    if (stem_fused) {
      if (rg_apply || dy_q8) { ys_set_error("backward: %s cannot take the fused BatchNorm backward", c.name.c_str()); return YS_ERR_STATE; }
    } else if (dy_q8) {
      YS_TRY(ys_bn_bwd_apply_q8_launch(st, ob.grad, ob.ldc, c.out.coff, y, M, c.cout, chan_ptr(m, c, 0), chan_ptr(m, c, 1), chan_ptr(m, c, 4),
                                       chan_ptr(m, c, 5), c.act ? 1 : 0, dyb, m->q8, m->f8_scales + 4L * c.idx + 2,
                                       m->amax_dy + (size_t)c.idx * YS_AMAX_WAYS, rg_apply, rgl, rgc));
    } else {
      YS_TRY(ys_bn_bwd_apply_launch(st, m->dtype, ob.grad, ob.ldc, c.out.coff, y, M, c.cout, chan_ptr(m, c, 0), chan_ptr(m, c, 1),
                                    chan_ptr(m, c, 4), chan_ptr(m, c, 5), c.act ? 1 : 0, dyb, nullptr, rg_apply, rgl, rgc));
    }
    dy = dyb; dy_ldc = c.cout; dy_coff = 0;
    if (stem_fused) { dy = ob.grad; dy_ldc = ob.ldc; dy_coff = c.out.coff; }
    }
  } else {
    // plain Conv2d with bias (head outputs): dy is the loss gradient itself
    dy = view_ptr(m, ob.grad, ob, c.out_rowoff); dy_ldc = ob.ldc; dy_coff = c.out.coff; dy_bstride = ob.rows_per_b;
    YS_TRY(ys_colsum_launch(st, m->dtype, dy, dy_ldc, dy_coff, M, (long)c.Hout * c.Wout, dy_bstride, c.cout, m->stat_partial,
                            m->grads + c.g_off));
  }
  const bool no_dx = reads_detached_map(m, c);
  if (c.dw) {
    YS_TRY(ys_dwconv_wgrad_launch(st, m->dtype, ib.act, ib.ldc, c.in.coff, dy, B, c.Hin, c.Win, c.cout, m->stat_partial, m->grads + c.w_off));
    if (no_dx) return YS_OK;
    int mode = 0;
    YS_TRY(claim_grad(m, c.in, &mode, c.name));
    YS_TRY(ys_dwconv_launch(st, m->dtype, 1, dy, c.cout, 0, B, c.Hin, c.Win, c.cout, m->params + c.w_off, ib.grad, ib.ldc, c.in.coff, mode));
    return YS_OK;
  }
  // ---- wgrad: queued for the second stream (issued at once without it)
  if (c.bn && m->overlap && dy != c.dy_own && !stem_fused && !stem_scratch) { ys_set_error("backward: %s has no dy buffer of its own", c.name.c_str()); return YS_ERR_STATE; }
  YS_TRY(queue_wgrad(m, c, B, dy, dy_ldc, dy_coff, dy_bstride, stem_fused));
  // ---- dgrad (gather form with flipped/transposed weights)
  if (!c.first && !no_dx) {
    ConvArgs a = dgrad_args(m, c, B, dy, dy_ldc, dy_coff, dy_bstride);
    YS_TRY(claim_grad(m, c.in, &a.accumulate, c.name));
    if (m->f8 && c.f8_bwd) {
      unsigned* slots = m->amax_dy + (size_t)c.idx * YS_AMAX_WAYS;
      if (m->f8_sg_valid) {   // dgrad with the gradient quantised to e5m2 and the e4m3 dgrad weights; records amax(|dy|) itself
        f8_dgrad_operands(m, c, a); a.amax = slots;
        a.q8 = m->q8;
        if (dy_q8) { a.x8 = m->q8; a.amax = nullptr; }     // image and maximum already produced by the BN backward pass
      } else {
        YS_TRY(ys_f8_view_amax_launch(st, dy, M, c.cout, dy_ldc, dy_coff, slots));
      }
    }
    if (c.bn && c.cout_ld != c.cout) { ys_set_error("backward: padded BN conv unsupported"); return YS_ERR_UNSUPPORTED; }
    attach_bnred_feeds_if_fit(m, c, a);   // this launch completes dz of the producers in c.feeds: its epilogue takes their BN-backward sums (BnRedSeg)
    YS_TRY(ys_conv_launch(st, m->dtype, a));
  }
  return YS_OK;
}

// ---- grouped backward of one head stage (mirror of run_conv_fwd_group): BN backward finalize + apply as one launch each, the weight
// gradients handed to the weight-gradient stream behind ONE event, the input gradients as one grouped dgrad launch when the problems
// share a kernel variant.  Falls back to run_conv_bwd per unit whenever a unit needs something the grouped form does not carry.
static int run_conv_bwd_group(ys_model* m, ConvL* const* cs, int n, int B) {
  hipStream_t st = m->ctx->stream;
  bool ok = n >= 2 && n <= YS_GROUP_MAX && !m->f8;
  for (int i = 0; i < n && ok; i++) {
    const ConvL& c = *cs[i];
    if (reads_detached_map(m, c)) { ok = false; break; }   // one2one pass: no input gradient (run_conv_bwd)
    ok = !c.dw && !c.ct && !c.has_res && !c.first && c.gstat_off >= 0 && c.bn == cs[0]->bn && c.act == cs[0]->act && (!c.bn || (c.dy_own && c.cout_ld == c.cout));
    if (ok && c.bn) ok = bnred_ready(c);   // sums already produced by the consumers' dgrads
  }
  if (!ok) { for (int i = 0; i < n; i++) YS_TRY(run_conv_bwd(m, *cs[i], B)); return YS_OK; }
  const void* dy[YS_GROUP_MAX]; int dy_ldc[YS_GROUP_MAX], dy_coff[YS_GROUP_MAX]; long dy_bs[YS_GROUP_MAX];
  if (cs[0]->bn) {
    ChanFinProb fp[YS_GROUP_MAX];
    BnBwdProb bp[YS_GROUP_MAX];
    for (int i = 0; i < n; i++) {
      ConvL& c = *cs[i];
      const Buf& ob = m->bufs[c.out.buf];
      const long M = (long)B * c.Hout * c.Wout;
      fp[i] = bn_bwd_fin(m, c, bnred_src(m, c), M);
      c.red_seen = 0;
      bp[i] = BnBwdProb{ob.grad, ob.ldc, c.out.coff, y_ptr(m, c), M, c.cout, chan_ptr(m, c, 0), chan_ptr(m, c, 1), chan_ptr(m, c, 4), chan_ptr(m, c, 5), c.dy_own, nullptr, 0, 0};
      dy[i] = c.dy_own; dy_ldc[i] = c.cout; dy_coff[i] = 0; dy_bs[i] = (long)c.Hout * c.Wout;
    }
    YS_TRY(ys_bn_bwd_finalize_group_launch(st, fp, n));
    YS_TRY(ys_bn_bwd_apply_group_launch(st, m->dtype, bp, n, cs[0]->act ? 1 : 0));
  } else {
    for (int i = 0; i < n; i++) {
      ConvL& c = *cs[i];
      const Buf& ob = m->bufs[c.out.buf];
      const long M = (long)B * c.Hout * c.Wout;
      dy[i] = view_ptr(m, ob.grad, ob, c.out_rowoff); dy_ldc[i] = ob.ldc; dy_coff[i] = c.out.coff; dy_bs[i] = ob.rows_per_b;
      YS_TRY(ys_colsum_launch(st, m->dtype, dy[i], dy_ldc[i], dy_coff[i], M, (long)c.Hout * c.Wout, dy_bs[i], c.cout, m->stat_partial, m->grads + c.g_off));
    }
  }
  // ---- weight gradients: every dy of the stage is complete on `st` here -- queued, and handed over together
  for (int i = 0; i < n; i++) YS_TRY(queue_wgrad(m, *cs[i], B, dy[i], dy_ldc[i], dy_coff[i], dy_bs[i]));
  YS_TRY(flush_wgrads(m, B));
  // ---- input gradients
  ConvArgs a[YS_GROUP_MAX];
  int cap[YS_GROUP_MAX] = {0, 0, 0}, rows[YS_GROUP_MAX] = {0, 0, 0};
  for (int i = 0; i < n; i++) {
    ConvL& c = *cs[i];
    a[i] = dgrad_args(m, c, B, dy[i], dy_ldc[i], dy_coff[i], dy_bs[i]);
    YS_TRY(claim_grad(m, c.in, &a[i].accumulate, c.name));
    for (auto& f : c.feeds) cap[i] = cap[i] ? std::min(cap[i], f.rows_cap) : f.rows_cap;
    if (!c.feeds.empty()) { a[i].nred = (int)c.feeds.size(); }   // (segments are attached once the row counts are known)
  }
  // a grouped launch needs the segment tables before it starts and its row counts are only known after planning: plan first (dry run)
  int rc = m->dtype == YS_BF16 ? ys_conv_p2_group_launch(st, a, n, cap, rows, true) : YS_ERR_UNSUPPORTED;
  if (rc == YS_OK) {
    for (int i = 0; i < n; i++) { a[i].nred = 0; if (!cs[i]->feeds.empty()) attach_bnred_feeds(m, *cs[i], a[i], rows[i]); }
    YS_TRY(ys_conv_p2_group_launch(st, a, n, cap, rows));
  } else if (rc == YS_ERR_UNSUPPORTED) {
    for (int i = 0; i < n; i++) { attach_bnred_feeds_if_fit(m, *cs[i], a[i]); YS_TRY(ys_conv_launch(st, m->dtype, a[i])); }
  } else return rc;
  return YS_OK;
}

// the weight-gradient stream has work the main stream has not waited for: order the main stream behind it
int join_wgrad_stream(ys_model* m) {
  if (m->st2 && m->st2_dirty) {
    YS_CHECK_HIP(hipEventRecord(m->ev_join, m->st2));
    YS_CHECK_HIP(hipStreamWaitEvent(m->ctx->stream, m->ev_join, 0));
    m->st2_dirty = false;
  }
  return YS_OK;
}

// async_end: leave the weight-gradient stream unjoined (its split reduction runs there too) and record the segment's completion events
int backward_range(ys_model* m, int seg_lo, int seg_hi, bool async_end, bool seg_events) {
  hipStream_t st = m->ctx->stream;
  const int B = m->B;
  YS_TRY(plan_bnred(m, B));
  if (m->e2e && seg_lo == 0 && !m->e2e_pass) {
    // End2End (Head.cs:89-106): the towers ran twice on the same values with the same parameters -- on x (one2many) and on x.detach()
    // (one2one).  Backprop is linear in the upstream gradient, so two passes through the towers with the SAME saved activations give
    // the sum: this pass carries the one2one gradients (parameter gradients and the inner input gradients, nothing into the feature
    // maps), the regular pass below the one2many gradients.  The head's split partials are reduced and the weight-gradient stream is
    // joined in between: the second pass reuses every dy buffer and partial region.
    auto swap_o2o_grads = [&]() {
      std::swap(m->bufs[m->pd_buf].grad, m->o2o_dpd); std::swap(m->bufs[m->ps_buf].grad, m->o2o_dps);
      if (m->o2o_dmc) std::swap(m->bufs[m->mc_buf].grad, m->o2o_dmc);   // cv4 is aliased too (Segment, Head.cs:245-357: Proto ran once and gets no one2one gradient; Obb, Head.cs:454-469: the angle logits; Pose, Head.cs:565-580: the raw keypoints, padded channels included)
    };
    swap_o2o_grads();
    m->e2e_pass = true;
    const int rc = backward_range(m, 0, 0, false, false);
    m->e2e_pass = false;
    swap_o2o_grads();
    YS_TRY(rc);
    reset_grad_state(m);
  }
  for (int i = (int)m->ops.size() - 1; i >= 0; i--) {
    const Op& op = m->ops[i];
    if (op.seg < seg_lo || op.seg > seg_hi) continue;
    if (m->e2e_pass && op.type == OP_CONV && m->convs[op.conv].proto) continue;   // one2one["proto"] = proto.detach() (Head.cs:297)
    if (op.type == OP_CONV && m->convs[op.conv].group >= 0) {
      ConvL* gc[YS_GROUP_MAX];
      const int gn = group_run(m, i, -1, gc);
      YS_TRY(run_conv_bwd_group(m, gc, gn, B));
      i -= gn - 1;
    } else if (op.type == OP_CONV) {
      YS_TRY(run_conv_bwd(m, m->convs[op.conv], B));
    } else if (op.type == OP_ATTN) {
      // d(qkv) = [dq | dk | dv]; the v part already holds the gradient that arrived through pe(v) (OP_VCOPY backward)
      const Buf& ib = m->bufs[op.in.buf];
      const Buf& ob = m->bufs[op.out.buf];
      const long nn = (long)B * op.heads * (long)(op.H * op.W) * (op.H * op.W);
      YS_TRY(ys_attn_bwd_launch(st, m->dtype, ib.act, ib.ldc, B, op.H * op.W, op.heads, op.kd, op.hd, ob.grad, ob.ldc,
                                m->attn_ws + op.aux_off, m->attn_ws + op.aux_off + nn, ib.grad));
      Buf& qb = m->bufs[op.in.buf];
      std::fill(qb.gw.begin(), qb.gw.end(), 1);
    } else if (op.type == OP_VCOPY) {
      const Buf& ib = m->bufs[op.in.buf];
      const Buf& ob = m->bufs[op.out.buf];
      YS_TRY(ys_attn_v_copy_launch(st, m->dtype, ob.grad, ib.grad, (long)B * op.H * op.W, ib.ldc, op.heads, op.kd, op.hd, ob.ldc, 1));
    } else if (op.type == OP_COPY) {
      const Buf& ib = m->bufs[op.in.buf];
      const Buf& ob = m->bufs[op.out.buf];
      int mode = 0;
      YS_TRY(claim_grad(m, op.in, &mode, "op " + std::to_string(i)));
      YS_TRY(ys_copy_view_launch(st, m->dtype, ob.grad, ob.ldc, op.out.coff, (long)B * op.H * op.W, op.in.C, ib.grad, ib.ldc, op.in.coff, mode));
    } else if (op.type == OP_POOL) {
      // nothing to launch: the Classify Conv unit's BN / SiLU backward (run_conv_bwd, pool_next) reads dpooled itself
      if (grad_mode(m, op.in) != 0) { ys_set_error("backward: the Classify map has a second gradient writer (op %d)", i); return YS_ERR_STATE; }
    } else if (int pc[4]; op.type == OP_MAXPOOL && sppf_chain(m, i - 2, pc)) {
      // the three pools' backward in one launch; the slice states move as the three launches would move them (pool 2's input first)
      unsigned char* am[3]; int mode[3];
      for (int k = 2; k >= 0; k--) {
        am[k] = m->argmax + m->ops[i - 2 + k].aux_off;
        YS_TRY(claim_grad(m, m->ops[i - 2 + k].in, &mode[k], "op " + std::to_string(i - 2 + k)));
      }
      const Buf& gb = m->bufs[op.in.buf];
      YS_TRY(ys_sppf_pool3_bwd_launch(st, m->dtype, gb.grad, gb.ldc, pc, B, op.H, op.W, op.in.C, am, mode));
      i -= 2;
    } else {
      const Buf& ib = m->bufs[op.in.buf];
      const Buf& ob = m->bufs[op.out.buf];
      int mode = 0;
      YS_TRY(claim_grad(m, op.in, &mode, "op " + std::to_string(i)));
      if (op.type == OP_MAXPOOL)
        YS_TRY(ys_maxpool5_bwd_launch(st, m->dtype, ob.grad, ob.ldc, op.out.coff, B, op.H, op.W, op.in.C, m->argmax + op.aux_off,
                                      ib.grad, ib.ldc, op.in.coff, mode));
      else
        YS_TRY(ys_upsample2x_bwd_launch(st, m->dtype, ob.grad, ob.ldc, op.out.coff, B, op.H, op.W, op.in.C, ib.grad, ib.ldc,
                                        op.in.coff, mode));
    }
  }
  // the segment's gradients are complete only when the weight-gradient stream has drained: the main stream waits for it here, unless the
  // caller asked for an asynchronous end -- then the split reduction below goes to that stream as well, nothing on the main stream waits,
  // and whoever consumes the segment's gradients (the all-reduce) waits on the two events recorded at the end
  // split reduction of weight gradients [lo, hi) of the descriptor table in one launch on stream sr (the partial slabs sit in per-layer regions)
  auto reduce_range = [&](int lo, int hi, hipStream_t sr) -> int {
    if (hi <= lo) return YS_OK;
    long blk = 0;
    for (int i = lo; i < hi; i++) { m->red_host[i].blk0 = blk; blk += (m->red_host[i].n + YS_WGRED_OUT_PER_BLOCK - 1) / YS_WGRED_OUT_PER_BLOCK; }
    if (m->red_uploaded.size() != m->red_host.size()) m->red_uploaded.assign(m->red_host.size(), WgRedDesc{});
    if (memcmp(&m->red_uploaded[lo], &m->red_host[lo], (size_t)(hi - lo) * sizeof(WgRedDesc)) != 0) {   // first step / batch size / launch partition changed
      YS_CHECK_HIP(hipMemcpyAsync(m->red_dev + lo, &m->red_host[lo], (size_t)(hi - lo) * sizeof(WgRedDesc), hipMemcpyHostToDevice, st));
      YS_CHECK_HIP(hipStreamSynchronize(st));
      memcpy(&m->red_uploaded[lo], &m->red_host[lo], (size_t)(hi - lo) * sizeof(WgRedDesc));
    }
    return ys_wgrad_reduce_batched_launch(sr, m->red_dev + lo, hi - lo, blk);
  };
  // one2one pass: Proto's units were skipped above, so their descriptors (the tail of the head segment's run) are left out of this reduction
  const int rlo = m->red_first[seg_lo], rhi = m->e2e_pass ? m->red_proto0 : m->red_first[seg_hi + 1];
  // The step's LAST dependency chain is dgrad(model.1) -> BN backward of model.0 -> stem weight gradient -> split reduction -> AdamW (round-6 trace: 200 us with the
  // main stream idle).  In the one-call backward the stem's weight gradient is therefore handed over on its own, AFTER the reduction of everything else in its
  // segment has been queued on the second stream: that reduction (48 us) then runs while the main stream is still in the BatchNorm backward of model.0, and only
  // the stem's own slabs are reduced behind its weight gradient.  (With the BatchNorm backward inside the stem's weight-gradient kernel -- PendWg::bnb -- that link is
  // gone from the chain and the launch runs on the main stream: below.)
  bool stem_split = false;
  ys_model::PendWg stem_job{};
  if (async_end && !seg_events && m->overlap && seg_hi == ys_model::NSEG - 1 && !m->pend_wg.empty() && m->convs[m->pend_wg.back().conv].first &&
      m->convs[m->pend_wg.back().conv].red_slot == rlo && m->defer_wgred && rhi - rlo > 1) {
    stem_split = true; stem_job = m->pend_wg.back(); m->pend_wg.pop_back();
  }
  YS_TRY(flush_wgrads(m, B));
  const bool on_st2 = async_end && m->overlap && (m->st2_dirty || stem_split);
  hipStream_t sr = on_st2 ? m->st2 : st;
  if (!on_st2) YS_TRY(join_wgrad_stream(m));
  if (m->f8 && seg_hi == ys_model::NSEG - 1) m->f8_bwd_done = true;     // every gradient maximum of the step is recorded (last segment = stem)
  if (stem_split && stem_job.bnb) {
    // The stem's weight gradient with its BatchNorm backward inside needs nothing from the second stream and the main stream has nothing else left: it runs HERE,
    // beside the reduction of the rest of the segment on the second stream, with no hand-over event -- and reads the unit's output and gradient map in stream order.
    YS_TRY(reduce_range(rlo + 1, rhi, sr));
    m->st2_dirty = true;
    YS_TRY(launch_wgrad(m, m->convs[stem_job.conv], B, stem_job.dy, stem_job.ldc, stem_job.coff, stem_job.bstride, st, true));
    YS_TRY(reduce_range(rlo, rlo + 1, st));
  } else if (stem_split) {
    YS_TRY(reduce_range(rlo + 1, rhi, sr));
    m->pend_wg.push_back(stem_job);
    YS_TRY(flush_wgrads(m, B));
    YS_TRY(reduce_range(rlo, rlo + 1, sr));
  } else {
    YS_TRY(reduce_range(rlo, rhi, sr));
  }
  if (async_end && seg_events) {
    for (int sgi = seg_lo; sgi <= seg_hi; sgi++) {
      m->seg_on_st2[sgi] = on_st2;
      YS_CHECK_HIP(hipEventRecord(m->ev_seg_m[sgi], st));
      if (on_st2) YS_CHECK_HIP(hipEventRecord(m->ev_seg_w[sgi], m->st2));
    }
  }
  YS_CHECK_HIP(hipGetLastError());
  return YS_OK;
}

void reset_grad_state(ys_model* m) {
  for (auto& b : m->bufs) std::fill(b.gw.begin(), b.gw.end(), 0);
  for (auto& c : m->convs) c.red_seen = 0;
  auto written = [&](int buf) { std::fill(m->bufs[buf].gw.begin(), m->bufs[buf].gw.end(), 1); };   // its gradient is already there
  if (m->is_block) return written(m->blk_out);   // the caller's dy
  if (m->cls) return written(m->logit_buf);      // dlogits (ys_loss_classify)
  written(m->pd_buf); written(m->ps_buf);        // the loss wrote the head gradients
  if (m->segment) written(m->pr_buf);
  if (m->segment || m->xkind >= 2) written(m->mc_buf);   // mask-coefficient / angle-logit / keypoint gradients
}

}  // namespace ysm
