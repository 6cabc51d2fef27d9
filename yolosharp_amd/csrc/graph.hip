// graph.hip -- graph builder behind ys_model_create / ys_block_create / ys_head_create (the handle: ys_model.h; layout and allocation: plan.hip; the step:
// model.hip; the entry points: model_api.hip).
//
// Builds the reference's Yolov8 detect graph (Models/Yolo.cs:41-89: widths/depths table :43-55, layer list
// :56-87, skip router :92-134) out of Conv units (Modules/Convs.cs:36-62), C2f/Bottleneck
// (Modules/Block.cs:371-399, 572-608), SPPF (Block.cs:236-285), Upsample+Concat (Yolo.cs:70-75) and the
// Detect head (Modules/Head.cs:35-53,71-106,204-223), as a flat list of device ops over NHWC buffers:
//   * every Concat is a shared buffer: producers write their channel slice, chunk(2,1) is a view
//   * Bottleneck's shortcut add is fused into the BN/SiLU apply pass of its cv2
//   * Detect towers write straight into [B, A, C] (= the permuted layout the loss consumes)
#include "ys_model.h"
#include <algorithm>

namespace ysm {

int new_buf(ys_model* m, int H, int W, int C) {
  Buf b; b.H = H; b.W = W; b.ldc = C; b.rows_per_b = (long)H * W; b.gw.assign(C, 0);
  m->bufs.push_back(b);
  return (int)m->bufs.size() - 1;
}

namespace {

// one Conv unit (conv+BN+act) or plain biased Conv2d; returns conv index and appends the op
int add_conv(ys_model* m, const std::string& name, View in, View out, int cin, int cout, int k, int s, bool bn, bool act,
             int Hin, int Win, int seg, const View* res = nullptr, bool dw = false, int pad = -1) {
  ConvL c; c.name = name; c.in = in; c.out = out; c.cin = cin; c.cout = cout; c.k = k; c.s = s; c.bn = bn; c.act = act; c.dw = dw;
  c.cin_pad = in.C; c.Hin = Hin; c.Win = Win;
  const int p = c.pad = pad < 0 ? k / 2 : pad;      // autopad (Convs.cs:36-62) unless the module names its padding (Yolov5u's model.0: k = 6, p = 2)
  c.Hout = (Hin + 2 * p - k) / s + 1; c.Wout = (Win + 2 * p - k) / s + 1;
  c.cout_ld = (cout + m->epl - 1) / m->epl * m->epl;
  c.cout_real = cout;
  c.seg = seg;
  if (res) { c.res = *res; c.has_res = true; }
  c.idx = (int)m->convs.size();
  m->convs.push_back(c);
  Op op; op.type = OP_CONV; op.conv = (int)m->convs.size() - 1; op.in = in; op.out = out; op.H = Hin; op.W = Win; op.seg = seg;
  m->ops.push_back(op);
  return op.conv;
}

// registration-list entry of member `mem` of a fused convolution (plain convolutions: the index itself)
inline int reg_entry(int conv, int mem) { return conv | (mem << 20); }
int add_conv_reg(ys_model* m, const std::string& name, View in, View out, int cin, int cout, int k, int s, bool bn, bool act,
                 int Hin, int Win, int seg, const View* res = nullptr, bool dw = false, int pad = -1) {
  const int i = add_conv(m, name, in, out, cin, cout, k, s, bn, act, Hin, Win, seg, res, dw, pad);
  m->reg.push_back(i);
  return i;
}

// Bottleneck (Block.cs:572-608) k1 x k1, k2 x k2 (the default k = (3, 3)) with hidden = int(c*e); returns conv indices {cv1, cv2}
std::pair<int, int> add_bottleneck(ys_model* m, const std::string& name, View in, View out, int c, float e, bool shortcut, int H, int W, int seg,
                                   int k1 = 3, int k2 = 3) {
  const int c_ = (int)(c * e);
  const int tmp = new_buf(m, H, W, c_);
  const int a = add_conv(m, name + ".cv1", in, View{tmp, 0, c_}, c, c_, k1, 1, true, true, H, W, seg);
  const int b = add_conv(m, name + ".cv2", View{tmp, 0, c_}, out, c_, c, k2, 1, true, true, H, W, seg, shortcut ? &in : nullptr);
  return {a, b};
}

// C3 (Block.cs:404-442): cv3(cat(m(cv1(x)), cv2(x))), m = n Bottlenecks(c_, c_, k = (k1, 3), e=1.0), c_ = int(c2 * 0.5); registration
// order cv1, cv2, cv3, m.* ; appends its conv indices (registration order) to `regs`.  C3 itself has k1 = 1 (:429), C3k (Block.cs:611-620) k1 = 3
void add_c3_body(ys_model* m, const std::string& name, View in, View out, int c1, int c2, int n, bool shortcut, int k1, int H, int W, int seg,
                 std::vector<int>& regs) {
  const int c_ = (int)(c2 * 0.5f);
  const int cat = new_buf(m, H, W, 2 * c_);
  int cur = new_buf(m, H, W, c_);
  const int i1 = add_conv(m, name + ".cv1", in, View{cur, 0, c_}, c1, c_, 1, 1, true, true, H, W, seg);
  std::vector<int> mids;
  for (int i = 0; i < n; i++) {
    const View bin{cur, 0, c_};
    View bout;
    if (i == n - 1) bout = View{cat, 0, c_};
    else { cur = new_buf(m, H, W, c_); bout = View{cur, 0, c_}; }
    auto pr = add_bottleneck(m, name + ".m." + std::to_string(i), bin, bout, c_, 1.0f, shortcut, H, W, seg, k1, 3);
    mids.push_back(pr.first); mids.push_back(pr.second);
  }
  const int i2 = add_conv(m, name + ".cv2", in, View{cat, c_, c_}, c1, c_, 1, 1, true, true, H, W, seg);
  const int i3 = add_conv(m, name + ".cv3", View{cat, 0, 2 * c_}, out, 2 * c_, c2, 1, 1, true, true, H, W, seg);
  regs.push_back(i1); regs.push_back(i2); regs.push_back(i3);
  for (int i : mids) regs.push_back(i);
}
void add_c3k(ys_model* m, const std::string& name, View in, View out, int c1, int c2, int n, bool shortcut, int H, int W, int seg,
             std::vector<int>& regs) {
  add_c3_body(m, name, in, out, c1, c2, n, shortcut, 3, H, W, seg, regs);
}
// C3 as a module of its own (Yolov5u, ys_block_create): registered straight into the model's list
void add_c3(ys_model* m, const std::string& name, View in, View out, int c1, int c2, int n, bool shortcut, int H, int W, int seg) {
  add_c3_body(m, name, in, out, c1, c2, n, shortcut, 1, H, W, seg, m->reg);
}

// C2f (Block.cs:371-399): cv1 1x1 -> chunk -> n Bottlenecks (3x3,3x3, e=1.0) -> cat -> cv2 1x1, and C3k2 (Block.cs:623-662): the same with hidden width
// int(c2 * e) and m[i] = C3k(c,c,2) or Bottleneck(c,c,e=0.5), shortcut always on.  `be`: the Bottlenecks' expansion
void add_c2(ys_model* m, const std::string& name, View xin, View xout, int c1, int c2, int n, float e, bool c3k, float be, bool shortcut, int H, int W, int seg) {
  const int c = (int)(c2 * e);
  const int cat = new_buf(m, H, W, (2 + n) * c);
  const int i1 = add_conv(m, name + ".cv1", xin, View{cat, 0, 2 * c}, c1, 2 * c, 1, 1, true, true, H, W, seg);
  std::vector<int> mids;
  for (int i = 0; i < n; i++) {
    const View bin{cat, (1 + i) * c, c};
    const View bout{cat, (2 + i) * c, c};
    const std::string bp = name + ".m." + std::to_string(i);
    if (c3k) add_c3k(m, bp, bin, bout, c, c, 2, true, H, W, seg, mids);
    else { auto pr = add_bottleneck(m, bp, bin, bout, c, be, shortcut, H, W, seg); mids.push_back(pr.first); mids.push_back(pr.second); }
  }
  const int i2 = add_conv(m, name + ".cv2", View{cat, 0, (2 + n) * c}, xout, (2 + n) * c, c2, 1, 1, true, true, H, W, seg);
  m->reg.push_back(i1); m->reg.push_back(i2);            // registration order: cv1, cv2, m.* (Block.cs:373-376)
  for (int i : mids) m->reg.push_back(i);
}
void add_c2f(ys_model* m, const std::string& name, View xin, View xout, int c1, int c2, int n, bool shortcut, int H, int W, int seg) {
  add_c2(m, name, xin, xout, c1, c2, n, 0.5f, false, 1.0f, shortcut, H, W, seg);
}
void add_c3k2(ys_model* m, const std::string& name, View xin, View xout, int c1, int c2, int n, bool c3k, float e, int H, int W, int seg) {
  add_c2(m, name, xin, xout, c1, c2, n, e, c3k, 0.5f, true, H, W, seg);
}

// C2PSA (Block.cs:664-810).  Reference quirks kept: qkv / proj / pe and both ffn convs all use the default SiLU.
void add_c2psa(ys_model* m, const std::string& name, View xin, View xout, int c1, int n, int H, int W, int seg) {
  const int c = (int)(c1 * 0.5f);
  const int cat = new_buf(m, H, W, 2 * c);       // cv1 output: a | b
  const int cat2 = new_buf(m, H, W, 2 * c);      // cv2 input:  a | b_final
  const int i1 = add_conv(m, name + ".cv1", xin, View{cat, 0, 2 * c}, c1, 2 * c, 1, 1, true, true, H, W, seg);
  { Op op; op.type = OP_COPY; op.in = View{cat, 0, c}; op.out = View{cat2, 0, c}; op.H = H; op.W = W; op.seg = seg; m->ops.push_back(op); }
  std::vector<int> mids;
  View bcur{cat, c, c};
  const int heads = c / 64, hd = c / heads, kd = (int)(hd * 0.5f);
  const int hq = c + 2 * kd * heads;
  for (int i = 0; i < n; i++) {
    const std::string bp = name + ".m." + std::to_string(i);
    const int qb = new_buf(m, H, W, hq), ao = new_buf(m, H, W, c), vb = new_buf(m, H, W, c), sb = new_buf(m, H, W, c);
    const int b1 = new_buf(m, H, W, c), f1 = new_buf(m, H, W, 2 * c);
    const int iq = add_conv(m, bp + ".attn.qkv", bcur, View{qb, 0, hq}, c, hq, 1, 1, true, true, H, W, seg);
    { Op op; op.type = OP_ATTN; op.in = View{qb, 0, hq}; op.out = View{ao, 0, c}; op.H = H; op.W = W; op.seg = seg; op.heads = heads; op.kd = kd; op.hd = hd; m->ops.push_back(op); }
    { Op op; op.type = OP_VCOPY; op.in = View{qb, 0, hq}; op.out = View{vb, 0, c}; op.H = H; op.W = W; op.seg = seg; op.heads = heads; op.kd = kd; op.hd = hd; m->ops.push_back(op); }
    const View aov{ao, 0, c};
    const int ipe = add_conv(m, bp + ".attn.pe", View{vb, 0, c}, View{sb, 0, c}, c, c, 3, 1, true, true, H, W, seg, &aov, true);
    const int ipr = add_conv(m, bp + ".attn.proj", View{sb, 0, c}, View{b1, 0, c}, c, c, 1, 1, true, true, H, W, seg, &bcur);
    const int if0 = add_conv(m, bp + ".ffn.0", View{b1, 0, c}, View{f1, 0, 2 * c}, c, 2 * c, 1, 1, true, true, H, W, seg);
    const View b1v{b1, 0, c};
    View bnext;
    if (i == n - 1) bnext = View{cat2, c, c};
    else { const int nb = new_buf(m, H, W, c); bnext = View{nb, 0, c}; }
    const int if1 = add_conv(m, bp + ".ffn.1", View{f1, 0, 2 * c}, bnext, 2 * c, c, 1, 1, true, true, H, W, seg, &b1v);
    mids.push_back(iq); mids.push_back(ipr); mids.push_back(ipe); mids.push_back(if0); mids.push_back(if1);   // qkv, proj, pe (Block.cs:744-746)
    bcur = bnext;
  }
  const int i2 = add_conv(m, name + ".cv2", View{cat2, 0, 2 * c}, xout, 2 * c, c1, 1, 1, true, true, H, W, seg);
  m->reg.push_back(i1); m->reg.push_back(i2);
  for (int i : mids) m->reg.push_back(i);
}

void add_sppf(ys_model* m, const std::string& name, View xin, View xout, int c1, int H, int W, int seg) {
  // SPPF (Block.cs:236-285): cv1 has NO activation (:257); three chained 5x5 pools
  const int c_ = c1 / 2;
  const int catS = new_buf(m, H, W, 4 * c_);
  add_conv_reg(m, name + ".cv1", xin, View{catS, 0, c_}, c1, c_, 1, 1, true, false, H, W, seg);
  for (int i = 0; i < 3; i++) {
    Op op; op.type = OP_MAXPOOL; op.in = View{catS, i * c_, c_}; op.out = View{catS, (i + 1) * c_, c_}; op.H = H; op.W = W; op.seg = seg;
    m->ops.push_back(op);
  }
  add_conv_reg(m, name + ".cv2", View{catS, 0, 4 * c_}, xout, 4 * c_, c1, 1, 1, true, true, H, W, seg);
}

// Proto (Block.cs:51-84): cv1 3x3 -> ConvTranspose2d(2,2,bias) -> cv2 3x3 -> cv3 1x1; field / registration order cv1, cv2, cv3,
// upsample (:53-56).  Returns the output buffer [2H][2W][pad(nm)].
int add_proto(ys_model* m, const std::string& name, View in, int c1, int npr, int nm, int H, int W, int seg) {
  const int ld = (nm + m->epl - 1) / m->epl * m->epl;
  const int pa = new_buf(m, H, W, npr), pu = new_buf(m, 2 * H, 2 * W, npr), pb = new_buf(m, 2 * H, 2 * W, npr);
  const int out = new_buf(m, 2 * H, 2 * W, ld);
  const int p1 = add_conv(m, name + ".cv1", in, View{pa, 0, npr}, c1, npr, 3, 1, true, true, H, W, seg);
  const int pup = add_conv(m, name + ".upsample", View{pa, 0, npr}, View{pu, 0, npr}, npr, npr, 1, 1, false, false, H, W, seg);
  m->convs[pup].ct = true; m->convs[pup].Hout = 2 * H; m->convs[pup].Wout = 2 * W;
  const int p2 = add_conv(m, name + ".cv2", View{pu, 0, npr}, View{pb, 0, npr}, npr, npr, 3, 1, true, true, 2 * H, 2 * W, seg);
  const int p3 = add_conv(m, name + ".cv3", View{pb, 0, npr}, View{out, 0, nm}, npr, nm, 1, 1, true, true, 2 * H, 2 * W, seg);
  m->reg.push_back(p1); m->reg.push_back(p2); m->reg.push_back(p3); m->reg.push_back(pup);
  return out;
}

}  // namespace

// Detect (Head.cs:35-53): c2 = max(16, ch0/4, 4*reg_max), c3 = max(ch0, min(nc,100)); strides fixed {8,16,32} (:43).
// legacy=false (v11, Head.cs:50): each 3x3 Conv of the cls tower becomes DWConv3x3(x->x) + Conv1x1(x->c3).
int add_detect(ys_model* m, const std::string& hp, const int* pv, const int* ch, const int* hh, const int* ww, bool legacy, int seg) {
  const ys_model_desc& d = m->d;
  const int c2 = std::max(16, std::max(ch[0] / 4, d.reg_max * 4));
  const int c3 = std::max(ch[0], std::min(d.nc, 100));
  if (c2 % m->epl || c3 % m->epl) { ys_set_error("model: head widths c2=%d c3=%d must be multiples of %d", c2, c3, m->epl); return YS_ERR_UNSUPPORTED; }
  m->head_prefix = hp;
  m->head_conv0 = (int)m->convs.size();
  for (int i = 0; i < 3; i++) m->det_in[i] = pv[i];
  m->nl = 3; m->A = 0;
  for (int i = 0; i < 3; i++) { m->lvl_off[i] = m->A; m->lvl_w[i] = ww[i]; m->lvl_h[i] = hh[i]; m->A += hh[i] * ww[i]; }
  m->ld_pd = (4 * d.reg_max + m->epl - 1) / m->epl * m->epl;
  m->ld_ps = (d.nc + m->epl - 1) / m->epl * m->epl;
  m->pd_buf = new_buf(m, 1, m->A, m->ld_pd);
  m->ps_buf = new_buf(m, 1, m->A, m->ld_ps);
  // Shared-input fusion (round 4).  cv2[i][0] = Conv(x, c2, 3) and cv3[i][0] = Conv(x, c3, 3) -- and Segment's cv4[i][0] = Conv(x, c4, 3) --
  // read the SAME x[i] (Head.cs:47-48, 254-259, consumed at :81-82): they run as ONE convolution with Cout = c2 + c3 (+ c4) into one
  // buffer whose channel slices the second tower layers read.  BatchNorm and SiLU are per channel, so this is exact; the input is
  // read once in the forward and in the weight gradient, and the input gradient is ONE dgrad with K = 9 (c2 + c3 + c4) instead of an
  // overwrite followed by read-modify-write accumulations.  The state_dict keeps the reference's module names (ConvL::members).
  // v11 heads (legacy = false) start their class tower with a depthwise unit: nothing to fuse with there.  YS_HEAD_FUSE=0: one launch each.
  const int c4s = d.task == YS_SEGMENT ? std::max(ch[0] / 4, 32) : 0;
  const int cf = c2 + c3 + c4s;
  bool fuse = legacy && (YS_OPT_INT("HEAD_FUSE", 1) != 0) && (c4s % m->epl) == 0;
  if (m->f8 && (cf % 32 || c2 % 32 || c3 % 32)) fuse = false;   // fp8 mode: the dgrad of a fused layer must still qualify for the fp8 kernel (K units of 32)
  int fbuf[3] = {-1, -1, -1}, fconv[3] = {-1, -1, -1};
  const size_t op0 = m->ops.size();
  auto tag = [&](int idx, int tower, int depth) { m->convs[idx].stage = tower * 4 + depth; };   // towers: 0 cv2, 1 cv3, 2 proto, 3 cv4
  for (int t = 0; t < 2; t++) {   // cv2 towers for all levels, then cv3 towers (registration order cv2.*, cv3.*)
    for (int i = 0; i < 3; i++) {
      const int cm = t == 0 ? c2 : c3;
      const int co = t == 0 ? 4 * d.reg_max : d.nc;
      const int ob = t == 0 ? m->pd_buf : m->ps_buf;
      const std::string tp = hp + (t == 0 ? ".cv2." : ".cv3.") + std::to_string(i);
      const int t1 = new_buf(m, hh[i], ww[i], cm);
      if (fuse) {
        if (t == 0) {
          fbuf[i] = new_buf(m, hh[i], ww[i], cf);
          fconv[i] = add_conv(m, tp + ".0+cv3" + (c4s ? "+cv4" : ""), View{pv[i], 0, ch[i]}, View{fbuf[i], 0, cf}, ch[i], cf, 3, 1, true, true, hh[i], ww[i], seg);
          ConvL& fc = m->convs[fconv[i]];
          fc.members.push_back({tp + ".0", 0, c2});
          fc.members.push_back({hp + ".cv3." + std::to_string(i) + ".0", c2, c3});
          if (c4s) fc.members.push_back({hp + ".cv4." + std::to_string(i) + ".0", c2 + c3, c4s});
          tag(fconv[i], 0, 0);
        }
        m->reg.push_back(reg_entry(fconv[i], t));
        tag(add_conv_reg(m, tp + ".1", View{fbuf[i], t == 0 ? 0 : c2, cm}, View{t1, 0, cm}, cm, cm, 3, 1, true, true, hh[i], ww[i], seg), t, 1);
      } else if (t == 0 || legacy) {
        const int t0 = new_buf(m, hh[i], ww[i], cm);
        tag(add_conv_reg(m, tp + ".0", View{pv[i], 0, ch[i]}, View{t0, 0, cm}, ch[i], cm, 3, 1, true, true, hh[i], ww[i], seg), t, 0);
        tag(add_conv_reg(m, tp + ".1", View{t0, 0, cm}, View{t1, 0, cm}, cm, cm, 3, 1, true, true, hh[i], ww[i], seg), t, 1);
      } else {
        const int t0 = new_buf(m, hh[i], ww[i], cm);
        const int d0 = new_buf(m, hh[i], ww[i], ch[i]), d1 = new_buf(m, hh[i], ww[i], cm);
        add_conv_reg(m, tp + ".0.0", View{pv[i], 0, ch[i]}, View{d0, 0, ch[i]}, ch[i], ch[i], 3, 1, true, true, hh[i], ww[i], seg, nullptr, true);
        add_conv_reg(m, tp + ".0.1", View{d0, 0, ch[i]}, View{t0, 0, cm}, ch[i], cm, 1, 1, true, true, hh[i], ww[i], seg);
        add_conv_reg(m, tp + ".1.0", View{t0, 0, cm}, View{d1, 0, cm}, cm, cm, 3, 1, true, true, hh[i], ww[i], seg, nullptr, true);
        add_conv_reg(m, tp + ".1.1", View{d1, 0, cm}, View{t1, 0, cm}, cm, cm, 1, 1, true, true, hh[i], ww[i], seg);
      }
      const int cc = add_conv_reg(m, tp + ".2", View{t1, 0, cm}, View{ob, 0, co}, cm, co, 1, 1, false, false, hh[i], ww[i], seg);
      m->convs[cc].out_rowoff = m->lvl_off[i];
      tag(cc, t, 2);
    }
  }
  m->dfl_after_conv = m->reg.back();
  if (d.task == YS_SEGMENT) {
    // Segment (Head.cs:238-324): Proto(ch0, npr = ch0, nm = 32) on P3 (Yolo.cs:348,366) and the cv4 towers (c4 = max(ch0/4, nm))
    m->segment = true; m->nm = 32; m->n_items = 5;
    const int nm = m->nm, npr = ch[0];
    const int c4 = std::max(ch[0] / 4, nm);
    if (c4 % m->epl || npr % m->epl) { ys_set_error("model: segment widths c4=%d npr=%d must be multiples of %d", c4, npr, m->epl); return YS_ERR_UNSUPPORTED; }
    m->ld_mc = (nm + m->epl - 1) / m->epl * m->epl;
    m->ld_pr = m->ld_mc;
    m->mh = 2 * hh[0]; m->mw = 2 * ww[0];
    {
      const size_t pc0 = m->convs.size();
      m->pr_buf = add_proto(m, hp + ".proto", View{pv[0], 0, ch[0]}, ch[0], npr, nm, hh[0], ww[0], seg);
      for (size_t k = pc0; k < m->convs.size(); k++) { m->convs[k].stage = 2 * 4 + (int)(k - pc0); m->convs[k].proto = true; }   // a chain: one unit per stage
    }
    m->mc_buf = new_buf(m, 1, m->A, m->ld_mc);
    for (int i = 0; i < 3; i++) {
      const std::string tp = hp + ".cv4." + std::to_string(i);
      const int t1 = new_buf(m, hh[i], ww[i], c4);
      if (fuse) {                 // cv4[i][0] ran inside the level's fused first convolution (channels [c2 + c3, c2 + c3 + c4) of its output)
        m->reg.push_back(reg_entry(fconv[i], 2));
        tag(add_conv_reg(m, tp + ".1", View{fbuf[i], c2 + c3, c4}, View{t1, 0, c4}, c4, c4, 3, 1, true, true, hh[i], ww[i], seg), 4, 1);
      } else {
        const int t0 = new_buf(m, hh[i], ww[i], c4);
        tag(add_conv_reg(m, tp + ".0", View{pv[i], 0, ch[i]}, View{t0, 0, c4}, ch[i], c4, 3, 1, true, true, hh[i], ww[i], seg), 4, 0);
        tag(add_conv_reg(m, tp + ".1", View{t0, 0, c4}, View{t1, 0, c4}, c4, c4, 3, 1, true, true, hh[i], ww[i], seg), 4, 1);
      }
      const int cc = add_conv_reg(m, tp + ".2", View{t1, 0, c4}, View{m->mc_buf, 0, nm}, c4, nm, 1, 1, false, false, hh[i], ww[i], seg);
      m->convs[cc].out_rowoff = m->lvl_off[i];
      tag(cc, 4, 2);
    }
    m->xkind = 1;
  } else if (d.task == YS_OBB || d.task == YS_POSE) {
    // Obb: ne = 1 angle logit per anchor (Head.cs:384-390); Pose: nk = kpt_num * kpt_dim outputs (Head.cs:492-499).  Both add
    // only the cv4 towers (c4 = max(ch0/4, ne|nk)) after Detect's own modules
    const bool obb = d.task == YS_OBB;
    m->kdim = d.kpt_dim > 0 ? d.kpt_dim : 3;
    const int nx = obb ? 1 : (d.kpt_num > 0 ? d.kpt_num : 17) * m->kdim;
    if (!obb && m->kdim != 2 && m->kdim != 3) { ys_set_error("model: keypoint dim %d (2 or 3)", m->kdim); return YS_ERR_INVALID_ARG; }
    m->nm = nx; m->xkind = obb ? 2 : 3;
    m->n_items = obb ? 4 : 5;      // v8OBBLoss: box, cls, dfl, angle (Loss.cs:546); v8PoseLoss: box, pose, kobj, cls, dfl (Loss.cs:923)
    const int c4 = std::max(ch[0] / 4, nx);                      // Pose n/s/m: 51, not a multiple of the 16-byte unit
    const int c4p = (c4 + m->epl - 1) / m->epl * m->epl;         // tower buffers are padded; the pad channels stay zero
    m->ld_mc = (nx + m->epl - 1) / m->epl * m->epl;
    m->mc_buf = new_buf(m, 1, m->A, m->ld_mc);
    for (int i = 0; i < 3; i++) {
      const std::string tp = hp + ".cv4." + std::to_string(i);
      const int t0 = new_buf(m, hh[i], ww[i], c4p), t1 = new_buf(m, hh[i], ww[i], c4p);
      const int k0 = add_conv_reg(m, tp + ".0", View{pv[i], 0, ch[i]}, View{t0, 0, c4p}, ch[i], c4p, 3, 1, true, true, hh[i], ww[i], seg);
      const int k1 = add_conv_reg(m, tp + ".1", View{t0, 0, c4p}, View{t1, 0, c4p}, c4, c4p, 3, 1, true, true, hh[i], ww[i], seg);
      m->convs[k0].cout_real = m->convs[k1].cout_real = c4;
      const int cc = add_conv_reg(m, tp + ".2", View{t1, 0, c4p}, View{m->mc_buf, 0, nx}, c4, nx, 1, 1, false, false, hh[i], ww[i], seg);
      m->convs[cc].out_rowoff = m->lvl_off[i];
      tag(k0, 4, 0); tag(k1, 4, 1); tag(cc, 4, 2);
    }
  }
  // Level-parallel schedule (v8 heads; YS_GROUP=0 keeps the level-major order and single launches): the head's ops stage-major -- the same
  // tower layer of P3, P4, P5 next to each other -- and every stage of >= 2 units is one group.  Units of a stage read and write disjoint
  // buffers (per-level towers, per-level rows of the prediction buffers); a stage only depends on earlier stages of its own tower and on
  // the (fused) first layers, which sort first.
  const bool group_on = legacy && (YS_OPT_INT("GROUP", 1) != 0) && !m->f8;
  if (group_on) {
    bool all = true;
    for (size_t k = op0; k < m->ops.size(); k++) all = all && m->ops[k].type == OP_CONV && m->convs[m->ops[k].conv].stage >= 0;
    if (all) {
      std::stable_sort(m->ops.begin() + op0, m->ops.end(), [&](const Op& x, const Op& y) { return m->convs[x.conv].stage < m->convs[y.conv].stage; });
      int gid = 0;
      for (size_t k = op0; k < m->ops.size();) {
        size_t e = k + 1;
        while (e < m->ops.size() && m->convs[m->ops[e].conv].stage == m->convs[m->ops[k].conv].stage) e++;
        const ConvL& c0 = m->convs[m->ops[k].conv];
        if (e - k >= 2 && (int)(e - k) <= YS_GROUP_MAX && !c0.dw && !c0.ct) { for (size_t j = k; j < e; j++) m->convs[m->ops[j].conv].group = gid; gid++; }
        k = e;
      }
    }
  }
  return YS_OK;
}

// Classify (Head.cs:612-644): Conv(c1, 1280, 1) -> AdaptiveAvgPool2d(1) -> flatten -> Dropout(0) -> Linear(1280, nc), all in segment `seg`.
// The pool is an op of its own (OP_POOL); in training it also applies the Conv unit's BN + SiLU, so the activated 1280-channel map is never
// written.  Linear is a plain 1x1 convolution with bias on a 1 x 1 map: M = B rows, nc output channels padded to the 16-byte unit like the
// Detect class towers -- its forward, weight / input gradients, weight shadows and optimizer groups are the convolution machinery's.
int add_classify(ys_model* m, const std::string& hp, View in, int c1, int H, int W, int seg) {
  const int c_ = 1280;   // efficientnet_b0 size (Head.cs:622)
  m->cls = true; m->n_items = 1; m->head_prefix = hp; m->nl = 0; m->A = 0;
  m->ld_cls = (m->d.nc + m->epl - 1) / m->epl * m->epl;
  const int cb = new_buf(m, H, W, c_);
  m->bufs[cb].need_grad = false;   // its gradient dpooled / HW is never materialised (run_conv_bwd, pool_next)
  m->pool_buf = new_buf(m, 1, 1, c_);
  m->logit_buf = new_buf(m, 1, 1, m->ld_cls);
  m->cls_conv = add_conv_reg(m, hp + ".conv", in, View{cb, 0, c_}, c1, c_, 1, 1, true, true, H, W, seg);
  m->convs[m->cls_conv].pool_next = true;
  { Op op; op.type = OP_POOL; op.conv = m->cls_conv; op.in = View{cb, 0, c_}; op.out = View{m->pool_buf, 0, c_}; op.H = H; op.W = W; op.seg = seg; m->ops.push_back(op); }
  const int li = add_conv_reg(m, hp + ".linear", View{m->pool_buf, 0, c_}, View{m->logit_buf, 0, m->d.nc}, c_, m->d.nc, 1, 1, false, false, 1, 1, seg);
  m->convs[li].linear = true;
  return YS_OK;
}

// ---- size tables (Yolo.cs:43-55 / :200-215), shared by the detect and classify graphs
static int v8_widths(ys_model* m, int w[5], int dep[3]) {
  static const float dm[5] = {0.34f, 0.34f, 0.67f, 1.0f, 1.0f};
  static const float wm[5] = {0.25f, 0.5f, 0.75f, 1.0f, 1.25f};
  static const int mc[5] = {1024, 1024, 576, 512, 640};
  const int base_w[5] = {64, 128, 256, 512, 1024};
  const int sz = m->d.size;
  for (int i = 0; i < 5; i++) w[i] = std::min((int)(base_w[i] * wm[sz]), mc[sz]);   // Yolo.cs:53
  dep[0] = (int)(3 * dm[sz]); dep[1] = (int)(6 * dm[sz]); dep[2] = (int)(9 * dm[sz]);   // Yolo.cs:54
  for (int i = 0; i < 5; i++)
    if (w[i] % m->epl || ((int)(w[i] * 0.5f)) % m->epl) { ys_set_error("model: width %d not a multiple of %d", w[i], m->epl); return YS_ERR_UNSUPPORTED; }
  return YS_OK;
}

static void new_input_buf(ys_model* m) {
  m->in_buf = new_buf(m, m->d.height, m->d.width, m->epl);
  m->bufs[m->in_buf].need_grad = false;
}

// Yolov8 model.0 - model.8 (Yolo.cs:56-66) from the input buffer; model.4 / model.6 / model.8 write the given views.  Backward segments:
// s04 for model.0-4, s56 for model.5-6, s78 for model.7-8
static void v8_backbone(ys_model* m, const int* w, const int* dep, View v4, View v6, View v8, int s04, int s56, int s78) {
  const int H = m->d.height, W = m->d.width;
  const int H2 = H / 2, W2 = W / 2, H4 = H / 4, W4 = W / 4, H8 = H / 8, W8 = W / 8, H16 = H / 16, W16 = W / 16, H32 = H / 32, W32 = W / 32;
  const int b0 = new_buf(m, H2, W2, w[0]), b1 = new_buf(m, H4, W4, w[1]), b2 = new_buf(m, H4, W4, w[1]);
  const int b3 = new_buf(m, H8, W8, w[2]), b5 = new_buf(m, H16, W16, w[3]), b7 = new_buf(m, H32, W32, w[4]);
  int ci = add_conv_reg(m, "model.0", View{m->in_buf, 0, m->epl}, View{b0, 0, w[0]}, 3, w[0], 3, 2, true, true, H, W, s04);
  m->convs[ci].first = true;
  add_conv_reg(m, "model.1", View{b0, 0, w[0]}, View{b1, 0, w[1]}, w[0], w[1], 3, 2, true, true, H2, W2, s04);
  add_c2f(m, "model.2", View{b1, 0, w[1]}, View{b2, 0, w[1]}, w[1], w[1], dep[0], true, H4, W4, s04);
  add_conv_reg(m, "model.3", View{b2, 0, w[1]}, View{b3, 0, w[2]}, w[1], w[2], 3, 2, true, true, H4, W4, s04);
  add_c2f(m, "model.4", View{b3, 0, w[2]}, v4, w[2], w[2], dep[1], true, H8, W8, s04);
  add_conv_reg(m, "model.5", v4, View{b5, 0, w[3]}, w[2], w[3], 3, 2, true, true, H8, W8, s56);
  add_c2f(m, "model.6", View{b5, 0, w[3]}, v6, w[3], w[3], dep[1], true, H16, W16, s56);
  add_conv_reg(m, "model.7", v6, View{b7, 0, w[4]}, w[3], w[4], 3, 2, true, true, H16, W16, s78);
  add_c2f(m, "model.8", View{b7, 0, w[4]}, v8, w[4], w[4], dep[0], true, H32, W32, s78);
}

// Yolov8Classify (Yolo.cs:537-554): the Yolov8 list without its last 14 modules -- model.0 - model.8, no SPPF -- then Classify(widths[4], nc)
int build_v8_classify(ys_model* m) {
  int w[5], dep[3];
  YS_TRY(v8_widths(m, w, dep));
  const int H8 = m->d.height / 8, W8 = m->d.width / 8, H16 = m->d.height / 16, W16 = m->d.width / 16, H32 = m->d.height / 32, W32 = m->d.width / 32;
  new_input_buf(m);
  const int b4 = new_buf(m, H8, W8, w[2]), b6 = new_buf(m, H16, W16, w[3]), b8 = new_buf(m, H32, W32, w[4]);
  // backward segments: head (1280-channel Conv, pool, Linear), model.7-8, model.5-6, stem (model.0-4)
  v8_backbone(m, w, dep, View{b4, 0, w[2]}, View{b6, 0, w[3]}, View{b8, 0, w[4]}, 3, 2, 1);
  return add_classify(m, "model.9", View{b8, 0, w[4]}, w[4], H32, W32, 0);
}

int build_v8_detect(ys_model* m) {
  const ys_model_desc& d = m->d;
  int w[5], dep[3];
  YS_TRY(v8_widths(m, w, dep));
  const int H = d.height, W = d.width;
  const int H8 = H / 8, W8 = W / 8, H16 = H / 16, W16 = W / 16, H32 = H / 32, W32 = W / 32;
  new_input_buf(m);
  // concat buffers of the neck (Yolo.cs:70-84; concat order [x, skip], Yolo.cs:107)
  const int cat11 = new_buf(m, H16, W16, w[4] + w[3]);
  const int cat14 = new_buf(m, H8, W8, w[3] + w[2]);
  const int cat17 = new_buf(m, H16, W16, w[2] + w[3]);
  const int cat20 = new_buf(m, H32, W32, w[3] + w[4]);
  const int b8 = new_buf(m, H32, W32, w[4]);
  const int b15 = new_buf(m, H8, W8, w[2]), b18 = new_buf(m, H16, W16, w[3]), b21 = new_buf(m, H32, W32, w[4]);
  const View v4{cat14, w[3], w[2]}, v6{cat11, w[4], w[3]}, v9{cat20, w[3], w[4]}, v12{cat17, w[2], w[3]};
  // backward segments: head first, stem last.  The backbone is cut after model.4: the all-reduce of the LAST segment has no
  // backward left to hide behind, so it should be the smallest (model.0-4: 2.5 % of YOLOv8n's parameters, 4 % of YOLOv8s')
  const int SB = 2, SN = 1, SH = 0, SS = 3;

  v8_backbone(m, w, dep, v4, v6, View{b8, 0, w[4]}, SS, SB, SB);
  add_sppf(m, "model.9", View{b8, 0, w[4]}, v9, w[4], H32, W32, SB);
  { Op op; op.type = OP_UPSAMPLE; op.in = v9; op.out = View{cat11, 0, w[4]}; op.H = H32; op.W = W32; op.seg = SN; m->ops.push_back(op); }
  add_c2f(m, "model.12", View{cat11, 0, w[4] + w[3]}, v12, w[4] + w[3], w[3], dep[0], false, H16, W16, SN);
  { Op op; op.type = OP_UPSAMPLE; op.in = v12; op.out = View{cat14, 0, w[3]}; op.H = H16; op.W = W16; op.seg = SN; m->ops.push_back(op); }
  add_c2f(m, "model.15", View{cat14, 0, w[3] + w[2]}, View{b15, 0, w[2]}, w[3] + w[2], w[2], dep[0], false, H8, W8, SN);
  add_conv_reg(m, "model.16", View{b15, 0, w[2]}, View{cat17, 0, w[2]}, w[2], w[2], 3, 2, true, true, H8, W8, SN);
  add_c2f(m, "model.18", View{cat17, 0, w[2] + w[3]}, View{b18, 0, w[3]}, w[2] + w[3], w[3], dep[0], false, H16, W16, SN);
  add_conv_reg(m, "model.19", View{b18, 0, w[3]}, View{cat20, 0, w[3]}, w[3], w[3], 3, 2, true, true, H16, W16, SN);
  add_c2f(m, "model.21", View{cat20, 0, w[3] + w[4]}, View{b21, 0, w[4]}, w[3] + w[4], w[4], dep[0], false, H32, W32, SN);
  const int ch[3] = {w[2], w[3], w[4]};
  const int hh[3] = {H8, H16, H32}, ww[3] = {W8, W16, W32};
  const int pv[3] = {b15, b18, b21};
  return add_detect(m, "model.22", pv, ch, hh, ww, true, SH);
}

// Yolov11 detect (Yolo.cs:200-258): C3k2 backbone/neck (shortcut=true everywhere: C3k2's default), SPPF, C2PSA, Detect(legacy=false)
static int v11_widths(ys_model* m, int w[5], int* n, bool* uc) {
  static const float dm[5] = {0.5f, 0.5f, 0.5f, 1.0f, 1.0f};
  static const float wm[5] = {0.25f, 0.5f, 1.0f, 1.0f, 1.5f};
  static const int mc[5] = {1024, 1024, 512, 512, 768};
  static const bool c3k_sz[5] = {false, false, true, true, true};
  const int base_w[5] = {64, 128, 256, 512, 1024};
  const int sz = m->d.size;
  for (int i = 0; i < 5; i++) w[i] = std::min((int)(base_w[i] * wm[sz]), mc[sz]);
  *n = (int)(2 * dm[sz]);
  *uc = c3k_sz[sz];
  if (((int)(w[2] * 0.25f) / 2) % m->epl) {
    ys_set_error("model: YOLOv11 size %d needs hidden widths that are multiples of %d (use the f32 model for n)", sz, m->epl);
    return YS_ERR_UNSUPPORTED;
  }
  if ((w[4] / 2) % 64) { ys_set_error("model: C2PSA needs c %% 64 == 0"); return YS_ERR_UNSUPPORTED; }
  return YS_OK;
}

// Yolov11 model.0 - model.10 (Yolo.cs:216-227): C3k2 backbone, SPPF, C2PSA.  model.4 / model.6 / model.10 write the given views;
// backward segments s04 for model.0-4, s58 for model.5-8, s910 for model.9-10
static void v11_backbone(ys_model* m, const int* w, int n, bool uc, View v4, View v6, View v10, int s04, int s58, int s910) {
  const int H = m->d.height, W = m->d.width;
  const int H2 = H / 2, W2 = W / 2, H4 = H / 4, W4 = W / 4, H8 = H / 8, W8 = W / 8, H16 = H / 16, W16 = W / 16, H32 = H / 32, W32 = W / 32;
  const int SS = s04, SB = s58;
  const int b0 = new_buf(m, H2, W2, w[0]), b1 = new_buf(m, H4, W4, w[1]), b2 = new_buf(m, H4, W4, w[2]);
  const int b3 = new_buf(m, H8, W8, w[2]), b5 = new_buf(m, H16, W16, w[3]), b7 = new_buf(m, H32, W32, w[4]);
  const int b8 = new_buf(m, H32, W32, w[4]), b9 = new_buf(m, H32, W32, w[4]);
  int ci = add_conv_reg(m, "model.0", View{m->in_buf, 0, m->epl}, View{b0, 0, w[0]}, 3, w[0], 3, 2, true, true, H, W, SS);
  m->convs[ci].first = true;
  add_conv_reg(m, "model.1", View{b0, 0, w[0]}, View{b1, 0, w[1]}, w[0], w[1], 3, 2, true, true, H2, W2, SS);
  add_c3k2(m, "model.2", View{b1, 0, w[1]}, View{b2, 0, w[2]}, w[1], w[2], n, uc, 0.25f, H4, W4, SS);
  add_conv_reg(m, "model.3", View{b2, 0, w[2]}, View{b3, 0, w[2]}, w[2], w[2], 3, 2, true, true, H4, W4, SS);
  add_c3k2(m, "model.4", View{b3, 0, w[2]}, v4, w[2], w[3], n, uc, 0.25f, H8, W8, SS);
  add_conv_reg(m, "model.5", v4, View{b5, 0, w[3]}, w[3], w[3], 3, 2, true, true, H8, W8, SB);
  add_c3k2(m, "model.6", View{b5, 0, w[3]}, v6, w[3], w[3], n, true, 0.5f, H16, W16, SB);
  add_conv_reg(m, "model.7", v6, View{b7, 0, w[4]}, w[3], w[4], 3, 2, true, true, H16, W16, SB);
  add_c3k2(m, "model.8", View{b7, 0, w[4]}, View{b8, 0, w[4]}, w[4], w[4], n, true, 0.5f, H32, W32, SB);
  add_sppf(m, "model.9", View{b8, 0, w[4]}, View{b9, 0, w[4]}, w[4], H32, W32, s910);
  add_c2psa(m, "model.10", View{b9, 0, w[4]}, v10, w[4], n, H32, W32, s910);
}

// Yolov11Classify (Yolo.cs:556-573): the Yolov11 list without its last 13 modules -- model.0 - model.10, SPPF and C2PSA kept -- then
// Classify(widths[4], nc) as model.11
int build_v11_classify(ys_model* m) {
  int w[5], n; bool uc;
  YS_TRY(v11_widths(m, w, &n, &uc));
  const int H8 = m->d.height / 8, W8 = m->d.width / 8, H16 = m->d.height / 16, W16 = m->d.width / 16, H32 = m->d.height / 32, W32 = m->d.width / 32;
  new_input_buf(m);
  const int b4 = new_buf(m, H8, W8, w[3]), b6 = new_buf(m, H16, W16, w[3]), b10 = new_buf(m, H32, W32, w[4]);
  // backward segments: head (1280-channel Conv, pool, Linear), model.9-10, model.5-8, stem (model.0-4)
  v11_backbone(m, w, n, uc, View{b4, 0, w[3]}, View{b6, 0, w[3]}, View{b10, 0, w[4]}, 3, 2, 1);
  return add_classify(m, "model.11", View{b10, 0, w[4]}, w[4], H32, W32, 0);
}

int build_v11_detect(ys_model* m) {
  int w[5], n; bool uc;
  YS_TRY(v11_widths(m, w, &n, &uc));
  const ys_model_desc& d = m->d;
  const int H = d.height, W = d.width;
  const int H8 = H / 8, W8 = W / 8, H16 = H / 16, W16 = W / 16, H32 = H / 32, W32 = W / 32;
  new_input_buf(m);
  const int cat12 = new_buf(m, H16, W16, w[4] + w[3]);   // [up(L10) | L6]
  const int cat15 = new_buf(m, H8, W8, w[3] + w[3]);     // [up(L13) | L4]
  const int cat18 = new_buf(m, H16, W16, w[2] + w[3]);   // [L17 | L13]
  const int cat21 = new_buf(m, H32, W32, w[3] + w[4]);   // [L20 | L10]
  const int b16 = new_buf(m, H8, W8, w[2]), b19 = new_buf(m, H16, W16, w[3]), b22 = new_buf(m, H32, W32, w[4]);
  const View v4{cat15, w[3], w[3]}, v6{cat12, w[4], w[3]}, v10{cat21, w[3], w[4]}, v13{cat18, w[2], w[3]};
  const int SB = 2, SN = 1, SH = 0, SS = 3;   // stem segment: see build_v8_detect
  v11_backbone(m, w, n, uc, v4, v6, v10, SS, SB, SB);
  { Op op; op.type = OP_UPSAMPLE; op.in = v10; op.out = View{cat12, 0, w[4]}; op.H = H32; op.W = W32; op.seg = SN; m->ops.push_back(op); }
  add_c3k2(m, "model.13", View{cat12, 0, w[4] + w[3]}, v13, w[4] + w[3], w[3], n, uc, 0.5f, H16, W16, SN);
  { Op op; op.type = OP_UPSAMPLE; op.in = v13; op.out = View{cat15, 0, w[3]}; op.H = H16; op.W = W16; op.seg = SN; m->ops.push_back(op); }
  add_c3k2(m, "model.16", View{cat15, 0, w[3] + w[3]}, View{b16, 0, w[2]}, w[3] + w[3], w[2], n, uc, 0.5f, H8, W8, SN);
  add_conv_reg(m, "model.17", View{b16, 0, w[2]}, View{cat18, 0, w[2]}, w[2], w[2], 3, 2, true, true, H8, W8, SN);
  add_c3k2(m, "model.19", View{cat18, 0, w[2] + w[3]}, View{b19, 0, w[3]}, w[2] + w[3], w[3], n, uc, 0.5f, H16, W16, SN);
  add_conv_reg(m, "model.20", View{b19, 0, w[3]}, View{cat21, 0, w[3]}, w[3], w[3], 3, 2, true, true, H16, W16, SN);
  add_c3k2(m, "model.22", View{cat21, 0, w[3] + w[4]}, View{b22, 0, w[4]}, w[3] + w[4], w[4], n, true, 0.5f, H32, W32, SN);
  const int ch[3] = {w[2], w[3], w[4]};
  const int hh[3] = {H8, H16, H32}, ww[3] = {W8, W16, W32};
  const int pv[3] = {b16, b19, b22};
  return add_detect(m, "model.23", pv, ch, hh, ww, false, SH);
}

// Yolov5u detect (Yolo.cs:137-198): Conv(3, c, 6, 2, 2) stem, C3 backbone / neck, SPPF, Detect (the v8 head, legacy = true) as model.24.  Widths and depths are
// :147-158: int(w * width_multiple) with NO max_channels clamp, depths int(d * depth_multiple) in float arithmetic.  Skip router :139 outputIndexs
// {4, 6, 10, 14, 17, 20, 23} with Yolov8's concatIndex {1, 0, 3, 2}: cat12 = [up(L10) | L6], cat16 = [up(L14) | L4], cat19 = [L18 | L14], cat22 = [L21 | L10]
int build_v5u_detect(ys_model* m) {
  static const float dm[5] = {0.34f, 0.34f, 0.67f, 1.0f, 1.34f};
  static const float wm[5] = {0.25f, 0.5f, 0.75f, 1.0f, 1.25f};
  const int base_w[5] = {64, 128, 256, 512, 1024};
  const ys_model_desc& d = m->d;
  int w[5], dep[3];
  for (int i = 0; i < 5; i++) w[i] = (int)(base_w[i] * wm[d.size]);
  dep[0] = (int)(3 * dm[d.size]); dep[1] = (int)(6 * dm[d.size]); dep[2] = (int)(9 * dm[d.size]);
  for (int i = 0; i < 5; i++)
    if (w[i] % m->epl || ((int)(w[i] * 0.5f)) % m->epl) { ys_set_error("model: width %d not a multiple of %d", w[i], m->epl); return YS_ERR_UNSUPPORTED; }
  const int H = d.height, W = d.width;
  const int H2 = H / 2, W2 = W / 2, H4 = H / 4, W4 = W / 4, H8 = H / 8, W8 = W / 8, H16 = H / 16, W16 = W / 16, H32 = H / 32, W32 = W / 32;
  new_input_buf(m);
  const int cat12 = new_buf(m, H16, W16, w[3] + w[3]);   // [up(L10) | L6]
  const int cat16 = new_buf(m, H8, W8, w[2] + w[2]);     // [up(L14) | L4]
  const int cat19 = new_buf(m, H16, W16, w[2] + w[2]);   // [L18 | L14]
  const int cat22 = new_buf(m, H32, W32, w[3] + w[3]);   // [L21 | L10]
  const int b0 = new_buf(m, H2, W2, w[0]), b1 = new_buf(m, H4, W4, w[1]), b2 = new_buf(m, H4, W4, w[1]);
  const int b3 = new_buf(m, H8, W8, w[2]), b5 = new_buf(m, H16, W16, w[3]), b7 = new_buf(m, H32, W32, w[4]);
  const int b8 = new_buf(m, H32, W32, w[4]), b9 = new_buf(m, H32, W32, w[4]), b13 = new_buf(m, H16, W16, w[3]);
  const int b17 = new_buf(m, H8, W8, w[2]), b20 = new_buf(m, H16, W16, w[3]), b23 = new_buf(m, H32, W32, w[4]);
  const View v4{cat16, w[2], w[2]}, v6{cat12, w[3], w[3]}, v10{cat22, w[3], w[3]}, v14{cat19, w[2], w[2]};
  const int SB = 2, SN = 1, SH = 0, SS = 3;   // backward segments: see build_v8_detect
  int ci = add_conv_reg(m, "model.0", View{m->in_buf, 0, m->epl}, View{b0, 0, w[0]}, 3, w[0], 6, 2, true, true, H, W, SS, nullptr, false, 2);
  m->convs[ci].first = true;
  add_conv_reg(m, "model.1", View{b0, 0, w[0]}, View{b1, 0, w[1]}, w[0], w[1], 3, 2, true, true, H2, W2, SS);
  add_c3(m, "model.2", View{b1, 0, w[1]}, View{b2, 0, w[1]}, w[1], w[1], dep[0], true, H4, W4, SS);
  add_conv_reg(m, "model.3", View{b2, 0, w[1]}, View{b3, 0, w[2]}, w[1], w[2], 3, 2, true, true, H4, W4, SS);
  add_c3(m, "model.4", View{b3, 0, w[2]}, v4, w[2], w[2], dep[1], true, H8, W8, SS);
  add_conv_reg(m, "model.5", v4, View{b5, 0, w[3]}, w[2], w[3], 3, 2, true, true, H8, W8, SB);
  add_c3(m, "model.6", View{b5, 0, w[3]}, v6, w[3], w[3], dep[2], true, H16, W16, SB);
  add_conv_reg(m, "model.7", v6, View{b7, 0, w[4]}, w[3], w[4], 3, 2, true, true, H16, W16, SB);
  add_c3(m, "model.8", View{b7, 0, w[4]}, View{b8, 0, w[4]}, w[4], w[4], dep[0], true, H32, W32, SB);
  add_sppf(m, "model.9", View{b8, 0, w[4]}, View{b9, 0, w[4]}, w[4], H32, W32, SB);
  add_conv_reg(m, "model.10", View{b9, 0, w[4]}, v10, w[4], w[3], 1, 1, true, true, H32, W32, SN);
  { Op op; op.type = OP_UPSAMPLE; op.in = v10; op.out = View{cat12, 0, w[3]}; op.H = H32; op.W = W32; op.seg = SN; m->ops.push_back(op); }
  add_c3(m, "model.13", View{cat12, 0, 2 * w[3]}, View{b13, 0, w[3]}, w[4], w[3], dep[0], false, H16, W16, SN);
  add_conv_reg(m, "model.14", View{b13, 0, w[3]}, v14, w[3], w[2], 1, 1, true, true, H16, W16, SN);
  { Op op; op.type = OP_UPSAMPLE; op.in = v14; op.out = View{cat16, 0, w[2]}; op.H = H16; op.W = W16; op.seg = SN; m->ops.push_back(op); }
  add_c3(m, "model.17", View{cat16, 0, 2 * w[2]}, View{b17, 0, w[2]}, w[3], w[2], dep[0], false, H8, W8, SN);
  add_conv_reg(m, "model.18", View{b17, 0, w[2]}, View{cat19, 0, w[2]}, w[2], w[2], 3, 2, true, true, H8, W8, SN);
  add_c3(m, "model.20", View{cat19, 0, 2 * w[2]}, View{b20, 0, w[3]}, w[3], w[3], dep[0], false, H16, W16, SN);
  add_conv_reg(m, "model.21", View{b20, 0, w[3]}, View{cat22, 0, w[3]}, w[3], w[3], 3, 2, true, true, H16, W16, SN);
  add_c3(m, "model.23", View{cat22, 0, 2 * w[3]}, View{b23, 0, w[4]}, w[4], w[4], dep[0], false, H32, W32, SN);
  const int ch[3] = {w[2], w[3], w[4]};
  const int hh[3] = {H8, H16, H32}, ww[3] = {W8, W16, W32};
  const int pv[3] = {b17, b20, b23};
  return add_detect(m, "model.24", pv, ch, hh, ww, true, SH);
}

// Standalone block graph (ys_block_create): input buffer -> one module -> output buffer.  Modules are built with the
// prefix "block" and the tensor names are made module-relative afterwards (layout_block_names).
int build_block(ys_model* m, const ys_block_desc& bd) {
  const int epl = m->epl, H = bd.height, W = bd.width, c1 = bd.c1, c2 = bd.c2;
  auto bad = [&](int v, const char* what) {
    if (v > 0 && v % epl == 0) return false;
    ys_set_error("ys_block_create: %s = %d must be a positive multiple of %d for this dtype", what, v, epl);
    return true;
  };
  if (bad(c1, "c1") || bad(c2, "c2")) return YS_ERR_UNSUPPORTED;
  const float e = bd.e > 0.f ? bd.e : 0.5f;
  m->in_buf = new_buf(m, H, W, c1);
  const View vin{m->in_buf, 0, c1};
  int Ho = H, Wo = W;
  if (bd.kind == YS_BLOCK_CONV) {
    if ((bd.k != 1 && bd.k != 3) || (bd.s != 1 && bd.s != 2)) { ys_set_error("ys_block_create: Conv k=%d s=%d unsupported (k in {1,3}, s in {1,2})", bd.k, bd.s); return YS_ERR_UNSUPPORTED; }
    const int p = bd.k / 2;
    Ho = (H + 2 * p - bd.k) / bd.s + 1; Wo = (W + 2 * p - bd.k) / bd.s + 1;
  } else if (bd.kind == YS_BLOCK_PROTO) {
    Ho = 2 * H; Wo = 2 * W;
  }
  m->blk_out = new_buf(m, Ho, Wo, c2);
  const View vout{m->blk_out, 0, c2};
  const std::string nm = "block";
  switch (bd.kind) {
    case YS_BLOCK_CONV:
      add_conv_reg(m, nm, vin, vout, c1, c2, bd.k, bd.s, true, bd.act != 0, H, W, 0);
      break;
    case YS_BLOCK_BOTTLENECK: {
      if (c1 != c2) { ys_set_error("ys_block_create: Bottleneck needs c1 == c2 (the graphs' only use)"); return YS_ERR_UNSUPPORTED; }
      if (bad((int)(c2 * e), "Bottleneck hidden width")) return YS_ERR_UNSUPPORTED;
      auto pr = add_bottleneck(m, nm, vin, vout, c2, e, bd.shortcut != 0, H, W, 0);
      m->reg.push_back(pr.first); m->reg.push_back(pr.second);
      break;
    }
    case YS_BLOCK_C2F:
      if (bd.n < 1 || bad((int)(c2 * 0.5f), "C2f hidden width")) { if (bd.n < 1) ys_set_error("ys_block_create: n = %d", bd.n); return YS_ERR_UNSUPPORTED; }
      add_c2f(m, nm, vin, vout, c1, c2, bd.n, bd.shortcut != 0, H, W, 0);
      break;
    case YS_BLOCK_C3:
      if (bd.n < 1) { ys_set_error("ys_block_create: n = %d", bd.n); return YS_ERR_UNSUPPORTED; }
      if (bad((int)(c2 * 0.5f), "C3 hidden width")) return YS_ERR_UNSUPPORTED;
      add_c3(m, nm, vin, vout, c1, c2, bd.n, bd.shortcut != 0, H, W, 0);
      break;
    case YS_BLOCK_C3K2: {
      const int c = (int)(c2 * e);
      if (bd.n < 1) { ys_set_error("ys_block_create: n = %d", bd.n); return YS_ERR_UNSUPPORTED; }
      if (bad(c, "C3k2 hidden width") || bad((int)(c * 0.5f), "C3k2 inner hidden width")) return YS_ERR_UNSUPPORTED;
      add_c3k2(m, nm, vin, vout, c1, c2, bd.n, bd.c3k != 0, e, H, W, 0);
      break;
    }
    case YS_BLOCK_SPPF:
      if (c1 != c2) { ys_set_error("ys_block_create: SPPF needs c1 == c2 (the graphs' only use)"); return YS_ERR_UNSUPPORTED; }
      if (bad(c1 / 2, "SPPF hidden width")) return YS_ERR_UNSUPPORTED;
      add_sppf(m, nm, vin, vout, c1, H, W, 0);
      break;
    case YS_BLOCK_C2PSA:
      if (c1 != c2 || (c1 / 2) % 64 || bd.n < 1) { ys_set_error("ys_block_create: C2PSA needs c1 == c2, (c1/2) %% 64 == 0 and n >= 1"); return YS_ERR_UNSUPPORTED; }
      add_c2psa(m, nm, vin, vout, c1, bd.n, H, W, 0);
      break;
    case YS_BLOCK_PROTO: {
      if (bad(bd.n, "Proto hidden width (n)")) return YS_ERR_UNSUPPORTED;
      // add_proto allocates its own output buffer: use it as the block output
      m->bufs.pop_back();
      m->blk_out = add_proto(m, nm, vin, c1, bd.n, c2, H, W, 0);
      break;
    }
    default:
      ys_set_error("ys_block_create: unknown block kind %d", bd.kind);
      return YS_ERR_INVALID_ARG;
  }
  return YS_OK;
}

}  // namespace ysm
