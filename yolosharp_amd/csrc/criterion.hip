// criterion.hip -- the criterion, End2End setup and output accessors of a model handle (ys_model.h): ys_model_get_output / _set_preds, the
// ys_model_*e2e* / one2one entries, ys_model_reserve_labels and the ys_loss_* ABI (ys_loss_read_targets: the assignment, for tests).  Host code only: the kernels are loss.hip, segloss.hip, poseloss.hip,
// classify.hip and e2e.hip, reached through their launchers (ys_kernels.h).  Of the other units of the handle it uses the fields, and plan.hip's dev_alloc and alloc_label_ws.
//
// Criteria (Utils/Loss.cs): v8DetectionLoss :330-484, v8OBBLoss :486-684, v8SegmentationLoss :711-780, v8PoseLoss :870-1071, v8ClassificationLoss
// :1073-1091 and, over the aliased one2one towers of an End2End model (Modules/Head.cs:89-127, 152-167), E2EDetectLoss :1094-1118, E2EOBBLoss :1120-1177,
// E2ESegmentLoss :1179-1236, E2EPoseLoss :1238-1295: two passes of the task's criterion over the SAME head outputs, the second with its own gradient and scalar buffers.
#include "ys_model.h"
#include <cmath>
#include <cstring>
#include <algorithm>

using ysm::dev_alloc;
using ysm::alloc_label_ws;

extern "C" {

// ys_model_get_output: the head outputs that are one unpack of a head buffer.  head = ys_model::xkind of the model that has the key (0: every model);
// buf = the buffer read, which also fixes the shape [B][C][rows]; grad: the criterion's gradient instead of the activations (needs that criterion to have
// run); o2o: a key of the one2one branch (End2End models only) -- its values ARE the one2many ones (aliased towers read the same input, Head.cs:94-96,
// 152-167), its gradients are the second criterion pass's own buffers; angle: Obb.forward_head's (sigmoid - 0.25) * pi over the unpacked logits (Head.cs:421-433).
enum { OUT_PD, OUT_PS, OUT_MC, OUT_PR };   // boxes [4*reg_max][A], scores [nc][A], cv4 = coefficients | angle logit | raw kpts [nm][A], prototypes [nm][mh*mw] (Head.cs:289-296, 531-543)
struct OutKey { const char* key; int head, buf; bool grad, o2o, angle; };
static const OutKey OUT_KEYS[] = {
  {"boxes", 0, OUT_PD, false, false, false},               {"scores", 0, OUT_PS, false, false, false},
  {"dboxes", 0, OUT_PD, true, false, false},               {"dscores", 0, OUT_PS, true, false, false},
  {"one2one_boxes", 0, OUT_PD, false, true, false},        {"one2one_scores", 0, OUT_PS, false, true, false},
  {"one2one_dboxes", 0, OUT_PD, true, true, false},        {"one2one_dscores", 0, OUT_PS, true, true, false},
  {"mask_coefficient", 1, OUT_MC, false, false, false},    {"dmask_coefficient", 1, OUT_MC, true, false, false},
  {"one2one_mask_coefficient", 1, OUT_MC, false, true, false}, {"one2one_dmask_coefficient", 1, OUT_MC, true, true, false},
  {"proto", 1, OUT_PR, false, false, false},               {"dproto", 1, OUT_PR, true, false, false},
  {"angle", 2, OUT_MC, false, false, true},                {"dangle", 2, OUT_MC, true, false, false},     // the gradients are w.r.t. the raw kpts | the angle LOGIT
  {"one2one_angle", 2, OUT_MC, false, true, true},         {"one2one_dangle", 2, OUT_MC, true, true, false},
  {"kpts", 3, OUT_MC, false, false, false},                {"dkpts", 3, OUT_MC, true, false, false},
  {"one2one_kpts", 3, OUT_MC, false, true, false},         {"one2one_dkpts", 3, OUT_MC, true, true, false},
};

int ys_model_get_output(ys_model* m, const char* key, float* host, size_t count) {
  YS_REQUIRE(m && key && host, "ys_model_get_output: null argument");
  YS_REQUIRE(!m->is_block, "ys_model_get_output: this handle is a block (use ys_block_forward / ys_block_backward)");
  YS_REQUIRE(m->have_fwd, "ys_model_get_output: no forward has run");
  hipStream_t st = m->ctx->stream;
  const int B = m->B;
  const std::string k(key);
  const bool cls_key = k == "cls" || k == "dcls" || k == "logits";
  if (m->cls != cls_key) {
    ys_set_error(m->cls ? "ys_model_get_output: a classify model has the outputs \"cls\", \"logits\" and \"dcls\" (not '%s')"
                        : "ys_model_get_output: '%s' is an output of classify models only", key);
    return YS_ERR_INVALID_ARG;
  }
  if (cls_key) {
    // Classify.forward (Head.cs:635-643): "cls" = logits in training, softmax(logits, 1) in eval; "logits" = the logits in both modes;
    // "dcls" = d(loss) / d(logits) after ys_loss_classify.  All [B, nc].
    YS_REQUIRE(count == (size_t)B * m->d.nc, "ys_model_get_output(%s): expected %zu elements", key, (size_t)B * m->d.nc);
    YS_REQUIRE(k != "dcls" || m->have_loss, "ys_model_get_output(dcls): no loss has run");
    if (k == "cls" && !m->fwd_training) {
      YS_CHECK_HIP(hipMemcpyAsync(host, m->pred, count * 4, hipMemcpyDeviceToHost, st));
    } else {
      const Buf& b = m->bufs[m->logit_buf];
      YS_TRY(ys_unpack_nchw_launch(st, m->dtype, k == "dcls" ? b.grad : b.act, b.ldc, 0, B, m->d.nc, 1, m->out_stage));
      YS_CHECK_HIP(hipMemcpyAsync(host, m->out_stage, count * 4, hipMemcpyDeviceToHost, st));
    }
  } else if (k == "model0_raw" || k == "model0_dy") {
    // model.0 after a training-mode forward, [B, c, H/2, W/2] as stored: "model0_raw" its raw (pre-BatchNorm) output, "model0_dy" -- after the backward -- the
    // gradient w.r.t. that output, i.e. the two operands its weight gradient is formed from.  What the stem routes (conv_stem.hip / conv_stem6.hip against the
    // packed copy + generic kernels) are compared on.  model.0 is the last unit of the backward: nothing overwrites its dy before the next backward
    YS_REQUIRE(!m->is_head && !m->convs.empty() && m->convs[0].first && m->convs[0].bn, "ys_model_get_output(%s): not a full model", key);
    YS_REQUIRE(m->fwd_training && m->training, "ys_model_get_output(%s): the last forward did not run in training mode", key);
    const ConvL& c = m->convs[0];
    const bool want_dy = k == "model0_dy";
    YS_REQUIRE(!want_dy || !ysm::stem_bnb_planned(m), "ys_model_get_output(model0_dy): this model forms model.0's dy inside its weight-gradient kernel (STEM_BNB_FUSE)");
    if (want_dy) YS_TRY(ysm::join_wgrad_stream(m));
    const long rpb = (long)c.Hout * c.Wout;
    YS_REQUIRE(count == (size_t)B * c.cout * rpb, "ys_model_get_output(%s): expected %zu elements", key, (size_t)B * c.cout * rpb);
    const void* src = want_dy ? ((m->overlap && c.dy_own) ? c.dy_own : m->dy_scratch) : (const void*)((const char*)m->y_all + (size_t)c.y_off * m->es);
    float* tmp = nullptr;
    YS_CHECK_HIP(hipMalloc((void**)&tmp, count * 4));
    int rc = ys_unpack_nchw_launch(st, m->dtype, src, c.cout, 0, B, c.cout, rpb, tmp);
    if (rc == YS_OK && hipMemcpyAsync(host, tmp, count * 4, hipMemcpyDeviceToHost, st) != hipSuccess) rc = YS_ERR_HIP;
    if (hipStreamSynchronize(st) != hipSuccess && rc == YS_OK) rc = YS_ERR_HIP;
    (void)hipFree(tmp);
    if (rc != YS_OK) return rc;
  } else if (k == "det") {
    // End2End eval forward: Detect.postprocess (Head.cs:117-127) -> [B, k, 6] = (x1, y1, x2, y2, score, class), k = min(max_det, A); End2End Segment: + the
    // nm mask coefficients of the anchor (Head.cs:321-339); OBB: + the angle (Head.cs:439-452); Pose: + the nk decoded keypoint values (Head.cs:550-563)
    YS_REQUIRE(m->e2e, "ys_model_get_output(det): not an End2End model (ys_model_one2one_init)");
    YS_REQUIRE(!m->fwd_training && !m->training, "ys_model_get_output(det): the last forward ran in training mode");
    const size_t n = (size_t)B * std::min(m->max_det, m->A) * (6 + m->nm);
    YS_REQUIRE(count == n, "ys_model_get_output(det): expected %zu elements", n);
    YS_CHECK_HIP(hipMemcpyAsync(host, m->det_rows, count * 4, hipMemcpyDeviceToHost, st));
  } else if (k == "pred") {
    const size_t pc = (size_t)(4 + m->d.nc + m->nm);
    YS_REQUIRE(!m->training, "ys_model_get_output(pred): model is in training mode (Detect returns preds only, Head.cs:103-106)");
    YS_REQUIRE(count == (size_t)B * pc * m->A, "ys_model_get_output(pred): expected %zu elements", (size_t)B * pc * m->A);
    YS_CHECK_HIP(hipMemcpyAsync(host, m->pred, count * 4, hipMemcpyDeviceToHost, st));
  } else {
    const int head = m->segment ? 1 : m->xkind;
    const OutKey* e = nullptr;
    for (const OutKey& r : OUT_KEYS) if (k == r.key && (r.head == 0 || r.head == head)) e = &r;
    if (!e) { ys_set_error("ys_model_get_output: unknown key '%s'", key); return YS_ERR_INVALID_ARG; }
    const int bufs[4] = {m->pd_buf, m->ps_buf, m->mc_buf, m->pr_buf};
    void* const o2o_grad[4] = {m->o2o_dpd, m->o2o_dps, m->o2o_dmc, nullptr};
    const int C = e->buf == OUT_PD ? 4 * m->d.reg_max : e->buf == OUT_PS ? m->d.nc : m->nm;
    const long rows = e->buf == OUT_PR ? (long)m->mh * m->mw : m->A;
    const bool ran = e->buf == OUT_PD || e->buf == OUT_PS ? m->have_loss : m->have_seg_loss;   // cv4 / Proto gradients come from the task's own criterion
    YS_REQUIRE(!e->o2o || m->e2e, "ys_model_get_output(%s): not an End2End model (%s)", key,
               head == 1 ? "ys_model_e2e_init" : head == 2 ? "ys_model_e2e_obb_init" : head == 3 ? "ys_model_e2e_pose_init" : "ys_model_one2one_init");
    YS_REQUIRE(!e->grad || ran, "ys_model_get_output(%s): the model's criterion has not run", key);
    YS_REQUIRE(count == (size_t)B * C * rows, "ys_model_get_output(%s): expected %zu elements", key, (size_t)B * C * rows);
    const Buf& b = m->bufs[bufs[e->buf]];
    YS_TRY(ys_unpack_nchw_launch(st, m->dtype, !e->grad ? b.act : e->o2o ? o2o_grad[e->buf] : b.grad, b.ldc, 0, B, C, rows, m->out_stage));
    if (e->angle) YS_TRY(ys_obb_angle_launch(st, m->out_stage, (long)count));
    YS_CHECK_HIP(hipMemcpyAsync(host, m->out_stage, count * 4, hipMemcpyDeviceToHost, st));
  }
  YS_CHECK_HIP(hipStreamSynchronize(st));
  return YS_OK;
}

// The criterion's `preds` argument supplied by the caller (Loss.cs:411 `forward(preds, batch)`): head outputs in the reference layout
// -- boxes [B, 4*reg_max, A], scores [B, nc, A] and, for Segment models, mask_coefficient [B, nm, A] and proto [B, nm, H/4, W/4] --
// are packed into the engine's head buffers as if a forward had produced them.  ys_loss_detect / ys_loss_segment and the
// "dboxes" / "dscores" / ... gradient outputs then work on them; ys_model_backward is refused (no graph state behind these preds).
int ys_model_set_preds(ys_model* m, int batch, const float* boxes, const float* scores, const float* mask_coefficient, const float* proto) {
  YS_REQUIRE(m && !m->is_block && boxes && scores, "ys_model_set_preds: null argument or block handle");
  YS_REQUIRE(!m->cls, "ys_model_set_preds: a classify model has no detection outputs (its criterion is ys_loss_classify)");
  YS_REQUIRE(batch > 0 && batch <= m->maxB, "ys_model_set_preds: batch %d outside (0, %d]", batch, m->maxB);
  YS_REQUIRE(!m->segment || (mask_coefficient && proto), "ys_model_set_preds: a Segment model needs mask_coefficient and proto");
  YS_REQUIRE(m->xkind < 2 || mask_coefficient, "ys_model_set_preds: a Pose / Obb model takes its raw kpts [B,nk,A] / angle LOGITS [B,1,A] in the mask_coefficient argument");
  YS_CHECK_HIP(hipSetDevice(m->ctx->device));
  hipStream_t st = m->ctx->stream;
  struct Item { const float* src; int buf; int C; long rows; } items[4] = {
    {boxes, m->pd_buf, 4 * m->d.reg_max, m->A}, {scores, m->ps_buf, m->d.nc, m->A},
    {m->segment || m->xkind >= 2 ? mask_coefficient : nullptr, m->mc_buf, m->nm, m->A}, {m->segment ? proto : nullptr, m->pr_buf, m->nm, (long)m->mh * m->mw}};
  for (const Item& it : items) {
    if (!it.src) continue;
    const Buf& b = m->bufs[it.buf];
    const size_t cnt = (size_t)batch * it.C * it.rows;
    YS_REQUIRE((long)cnt <= m->n_out_stage, "ys_model_set_preds: staging buffer too small");
    YS_CHECK_HIP(hipMemcpyAsync(m->out_stage, it.src, cnt * 4, hipMemcpyHostToDevice, st));
    YS_TRY(ys_pack_input_launch(st, m->dtype, m->out_stage, batch, it.C, 1, (int)it.rows, b.ldc, b.act));
    YS_CHECK_HIP(hipStreamSynchronize(st));   // out_stage is reused by the next item
  }
  m->B = batch; m->have_fwd = true; m->fwd_training = false; m->have_loss = false; m->have_seg_loss = false;
  return YS_OK;
}

// The tail of an eval forward alone (ysm::eval_tail): `pred` (and "det") from the head buffers as they stand -- after ys_model_set_preds the decode of
// values the caller chose, after an eval forward the same `pred` again.
int ys_model_decode_preds(ys_model* m) {
  YS_REQUIRE(m, "ys_model_decode_preds: null argument");
  YS_REQUIRE(!m->is_block && !m->cls && m->pd_buf >= 0, "ys_model_decode_preds: not a detection-family model (block handles and classify models have no decode)");
  YS_REQUIRE(!m->training, "ys_model_decode_preds: model is in training mode (Detect returns preds only, Head.cs:103-106)");
  YS_REQUIRE(m->have_fwd, "ys_model_decode_preds: needs ys_model_set_preds or a forward first");
  YS_CHECK_HIP(hipSetDevice(m->ctx->device));
  YS_TRY(ysm::eval_tail(m, m->B));
  YS_CHECK_HIP(hipGetLastError());
  return YS_OK;
}

int ys_model_pred_device(ys_model* m, float** dptr) {
  YS_REQUIRE(m && dptr, "null argument");
  *dptr = m->pred;
  return YS_OK;
}

// YoloBaseTaskModel.One2one_Init -> Detect.one2one_init (Head.cs:152-167): the one2one towers are the SAME Sequential objects as cv2 / cv3
// (CopyTo copies references), so the model gains no tensor -- only the second criterion pass's gradient / scalar buffers, the snapshot of
// the towers' running statistics (their second momentum update) and the top-k output of the eval forward.  Segment.one2one_init (Head.cs:245-357) and
// Obb.one2one_init (Head.cs:454-469) and Pose.one2one_init (Head.cs:565-580) alias cv4 as well; their criteria carry the gain schedule of `epochs` steps (Loss.cs:1138-1148, 1197-1207).
// tasks: bit t = the entry accepts full models of ys_task t; the check order is unsupported handle, then second call.
static int e2e_init(ys_model* m, int max_det, int epochs, unsigned tasks, const char* entry, const char* refusal) {
  const bool full = !m->is_block && !m->is_head && !m->cls && m->pd_buf >= 0 && (m->d.task == YS_DETECT || m->mc_buf >= 0);
  if (!full || !((tasks >> m->d.task) & 1u)) { ys_set_error("%s: %s", entry, refusal); return YS_ERR_UNSUPPORTED; }
  if (m->e2e) { ys_set_error("%s: already initialised", entry); return YS_ERR_STATE; }
  const bool cv4 = m->segment || m->xkind >= 2;
  YS_CHECK_HIP(hipSetDevice(m->ctx->device));
  const int B = m->maxB;
  m->max_det = max_det > 0 ? max_det : 300;     // Detect.max_det (Head.cs:13)
  const int k = std::min(m->max_det, m->A);
  const Buf &pb = m->bufs[m->pd_buf], &sb = m->bufs[m->ps_buf];
  YS_TRY(dev_alloc(m, &m->o2o_dpd, (size_t)B * pb.rows_per_b * pb.ldc * m->es));
  YS_TRY(dev_alloc(m, &m->o2o_dps, (size_t)B * sb.rows_per_b * sb.ldc * m->es));
  if (cv4) { const Buf& cb = m->bufs[m->mc_buf]; YS_TRY(dev_alloc(m, &m->o2o_dmc, (size_t)B * cb.rows_per_b * cb.ldc * m->es)); }
  YS_TRY(dev_alloc(m, (void**)&m->scalars2, 64 * 4 + 64 * 8 * 8));
  YS_TRY(dev_alloc(m, (void**)&m->det_rows, (size_t)B * k * (6 + m->nm) * 4));
  YS_TRY(dev_alloc(m, (void**)&m->det_anchor, (size_t)B * k * 8));
  YS_TRY(dev_alloc(m, &m->det_ws, ys_e2e_topk_ws_bytes(B, m->d.nc, m->A, m->max_det)));
  // the towers' BatchNorm state as contiguous runs of `state`.  A Detect head's units are the last of `convs` and their state is the tail of `state`: one
  // run.  In a Segment head Proto's units sit between cv3 and cv4; Proto runs once per forward (Head.cs:283-307), so its words are in no run.
  std::vector<std::pair<long, long>> iv;        // [begin, end) words of every tower unit
  for (size_t i = (size_t)m->head_conv0; i < m->convs.size(); i++) {
    const ConvL& c = m->convs[i];
    if (!c.bn || c.proto) continue;
    iv.push_back({c.rm_off, c.rm_off + c.cout}); iv.push_back({c.rv_off, c.rv_off + c.cout}); iv.push_back({c.nbt_off, c.nbt_off + 1});
  }
  std::sort(iv.begin(), iv.end());
  m->n_hstate_rng = 0; m->n_hstate = 0;
  for (auto& v : iv) {
    if (m->n_hstate_rng > 0 && m->hstate_rng[m->n_hstate_rng - 1].off + m->hstate_rng[m->n_hstate_rng - 1].count == v.first) { m->hstate_rng[m->n_hstate_rng - 1].count += v.second - v.first; }
    else {
      if (m->n_hstate_rng == 4) { ys_set_error("ys_model_e2e_init: internal: the towers' statistics lie in more than 4 runs of the state"); return YS_ERR_STATE; }
      m->hstate_rng[m->n_hstate_rng++] = ys_model::Range{v.first, v.second - v.first};
    }
    m->n_hstate += v.second - v.first;
  }
  for (int i = 0; i < (int)m->convs.size(); i++) {          // no other unit's state inside a run
    const ConvL& c = m->convs[i];
    if (!c.bn || (i >= m->head_conv0 && !c.proto)) continue;
    for (int r = 0; r < m->n_hstate_rng; r++)
      if (c.rm_off < m->hstate_rng[r].off + m->hstate_rng[r].count && c.nbt_off >= m->hstate_rng[r].off) { ys_set_error("ys_model_e2e_init: internal: %s lies inside the towers' statistics", c.name.c_str()); return YS_ERR_STATE; }
  }
  if (m->n_hstate > 0) {
    std::vector<unsigned char> isc((size_t)m->n_hstate, 0);
    long so = 0;
    for (int r = 0; r < m->n_hstate_rng; r++) {
      for (size_t i = (size_t)m->head_conv0; i < m->convs.size(); i++) {
        const ConvL& c = m->convs[i];
        if (c.bn && !c.proto && c.nbt_off >= m->hstate_rng[r].off && c.nbt_off < m->hstate_rng[r].off + m->hstate_rng[r].count) isc[(size_t)(so + c.nbt_off - m->hstate_rng[r].off)] = 1;
      }
      so += m->hstate_rng[r].count;
    }
    YS_TRY(dev_alloc(m, (void**)&m->hstate_snap, (size_t)m->n_hstate * 4));
    YS_TRY(dev_alloc(m, (void**)&m->hstate_count, (size_t)m->n_hstate));
    YS_CHECK_HIP(hipMemcpyAsync(m->hstate_count, isc.data(), isc.size(), hipMemcpyHostToDevice, m->ctx->stream));
    YS_CHECK_HIP(hipStreamSynchronize(m->ctx->stream));
  }
  m->e2e = true;
  if (cv4) { m->e2e_epochs = epochs > 0 ? epochs : 100; m->e2e_updates = 0; m->o2m = 0.8f; m->o2o = 1.0f - 0.8f; }
  m->have_fwd = false; m->have_loss = false; m->have_seg_loss = false;      // "pred" changes its box format: a forward from before the switch is not an End2End one
  return YS_OK;
}

int ys_model_one2one_init(ys_model* m, int max_det) {
  YS_REQUIRE(m, "ys_model_one2one_init: null model");
  YS_REQUIRE(max_det >= 0, "ys_model_one2one_init: max_det = %d", max_det);
  return e2e_init(m, max_det, 0, 1u << YS_DETECT, "ys_model_one2one_init",
                  "End2End through this entry is built for full Detect models (Segment models: ys_model_e2e_init; OBB models: ys_model_e2e_obb_init; Pose models: ys_model_e2e_pose_init; the standalone heads are not built)");
}

// One2one_Init for Detect AND Segment models (Models/Segmenter.cs:17-24).  epochs: ignored by Detect models, whose criterion is unweighted.
int ys_model_e2e_init(ys_model* m, int max_det, int epochs) {
  YS_REQUIRE(m, "ys_model_e2e_init: null model");
  YS_REQUIRE(max_det >= 0 && epochs >= 0, "ys_model_e2e_init: max_det = %d, epochs = %d", max_det, epochs);
  return e2e_init(m, max_det, epochs, 1u << YS_DETECT | 1u << YS_SEGMENT, "ys_model_e2e_init",
                  "this entry is One2one_Init for full Detect and Segment models (OBB models: ys_model_e2e_obb_init; Pose models: ys_model_e2e_pose_init; the standalone heads are not built)");
}

// One2one_Init for OBB models (Models/Obber.cs:18-24).  An entry of its own: ys_model_one2one_init and ys_model_e2e_init keep refusing OBB models.
int ys_model_e2e_obb_init(ys_model* m, int max_det, int epochs) {
  YS_REQUIRE(m, "ys_model_e2e_obb_init: null model");
  YS_REQUIRE(max_det >= 0 && epochs >= 0, "ys_model_e2e_obb_init: max_det = %d, epochs = %d", max_det, epochs);
  return e2e_init(m, max_det, epochs, 1u << YS_OBB, "ys_model_e2e_obb_init",
                  "this entry is One2one_Init for full OBB models (Detect: ys_model_one2one_init; Segment: ys_model_e2e_init; Pose: ys_model_e2e_pose_init)");
}

// One2one_Init for Pose models (Models/PoseDetector.cs:21-36).  An entry of its own: the three entries above keep refusing Pose models.
int ys_model_e2e_pose_init(ys_model* m, int max_det, int epochs) {
  YS_REQUIRE(m, "ys_model_e2e_pose_init: null model");
  YS_REQUIRE(max_det >= 0 && epochs >= 0, "ys_model_e2e_pose_init: max_det = %d, epochs = %d", max_det, epochs);
  return e2e_init(m, max_det, epochs, 1u << YS_POSE, "ys_model_e2e_pose_init",
                  "this entry is One2one_Init for full Pose models (Detect: ys_model_one2one_init; Segment: ys_model_e2e_init; OBB: ys_model_e2e_obb_init)");
}

// E2ESegmentLoss.update() (Loss.cs:1225-1235), E2EOBBLoss.update() (Loss.cs:1166-1176) and E2EPoseLoss.update() (Loss.cs:1284-1294), the same chain.  The reference's training loop calls update() for
// E2EOBBLoss only (YoloBaseTaskModel.cs:350-353; E2EPoseLoss is a class of its own), so a Segment or Pose run of the reference keeps 0.8 / 0.2 for its whole life; callers that want the schedule call this once per epoch.
int ys_model_e2e_update(ys_model* m) {
  YS_REQUIRE(m, "ys_model_e2e_update: null model");
  YS_REQUIRE(m->e2e, "ys_model_e2e_update: not an End2End model (ys_model_e2e_init)");
  if (!m->e2e_cv4()) return YS_OK;  // E2EDetectLoss has no gains
  m->e2e_updates += 1;
  const int den = m->e2e_epochs - 1 > 1 ? m->e2e_epochs - 1 : 1;
  const float r = 1.0f - (float)m->e2e_updates / (float)den;
  m->o2m = (r > 0.f ? r : 0.f) * (0.8f - 0.1f) + 0.1f;
  const float o = 1.0f - m->o2m;
  m->o2o = o > 0.f ? o : 0.f;
  return YS_OK;
}

int ys_model_e2e_gains(ys_model* m, float* o2m, float* o2o) {
  YS_REQUIRE(m && o2m && o2o, "ys_model_e2e_gains: null argument");
  YS_REQUIRE(m->e2e, "ys_model_e2e_gains: not an End2End model (ys_model_e2e_init)");
  *o2m = m->o2m; *o2o = m->o2o;
  return YS_OK;
}

int ys_model_det_device(ys_model* m, float** rows, int* k) {
  YS_REQUIRE(m && rows && k, "ys_model_det_device: null argument");
  YS_REQUIRE(m->e2e, "ys_model_det_device: not an End2End model (ys_model_one2one_init / ys_model_e2e_init / _obb_init / _pose_init)");
  *rows = m->det_rows; *k = std::min(m->max_det, m->A);
  return YS_OK;
}

int ys_model_reserve_labels(ys_model* m, int per_image) {
  YS_REQUIRE(m && !m->is_block, "ys_model_reserve_labels: needs a full model");
  YS_REQUIRE(per_image > 0, "ys_model_reserve_labels: per_image = %d", per_image);
  if (per_image <= m->gcap) return YS_OK;
  YS_CHECK_HIP(hipSetDevice(m->ctx->device));
  m->have_loss = false; m->have_seg_loss = false;
  return alloc_label_ws(m, (per_image + 15) / 16 * 16);
}

// The one2one criterion pass of an End2End model, from the arguments of its one2many pass.  E2EDetectLoss (Loss.cs:1094-1118): v8DetectionLoss(tal_topk 1),
// unweighted.  E2ESegmentLoss (Loss.cs:1179-1236) / E2EOBBLoss (Loss.cs:1120-1177) / E2EPoseLoss (Loss.cs:1238-1295): the task's criterion with tal_topk 7, tal_topk2 1, weighted with o2o.
// The one2one head outputs ARE the one2many ones (aliased towers, same input values), so the pass reads the same pd / ps / pa.  It pads its own GT again
// (loss_prep_body: the thin-box widening of Tal.cs:283-287 lands in a fresh tensor, as in the reference where each criterion calls preprocess itself) and
// reuses the first pass's assignment workspaces: the stream is in order, and what outlives a pass are its gradients and its scalars -- those get buffers of
// their own.  A Detect model keeps o2o = 1, so its factors are the plain constants.
static LossArgs one2one_pass(const ys_model* m, LossArgs a) {
  const bool cv4 = m->e2e_cv4();
  a.topk = cv4 ? 7 : 1; a.topk2 = cv4 ? 1 : 0;
  a.dpd = m->o2o_dpd; a.dps = m->o2o_dps; a.dpa = m->o2o_dmc; a.scalars = m->scalars2;
  a.hyp_box = 7.5f * m->o2o; a.hyp_cls = 0.5f * m->o2o; a.hyp_dfl = 1.5f * m->o2o; a.hyp_angle = 1.0f * m->o2o;
  return a;
}

// aux_follows: the caller is the task's own criterion (mask / keypoint / angle terms); first: receives the arguments of the one2many pass
static int loss_detect_core(ys_model* m, const float* batch_idx, const float* cls, const float* bboxes, int n, int on_device, bool aux_follows,
                            LossArgs* first = nullptr) {
  YS_REQUIRE(m, "null model");
  // Training forward -> the criterion feeds backward (Amp.cs:338-348).  Eval forward -> validation loss on the eval-mode preds
  // (Detector.cs:94-97): the head logits are produced in both modes; only backward needs the training-mode state.
  YS_REQUIRE(!m->is_block && m->have_fwd, "ys_loss_detect: needs a forward of a full model first");
  YS_REQUIRE(!m->cls, "ys_loss_detect: a classify model's criterion is ys_loss_classify (Loss.cs:1073-1091)");
  YS_REQUIRE(m->xkind != 2 || aux_follows, "ys_loss_detect: an OBB model's criterion is ys_loss_obb (oriented labels, Loss.cs:486-684)");
  YS_REQUIRE(m->xkind != 3 || aux_follows, "ys_loss_detect: a Pose model's criterion is ys_loss_pose (keypoint terms, Loss.cs:870-1071)");
  YS_REQUIRE(!(m->e2e && m->segment) || aux_follows, "ys_loss_detect: an End2End Segment model's criterion is ys_loss_segment (E2ESegmentLoss: two detect passes and two mask terms, Loss.cs:1179-1236)");
  const bool rot = m->xkind == 2;
  const size_t lbytes = rot ? 20 : 16;
  YS_REQUIRE(n >= 0, "ys_loss_detect: n_labels = %d", n);
  YS_REQUIRE(n == 0 || (batch_idx && cls && bboxes), "ys_loss_detect: null label arrays");
  YS_CHECK_HIP(hipSetDevice(m->ctx->device));
  hipStream_t st = m->ctx->stream;
  const float *bi = batch_idx, *cl = cls, *bb = bboxes;
  int host_cmax = 0;                           // host labels: the largest per-image count (0 = unknown)
  if (!on_device && n > 0) {
    // host labels: size the padded GT workspace from the batch itself, like the reference's counts.max() (Loss.cs:376-380)
    std::vector<int> cnt(m->B, 0);
    int mx = 0;
    for (int i = 0; i < n; i++) { const int b = (int)batch_idx[i]; if (b >= 0 && b < m->B) mx = std::max(mx, ++cnt[b]); }
    // every label row is staged (rows whose batch_idx lies outside [0, B) are ignored by the kernels, like the reference's
    // `batch_idx == j` matches): the staging arrays hold gcap * max_batch rows, so n itself bounds the capacity too
    host_cmax = mx > 0 ? mx : 1;
    const int per_rows = (n + m->maxB - 1) / m->maxB;
    if (per_rows > mx) mx = per_rows;
    if (mx > m->gcap) YS_TRY(alloc_label_ws(m, (mx + 15) / 16 * 16));
    YS_REQUIRE(n <= m->max_labels, "ys_loss_detect: %d label rows exceed the staging capacity %d", n, m->max_labels);
    YS_CHECK_HIP(hipMemcpyAsync(m->lab_bidx, batch_idx, (size_t)n * 4, hipMemcpyHostToDevice, st));
    YS_CHECK_HIP(hipMemcpyAsync(m->lab_cls, cls, (size_t)n * 4, hipMemcpyHostToDevice, st));
    YS_CHECK_HIP(hipMemcpyAsync(m->lab_box, bboxes, (size_t)n * lbytes, hipMemcpyHostToDevice, st));
    bi = m->lab_bidx; cl = m->lab_cls; bb = m->lab_box;
  }
  YsTimer timer(m->ctx, "loss");
  LossArgs a{};
  a.pd = m->bufs[m->pd_buf].act; a.ps = m->bufs[m->ps_buf].act; a.dpd = m->bufs[m->pd_buf].grad; a.dps = m->bufs[m->ps_buf].grad;
  a.ld_pd = m->ld_pd; a.ld_ps = m->ld_ps; a.B = m->B; a.A = m->A; a.nc = m->d.nc; a.reg_max = m->d.reg_max;
  a.H = m->d.height; a.W = m->d.width; a.nl = m->nl;
  for (int i = 0; i < 4; i++) { a.lvl_off[i] = m->lvl_off[i]; a.lvl_w[i] = m->lvl_w[i]; a.lvl_h[i] = m->lvl_h[i]; a.lvl_stride[i] = m->lvl_stride[i]; }
  a.batch_idx = bi; a.cls = cl; a.bboxes = bb; a.n_labels = n; a.gcap = m->gcap;
  a.gmax = (host_cmax > 0 && host_cmax < m->gcap) ? host_cmax : m->gcap;
  a.gt_count = m->gt_count; a.gt_box = m->gt_box; a.gt_cls = m->gt_cls; a.pbox = m->pbox; a.ov = m->ov; a.align = m->align;
  a.mpos = m->mpos; a.pos_align = m->pos_align; a.pos_ov = m->pos_ov; a.fg_gt = m->fg_gt; a.tnorm = m->tnorm;
  a.partial = m->loss_partial; a.scalars = m->scalars;
  // Loss.cs:344,357.  E2ESegmentLoss / E2EOBBLoss (Loss.cs:1222): loss = o2m * L_one2many + o2o * L_one2one.  Items and gradients are linear in the hyp_*
  // factors, so the gain rides on them: no scale pass over any buffer.  Every other model has o2m = 1
  a.hyp_box = 7.5f * m->o2m; a.hyp_cls = 0.5f * m->o2m; a.hyp_dfl = 1.5f * m->o2m; a.topk = 10;
  if (rot) {                                                             // Loss.cs:489: hyp_angle = 1
    const Buf& ab = m->bufs[m->mc_buf];
    a.rot = 1; a.pa = ab.act; a.dpa = ab.grad; a.ld_pa = m->ld_mc; a.hyp_angle = 1.0f * m->o2m;
  }
  YS_TRY(ys_loss_detect_launch(st, m->dtype, a));
  if (first) *first = a;
  if (m->e2e && !m->segment && m->xkind != 3) YS_TRY(ys_loss_detect_launch(st, m->dtype, one2one_pass(m, a)));   // Segment / Pose: ys_loss_segment / ys_loss_pose run it, after their first mask / keypoint term
  YS_CHECK_HIP(hipGetLastError());
  m->have_loss = true;
  return YS_OK;
}

int ys_loss_detect(ys_model* m, const float* batch_idx, const float* cls, const float* bboxes, int n, int on_device) {
  return loss_detect_core(m, batch_idx, cls, bboxes, n, on_device, false);
}

// v8SegmentationLoss (Loss.cs:711-780): detection part + assignment (loss.hip), then the mask term (segloss.hip).
// masks: [B][mh][mw] fp32, overlap-encoded instance ids (0 = background, g+1 = the image's g-th label; YoloDataset.cs:265-267).
int ys_loss_segment(ys_model* m, const float* batch_idx, const float* cls, const float* bboxes, int n, const float* masks, int on_device,
                    int crop_mode) {
  YS_REQUIRE(m && m->segment, "ys_loss_segment: model has no Segment head");
  YS_REQUIRE(masks, "ys_loss_segment: null masks");
  LossArgs a{};
  YS_TRY(loss_detect_core(m, batch_idx, cls, bboxes, n, on_device, true, &a));
  m->have_loss = false;
  hipStream_t st = m->ctx->stream;
  const float* mk = masks;
  if (!on_device) {
    YS_CHECK_HIP(hipMemcpyAsync(m->masks_dev, masks, (size_t)m->B * m->mh * m->mw * 4, hipMemcpyHostToDevice, st));
    mk = m->masks_dev;
  }
  YsTimer timer(m->ctx, "loss_seg");
  const Buf& mc = m->bufs[m->mc_buf];
  const Buf& pr = m->bufs[m->pr_buf];
  YS_TRY(ys_loss_segment_launch(st, m->dtype, mc.act, mc.grad, m->ld_mc, pr.act, pr.grad, m->ld_pr, mk, m->fg_gt, m->gt_box, m->seg_cnt,
                                m->seg_off, m->seg_list, m->seg_ent, m->seg_part, m->scalars, m->B, m->A, m->nm, m->mh, m->mw, m->gcap,
                                m->d.height, m->d.width, crop_mode, m->o2m));
  if (m->e2e) {
    // E2ESegmentLoss (Loss.cs:1179-1236): the one2one criterion = v8SegmentationLoss(tal_topk 7, tal_topk2 1) on the same head outputs (aliased towers).
    // The mask term above has read the first assignment (fg_gt, gt_box, seg_*); the second detect pass may now overwrite those workspaces.  Its gradients
    // and scalars have buffers of their own; its mask term writes the one2one coefficient gradient and NO prototype gradient (proto.detach(), Head.cs:297).
    YS_TRY(ys_loss_detect_launch(st, m->dtype, one2one_pass(m, a)));
    YS_TRY(ys_loss_segment_launch(st, m->dtype, mc.act, m->o2o_dmc, m->ld_mc, pr.act, nullptr, m->ld_pr, mk, m->fg_gt, m->gt_box, m->seg_cnt,
                                  m->seg_off, m->seg_list, m->seg_ent, m->seg_part, m->scalars2, m->B, m->A, m->nm, m->mh, m->mw, m->gcap,
                                  m->d.height, m->d.width, crop_mode, m->o2o));
  }
  YS_CHECK_HIP(hipGetLastError());
  m->have_loss = true; m->have_seg_loss = true;
  return YS_OK;
}

// v8OBBLoss (Loss.cs:486-684): the loss.hip pipeline in its rotated mode (probiou assigner and box term, rbox2dist DFL targets,
// angle term).  bboxes: fp32 [n][5] = normalised cx, cy, w, h + angle in radians.
int ys_loss_obb(ys_model* m, const float* batch_idx, const float* cls, const float* bboxes, int n, int on_device) {
  YS_REQUIRE(m && m->xkind == 2, "ys_loss_obb: model has no Obb head");
  YS_TRY(loss_detect_core(m, batch_idx, cls, bboxes, n, on_device, true));
  m->have_seg_loss = true;
  return YS_OK;
}

// v8PoseLoss (Loss.cs:870-1071): detection part + assignment (loss.hip), then the keypoint terms (poseloss.hip).  On an End2End model (ys_model_e2e_pose_init)
// E2EPoseLoss: detect(tal_topk 10) -> keypoint terms -> detect(tal_topk 7, keep-best) -> keypoint terms, each pair weighted with its gain.
// keypoints: fp32 [n][kpt_num][kpt_dim] normalised to the image like bboxes (x, y[, visibility]); row i belongs to label i.
int ys_loss_pose(ys_model* m, const float* batch_idx, const float* cls, const float* bboxes, int n, const float* keypoints, int on_device) {
  YS_REQUIRE(m && m->xkind == 3, "ys_loss_pose: model has no Pose head");
  YS_REQUIRE(n == 0 || keypoints, "ys_loss_pose: null keypoints");
  if (!on_device && batch_idx)                 // keypoint rows are addressed by a label's rank within its image: collate order only
    for (int i = 1; i < n; i++)
      YS_REQUIRE(batch_idx[i] >= batch_idx[i - 1], "ys_loss_pose: labels must be grouped by image in collate order (batch_idx[%d] = %g < batch_idx[%d] = %g)",
                 i, (double)batch_idx[i], i - 1, (double)batch_idx[i - 1]);
  LossArgs first{};
  YS_TRY(loss_detect_core(m, batch_idx, cls, bboxes, n, on_device, true, &first));
  m->have_loss = false;
  hipStream_t st = m->ctx->stream;
  const float* kp = keypoints;
  if (!on_device && n > 0) {
    YS_REQUIRE(n <= m->max_labels, "ys_loss_pose: %d labels exceed the staging capacity %d", n, m->max_labels);
    YS_CHECK_HIP(hipMemcpyAsync(m->kp_dev, keypoints, (size_t)n * m->nm * 4, hipMemcpyHostToDevice, st));
    kp = m->kp_dev;
  }
  YsTimer timer(m->ctx, "loss_pose");
  const Buf& kb = m->bufs[m->mc_buf];
  PoseArgs a{};
  a.kp = kb.act; a.dkp = kb.grad; a.ld = m->ld_mc; a.fg_gt = m->fg_gt; a.gt_box = m->gt_box;
  a.gt_src = m->gt_cls + 2L * m->B * m->gcap;
  a.keypoints = kp; a.part = m->seg_part; a.scalars = m->scalars;
  a.B = m->B; a.A = m->A; a.K = m->nm / m->kdim; a.D = m->kdim; a.gcap = m->gcap; a.H = m->d.height; a.W = m->d.width; a.nl = m->nl;
  for (int i = 0; i < 4; i++) { a.lvl_off[i] = m->lvl_off[i]; a.lvl_w[i] = m->lvl_w[i]; a.lvl_stride[i] = m->lvl_stride[i]; }
  a.hyp_pose = 12.0f * m->o2m; a.hyp_kobj = 1.0f * m->o2m;                                // Loss.cs:896; E2EPoseLoss: the gain rides on them (a plain model has o2m = 1)
  static const float oks[17] = {0.026f, 0.025f, 0.025f, 0.035f, 0.035f, 0.079f, 0.079f, 0.072f, 0.072f, 0.062f, 0.062f, 0.107f, 0.107f,
                                0.087f, 0.087f, 0.089f, 0.089f};                          // OKS_SIGMA (Loss.cs:9-16)
  const bool coco = a.K == 17 && a.D == 3;                                                // Loss.cs:903-905
  for (int k = 0; k < a.K && k < YS_POSE_KMAX; k++) a.sigma[k] = coco ? oks[k] : 1.0f / (float)a.K;
  YS_TRY(ys_loss_pose_launch(st, m->dtype, a, m->seg_cnt, m->seg_off, m->seg_list));
  if (m->e2e) {
    // E2EPoseLoss (Loss.cs:1238-1295): the one2one criterion = v8PoseLoss(tal_topk 7, tal_topk2 1) on the same head outputs (aliased towers).  The keypoint
    // term above has read the first assignment (fg_gt, gt_box, gt_src, seg_cnt / off / list); the second detect pass may now overwrite those workspaces.
    // Its gradients and scalars have buffers of their own: the launch clears the whole one2one keypoint gradient (padding included) like the one2many one,
    // and reuses seg_part, which the first launch's finalize has read by then (one stream).
    YS_TRY(ys_loss_detect_launch(st, m->dtype, one2one_pass(m, first)));
    a.dkp = m->o2o_dmc; a.scalars = m->scalars2; a.hyp_pose = 12.0f * m->o2o; a.hyp_kobj = 1.0f * m->o2o;
    YS_TRY(ys_loss_pose_launch(st, m->dtype, a, m->seg_cnt, m->seg_off, m->seg_list));
  }
  YS_CHECK_HIP(hipGetLastError());
  m->have_loss = true; m->have_seg_loss = true;
  return YS_OK;
}

// v8ClassificationLoss (Loss.cs:1073-1091): cross_entropy(preds["cls"], batch["cls"].view(-1)), mean reduction, and d(loss)/d(logits)
// = (softmax - onehot) / B into the logits' gradient buffer.  cls: fp32 class ids [batch].  Works after a training forward (the step) and
// after an eval forward (Classifier.Val's loss on the eval logits, Classifier.cs:90-93).
int ys_loss_classify(ys_model* m, const float* cls, int batch, int on_device) {
  YS_REQUIRE(m && cls, "ys_loss_classify: null argument");
  YS_REQUIRE(m->cls, "ys_loss_classify: the model has no Classify head (task %d)", m->d.task);
  YS_REQUIRE(m->have_fwd, "ys_loss_classify: needs a forward first");
  YS_REQUIRE(batch == m->B, "ys_loss_classify: batch %d differs from the last forward's %d", batch, m->B);
  if (!on_device)
    for (int i = 0; i < batch; i++)
      YS_REQUIRE(cls[i] >= 0.f && cls[i] < (float)m->d.nc && cls[i] == floorf(cls[i]), "ys_loss_classify: label %g of image %d is not a class id in [0, %d)",
                 (double)cls[i], i, m->d.nc);
  YS_CHECK_HIP(hipSetDevice(m->ctx->device));
  hipStream_t st = m->ctx->stream;
  const float* lab = cls;
  if (!on_device) { YS_CHECK_HIP(hipMemcpyAsync(m->cls_lab, cls, (size_t)batch * 4, hipMemcpyHostToDevice, st)); lab = m->cls_lab; }
  YsTimer timer(m->ctx, "loss");
  const Buf& lb = m->bufs[m->logit_buf];
  YS_TRY(ys_cls_xent_launch(st, m->dtype, lb.act, m->ld_cls, batch, m->d.nc, lab, lb.grad, nullptr, m->cls_rows, m->scalars));
  YS_CHECK_HIP(hipGetLastError());
  m->have_loss = true; m->have_seg_loss = true;
  return YS_OK;
}

// The criterion's scalars on the host: h[1..3] box / cls / dfl, h[4] the loss sum, h[8] seg, h[10..11] pose / kobj, h[13] angle, h[14] invalid class ids
// (Classify), h[15] the batch's largest per-image label count.  Device-resident labels cannot size the workspace without a host sync: the prep kernel records
// that count and this first synchronising read refuses a truncated assignment instead of returning it.  End2End: the items / loss of the one2one criterion
// pass are added to the one2many ones (Loss.cs:1113-1117; both already carry their gain).
static int read_scalars(ys_model* m, float h[16]) {
  float g[16];
  YS_CHECK_HIP(hipMemcpyAsync(h, m->scalars, sizeof(g), hipMemcpyDeviceToHost, m->ctx->stream));
  if (m->e2e) YS_CHECK_HIP(hipMemcpyAsync(g, m->scalars2, sizeof(g), hipMemcpyDeviceToHost, m->ctx->stream));
  YS_CHECK_HIP(hipStreamSynchronize(m->ctx->stream));
  if (m->e2e) {
    for (int i = 1; i <= 4; i++) h[i] += g[i];
    if (m->segment) h[8] += g[8];            // the mask term
    if (m->xkind == 2) h[13] += g[13];       // the angle term
    if (m->xkind == 3) { h[10] += g[10]; h[11] += g[11]; }   // the keypoint terms
  }
  if (m->cls || (int)h[15] <= m->gcap) return YS_OK;
  m->have_loss = false; m->have_seg_loss = false;
  ys_set_error("loss: an image of this batch has %d labels but the workspace holds %d per image (the reference pads to the batch maximum, "
               "Loss.cs:363-390): call ys_model_reserve_labels(model, %d) or pass max_labels at creation, then repeat the step",
               (int)h[15], m->gcap, (int)h[15]);
  return YS_ERR_INVALID_ARG;
}

// loss items in the reference's order: detect [box, cls, dfl] (Loss.cs:414); segment [box, seg, cls, dfl, semseg] (Loss.cs:719)
int ys_loss_read_items(ys_model* m, float* items, int n_items, float* loss_sum) {
  YS_REQUIRE(m && m->have_loss, "ys_loss_read_items: no loss has run");
  YS_REQUIRE(items && n_items == m->n_items, "ys_loss_read_items: this model's criterion has %d items", m->n_items);
  float h[16];
  YS_TRY(read_scalars(m, h));
  if (m->cls) {                // v8ClassificationLoss: one item, the batch mean, which is also the scalar backward() runs on (Loss.cs:1086-1088)
    if (h[14] != 0.f) {
      m->have_loss = false;
      ys_set_error("ys_loss_classify: %d label(s) of this batch are not class ids in [0, %d)", (int)h[14], m->d.nc);
      return YS_ERR_INVALID_ARG;
    }
    items[0] = h[1];
    if (loss_sum) *loss_sum = h[4];
    return YS_OK;
  }
  if (m->segment) {
    YS_REQUIRE(m->have_seg_loss, "ys_loss_read_items: the Segment model needs ys_loss_segment");
    items[0] = h[1]; items[1] = h[8]; items[2] = h[2]; items[3] = h[3]; items[4] = 0.f;
  } else if (m->xkind == 2) {
    items[0] = h[1]; items[1] = h[2]; items[2] = h[3]; items[3] = h[13];                     // box, cls, dfl, angle (Loss.cs:619)
  } else if (m->xkind == 3) {
    YS_REQUIRE(m->have_seg_loss, "ys_loss_read_items: the Pose model needs ys_loss_pose");
    items[0] = h[1]; items[1] = h[10]; items[2] = h[11]; items[3] = h[2]; items[4] = h[3];   // box, pose, kobj, cls, dfl (Loss.cs:965)
  } else {
    items[0] = h[1]; items[1] = h[2]; items[2] = h[3];
  }
  if (loss_sum) *loss_sum = h[4];
  return YS_OK;
}

int ys_loss_read(ys_model* m, float loss_items[3], float* loss_sum) {
  YS_REQUIRE(m && m->have_loss, "ys_loss_read: no loss has run");
  YS_REQUIRE(!m->cls, "ys_loss_read: a classify model has one loss item (ys_loss_read_items with n_items = 1)");
  float h[16];
  YS_TRY(read_scalars(m, h));
  if (loss_items) { loss_items[0] = h[1]; loss_items[1] = h[2]; loss_items[2] = h[3]; }
  if (loss_sum) *loss_sum = h[4];
  return YS_OK;
}

// The assignment behind the last criterion call (tests compare it with a reference assigner anchor by anchor): target_gt_idx [B*A] = the label slot within
// the anchor's image (order of appearance), -1 = background; target_score [B*A] = the anchor's normalised target score (target_scores.sum(-1), Loss.cs:138);
// *tss = target_scores_sum = max(sum, 1) (Loss.cs:444).  The workspaces are shared by the passes of an End2End criterion, so there this is the one2one pass.
// Synchronising and read-only; any of the three outputs may be null.
int ys_loss_read_targets(ys_model* m, int32_t* target_gt_idx, float* target_score, float* tss) {
  YS_REQUIRE(m && !m->is_block, "ys_loss_read_targets: needs a full model");
  YS_REQUIRE(!m->cls, "ys_loss_read_targets: a classify model's criterion assigns no targets");
  YS_REQUIRE(m->have_loss, "ys_loss_read_targets: no loss has run");
  hipStream_t st = m->ctx->stream;
  const size_t n = (size_t)m->B * m->A;
  if (target_gt_idx) YS_CHECK_HIP(hipMemcpyAsync(target_gt_idx, m->fg_gt, n * 4, hipMemcpyDeviceToHost, st));
  if (target_score) YS_CHECK_HIP(hipMemcpyAsync(target_score, m->tnorm, n * 4, hipMemcpyDeviceToHost, st));
  if (tss) YS_CHECK_HIP(hipMemcpyAsync(tss, m->e2e ? m->scalars2 : m->scalars, 4, hipMemcpyDeviceToHost, st));
  YS_CHECK_HIP(hipStreamSynchronize(st));
  return YS_OK;
}

}  // extern "C"
