// model_api.hip -- the ys_model_* / ys_optim_* / ys_block_* / ys_head_* entry points (include/yolosharp_hip.h): argument checks, handle creation and
// destruction, tensor access, and the calls into the graph builder (graph.hip), the planner (plan.hip) and the step (model.hip).  The criterion, End2End
// setup and output accessors are criterion.hip's.
#include "ys_model.h"
#include <cmath>
#include <cstring>
#include <algorithm>

using namespace ysm;

namespace {

TensorRec* find_tensor(ys_model* m, const char* name) {
  for (auto& t : m->tensors) if (t.name == name) return &t;
  return nullptr;
}

// splitmix64 -> uniform(-bound, bound)
struct Rng {
  uint64_t s;
  uint64_t next() { uint64_t z = (s += 0x9E3779B97F4A7C15ull); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
  float uni(float b) { return ((float)((next() >> 40) & 0xFFFFFF) / 16777216.0f * 2.0f - 1.0f) * b; }
};

// what the three create entries share: a fresh handle with the storage type of `dtype`.  YS_FP8 = the bf16 engine (storage, BN, losses, weight gradients,
// optimizer) with fp8 MFMA forward / dgrad convolutions
ys_model* new_handle(ys_ctx* ctx, int dtype, int max_batch) {
  ys_model* m = new ys_model();
  m->f8 = dtype == YS_FP8;
  const int store = m->f8 ? YS_BF16 : dtype;
  m->ctx = ctx; m->dtype = store; m->epl = store == YS_BF16 ? 8 : 4; m->es = store == YS_BF16 ? 2 : 4;
  m->maxB = max_batch;
  return m;
}
// ... and how they end once the graph is built (st = the builder's status): parameter layout, module-relative tensor names for a standalone handle (its
// modules were built under the prefix `strip`), allocation, default weights.  Destroys the handle on failure
int finish_handle(ys_model* m, int st, const char* strip, ys_model** out) {
  if (st == YS_OK) st = layout_params(m);
  if (st == YS_OK && strip) { const size_t n = strlen(strip); for (auto& t : m->tensors) if (t.name.compare(0, n, strip) == 0) t.name.erase(0, n); }
  if (st == YS_OK) st = allocate(m);
  if (st == YS_OK) st = ys_model_init_weights(m, 0);
  if (st != YS_OK) { ys_model_destroy(m); return st; }
  *out = m;
  return YS_OK;
}

}  // namespace

extern "C" {

int ys_model_create(ys_ctx* ctx, const ys_model_desc* desc, ys_model** out) {
  YS_REQUIRE(ctx && desc && out, "ys_model_create: null argument");
  YS_REQUIRE(desc->dtype == YS_F32 || desc->dtype == YS_BF16 || desc->dtype == YS_FP8, "ys_model_create: dtype %d unsupported", desc->dtype);
  if ((desc->family != YS_YOLOV8 && desc->family != YS_YOLOV11 && desc->family != YS_YOLOV5U) || desc->task < YS_DETECT || desc->task > YS_CLASSIFY) {
    ys_set_error("ys_model_create: YOLOv8 / YOLOv11 detect, segment, obb, pose and classify and YOLOv5u detect are built (family %d task %d)", desc->family, desc->task);
    return YS_ERR_UNSUPPORTED;
  }
  if (desc->family == YS_YOLOV5U && desc->task != YS_DETECT) {
    ys_set_error("ys_model_create: YOLOv5u is built for the detect task (with End2End); its segment, obb, pose and classify graphs are not (task %d)", desc->task);
    return YS_ERR_UNSUPPORTED;
  }
  if (desc->family == YS_YOLOV5U && desc->dtype == YS_FP8) {
    ys_set_error("ys_model_create: YOLOv5u runs in YS_F32 or YS_BF16; YS_FP8 is not built for this family");
    return YS_ERR_UNSUPPORTED;
  }
  if (desc->task == YS_CLASSIFY && desc->dtype == YS_FP8) {
    ys_set_error("ys_model_create: the classify graphs run in YS_F32 or YS_BF16; YS_FP8 is not built for them");
    return YS_ERR_UNSUPPORTED;
  }
  YS_REQUIRE(desc->size >= 0 && desc->size <= 4, "ys_model_create: size %d out of range", desc->size);
  YS_REQUIRE(desc->nc > 0 && (desc->task == YS_CLASSIFY || (desc->reg_max > 1 && desc->reg_max <= 32)), "ys_model_create: nc=%d reg_max=%d", desc->nc, desc->reg_max);
  YS_REQUIRE(desc->height > 0 && desc->width > 0 && desc->height % 32 == 0 && desc->width % 32 == 0,
             "ys_model_create: image size %dx%d must be a positive multiple of 32", desc->height, desc->width);
  YS_REQUIRE(desc->max_batch > 0, "ys_model_create: max_batch %d", desc->max_batch);
  YS_CHECK_HIP(hipSetDevice(ctx->device));
  ys_model* m = new_handle(ctx, desc->dtype, desc->max_batch);
  m->d = *desc;
  for (int j = 0; j < 64; j++) m->dfl_w[j] = (float)j;
  const int st = desc->task == YS_CLASSIFY ? (desc->family == YS_YOLOV11 ? build_v11_classify(m) : build_v8_classify(m))
                                           : (desc->family == YS_YOLOV11 ? build_v11_detect(m) : desc->family == YS_YOLOV5U ? build_v5u_detect(m) : build_v8_detect(m));
  return finish_handle(m, st, nullptr, out);
}

int ys_model_destroy(ys_model* m) {
  if (!m) return YS_OK;
  hipSetDevice(m->ctx->device);
  hipStreamSynchronize(m->ctx->stream);
  if (m->st2) {
    hipStreamSynchronize(m->st2);
    for (hipEvent_t ev : m->ev_hand) if (ev) hipEventDestroy(ev);
    if (m->ev_join) hipEventDestroy(m->ev_join);
    hipStreamDestroy(m->st2);
  }
  for (int k = 0; k < ys_model::NSEG; k++) { if (m->ev_seg_m[k]) hipEventDestroy(m->ev_seg_m[k]); if (m->ev_seg_w[k]) hipEventDestroy(m->ev_seg_w[k]); }
  for (void* p : m->allocs) hipFree(p);
  delete m;
  return YS_OK;
}

}  // extern "C"
ys_ctx* ys_model_ctx(ys_model* m) { return m->ctx; }   // for dist.hip
extern "C" {
int ys_model_num_tensors(ys_model* m) { return m ? (int)m->tensors.size() : 0; }
int ys_model_num_anchors(ys_model* m) { return m ? m->A : 0; }
int64_t ys_model_num_params(ys_model* m) { return m ? (int64_t)m->n_params_real : 0; }

int ys_model_tensor_info(ys_model* m, int index, char* name, int name_cap, int32_t* ndim, int64_t shape[4], int32_t* is_param) {
  YS_REQUIRE(m && index >= 0 && index < (int)m->tensors.size(), "ys_model_tensor_info: index %d out of range", index);
  const TensorRec& t = m->tensors[index];
  if (name && name_cap > 0) { strncpy(name, t.name.c_str(), name_cap - 1); name[name_cap - 1] = 0; }
  if (ndim) *ndim = t.ndim;
  if (shape) for (int i = 0; i < 4; i++) shape[i] = i < t.ndim ? t.shape[i] : 1;
  if (is_param) *is_param = t.is_param ? 1 : 0;
  return YS_OK;
}

static int tensor_io(ys_model* m, const char* name, float* host, size_t count, int what /*0 set,1 get,2 get grad*/) {
  YS_REQUIRE(m && name && host, "tensor io: null argument");
  if (what == 2) YS_TRY(join_wgrad_stream(m));   // asynchronous segment ends: gradients are complete once the weight-gradient stream has drained
  TensorRec* t = find_tensor(m, name);
  YS_REQUIRE(t != nullptr, "unknown tensor '%s'", name);
  YS_REQUIRE((long)count == t->count, "tensor '%s' has %ld elements, caller passed %zu", name, t->count, count);
  hipStream_t st = m->ctx->stream;
  if (t->kind == 3) {
    YS_REQUIRE(what != 2, "'%s' has no gradient (DFL is only used in eval, Head.cs:221)", name);
    if (what == 0) memcpy(m->dfl_w, host, count * 4); else memcpy(host, m->dfl_w, count * 4);
    return YS_OK;
  }
  float* dev = t->kind == 2 ? m->state + t->off : (what == 2 ? m->grads + t->off : m->params + t->off);
  YS_REQUIRE(!(what == 2 && t->kind == 2), "'%s' is a buffer and has no gradient", name);
  if (t->kind == 0 || t->kind == 4 || t->kind == 5) {
    // edge layout [outer][d0][d1][d2] <-> [outer][d2][d1][d0] inside: conv weight OIHW <-> [Cout][taps][Cin] (outer = the module's own rows: a member of a fused
    // convolution owns a row range), depthwise [C][3][3] <-> [9][C], ConvTranspose2d [Cin][Cout][2][2] <-> [phase][Cout][Cin]
    const ConvL& c = m->convs[t->conv];
    const size_t outer = t->kind == 0 ? (size_t)t->shape[0] : 1, d0 = t->kind == 4 ? c.cout : c.cin, d1 = t->kind == 5 ? c.cout : 1;
    const size_t d2 = t->kind == 0 ? c.k * c.k : t->kind == 4 ? 9 : 4;
    std::vector<float> tmp(count);
    auto permute = [&](const float* edge_in, float* edge_out) {      // one of the two is null: the other direction
      size_t e = 0;
      for (size_t o = 0; o < outer; o++) for (size_t i0 = 0; i0 < d0; i0++) for (size_t i1 = 0; i1 < d1; i1++) for (size_t i2 = 0; i2 < d2; i2++, e++) {
        const size_t in = ((o * d2 + i2) * d1 + i1) * d0 + i0;
        if (edge_in) tmp[in] = edge_in[e]; else edge_out[e] = tmp[in];
      }
    };
    if (what == 0) permute(host, nullptr);
    if (what == 0) YS_CHECK_HIP(hipMemcpyAsync(dev, tmp.data(), count * 4, hipMemcpyHostToDevice, st));
    else YS_CHECK_HIP(hipMemcpyAsync(tmp.data(), dev, count * 4, hipMemcpyDeviceToHost, st));
    YS_CHECK_HIP(hipStreamSynchronize(st));
    if (what != 0) permute(nullptr, host);
    else if (t->kind != 4) m->weights_dirty = true;                  // (depthwise kernels read the fp32 master weights directly: no shadow to prepare)
  } else {
    if (what == 0) YS_CHECK_HIP(hipMemcpyAsync(dev, host, count * 4, hipMemcpyHostToDevice, st));
    else YS_CHECK_HIP(hipMemcpyAsync(host, dev, count * 4, hipMemcpyDeviceToHost, st));
    YS_CHECK_HIP(hipStreamSynchronize(st));
    if (what == 0) m->eval_coeffs_dirty = true;
  }
  return YS_OK;
}
int ys_model_set_tensor(ys_model* m, const char* name, const float* host, size_t count) { return tensor_io(m, name, (float*)host, count, 0); }
int ys_model_get_tensor(ys_model* m, const char* name, float* host, size_t count) { return tensor_io(m, name, host, count, 1); }
int ys_model_get_grad(ys_model* m, const char* name, float* host, size_t count) { return tensor_io(m, name, host, count, 2); }

int ys_model_init_weights(ys_model* m, uint64_t seed) {
  YS_REQUIRE(m, "null model");
  std::vector<float> p(m->n_params, 0.f), s(m->n_state, 0.f);
  Rng rng{seed * 0x9E3779B97F4A7C15ull + 0x1234567ull};
  for (const auto& c : m->convs) {
    const long nw = c.dw ? (long)c.cout * 9 : c.ct ? 4L * c.cout * c.cin : (long)c.cout * c.k * c.k * c.cin;
    const float bound = c.ct ? 1.0f / sqrtf((float)(c.cout * 4)) : 1.0f / sqrtf((float)((c.dw ? 1 : c.cin) * c.k * c.k));   // kaiming_uniform(a=sqrt 5): 1/sqrt(fan_in)
    const long nwr = c.cout_real == c.cout ? nw : (long)c.cout_real * c.k * c.k * c.cin;   // padded rows stay zero
    for (long i = 0; i < nwr; i++) p[c.w_off + i] = rng.uni(bound);
    if (c.bn) {
      for (int i = 0; i < c.cout; i++) { p[c.g_off + i] = 1.f; p[c.b_off + i] = 0.f; s[c.rm_off + i] = 0.f; s[c.rv_off + i] = 1.f; }
      s[c.nbt_off] = 0.f;
    } else {
      for (int i = 0; i < c.cout_real; i++) p[c.g_off + i] = rng.uni(bound);   // Conv2d bias: U(-1/sqrt(fan_in), +)
    }
  }
  hipStream_t st = m->ctx->stream;
  YS_CHECK_HIP(hipMemcpyAsync(m->params, p.data(), p.size() * 4, hipMemcpyHostToDevice, st));
  YS_CHECK_HIP(hipMemcpyAsync(m->state, s.data(), s.size() * 4, hipMemcpyHostToDevice, st));
  YS_CHECK_HIP(hipMemsetAsync(m->grads, 0, (size_t)m->n_params * 4, st));
  YS_CHECK_HIP(hipMemsetAsync(m->adam_m, 0, (size_t)m->n_params * 4, st));
  YS_CHECK_HIP(hipMemsetAsync(m->adam_v, 0, (size_t)m->n_params * 4, st));
  YS_CHECK_HIP(hipStreamSynchronize(st));
  m->step = 0; m->weights_dirty = true; m->eval_coeffs_dirty = true;
  return YS_OK;
}

int ys_model_set_training(ys_model* m, int training) {
  YS_REQUIRE(m, "null model");
  m->training = training != 0;
  if (!m->training) m->eval_coeffs_dirty = true;
  return YS_OK;
}

int ys_model_forward(ys_model* m, const float* images, int on_device, int batch) {
  YS_REQUIRE(m && images, "ys_model_forward: null argument");
  YS_REQUIRE(!m->is_block && !m->is_head, "ys_model_forward: this handle is a block / head (use ys_block_forward or ys_head_forward)");
  YS_REQUIRE(batch > 0 && batch <= m->maxB, "ys_model_forward: batch %d outside (0, %d]", batch, m->maxB);
  YS_CHECK_HIP(hipSetDevice(m->ctx->device));
  hipStream_t st = m->ctx->stream;
  const float* src = images;
  YS_TRY(join_wgrad_stream(m));   // the previous backward's weight-gradient kernels (model.0 reads the input buffer / the staged image) may still run on the second stream
  if (!on_device) {
    YS_CHECK_HIP(hipMemcpyAsync(m->img_dev, images, (size_t)batch * 3 * m->d.height * m->d.width * 4, hipMemcpyHostToDevice, st));
    src = m->img_dev;
  }
  YsTimer timer(m->ctx, "forward");
  m->B = batch;
  // model.0 reads the fp32 planes itself when it can (conv_stem.hip): no packed bf16 NHWC copy of the image.  The weight gradient of
  // this step reads the same planes again, so a device-resident image must stay unchanged until the step's backward has run (the
  // autograd rule of the reference: Utils/Amp.cs:348 differentiates through the tensor it was handed).
  m->in_f32 = nullptr;
  if (stem_direct(m)) m->in_f32 = src;
  else YS_TRY(ys_pack_input_launch(st, m->dtype, src, batch, 3, m->d.height, m->d.width, m->epl, m->bufs[m->in_buf].act));
  YS_TRY(forward_impl(m, batch));
  m->have_fwd = true; m->fwd_training = m->training; m->have_loss = false; m->have_seg_loss = false;
  return YS_OK;
}

// Predict-side input path (Models/Detector.cs:31-41): uint8 RGB planes [B,3,h,w] -> zero-pad mode with value 114 on the bottom /
// right up to the model's (H, W) -> / 255 -> the NHWC input buffer, in one kernel (no fp32 image is materialised).
int ys_model_forward_u8(ys_model* m, const uint8_t* images, int on_device, int batch, int h, int w) {
  YS_REQUIRE(m && images, "ys_model_forward_u8: null argument");
  YS_REQUIRE(!m->is_block && !m->is_head, "ys_model_forward_u8: this handle is a block / head (use ys_block_forward or ys_head_forward)");
  YS_REQUIRE(batch > 0 && batch <= m->maxB, "ys_model_forward_u8: batch %d outside (0, %d]", batch, m->maxB);
  YS_REQUIRE(h > 0 && w > 0 && h <= m->d.height && w <= m->d.width, "ys_model_forward_u8: image %dx%d does not fit the model's %dx%d", h, w, m->d.height, m->d.width);
  YS_CHECK_HIP(hipSetDevice(m->ctx->device));
  hipStream_t st = m->ctx->stream;
  const unsigned char* src = images;
  if (!on_device) {
    YS_TRY(join_wgrad_stream(m)); // the staging buffer may be the fp32 image the previous step's model.0 weight gradient still reads
    YS_CHECK_HIP(hipMemcpyAsync(m->img_dev, images, (size_t)batch * 3 * h * w, hipMemcpyHostToDevice, st));
    src = (const unsigned char*)m->img_dev;
  }
  YsTimer timer(m->ctx, "forward");
  m->B = batch;
  YS_TRY(join_wgrad_stream(m));   // as in ys_model_forward: the input buffer is rewritten below
  m->in_f32 = nullptr;            // uint8 planes: the packed input buffer is the layer's input
  YS_TRY(ys_pack_input_u8_launch(st, m->dtype, src, batch, 3, h, w, m->d.height, m->d.width, m->epl, m->bufs[m->in_buf].act));
  YS_TRY(forward_impl(m, batch));
  m->have_fwd = true; m->fwd_training = m->training; m->have_loss = false; m->have_seg_loss = false;
  return YS_OK;
}

int ys_model_backward_segments(ys_model* m) { (void)m; return ys_model::NSEG; }

static int backward_segment(ys_model* m, int seg, bool async_end, const char* who) {
  YS_REQUIRE(m && m->have_loss, "ys_model_backward: needs forward + loss first");
  YS_REQUIRE(m->fwd_training, "ys_model_backward: the last forward ran in eval mode (no batch statistics / pre-BN outputs were kept)");
  YS_REQUIRE(seg >= 0 && seg < ys_model::NSEG, "%s: segment %d out of range", who, seg);
  YS_CHECK_HIP(hipSetDevice(m->ctx->device));
  if (seg == 0) { YS_TRY(join_wgrad_stream(m)); reset_grad_state(m); }   // (the join: see ys_model_backward)
  return backward_range(m, seg, seg, async_end);
}
int ys_model_backward_segment(ys_model* m, int seg) { return backward_segment(m, seg, false, "ys_model_backward_segment"); }
int ys_model_backward_segment_async(ys_model* m, int seg) { return backward_segment(m, seg, true, "ys_model_backward_segment_async"); }

int ys_model_segment_fence(ys_model* m, int seg, void* stream) {
  YS_REQUIRE(m && seg >= 0 && seg < ys_model::NSEG, "ys_model_segment_fence: bad argument");
  YS_REQUIRE(m->ev_seg_m[seg], "ys_model_segment_fence: model not built");
  YS_CHECK_HIP(hipSetDevice(m->ctx->device));
  hipStream_t s = (hipStream_t)stream;
  YS_CHECK_HIP(hipStreamWaitEvent(s, m->ev_seg_m[seg], 0));
  if (m->seg_on_st2[seg]) YS_CHECK_HIP(hipStreamWaitEvent(s, m->ev_seg_w[seg], 0));
  return YS_OK;
}

int ys_model_backward(ys_model* m) {
  YS_REQUIRE(m && m->have_loss, "ys_model_backward: needs forward + loss first");
  YS_REQUIRE(m->fwd_training, "ys_model_backward: the last forward ran in eval mode (no batch statistics / pre-BN outputs were kept)");
  YS_REQUIRE(!m->segment || m->have_seg_loss, "ys_model_backward: the Segment model needs ys_loss_segment (mask gradients)");
  YS_CHECK_HIP(hipSetDevice(m->ctx->device));
  YsTimer timer(m->ctx, "backward");
  // model.0's weight-gradient kernel reads that unit's raw output and the gradient map of its output (its BatchNorm backward runs inside it, run_conv_bwd: stem_fused).
  // Where the launch went to the SECOND STREAM (the per-segment calls), it does so after the backward call has returned: every later writer of the two is ordered
  // behind it by joining the stream -- the next forward does (forward_impl / ys_model_forward), and so does a backward that follows without one, whose dgrad of
  // model.1 rewrites the gradient map.
  YS_TRY(join_wgrad_stream(m));
  reset_grad_state(m);
  // Round 6: the one-call backward ends every segment asynchronously as well -- a segment's split reduction (wgrad_reduce_batched_kernel: 1.08 GB of partial slabs per
  // YOLOv8n step, 0.21 ms when it runs alone at the end) goes to the weight-gradient stream behind that segment's weight gradients and runs beside the next segment's
  // BN-backward / dgrad chain; only the last (stem) segment's share is left for the end.  Nothing on the main stream waits: AdamW, zero_grad, gradient reads and the
  // next forward order themselves behind the second stream (join_wgrad_stream), as they do after ys_model_backward_segment_async.  Same kernels, same operands, same
  // order per stream: bit-identical gradients (tests/test_dist.py::test_async_segment_ends_give_the_same_gradients compares the two forms).
  if (m->overlap) {
    m->hold_stem = true;
    int rc = YS_OK;
    for (int sg = 0; sg < ys_model::NSEG && rc == YS_OK; sg++) rc = backward_range(m, sg, sg, true, false);
    m->hold_stem = false;
    return rc;
  }
  return backward_range(m, 0, ys_model::NSEG - 1);
}

int ys_model_segment_grad_range(ys_model* m, int seg, int64_t* offset, int64_t* count) {
  YS_REQUIRE(m && offset && count && seg >= 0 && seg < ys_model::NSEG, "ys_model_segment_grad_range: bad argument");
  *offset = m->seg_group[seg][0].off;
  *count = m->seg_group[seg][0].count + m->seg_group[seg][1].count + m->seg_group[seg][2].count;
  return YS_OK;
}

int ys_model_set_overlap(ys_model* m, int on) {
  YS_REQUIRE(m, "null model");
  if (m->st2_dirty) {                     // drain the weight-gradient stream before the mode changes
    YS_CHECK_HIP(hipEventRecord(m->ev_join, m->st2));
    YS_CHECK_HIP(hipStreamWaitEvent(m->ctx->stream, m->ev_join, 0));
    m->st2_dirty = false;
  }
  m->overlap = on != 0 && m->overlap_built;
  return YS_OK;
}

int ys_model_zero_grad(ys_model* m) {
  YS_REQUIRE(m, "null model");
  YS_TRY(join_wgrad_stream(m));              // asynchronous segment ends: the weight-gradient stream may still be adding into the buffer
  YS_CHECK_HIP(hipMemsetAsync(m->grads, 0, (size_t)m->n_params * 4, m->ctx->stream));
  return YS_OK;
}

int ys_model_grad_buffer(ys_model* m, float** dptr, int64_t* count) {
  YS_REQUIRE(m && dptr && count, "null argument");
  *dptr = m->grads; *count = m->n_params;
  return YS_OK;
}
int ys_model_param_buffer(ys_model* m, float** dptr, int64_t* count) {
  YS_REQUIRE(m && dptr && count, "null argument");
  *dptr = m->params; *count = m->n_params;
  return YS_OK;
}

// Parameter-group construction of the optimizer.  mode 0 (default): three DISJOINT groups (bias | conv weight | bn weight).
// mode 1: the reference's groups exactly as written (YoloBaseTaskModel.cs:144-151) -- name.Contains("bias") | Contains("weight") |
// Contains("bn") -- in which every BatchNorm weight and bias is listed twice; TorchSharp keys the optimizer state by parameter, so
// such a parameter receives two AdamW updates per step() from one shared state.  Must be chosen before the
// first optimizer step.
int ys_optim_set_param_groups(ys_model* m, int mode) {
  YS_REQUIRE(m && (mode == 0 || mode == 1), "ys_optim_set_param_groups: mode %d", mode);
  YS_REQUIRE(m->step == 0 || mode == m->group_mode, "ys_optim_set_param_groups: the optimizer has already stepped");
  if (mode == 1 && !m->bn_mask) {
    YS_CHECK_HIP(hipSetDevice(m->ctx->device));
    std::vector<unsigned char> h((size_t)m->n_params, 0);
    for (const auto& c : m->convs)
      if (c.bn) for (int i = 0; i < c.cout; i++) { h[c.g_off + i] = 1; h[c.b_off + i] = 1; }
    YS_TRY(dev_alloc(m, (void**)&m->bn_mask, h.size(), false));
    YS_CHECK_HIP(hipMemcpyAsync(m->bn_mask, h.data(), h.size(), hipMemcpyHostToDevice, m->ctx->stream));
    YS_CHECK_HIP(hipStreamSynchronize(m->ctx->stream));
  }
  m->group_mode = mode;
  return YS_OK;
}

int ys_optim_adamw_step(ys_model* m, const float* lr_per_group, int ngroups, float beta1, float beta2, float eps, float wd) {
  YS_REQUIRE(m && lr_per_group && ngroups >= 1, "ys_optim_adamw_step: bad argument");
  YS_CHECK_HIP(hipSetDevice(m->ctx->device));
  YS_TRY(join_wgrad_stream(m));              // asynchronous segment ends (ys_model_backward_segment_async): every gradient is in before the update
  YsTimer timer(m->ctx, "optim");
  m->step += 1;
  const float bc1 = 1.0f - powf(beta1, (float)m->step), bc2 = 1.0f - powf(beta2, (float)m->step);
  AdamwRanges rg{};                          // one launch for the 3 segments x 3 groups (was nine ~5 us launches)
  auto lr_of = [&](int g) { return lr_per_group[g < ngroups ? g : ngroups - 1]; };
  for (int seg = 0; seg < ys_model::NSEG; seg++)
    for (int g = 0; g < 3; g++) {
      const auto r = m->seg_group[seg][g];
      if (r.count <= 0) continue;
      // reference mode: bn.weight is met first in the "weight" group (lr of group 1), then again in the "bn" group
      rg.off[rg.n] = r.off; rg.count[rg.n] = r.count; rg.lr[rg.n] = lr_of(m->group_mode == 1 && g == 2 ? 1 : g);
      rg.n++;
    }
  AdamwDup dup{};
  if (m->group_mode == 1) {
    const double s1 = 2.0 * (double)m->step - 1.0, s2 = 2.0 * (double)m->step;
    dup.mask = m->bn_mask; dup.lr_second = lr_of(2);
    dup.bc1_first = (float)(1.0 - pow((double)beta1, s1)); dup.bc2s_first = sqrtf((float)(1.0 - pow((double)beta2, s1)));
    dup.bc1_second = (float)(1.0 - pow((double)beta1, s2)); dup.bc2s_second = sqrtf((float)(1.0 - pow((double)beta2, s2)));
  }
  YS_TRY(ys_adamw_ranges_launch(m->ctx->stream, m->params, m->grads, m->adam_m, m->adam_v, m->n_params, rg, beta1, beta2, eps, wd, bc1, bc2,
                                m->group_mode == 1 ? &dup : nullptr));
  m->weights_dirty = true; m->eval_coeffs_dirty = true;
  YS_CHECK_HIP(hipGetLastError());
  return YS_OK;
}


// ------------------------------------------------------------------ standalone blocks (include/yolosharp_hip.h "per-block entry points")
int ys_block_create(ys_ctx* ctx, const ys_block_desc* bd, ys_model** out) {
  YS_REQUIRE(ctx && bd && out, "ys_block_create: null argument");
  YS_REQUIRE(bd->dtype == YS_F32 || bd->dtype == YS_BF16 || bd->dtype == YS_FP8, "ys_block_create: dtype %d unsupported", bd->dtype);
  YS_REQUIRE(bd->height > 0 && bd->width > 0 && bd->max_batch > 0, "ys_block_create: geometry %dx%d batch %d", bd->height, bd->width, bd->max_batch);
  YS_CHECK_HIP(hipSetDevice(ctx->device));
  ys_model* m = new_handle(ctx, bd->dtype, bd->max_batch);
  m->is_block = true; m->blk_c1 = bd->c1; m->blk_c2 = bd->c2; m->A = 0; m->nl = 0;
  m->d = ys_model_desc{}; m->d.height = bd->height; m->d.width = bd->width; m->d.max_batch = bd->max_batch; m->d.dtype = bd->dtype;
  m->d.reg_max = 1; m->d.max_labels = 1;
  return finish_handle(m, build_block(m, *bd), "block.", out);
}

int ys_block_output_shape(ys_model* m, int32_t shape_chw[3]) {
  YS_REQUIRE(m && m->is_block && shape_chw, "ys_block_output_shape: not a block handle");
  const Buf& ob = m->bufs[m->blk_out];
  shape_chw[0] = m->blk_c2; shape_chw[1] = ob.H; shape_chw[2] = ob.W;
  return YS_OK;
}

int ys_block_forward(ys_model* m, const float* x, int on_device, int batch, float* y) {
  YS_REQUIRE(m && m->is_block && x && y, "ys_block_forward: null argument or not a block handle");
  YS_REQUIRE(batch > 0 && batch <= m->maxB, "ys_block_forward: batch %d outside (0, %d]", batch, m->maxB);
  YS_CHECK_HIP(hipSetDevice(m->ctx->device));
  hipStream_t st = m->ctx->stream;
  const Buf& ib = m->bufs[m->in_buf];
  const Buf& ob = m->bufs[m->blk_out];
  const size_t nx = (size_t)batch * m->blk_c1 * ib.rows_per_b, ny = (size_t)batch * m->blk_c2 * ob.rows_per_b;
  const float* src = x;
  if (!on_device) { YS_CHECK_HIP(hipMemcpyAsync(m->img_dev, x, nx * 4, hipMemcpyHostToDevice, st)); src = m->img_dev; }
  m->B = batch;
  YS_TRY(join_wgrad_stream(m));
  YS_TRY(ys_pack_input_launch(st, m->dtype, src, batch, m->blk_c1, ib.H, ib.W, ib.ldc, ib.act));
  YS_TRY(forward_impl(m, batch));
  m->have_fwd = m->training;   // only a training-mode forward keeps what backward needs (pre-BN outputs, batch statistics)
  float* dst = on_device ? y : m->out_stage;
  YS_TRY(ys_unpack_nchw_launch(st, m->dtype, ob.act, ob.ldc, 0, batch, m->blk_c2, ob.rows_per_b, dst));
  if (!on_device) { YS_CHECK_HIP(hipMemcpyAsync(y, m->out_stage, ny * 4, hipMemcpyDeviceToHost, st)); YS_CHECK_HIP(hipStreamSynchronize(st)); }
  return YS_OK;
}

int ys_block_backward(ys_model* m, const float* dy, int on_device, float* dx) {
  YS_REQUIRE(m && m->is_block && dy, "ys_block_backward: null argument or not a block handle");
  YS_REQUIRE(m->have_fwd && m->training, "ys_block_backward: needs a training-mode ys_block_forward first");
  YS_CHECK_HIP(hipSetDevice(m->ctx->device));
  hipStream_t st = m->ctx->stream;
  const int B = m->B;
  const Buf& ib = m->bufs[m->in_buf];
  const Buf& ob = m->bufs[m->blk_out];
  const size_t nx = (size_t)B * m->blk_c1 * ib.rows_per_b, ny = (size_t)B * m->blk_c2 * ob.rows_per_b;
  const float* src = dy;
  if (!on_device) { YS_CHECK_HIP(hipMemcpyAsync(m->out_stage, dy, ny * 4, hipMemcpyHostToDevice, st)); src = m->out_stage; }
  YS_TRY(ys_pack_input_launch(st, m->dtype, src, B, m->blk_c2, ob.H, ob.W, ob.ldc, ob.grad));
  reset_grad_state(m);
  YS_TRY(backward_range(m, 0, ys_model::NSEG - 1));
  if (dx) {
    float* dst = on_device ? dx : m->img_dev;
    YS_TRY(ys_unpack_nchw_launch(st, m->dtype, ib.grad, ib.ldc, 0, B, m->blk_c1, ib.rows_per_b, dst));
    if (!on_device) YS_CHECK_HIP(hipMemcpyAsync(dx, m->img_dev, nx * 4, hipMemcpyDeviceToHost, st));
  }
  YS_CHECK_HIP(hipStreamSynchronize(st));
  return YS_OK;
}


// ---- heads as standalone modules (Head.cs:8-236 Detect, :238-374 Segment, :376-482 Obb, :484-606 Pose): three input buffers + add_detect
int ys_head_create(ys_ctx* ctx, const ys_head_desc* hd, ys_model** out) {
  YS_REQUIRE(ctx && hd && out, "ys_head_create: null argument");
  YS_REQUIRE(hd->dtype == YS_F32 || hd->dtype == YS_BF16 || hd->dtype == YS_FP8, "ys_head_create: dtype %d unsupported", hd->dtype);
  YS_REQUIRE((hd->family == YS_YOLOV8 || hd->family == YS_YOLOV11) && hd->task >= YS_DETECT && hd->task <= YS_CLASSIFY, "ys_head_create: family %d task %d", hd->family, hd->task);
  YS_REQUIRE(hd->nc > 0 && (hd->task == YS_CLASSIFY || (hd->reg_max > 1 && hd->reg_max <= 32)), "ys_head_create: nc=%d reg_max=%d", hd->nc, hd->reg_max);
  if (hd->task == YS_CLASSIFY && hd->dtype == YS_FP8) { ys_set_error("ys_head_create: the Classify head runs in YS_F32 or YS_BF16; YS_FP8 is not built for it"); return YS_ERR_UNSUPPORTED; }
  YS_REQUIRE(hd->height > 0 && hd->width > 0 && hd->height % 32 == 0 && hd->width % 32 == 0, "ys_head_create: image size %dx%d must be a positive multiple of 32", hd->height, hd->width);
  YS_REQUIRE(hd->max_batch > 0, "ys_head_create: max_batch %d", hd->max_batch);
  YS_CHECK_HIP(hipSetDevice(ctx->device));
  ys_model* m = new_handle(ctx, hd->dtype, hd->max_batch);
  m->is_head = true;
  m->d = ys_model_desc{}; m->d.family = hd->family; m->d.task = hd->task; m->d.nc = hd->nc; m->d.reg_max = hd->reg_max;
  m->d.height = hd->height; m->d.width = hd->width; m->d.max_batch = hd->max_batch; m->d.dtype = hd->dtype;
  m->d.kpt_num = hd->kpt_num; m->d.kpt_dim = hd->kpt_dim;
  for (int j = 0; j < 64; j++) m->dfl_w[j] = (float)j;
  int st = YS_OK;
  if (hd->task == YS_CLASSIFY) {   // Classify(c1 = ch[0], nc) on one [height / 32, width / 32] map; ch[1], ch[2] are ignored
    const int c1 = hd->ch[0], h = hd->height / 32, w = hd->width / 32;
    if (c1 <= 0 || c1 % m->epl) { ys_set_error("ys_head_create: ch[0] = %d must be a positive multiple of %d for this dtype", c1, m->epl); st = YS_ERR_UNSUPPORTED; }
    if (st == YS_OK) {
      m->head_in[0] = new_buf(m, h, w, c1); m->head_ch[0] = c1; m->in_buf = m->head_in[0];
      st = add_classify(m, "head", View{m->head_in[0], 0, c1}, c1, h, w, 0);
    }
    m->blk_c1 = (c1 + 1023) / 1024;                                                         // host staging (allocate): c1 * (H / 32) * (W / 32) <= blk_c1 * H * W
    return finish_handle(m, st, "head.", out);
  }
  int hh[3], ww[3], ch[3];
  for (int i = 0; i < 3 && st == YS_OK; i++) {
    hh[i] = hd->height / (8 << i); ww[i] = hd->width / (8 << i); ch[i] = hd->ch[i];
    if (ch[i] <= 0 || ch[i] % m->epl) { ys_set_error("ys_head_create: ch[%d] = %d must be a positive multiple of %d for this dtype", i, ch[i], m->epl); st = YS_ERR_UNSUPPORTED; break; }
    m->head_in[i] = new_buf(m, hh[i], ww[i], ch[i]);
    m->head_ch[i] = ch[i];
  }
  m->in_buf = m->head_in[0];
  if (st == YS_OK) st = add_detect(m, "head", m->head_in, ch, hh, ww, hd->family == YS_YOLOV8, 0);
  int cst = 1;                                                                              // host staging (allocate: B * max(3, blk_c1) * H * W floats)
  for (int i = 0; i < 3 && st == YS_OK; i++) cst = std::max(cst, (ch[i] + (64 << (2 * i)) - 1) / (64 << (2 * i)));   // ch_i * (H / s_i) * (W / s_i) <= cst * H * W
  m->blk_c1 = cst;
  return finish_handle(m, st, "head.", out);                                                // module-relative names (Detect's own state_dict)
}

int ys_head_forward(ys_model* m, const float* const x[3], int on_device, int batch) {
  YS_REQUIRE(m && m->is_head && x && x[0] && (m->cls || (x[1] && x[2])), "ys_head_forward: null argument or not a head handle");
  YS_REQUIRE(batch > 0 && batch <= m->maxB, "ys_head_forward: batch %d outside (0, %d]", batch, m->maxB);
  YS_CHECK_HIP(hipSetDevice(m->ctx->device));
  hipStream_t st = m->ctx->stream;
  YsTimer timer(m->ctx, "forward");
  m->B = batch;
  YS_TRY(join_wgrad_stream(m));   // the level inputs are rewritten below; the previous backward's weight-gradient kernels read them
  for (int i = 0; i < 3; i++) {
    if (m->head_in[i] < 0) continue;                                 // Classify: one input
    const Buf& ib = m->bufs[m->head_in[i]];
    const float* src = x[i];
    if (!on_device) {
      YS_CHECK_HIP(hipMemcpyAsync(m->img_dev, x[i], (size_t)batch * m->head_ch[i] * ib.rows_per_b * 4, hipMemcpyHostToDevice, st));
      src = m->img_dev;
    }
    YS_TRY(ys_pack_input_launch(st, m->dtype, src, batch, m->head_ch[i], ib.H, ib.W, ib.ldc, ib.act));
    if (!on_device) YS_CHECK_HIP(hipStreamSynchronize(st));          // the staging buffer is reused by the next level
  }
  YS_TRY(forward_impl(m, batch));
  m->have_fwd = true; m->fwd_training = m->training; m->have_loss = false; m->have_seg_loss = false;
  return YS_OK;
}

int ys_head_set_grads(ys_model* m, const float* dboxes, const float* dscores, const float* dextra, const float* dproto) {
  YS_REQUIRE(m && m->is_head && dscores && (m->cls || dboxes), "ys_head_set_grads: null argument or not a head handle");
  YS_REQUIRE(m->have_fwd && m->fwd_training, "ys_head_set_grads: needs a training-mode ys_head_forward first");
  if (m->cls) {                    // Classify: dscores = d(loss) / d(logits) [B, nc]; the other arguments are ignored
    YS_CHECK_HIP(hipSetDevice(m->ctx->device));
    hipStream_t st = m->ctx->stream;
    const Buf& b = m->bufs[m->logit_buf];
    YS_CHECK_HIP(hipMemcpyAsync(m->out_stage, dscores, (size_t)m->B * m->d.nc * 4, hipMemcpyHostToDevice, st));
    YS_TRY(ys_pack_input_launch(st, m->dtype, m->out_stage, m->B, m->d.nc, 1, 1, b.ldc, b.grad));
    YS_CHECK_HIP(hipStreamSynchronize(st));
    m->have_loss = true; m->have_seg_loss = true;
    return YS_OK;
  }
  YS_REQUIRE(!m->segment || (dextra && dproto), "ys_head_set_grads: a Segment head needs dmask_coefficient and dproto");
  YS_REQUIRE(m->xkind < 2 || dextra, "ys_head_set_grads: an Obb / Pose head needs the gradient of its angle logits / keypoints");
  YS_CHECK_HIP(hipSetDevice(m->ctx->device));
  hipStream_t st = m->ctx->stream;
  const int B = m->B;
  struct Item { const float* src; int buf; int C; long rows; } items[4] = {
    {dboxes, m->pd_buf, 4 * m->d.reg_max, m->A}, {dscores, m->ps_buf, m->d.nc, m->A},
    {m->segment || m->xkind >= 2 ? dextra : nullptr, m->mc_buf, m->nm, m->A}, {m->segment ? dproto : nullptr, m->pr_buf, m->nm, (long)m->mh * m->mw}};
  for (const Item& it : items) {
    if (!it.src) continue;
    const Buf& b = m->bufs[it.buf];
    const size_t cnt = (size_t)B * it.C * it.rows;
    YS_REQUIRE((long)cnt <= m->n_out_stage, "ys_head_set_grads: staging buffer too small");
    YS_CHECK_HIP(hipMemcpyAsync(m->out_stage, it.src, cnt * 4, hipMemcpyHostToDevice, st));
    YS_TRY(ys_pack_input_launch(st, m->dtype, m->out_stage, B, it.C, 1, (int)it.rows, b.ldc, b.grad));
    YS_CHECK_HIP(hipStreamSynchronize(st));   // out_stage is reused by the next item
  }
  m->have_loss = true; m->have_seg_loss = true;
  return YS_OK;
}

int ys_head_backward(ys_model* m, int on_device, float* const dx[3]) {
  YS_REQUIRE(m && m->is_head, "ys_head_backward: not a head handle");
  YS_REQUIRE(m->have_loss && m->fwd_training, "ys_head_backward: needs a training-mode ys_head_forward and a criterion (ys_loss_*) or ys_head_set_grads first");
  YS_REQUIRE(!m->segment || m->have_seg_loss, "ys_head_backward: the Segment head needs ys_loss_segment (mask gradients)");
  YS_CHECK_HIP(hipSetDevice(m->ctx->device));
  hipStream_t st = m->ctx->stream;
  YsTimer timer(m->ctx, "backward");
  reset_grad_state(m);
  YS_TRY(backward_range(m, 0, ys_model::NSEG - 1));
  for (int i = 0; i < 3 && dx; i++) {
    if (!dx[i] || m->head_in[i] < 0) continue;
    const Buf& ib = m->bufs[m->head_in[i]];
    const size_t n = (size_t)m->B * m->head_ch[i] * ib.rows_per_b;
    float* dst = on_device ? dx[i] : m->img_dev;
    YS_TRY(ys_unpack_nchw_launch(st, m->dtype, ib.grad, ib.ldc, 0, m->B, m->head_ch[i], ib.rows_per_b, dst));
    if (!on_device) { YS_CHECK_HIP(hipMemcpyAsync(dx[i], m->img_dev, n * 4, hipMemcpyDeviceToHost, st)); YS_CHECK_HIP(hipStreamSynchronize(st)); }
  }
  YS_CHECK_HIP(hipStreamSynchronize(st));
  return YS_OK;
}

}  // extern "C"

