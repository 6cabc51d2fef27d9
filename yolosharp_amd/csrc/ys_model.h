// ys_model.h -- the model handle behind the ys_model_* / ys_optim_* / ys_block_* / ys_head_* / ys_loss_* ABI: graph records, struct ys_model and what the
// handle's units call of each other (namespace ysm, at the end).  Shared by graph.hip, plan.hip, model.hip, model_api.hip and criterion.hip only.
#pragma once
#include "ys_internal.h"
#include "ys_kernels.h"

struct View { int buf = -1; int coff = 0; int C = 0; };

struct Buf {
  int H = 0, W = 0, ldc = 0;
  long rows_per_b = 0;   // H*W (or A for head outputs)
  void* act = nullptr;
  void* grad = nullptr;
  bool need_grad = true;
  std::vector<char> gw;  // per-channel "gradient already written in this backward pass"
};

struct ConvL {
  std::string name;      // state_dict prefix
  int cin = 0, cout = 0, k = 1, s = 1;
  int pad = 0;           // zero padding on every side: k / 2 (autopad) unless the module names it (Yolov5u model.0: k 6, p 2)
  int cin_pad = 0;       // channels of the input view (first layer: 3 -> EPL)
  int cout_ld = 0;       // channels incl. padding in the dgrad weight matrix / dy rows
  int cout_real = 0;     // output channels of the reference module.  cout > cout_real only for the Pose towers (51 -> next 16-byte
                         // multiple): the extra rows of every parameter stay zero, so the extra channels are exactly 0 in both BN modes,
                         // receive zero gradients, and the state_dict surface lists the cout_real prefix
  bool bn = true, act = true;
  View in, out, res;
  bool has_res = false;
  int Hin = 0, Win = 0, Hout = 0, Wout = 0;
  long out_rowoff = 0;   // head outputs: first row of this level inside [B][A]
  long w_off = -1, g_off = -1, b_off = -1;   // flat parameter offsets (floats): weight, bn.weight|bias, bn.bias
  long rm_off = -1, rv_off = -1, nbt_off = -1;  // running stats in `state`
  long wf_off = 0, wd_off = 0;               // element offsets into wf_all / wd_all
  long y_off = 0;                             // element offset into y_all (bn layers)
  long acc_off = -1;                          // BatchNorm unit: offset (64-bit words) of its statistics accumulators in ys_model::stat_acc_all
  long ch_off = 0;                            // offset into per-channel scratch (scale.. c2), floats
  int seg = 0;
  bool first = false;
  bool dw = false;       // depthwise 3x3 (groups = channels): weights [9][C] fp32, no MFMA path
  bool f8_fwd = false, f8_bwd = false;   // fp8 mode: forward / dgrad of this layer may run the fp8 kernel (f8.hip recipe)
  int idx = -1, prep_idx = -1;           // own index in ys_model::convs; first PrepDesc (weight-amax slot)
  long wgp_off = -1; int wgp_splits = 0; // own region of the weight-gradient partial workspace (floats) and the splits it holds; -1 = shared scratch + immediate reduce
  int red_slot = -1;                     // index into ys_model::red_host (deferred split reduction)
  bool proto = false;    // a unit of Segment's Proto: runs ONCE per End2End forward (Head.cs:283-307) -- no second statistics update, no one2one backward pass
  bool ct = false;       // ConvTranspose2d(k=2,s=2,bias) = four 1x1 phase GEMMs (Proto.upsample, Block.cs:69); weights [4][Cout][Cin]
  // fused BN-backward reduction (BnRedSeg, ys_kernels.h).  As a consumer: the producers whose dz this layer's dgrad completes
  // (it is their first reader in forward order = last gradient writer in backward order).  As a producer: where its sums come from.
  struct RedFeed { int prod; int c0, c1, yc0; long part_off; int rows_cap, rows; };
  struct RedSrc { int cons, feed; };
  std::vector<RedFeed> feeds;
  std::vector<RedSrc> red_src;           // sorted by producer channel
  bool red_ok = false; int red_seen = 0; // every source is a supported dgrad launch / sources attached in the current backward pass
  // Several reference modules executed as ONE convolution (shared-input fusion, add_detect): member k owns output rows
  // [row0, row0 + rows) of this layer's weight / BN vectors and appears in the state_dict under its own module name.  Empty = one module.
  struct Member { std::string name; int row0, rows; };
  std::vector<Member> members;
  // Level-parallel execution of the head (round 4): `stage` orders the head's ops stage-major (all pyramid levels of one tower layer next
  // to each other); ops of one `group` (>= 0) are consecutive in ys_model::ops, mutually independent, and run as grouped launches
  // (run_conv_fwd_group / run_conv_bwd_group).  Grouped units own their statistics rows and dy buffer (no shared scratch between problems).
  int stage = -1, group = -1;
  long gstat_off = -1;                   // floats into ys_model::stat_group
  void* dy_own = nullptr;
  bool linear = false;     // Classify's Linear(1280, nc) run as a 1x1 convolution on a 1 x 1 map (M = B): state_dict weight [nc, 1280]
  bool pool_next = false;  // Classify's Conv unit: in training its BN + SiLU apply is left to the pool op that follows (OP_POOL reads y)
};

enum OpType { OP_CONV = 0, OP_MAXPOOL = 1, OP_UPSAMPLE = 2, OP_ATTN = 3, OP_VCOPY = 4, OP_COPY = 5, OP_POOL = 6 };   // OP_POOL: Classify's AdaptiveAvgPool2d(1) (op.conv = its Conv unit)
struct Op { int type; int conv = -1; View in, out; int H = 0, W = 0; long aux_off = 0; int seg = 0; int heads = 0, kd = 0, hd = 0; };

struct TensorRec {
  std::string name;
  int ndim = 1; int64_t shape[4] = {1, 1, 1, 1};
  bool is_param = true;
  int kind = 0;     // 0 conv weight (OIHW at the edge), 1 vector in flat params, 2 vector in state, 3 dfl weight
  int conv = -1;
  long off = 0, count = 0;
};

struct PrepDesc { long w_off, wf_off, wd_off, nf_start, nd_start; int cout, taps, cin_real, cin_pad, cout_pad, has_wd, phase;
                  long tile_start; int tiles_ci, tiles_co, layer, pad_; };   // round 5 (weight_prep_fast_kernel): 64 x 64 transpose tiles of the dgrad shadow, prefix over the table; layer = index in the full table (weight-amax slot)

struct ys_model {
  ys_ctx* ctx = nullptr;
  ys_model_desc d{};
  int dtype = 0, epl = 4; size_t es = 4;
  int maxB = 0, B = 0;
  int A = 0, nl = 3;
  int lvl_off[4] = {0}, lvl_w[4] = {0}, lvl_h[4] = {0}, lvl_stride[4] = {8, 16, 32, 64};
  bool training = true;
  std::vector<Buf> bufs;
  std::vector<ConvL> convs;
  std::vector<Op> ops;
  std::vector<TensorRec> tensors;
  std::vector<int> reg;          // conv indices in the reference's module REGISTRATION order (state_dict order)
  std::string head_prefix;       // "model.22" (v8) / "model.23" (v11)
  float* attn_ws = nullptr; long n_attn = 0;   // softmax probabilities + dS of the C2PSA attention ops
  // segmentation (Head.cs:238-324): mask coefficients [B][A][ld_mc], prototypes [B][mh*mw][ld_pr]
  bool segment = false; int nm = 0, mc_buf = -1, pr_buf = -1, ld_mc = 0, ld_pr = 0, mh = 0, mw = 0;
  // Obb (Head.cs:376-482) / Pose (Head.cs:484-606) reuse the cv4 output buffer: nm = ne (1) / nk (kpt_num * kpt_dim) channels
  float* kp_dev = nullptr;       // Pose: staged keypoint labels [max_labels][K][D] (grows with the label workspace)
  int xkind = 0, kdim = 3;       // 0 none, 1 mask coefficients, 2 angle logit, 3 keypoints (argument of ys_detect_decode_launch)
  float* masks_dev = nullptr; int *seg_cnt = nullptr, *seg_off = nullptr, *seg_list = nullptr; float *seg_ent = nullptr, *seg_part = nullptr;
  int n_items = 3; bool have_seg_loss = false;
  int dfl_after_conv = -1;   // the DFL weight registers right after Detect's cv2/cv3 (Head.cs:52-56), before Segment's proto/cv4
  int in_buf = -1, pd_buf = -1, ps_buf = -1;
  bool is_block = false; int blk_out = -1, blk_c1 = 3, blk_c2 = 0;   // standalone block handle (ys_block_create)
  bool is_head = false; int head_in[3] = {-1, -1, -1}, head_ch[3] = {0, 0, 0};   // standalone head handle (ys_head_create): P3 / P4 / P5 input buffers
  int ld_pd = 0, ld_ps = 0;
  // Classify (Head.cs:612-644): pooled [B][1280] and logits [B][ld_cls] buffers (1 x 1 maps), per-row losses + invalid-label flags [2B]
  bool cls = false; int cls_conv = -1, pool_buf = -1, logit_buf = -1, ld_cls = 0;
  float *cls_rows = nullptr, *cls_lab = nullptr;
  // flat fp32 parameter state
  long n_params = 0, n_params_real = 0;          // flat length incl. the zero rows of padded towers / the reference's parameter count
  float *params = nullptr, *grads = nullptr, *adam_m = nullptr, *adam_v = nullptr;
  float* state = nullptr; long n_state = 0;     // running_mean / running_var / num_batches_tracked
  float dfl_w[64];
  struct Range { long off, count; };
  static constexpr int NSEG = 4;                 // backward segments: head, neck, late backbone, stem (the last, exposed all-reduce is the smallest)
  Range seg_group[NSEG][3];                      // [segment][adamw group]
  long step = 0;
  // fp8 mode (ys_dtype YS_FP8: bf16 storage + fp8 MFMA convolutions, f8.hip)
  bool f8 = false, f8_sx_valid = false, f8_sg_valid = false, f8_bwd_done = false;
  unsigned char *wf8_all = nullptr, *wd8_all = nullptr;
  int q8_fwd_ready = -1;                  // forward: conv index whose input image already sits in q8 (written by its producer's BN pass)
  unsigned char* q8 = nullptr;            // scratch: fp8 image of one convolution input (blocked-GEMM fp8 kernel, quantised by ys_conv_launch)
  float *amax_w = nullptr, *f8_scales = nullptr; unsigned *amax_act = nullptr, *amax_dy = nullptr;
  F8Layer* f8_layers = nullptr; F8Conv* f8_convs = nullptr; int n_f8_convs = 0; long n_wf_pending = 0, n_wd_pending = 0;
  int group_mode = 0;                            // 0 = disjoint groups, 1 = the reference's overlapping groups as written
  unsigned char* bn_mask = nullptr;              // [n_params] 1 = BatchNorm weight / bias (listed twice in the reference's groups)
  // T weights
  void *wf_all = nullptr, *wd_all = nullptr; long n_wf = 0, n_wd = 0;
  PrepDesc* prep_dev = nullptr; int n_prep = 0; long prep_nf = 0, prep_nd = 0;
  bool prep_fast = false;
  PrepDesc* prep_tile_dev = nullptr; int n_prep_tile = 0; long prep_tiles = 0;          // layers whose dgrad shadow is a plain transpose (tile_start prefix)
  PrepDesc* prep_phase_dev = nullptr; int n_prep_phase = 0; long prep_nd_phase = 0;     // stride-2 layers with phase-major dgrad shadows (nd_start = compact prefix)
  bool weights_dirty = true, eval_coeffs_dirty = true;
  // activations
  void* y_all = nullptr; long n_y = 0;
  void* dy_scratch = nullptr; long n_dy = 0;
  // weight gradients run on a second stream, concurrently with the BN-backward / dgrad chain of the following layers
  // (both mostly latency-bound).  A hand-over is one event recorded on the main stream that the second stream waits for: N_HAND + 1 events, taken in
  // rotation by flush_wgrads (all of them, in index order); the ConvTranspose path always records the last one (run_convT_bwd)
  static constexpr int N_HAND = 4;
  // round 6: weight gradients are handed to the second stream in BATCHES.  Every BatchNorm unit keeps its own dy buffer (ConvL::dy_own: nothing shared to wait for),
  // a unit's weight-gradient launch is queued instead of issued, and ONE event record / wait pair hands a whole batch over (flush_wgrads).  A rocprofv3 trace of
  // config 2 showed what the per-layer hand-off cost: every hipEventRecord between two kernels of the main stream is a ~6.6 us bubble (29 + 10 + 5 of them per step
  // between bn_bwd_apply and the dgrad that follows) and every ring-slot wait another ~6 us (21 per step): 0.6 ms of an 8.7 ms step with no kernel running on
  // the main stream, all of it in the backward pass (the forward has none).
  struct PendWg { int conv; const void* dy; int ldc, coff; long bstride; bool bnb; };   // bnb: dy is dz, the BatchNorm backward runs inside the kernel (model.0)
  std::vector<PendWg> pend_wg; double pend_mb = 0.0; int hand_next = 0;
  bool hold_stem = false;                      // one-call backward: model.0's weight gradient stays queued until the segment end (backward_range: stem_split)
  // head lanes (round 3): the towers of the three pyramid levels are independent chains (own buffers, own rows of the prediction buffers);
  // the P4 / P5 chains are short, latency-bound launches (100-400 workgroups) that run beside the P3 chain on two side streams
  // asynchronous segment ends (data-parallel step): the weight-gradient stream is NOT joined into the main stream when a backward segment
  // ends; the segment's completion is two events (main stream, weight-gradient stream) a communication stream waits on (ys_model_segment_fence)
  hipEvent_t ev_seg_m[NSEG] = {nullptr, nullptr, nullptr, nullptr}, ev_seg_w[NSEG] = {nullptr, nullptr, nullptr, nullptr};
  bool seg_on_st2[NSEG] = {false, false, false, false};
  bool overlap = false, overlap_built = false; hipStream_t st2 = nullptr;   // overlap_built: second stream / per-unit dy buffers / hand-over events exist; overlap: in use (ys_model_set_overlap)
  hipEvent_t ev_hand[N_HAND + 1] = {nullptr}, ev_join = nullptr;    // hand-over events (a wait binds to the record that preceded it)
  bool st2_dirty = false;
  float* chan = nullptr; long n_chan = 0;       // per conv: scale, shift, mean, rstd, c1, c2 (6*cout)
  float* stat_partial = nullptr; long n_stat = 0;
  unsigned long long* stat_acc_all = nullptr; long n_stat_acc = 0;   // round 5: [unit][YS_STAT_SHARDS][cout][2] fixed-point statistics sums, cleared by ONE memset per training forward
  bool bn_atomic = false;                                            // BatchNorm units take their statistics through them and finalize inside the apply pass
  float* stat_group = nullptr;                  // statistics rows of the grouped head stages (one region per unit, ConvL::gstat_off)
  float* wg_partial = nullptr; long n_wgp = 0;   // [shared scratch (ConvTranspose phases) | one region per convolution]
  // deferred split reduction of the weight gradients: one batched launch per backward_range call instead of one per layer
  std::vector<WgRedDesc> red_host, red_uploaded; WgRedDesc* red_dev = nullptr; int red_first[NSEG + 1] = {0, 0, 0, 0, 0}; int red_proto0 = 0;   // red_proto0: first descriptor of Proto's units in segment 0 (they sort last there)
  bool defer_wgred = true;
  // fused BN-backward reduction: planned per batch size (plan_bnred), partial rows of every (producer, consumer) pair
  bool bnred_on = true; int bnred_B = -1; float* bnred_part = nullptr; long n_bnred = 0;
  unsigned char* argmax = nullptr; long n_argmax = 0;
  float* img_dev = nullptr;                      // staging for host images
  bool stem_on = true;                           // YS_STEM_DIRECT=0 at creation: model.0 reads the packed bf16 copy like every other layer
  bool stem_bnb_fuse = true;                     // YS_STEM_BNB_FUSE=0 at creation: model.0's BatchNorm backward apply pass runs on its own
  bool sppf_fuse = true;                         // YS_SPPF_FUSE=0 at creation: SPPF's three pools run as three launches (the fused form's reference)
  const float* in_f32 = nullptr;                 // the fp32 NCHW image of the current step when model.0 reads it directly (conv_stem.hip); null = the packed input buffer holds it
  float* pred = nullptr;                         // [B][4+nc][A] fp32 (eval)
  float* out_stage = nullptr; long n_out_stage = 0;
  // loss
  int gcap = 64; int max_labels = 0;
  float *lab_bidx = nullptr, *lab_cls = nullptr, *lab_box = nullptr;
  int* gt_count = nullptr; float* gt_box = nullptr; int* gt_cls = nullptr; float* pbox = nullptr;
  float *ov = nullptr, *align = nullptr; unsigned char* mpos = nullptr; unsigned *pos_align = nullptr, *pos_ov = nullptr;
  int* fg_gt = nullptr; float* tnorm = nullptr; float* loss_partial = nullptr; float* scalars = nullptr;
  // End2End (criterion.hip; Head.cs:89-127, 152-167): the one2one towers ALIAS cv2 / cv3 -- no tensors of their own.  Their criterion pass writes its
  // gradients and scalars here; the eval forward adds the top-k rows "det" [B][k][6 + nm] (Detect: nm = 0; Segment: + the anchor's coefficients; OBB: + the angle; Pose: + the decoded keypoints)
  bool e2e = false; int max_det = 300;
  void *o2o_dpd = nullptr, *o2o_dps = nullptr, *o2o_dmc = nullptr; float* scalars2 = nullptr;
  // Segment (Head.cs:245-357, Proto runs once) and OBB (Head.cs:454-469) alias cv4 as well.  E2ESegmentLoss / E2EOBBLoss weight their two criteria with the
  // gains o2m / o2o (0.8 / 0.2 until ys_model_e2e_update moves them); every other model keeps 1 / 1 (E2EDetectLoss is unweighted).  "pred" of an OBB model
  // keeps its xywh + angle form (Obb.decode_bboxes ignores end2end, Head.cs:434-437).  Pose (Head.cs:485-610; E2EPoseLoss, Loss.cs:1238-1295) aliases cv4 the
  // same way: o2o_dmc holds the one2one gradient of the raw keypoints, "pred" takes xyxy boxes (Detect.decode_bboxes, Head.cs:201) and det_rows is [B][k][6 + nk]
  bool e2e_cv4() const { return e2e && (segment || xkind >= 2); }
  float o2m = 1.0f, o2o = 1.0f; int e2e_updates = 0, e2e_epochs = 100;
  float* det_rows = nullptr; long long* det_anchor = nullptr; void* det_ws = nullptr;
  int head_conv0 = 0, det_in[3] = {-1, -1, -1};       // first tower unit in `convs`; the three feature maps the head reads
  // the towers' running statistics as contiguous runs of `state` (Detect: one, the tail; Segment: Proto's units lie between cv3 and cv4 and are left out);
  // snapshot and num_batches_tracked mask hold the runs back to back (n_hstate words)
  long n_hstate = 0; float* hstate_snap = nullptr; unsigned char* hstate_count = nullptr;
  Range hstate_rng[4]; int n_hstate_rng = 0;
  bool e2e_pass = false;                              // backward: the one2one pass through the towers is running (no gradient into det_in)
  bool have_fwd = false, have_loss = false;
  bool fwd_training = false;   // the last forward kept what backward needs (training-mode BN statistics, pre-BN outputs)
  std::vector<void*> allocs;
};

// What the units behind the handle call of each other.  Everything else in them is file-local.
namespace ysm {

constexpr float BN_EPS = 1e-3f, BN_MOMENTUM = 0.03f;   // every BatchNorm2d of the reference (Modules/Convs.cs:36-62)

inline char* view_ptr(ys_model* m, void* base, const Buf& b, long row0) { return (char*)base + (size_t)row0 * b.ldc * m->es; }

// graph.hip -- the op list: buffers, Conv units, blocks, heads and the whole-model graphs
int new_buf(ys_model* m, int H, int W, int C);
int add_detect(ys_model* m, const std::string& hp, const int* pv, const int* ch, const int* hh, const int* ww, bool legacy, int seg);
int add_classify(ys_model* m, const std::string& hp, View in, int c1, int H, int W, int seg);
int build_v8_detect(ys_model* m);
int build_v8_classify(ys_model* m);
int build_v11_detect(ys_model* m);
int build_v5u_detect(ys_model* m);
int build_v11_classify(ys_model* m);
int build_block(ys_model* m, const ys_block_desc& bd);

// plan.hip -- parameter layout, weight shadows, every allocation, and the plans the step follows
int dev_alloc(ys_model* m, void** p, size_t bytes, bool zero = true);   // hipMalloc tracked in ys_model::allocs (freed with the model), zero-filled on the stream
int alloc_label_ws(ys_model* m, int gcap);                              // (re)allocates the criterion's ground-truth workspace for gcap labels per image
int layout_params(ys_model* m);
int allocate(ys_model* m);
int prep_weights(ys_model* m);             // master weights -> forward / dgrad shadows, when they changed
bool stem_direct(const ys_model* m);       // model.0 reads the fp32 image planes itself (conv_stem.hip)
bool stem_bnb_planned(const ys_model* m);  // ... and its BatchNorm backward runs inside its weight-gradient kernel
int plan_bnred(ys_model* m, int B);        // fused BN-backward reduction: which dgrad launches feed which producers
// Weight-gradient geometry of layer c reading dy as a [M][dy_ldc] view -- THE place that fills it: workspace sizing (allocate) and launch see the same plan.
// phase >= 0: that output phase of a ConvTranspose unit (1x1 GEMM over the input grid, dy rows strided over the 2x grid).  x / dy / partial are the caller's.
WgradArgs wgrad_args(const ys_model* m, const ConvL& c, int B, int dy_ldc, int dy_coff, long dy_bstride, int phase = -1);

// model.hip -- the step
ConvArgs dgrad_args(ys_model* m, const ConvL& c, int B, const void* dy, int dy_ldc, int dy_coff, long dy_bstride);
void f8_dgrad_operands(const ys_model* m, const ConvL& c, ConvArgs& a);   // fp8 dgrad: e4m3 dgrad weights and the unit's gradient scale pair (plan_bnred predicts with the same)
int join_wgrad_stream(ys_model* m);        // order the main stream behind the weight-gradient stream
int forward_impl(ys_model* m, int B);
int eval_tail(ys_model* m, int B);         // decode + Segment coefficient append + End2End top-k on the head buffers of B images
void reset_grad_state(ys_model* m);
// async_end: leave the weight-gradient stream unjoined (its split reduction runs there too) and record the segment's completion events
int backward_range(ys_model* m, int seg_lo, int seg_hi, bool async_end = false, bool seg_events = true);

}  // namespace ysm
