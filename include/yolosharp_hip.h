/* yolosharp_hip.h -- C ABI of libyolosharp_hip.so: an MI355X (gfx950) native engine for the
 * YOLO forward / loss / backward / AdamW / NMS hot path of IntptrMax/YoloSharp.
 *
 * The reference has no FFI of its own (it is 100 % managed C# on TorchSharp); the "operator API"
 * it exposes is the TorchSharp module surface.  Each entry point below names the reference
 * interface (file:line under /root/reference/YoloSharp) whose arithmetic it replaces.  A C# host
 * binds these with P/Invoke; tests bind them with ctypes.
 *
 * Conventions: extern "C", blittable arguments only, opaque handles, int32 status return
 * (YS_OK == 0), thread-local error text via ys_last_error(), no callbacks, no exceptions across
 * the boundary.  Tensors crossing the edge are plain fp32 in the reference's own layouts
 * (images NCHW, weights OIHW, predictions [B,C,A]); internal layouts (NHWC bf16/f32) never leak.
 * Pointers flagged `on_device` are HIP device pointers that are already resident in HBM;
 * otherwise they are host pointers and the call copies (and, for outputs, synchronises).
 * One HIP stream per ys_ctx; calls on one ctx must be serialised by the caller.
 */
#ifndef YOLOSHARP_HIP_H
#define YOLOSHARP_HIP_H
#include <stdint.h>
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

#define YS_API __attribute__((visibility("default")))

typedef struct ys_ctx ys_ctx;
typedef struct ys_model ys_model;

enum ys_status {
  YS_OK = 0,
  YS_ERR_INVALID_ARG = 1, /* mirrors the reference's ArgumentException (e.g. Ops.cs:248-255) */
  YS_ERR_HIP = 2,
  YS_ERR_OOM = 3,
  YS_ERR_UNSUPPORTED = 4,
  YS_ERR_STATE = 5
};
/* compute/storage type of activations+weights.  YS_FP8 (BASELINE config 5): bf16 storage, statistics and optimizer with the
 * forward / input-gradient convolutions on the fp8 MFMA path -- e4m3 weights (current per-tensor scale) and activations, e5m2
 * gradients (delayed per-tensor scales), fp32 accumulation; layers whose channel count is not a multiple of 32 stay in bf16. */
enum ys_dtype { YS_F32 = 0, YS_BF16 = 1, YS_FP8 = 2 };
enum ys_family { YS_YOLOV5U = 5, YS_YOLOV8 = 8, YS_YOLOV11 = 11 };   /* Models/Yolo.cs:137-198, :10-135, :200-258.  YS_YOLOV5U: the detect task only
                                                                        (with End2End); its other tasks are refused with YS_ERR_UNSUPPORTED */
enum ys_size { YS_N = 0, YS_S = 1, YS_M = 2, YS_L = 3, YS_X = 4 }; /* Types/YoloTypes.cs YoloSize; Yolo.cs:43-51 */
enum ys_task { YS_DETECT = 0, YS_SEGMENT = 1, YS_OBB = 2, YS_POSE = 3,
               YS_CLASSIFY = 4 };   /* Config.cs TaskType.  YS_CLASSIFY: Yolov8Classify / Yolov11Classify (Models/Yolo.cs:537-573),
                                       the Yolov8 list without its last 14 modules (model.0-8, no SPPF) / the Yolov11 list without its last
                                       13 (model.0-10) + Head.Classify (Modules/Head.cs:612-644) as model.9 / model.11: Conv(c1, 1280, 1),
                                       AdaptiveAvgPool2d(1), flatten, Dropout(0), Linear(1280, nc).  YS_F32 and YS_BF16 only (YS_FP8 is
                                       refused with YS_ERR_UNSUPPORTED); reg_max is not used */

YS_API const char* ys_last_error(void);
YS_API int ys_version(void);
/* 1 when built by hipcc for gfx950, 0 for the test-only CPU interpreter build (never shipped). */
YS_API int ys_is_device_build(void);

/* ---- context: one device + one stream ------------------------------------------------------ */
YS_API int ys_ctx_create(int device, ys_ctx** out);
/* Same, but run on a caller-owned hipStream_t (e.g. torch's current stream) so that RCCL
 * collectives issued by the host order correctly against the engine's kernels. */
YS_API int ys_ctx_create_on_stream(int device, void* hip_stream, ys_ctx** out);
YS_API int ys_ctx_destroy(ys_ctx* ctx);
YS_API int ys_ctx_synchronize(ys_ctx* ctx);
YS_API void* ys_ctx_stream(ys_ctx* ctx);

/* ---- model: replaces Models/Yolo.cs Yolov8 (:10-135) built from Modules/Convs.cs Conv (:36-62),
 *      Modules/Block.cs C2f (:371-399) / Bottleneck (:572-608) / SPPF (:236-285),
 *      Modules/Head.cs Detect (:8-236) ---------------------------------------------------------- */
typedef struct ys_model_desc {
  int32_t family;     /* ys_family */
  int32_t size;       /* ys_size */
  int32_t task;       /* ys_task */
  int32_t nc;         /* number of classes (Config.NumberClass) */
  int32_t reg_max;    /* DFL bins (16) */
  int32_t height;     /* input H (multiple of 32) */
  int32_t width;      /* input W (multiple of 32) */
  int32_t max_batch;  /* capacity; forward may use any B <= max_batch */
  int32_t dtype;      /* ys_dtype: YS_F32 = parity path, YS_BF16 = performance path, YS_FP8 = bf16 + fp8 MFMA convolutions */
  int32_t max_labels; /* initial capacity of ground-truth rows PER IMAGE for the loss (0 = 64).  Not a limit: host-label loss calls
                         grow the workspace to the batch's largest per-image count (the reference pads to counts.max(),
                         Utils/Loss.cs:363-390); device-label callers reserve with ys_model_reserve_labels */
  int32_t kpt_num;    /* YS_POSE: keypoints per object (0 = 17, Models/Yolo.cs:473) */
  int32_t kpt_dim;    /* YS_POSE: 2 = (x, y), 3 = (x, y, visibility) (0 = 3) */
} ys_model_desc;

/* Built: YS_YOLOV8 / YS_YOLOV11 for all five tasks; YS_YOLOV5U (Yolo.cs:137-198: Conv(3, c, 6, 2, 2) stem, C3 blocks, SPPF, the Yolov8 Detect head as
 * model.24) for YS_DETECT in YS_F32 / YS_BF16 -- its segment / obb / pose / classify tasks and YS_FP8 return YS_ERR_UNSUPPORTED.  The size parameter is
 * honoured for every family (the reference's Detector.cs:17 never passes yoloSize for Yolov5u, so a reference v5u detector is always size n). */
YS_API int ys_model_create(ys_ctx* ctx, const ys_model_desc* desc, ys_model** out);
YS_API int ys_model_destroy(ys_model* m);

/* state_dict surface (names and order as TorchSharp's named_parameters()+buffers, e.g.
 * "model.0.conv.weight" [16,3,3,3]; Yolo.cs:10-39, YoloBaseTaskModel.cs:31-32,470-490). */
YS_API int ys_model_num_tensors(ys_model* m);
YS_API int ys_model_tensor_info(ys_model* m, int index, char* name, int name_cap,
                                int32_t* ndim, int64_t shape[4], int32_t* is_param);
/* OIHW / [C] fp32 host arrays at the edge. */
YS_API int ys_model_set_tensor(ys_model* m, const char* name, const float* host, size_t count);
YS_API int ys_model_get_tensor(ys_model* m, const char* name, float* host, size_t count);
YS_API int ys_model_get_grad(ys_model* m, const char* name, float* host, size_t count);
/* PyTorch-default initialisation of every tensor (kaiming-uniform(a=sqrt 5) conv weights and
 * biases, BN gamma=1 beta=0, running stats 0/1) from a 64-bit seed (deterministic, host-side). */
YS_API int ys_model_init_weights(ys_model* m, uint64_t seed);
YS_API int ys_model_set_training(ys_model* m, int training);   /* Module.train()/eval() */
YS_API int ys_model_num_anchors(ys_model* m);                  /* A = sum_l (H/s_l)(W/s_l); 0 for a classify model */
YS_API int64_t ys_model_num_params(ys_model* m);

/* Yolov8.forward (Yolo.cs:92-134).  images: fp32 NCHW [B,3,H,W] in [0,1].
 * training: Detect returns preds only (Head.cs:89-106): "boxes" [B,4*reg_max,A], "scores" [B,nc,A].
 * eval: additionally Detect._inference (Head.cs:204-223): "pred" [B,4+nc,A] (xywh*stride, sigmoid). */
YS_API int ys_model_forward(ys_model* m, const float* images, int on_device, int batch);
/* Predict-side input path (Models/Detector.cs:31-41): uint8 RGB planes [B,3,h,w] (0..255) are padded on the bottom / right
 * with 114 up to the model's (height, width), divided by 255 and packed on the device; then the forward above. */
YS_API int ys_model_forward_u8(ys_model* m, const uint8_t* images, int on_device, int batch, int h, int w);
/* Copy an output to a host fp32 array in the reference layout: key = "boxes" | "scores" | "pred";
 * Segment models (Head.cs:283-313) add "mask_coefficient" [B,nm,A] and "proto" [B,nm,H/4,W/4], and their eval
 * "pred" is [B,4+nc+nm,A] (raw mask coefficients appended).  "dboxes" | "dscores" | "dmask_coefficient" | "dproto"
 * return the loss gradients w.r.t. those outputs after a loss call. */
/* Classify models (Head.cs:635-643) have their own keys, all [B, nc]: "cls" = the logits after a training forward, softmax(logits, 1)
 * after an eval forward; "logits" = the logits in both modes; "dcls" = d(loss)/d(logits) after ys_loss_classify.  Every other key
 * is refused on a classify model (YS_ERR_INVALID_ARG), and these keys on the other tasks. */
/* "model0_raw" (full models, after a training-mode forward): the raw (pre-BatchNorm) output of model.0, [B, c, H/2, W/2], as stored; "model0_dy" (after the
 * backward; refused where the BatchNorm backward runs inside the stem's weight-gradient kernel): the gradient w.r.t. it.  The tensors the stem routes
 * (STEM_DIRECT = 1 / 0) are compared on. */
YS_API int ys_model_get_output(ys_model* m, const char* key, float* host, size_t count);
/* The criterion's `preds` argument supplied by the caller (Utils/Loss.cs:411 `forward(preds, batch)`): host fp32 head outputs in the
 * reference layout -- boxes [B,4*reg_max,A], scores [B,nc,A], and for Segment models mask_coefficient [B,nm,A] + proto
 * [B,nm,H/4,W/4] (NULL otherwise) -- become the engine's head buffers, as if a forward had produced them.  ys_loss_detect /
 * ys_loss_segment and the "dboxes" / "dscores" / "dmask_coefficient" / "dproto" outputs then work on them; ys_model_backward
 * is refused (there is no graph state behind such preds). */
YS_API int ys_model_set_preds(ys_model* m, int batch, const float* boxes, const float* scores,
                              const float* mask_coefficient, const float* proto);
/* The tail of an eval forward alone: Detect._inference (and the Segment / Obb / Pose forms; End2End: the top-k post-process too) on the head
 * buffers as they stand, for the batch of the last ys_model_set_preds / forward -> "pred" (and "det").  After ys_model_set_preds: the decode of the
 * caller's values; after an eval forward: the same "pred" again, bit for bit.  Needs eval mode, a Detect / Segment / OBB / Pose model (or head
 * handle) and a prior ys_model_set_preds or forward: YS_ERR_INVALID_ARG otherwise.  Asynchronous. */
YS_API int ys_model_decode_preds(ys_model* m);
/* Device pointer of the eval prediction [B,4+nc,A] fp32 (input of ys_nms_batched); classify models: the eval probabilities [B,nc]. */
YS_API int ys_model_pred_device(ys_model* m, float** dptr);

/* v8DetectionLoss.forward (Utils/Loss.cs:411-484) + TaskAlignedAssigner (Utils/Tal.cs:13-258)
 * + BboxLoss/DFLoss (Loss.cs:94-167) + bbox_iou CIoU (Utils/Metrics.cs:36-111), and d(sum(loss*B))/d(preds).
 * Labels use the collate contract (Data/YoloDataLoader.cs:18-44): batch_idx[n], cls[n], bboxes[n,4]
 * normalised cxcywh, all fp32.  Asynchronous: results stay on the device until ys_loss_read.
 * Works after a training-mode forward (the step's criterion, Amp.cs:338-348) and after an eval-mode forward (the validation loss
 * on the eval preds, Models/Detector.cs:94-97); only ys_model_backward needs the training-mode forward.
 * Label capacity: with host labels the padded ground-truth workspace grows to the batch's largest per-image label count, like
 * the reference's counts.max() (Loss.cs:376-380).  With device labels (no host sync) an image holding more labels than the
 * workspace makes ys_loss_read* return YS_ERR_INVALID_ARG -- never a silently truncated assignment; reserve first. */
YS_API int ys_loss_detect(ys_model* m, const float* batch_idx, const float* cls, const float* bboxes,
                          int n_labels, int on_device);
/* loss_items[3] = (box, cls, dfl) un-multiplied (the reference's loss_detach), *loss_sum = sum(items)*B
 * (the scalar the reference calls backward() on, Amp.cs:340).  Synchronises the stream. */
YS_API int ys_loss_read(ys_model* m, float loss_items[3], float* loss_sum);
/* Grow the per-image ground-truth capacity of the loss workspace ahead of device-label calls (no-op when already large enough). */
YS_API int ys_model_reserve_labels(ys_model* m, int per_image);

/* ---- End2End detection (Config.End2End, Data/Config.cs:239; Models/Detector.cs:17-23).
 * ys_model_one2one_init = YoloBaseTaskModel.One2one_Init -> Detect.one2one_init (Modules/Head.cs:152-167): the one2one towers are the SAME
 * modules as cv2 / cv3 (the reference copies references, SaveWeight drops the one2one keys), so the model gains NO tensor: ys_model_num_tensors /
 * tensor_info / num_params are unchanged and weight files move freely between End2End and plain models.  max_det: rows of the post-process
 * (0 = 300, Head.cs:13).  YS_DETECT models of every family (YS_YOLOV5U carries the same Detect head) and every dtype built for it; Segment / OBB / Pose / Classify models and the standalone block /
 * head handles return YS_ERR_UNSUPPORTED (Segment models take ys_model_e2e_init, OBB models ys_model_e2e_obb_init, Pose models ys_model_e2e_pose_init below).  Call it once, after ys_model_create.  From then on:
 *   training forward (Head.cs:89-106): "one2one_boxes" / "one2one_scores" are outputs (the same values as "boxes" / "scores": same modules,
 *     same input values); the BatchNorm units of the towers update their running statistics twice, num_batches_tracked += 2.
 *   ys_loss_detect = E2EDetectLoss (Utils/Loss.cs:1094-1118): v8DetectionLoss(tal_topk 10) on one2many + v8DetectionLoss(tal_topk 1) on
 *     one2one; ys_loss_read / ys_loss_read_items return the SUM of the two item triples and losses; "dboxes" / "dscores" are the one2many
 *     gradients, "one2one_dboxes" / "one2one_dscores" the one2one ones.  ys_model_set_preds feeds both branches.
 *   ys_model_backward and its segment / async / all-reduce forms: tower parameters receive the gradients of both branches, the three feature
 *     maps (and everything below) the one2many gradient only (the one2one branch reads x.detach()).
 *   eval forward (Head.cs:107-127, 199-202): "pred" [B, 4+nc, A] holds xyxy boxes (x stride); "det" [B, k, 6] = (x1, y1, x2, y2, score,
 *     class), k = min(max_det, A), is ys_e2e_topk of it.  ys_model_det_device: the device pointer of "det" and k. */
YS_API int ys_model_one2one_init(ys_model* m, int max_det);
YS_API int ys_model_det_device(ys_model* m, float** rows, int* k);
/* ---- End2End for Segment models (Models/Segmenter.cs:17-24; Segment.one2one_init, Modules/Head.cs:245-357; E2ESegmentLoss, Utils/Loss.cs:1179-1236).
 * ys_model_e2e_init is One2one_Init for YS_DETECT models (identical to ys_model_one2one_init; `epochs` ignored) AND for YS_SEGMENT models of both
 * families and every dtype; OBB / Pose / Classify models and the block / head handles return YS_ERR_UNSUPPORTED, a second call YS_ERR_STATE.
 * max_det 0 = 300; epochs 0 = 100 (the length of the criterion's gain schedule).  ys_model_one2one_init keeps refusing Segment models.  The towers
 * cv2, cv3 AND cv4 are aliased, so again NO tensor is added and `.bin` files move freely between plain and End2End Segment models.  From then on:
 *   training forward (Head.cs:89-106, 283-307): the one2one branch = the three towers again on x.detach(); Proto runs ONCE (one2one["proto"] =
 *     proto.detach()).  "one2one_boxes" / "one2one_scores" / "one2one_mask_coefficient" are the one2many values; the BatchNorm units of cv2 / cv3 / cv4
 *     move their running statistics twice per forward (num_batches_tracked += 2), Proto's once.
 *   ys_loss_segment = E2ESegmentLoss: v8SegmentationLoss(tal_topk 10) on one2many and v8SegmentationLoss(tal_topk 7, tal_topk2 1) on one2one,
 *     combined as o2m * L_one2many + o2o * L_one2one -- ys_loss_read_items returns the weighted 5 items, *loss_sum their sum * B.  ys_loss_segment is the
 *     only criterion entry of such a model: ys_loss_detect on it returns YS_ERR_INVALID_ARG.  tal_topk2 = 1
 *     (Utils/Tal.cs:242-250): after anchors claimed by several boxes are resolved, every box keeps its single best positive (ys_tal_keep_best).
 *     "dboxes" / "dscores" / "dmask_coefficient" / "dproto" are the one2many gradients (x o2m), "one2one_dboxes" / "one2one_dscores" /
 *     "one2one_dmask_coefficient" the one2one ones (x o2o); the one2one branch sends nothing into the prototypes.
 *   gains: o2m = 0.8, o2o = 0.2 at creation.  ys_model_e2e_update = E2ESegmentLoss.update(): updates += 1; o2m = max(1 - updates /
 *     max(epochs - 1, 1), 0) * 0.7 + 0.1; o2o = max(1 - o2m, 0).  The reference's training loop calls update() for E2EOBBLoss only
 *     (YoloBaseTaskModel.cs:350-353), so ITS Segment runs stay at 0.8 / 0.2; call it once per epoch to get the schedule.  On a Detect End2End
 *     model the gains are 1 / 1 (E2EDetectLoss is unweighted) and ys_model_e2e_update does nothing.
 *   backward (all forms): towers receive o2m * g_one2many + o2o * g_one2one; the feature maps, Proto and everything below o2m * g_one2many.
 *   eval forward (Head.cs:107-127, 309-339): "pred" [B, 4+nc+nm, A] with xyxy boxes; "det" [B, k, 6+nm] = (x1, y1, x2, y2, score, class,
 *     mc[0..nm)) = ys_e2e_topk_ex(pred, extra = nm); ys_model_det_device returns its pointer and k (row length 6 + nm). */
YS_API int ys_model_e2e_init(ys_model* m, int max_det, int epochs);
YS_API int ys_model_e2e_update(ys_model* m);
YS_API int ys_model_e2e_gains(ys_model* m, float* o2m, float* o2o);
/* ---- End2End for OBB models (Models/Obber.cs:18-24; Obb.one2one_init, Modules/Head.cs:454-469; E2EOBBLoss, Utils/Loss.cs:1120-1177).
 * One2one_Init for YS_OBB models of both families and every dtype.  max_det 0 = 300; epochs 0 = 100.  Every other task, a block handle or a head handle
 * returns YS_ERR_UNSUPPORTED, a second call YS_ERR_STATE; ys_model_one2one_init and ys_model_e2e_init keep refusing OBB models.  cv2, cv3 and cv4
 * are aliased (no Proto), so NO tensor is added and `.bin` files move freely between plain and End2End OBB models.  From then on:
 *   training forward: "one2one_boxes" / "one2one_scores" / "one2one_angle" are the one2many values; the BatchNorm units of cv2 / cv3 / cv4 move
 *     their running statistics twice per forward (num_batches_tracked += 2), the trunk once.
 *   ys_loss_obb = E2EOBBLoss: v8OBBLoss(tal_topk 10) on one2many and v8OBBLoss(tal_topk 7, tal_topk2 1) on one2one (the rotated assigner followed by
 *     ys_tal_keep_best's stage), combined as o2m * L_one2many + o2o * L_one2one; ys_loss_read_items returns the weighted 4 items (box, cls, dfl,
 *     angle), *loss_sum their sum * B.  It also runs after an eval forward (the Val loss, Obber.cs:94-95).  "dboxes" / "dscores" / "dangle" are the
 *     one2many gradients (x o2m), "one2one_dboxes" / "one2one_dscores" / "one2one_dangle" the one2one ones (x o2o; angle: with respect to the logit).
 *   gains: 0.8 / 0.2 at creation; ys_model_e2e_update = E2EOBBLoss.update() (the chain given above), ys_model_e2e_gains reads them.  This is the
 *     one criterion whose schedule the reference's loop steps (YoloBaseTaskModel.cs:350-353): once after every epoch.
 *   backward (all forms): towers receive o2m * g_one2many + o2o * g_one2one; the feature maps and everything below o2m * g_one2many.
 *   eval forward: Obb.decode_bboxes ignores end2end (Head.cs:434-437), so "pred" [B, 4+nc+1, A] stays (xywh of dist2rbox * stride, probabilities,
 *     angle), bit for bit a plain OBB model's; "det" [B, k, 7] = (cx, cy, w, h, score, class, angle) = ys_e2e_topk_ex(pred, extra = 1)
 *     (Obb.postprocess, Head.cs:439-452), k = min(max_det, A); ys_model_det_device returns its pointer and k.
 *   YS_FP8 models are accepted like fp8 Segment / Detect models by ys_model_e2e_init (the criterion and the one2one pass are dtype-agnostic). */
YS_API int ys_model_e2e_obb_init(ys_model* m, int max_det, int epochs);
/* ---- End2End for Pose models (Models/PoseDetector.cs:21-36; Pose.one2one_init, Modules/Head.cs:565-580; E2EPoseLoss, Utils/Loss.cs:1238-1295).
 * One2one_Init for YS_POSE models of both families and every dtype.  max_det 0 = 300; epochs 0 = 100.  Every other task, a block handle or a head handle
 * returns YS_ERR_UNSUPPORTED, a second call YS_ERR_STATE; the three entries above keep refusing Pose models.  cv2, cv3 and cv4 are aliased (no Proto),
 * so NO tensor is added and `.bin` files move freely between plain and End2End Pose models.  From then on:
 *   training forward: "one2one_boxes" / "one2one_scores" / "one2one_kpts" are the one2many values; the BatchNorm units of cv2 / cv3 / cv4 move their
 *     running statistics twice per forward (num_batches_tracked += 2), the trunk once.
 *   ys_loss_pose = E2EPoseLoss: v8PoseLoss(tal_topk 10) on one2many and v8PoseLoss(tal_topk 7, tal_topk2 1) on one2one (the assigner followed by
 *     ys_tal_keep_best's stage; the one2many criterion is built with tal_topk2 = tal_topk and runs no second stage, Tal.cs:242), combined as
 *     o2m * L_one2many + o2o * L_one2one; ys_loss_read_items returns the weighted 5 items (box, pose, kobj, cls, dfl), *loss_sum their sum * B.  It also
 *     runs after an eval forward (the Val loss, PoseDetector.cs:123-124).  "dboxes" / "dscores" / "dkpts" are the one2many gradients (x o2m),
 *     "one2one_dboxes" / "one2one_dscores" / "one2one_dkpts" the one2one ones (x o2o).  ys_loss_detect alone stays refused.
 *   gains: 0.8 / 0.2 at creation; ys_model_e2e_update = E2EPoseLoss.update(), ys_model_e2e_gains reads them.  The reference's loop steps the schedule only
 *     `if (loss is Loss.E2EOBBLoss)` (YoloBaseTaskModel.cs:350-353) and E2EPoseLoss is a class of its own, so a Pose run of the reference keeps 0.8 / 0.2:
 *     leave ys_model_e2e_update out to reproduce it.
 *   backward (all forms): towers receive o2m * g_one2many + o2o * g_one2one; the feature maps and everything below o2m * g_one2many.  The zero rows of
 *     the padded keypoint towers keep zero gradients and parameters.
 *   eval forward: "pred" [B, 4+nc+nk, A] carries xyxy boxes (Detect.decode_bboxes under end2end, Head.cs:201) and the decoded keypoints; "det"
 *     [B, k, 6+nk] = (x1, y1, x2, y2, score, class, the nk keypoint values of the selected anchor) = ys_e2e_topk_ex(pred, extra = nk) (Pose.postprocess,
 *     Head.cs:550-563), k = min(max_det, A); ys_model_det_device returns its pointer and k. */
YS_API int ys_model_e2e_pose_init(ys_model* m, int max_det, int epochs);
/* Detect.postprocess / get_topk_index with agnostic_nms = false (Head.cs:117-127, 175-196) over pred [B, 4+nc, A] fp32 (boxes in any
 * format, class scores): k = min(max_det, A); stage 1 = the k anchors with the largest max-over-classes score; stage 2 = the k largest of the
 * k * nc gathered scores, flattened [stage-1 rank][class]; out_rows [B, k, 6] = (box[0..3], score, class), out_anchor [B, k] = the anchor
 * index, ordered by score descending.  TIES: ATen leaves the order among equal values unspecified; here the lower index comes first -- the
 * anchor index in stage 1, the flattened [stage-1 rank][class] index in stage 2.  +0 = -0; NaN counts as the largest value.  The result is
 * a pure function of the input (no floating-point atomics).  Any A, nc, max_det >= 1 with k * nc < 2^30.  `on_device` applies to all pointers. */
YS_API int ys_e2e_topk(ys_ctx* ctx, const float* pred, int on_device, int batch, int nc, int anchors, int max_det,
                       float* out_rows, int64_t* out_anchor);
/* Ops.non_max_suppression(end2end: true) (Utils/Ops.cs:258-267): rows [B, k, 6] ordered by score (ys_e2e_topk) -> out_count[b] = the number
 * of leading rows with score > conf_thres, at most max_det; the rows are not moved (the kept set is a prefix).  conf_thres outside [0,1] ->
 * YS_ERR_INVALID_ARG (ArgumentException in the reference).  `on_device` applies to rows and out_count. */
YS_API int ys_e2e_select(ys_ctx* ctx, const float* rows, int on_device, int batch, int k, float conf_thres, int max_det, int32_t* out_count);
/* ys_e2e_topk over pred [B, 4+nc+extra, A] (Segment.postprocess, Head.cs:321-339): the same two-stage selection and tie rule on the nc class
 * scores; out_rows [B, k, 6+extra] additionally carries the `extra` trailing channels pred[b, 4+nc+j, anchor] of the selected anchor (the mask
 * coefficients).  extra = 0 is ys_e2e_topk, bit for bit.  ys_e2e_select_ex: ys_e2e_select on rows of row_len >= 6 floats. */
YS_API int ys_e2e_topk_ex(ys_ctx* ctx, const float* pred, int on_device, int batch, int nc, int extra, int anchors, int max_det,
                          float* out_rows, int64_t* out_anchor);
YS_API int ys_e2e_select_ex(ys_ctx* ctx, const float* rows, int on_device, int batch, int k, int row_len, float conf_thres, int max_det,
                            int32_t* out_count);
/* The assigner's second stage, tal_topk2 = 1 (Utils/Tal.cs:242-250), on its own -- the kernel the End2End Segment and OBB criteria run.  align
 * [B, G, A] fp32, mask_pos [B, G, A] uint8 (in / out), gt_count [B] in [0, G]: in every row g < gt_count[b] only the anchor that comes first in
 * (align * mask_pos descending, anchor index ascending) order over ALL A anchors keeps its mask bit.  So among equal positives the lower index
 * stays, and a row whose positives all carry align = 0 ties with every other anchor: it keeps anchor 0 if that is a positive of the row and ends
 * empty otherwise (what a stable descending sort of the reference's expression gives).  Rows >= gt_count[b] are untouched.  No atomics. */
YS_API int ys_tal_keep_best(ys_ctx* ctx, const float* align, uint8_t* mask_pos, const int32_t* gt_count, int on_device, int batch, int boxes,
                            int anchors);

/* v8SegmentationLoss.forward (Utils/Loss.cs:688-863) for task = YS_SEGMENT models: the detection terms and
 * assignment above, then calculate_segmentation_loss / single_mask_loss (:794-863) with Ops.crop_mask
 * (Utils/Ops.cs:409-449) and the gradients w.r.t. "mask_coefficient" and "proto".
 * masks: fp32 [B, H/4, W/4] overlap-encoded instance ids (0 = background, k = the image's k-th label, 1-based;
 * Data/YoloDataset.cs:265-267, overlap_mask = true).  crop_mode 0 = crop_mask's broadcast form (:437-447, the
 * branch an accelerator run takes); 1 = its CPU "n < 50" integer-truncation branch (:421-435). */
YS_API int ys_loss_segment(ys_model* m, const float* batch_idx, const float* cls, const float* bboxes,
                           int n_labels, const float* masks, int on_device, int crop_mode);
/* v8OBBLoss.forward (Utils/Loss.cs:486-684) + RotatedTaskAlignedAssigner (Utils/Tal.cs:260-310) + RotatedBboxLoss
 * (Loss.cs:190-228) for task = YS_OBB models.  bboxes: fp32 [n_labels, 5] = normalised cx, cy, w, h + angle (radians).
 * Labels thinner than 2 pixels are dropped (Loss.cs:563).  Items (box, cls, dfl, angle) via ys_loss_read_items(n_items = 4).
 * The angle head output is kept as the LOGIT: ys_model_get_output("angle") applies (sigmoid - 0.25) * pi (Head.cs:429),
 * "dangle" is the gradient w.r.t. the logit, and ys_model_set_preds takes angle logits [B,1,A] in its mask_coefficient argument. */
YS_API int ys_loss_obb(ys_model* m, const float* batch_idx, const float* cls, const float* bboxes,
                       int n_labels, int on_device);
/* v8PoseLoss.forward (Utils/Loss.cs:870-1071, KeypointLoss :169-188) for task = YS_POSE models: the detection terms and
 * assignment of ys_loss_detect, then the keypoint location (OKS-style, hyp_pose 12) and visibility (BCE, hyp_kobj 1) terms and
 * d(sum(loss*B))/d(raw kpts).  keypoints: fp32 [n_labels, kpt_num, kpt_dim] normalised like bboxes (x, y[, visibility]), row i
 * belongs to label i (YoloDataset keypoints, batch["keypoints"]).  Labels must be grouped by image in collate order (batch_idx
 * non-decreasing), as YoloDataset's collate produces them: the reference's _select_target_keypoints (Loss.cs:1040-1071) indexes
 * the keypoint rows by each label's rank within its image and is only defined for that order; host labels are validated
 * (YS_ERR_INVALID_ARG otherwise), device labels are the caller's responsibility.  A Pose model's ys_model_set_preds takes its raw kpts
 * [B, nk, A] in the mask_coefficient argument; ys_model_get_output("dkpts") returns the gradient. */
YS_API int ys_loss_pose(ys_model* m, const float* batch_idx, const float* cls, const float* bboxes,
                        int n_labels, const float* keypoints, int on_device);
/* v8ClassificationLoss.forward (Utils/Loss.cs:1073-1091) for task = YS_CLASSIFY models: cross_entropy(preds["cls"], batch["cls"].view(-1))
 * with mean reduction -- NOT multiplied by the batch size, unlike the detection losses -- and d(loss)/d(logits) = (softmax - onehot) / B.
 * cls: fp32 class ids [batch]; batch must equal the last forward's.  Works after a training forward (the step) and after an eval forward
 * (Classifier.Val's loss, Models/Classifier.cs:90-93).  A host label outside [0, nc) (or not integral) is refused at once with
 * YS_ERR_INVALID_ARG; device labels are checked on the device and the refusal comes from ys_loss_read_items.  Other tasks: refused. */
YS_API int ys_loss_classify(ys_model* m, const float* cls, int batch, int on_device);
/* Loss items in the criterion's own order: detect n_items = 3 (box, cls, dfl; Loss.cs:414); classify n_items = 1 (Loss.cs:1088);
 * segment n_items = 5 (box, seg, cls, dfl, semseg = 0; Loss.cs:719); pose n_items = 5 (box, pose, kobj, cls, dfl; Loss.cs:923);
 * obb n_items = 4 (box, cls, dfl, angle; Loss.cs:546).
 * *loss_sum = sum(items)*B (classify: the mean loss itself, the scalar the reference calls backward() on). */
YS_API int ys_loss_read_items(ys_model* m, float* loss_items, int n_items, float* loss_sum);
/* The assignment behind the last criterion call, for tests that hold it against a reference assigner: target_gt_idx [B*A] = the label slot within the
 * anchor's image (labels in order of appearance), -1 = background; target_score [B*A] = the anchor's normalised target score (target_scores.sum(-1),
 * Loss.cs:138); *tss = target_scores_sum = max(sum, 1) (Loss.cs:444).  On an End2End model: of the one2one pass, which ran last over the shared
 * workspaces.  Synchronising, read-only; any output may be NULL.  Refused before a criterion has run and on classify models. */
YS_API int ys_loss_read_targets(ys_model* m, int32_t* target_gt_idx, float* target_score, float* tss);

/* autograd backward of sum(loss*B) through the whole graph (Amp.cs:348,370). Gradients accumulate
 * into the flat fp32 gradient buffer like torch's .grad (call ys_model_zero_grad between steps). */
YS_API int ys_model_backward(ys_model* m);
/* Backward in `nseg` consecutive segments (0 = head ... nseg-1 = stem) so the host can launch the
 * RCCL all-reduce of a finished gradient bucket while later segments still run. */
YS_API int ys_model_backward_segments(ys_model* m);
YS_API int ys_model_backward_segment(ys_model* m, int seg);
/* The same segment WITHOUT ordering the context stream behind the weight-gradient stream when it ends (ys_model_backward_segment
 * waits there, which stalls the next segment's kernels for the weight gradients still queued -- measured 1.1 ms of an 11.4 ms
 * data-parallel step on one MI355X).  The segment's gradients are complete once ys_model_segment_fence's events have fired:
 * ys_model_segment_fence(m, seg, stream) makes `stream` (a hipStream_t, e.g. the stream the all-reduce is issued on) wait for them.
 * ys_optim_adamw_step, ys_model_zero_grad, ys_model_get_grad and the next forward order the context stream behind the
 * weight-gradient stream themselves.  No reference counterpart (single-device autograd, Amp.cs:348). */
YS_API int ys_model_backward_segment_async(ys_model* m, int seg);
YS_API int ys_model_segment_fence(ys_model* m, int seg, void* stream);
/* [offset,count) (in floats) of the flat gradient buffer completed by segment `seg`. */
YS_API int ys_model_segment_grad_range(ys_model* m, int seg, int64_t* offset, int64_t* count);
YS_API int ys_model_zero_grad(ys_model* m);
/* Weight-gradient kernels of a backward pass run on a second stream, concurrently with the BatchNorm-backward / input-gradient chain
 * of the following layers (default on; results are identical either way -- every reduction has a fixed order).  on = 0 runs
 * everything on the context stream (per-kernel profiling: co-running kernels time-slice the CUs and inflate each other's durations).
 * No reference counterpart (TorchSharp's autograd engine schedules its own streams). */
YS_API int ys_model_set_overlap(ys_model* m, int on);
/* flat fp32 device buffers (all parameters / all gradients, same order) for collectives. */
YS_API int ys_model_grad_buffer(ys_model* m, float** dptr, int64_t* count);
YS_API int ys_model_param_buffer(ys_model* m, float** dptr, int64_t* count);

/* ---- data-parallel exchange (the reference has no multi-GPU path of its own) ------------------------------
 * One process (and one ys_ctx) per GPU; gradients of a step are SUM-all-reduced over RCCL / xGMI before AdamW.
 * ys_dist_unique_id: rank 0 creates the 128-byte RCCL id and ships it to the other ranks by any host channel.
 * ys_dist_init: joins the communicator (collective) and runs one 4-byte all-reduce so that RCCL's lazily created streams exist when
 * it returns.  CALL IT BEFORE ys_model_create: hardware queues are handed out in stream-creation order, and a communicator built after
 * the model can push the engine's main and weight-gradient streams onto one queue (no overlap; 11.6 vs 10.3 ms/step measured).
 * ys_dist_allreduce_grads(m, seg): asynchronous SUM all-reduce of a
 * backward segment's gradient range (seg < 0: the whole buffer) on a communication stream ordered after the engine stream.
 * ys_dist_wait: the engine stream waits for the outstanding all-reduces.  ys_model_backward_allreduce = the four backward
 * segments with each finished segment's all-reduce overlapped with the next (the loop bench.py runs through torch.distributed).
 * RCCL is dlopen'ed on first use; single-GPU processes never load it. */
/* Tuning / routing options (process-wide; the kernel plans read them at every launch).  Keys are the historical environment names without the YS_ prefix
 * (e.g. "GEMM_MIN_M", "GEMM_HALO", "BNRED"); at library load every YS_<KEY>=<number> environment variable seeds the table, after that only these calls
 * change it.  Production hosts never need them: the defaults are the measured optimum; the test-suite lowers size gates so that oracle-sized shapes reach
 * the wide-layer kernels (tests/conftest.py), the A/B scripts under tools/ flip one switch per run. */
YS_API int ys_set_option(const char* key, double value);
YS_API int ys_unset_option(const char* key);
/* the table's entry for `key` (set by ys_set_option or seeded from the environment at load): *is_set = 0 and *value = 0 when the built-in default applies.
 * Lets a caller change an option temporarily and put back exactly what was there (Engine.options in the Python host). */
YS_API int ys_get_option(const char* key, double* value, int* is_set);

YS_API int ys_dist_unique_id(void* id128);
YS_API int ys_dist_init(ys_ctx* ctx, int rank, int world, const void* id128);
YS_API int ys_dist_destroy(ys_ctx* ctx);
YS_API int ys_dist_allreduce_grads(ys_model* m, int segment);
YS_API int ys_dist_wait(ys_model* m);
YS_API int ys_model_backward_allreduce(ys_model* m);

/* torch.optim.AdamW.step (built YoloBaseTaskModel.cs:144-153, stepped Amp.cs:355-356,371-372):
 * decoupled weight decay, bias-corrected.  Parameter groups follow the reference's name rule:
 * group 0 = names containing "bias", 1 = "weight" (non-BN), 2 = "bn" weights.  lr comes from the host
 * (warm-up / LambdaLR stay in C#, YoloBaseTaskModel.cs:306-319). */
YS_API int ys_optim_adamw_step(ys_model* m, const float* lr_per_group, int ngroups,
                               float beta1, float beta2, float eps, float weight_decay);
/* Parameter-group construction.  mode 0 (default): the name rule above made DISJOINT.  mode 1: the reference's three groups exactly
 * as written (YoloBaseTaskModel.cs:144-151: Contains("bias") | Contains("weight") | Contains("bn")), in which every BatchNorm
 * weight / bias is listed twice: TorchSharp keys optimizer state by parameter, so such a parameter receives two consecutive AdamW
 * updates per step() from one shared state -- first with its first group's learning rate, then with the bn group's, its step
 * counter advancing by two.  Choose before the first optimizer step. */
YS_API int ys_optim_set_param_groups(ys_model* m, int mode);

/* Ops.non_max_suppression (Utils/Ops.cs:239-371) incl. torchvision.ops.nms (:357).
 * pred: [B, C=4+nc+extra, A] fp32 xywh + class probabilities; boxes are converted to xyxy IN PLACE
 * like the reference (:288-291).  out_rows [B,max_det,6+extra] = (x1,y1,x2,y2,conf,cls,extra...),
 * out_keep [B,max_det] = original anchor index, out_count [B].  `on_device` applies to all four
 * pointers.  conf/iou outside [0,1] -> YS_ERR_INVALID_ARG (ArgumentException in the reference). */
YS_API int ys_nms_batched(ys_ctx* ctx, float* pred, int on_device, int batch, int channels, int anchors,
                          float conf_thres, float iou_thres, int max_det, int nc, int max_nms, int max_wh,
                          float* out_rows, int64_t* out_keep, int32_t* out_count);

/* Ops.non_max_suppression(rotated: true) (Utils/Ops.cs:286,349-353): oriented boxes.  pred [B, 4+nc+extra, A] with the angle
 * (radians) as the LAST channel; boxes stay xywh (no in-place conversion); candidates are ordered by score and candidate j is
 * dropped iff any earlier candidate i has Metrics.batch_probiou(i, j) >= iou_thres (Ops.nms_rotated, :373-401 -- not the greedy
 * rule of ys_nms_batched).  Outputs as ys_nms_batched with rows (x, y, w, h, conf, cls, extra..., angle). */
YS_API int ys_nms_rotated_batched(ys_ctx* ctx, float* pred, int on_device, int batch, int channels, int anchors,
                                  float conf_thres, float iou_thres, int max_det, int nc, int max_nms, int max_wh,
                                  float* out_rows, int64_t* out_keep, int32_t* out_count);

/* Metrics.probiou (Utils/Metrics.cs:137-177): probabilistic IoU of n pairs of oriented boxes xywhr [n,5] -> out [n]; ciou != 0 adds
 * the aspect-ratio term of the reference's CIoU option.  Metrics.batch_probiou (:223-258): all pairs, out [n, m].  eps: the
 * reference's 1e-7.  `on_device` applies to all pointers. */
YS_API int ys_probiou(ys_ctx* ctx, const float* obb1, const float* obb2, int on_device, int n, int ciou, float eps, float* out);
YS_API int ys_batch_probiou(ys_ctx* ctx, const float* obb1, int n, const float* obb2, int m, int on_device, float eps, float* out);

/* Validation, per-image part of Detector.Val (Models/Detector.cs:103-120), batched on the device:
 * GT boxes = bboxes[batch_idx == b] * (W,H,W,H) -> xyxy (Utils/Ops.cs:68-81); iou = Metrics.box_iou(gt, pred[:,0:4])
 * (Utils/Metrics.cs:16-34); correct = match_predictions(pred[:,5], cls, iou) (Models/YoloBaseTaskModel.cs:377-446) for the
 * IoU thresholds linspace(0.5, 0.95, 10).  rows [B,max_det,row_stride] / count [B] are ys_nms_batched outputs;
 * correct: uint8 [B, max_det, 10].  `on_device` applies to rows, count, the label arrays and correct. */
YS_API int ys_val_match_batched(ys_ctx* ctx, const float* rows, const int32_t* count, int on_device, int batch, int max_det,
                                int row_stride, const float* batch_idx, const float* cls, const float* bboxes, int n_labels,
                                float img_w, float img_h, uint8_t* correct);
/* Obber.Val (Models/Obber.cs:102-114) for a whole batch: per image b, GT = bboxes[batch_idx == b] as (cx*W, cy*H, w*W, h*H, angle),
 * predictions = rows[b, 0:count[b]] columns 0..3 + column angle_col; iou = Metrics.batch_probiou(GT, pred) (eps 1e-7);
 * correct[b] = match_predictions(rows[:, 5], cls, iou) for linspace(0.5, 0.95, 10).  rows [B, max_det, row_stride], bboxes [n, 5].
 * One launch, one workgroup per image; the same probiou function as ys_batch_probiou, so `correct` equals ys_batch_probiou +
 * ys_match_predictions per image bit for bit.  row_stride >= 7, 6 <= angle_col < row_stride.  Like ys_val_match_batched the label workspace holds
 * n_labels entries per image, so no image can exceed it. */
YS_API int ys_val_match_rotated_batched(ys_ctx* ctx, const float* rows, const int32_t* count, int on_device, int batch, int max_det,
                                        int row_stride, int angle_col, const float* batch_idx, const float* cls, const float* bboxes,
                                        int n_labels, float img_w, float img_h, uint8_t* correct);
/* PoseDetector.Val (Models/PoseDetector.cs:131-165) for a whole batch: per image b, GT boxes = xyxy of bboxes[batch_idx == b] * (W, H, W, H), GT keypoints
 * = keypoints[batch_idx == b] * (W, H, 1) (label_kpt_dim == 2: a "seen" column of ones is appended), area = w * h * 0.53; predictions = rows[b, 0:count[b]]:
 * columns 0..3 the xyxy box, 5 the class, kpt_col.. the kpt_num * kpt_dim keypoint values.  correct_box[b] = match_predictions(rows[:, 5], cls,
 * Metrics.box_iou(GT, pred)), correct_pose[b] = match_predictions(rows[:, 5], cls, Metrics.kpt_iou(GT kpts, pred kpts, OKS_SIGMA, area)) for
 * linspace(0.5, 0.95, 10).  rows [B, max_det, row_stride], bboxes [n, 4], keypoints [n, kpt_num, label_kpt_dim], both outputs [B, max_det, 10].
 * One launch, one workgroup per image; the same IoU / OKS functions as ys_box_iou / ys_kpt_iou, so both outputs equal those + ys_match_predictions
 * per image bit for bit.  kpt_num <= 64, kpt_dim and label_kpt_dim 2 or 3, 6 <= kpt_col, kpt_col + kpt_num * kpt_dim <= row_stride.  Like
 * ys_val_match_batched the label workspace holds n_labels entries per image, so no image can exceed it. */
YS_API int ys_val_match_pose_batched(ys_ctx* ctx, const float* rows, const int32_t* count, int on_device, int batch, int max_det, int row_stride,
                                     int kpt_col, int kpt_num, int kpt_dim, const float* batch_idx, const float* cls, const float* bboxes,
                                     const float* keypoints, int label_kpt_dim, int n_labels, float img_w, float img_h, uint8_t* correct_box,
                                     uint8_t* correct_pose);
/* Metrics.box_iou (Utils/Metrics.cs:16-34): iou [n, m] of xyxy boxes, fp32, eps as given (reference default 1e-7). */
YS_API int ys_box_iou(ys_ctx* ctx, const float* box1, int n, const float* box2, int m, float eps, int on_device, float* iou);

/* Metrics.mask_iou (Utils/Metrics.cs:120-125) as Segmenter.Val uses it (Models/Segmenter.cs:131-143): mask1[k] = (gt_ids == k+1),
 * k < nl, from the image's overlap-encoded instance-id map [npix] (fp32 ids, YoloDataset.cs:265-267); mask2 = pred_masks uint8
 * [n, npix] (ys_process_mask output) -> iou fp32 [nl, n].  Bit-exact: the reference's float matmul of 0/1 masks is an integer count. */
YS_API int ys_mask_iou(ys_ctx* ctx, const float* gt_ids, int nl, const uint8_t* pred_masks, int n, int npix, float eps,
                       int on_device, float* iou);
/* Metrics.kpt_iou (Utils/Metrics.cs:186-212) as PoseDetector.Val uses it (Models/PoseDetector.cs:150-158): object keypoint similarity
 * [n, m] of ground-truth keypoints kpt1 [n, K, 3] (pixels, visibility; 2-D labels get a visibility column of ones on the host,
 * PoseDetector.cs:144-148) against predicted keypoints kpt2 [m, K, kpt_dim]; area [n] = w * h * 0.53 of the labels' boxes;
 * sigmas = the COCO OKS sigmas when K == 17, else 1/K. */
YS_API int ys_kpt_iou(ys_ctx* ctx, const float* kpt1, int n, const float* kpt2, int m, const float* area, int kpt_num, int kpt_dim,
                      float eps, int on_device, float* iou);
/* match_predictions (Models/YoloBaseTaskModel.cs:377-446) on a caller-supplied IoU matrix [nl, n] (box, mask, OBB or keypoint
 * IoU alike): correct uint8 [n, 10] for the thresholds linspace(0.5, 0.95, 10). */
YS_API int ys_match_predictions(ys_ctx* ctx, const float* pred_cls, int n, const float* true_cls, int nl, const float* iou,
                                int on_device, uint8_t* correct);

/* Classifier.Val's ranking (Models/Classifier.cs:95-100: softmax scores argsort descending, first 5): idx[rows, k] int32 = the indices
 * of the k largest scores of each row of scores[rows, cols] fp32, in descending order; ties go to the lower index, NaN scores are never
 * picked (-1 fills a row with fewer than k comparable entries).  1 <= k <= min(16, cols).  `on_device` applies to scores and idx. */
YS_API int ys_cls_topk(ys_ctx* ctx, const float* scores, int on_device, int rows, int cols, int k, int32_t* idx);

/* Ops.process_mask (Utils/Ops.cs:462-489), used by Segmenter post-processing (Models/Segmenter.cs:131-160 region):
 * masks = masks_in[n,nm] @ protos[nm,mh,mw], cropped to boxes (xyxy, image pixels) scaled to the mask grid,
 * optionally bilinearly upsampled (align_corners = false) to (ih, iw), thresholded > 0.
 * out: uint8 [n, oh, ow], (oh, ow) = upsample ? (ih, iw) : (mh, mw).  `on_device` applies to all pointers. */
YS_API int ys_process_mask(ys_ctx* ctx, const float* protos, const float* masks_in, const float* boxes, int on_device,
                           int n, int nm, int mh, int mw, int ih, int iw, int upsample, int crop_mode, uint8_t* out);

/* Input side: Augment.LetterBox.LetterboxImage (Data/Augment.cs:757-778) and Augment.Rectangle.RectangleImage
 * (:836-857): ratio = min(fit_w / w, fit_h / h), new = (int)(size * ratio), torchvision resize (TorchVision.NET default: nearest) and
 * constant padding with `color` (114 for images, 0 for masks), centred on an out_w x out_h canvas.  LetterBox: fit = out;
 * Rectangle: fit = the label's resized shape, out = its rectangle shape.  Planes [C,h,w] -> [C,out_h,out_w], uint8 or fp32
 * (is_float).  *pad_l / *pad_u = the offsets the reference adds to boxes / keypoints / OBB corners. */
YS_API int ys_letterbox(ys_ctx* ctx, const void* src, int is_float, int on_device, int C, int h, int w, int fit_w, int fit_h,
                        int out_w, int out_h, int color, void* dst, int32_t* pad_l, int32_t* pad_u);

/* ---- training input on the device: the reference's default training pipeline (ImageProcessType.Mosiac,
 * Data/YoloDataset.cs:57-151) -- Augment.Mosaic._mosaic4 (Data/Augment.cs:158-274), Augment.RandomPerspective (:315-695), FlipLR / FlipUD
 * (:860-966), Normalize (Data/Struct.cs:99-121), mul(1/255) and the collate (Data/YoloDataLoader.cs:18-44) -- as one call per batch for the
 * images and one for the labels.  The random draws stay on the host: an item carries the parameters the reference draws (four source indices,
 * the mosaic centre, the forward matrix exactly as affine_transform returns it, the two flip decisions).
 * The sources live in one uint8 `arena`: source k has its RGB planes [3][h][w] at byte offset img_off and, optionally, its overlap-encoded
 * instance-id mask [mh][mw] at mask_off (-1 = none).  The library cannot see the arena's size: offsets and sizes are the caller's
 * responsibility.
 *
 * ys_augment_mosaic: images fp32 [batch, 3, imgsz, imgsz] in [0, 1]; masks (may be NULL) fp32 [batch, imgsz / mask_ratio, imgsz / mask_ratio],
 * the layout ys_loss_segment reads.  The 2s x 2s canvas of _mosaic4 is never materialised: canvas pixel (Y, X) is 114 (masks 0) or the pixel of
 * the tile whose rectangle (:184-203; masks: every bound / mask_ratio, :207-209) holds it.  The warp restates Warp{Affine,Perspective}WithGridSample:
 * src = M_inv (x, y, 1) / w; outside 0 <= src <= in - 1 the border value (114; masks 0); inside grid_sample(bilinear, border, align_corners = false)
 * at grid = src / (in - 1) * 2 - 1 -- i.e. at src * in / (in - 1) - 0.5, NOT at src -- then clamp(0, 255) and truncation to a byte; masks take the
 * same BILINEAR path on their id bytes with M_mask = S_inv M S (:371-389).  perspective != 0 selects the perspective form (all of M, divide by w;
 * the reference's `perspective > 0`), 0 the affine form (rows 0-1 of M over (0, 0, 1)).  M is inverted, the source position evaluated and the
 * four bytes blended in double (the reference: fp32), the blend as a nested interpolation that is exact on constant regions.  Flips are folded into the output coordinate; a byte b becomes
 * (float)b * (1 / 255.0f).
 *
 * ys_augment_labels: per-source label tables -- lab_off [n_src + 1] (labels of source k = [lab_off[k], lab_off[k + 1])), cls [n], boxes [n, 4]
 * pixel xyxy in the source's own frame, keypoints [n, kpt_num, 3] pixels + visibility (NULL = none) -- become the collate's rows for the same
 * items: per image, tiles in order, labels in order: + (padw, padh), clip to [0, 2s], keep if area > 0 && area > 0.7 * org_area (:238-256);
 * apply_bboxes (:546-568), clip_boxes to [0, s], keep if area > 0 (:681-692); apply_keypoints (:581-601, always divides by w) + clip_keypoints
 * (Utils/Ops.cs:166-183); the flips; cxcywh / s, keypoints x, y / s.  Rows are COMPACTED in collate order (batch_idx non-decreasing, stable within
 * an image) into arrays of `capacity` rows: out_batch_idx [capacity], out_cls [capacity], out_bboxes [capacity, 4], out_keypoints
 * [capacity, kpt_num, 3] (NULL iff keypoints is NULL); rows [*out_count, capacity) hold batch_idx -1 and zeros, which ys_loss_* skip -- a caller
 * passes n_labels = capacity with on_device = 1 and never reads *out_count on the host.
 * QUIRK kept by default: FlipLR / FlipUD set x <- s - x on columns 0 and 2 (y: 1 and 3) WITHOUT swapping them (:890-891, :945-946), so a flipped
 * box has a negative width / height after cxcywh.  flags & YS_AUG_SORT_FLIPPED writes (min, max) instead.
 *
 * on_device applies to every pointer of a call; with device pointers both calls are asynchronous on the context's stream.  With host pointers
 * (on_device = 0) the items are validated and YS_ERR_INVALID_ARG is returned for: a src outside [0, n_src), imgsz odd or < 2, xc / yc outside
 * [0, 2 * imgsz], a singular M, and a capacity below the sum of the four tiles' label counts of some image.  Device items cannot be read by the
 * host: an item that fails those checks yields an all-114 image (zero masks) and no labels; if more rows are kept than `capacity`, *out_count holds
 * the true total (> capacity) and the rows past capacity are not written.  Nothing is truncated silently.
 * Scope: kpt_dim must be 3 (apply_keypoints reads column 2; 2 -> YS_ERR_INVALID_ARG).  OBB corner labels are the *_obb entries further down.  Not built:
 * the `rand > p` case of Augment.Mosaic (the reference then
 * yields images of unequal sizes its own collate cannot stack).  RandomHSV, the last transform of both chains, is the ys_aug_jitter row of the
 * *_jitter entries further down.  The other no-mosaic case -- the LetterBox pipeline the reference trains on once the
 * mosaic is closed -- is ys_augment_letterbox / ys_augment_letterbox_labels below.  Deviations: a label-free sample is still warped (RandomPerspective.Apply returns the
 * unwarped 2s x 2s canvas, :666-669); where the reference's mask slice would run past the source mask (it throws) the kernel reads 0. */
typedef struct ys_aug_src { int64_t img_off, mask_off; int32_t h, w, mh, mw; } ys_aug_src;
typedef struct ys_aug_item { int32_t src[4]; int32_t xc, yc; float M[9]; int32_t flip_lr, flip_ud; } ys_aug_item;
#define YS_AUG_SORT_FLIPPED 1
YS_API int ys_augment_mosaic(ys_ctx* ctx, const uint8_t* arena, const ys_aug_src* srcs, int n_src, const ys_aug_item* items, int batch,
                             int on_device, int imgsz, int mask_ratio, int perspective, float* images, float* masks);
YS_API int ys_augment_labels(ys_ctx* ctx, const ys_aug_src* srcs, const int32_t* lab_off, const float* cls, const float* boxes,
                             const float* keypoints, int kpt_num, int kpt_dim, const ys_aug_item* items, int batch, int on_device,
                             int imgsz, int perspective, int flags, int capacity, float* out_batch_idx, float* out_cls, float* out_bboxes,
                             float* out_keypoints, int32_t* out_count);

/* ---- the LetterBox (close-mosaic) training input: what YoloDataset.CloseMosaic(true) builds (Data/YoloDataset.cs:378-429; the training loop calls it
 * with `epoch > Config.CloseMosaic`, Models/YoloBaseTaskModel.cs:180, so with the default 0 every epoch trains on it) and what ImageProcessType.Letterbox
 * is (:70-74): LetterBox(imgsz, imgsz, mask_ratio) (Data/Augment.cs:698-778) + FlipLR + FlipUD (:860-966) + Normalize + mul(1/255) + collate.
 * Same arena, ys_aug_src and label tables and the same ys_aug_item table as the Mosaic entries: both calls read only src[0], flip_lr and flip_ud of an
 * item and ignore the rest, so one item table serves both branches.
 *
 * ys_augment_letterbox: images fp32 [batch, 3, imgsz, imgsz]; masks (may be NULL) fp32 [batch, imgsz / mask_ratio, imgsz / mask_ratio] whole ids.
 * LetterboxImage (:756-777) in the reference's fp32 arithmetic: ratio = min(s / (float)w, s / (float)h), new_w = (int)(w * ratio), new_h likewise,
 * pad_l = (s - new_w) / 2, pad_u = (s - new_h) / 2; the resize is ys_letterbox's nearest rule src = min(floor(dst * (float)in / out), in - 1); 114
 * outside the window; the flips folded into the output coordinate; a byte b becomes (float)b * (1 / 255.0f).  The mask is letterboxed from ITS OWN
 * size [mh, mw] onto (imgsz / mask_ratio)^2 with fill 0 (:725) -- its pads are not the image's pads / mask_ratio, so mask and image can sit a fraction
 * of a cell apart (kept); a source without a mask gives a zero mask.  Nothing is blended: the output is bit-exact.
 *
 * ys_augment_letterbox_labels: EVERY label of src[0], in order (this branch has no thresholds), in the compacted layout of ys_augment_labels (tail
 * rows batch_idx -1 and zeros, *out_count = the total).  The reference carries cxcywh through this branch (bbox_format = cxcywh, YoloDataset.cs:303);
 * the tables hold pixel xyxy, converted here with cx = (x1 + x2) / 2, w = x2 - x1 (torchvision box_convert): a DEVIATION of a few fp32 roundings.
 * Then, as written in the reference: boxes + (pad_l, pad_u, 0, 0) (:735-738), keypoints + (pad_l, pad_u) (:741-744), NEITHER scaled by ratio (kept;
 * exact whenever ratio == 1, i.e. when the loader has resized the long side to imgsz), the flips, mul(1f / imgsz) (Struct.cs:106-115).
 * QUIRK kept by default: FlipLR / FlipUD test bbox_format != xywh, which is true for cxcywh, and rewrite columns 0 AND 2 (1 AND 3) as s - value
 * (:888-892, :943-947): a flipped box's width (height) becomes s - w.  flags & YS_AUG_FLIP_KEEP_SIZE leaves columns 2 / 3 alone.
 * YS_AUG_SORT_FLIPPED is ignored here; ys_augment_labels takes YS_AUG_SORT_FLIPPED only.  Keypoints: x <- s - x / y <- s - y without a left / right
 * index swap (the reference has none); visibility untouched.  kpt_dim must be 3.
 *
 * Host pointers (on_device = 0): YS_ERR_INVALID_ARG for a src[0] outside [0, n_src) or without an image, imgsz odd or < 2, and a capacity below the
 * batch's label total.  Device pointers: an item that fails those checks yields an all-114 image, a zero mask and no rows; a total above `capacity` is
 * reported in *out_count and the rows past capacity are not written. */
#define YS_AUG_FLIP_KEEP_SIZE 2
YS_API int ys_augment_letterbox(ys_ctx* ctx, const uint8_t* arena, const ys_aug_src* srcs, int n_src, const ys_aug_item* items, int batch,
                                int on_device, int imgsz, int mask_ratio, float* images, float* masks);
YS_API int ys_augment_letterbox_labels(ys_ctx* ctx, const ys_aug_src* srcs, int n_src, const int32_t* lab_off, const float* cls, const float* boxes,
                                       const float* keypoints, int kpt_num, int kpt_dim, const ys_aug_item* items, int batch, int on_device,
                                       int imgsz, int flags, int capacity, float* out_batch_idx, float* out_cls, float* out_bboxes,
                                       float* out_keypoints, int32_t* out_count);

/* ---- ColorJitter (RandomHSV): the last transform of both training chains (Data/YoloDataset.cs:86, :416; Data/Augment.cs:968-987):
 * torchvision.transforms.ColorJitter(brightness 0.4, contrast 0, saturation 0.7, hue 0.015) on the uint8 image -- after RandomPerspective the image is
 * uint8 again (:452-454, :527-529).  ClassificationDataset ends its chain with the same operator and a non-zero contrast (Data/ClassificationDataset.cs:122).
 * TorchVision.NET's source is not part of the reference tree: the contract is torchvision's public uint8 algorithm (transforms/_functional_tensor.py),
 * restated here; parity with TorchVision.NET is UNPINNED.  Every op ends in a uint8 image (truncation between the ops, not once at the end); the factors
 * are fp32 (torchvision draws them as fp32 and carries them as Python doubles; 1.0 - f formed in double and rounded is 1.0f - f); every step is one
 * separately rounded fp32 operation with correctly rounded divisions, so the output is bit-exact against an fp32 restatement (tests/color_jitter_ref.py).
 *   blend(a, b, f) = trunc(clamp(f * a + (1 - f) * b, 0, 255));  gray = trunc((0.2989f r + 0.587f g) + 0.114f b)
 *   op 0 brightness: blend(c, 0, f)      op 1 contrast: blend(c, mean, f), mean = the fp32 mean of gray over the image in its state at that point
 *   op 2 saturation: blend(c, gray, f)   op 3 hue: c / 255, _rgb2hsv, h = (h + f) mod 1 (Python-style), _hsv2rgb, trunc(v * 255.999f)
 * A row holds what ColorJitter.get_params draws for one image: order[k] = the op id run in slot k (randperm(4)), or -1 for nothing (an op whose gain is 0
 * keeps its slot and is skipped); factor[id] is indexed by op id.  A row is valid if its ids are in {-1, 0..3} with no id twice, factors 0..2 are finite
 * and >= 0 and the hue factor is in [-0.5, 0.5].  The draws stay on the host like every other draw of this pipeline.
 *
 * ys_augment_mosaic_jitter / ys_augment_letterbox_jitter: the plain entries with `jitter` [batch] rows applied to the bytes in the gather kernels'
 * epilogue, in front of the mul(1 / 255): no extra pass over the images.  The 114 of the border / padding is jittered like every other pixel.
 * jitter == NULL IS the plain entry (the same kernel).  The rows follow the call's on_device.  A row that runs contrast is YS_ERR_UNSUPPORTED here (the
 * mean would need the gather twice; the reference's box tasks pass contrast 0).  Host pointers: an invalid row is YS_ERR_INVALID_ARG.  Device pointers:
 * an invalid or contrast row yields the all-114 image, not jittered, like a refused item; masks and labels do not read the rows.
 *
 * ys_color_jitter: the operator on its own, all four ops, src uint8 [batch, 3, h, w] -> dst uint8 (dst_is_float = 0) or fp32 byte * (1 / 255.0f).
 * Contrast takes two launches: a reduction replays the ops in front of it and sums gray per image with integer atomics (any order, the same sum), the
 * apply pass forms mean = (float)sum / (float)(h * w).  For h * w <= 65536 every partial sum is an exact fp32 integer and this equals torch.mean bit
 * for bit; above that torch's own fp32 summation order decides the last bit of its mean -- the one DEVIATION.  Invalid rows: YS_ERR_INVALID_ARG with
 * host pointers, the all-114 image with device pointers.  src and dst must not overlap. */
typedef struct ys_aug_jitter { int32_t order[4]; float factor[4]; } ys_aug_jitter;
YS_API int ys_augment_mosaic_jitter(ys_ctx* ctx, const uint8_t* arena, const ys_aug_src* srcs, int n_src, const ys_aug_item* items, int batch,
                                    int on_device, int imgsz, int mask_ratio, int perspective, const ys_aug_jitter* jitter, float* images,
                                    float* masks);
YS_API int ys_augment_letterbox_jitter(ys_ctx* ctx, const uint8_t* arena, const ys_aug_src* srcs, int n_src, const ys_aug_item* items, int batch,
                                       int on_device, int imgsz, int mask_ratio, const ys_aug_jitter* jitter, float* images, float* masks);
YS_API int ys_color_jitter(ys_ctx* ctx, const uint8_t* src, const ys_aug_jitter* jitter, int batch, int h, int w, int on_device, void* dst,
                           int dst_is_float);

/* ---- OBB corner labels for the training input (Data/YoloDataset.cs:110-129, 216-244; Utils/Ops.cs:44-54): an OBB label carries four corners
 * [n, 4, 2] (pixels, the source's frame) beside its axis-aligned box; the criterion's row is xyxyxyxy2xywhr of the transformed corners -- OpenCV
 * MinAreaRect, host code in the reference -- with columns 0-3 divided by imgsz, and it REPLACES the box: ys_loss_obb never sees the axis-aligned one.
 *
 * ys_xyxyxyxy2xywhr: the operator on its own.  corners [n, 4, 2] -> out [n, 5] = (cx, cy, w, h) in the corners' units and the angle in radians; no
 * division by imgsz; n = 0 is a no-op.  CONTRACT: the enclosing rectangle of minimum area, in OpenCV >= 4.5.1's documented canonical form (the
 * reference pins OpenCvSharp 4.11): angle in (0, pi/2], w = the side whose direction makes `angle` with the +x axis, h = the other side.  An
 * axis-aligned rectangle is therefore angle = pi/2 with (w, h) = (y extent, x extent), never angle = 0; a rectangle has exactly one such row.
 * How: the minimum-area rectangle has a side along a hull edge and every hull edge is one of the 6 point pairs, so the minimum of the bounding
 * rectangles along the 6 pair directions -- order (0,1) (1,2) (2,3) (3,0) (0,2) (1,3), zero-length pairs skipped, the FIRST strict minimum wins -- is
 * the answer, and a pure function of the input.  fp32 in and out; the differences, projections, areas and atan2 in between are double.
 * Degenerate inputs give finite rows: four identical points (x, y, 0, 0, 0); exactly collinear points w = the span, h = 0 and the line's OWN
 * direction folded by half turns into (0, pi] -- the one kind of row whose angle can exceed pi/2 (a line in the second quadrant; a horizontal one is
 * pi): with w as the span a quarter-turn fold would describe the segment turned by 90 degrees.  DEVIATION: OpenCV leaves the raw atan2 of the line,
 * in (-pi, pi], there.  These rows are reachable: the Mosaic keep decision is made on the box of
 * the transformed axis-aligned box, which can overlap the image while all four clipped corners lie on one border.
 * UNPINNED: OpenCV is not available to this project's tests, so the choice among geometrically DIFFERENT rectangles of equal area -- an acute
 * triangle (one corner repeated): all three edges tie exactly; many quads clipped to the image -- is the pair order above, not pinned against the
 * reference binary.  It matters: of 20 000 random boxes of 2-16 px on a 64 px image about 2 % of the kept labels had a geometrically different
 * rectangle within 1e-4 of the minimum area, with large, heavily clipped boxes about 16 % (float64 brute force on the CPU).
 *
 * ys_augment_labels_obb = ys_augment_labels with corners [n, 4, 2] in place of the keypoint arguments and out_bboxes [capacity, 5] in place of the box
 * and keypoint outputs: same two-pass count / scan / write, compaction order, tail rows (batch_idx -1, zeros), *out_count, capacity rule and
 * host-pointer validation.  `boxes` [n, 4] stays an input: it ALONE decides which rows are kept, exactly as in ys_augment_labels (quirk kept: the
 * reference filters on the axis-aligned box, :245 and :683-684).  A kept row, fp32 in the reference's order: corners + (padw, padh), NOT clipped to
 * the canvas (:253-256); (x, y, 1) . M^T, divided by the third component only when perspective != 0 (apply_obb_corners, :604-635; apply_keypoints
 * always divides); clamp to [0, imgsz] (clip_obb_corners, Utils/Ops.cs:191-199); FlipLR x <- s - x, FlipUD y <- s - y; the rectangle; columns 0-3
 * / (float)imgsz (a division, YoloDataset.cs:121).  flags must be 0 (YS_ERR_INVALID_ARG otherwise): the box-flip switches have nothing to act on.
 *
 * ys_augment_letterbox_labels_obb, the same relative to ys_augment_letterbox_labels: every label kept, corners + (pad_l, pad_u) NOT scaled by ratio
 * (the quirk that branch keeps for boxes, :746-749), NOTHING clipped (a corner outside [0, imgsz] stays there), the flips (:825-828), the rectangle,
 * the division. */
YS_API int ys_xyxyxyxy2xywhr(ys_ctx* ctx, const float* corners, int n, int on_device, float* out);
YS_API int ys_augment_labels_obb(ys_ctx* ctx, const ys_aug_src* srcs, const int32_t* lab_off, const float* cls, const float* boxes,
                                 const float* corners, const ys_aug_item* items, int batch, int on_device, int imgsz, int perspective, int flags,
                                 int capacity, float* out_batch_idx, float* out_cls, float* out_bboxes, int32_t* out_count);
YS_API int ys_augment_letterbox_labels_obb(ys_ctx* ctx, const ys_aug_src* srcs, int n_src, const int32_t* lab_off, const float* cls, const float* boxes,
                                           const float* corners, const ys_aug_item* items, int batch, int on_device, int imgsz, int flags, int capacity,
                                           float* out_batch_idx, float* out_cls, float* out_bboxes, int32_t* out_count);

/* ---- The classification input (Data/ClassificationDataset.cs:90-131, GetTensor :70-88) with Auto_Augment = None, as one fused gather per batch:
 *   train  RandomResizedCrop(imgsz, scale, ratio) (:95) -> RandomHorizontalFlip (:98) -> RandomVerticalFlip (:102) -> RandomErasing (:120; the
 *          reference's own class, :166-226) -> ColorJitter(brightness = vgain, contrast = vgain, saturation = sgain, hue = hgain) (:122) -> mul(1 / 255.0f) (:79)
 *   val    Resize(imgsz) (:126) -> CenterCrop(imgsz) (:127) -> mul(1 / 255.0f)
 *   label  the source's class id, one per image (:80-83)
 * Same arena and ys_aug_src table as the other augment entries (the mask fields are ignored); src_cls [n_src] fp32 class ids; items / jitter [batch];
 * images fp32 [batch, 3, imgsz, imgsz]; out_cls fp32 [batch] = src_cls[items[b].src], what ys_loss_classify(..., on_device = 1) reads.  All tables
 * follow on_device.  imgsz in [1, 16384] (odd sizes take scalar stores).  No cropped, resized or uint8 intermediate image exists.
 *
 * An item is the DRAWN geometry, general enough for both chains.  With y' = flip_ud ? imgsz - 1 - y : y and x' likewise,
 *   out[y][x] = src[top + min(floor((y' + oy) * ((float)ch / (float)oh)), ch - 1)][left + min(floor((x' + ox) * ((float)cw / (float)ow)), cw - 1)]
 * -- the nearest rule of ys_letterbox / ys_augment_letterbox (ATen legacy nearest, fp32) on the crop window (top, left, ch, cw) of the source, resized
 * to (oh, ow), of which the imgsz x imgsz window at (oy, ox) is taken.  Train: oh = ow = imgsz, oy = ox = 0.  Val: top = left = 0, (ch, cw) = (H, W),
 * (oh, ow) the resized size, (oy, ox) the centre-crop offset.
 * Erase: in the output frame, after the flips and in front of the jitter, a pixel of [er_y, er_y + er_h) x [er_x, er_x + er_w) takes one noise byte
 * per channel in place of the gathered one.  The reference writes torch.empty(c, h, w).normal_() into the uint8 image; ATen's CPU cast truncates
 * toward zero and wraps mod 256.  The byte has exactly the distribution of (uint8)(int64)z, z ~ N(0, 1): value k = 0 covers (-1, 1), k > 0 [k, k + 1),
 * k < 0 (k - 1, k]; thresholds round(2^32 * cumulative probability) for k = -6 .. 6 on one 32-bit word (DEVIATION: the tails beyond +-7, mass 2.6e-12,
 * fold into +-6).  The word is counter-based, independent of the launch shape (uint32 arithmetic, c = channel, (y, x) = output pixel):
 *   u = mix32(mix32(er_seed ^ (c * 0x9e3779b9u)) + (y * imgsz + x));   mix32(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16
 * The reference's torch RNG stream cannot be matched; every draw of this pipeline is the host's.
 * Jitter: the bytes go through the image's ys_aug_jitter row (the arithmetic of ys_color_jitter), ALL four ops: contrast's mean is taken over the
 * imgsz x imgsz output in its state in front of the contrast op, by a reduction launch that replays gather, erase and the ops ahead of it (integer
 * atomics; mean = (float)sum / (float)(imgsz * imgsz): torch.mean's value bit for bit for imgsz * imgsz <= 65536, 224 included; above that the
 * DEVIATION of ys_color_jitter carries over).  A host-pointer batch without a contrast row, and jitter == NULL (no jitter: the val chain), take one
 * launch; with device pointers the reduction runs and leaves at once where a row has no contrast.
 * An item is valid when 0 <= src < n_src and the source has an image; ch, cw >= 1, top, left >= 0, top + ch <= H, left + cw <= W; oh, ow >= 1,
 * oy, ox >= 0, oy + imgsz <= oh, ox + imgsz <= ow; the flips are 0 or 1; the erase rectangle is all zero (none) or er_h, er_w >= 1 inside
 * [0, imgsz)^2.  Host pointers: the first invalid item or jitter row is YS_ERR_INVALID_ARG.  Device pointers: that image is all 114 * (1 / 255.0f),
 * not jittered, and out_cls[b] = -1; the other images of the batch are unaffected.
 * QUIRKS of the reference a host reproduces in its draws (yolosharp_amd/augment.py draw_classify_items): RandomErasing's gate is a NORMAL draw,
 * `randn > p` skips (:218): at p = 0.4 an image is erased with probability 0.655; its accept test is strict (h < H and w < W, :201); ten failed tries
 * erase the image with itself (nothing).  Not built: Auto_Augment (AutoAugment -- the reference's default -- RandAugment, AugMix).
 * UNPINNED (TorchVision.NET's source is not in the reference tree): the interpolation of RandomResizedCrop / Resize (nearest here, as for
 * functional.resize elsewhere in this project); whether Resize(int) is smaller-edge or square; CenterCrop's rounding; the accept condition of the
 * crop tries.  The item is general: a host that knows better fills it differently, the kernel does not change. */
typedef struct ys_cls_item { int32_t src, top, left, ch, cw, oh, ow, oy, ox, flip_lr, flip_ud, er_y, er_x, er_h, er_w; uint32_t er_seed; } ys_cls_item;   /* 64 bytes */
YS_API int ys_augment_classify(ys_ctx* ctx, const uint8_t* arena, const ys_aug_src* srcs, int n_src, const float* src_cls,
                               const ys_cls_item* items, int batch, int on_device, int imgsz, const ys_aug_jitter* jitter,
                               float* images, float* out_cls);

/* ---- AutoAugment / RandAugment for the classification input (Data/ClassificationDataset.cs:105-116: with Config.Auto_Augment = AutoAugment, the reference's
 * default (Data/Config.cs:228), or RandAugment the transform stands between the flips and RandomErasing).  The operators are torchvision's tensor / uint8
 * path with nearest interpolation and fill = None (out-of-image is 0).  An image brings one ys_aa_row: two slots, run in order, each an op id, its argument
 * and -- for the affine ops -- torchvision's INVERSE matrix theta, which the host builds in float64 with _get_inverse_affine_matrix(center, angle, translate,
 * scale = 1, shear) and rounds to fp32: Rotate center [0, 0], angle = -magnitude; ShearX center [-w/2, -h/2], shear [degrees(atan(m)), 0]; ShearY likewise
 * with the second component; TranslateX / Y translate [int(m), 0] / [0, int(m)], center [0, 0].  Op ids, torchvision's _augmentation_space order:
 *   -1 none (the slot's probability draw failed, RandAugment's Identity)   0 ShearX  1 ShearY  2 TranslateX  3 TranslateY  4 Rotate   (theta)
 *    5 Brightness  6 Color (saturation)  7 Contrast  8 Sharpness   (arg = 1 + m)      9 Posterize (arg = bits)  10 Solarize (arg = threshold)
 *   11 AutoContrast  12 Equalize  13 Invert
 * Arithmetic, every fp32 operation rounded on its own, divisions correctly rounded (w, h = the image's width and height as fp32):
 *   affine   r[0..2] = theta[0..2] / (0.5f * w), r[3..5] = theta[3..5] / (0.5f * h); bx = (float)x + (-w * 0.5f + 0.5f), by = (float)y + (-h * 0.5f + 0.5f);
 *            gx = (bx * r0 + by * r1) + r2, gy = (bx * r3 + by * r4) + r5; ux = ((gx + 1) * w - 1) / 2, uy likewise; ix = nearbyint(ux), iy = nearbyint(uy)
 *            (half to even); out[y][x] = in[iy][ix] inside the image, 0 outside
 *   blends   blend(a, b, f) of ys_color_jitter with b = 0 (Brightness), the pixel's gray (Color), the fp32 mean of gray over the image in its state in
 *            front of THIS op (Contrast; the DEVIATION of ys_color_jitter above 65536 pixels carries over), or the 3 x 3 filter [[1,1,1],[1,5,1],[1,1,1]] / 13
 *            rounded to nearest on the interior and the input itself on the border row and column (Sharpness; h <= 2 or w <= 2: the image is unchanged).
 *            The filter's sum S is an integer and S / 13 is never within 1 / 26 of a half, so the byte is (S + 6) / 13 in integers for any summation order.
 *   Posterize v & -(1 << (8 - bits)), bits = (int)arg in 0 .. 8;   Solarize (float)v >= arg ? 255 - v : v;   Invert 255 - v
 *   AutoContrast  per channel: scale = (1.0f / (max - min)) * 255.0f (torchvision writes bound / (max - min) with a Python number on top, which torch
 *                 evaluates as reciprocal() * bound: two roundings, e.g. max - min = 179 gives 1.42458093 where one division gives 1.42458105),
 *                 (min, scale) = (0, 1) where max == min; trunc(clamp(((float)v - min) * scale, 0, 255))
 *   Equalize      per channel, in integers: step = (N - hist[last non-empty bin]) / 255 (floor); step == 0 leaves the channel unchanged; else lut[0] = 0,
 *                 lut[v] = min((cumsum_inclusive[v - 1] + step / 2) / step, 255)
 * A row is invalid when an op id is outside -1 .. 13, Posterize's bits are outside 0 .. 8, or an arg or theta entry (of either slot, used or not) is not finite.
 *
 * ys_auto_augment_ops: the two slots on their own, in uint8 [B, 3, H, W] -> out uint8, any H, W in 1 .. 16384, in and out not overlapping.  A slot is a
 * statistics launch (histograms in LDS and gray sums, flushed with integer atomics into zeroed per-image rows: deterministic; images whose slot needs none
 * leave at once; skipped for a host-resident table no row of which needs it) and an apply launch.  Host pointers: the first invalid row is
 * YS_ERR_INVALID_ARG.  Device pointers: that image is all 114.
 *
 * ys_augment_classify_aa: ys_augment_classify with the rows `aa` [batch] (following on_device): crop -> flips -> slot 0 -> slot 1 -> erase -> jitter ->
 * mul(1 / 255.0f), every stage on the imgsz x imgsz image.  aa == NULL IS ys_augment_classify.  Otherwise crop + flips are staged as uint8
 * [batch, 3, imgsz, imgsz] in the context's workspace (a quarter of the output's bytes, and a second image to ping-pong), the slots run on them and the
 * erase + jitter launches read the staged bytes in place of the source: seven launches at most, none per image, and the host never waits.  Invalid rows:
 * YS_ERR_INVALID_ARG naming the row with host pointers; with device pointers that image is all 114 * (1 / 255.0f), class -1, its neighbours untouched.
 * UNPINNED: TorchVision.NET's source is not in the reference tree and torchvision is not available to this project's tests: the operator arithmetic
 * above, the ImageNet policy table and the magnitude spaces (yolosharp_amd/augment.py) are torchvision's public ones as this project restates them
 * (tests/aa_ref.py, written with torch's own operators); the reference's torch RNG stream cannot be matched in any case.  Not built: AugMix. */
typedef struct ys_aa_row { int32_t op[2]; float arg[2]; float theta[2][6]; } ys_aa_row;   /* 64 bytes */
YS_API int ys_augment_classify_aa(ys_ctx* ctx, const uint8_t* arena, const ys_aug_src* srcs, int n_src, const float* src_cls,
                                  const ys_cls_item* items, int batch, int on_device, int imgsz, const ys_aa_row* aa,
                                  const ys_aug_jitter* jitter, float* images, float* out_cls);
YS_API int ys_auto_augment_ops(ys_ctx* ctx, const uint8_t* in, int B, int H, int W, const ys_aa_row* rows, int on_device, uint8_t* out);

/* ---- per-operator entry points (unit parity; a TorchSharp-free C# Conv wrapper) ---------------
 * Convs.Conv.forward (Convs.cs:36-62): y = act(BN(conv2d(x))) on fp32 NCHW / OIHW HOST arrays at the
 * edge (the call stages them through HBM).  training != 0 uses batch statistics and updates running stats (momentum 0.03, eps 1e-3). */
YS_API int ys_conv_bn_act_fwd(ys_ctx* ctx, int dtype, const float* x_nchw, int B, int Cin, int H, int W,
                              const float* w_oihw, int Cout, int k, int stride,
                              const float* bn_gamma, const float* bn_beta, float* bn_mean, float* bn_var,
                              const float* bias, int act_silu, int training, float* y_nchw);

/* The same unit with the statistics path chosen (training-mode BatchNorm only; otherwise stat_mode is ignored):
 *   stat_mode 0  one statistics row per workgroup row of the convolution, a finalize launch, a BN + SiLU apply launch (= ys_conv_bn_act_fwd)
 *   stat_mode 1  what a model with the default BN_ATOMIC = 1 runs: the convolution epilogues add their sums into zeroed 2^-20 fixed-point
 *                accumulators and the apply pass finalizes from them (no finalize launch); YS_F32 / YS_BF16 only
 * Optional outputs (may be NULL; training-mode BatchNorm only): y_raw [B,Cout,Ho,Wo] the convolution output the statistics are taken over,
 * coef [4][Cout] = scale, shift, mean, rstd of this batch, *stat_rows the number of workgroup partial sums per channel the launch produced. */
YS_API int ys_conv_bn_act_fwd_ex(ys_ctx* ctx, int dtype, const float* x_nchw, int B, int Cin, int H, int W,
                                 const float* w_oihw, int Cout, int k, int stride,
                                 const float* bn_gamma, const float* bn_beta, float* bn_mean, float* bn_var,
                                 const float* bias, int act_silu, int training, int stat_mode, float* y_nchw,
                                 float* y_raw, float* coef, int32_t* stat_rows);

/* The Yolov5u stem Conv(3, Cout, k = 6, s = 2, p = 2) (Models/Yolo.cs:163) on exactly the kernels a bf16 model runs for its model.0 (csrc/conv_stem6.hip), which
 * read the fp32 NCHW image themselves.  Cout in {16, 32, 48, 64, 80}; any other shape returns YS_ERR_UNSUPPORTED (a model runs such a layer on the generic
 * kernels).  fp32 HOST arrays; Ho = (H - 2) / 2 + 1, Wo = (W - 2) / 2 + 1.
 * ys_stem6_fwd: scale == NULL is the training form -- y_nchw [B,Cout,Ho,Wo] = the raw convolution output as the bf16 values the kernel stored, stats [2][Cout] =
 *   the per-channel sum and sum of squares of those values as the kernel produced them (stat_mode 0: fp32 rows, one per workgroup, added up here in double;
 *   stat_mode 1: the 2^-20 fixed-point accumulators, exact sums of the workgroups' rounded partials).  Otherwise eval: y = act(scale * conv + shift) with
 *   act != 0 = SiLU, stats unused (may be NULL).
 * ys_stem6_wgrad: dw_oihw [Cout,3,6,6] = the weight gradient for dy_nchw [B,Cout,Ho,Wo] (rounded to bf16 on the way in, like x): the kernel's partial slabs
 *   followed by the split reduction a model's backward segment runs. */
YS_API int ys_stem6_fwd(ys_ctx* ctx, const float* x_nchw, int B, int H, int W, const float* w_oihw, int Cout, int stat_mode,
                        const float* scale, const float* shift, int act, float* y_nchw, double* stats);
YS_API int ys_stem6_wgrad(ys_ctx* ctx, const float* x_nchw, int B, int H, int W, const float* dy_nchw, int Cout, float* dw_oihw);

/* autograd of the same conv2d (Amp.cs:348,370): given dy [B,Cout,Ho,Wo] returns dx [B,Cin,H,W] (optional, may be
 * NULL) and dw [Cout,Cin,k,k]; all fp32 host arrays. */
YS_API int ys_conv_bwd(ys_ctx* ctx, int dtype, const float* x_nchw, int B, int Cin, int H, int W,
                       const float* w_oihw, int Cout, int k, int stride, const float* dy_nchw,
                       float* dx_nchw, float* dw_oihw);

/* ---- YOLOv11-only operators, one stateless call per kernel family (unit parity of csrc/attn_dw.hip against float64).
 * fp32 HOST arrays at the edge in the reference's layouts; dtype = YS_F32 or YS_BF16 is the storage type on the device.  Every
 * operand is placed inside a WIDER NHWC device buffer the way the model's shared activation buffers hold it: `*_pad` extra
 * channels behind the tensor (attention) or a row pitch `*_ldc` >= C and a first channel `*_coff` (depthwise; 0, 0 = dense).
 * The rest of each buffer the kernels write to -- and a guard behind the probability matrices -- is pre-filled with a sentinel;
 * *view_intact (may be NULL) is 1 when every sentinel element survived the call, 0 when a kernel wrote outside its view.
 * Unsupported geometry (N > 1600, kd > 128, hd > 256, C not a multiple of the 16-byte vector, C / vector > 256 for the weight
 * gradient) returns the launcher's YS_ERR_UNSUPPORTED before any kernel is started.
 *
 * Attention core of Block.Attention (Block.cs:763-805), per head: P = softmax(q^T k * kd^-0.5), ao = v P^T.
 * qkv [B, heads*(2*kd+hd), N] in the reference's view(B, heads, 2*kd+hd, N) order; ao [B, heads*hd, N];
 * P (optional, may be NULL) [B*heads, N, N] fp32 probabilities, row = query. */
YS_API int ys_attn_fwd(ys_ctx* ctx, int dtype, const float* qkv, int B, int N, int heads, int kd, int hd, int ldq_pad, int ldo_pad,
                       float* ao, float* P, int32_t* view_intact);
/* its backward: runs the forward for P, then dq | dk | dv in the qkv layout.  dv_in [B, heads*hd, N] (may be NULL = zeros) is the
 * gradient that already sits in the v slice (it arrived through pe(v)); the kernels ADD P^T dO to it. */
YS_API int ys_attn_bwd(ys_ctx* ctx, int dtype, const float* qkv, int B, int N, int heads, int kd, int hd, int ldq_pad, int ldo_pad,
                       const float* dao, const float* dv_in, float* dqkv, int32_t* view_intact);
/* Depthwise 3x3 / stride 1 / pad 1 (Convs.DWConv, Convs.cs:108-114; groups = C): x, y [B,C,H,W], w [C,1,3,3]. */
YS_API int ys_dwconv3x3_fwd(ys_ctx* ctx, int dtype, const float* x, int B, int C, int H, int W, const float* w,
                            int x_ldc, int x_coff, int y_ldc, int y_coff, float* y, int32_t* view_intact);
/* its autograd given dy [B,C,H,W]: dx [B,C,H,W] (may be NULL; with accumulate != 0 it holds the gradient already in the
 * buffer on entry and receives dx_in + dx, one rounding) and dw [C,1,3,3] (may be NULL; fp32 for both dtypes). */
YS_API int ys_dwconv3x3_bwd(ys_ctx* ctx, int dtype, const float* x, int B, int C, int H, int W, const float* w, const float* dy,
                            int x_ldc, int x_coff, int dx_ldc, int dx_coff, int accumulate, float* dx, float* dw,
                            int32_t* view_intact);

/* ---- BatchNorm training kernels (csrc/batchnorm.hip), one stateless call per launch sequence of a Conv unit (unit parity against float64).
 * Host tensors are CHANNEL-MAJOR [C][rows] fp32 (NCHW with B = 1); C is a multiple of the 16-byte vector (4 fp32 / 8 bf16).  y and dy are dense on the
 * device as in the model; z, res, dz and rg sit at channel `*_coff` of a [rows][*_coff + C + *_pad] buffer pre-filled with a sentinel, and every workspace
 * carries a sentinel guard; view_intact = 1 when all of it survived.  eps = 1e-3, momentum = 0.03; the batch count is `rows`. */
typedef struct ys_bn_fwd_case {
  const float* y;                 /* [C][rows] pre-BN output (rounded to the storage type on the device) */
  const float* gamma;             /* [C] */
  const float* beta;              /* [C] */
  float* run_mean;                /* [C] in / out */
  float* run_var;                 /* [C] in / out */
  float* nbt;                     /* num_batches_tracked as ONE float, in / out; may be NULL */
  const float* res;               /* optional residual [C][rows], added after the activation */
  const float* partial;           /* mode 1: [P][2][C] partial (sum, sum of squares) rows, pushed through the fixed-point accumulator */
  float* z;                       /* out [C][rows] */
  float* coef;                    /* out [4][C]: scale, shift, mean, rstd */
  float* part_out;                /* modes 0 / 2, optional: the partial rows the statistics launch wrote, [nblk][2][C] (room for 768 rows) */
  int64_t* acc_out;               /* mode 1, optional: the raw accumulators [8 shards][C][2] after the push (2^-20 fixed point; bit 62 of word 1 = poison) */
  int32_t rows, C;
  int32_t res_pad, res_coff;
  int32_t z_pad, z_coff;
  int32_t res_shares_z;           /* != 0: res and z are views of ONE buffer (pitch from the larger coff + C, plus z_pad) */
  int32_t P;                      /* mode 1: partial rows */
  int32_t nblk;                   /* out: partial rows of the statistics launch (modes 0 / 2) */
  int32_t view_intact;            /* out */
} ys_bn_fwd_case;
/* mode 0: ys_chan_stats_launch -> ys_bn_finalize_launch -> ys_bn_act_apply_launch (the depthwise unit's path); n = 1
 * mode 1: `partial` through ys_stat_acc_add (the device function of every convolution epilogue) -> ys_bn_fin_apply_launch; n = 1
 * mode 2: ys_chan_stats_launch per problem, then ONE ys_bn_finalize_group_launch + ONE ys_bn_act_apply_group_launch over the n problems
 * More than 256 vectors per row (modes 0 / 2) returns YS_ERR_UNSUPPORTED, more than 9 problems the grouped launcher's status; nothing is launched. */
YS_API int ys_bn_train_fwd(ys_ctx* ctx, int dtype, int mode, int act_silu, int n, ys_bn_fwd_case* cases);

typedef struct ys_bn_bwd_case {
  const float* dz;                /* [C][rows] gradient of the unit's output, inside a padded view */
  const float* y;                 /* [C][rows] pre-BN output of the forward pass */
  const float* coef;              /* [4][C]: scale, shift, mean, rstd of the forward pass */
  float* dgamma;                  /* [C] in / out (the kernels accumulate) */
  float* dbeta;                   /* [C] in / out */
  float* rg;                      /* optional [C][rows] in / out: the residual input's gradient view, receives rg + dz */
  const float* src_part[3];       /* mode 3: partial rows [src_nblk[k]][2][C] of source k */
  float* dy;                      /* out [C][rows] */
  float* k23;                     /* out [2][C]: k2, k3 of dy = scale * du - k2 - y * k3 */
  float* part_out;                /* optional: the partial rows of the reduction launch, [nblk][2][C] (room for 768 rows) */
  int32_t rows, C;
  int32_t dz_pad, dz_coff;
  int32_t rg_pad, rg_coff;
  int32_t nsrc;                   /* mode 3: sources in use; source k covers channels [src_c1[k - 1], src_c1[k]) */
  int32_t src_nblk[3];
  int32_t src_c1[3];
  int32_t nblk;                   /* out */
  int32_t view_intact;            /* out */
} ys_bn_bwd_case;
/* mode 0: ys_bn_bwd_reduce_launch (carries rg) -> ys_bn_bwd_finalize_launch -> ys_bn_bwd_apply_launch; n = 1
 * mode 1: the same with rg carried by the apply pass (the schedule of a unit whose reduction is fused into a dgrad epilogue); n = 1
 * mode 2: the reduction per problem, then ONE ys_bn_bwd_finalize_group_launch + ONE ys_bn_bwd_apply_group_launch (which carries rg) over n problems
 * mode 3: ys_bn_bwd_finalize_src_launch alone on the caller's partial rows (dz, y, dy, rg unused); n = 1 */
YS_API int ys_bn_train_bwd(ys_ctx* ctx, int dtype, int mode, int act_silu, int n, ys_bn_bwd_case* cases);

/* grad[C] += column sums of x [B,C,rows_per_b] (the bias gradients): the view starts at channel coff of a [B * bstride][coff + Cp + ld_pad] buffer,
 * Cp = C rounded up to the vector over ZEROED padding channels; images are bstride >= rows_per_b rows apart (the head outputs). */
YS_API int ys_colsum(ys_ctx* ctx, int dtype, const float* x, int B, int C, int rows_per_b, int bstride, int ld_pad, int coff, float* grad,
                     int32_t* view_intact);
/* Nearest 2x up-sample src [B,C,H,W] -> dst [B,C,2H,2W] (backward = 0) or its gradient src [B,C,2H,2W] -> dst [B,C,H,W] (backward = 1; with
 * accumulate != 0 dst holds the gradient already in the buffer and receives dst + sum, one rounding); row pitch *_ldc >= *_coff + C. */
YS_API int ys_upsample2x(ys_ctx* ctx, int dtype, int backward, const float* src, int B, int H, int W, int C, int s_ldc, int s_coff, int d_ldc,
                         int d_coff, int accumulate, float* dst, int32_t* view_intact);
/* dst view (+)= src view; src, dst [C][rows]. */
YS_API int ys_copy_view(ys_ctx* ctx, int dtype, const float* src, int rows, int C, int s_ldc, int s_coff, int d_ldc, int d_coff, int accumulate,
                        float* dst, int32_t* view_intact);

/* ---- fp8 convolution path (csrc/f8.hip and the quantising passes of csrc/batchnorm.hip), one stateless call per kernel (unit parity against exact
 * references: OCP e4m3fn / e5m2, round to nearest even, saturating).  Sentinels and guards as above.
 *
 * One quantiser launch on x [rows][C] fp32 (ROW-major), stored as bf16 at channel coff of a [rows][coff + C + pad] buffer:
 *   kind 0 / 1  f8_quant_view_kernel<e4m3 / e5m2>: q8 [rows][C] = fp8(bf16(x) * qscale), records amax(|bf16(x)|)           (C % 16 == 0)
 *   kind 2      f8_view_amax_kernel alone: records amax, q8 unused (may be NULL)                                              (C % 8 == 0)
 *   kind 3      f8_quant_weights_kernel on the flat rows * C elements (any count; coff = pad = 0): qscale is amax_w, the multiplier 448 / amax_w (1 when
 *               amax_w is 0); records nothing
 * *amax = the maximum over the ys_f8_amax_ways() slots of the tensor; slots (may be NULL) receives the slots themselves -- one per workgroup index modulo the way
 * count, a slot no workgroup wrote stays 0. */
YS_API int ys_f8_quant(ys_ctx* ctx, int kind, const float* x, int rows, int C, int coff, int pad, float qscale, uint8_t* q8, float* amax, float* slots,
                       int32_t* view_intact);
YS_API int ys_f8_amax_ways(void);
/* The scale bookkeeping of a step: ys_f8_weight_amax_launch over the layers (offset, count) of the flat fp32 parameter array, then ys_f8_scales_launch over the
 * convolutions (conv_layer[c] = index of its layer).  amax_x / amax_dy [n_convs][ways] in / out (float values; cleared by the call), scales [n_convs][4] =
 * s_x, 1 / (s_x s_w), s_g, 1 / (s_g s_w) in / out (a convolution without a recorded maximum keeps s_x / s_g), amax_w [n_layers] out. */
YS_API int ys_f8_scales(ys_ctx* ctx, const float* params, int64_t n_params, const int64_t* layer_off, const int64_t* layer_count, int n_layers,
                        const int32_t* conv_layer, int n_convs, float* amax_x, float* amax_dy, float* scales, float* amax_w);
/* ys_bn_act_apply_q8_launch alone (bf16 storage) with the caller's coefficients: z = act(y scale + shift) (+ res) into its padded view, q8 [rows][C] =
 * e4m3(z qscale) of the STORED z, *amax = max |z|.  y, res, z channel-major [C][rows] as in ys_bn_train_fwd; q8 row-major as on the device. */
YS_API int ys_bn_apply_q8_fwd(ys_ctx* ctx, int act_silu, const float* y, int rows, int C, const float* scale, const float* shift, const float* res, int res_pad,
                              int res_coff, int z_pad, int z_coff, int res_shares_z, float qscale, float* z, uint8_t* q8, float* amax, int32_t* view_intact);
/* ys_bn_bwd_apply_q8_launch alone: coef [4][C] = scale, shift, k2, k3; dy = scale du - k2 - y k3 (dense), q8 = e5m2(dy qscale) of the stored dy, *amax = max |dy|;
 * rg (optional, in / out, padded view) receives rg + dz. */
YS_API int ys_bn_apply_q8_bwd(ys_ctx* ctx, int act_silu, const float* dz, const float* y, int rows, int C, const float* coef, int dz_pad, int dz_coff, float* rg,
                              int rg_pad, int rg_coff, float qscale, float* dy, uint8_t* q8, float* amax, int32_t* view_intact);
/* The fp8 branch of ys_conv_bn_act_fwd_ex (dtype YS_FP8, stat_mode 0; Cin % 32 == 0) with a DELAYED activation scale: prev_amax > 0 replaces the input's own
 * amax in s_x = 0.5 * 448 / amax (0 = current scaling, as ys_conv_bn_act_fwd).  The launch records amax(|bf16(x)|) through ConvArgs::amax as a model's step
 * does: *amax = the maximum over the ways; scales [4] = s_x, 1 / (s_x s_w), s_g, 1 / (s_g s_w) as used. */
YS_API int ys_conv_f8_fwd(ys_ctx* ctx, const float* x_nchw, int B, int Cin, int H, int W, const float* w_oihw, int Cout, int k, int stride,
                          const float* bn_gamma, const float* bn_beta, float* bn_mean, float* bn_var, const float* bias, int act_silu, int training,
                          float prev_amax, float* y_nchw, float* y_raw, float* coef, int32_t* stat_rows, float* scales, float* amax);
/* The fp8 input gradient of ys_conv_bwd (dy -> e5m2, weights -> e4m3; Cout % 32 == 0) with a delayed gradient scale s_g = 8192 / prev_amax (0 = current);
 * *amax = the recorded amax(|bf16(dy)|). */
YS_API int ys_conv_f8_dgrad(ys_ctx* ctx, int B, int Cin, int H, int W, const float* w_oihw, int Cout, int k, int stride, const float* dy_nchw,
                            float prev_amax, float* dx_nchw, float* scales, float* amax);

/* ---- per-block entry points: a TorchSharp-free body for the reference's block modules, one stateful handle per
 *      module instance (SURVEY 8b "ys_c2f_fwd/bwd, ys_c3k2_fwd/bwd, ys_sppf_fwd/bwd, ys_proto_fwd/bwd").  The handle IS a
 *      ys_model: ys_model_num_tensors / tensor_info / set_tensor / get_tensor / get_grad / init_weights / set_training /
 *      zero_grad / optim_adamw_step / destroy all apply, with the module-relative state_dict names TorchSharp gives a
 *      standalone module ("cv1.conv.weight", "m.0.cv2.bn.running_var", "upsample.bias", ...).
 *        YS_BLOCK_CONV        Convs.Conv        (Convs.cs:36-62)    c1->c2, k in {1,3}, s in {1,2}, act
 *        YS_BLOCK_BOTTLENECK  Block.Bottleneck  (Block.cs:572-608)  c1 == c2, 3x3/3x3, hidden int(c2*e), shortcut
 *        YS_BLOCK_C2F         Block.C2f         (Block.cs:371-399)  n Bottlenecks (e = 1.0), shortcut
 *        YS_BLOCK_C3K2        Block.C3k2        (Block.cs:623-662)  n x (C3k(c,c,2) if c3k else Bottleneck(c,c)), e, shortcut = true
 *        YS_BLOCK_SPPF        Block.SPPF        (Block.cs:236-285)  c1 == c2
 *        YS_BLOCK_C2PSA       Block.C2PSA       (Block.cs:664-810)  c1 == c2, (c1/2) % 64 == 0, n PSABlocks
 *        YS_BLOCK_PROTO       Block.Proto       (Block.cs:51-84)    c1 -> n (= c_, hidden) -> c2 masks, output 2H x 2W
 *        YS_BLOCK_C3          Block.C3          (Block.cs:404-442)  n Bottlenecks(k = (1, 3), e = 1.0) on int(c2 * 0.5) channels, shortcut
 *      Channel counts (c1, c2 and every hidden width) must be multiples of 4 (f32) / 8 (bf16): the widths the YOLO graphs use. */
typedef enum ys_block_kind {
  YS_BLOCK_CONV = 0, YS_BLOCK_BOTTLENECK = 1, YS_BLOCK_C2F = 2, YS_BLOCK_C3K2 = 3, YS_BLOCK_SPPF = 4, YS_BLOCK_C2PSA = 5,
  YS_BLOCK_PROTO = 6, YS_BLOCK_C3 = 7
} ys_block_kind;

typedef struct ys_block_desc {
  int32_t kind;       /* ys_block_kind */
  int32_t c1, c2;     /* input / output channels */
  int32_t n;          /* repeats (C2f, C3k2, C2PSA); hidden width c_ (Proto) */
  int32_t shortcut;   /* Bottleneck / C2f */
  int32_t c3k;        /* C3k2: use C3k inner blocks */
  float e;            /* expansion (Bottleneck, C3k2); 0 = the module's default (0.5) */
  int32_t k, s, act;  /* Conv */
  int32_t height;     /* input H */
  int32_t width;      /* input W */
  int32_t max_batch;
  int32_t dtype;      /* ys_dtype */
} ys_block_desc;

YS_API int ys_block_create(ys_ctx* ctx, const ys_block_desc* desc, ys_model** out);
/* output geometry of the block: [c, h, w] */
YS_API int ys_block_output_shape(ys_model* block, int32_t shape_chw[3]);
/* y = module.forward(x): x fp32 NCHW [batch,c1,H,W], y fp32 NCHW [batch,c2,Ho,Wo]; host arrays (on_device = 0) or device
 * pointers (1).  Training mode uses batch statistics and updates the running ones, exactly like the full model. */
YS_API int ys_block_forward(ys_model* block, const float* x_nchw, int on_device, int batch, float* y_nchw);
/* autograd of the last training-mode forward: given dy (shape of y) accumulates parameter gradients (read with
 * ys_model_get_grad) and writes dx (shape of x; may be NULL). */
YS_API int ys_block_backward(ys_model* block, const float* dy_nchw, int on_device, float* dx_nchw);

/* ---- the heads as standalone modules (Detect / Segment handles; round 3).
 * Modules/Head.cs:8-236 Detect, :238-374 Segment, :376-482 Obb, :484-606 Pose, :612-644 Classify: the three neck feature maps in, the criterion's
 * `preds` (training) / the decoded predictions (eval) out.  The handle is a ys_model without a backbone: the state_dict surface
 * (module-relative names "cv2.0.0.conv.weight", "cv3...", "dfl.conv.weight", "proto...", "cv4..."; Head.cs registration order),
 * ys_model_set_training, ys_model_get_output ("boxes", "scores", "pred", "mask_coefficient", "proto", "kpts", "angle" and their
 * "d..." gradients), ys_loss_detect / _segment / _obb / _pose, ys_model_zero_grad and the optimizer calls work on it unchanged. */
typedef struct ys_head_desc {
  int32_t family;        /* ys_family: YS_YOLOV8 = Detect(legacy: 3x3 cls tower), YS_YOLOV11 = depthwise + 1x1 cls tower (Head.cs:50) */
  int32_t task;          /* ys_task: which head */
  int32_t nc, reg_max;
  int32_t ch[3];         /* channels of P3, P4, P5 (multiples of 4 for f32, 8 for bf16).  YS_CLASSIFY: ch[0] = c1, ch[1] / ch[2] ignored */
  int32_t height, width; /* INPUT IMAGE size (multiple of 32): level i sees [height / s_i, width / s_i], s = 8, 16, 32 (Head.cs:43) */
  int32_t max_batch, dtype;
  int32_t kpt_num, kpt_dim;   /* YS_POSE (0 = 17 x 3) */
} ys_head_desc;
YS_API int ys_head_create(ys_ctx* ctx, const ys_head_desc* desc, ys_model** out);
/* x[i]: fp32 NCHW [batch, ch[i], height / s_i, width / s_i], host arrays (on_device = 0) or device pointers (1).
 * YS_CLASSIFY: x[0] only, [batch, c1, height / 32, width / 32]; the head's outputs are ys_model_get_output's "cls" / "logits". */
YS_API int ys_head_forward(ys_model* head, const float* const x[3], int on_device, int batch);
/* Gradients of the head outputs supplied by the caller instead of a ys_loss_* call: [B, 4*reg_max, A], [B, nc, A], the task's
 * extra output ([B, nm | 1 | nk, A]; NULL for Detect) and the prototypes ([B, nm, mh, mw]; Segment only); fp32 host arrays.
 * YS_CLASSIFY: dscores = d(loss)/d(logits) [B, nc]; the other three are ignored. */
YS_API int ys_head_set_grads(ys_model* head, const float* dboxes, const float* dscores, const float* dextra, const float* dproto);
/* autograd of the last training-mode ys_head_forward from the gradients the criterion (or ys_head_set_grads) left on the head outputs:
 * accumulates the parameter gradients and writes dx[i] (shape of x[i]; entries / the array may be NULL). */
YS_API int ys_head_backward(ys_model* head, int on_device, float* const dx[3]);

/* device memory helpers for hosts without a HIP binding of their own */
YS_API int ys_device_malloc(ys_ctx* ctx, size_t bytes, void** dptr);
YS_API int ys_device_free(ys_ctx* ctx, void* dptr);
YS_API int ys_memcpy_h2d(ys_ctx* ctx, void* dst, const void* src, size_t bytes);
YS_API int ys_memcpy_d2h(ys_ctx* ctx, void* dst, const void* src, size_t bytes);

/* timing of the most recent calls on this ctx's stream, measured with HIP events on that stream:
 * name = "forward" | "loss" | "backward" | "optim" | "nms"; returns ms of the last completed call. */
YS_API int ys_ctx_profile_enable(ys_ctx* ctx, int enable);
YS_API int ys_ctx_last_ms(ys_ctx* ctx, const char* name, float* ms);

/* per-kernel-class timing (HIP events on this ctx's stream around every launch of a class, e.g. "conv_igemm",
 * "conv_wgrad", "bn_act", "nms"); enable for a few UNTIMED steps, then read the launch count and summed duration. */
YS_API int ys_ctx_kernel_profile(ys_ctx* ctx, int enable);
YS_API int ys_ctx_kernel_profile_read(ys_ctx* ctx, const char* name, int32_t* launches, float* total_ms);
/* per-launch CSV (class,label,us) of everything recorded since profiling was enabled (triage tool) */
YS_API int ys_ctx_kernel_profile_dump(ys_ctx* ctx, const char* path);

#ifdef __cplusplus
}
#endif
#endif /* YOLOSHARP_HIP_H */
