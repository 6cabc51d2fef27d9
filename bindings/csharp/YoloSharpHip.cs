// YoloSharpHip.cs -- P/Invoke declarations for libyolosharp_hip.so (C ABI: include/yolosharp_hip.h).
// Drop this file into YoloSharp (e.g. YoloSharp/Native/YoloSharpHip.cs); INTEGRATION.md section 2 maps the reference's call sites
// (Models/YoloBaseTaskModel.cs:142-160, Models/Detector.cs:27-72, Utils/Amp.cs:260-286, Utils/Ops.cs:239-371) onto these entry points.
// Not compiled in this repository's image (no dotnet); tests/test_abi.py checks that every symbol declared here is exported by the
// library and declared in include/yolosharp_hip.h.
using System;
using System.Runtime.InteropServices;

namespace YoloSharp.Native
{
    [StructLayout(LayoutKind.Sequential)]
    internal struct YsHeadDesc
    {
        public int family;     // 8 = Detect(legacy), 11 = depthwise + 1x1 class tower (Modules/Head.cs:50)
        public int task;       // 0 Detect, 1 Segment, 2 Obb, 3 Pose, 4 Classify (ch[0] = c1 of one [height/32, width/32] map)
        public int nc, reg_max;
        [MarshalAs(UnmanagedType.ByValArray, SizeConst = 3)] public int[] ch;   // channels of P3, P4, P5
        public int height, width;   // input IMAGE size; level i sees [height / s_i, width / s_i], s = 8, 16, 32 (Head.cs:43)
        public int max_batch, dtype, kpt_num, kpt_dim;
    }

    [StructLayout(LayoutKind.Sequential)]
    internal struct YsModelDesc
    {
        public int family;     // 5 = Yolov5u (Models/Yolo.cs:137; task 0 only), 8 = Yolov8 (Models/Yolo.cs:10), 11 = Yolov11
        public int size;       // YoloSize n,s,m,l,x = 0..4 (Types/YoloTypes.cs)
        public int task;       // 0 detect, 1 segment, 2 obb, 3 pose, 4 classify (Yolov8Classify / Yolov11Classify; Float32 or BFloat16)
        public int nc, reg_max, height, width, max_batch;
        public int dtype;      // 0 = Float32 (parity path), 1 = BFloat16 (performance path), 2 = bf16 + fp8 MFMA convolutions
        public int max_labels; // INITIAL ground-truth capacity per image (0 -> 64); host-label loss calls grow it, see ys_model_reserve_labels
        public int kpt_num, kpt_dim; // task 3: Yolov8Pose(kpt_num: 17, kpt_dim: 3) (Models/Yolo.cs:473); 0 -> defaults
    }

    internal static class Hip
    {
        const string Lib = "yolosharp_hip";   // libyolosharp_hip.so next to the assembly / on LD_LIBRARY_PATH

        [DllImport(Lib)] internal static extern IntPtr ys_last_error();
        [DllImport(Lib)] internal static extern int ys_ctx_create(int device, out IntPtr ctx);
        [DllImport(Lib)] internal static extern int ys_ctx_destroy(IntPtr ctx);
        [DllImport(Lib)] internal static extern int ys_ctx_synchronize(IntPtr ctx);

        [DllImport(Lib)] internal static extern int ys_model_create(IntPtr ctx, ref YsModelDesc desc, out IntPtr model);
        [DllImport(Lib)] internal static extern int ys_model_destroy(IntPtr model);
        [DllImport(Lib)] internal static extern int ys_model_num_tensors(IntPtr model);
        [DllImport(Lib, CharSet = CharSet.Ansi)]
        internal static extern int ys_model_tensor_info(IntPtr model, int index, byte[] name, int nameCap,
                                                        out int ndim, [Out] long[] shape4, out int isParam);
        [DllImport(Lib, CharSet = CharSet.Ansi)]
        internal static extern int ys_model_set_tensor(IntPtr model, string name, float[] host, UIntPtr count);
        [DllImport(Lib, CharSet = CharSet.Ansi)]
        internal static extern int ys_model_get_tensor(IntPtr model, string name, [Out] float[] host, UIntPtr count);
        [DllImport(Lib)] internal static extern int ys_model_set_training(IntPtr model, int training);
        [DllImport(Lib)] internal static extern int ys_model_num_anchors(IntPtr model);

        [DllImport(Lib)] internal static extern int ys_model_forward(IntPtr model, float[] imagesNchw, int onDevice, int batch);
        [DllImport(Lib, CharSet = CharSet.Ansi)]
        internal static extern int ys_model_get_output(IntPtr model, string key, [Out] float[] host, UIntPtr count);
        [DllImport(Lib)] internal static extern int ys_model_pred_device(IntPtr model, out IntPtr dptr);

        [DllImport(Lib)] internal static extern int ys_loss_detect(IntPtr model, float[] batchIdx, float[] cls, float[] bboxes, int n, int onDevice);
        [DllImport(Lib)] internal static extern int ys_loss_read(IntPtr model, [Out] float[] items3, out float lossSum);
        // criterion on caller-supplied preds (Loss.cs:411 forward(preds, batch)); device-label callers reserve the per-image label capacity
        [DllImport(Lib)] internal static extern int ys_model_set_preds(IntPtr model, int batch, float[] boxes, float[] scores, float[] maskCoefficient, float[] proto);
        [DllImport(Lib)] internal static extern int ys_model_decode_preds(IntPtr model);
        [DllImport(Lib)] internal static extern int ys_model_reserve_labels(IntPtr model, int perImage);
        // End2End (Config.End2End = true, the reference's default): YoloBaseTaskModel.One2one_Init; outputs "one2one_boxes" / "one2one_scores" / "one2one_dboxes" /
        // "one2one_dscores" / "det" through ys_model_get_output; ys_loss_detect is then E2EDetectLoss; rows [B,k,6] of the eval forward stay on the device
        [DllImport(Lib)] internal static extern int ys_model_one2one_init(IntPtr model, int maxDet);
        [DllImport(Lib)] internal static extern int ys_model_det_device(IntPtr model, out IntPtr rows, out int k);
        [DllImport(Lib)] internal static extern int ys_e2e_topk(IntPtr ctx, float[] pred, int onDevice, int batch, int nc, int anchors, int maxDet, [Out] float[] rows, [Out] long[] anchor);
        [DllImport(Lib)] internal static extern int ys_e2e_select(IntPtr ctx, float[] rows, int onDevice, int batch, int k, float confThres, int maxDet, [Out] int[] count);
        // End2End Segment (Segmenter.cs:17-24): One2one_Init for Detect and Segment models; ys_loss_segment is then E2ESegmentLoss (gains 0.8 / 0.2; ys_model_e2e_update =
        // E2ESegmentLoss.update(), which the reference's loop never calls for Segment); outputs "one2one_mask_coefficient" / "one2one_dmask_coefficient"; "det" rows [B,k,6+nm]
        [DllImport(Lib)] internal static extern int ys_model_e2e_init(IntPtr model, int maxDet, int epochs);
        // End2End OBB (Obber.cs:18-24): One2one_Init for OBB models; ys_loss_obb is then E2EOBBLoss, whose update() the training loop calls after every epoch
        // (YoloBaseTaskModel.cs:350-353) = ys_model_e2e_update; outputs "one2one_angle" / "one2one_dangle"; "det" rows [B,k,7] = (cx, cy, w, h, score, class, angle)
        [DllImport(Lib)] internal static extern int ys_model_e2e_obb_init(IntPtr model, int maxDet, int epochs);
        // Obber.Val's per-image part (Obber.cs:102-114) for a batch: rows [B,maxDet,rowStride] (device or host), correct [B,maxDet,10]
        [DllImport(Lib)] internal static extern int ys_val_match_rotated_batched(IntPtr ctx, IntPtr rows, IntPtr count, int onDevice, int batch, int maxDet, int rowStride, int angleCol, IntPtr batchIdx, IntPtr cls, IntPtr bboxes, int nLabels, float imgW, float imgH, IntPtr correct);
        // End2End Pose (PoseDetector.cs:21-36): One2one_Init for Pose models; ys_loss_pose is then E2EPoseLoss (gains 0.8 / 0.2; the reference's loop never steps them for Pose);
        // outputs "one2one_kpts" / "one2one_dkpts"; "det" rows [B,k,6+nk] = (x1, y1, x2, y2, score, class, keypoints)
        [DllImport(Lib)] internal static extern int ys_model_e2e_pose_init(IntPtr model, int maxDet, int epochs);
        // PoseDetector.Val's per-image part (PoseDetector.cs:131-165) for a batch: rows [B,maxDet,rowStride] (device or host), correctBox / correctPose [B,maxDet,10]
        [DllImport(Lib)] internal static extern int ys_val_match_pose_batched(IntPtr ctx, IntPtr rows, IntPtr count, int onDevice, int batch, int maxDet, int rowStride, int kptCol, int kptNum, int kptDim, IntPtr batchIdx, IntPtr cls, IntPtr bboxes, IntPtr keypoints, int labelKptDim, int nLabels, float imgW, float imgH, IntPtr correctBox, IntPtr correctPose);
        [DllImport(Lib)] internal static extern int ys_model_e2e_update(IntPtr model);
        [DllImport(Lib)] internal static extern int ys_model_e2e_gains(IntPtr model, out float o2m, out float o2o);
        [DllImport(Lib)] internal static extern int ys_e2e_topk_ex(IntPtr ctx, float[] pred, int onDevice, int batch, int nc, int extra, int anchors, int maxDet, [Out] float[] rows, [Out] long[] anchor);
        [DllImport(Lib)] internal static extern int ys_e2e_select_ex(IntPtr ctx, float[] rows, int onDevice, int batch, int k, int rowLen, float confThres, int maxDet, [Out] int[] count);
        [DllImport(Lib)] internal static extern int ys_tal_keep_best(IntPtr ctx, float[] align, [In, Out] byte[] maskPos, int[] gtCount, int onDevice, int batch, int boxes, int anchors);
        // 0 = disjoint AdamW groups, 1 = the overlapping groups of YoloBaseTaskModel.cs:144-151 exactly as written
        [DllImport(Lib)] internal static extern int ys_optim_set_param_groups(IntPtr model, int mode);
        // Augment.LetterBox / Augment.Rectangle (Data/Augment.cs:698-857) on the device; uint8 planes (isFloat = 0) or fp32 masks
        [DllImport(Lib)] internal static extern int ys_letterbox(IntPtr ctx, byte[] src, int isFloat, int onDevice, int C, int h, int w, int fitW, int fitH,
                                                                 int outW, int outH, int color, [Out] byte[] dst, out int padL, out int padU);
        // Training input on the device (Data/YoloDataset.cs:57-151: Mosaic4 + RandomPerspective + FlipLR / FlipUD + Normalize + mul(1/255) + collate): the sources live in
        // one uint8 arena, an item carries what the reference draws per output image.  Device-resident callers pass IntPtr (on_device = 1) for every pointer.
        // Quirk kept: a flipped box keeps x1 > x2 (negative w after cxcywh) unless flags has YS_AUG_SORT_FLIPPED (1).  OBB corner labels: the *_obb entries below.  Not built: the `rand > p` case of Mosaic.
        [StructLayout(LayoutKind.Sequential)] internal struct YsAugSrc { public long imgOff, maskOff; public int h, w, mh, mw; }
        [StructLayout(LayoutKind.Sequential)] internal struct YsAugItem { public int src0, src1, src2, src3, xc, yc; public float m00, m01, m02, m10, m11, m12, m20, m21, m22; public int flipLr, flipUd; }
        [DllImport(Lib)] internal static extern int ys_augment_mosaic(IntPtr ctx, IntPtr arena, IntPtr srcs, int nSrc, IntPtr items, int batch, int onDevice, int imgsz,
                                                                      int maskRatio, int perspective, IntPtr images, IntPtr masks);
        [DllImport(Lib)] internal static extern int ys_augment_labels(IntPtr ctx, IntPtr srcs, IntPtr labOff, IntPtr cls, IntPtr boxes, IntPtr keypoints, int kptNum, int kptDim,
                                                                      IntPtr items, int batch, int onDevice, int imgsz, int perspective, int flags, int capacity,
                                                                      IntPtr outBatchIdx, IntPtr outCls, IntPtr outBboxes, IntPtr outKeypoints, IntPtr outCount);
        // The LetterBox pipeline of CloseMosaic(true) / ImageProcessType.Letterbox (Data/YoloDataset.cs:378-429: LetterBox + FlipLR / FlipUD + Normalize + mul(1/255) + collate) on
        // the same arena, tables and items: only src0, flipLr and flipUd of an item are read.  Quirk kept: a flipped cxcywh box's width becomes s - w (Augment.cs:888-892)
        // unless flags has YS_AUG_FLIP_KEEP_SIZE (2).
        internal const int YS_AUG_SORT_FLIPPED = 1, YS_AUG_FLIP_KEEP_SIZE = 2;
        [DllImport(Lib)] internal static extern int ys_augment_letterbox(IntPtr ctx, IntPtr arena, IntPtr srcs, int nSrc, IntPtr items, int batch, int onDevice, int imgsz,
                                                                         int maskRatio, IntPtr images, IntPtr masks);
        [DllImport(Lib)] internal static extern int ys_augment_letterbox_labels(IntPtr ctx, IntPtr srcs, int nSrc, IntPtr labOff, IntPtr cls, IntPtr boxes, IntPtr keypoints,
                                                                                int kptNum, int kptDim, IntPtr items, int batch, int onDevice, int imgsz, int flags, int capacity,
                                                                                IntPtr outBatchIdx, IntPtr outCls, IntPtr outBboxes, IntPtr outKeypoints, IntPtr outCount);
        // ColorJitter (RandomHSV, Data/Augment.cs:968-987; torchvision's uint8 algorithm, parity with TorchVision.NET unpinned): one row per output image holds what
        // get_params draws -- the op id of each slot (0 brightness, 1 contrast, 2 saturation, 3 hue, -1 nothing) and the factor of each op id.  The *_jitter entries are
        // the plain ones with the rows applied in the gather kernels' epilogue (jitter = IntPtr.Zero: the plain entry; a contrast row: YS_ERR_UNSUPPORTED);
        // ys_color_jitter is the operator on its own (all four ops; dst uint8 or fp32 byte / 255), e.g. for ClassificationDataset's chain.
        [StructLayout(LayoutKind.Sequential)] internal struct YsAugJitter { public int order0, order1, order2, order3; public float brightness, contrast, saturation, hue; }
        [DllImport(Lib)] internal static extern int ys_augment_mosaic_jitter(IntPtr ctx, IntPtr arena, IntPtr srcs, int nSrc, IntPtr items, int batch, int onDevice, int imgsz,
                                                                             int maskRatio, int perspective, IntPtr jitter, IntPtr images, IntPtr masks);
        [DllImport(Lib)] internal static extern int ys_augment_letterbox_jitter(IntPtr ctx, IntPtr arena, IntPtr srcs, int nSrc, IntPtr items, int batch, int onDevice,
                                                                                int imgsz, int maskRatio, IntPtr jitter, IntPtr images, IntPtr masks);
        [DllImport(Lib)] internal static extern int ys_color_jitter(IntPtr ctx, IntPtr src, IntPtr jitter, int batch, int h, int w, int onDevice, IntPtr dst, int dstIsFloat);
        // The classification input (Data/ClassificationDataset.cs:90-131, Auto_Augment = None): RandomResizedCrop / Resize + CenterCrop, the flips, RandomErasing,
        // ColorJitter (contrast included) and mul(1 / 255) as one gather from the uploaded uint8 arena; an item is the DRAWN geometry of one output image (the host keeps
        // the draws).  srcCls [nSrc] fp32 class ids; images fp32 [batch, 3, imgsz, imgsz]; outCls fp32 [batch] (what ys_loss_classify(onDevice = 1) reads).
        // jitter = IntPtr.Zero: no jitter (the val chain).  The interpolation (nearest), Resize(int) and CenterCrop's rounding are unpinned against TorchVision.NET.
        [StructLayout(LayoutKind.Sequential)] internal struct YsClsItem { public int src, top, left, ch, cw, oh, ow, oy, ox, flipLr, flipUd, erY, erX, erH, erW; public uint erSeed; }
        [DllImport(Lib)] internal static extern int ys_augment_classify(IntPtr ctx, IntPtr arena, IntPtr srcs, int nSrc, IntPtr srcCls, IntPtr items, int batch, int onDevice,
                                                                        int imgsz, IntPtr jitter, IntPtr images, IntPtr outCls);
        // Auto_Augment = AutoAugment (the reference's default) / RandAugment (Data/ClassificationDataset.cs:105-116): one YsAaRow per image = two operator slots run
        // between the flips and RandomErasing; op id in torchvision's _augmentation_space order (-1 nothing, 0 ShearX .. 13 Invert), arg = 1 + m for the blends / bits /
        // threshold, theta = torchvision's inverse affine matrix rounded to fp32 (the host keeps the policy, probability, sign and magnitude draws).  aa = IntPtr.Zero is
        // ys_augment_classify.  ys_auto_augment_ops is the two slots on their own on uint8 [b, 3, h, w].  AugMix is not built; the policy table, the magnitude spaces and
        // the operator arithmetic are torchvision's public ones, unpinned against TorchVision.NET.
        [StructLayout(LayoutKind.Sequential)] internal struct YsAaRow { public int op0, op1; public float arg0, arg1;
                                                                        public float t00, t01, t02, t03, t04, t05, t10, t11, t12, t13, t14, t15; }
        [DllImport(Lib)] internal static extern int ys_augment_classify_aa(IntPtr ctx, IntPtr arena, IntPtr srcs, int nSrc, IntPtr srcCls, IntPtr items, int batch, int onDevice,
                                                                           int imgsz, IntPtr aa, IntPtr jitter, IntPtr images, IntPtr outCls);
        [DllImport(Lib)] internal static extern int ys_auto_augment_ops(IntPtr ctx, IntPtr src, int batch, int h, int w, IntPtr rows, int onDevice, IntPtr dst);
        // OBB corner labels (Data/YoloDataset.cs:110-129; Utils/Ops.cs:44-54): corners [n, 4, 2] pixels in place of the keypoints, outBboxes [capacity, 5] = (cx, cy, w, h) / imgsz
        // and the angle of the minimum-area rectangle, angle in (0, pi/2], w along the angle (OpenCV >= 4.5.1's form; the choice among equal-area rectangles is unpinned
        // against OpenCV).  boxes [n, 4] alone decides what is kept; flags must be 0.  ys_xyxyxyxy2xywhr is the rectangle on its own: [n, 4, 2] -> [n, 5], pixels and radians.
        [DllImport(Lib)] internal static extern int ys_xyxyxyxy2xywhr(IntPtr ctx, IntPtr corners, int n, int onDevice, IntPtr outRows);
        [DllImport(Lib)] internal static extern int ys_augment_labels_obb(IntPtr ctx, IntPtr srcs, IntPtr labOff, IntPtr cls, IntPtr boxes, IntPtr corners, IntPtr items, int batch,
                                                                          int onDevice, int imgsz, int perspective, int flags, int capacity, IntPtr outBatchIdx, IntPtr outCls,
                                                                          IntPtr outBboxes, IntPtr outCount);
        [DllImport(Lib)] internal static extern int ys_augment_letterbox_labels_obb(IntPtr ctx, IntPtr srcs, int nSrc, IntPtr labOff, IntPtr cls, IntPtr boxes, IntPtr corners,
                                                                                    IntPtr items, int batch, int onDevice, int imgsz, int flags, int capacity,
                                                                                    IntPtr outBatchIdx, IntPtr outCls, IntPtr outBboxes, IntPtr outCount);
        // Classify task (Head.Classify / v8ClassificationLoss / Classifier.Val, Models/Classifier.cs): outputs "cls" / "logits" / "dcls" [B,nc]
        // through ys_model_get_output; one loss item (the mean) through ys_loss_read_items
        [DllImport(Lib)] internal static extern int ys_loss_classify(IntPtr model, float[] cls, int batch, int onDevice);
        [DllImport(Lib)] internal static extern int ys_cls_topk(IntPtr ctx, float[] scores, int onDevice, int rows, int cols, int k, [Out] int[] idx);
        // Obb / Pose tasks (Head.Obb / v8OBBLoss, Head.Pose / v8PoseLoss)
        [DllImport(Lib)] internal static extern int ys_loss_obb(IntPtr model, float[] batchIdx, float[] cls, float[] bboxes5, int n, int onDevice);
        [DllImport(Lib)] internal static extern int ys_loss_pose(IntPtr model, float[] batchIdx, float[] cls, float[] bboxes, int n, float[] keypoints, int onDevice);
        // Segment task (Head.Segment / v8SegmentationLoss / Ops.process_mask)
        [DllImport(Lib)] internal static extern int ys_loss_segment(IntPtr model, float[] batchIdx, float[] cls, float[] bboxes, int n,
                                                                    float[] masks /* [B,H/4,W/4] overlap-encoded ids */, int onDevice, int cropMode);
        [DllImport(Lib)] internal static extern int ys_loss_read_items(IntPtr model, [Out] float[] items, int nItems, out float lossSum);
        [DllImport(Lib)] internal static extern int ys_loss_read_targets(IntPtr model, [Out] int[] targetGtIdx /* [B*A], -1 = background */, [Out] float[] targetScore, out float tss);
        [DllImport(Lib)] internal static extern int ys_process_mask(IntPtr ctx, float[] protos, float[] masksIn, float[] boxes, int onDevice,
                                                                    int n, int nm, int mh, int mw, int ih, int iw, int upsample, int cropMode,
                                                                    [Out] byte[] outMasks);
        [DllImport(Lib)] internal static extern int ys_model_backward(IntPtr model);
        [DllImport(Lib)] internal static extern int ys_model_zero_grad(IntPtr model);
        [DllImport(Lib)] internal static extern int ys_model_set_overlap(IntPtr model, int on);   // weight-gradient kernels on a second stream (default on)
        [DllImport(Lib)] internal static extern int ys_optim_adamw_step(IntPtr model, float[] lrPerGroup, int nGroups,
                                                                        float beta1, float beta2, float eps, float weightDecay);

        [DllImport(Lib)] internal static extern int ys_mask_iou(IntPtr ctx, float[] gtIds, int nl, byte[] predMasks, int n, int npix, float eps,
                                                                int onDevice, [Out] float[] iou);
        [DllImport(Lib)] internal static extern int ys_match_predictions(IntPtr ctx, float[] predCls, int n, float[] trueCls, int nl, float[] iou,
                                                                         int onDevice, [Out] byte[] correct);
        // per-block handles (Modules.Conv / Bottleneck / C2f / C3k2 / SPPF / C2PSA / Proto / C3 as standalone Module<Tensor,Tensor>; kind 0..7 in that order)
        [StructLayout(LayoutKind.Sequential)] internal struct BlockDesc {
            public int kind, c1, c2, n, shortcut, c3k; public float e; public int k, s, act, height, width, maxBatch, dtype; }
        [DllImport(Lib)] internal static extern int ys_block_create(IntPtr ctx, ref BlockDesc desc, out IntPtr block);
        [DllImport(Lib)] internal static extern int ys_block_output_shape(IntPtr block, [Out] int[] chw);
        [DllImport(Lib)] internal static extern int ys_block_forward(IntPtr block, float[] xNchw, int onDevice, int batch, [Out] float[] yNchw);
        [DllImport(Lib)] internal static extern int ys_block_backward(IntPtr block, float[] dyNchw, int onDevice, [Out] float[] dxNchw);
        // Modules/Head.cs Detect / Segment / Obb / Pose as standalone modules (a ys_model without a backbone: state_dict, set_training,
        // get_output, the ys_loss_* criteria and the optimizer calls work on the handle unchanged)
        [DllImport(Lib)] internal static extern int ys_head_create(IntPtr ctx, ref YsHeadDesc desc, out IntPtr head);
        [DllImport(Lib)] internal static extern int ys_head_forward(IntPtr head, IntPtr[] xNchw3, int onDevice, int batch);   // pinned float[] or device pointers
        [DllImport(Lib)] internal static extern int ys_head_set_grads(IntPtr head, float[] dBoxes, float[] dScores, float[] dExtra, float[] dProto);
        [DllImport(Lib)] internal static extern int ys_head_backward(IntPtr head, int onDevice, IntPtr[] dxNchw3);

        // the Yolov5u stem Conv(3, c, 6, 2, 2) on the kernels a bf16 model runs for model.0 (unit parity; scale == null: training form)
        [DllImport(Lib)] internal static extern int ys_stem6_fwd(IntPtr ctx, float[] xNchw, int batch, int h, int w, float[] wOihw, int cout, int statMode,
                                                                 float[] scale, float[] shift, int act, [Out] float[] yNchw, [Out] double[] stats);
        [DllImport(Lib)] internal static extern int ys_stem6_wgrad(IntPtr ctx, float[] xNchw, int batch, int h, int w, float[] dyNchw, int cout, [Out] float[] dwOihw);

        [DllImport(Lib)] internal static extern int ys_nms_batched(IntPtr ctx, float[] pred, int onDevice, int batch, int channels, int anchors,
                                                                   float conf, float iou, int maxDet, int nc, int maxNms, int maxWh,
                                                                   [Out] float[] rows, [Out] long[] keep, [Out] int[] count);
        [DllImport(Lib)] internal static extern int ys_nms_rotated_batched(IntPtr ctx, float[] pred, int onDevice, int batch, int channels, int anchors,
                                                                   float conf, float iou, int maxDet, int nc, int maxNms, int maxWh,
                                                                   [Out] float[] rows, [Out] long[] keep, [Out] int[] count);
        [DllImport(Lib)] internal static extern int ys_probiou(IntPtr ctx, float[] obb1, float[] obb2, int onDevice, int n, int ciou, float eps, float[] output);
        [DllImport(Lib)] internal static extern int ys_batch_probiou(IntPtr ctx, float[] obb1, int n, float[] obb2, int m, int onDevice, float eps, float[] output);
        // data-parallel step without torch (include/yolosharp_hip.h "multi-GPU"): one process per GPU, rank 0 makes the 128-byte RCCL id and
        // ships it over any host channel.  ORDER MATTERS: call ys_dist_init right after ys_ctx_create and BEFORE ys_model_create -- the
        // communicator's streams must exist before the engine creates its weight-gradient stream (otherwise both engine streams can land
        // on one hardware queue and nothing overlaps: 11.6 instead of 10.3 ms/step measured at one rank; ys_dist_init also runs one
        // all-reduce so that RCCL's lazily created resources exist when it returns).
        // routing / tuning options (include/yolosharp_hip.h: process-wide table, seeded from YS_<KEY>=<number> environment variables at load)
        [DllImport(Lib)] internal static extern int ys_set_option([MarshalAs(UnmanagedType.LPStr)] string key, double value);
        [DllImport(Lib)] internal static extern int ys_unset_option([MarshalAs(UnmanagedType.LPStr)] string key);
        [DllImport(Lib)] internal static extern int ys_get_option([MarshalAs(UnmanagedType.LPStr)] string key, out double value, out int isSet);
        [DllImport(Lib)] internal static extern int ys_dist_unique_id([Out] byte[] id128);
        [DllImport(Lib)] internal static extern int ys_dist_init(IntPtr ctx, int rank, int world, byte[] id128);
        [DllImport(Lib)] internal static extern int ys_dist_destroy(IntPtr ctx);
        [DllImport(Lib)] internal static extern int ys_dist_allreduce_grads(IntPtr model, int segment);
        [DllImport(Lib)] internal static extern int ys_dist_wait(IntPtr model);
        [DllImport(Lib)] internal static extern int ys_model_backward_allreduce(IntPtr model);   // segmented backward, each segment's SUM all-reduce overlapped with the next
        // hosts with a collective of their own: asynchronous segment ends + a fence for their communication stream
        [DllImport(Lib)] internal static extern int ys_model_backward_segments(IntPtr model);
        [DllImport(Lib)] internal static extern int ys_model_backward_segment_async(IntPtr model, int seg);
        [DllImport(Lib)] internal static extern int ys_model_segment_fence(IntPtr model, int seg, IntPtr hipStream);
        [DllImport(Lib)] internal static extern int ys_model_segment_grad_range(IntPtr model, int seg, out long offset, out long count);

        internal static void Check(int status)
        {
            if (status == 0) return;
            string msg = Marshal.PtrToStringAnsi(ys_last_error()) ?? "yolosharp_hip error";
            if (status == 1) throw new ArgumentException(msg);   // same exception type as Ops.cs:248-255
            throw new InvalidOperationException($"yolosharp_hip status {status}: {msg}");
        }
    }
}
