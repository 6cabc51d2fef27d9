"""Host mirror of Models/Detector.cs on the engine: ImagePredict (:26-72) and Val (:76-154).

Everything per image / per anchor runs on the device (eval forward + decode, NMS, box_iou + match_predictions); only the
epoch-level ap_per_class (small) and the reference's integer truncation of the results stay on the host.  The model must have
been created with (height, width) = the padded image size: the reference pads bottom/right with 114 to a multiple of 32
before dividing by 255 (Detector.cs:35-41), this does the same."""
import contextlib

import numpy as np

from . import _lib
from . import metrics as M
from . import model as _model
from .engine import flatten_labels
from .model import AMPWrapper


class YoloResult:
    """Types/YoloResult: integer box (truncated like Detector.cs:52-68)."""
    __slots__ = ("ClassID", "Score", "CenterX", "CenterY", "Width", "Height", "Radian", "KeyPoints")

    def __init__(self, row):
        x, y = int(row[0]), int(row[1])
        rw, rh = int(row[2]) - x, int(row[3]) - y
        self.ClassID, self.Score = int(row[5]), float(row[4])
        self.CenterX, self.CenterY, self.Width, self.Height = x + rw // 2, y + rh // 2, rw, rh
        self.Radian, self.KeyPoints = 0.0, None

    def __repr__(self):
        return f"YoloResult(cls={self.ClassID}, score={self.Score:.3f}, cx={self.CenterX}, cy={self.CenterY}, w={self.Width}, h={self.Height})"


def pad_to_32(image_chw_u8):
    """Detector.cs:33-41: zero-pad mode with value 114 on the bottom / right to a multiple of 32, then / 255."""
    c, h, w = image_chw_u8.shape
    ph, pw = (32 - h % 32) % 32, (32 - w % 32) % 32
    out = np.full((c, h + ph, w + pw), 114.0, np.float32)
    out[:, :h, :w] = image_chw_u8
    return out / np.float32(255.0)


def clip_boxes(boxes, shape):
    """Ops.clip_boxes: xyxy clipped to (h, w)."""
    b = boxes.copy()
    b[:, [0, 2]] = np.clip(b[:, [0, 2]], 0, shape[1])
    b[:, [1, 3]] = np.clip(b[:, [1, 3]], 0, shape[0])
    return b


_ZERO4 = (0.0, 0.0, 0.0, 0.0)


def _sum(acc, items):
    return items if acc is None else acc + items


def _eval_forward(model, crit, data, fetch=True):
    """The prologue of every Val loop (Detector.cs:91-97): None for a batch with an empty batch_idx, else the eval forward and the criterion on the
    eval-mode preds -- one forward serves loss and post-process -- as (images, inference (None when not fetched), loss items)."""
    if np.asarray(data["batch_idx"]).size < 1:
        return None
    images = np.ascontiguousarray(data["images"], np.float32)
    model.eval()
    inference = model.forward(images, fetch=fetch)[0]
    return images, inference, crit.forward(None, data)[1]


def _gt_xyxy(bboxes, W, H):
    """Normalised cxcywh labels -> xyxy pixels (Detector.cs:110-112)."""
    gt = bboxes * np.array([W, H, W, H], np.float32)
    return np.concatenate((gt[:, :2] - gt[:, 2:] / 2, gt[:, :2] + gt[:, 2:] / 2), 1).astype(np.float32)


class _ValStats:
    """What a detection-style Val accumulates: the summed loss items and per image (tp per metric, conf, pred_cls, true_cls).  result() is Val's return
    value: (loss items, (P, R, mAP50, mAP50-95) per metric) from one ap_per_class per metric; zeros when no batch was taken."""

    def __init__(self, items, metrics):
        self.items, self.loss = items, None
        self.tps, self.cols = [[] for _ in range(metrics)], ([], [], [])

    def add_image(self, tps, rows, true_cls):
        for acc, v in zip(self.tps + list(self.cols), list(tps) + [rows[:, 4], rows[:, 5], true_cls]):
            acc.append(v)

    def result(self):
        if not self.tps[0]:
            return (np.zeros(self.items, np.float32),) + (_ZERO4,) * len(self.tps)
        conf, pc, tc = (np.concatenate(c) for c in self.cols)
        return (self.loss,) + tuple(M.val_summary(M.ap_per_class(np.concatenate(tp), conf, pc, tc)) for tp in self.tps)


class _DeviceMatch:
    """The device scratch of a device-resident Val loop and the calls on it, as a context manager: `cnt` [B], one `correct` [B, max_rows, 10] per metric
    and, when NMS produces the rows, `rows` [B, max_rows, row_len] and `keep` -- grown when a larger batch arrives, freed on every exit.
    select(B, bufs) fills bufs["cnt"] and returns the device pointer of the rows: ys_nms_batched into bufs["rows"], or ys_e2e_select(_ex) on the head's own
    rows.  match() runs it and then the per-image part as ONE launch (fn = ys_val_match_batched / _rotated_batched / _pose_batched, mid = its arguments
    between the row stride and the labels); only the rows, their counts and `correct` come back per batch."""

    def __init__(self, eng, select, fn, mid, row_len, max_rows, metrics=1, nms=False):
        self.eng, self.select, self.fn, self.mid, self.row_len, self.max_rows = eng, select, fn, mid, row_len, max_rows
        self.cor = ["cor%d" % i for i in range(metrics)]
        self.size = dict({"cnt": 4}, **{n: max_rows * 10 for n in self.cor})
        if nms:
            self.size.update(rows=max_rows * row_len * 4, keep=max_rows * 8)
        self.bufs, self.cap = {}, 0

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()

    def free(self):
        while self.bufs:
            self.eng.free(self.bufs.popitem()[1])
        self.cap = 0

    def match(self, B, labels, img_w, img_h):
        """-> (rows [count[b], row_len] per image, per metric the bool [count[b], 10] per image)"""
        eng, bufs, shape = self.eng, self.bufs, (B, self.max_rows, self.row_len)
        if B > self.cap:
            self.free()
            for n, per_image in self.size.items():
                bufs[n] = eng.malloc(B * per_image)
            self.cap = B
        d_rows = self.select(B, bufs)
        d_lab = []
        try:                       # the per-batch label buffers are released on the error paths too
            for a in labels:
                d_lab.append(eng.to_device(a))
            eng.val_match_call(self.fn, d_rows, bufs["cnt"], 1, shape, self.mid, labels, d_lab, img_w, img_h, [bufs[n] for n in self.cor])
            rows = eng.from_device(d_rows, shape, np.float32)
            cnt = eng.from_device(bufs["cnt"], (B,), np.int32)
            cors = [eng.from_device(bufs[n], shape[:2] + (10,), np.uint8) for n in self.cor]
        finally:
            for p_ in d_lab:
                eng.free(p_)
        return [rows[b, :cnt[b]] for b in range(B)], [[c[b, :cnt[b]].astype(bool) for b in range(B)] for c in cors]


class Detector:
    def __init__(self, model, end2end=None):
        """end2end (default: the model's own flag): Config.End2End (Config.cs:239) -- the model was built with end2end=True, predictions come
        from the head's own top-k rows and are only thresholded (Ops.cs:258-267), no NMS (Detector.cs:17-23, 44, 99)."""
        self.model, self.engine = model, model.engine
        self.amp = AMPWrapper(model)
        self.end2end = bool(getattr(model, "end2end", False)) if end2end is None else bool(end2end)
        if self.end2end and not getattr(model, "end2end", False):
            raise ValueError("Detector(end2end=True) needs a model created with end2end=True")

    def ImagePredict(self, image_chw_u8, predict_threshold=0.25, iou_threshold=0.5):
        """image: uint8 / float [3,H,W] in 0..255 (RGB).  Returns a list of YoloResult."""
        x = pad_to_32(np.asarray(image_chw_u8, np.float32))[None]
        assert x.shape[2:] == (self.model.height, self.model.width), "create the model with the padded image size"
        inference, _ = self.amp.Evaluate(x)
        output, _ = self.engine.non_max_suppression(inference["boxes"], predict_threshold, iou_threshold, end2end=self.end2end)
        return [YoloResult(r) for r in output[0]]

    # what a task supplies to the shared Val loop: the criterion, the item count of its loss, the number of metrics, the label layout, the NMS kind
    LOSS, ITEMS, METRICS, BOX_COLS, KPTS, ROTATED = "v8DetectionLoss", 3, 1, 4, False, False

    def Val(self, batches, conf_thres=0.1, iou_thres=0.7, max_det=300):
        """batches: iterable of dicts (images [B,3,H,W] in [0,1], batch_idx, cls, bboxes).  Returns
        (SUM over batches of the loss items, (P, R, mAP50, mAP50-95)) like Detector.Val (Detector.cs:76-154; :126 adds the items up).
        The predictions never leave the device between the eval forward, NMS and the matching (ys_model_pred_device ->
        ys_nms_batched -> ys_val_match_batched, all on device pointers); only the kept rows, their count and the `correct`
        matrix come back per batch, for the epoch-level ap_per_class on the host."""
        return self._val(batches, conf_thres, iou_thres, max_det)

    def _val(self, batches, conf_thres, iou_thres, max_det):
        """THE Val loop of the detection-style tasks: per batch the prologue, the rows and their per-image matching -- on the device (_device_match) or by
        the task's host per-image function (_match_image) -- into one _ValStats."""
        crit = getattr(_model, self.LOSS)(self.model)
        stats = _ValStats(self.ITEMS, self.METRICS)
        device = self._device_match(conf_thres, iou_thres, max_det)
        with device if device is not None else contextlib.nullcontext():
            for data in batches:
                step = _eval_forward(self.model, crit, data, fetch=device is None)
                if step is None:
                    continue
                images, inference, items = step
                stats.loss = _sum(stats.loss, items)
                B, _, H, W = images.shape
                labels = flatten_labels(data, self.BOX_COLS, self.model.kpt_num if self.KPTS else None, seen=device is None)
                if device is not None:
                    output, tps = device.match(B, labels, W, H)
                else:
                    output, _ = self.engine.non_max_suppression(inference["boxes"], conf_thres, iou_thres, max_det=max_det, nc=self.model.nc,
                                                                rotated=self.ROTATED, end2end=self.end2end)
                    ctx = self._batch_context(data, B)
                    tps = list(zip(*[self._match_image(rows, b, [a[labels[0] == b] for a in labels], W, H, ctx) for b, rows in enumerate(output)]))
                for b, rows in enumerate(output):
                    stats.add_image([tp[b] for tp in tps], rows, labels[1][labels[0] == b])
        return stats.result()

    def _batch_context(self, data, B):
        return None

    def _device_match(self, conf_thres, iou_thres, max_det):
        """The device-resident path (None: the host per-image path).  Detect takes it always: NMS on ys_model_pred_device, or the End2End rows."""
        eng, m = self.engine, self.model
        fn = eng.lib.ys_val_match_batched
        if self.end2end:
            return self._e2e_match(fn, (), 6 + m.NM, conf_thres, max_det)
        Cc = 4 + m.nc + m.NM

        def nms(B, bufs):
            eng.nms_device(m.pred_device(), B, Cc, m.A, conf_thres, iou_thres, max_det, m.nc, bufs["rows"], bufs["keep"], bufs["cnt"])
            return bufs["rows"]
        return _DeviceMatch(eng, nms, fn, (), 6 + m.NM, max_det, nms=True)

    def _e2e_match(self, fn, mid, row_len, conf_thres, max_det, metrics=1):
        """End2End: the rows are the head's own [B, k, row_len] (ys_model_det_device); the thresholding keeps a prefix of them (Ops.cs:258-267)."""
        eng = self.engine
        d_det, k = self.model.det_device()

        def select(B, bufs):
            if row_len == 6:
                _lib.check(eng.lib, eng.lib.ys_e2e_select(eng.ctx, d_det, 1, B, k, float(conf_thres), int(max_det), bufs["cnt"]))
            else:
                _lib.check(eng.lib, eng.lib.ys_e2e_select_ex(eng.ctx, d_det, 1, B, k, row_len, float(conf_thres), int(max_det), bufs["cnt"]))
            return d_det
        return _DeviceMatch(eng, select, fn, mid, row_len, k, metrics)


class Segmenter(Detector):
    """Models/Segmenter.cs:28-84: ImagePredict with instance masks -- eval forward (pred carries the 32 mask coefficients
    per anchor), NMS (the coefficients ride along as extra columns), Ops.process_mask on the device with upsample=True, boxes
    clipped to the original image and masks cropped to it (the padded region is bottom / right, so the resize of
    Segmenter.cs:56-57 is an identity crop here).  On an End2End model (model.e2e_init; Segmenter.cs:17-24, 44-57) the head's own top-k rows
    [B, k, 6+32] are only thresholded (Ops.cs:258-267, ys_e2e_select_ex) and the kept prefix feeds the same process_mask / mask_iou path."""

    def ImagePredict(self, image_chw_u8, predict_threshold=0.25, iou_threshold=0.5):
        img = np.asarray(image_chw_u8)
        h, w = img.shape[1:]
        self.model.eval()
        inference, preds = self.model.forward_u8(np.ascontiguousarray(img, np.uint8)[None])
        proto = self.model.get_output("proto")[0]
        output, _ = self.engine.non_max_suppression(inference["boxes"], predict_threshold, iou_threshold, nc=self.model.nc, end2end=self.end2end)
        rows = output[0]
        results = []
        if len(rows):
            masks = self.engine.process_mask(proto, rows[:, 6:], rows[:, :4], (self.model.height, self.model.width), upsample=True)
            rows[:, :4] = clip_boxes(rows[:, :4], (h, w))
            masks = masks[:, :h, :w]
            for r, mk in zip(rows, masks):
                res = YoloResult(r)
                results.append((res, mk))
        return results

    LOSS, ITEMS, METRICS = "v8SegmentationLoss", 5, 2

    def Val(self, batches, conf_thres=0.01, iou_thres=0.7, max_det=300):
        """Models/Segmenter.cs:85-185: per batch eval forward + loss, NMS (conf 0.01, IoU 0.7), and per image
        process_mask at the prototype resolution (:126 passes the proto size as `shape`, so the boxes are NOT rescaled -- kept),
        box IoU matching and mask IoU matching (Metrics.mask_iou on the overlap-encoded `masks`, :131-143) -- all on the device;
        the two epoch-level ap_per_class reductions stay on the host.  batches: dicts with images [B,3,H,W] in [0,1], batch_idx,
        cls, bboxes, masks [B,H/4,W/4].  Returns (summed loss items [5], box (P,R,mAP50,mAP50-95), mask (P,R,mAP50,mAP50-95))."""
        return self._val(batches, conf_thres, iou_thres, max_det)

    def _device_match(self, conf_thres, iou_thres, max_det):
        return None

    def _batch_context(self, data, B):
        proto = self.model.get_output("proto")
        return proto, np.asarray(data["masks"], np.float32).reshape((B,) + proto.shape[2:])

    def _match_image(self, rows, b, lab, W, H, ctx):
        eng, (_, cl, bb), (proto, gm) = self.engine, lab, ctx
        mh, mw = proto.shape[2:]
        masks = eng.process_mask(proto[b], rows[:, 6:], rows[:, :4], (mw, mh)) if len(rows) else np.zeros((0, mh, mw), bool)
        tp = eng.match_predictions(rows[:, 5], cl, eng.box_iou(_gt_xyxy(bb, W, H), rows[:, :4]))
        return tp, eng.match_predictions(rows[:, 5], cl, eng.mask_iou(gm[b], len(cl), masks))


class Obber(Detector):
    """Models/Obber.cs: ImagePredict (:28-68) = eval forward (pred = dist2rbox boxes, probabilities, angle) + rotated NMS, result =
    truncated centre / size + Radian; Val (:70-163) = eval forward + v8OBBLoss on the eval preds, rotated NMS (conf 0.01, IoU 0.7),
    Metrics.batch_probiou(labels xywh * scale + angle, predictions xywh + angle) -> match_predictions -> ap_per_class.
    On an End2End model (model.e2e_obb_init; Obber.cs:18-24) the head's own top-k rows [B, k, 7] are only thresholded (Ops.cs:258-267) and Val keeps
    them on the device: ys_model_det_device -> ys_e2e_select_ex -> ys_val_match_rotated_batched (one launch for the per-image part)."""

    def ImagePredict(self, image_chw_u8, predict_threshold=0.25, iou_threshold=0.5):
        x = pad_to_32(np.asarray(image_chw_u8, np.float32))[None]
        assert x.shape[2:] == (self.model.height, self.model.width), "create the model with the padded image size"
        inference, _ = self.amp.Evaluate(x)
        if self.end2end:
            output, _ = self.engine.non_max_suppression(inference["boxes"], predict_threshold, iou_threshold, nc=self.model.nc, end2end=True)
        else:
            output, _ = self.engine.non_max_suppression(inference["boxes"], predict_threshold, iou_threshold, nc=self.model.nc, rotated=True)
        results = []
        for r in output[0]:                                        # Obber.cs:55-63: the rotated rows stay xywh
            res = YoloResult.__new__(YoloResult)
            res.CenterX, res.CenterY, res.Width, res.Height = int(r[0]), int(r[1]), int(r[2]), int(r[3])
            res.Score, res.ClassID, res.Radian, res.KeyPoints = float(r[4]), int(r[5]), float(r[6]), None
            results.append(res)
        return results

    LOSS, ITEMS, BOX_COLS, ROTATED = "v8OBBLoss", 4, 5, True

    def Val(self, batches, conf_thres=0.01, iou_thres=0.7, max_det=300):
        return self._val(batches, conf_thres, iou_thres, max_det)

    def _device_match(self, conf_thres, iou_thres, max_det):
        if not self.end2end:
            return None
        return self._e2e_match(self.engine.lib.ys_val_match_rotated_batched, (6,), 7, conf_thres, max_det)      # E2EOBBLoss on the eval preds (Obber.cs:94-95)

    def _match_image(self, rows, b, lab, W, H, ctx):
        eng, (_, cl, bb) = self.engine, lab
        gt = np.concatenate((bb[:, :4] * np.array([W, H, W, H], np.float32), bb[:, 4:5]), 1).astype(np.float32)      # Obber.cs:108
        pred = np.concatenate((rows[:, :4], rows[:, 6:7]), 1).astype(np.float32)                                   # Obber.cs:102
        iou = eng.batch_probiou(gt, pred) if len(gt) and len(pred) else np.zeros((len(gt), len(pred)), np.float32)
        return (eng.match_predictions(rows[:, 5], cl, iou),)


class KeyPoint:
    __slots__ = ("X", "Y", "VisibilityScore")

    def __init__(self, x, y, v):
        self.X, self.Y, self.VisibilityScore = float(x), float(y), float(v)


class PoseDetector(Detector):
    """Models/PoseDetector.cs: ImagePredict (:39-98) = eval forward (pred carries the decoded keypoints) + NMS, result = the
    truncated box + KeyPoints (visibility 2.0 for 2-D keypoints); Val (:100-200) = eval forward + v8PoseLoss, NMS (conf 0.01, IoU
    0.7), box_iou matching and Metrics.kpt_iou (area = w * h * 0.53) matching -> ap_per_class twice.
    On an End2End model (model.e2e_pose_init; PoseDetector.cs:21-36, 57, 129) the head's own top-k rows [B, k, 6+nk] are only thresholded (Ops.cs:258-267)
    and Val keeps them on the device: ys_model_det_device -> ys_e2e_select_ex -> ys_val_match_pose_batched (one launch for the per-image part)."""

    def ImagePredict(self, image_chw_u8, predict_threshold=0.25, iou_threshold=0.5):
        x = pad_to_32(np.asarray(image_chw_u8, np.float32))[None]
        assert x.shape[2:] == (self.model.height, self.model.width), "create the model with the padded image size"
        inference, _ = self.amp.Evaluate(x)
        output, _ = self.engine.non_max_suppression(inference["boxes"], predict_threshold, iou_threshold, nc=self.model.nc, end2end=self.end2end)
        D = self.model.kpt_dim
        results = []
        for r in output[0]:
            res = YoloResult(r)
            kp = r[6:].reshape(-1, D)
            res.KeyPoints = [KeyPoint(k[0], k[1], k[2] if D == 3 else 2.0) for k in kp]
            results.append(res)
        return results

    LOSS, ITEMS, METRICS, KPTS = "v8PoseLoss", 5, 2, True

    def Val(self, batches, conf_thres=0.01, iou_thres=0.7, max_det=300):
        return self._val(batches, conf_thres, iou_thres, max_det)

    def _device_match(self, conf_thres, iou_thres, max_det):
        if not self.end2end:
            return None
        K, D = self.model.kpt_num, self.model.kpt_dim                 # E2EPoseLoss on the eval preds (PoseDetector.cs:123-124)
        return self._e2e_match(self.engine.lib.ys_val_match_pose_batched, (6, K, D), 6 + K * D, conf_thres, max_det, metrics=2)

    def _match_image(self, rows, b, lab, W, H, ctx):
        eng, (_, cl, bb, kp) = self.engine, lab
        gt_xyxy = _gt_xyxy(bb, W, H)
        tp = eng.match_predictions(rows[:, 5], cl, eng.box_iou(gt_xyxy, rows[:, :4]))
        gk = (kp * np.array([W, H, 1.0], np.float32)).astype(np.float32)                                         # PoseDetector.cs:153-155
        area = ((gt_xyxy[:, 2] - gt_xyxy[:, 0]) * (gt_xyxy[:, 3] - gt_xyxy[:, 1]) * np.float32(0.53)).astype(np.float32)
        oks = eng.kpt_iou(gk, rows[:, 6:].reshape(-1, self.model.kpt_num, self.model.kpt_dim), area)
        return tp, eng.match_predictions(rows[:, 5], cl, oks)


class ClassifyResult:
    """Types/YoloResult as Classifier.ImagePredict fills it (Classifier.cs:47-55): class id and score only."""
    __slots__ = ("ClassID", "Score")

    def __init__(self, cls_id, score):
        self.ClassID, self.Score = int(cls_id), float(score)

    def __repr__(self):
        return f"ClassifyResult(cls={self.ClassID}, score={self.Score:.4f})"


class Classifier:
    """Host mirror of Models/Classifier.cs on the engine: ImagePredict (:28-58) and Val (:61-120)."""

    def __init__(self, model):
        from .model import v8ClassificationLoss
        self.model, self.engine = model, model.engine
        self.amp = AMPWrapper(model)
        self.loss = v8ClassificationLoss(model)

    def ImagePredict(self, image_chw_u8, predict_threshold=0.25, iou_threshold=0.5):
        """image: uint8 / float [3,H,W] in 0..255.  Pad to a multiple of 32 with 114, / 255, eval forward; every class sorted by score
        (descending; the thresholds are unused, as in the reference)."""
        x = pad_to_32(np.asarray(image_chw_u8, np.float32))[None]
        assert x.shape[2:] == (self.model.height, self.model.width), "create the model with the padded image size"
        inference, _ = self.amp.Evaluate(x)
        p = inference["cls"][0]
        order = np.argsort(-p, kind="stable")                        # results.Sort by descending score (Classifier.cs:56)
        return [ClassifyResult(i, p[i]) for i in order]

    def Val(self, batches):
        """batches: iterable of dicts (images [B,3,H,W] in [0,1], batch_idx, cls [B]).  Returns (summed loss items [1], [top1, top5]):
        eval forward, the criterion on the eval logits, the top-min(nc, 5) classes of the softmax per image (ys_cls_topk), then top-1 /
        top-5 accuracy over the set.  Batches with an empty batch_idx are skipped (Classifier.cs:83-86).  A batch may also be an
        augment.ClassifyDeviceBatch (ClassifyAugmenter.val_batches): the eval forward runs from its device pointer and the criterion on its device labels."""
        from .augment import ClassifyDeviceBatch
        loss_sum, tops, targets = None, [], []
        k = min(self.model.nc, 5)
        for data in batches:
            if isinstance(data, ClassifyDeviceBatch):                # images and class ids already in HBM (ClassifyAugmenter.val_batches)
                m = self.model
                assert data.imgsz == m.height == m.width, (data.imgsz, m.height, m.width)
                m.eval()
                m.forward_device(data.images, data.batch)
                inference, _ = m._outputs()
                self.loss.forward_device(data.cls, data.batch)
                loss_sum = _sum(loss_sum, self.loss.read()[1])
                tops.append(self.engine.cls_topk(inference["cls"], k))
                targets.append(self.engine.from_device(data.cls, (data.batch,), np.float32))
                continue
            step = _eval_forward(self.model, self.loss, data)
            if step is None:
                continue
            _, inference, items = step
            loss_sum = _sum(loss_sum, items)
            tops.append(self.engine.cls_topk(inference["cls"], k))
            targets.append(np.asarray(data["cls"], np.float32).reshape(-1))
        if not tops:
            return np.zeros(1, np.float32), [0.0, 0.0]
        pred, tgt = np.concatenate(tops), np.concatenate(targets)
        correct = (tgt[:, None] == pred).astype(np.float32)
        return loss_sum, [float(correct[:, 0].mean()), float(correct.max(1).mean())]
