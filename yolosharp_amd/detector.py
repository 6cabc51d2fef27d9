"""Host mirror of Models/Detector.cs on the engine: ImagePredict (:26-72) and Val (:76-154).

Everything per image / per anchor runs on the device (eval forward + decode, NMS, box_iou + match_predictions); only the
epoch-level ap_per_class (small) and the reference's integer truncation of the results stay on the host.  The model must have
been created with (height, width) = the padded image size: the reference pads bottom/right with 114 to a multiple of 32
before dividing by 255 (Detector.cs:35-41), this does the same."""
import numpy as np

from . import _lib
from . import metrics as M
from .model import AMPWrapper, v8DetectionLoss


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

    def Val(self, batches, conf_thres=0.1, iou_thres=0.7, max_det=300):
        """batches: iterable of dicts (images [B,3,H,W] in [0,1], batch_idx, cls, bboxes).  Returns
        (SUM over batches of the loss items, (P, R, mAP50, mAP50-95)) like Detector.Val (Detector.cs:76-154; :126 adds the items up).
        The predictions never leave the device between the eval forward, NMS and the matching (ys_model_pred_device ->
        ys_nms_batched -> ys_val_match_batched, all on device pointers); only the kept rows, their count and the `correct`
        matrix come back per batch, for the epoch-level ap_per_class on the host."""
        crit = v8DetectionLoss(self.model)
        eng, m = self.engine, self.model
        tps, confs, pcls, tcls = [], [], [], []
        loss_sum, count = None, 0
        nc = m.nc
        Cc = 4 + nc + m.NM
        stride = Cc - nc + 2
        if self.end2end:          # the rows are the head's own [B, k, 6] (ys_model_det_device); the thresholding keeps a prefix of them
            d_det, max_rows = m.det_device()
        else:
            max_rows = max_det
        d_rows = d_keep = d_cnt = d_cor = None
        cap_b = 0
        try:
            for data in batches:
                if np.asarray(data["batch_idx"]).size < 1:          # Detector.cs:91-94
                    continue
                images = np.ascontiguousarray(data["images"], np.float32)
                B = images.shape[0]
                # eval forward, then the criterion on the eval-mode preds (Detector.cs:95-97): one forward serves loss and NMS
                m.eval()
                m.forward(images, fetch=False)
                _, items = crit.forward(None, data)
                loss_sum = items if loss_sum is None else loss_sum + items
                if B > cap_b:
                    for p_ in (d_rows, d_keep, d_cnt, d_cor):
                        if p_ is not None:
                            eng.free(p_)
                    if not self.end2end:
                        d_rows, d_keep = eng.malloc(B * max_det * stride * 4), eng.malloc(B * max_det * 8)
                    d_cnt, d_cor = eng.malloc(B * 4), eng.malloc(B * max_rows * 10)
                    cap_b = B
                if self.end2end:
                    _lib.check(eng.lib, eng.lib.ys_e2e_select(eng.ctx, d_det, 1, B, max_rows, float(conf_thres), int(max_det), d_cnt))
                    rows_dev = d_det
                else:
                    eng.nms_device(m.pred_device(), B, Cc, m.A, conf_thres, iou_thres, max_det, nc, d_rows, d_keep, d_cnt)
                    rows_dev = d_rows
                bi = np.ascontiguousarray(np.asarray(data["batch_idx"], np.float32).reshape(-1))
                cl = np.ascontiguousarray(np.asarray(data["cls"], np.float32).reshape(-1))
                bb = np.ascontiguousarray(np.asarray(data["bboxes"], np.float32).reshape(-1, 4))
                d_lab = []
                try:                       # the per-batch label buffers are released on the error paths too
                    for a in (bi, cl, bb):
                        d_lab.append(eng.to_device(a))
                    _lib.check(eng.lib, eng.lib.ys_val_match_batched(eng.ctx, rows_dev, d_cnt, 1, B, max_rows, stride, d_lab[0], d_lab[1], d_lab[2],
                                                                     bi.shape[0], float(images.shape[3]), float(images.shape[2]), d_cor))
                    rows = eng.from_device(rows_dev, (B, max_rows, stride), np.float32)
                    cnt = eng.from_device(d_cnt, (B,), np.int32)
                    cor = eng.from_device(d_cor, (B, max_rows, 10), np.uint8)
                finally:
                    for p_ in d_lab:
                        eng.free(p_)
                for b in range(B):
                    tps.append(cor[b, :cnt[b]].astype(bool)); confs.append(rows[b, :cnt[b], 4]); pcls.append(rows[b, :cnt[b], 5])
                    tcls.append(cl[bi == b])
                count += B
        finally:
            for p_ in (d_rows, d_keep, d_cnt, d_cor):
                if p_ is not None:
                    eng.free(p_)
        if not tps:
            return np.zeros(3, np.float32), (0.0, 0.0, 0.0, 0.0)
        stats = M.ap_per_class(np.concatenate(tps), np.concatenate(confs), np.concatenate(pcls), np.concatenate(tcls))
        return loss_sum, M.val_summary(stats)


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

    def Val(self, batches, conf_thres=0.01, iou_thres=0.7, max_det=300):
        """Models/Segmenter.cs:85-185: per batch eval forward + loss, NMS (conf 0.01, IoU 0.7), and per image
        process_mask at the prototype resolution (:126 passes the proto size as `shape`, so the boxes are NOT rescaled -- kept),
        box IoU matching and mask IoU matching (Metrics.mask_iou on the overlap-encoded `masks`, :131-143) -- all on the device;
        the two epoch-level ap_per_class reductions stay on the host.  batches: dicts with images [B,3,H,W] in [0,1], batch_idx,
        cls, bboxes, masks [B,H/4,W/4].  Returns (summed loss items [5], box (P,R,mAP50,mAP50-95), mask (P,R,mAP50,mAP50-95))."""
        from .model import v8SegmentationLoss
        crit = v8SegmentationLoss(self.model)
        tps, tpms, confs, pcls, tcls = [], [], [], [], []
        loss_sum = None
        nc = self.model.nc
        for data in batches:
            if np.asarray(data["batch_idx"]).size < 1:          # Segmenter.cs:105-108
                continue
            images = np.ascontiguousarray(data["images"], np.float32)
            B, _, H, W = images.shape
            inference, _ = self.amp.Evaluate(images)                # Segmenter.cs:110-112: eval preds feed loss and NMS
            _, items = crit.forward(None, data)
            loss_sum = items if loss_sum is None else loss_sum + items
            proto = self.model.get_output("proto")
            mh, mw = proto.shape[2:]
            output, _ = self.engine.non_max_suppression(inference["boxes"], conf_thres, iou_thres, max_det=max_det, nc=nc, end2end=self.end2end)
            bi = np.asarray(data["batch_idx"], np.float32).reshape(-1)
            cl = np.asarray(data["cls"], np.float32).reshape(-1)
            bb = np.asarray(data["bboxes"], np.float32).reshape(-1, 4)
            gm = np.asarray(data["masks"], np.float32).reshape(B, mh, mw)
            for b, rows in enumerate(output):
                sel = bi == b
                true_cls = cl[sel]
                nl = int(sel.sum())
                masks = self.engine.process_mask(proto[b], rows[:, 6:], rows[:, :4], (mw, mh)) if len(rows) else np.zeros((0, mh, mw), bool)
                gt = bb[sel] * np.array([W, H, W, H], np.float32)
                gt_xyxy = np.concatenate((gt[:, :2] - gt[:, 2:] / 2, gt[:, :2] + gt[:, 2:] / 2), 1).astype(np.float32)
                iou = self.engine.box_iou(gt_xyxy, rows[:, :4])
                tps.append(self.engine.match_predictions(rows[:, 5], true_cls, iou))
                miou = self.engine.mask_iou(gm[b], nl, masks)
                tpms.append(self.engine.match_predictions(rows[:, 5], true_cls, miou))
                confs.append(rows[:, 4]); pcls.append(rows[:, 5]); tcls.append(true_cls)
        conf, pc, tc = np.concatenate(confs), np.concatenate(pcls), np.concatenate(tcls)
        box = M.val_summary(M.ap_per_class(np.concatenate(tps), conf, pc, tc))
        mask = M.val_summary(M.ap_per_class(np.concatenate(tpms), conf, pc, tc))
        return loss_sum, box, mask


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

    def Val(self, batches, conf_thres=0.01, iou_thres=0.7, max_det=300):
        from .model import v8OBBLoss
        if self.end2end:
            return self._val_end2end(batches, conf_thres, max_det)
        crit = v8OBBLoss(self.model)
        tps, confs, pcls, tcls = [], [], [], []
        loss_sum = None
        nc = self.model.nc
        for data in batches:
            if np.asarray(data["batch_idx"]).size < 1:
                continue
            images = np.ascontiguousarray(data["images"], np.float32)
            B, _, H, W = images.shape
            inference, _ = self.amp.Evaluate(images)
            _, items = crit.forward(None, data)
            loss_sum = items if loss_sum is None else loss_sum + items
            output, _ = self.engine.non_max_suppression(inference["boxes"], conf_thres, iou_thres, max_det=max_det, nc=nc, rotated=True)
            bi = np.asarray(data["batch_idx"], np.float32).reshape(-1)
            cl = np.asarray(data["cls"], np.float32).reshape(-1)
            bb = np.asarray(data["bboxes"], np.float32).reshape(-1, 5)
            for b, rows in enumerate(output):
                sel = bi == b
                gt = np.concatenate((bb[sel, :4] * np.array([W, H, W, H], np.float32), bb[sel, 4:5]), 1).astype(np.float32)   # Obber.cs:108
                pred = np.concatenate((rows[:, :4], rows[:, 6:7]), 1).astype(np.float32)                                      # Obber.cs:102
                iou = self.engine.batch_probiou(gt, pred) if len(gt) and len(pred) else np.zeros((len(gt), len(pred)), np.float32)
                tps.append(self.engine.match_predictions(rows[:, 5], cl[sel], iou))
                confs.append(rows[:, 4]); pcls.append(rows[:, 5]); tcls.append(cl[sel])
        if not tps:
            return np.zeros(4, np.float32), (0.0, 0.0, 0.0, 0.0)
        stats = M.ap_per_class(np.concatenate(tps), np.concatenate(confs), np.concatenate(pcls), np.concatenate(tcls))
        return loss_sum, M.val_summary(stats)

    def _val_end2end(self, batches, conf_thres, max_det):
        """Val on an End2End model: the rows are the head's own [B, k, 7] (ys_model_det_device); thresholding keeps a prefix of them and the per-image
        probiou + match_predictions run as one launch on the device pointers.  Only rows, counts and `correct` come back per batch."""
        from .model import v8OBBLoss
        crit = v8OBBLoss(self.model)
        eng, m = self.engine, self.model
        tps, confs, pcls, tcls = [], [], [], []
        loss_sum = None
        d_det, k = m.det_device()
        d_cnt = d_cor = None
        cap_b = 0
        try:
            for data in batches:
                if np.asarray(data["batch_idx"]).size < 1:
                    continue
                images = np.ascontiguousarray(data["images"], np.float32)
                B, _, H, W = images.shape
                m.eval()
                m.forward(images, fetch=False)
                _, items = crit.forward(None, data)                 # Obber.cs:94-95: E2EOBBLoss on the eval preds
                loss_sum = items if loss_sum is None else loss_sum + items
                if B > cap_b:
                    for p_ in (d_cnt, d_cor):
                        if p_ is not None:
                            eng.free(p_)
                    d_cnt = d_cor = None
                    d_cnt, d_cor = eng.malloc(B * 4), eng.malloc(B * k * 10)
                    cap_b = B
                _lib.check(eng.lib, eng.lib.ys_e2e_select_ex(eng.ctx, d_det, 1, B, k, 7, float(conf_thres), int(max_det), d_cnt))
                bi = np.ascontiguousarray(np.asarray(data["batch_idx"], np.float32).reshape(-1))
                cl = np.ascontiguousarray(np.asarray(data["cls"], np.float32).reshape(-1))
                bb = np.ascontiguousarray(np.asarray(data["bboxes"], np.float32).reshape(-1, 5))
                d_lab = []
                try:
                    for a in (bi, cl, bb):
                        d_lab.append(eng.to_device(a))
                    _lib.check(eng.lib, eng.lib.ys_val_match_rotated_batched(eng.ctx, d_det, d_cnt, 1, B, k, 7, 6, d_lab[0], d_lab[1], d_lab[2],
                                                                             bi.shape[0], float(W), float(H), d_cor))
                    rows = eng.from_device(d_det, (B, k, 7), np.float32)
                    cnt = eng.from_device(d_cnt, (B,), np.int32)
                    cor = eng.from_device(d_cor, (B, k, 10), np.uint8)
                finally:
                    for p_ in d_lab:
                        eng.free(p_)
                for b in range(B):
                    tps.append(cor[b, :cnt[b]].astype(bool)); confs.append(rows[b, :cnt[b], 4]); pcls.append(rows[b, :cnt[b], 5])
                    tcls.append(cl[bi == b])
        finally:
            for p_ in (d_cnt, d_cor):
                if p_ is not None:
                    eng.free(p_)
        if not tps:
            return np.zeros(4, np.float32), (0.0, 0.0, 0.0, 0.0)
        stats = M.ap_per_class(np.concatenate(tps), np.concatenate(confs), np.concatenate(pcls), np.concatenate(tcls))
        return loss_sum, M.val_summary(stats)


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

    def Val(self, batches, conf_thres=0.01, iou_thres=0.7, max_det=300):
        from .model import v8PoseLoss
        if self.end2end:
            return self._val_end2end(batches, conf_thres, max_det)
        crit = v8PoseLoss(self.model)
        tps, tpps, confs, pcls, tcls = [], [], [], [], []
        loss_sum = None
        nc, K, D = self.model.nc, self.model.kpt_num, self.model.kpt_dim
        for data in batches:
            if np.asarray(data["batch_idx"]).size < 1:
                continue
            images = np.ascontiguousarray(data["images"], np.float32)
            B, _, H, W = images.shape
            inference, _ = self.amp.Evaluate(images)
            _, items = crit.forward(None, data)
            loss_sum = items if loss_sum is None else loss_sum + items
            output, _ = self.engine.non_max_suppression(inference["boxes"], conf_thres, iou_thres, max_det=max_det, nc=nc)
            bi = np.asarray(data["batch_idx"], np.float32).reshape(-1)
            cl = np.asarray(data["cls"], np.float32).reshape(-1)
            bb = np.asarray(data["bboxes"], np.float32).reshape(-1, 4)
            kp = np.asarray(data["keypoints"], np.float32).reshape(len(bi), K, -1)
            if kp.shape[2] == 2:                                   # PoseDetector.cs:144-148: "seen" column of ones
                kp = np.concatenate((kp, np.ones(kp.shape[:2] + (1,), np.float32)), 2)
            for b, rows in enumerate(output):
                sel = bi == b
                gt = bb[sel] * np.array([W, H, W, H], np.float32)
                gt_xyxy = np.concatenate((gt[:, :2] - gt[:, 2:] / 2, gt[:, :2] + gt[:, 2:] / 2), 1).astype(np.float32)
                tps.append(self.engine.match_predictions(rows[:, 5], cl[sel], self.engine.box_iou(gt_xyxy, rows[:, :4])))
                gk = (kp[sel] * np.array([W, H, 1.0], np.float32)).astype(np.float32)                       # PoseDetector.cs:153-155
                area = ((gt_xyxy[:, 2] - gt_xyxy[:, 0]) * (gt_xyxy[:, 3] - gt_xyxy[:, 1]) * np.float32(0.53)).astype(np.float32)
                oks = self.engine.kpt_iou(gk, rows[:, 6:].reshape(-1, K, D), area)
                tpps.append(self.engine.match_predictions(rows[:, 5], cl[sel], oks))
                confs.append(rows[:, 4]); pcls.append(rows[:, 5]); tcls.append(cl[sel])
        if not tps:
            return np.zeros(5, np.float32), (0.0, 0.0, 0.0, 0.0), (0.0, 0.0, 0.0, 0.0)
        conf, pc, tc = np.concatenate(confs), np.concatenate(pcls), np.concatenate(tcls)
        box = M.val_summary(M.ap_per_class(np.concatenate(tps), conf, pc, tc))
        pose = M.val_summary(M.ap_per_class(np.concatenate(tpps), conf, pc, tc))
        return loss_sum, box, pose

    def _val_end2end(self, batches, conf_thres, max_det):
        """Val on an End2End model: the rows are the head's own [B, k, 6+nk] (ys_model_det_device); thresholding keeps a prefix of them and the per-image
        box_iou / kpt_iou + two match_predictions run as one launch on the device pointers.  Only rows, counts and the two `correct` arrays come back per batch."""
        from .model import v8PoseLoss
        crit = v8PoseLoss(self.model)
        eng, m = self.engine, self.model
        K, D = m.kpt_num, m.kpt_dim
        rl = 6 + K * D
        tps, tpps, confs, pcls, tcls = [], [], [], [], []
        loss_sum = None
        d_det, k = m.det_device()
        d_cnt = d_cob = d_cop = None
        cap_b = 0
        try:
            for data in batches:
                if np.asarray(data["batch_idx"]).size < 1:
                    continue
                images = np.ascontiguousarray(data["images"], np.float32)
                B, _, H, W = images.shape
                m.eval()
                m.forward(images, fetch=False)
                _, items = crit.forward(None, data)                 # PoseDetector.cs:123-124: E2EPoseLoss on the eval preds
                loss_sum = items if loss_sum is None else loss_sum + items
                if B > cap_b:
                    for p_ in (d_cnt, d_cob, d_cop):
                        if p_ is not None:
                            eng.free(p_)
                    d_cnt = d_cob = d_cop = None
                    d_cnt, d_cob, d_cop = eng.malloc(B * 4), eng.malloc(B * k * 10), eng.malloc(B * k * 10)
                    cap_b = B
                _lib.check(eng.lib, eng.lib.ys_e2e_select_ex(eng.ctx, d_det, 1, B, k, rl, float(conf_thres), int(max_det), d_cnt))
                bi = np.ascontiguousarray(np.asarray(data["batch_idx"], np.float32).reshape(-1))
                cl = np.ascontiguousarray(np.asarray(data["cls"], np.float32).reshape(-1))
                bb = np.ascontiguousarray(np.asarray(data["bboxes"], np.float32).reshape(-1, 4))
                kp = np.ascontiguousarray(np.asarray(data["keypoints"], np.float32).reshape(len(bi), K, -1))
                d_lab = []
                try:
                    for a in (bi, cl, bb, kp):
                        d_lab.append(eng.to_device(a))
                    _lib.check(eng.lib, eng.lib.ys_val_match_pose_batched(eng.ctx, d_det, d_cnt, 1, B, k, rl, 6, K, D, d_lab[0], d_lab[1], d_lab[2], d_lab[3],
                                                                          kp.shape[2], bi.shape[0], float(W), float(H), d_cob, d_cop))
                    rows = eng.from_device(d_det, (B, k, rl), np.float32)
                    cnt = eng.from_device(d_cnt, (B,), np.int32)
                    cob = eng.from_device(d_cob, (B, k, 10), np.uint8)
                    cop = eng.from_device(d_cop, (B, k, 10), np.uint8)
                finally:
                    for p_ in d_lab:
                        eng.free(p_)
                for b in range(B):
                    tps.append(cob[b, :cnt[b]].astype(bool)); tpps.append(cop[b, :cnt[b]].astype(bool))
                    confs.append(rows[b, :cnt[b], 4]); pcls.append(rows[b, :cnt[b], 5]); tcls.append(cl[bi == b])
        finally:
            for p_ in (d_cnt, d_cob, d_cop):
                if p_ is not None:
                    eng.free(p_)
        if not tps:
            return np.zeros(5, np.float32), (0.0, 0.0, 0.0, 0.0), (0.0, 0.0, 0.0, 0.0)
        conf, pc, tc = np.concatenate(confs), np.concatenate(pcls), np.concatenate(tcls)
        box = M.val_summary(M.ap_per_class(np.concatenate(tps), conf, pc, tc))
        pose = M.val_summary(M.ap_per_class(np.concatenate(tpps), conf, pc, tc))
        return loss_sum, box, pose


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
                _, items = self.loss.read()
                loss_sum = items if loss_sum is None else loss_sum + items
                tops.append(self.engine.cls_topk(inference["cls"], k))
                targets.append(self.engine.from_device(data.cls, (data.batch,), np.float32))
                continue
            if np.asarray(data["batch_idx"]).size < 1:
                continue
            inference, _ = self.amp.Evaluate(np.ascontiguousarray(data["images"], np.float32))
            _, items = self.loss.forward(None, data)
            loss_sum = items if loss_sum is None else loss_sum + items
            tops.append(self.engine.cls_topk(inference["cls"], k))
            targets.append(np.asarray(data["cls"], np.float32).reshape(-1))
        if not tops:
            return np.zeros(1, np.float32), [0.0, 0.0]
        pred, tgt = np.concatenate(tops), np.concatenate(targets)
        correct = (tgt[:, None] == pred).astype(np.float32)
        return loss_sum, [float(correct[:, 0].mean()), float(correct.max(1).mean())]
