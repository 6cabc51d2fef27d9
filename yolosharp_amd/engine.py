"""Host-side mirror of the reference's operator surface over the C ABI (include/yolosharp_hip.h).

The reference is C# (TorchSharp); there is no dotnet toolchain in the build image, so the host side
is written in Python with the reference's names and argument meaning:

  Ops.non_max_suppression  <- YoloSharp/Utils/Ops.cs:239-371
  Convs.Conv.forward       <- YoloSharp/Modules/Convs.cs:36-62
  Yolov8 / v8DetectionLoss / AMPWrapper.TrainStep  (see model.py)

Everything numeric runs in libyolosharp_hip.so (hand-written HIP, gfx950).  numpy arrays cross the
boundary as plain fp32 host pointers; torch is not involved in the data path.
"""
import ctypes as C
import sys
import numpy as np

from . import _lib


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def flatten_labels(batch, box_cols=4, kpt_num=None, seen=False):
    """A collate dict's labels as contiguous fp32 arrays: (batch_idx [N], cls [N], bboxes [N, box_cols]) and, with kpt_num, keypoints [N, K, 2|3];
    seen: 2-column keypoints get the "seen" column of ones (PoseDetector.cs:144-148), which the device kernel appends itself."""
    def flat(key, *shape):
        return np.ascontiguousarray(np.asarray(batch[key], np.float32).reshape(shape))
    labels = flat("batch_idx", -1), flat("cls", -1), flat("bboxes", -1, box_cols)
    if kpt_num is None:
        return labels
    kp = flat("keypoints", labels[0].shape[0], int(kpt_num), -1)
    if seen and kp.shape[2] == 2:
        kp = np.concatenate((kp, np.ones(kp.shape[:2] + (1,), np.float32)), 2)
    return labels + (kp,)


_DTYPE_CODES = {"f32": 0, "float32": 0, "bf16": 1, "bfloat16": 1, "fp8": 2, "float8": 2, 0: 0, 1: 1, 2: 2}   # same names as model.DTYPES


def _dtype_code(dtype):
    try:
        return _DTYPE_CODES[dtype]
    except (KeyError, TypeError):
        raise ValueError("dtype %r: expected one of f32/float32, bf16/bfloat16, fp8/float8 (or the codes 0, 1, 2)" % (dtype,))


class Engine:
    """One device context (ys_ctx): owns a HIP stream; not thread-safe (callers serialise)."""

    def __init__(self, device=0, lib_path=None, stream=None):
        self.lib = _lib.load(lib_path)
        self.ctx = C.c_void_p()
        if stream is None:
            _lib.check(self.lib, self.lib.ys_ctx_create(device, C.byref(self.ctx)))
        else:
            _lib.check(self.lib, self.lib.ys_ctx_create_on_stream(device, C.c_void_p(stream), C.byref(self.ctx)))
        self.device = device
        self.stream = stream          # the caller's HIP stream the context runs on (None: a stream the library created for itself)

    def close(self):
        if self.ctx:
            self.lib.ys_ctx_destroy(self.ctx)
            self.ctx = C.c_void_p()

    def __del__(self):
        if sys is None or sys.is_finalizing():      # interpreter teardown: the HIP runtime may already be gone and destruction order is arbitrary
            return
        try:
            self.close()
        except Exception:
            pass

    @property
    def is_device_build(self):
        return bool(self.lib.ys_is_device_build())

    def synchronize(self):
        _lib.check(self.lib, self.lib.ys_ctx_synchronize(self.ctx))

    def profile(self, enable=True):
        _lib.check(self.lib, self.lib.ys_ctx_profile_enable(self.ctx, int(enable)))

    def last_ms(self, name):
        ms = C.c_float()
        _lib.check(self.lib, self.lib.ys_ctx_last_ms(self.ctx, name.encode(), C.byref(ms)))
        return ms.value

    def kernel_profile(self, enable=True):
        _lib.check(self.lib, self.lib.ys_ctx_kernel_profile(self.ctx, int(enable)))

    def kernel_profile_read(self, name):
        n, ms = C.c_int32(), C.c_float()
        _lib.check(self.lib, self.lib.ys_ctx_kernel_profile_read(self.ctx, name.encode(), C.byref(n), C.byref(ms)))
        return n.value, ms.value

    def kernel_profile_dump(self, path):
        _lib.check(self.lib, self.lib.ys_ctx_kernel_profile_dump(self.ctx, str(path).encode()))

    # ---- device memory helpers (bench keeps inputs resident in HBM)
    def malloc(self, nbytes):
        p = C.c_void_p()
        _lib.check(self.lib, self.lib.ys_device_malloc(self.ctx, nbytes, C.byref(p)))
        return p

    def free(self, p):
        _lib.check(self.lib, self.lib.ys_device_free(self.ctx, p))

    def to_device(self, arr):
        arr = np.ascontiguousarray(arr)
        p = self.malloc(arr.nbytes)
        _lib.check(self.lib, self.lib.ys_memcpy_h2d(self.ctx, p, _ptr(arr), arr.nbytes))
        return p

    def from_device(self, p, shape, dtype):
        out = np.empty(shape, dtype)
        _lib.check(self.lib, self.lib.ys_memcpy_d2h(self.ctx, _ptr(out), p, out.nbytes))
        return out

    # ---- tuning / routing options of the library (process-wide; include/yolosharp_hip.h ys_set_option)
    def set_option(self, key, value):
        _lib.check(self.lib, self.lib.ys_set_option(str(key).encode(), float(value)))

    def unset_option(self, key):
        _lib.check(self.lib, self.lib.ys_unset_option(str(key).encode()))

    def get_option(self, key):
        """The table's entry for `key` (None = not set: the built-in default applies)."""
        v, s = C.c_double(), C.c_int()
        _lib.check(self.lib, self.lib.ys_get_option(str(key).encode(), C.byref(v), C.byref(s)))
        return float(v.value) if s.value else None

    def options(self, **kw):
        """Context manager: set the options for the body, then put back what was there before -- a value set earlier or seeded from the environment at load
        (tests/conftest.py lowers size gates that way), or nothing (tests: `with engine.options(BNRED=0): ...`)."""
        import contextlib

        @contextlib.contextmanager
        def cm():
            old = {k: self.get_option(k) for k in kw}
            for k, v in kw.items():
                self.set_option(k, v)
            try:
                yield self
            finally:
                for k, v in old.items():
                    if v is None:
                        self.unset_option(k)
                    else:
                        self.set_option(k, v)
        return cm()

    # ---- data-parallel exchange through the C ABI (RCCL inside the library; bench.py uses torch.distributed instead)
    def dist_unique_id(self):
        buf = (C.c_ubyte * 128)()
        _lib.check(self.lib, self.lib.ys_dist_unique_id(buf))
        return bytes(buf)

    def dist_init(self, rank, world, unique_id):
        buf = (C.c_ubyte * 128).from_buffer_copy(unique_id)
        _lib.check(self.lib, self.lib.ys_dist_init(self.ctx, rank, world, buf))

    def dist_destroy(self):
        _lib.check(self.lib, self.lib.ys_dist_destroy(self.ctx))

    def cls_topk(self, scores, k=5):
        """Classifier.Val's argsort(1, descending)[:, :k] (Classifier.cs:95-100) on the device: scores [rows, cols] fp32 -> int32 [rows, k];
        ties go to the lower index."""
        x = np.ascontiguousarray(scores, np.float32)
        rows, cols = x.shape
        out = np.zeros((rows, k), np.int32)
        _lib.check(self.lib, self.lib.ys_cls_topk(self.ctx, _ptr(x), 0, rows, cols, k, _ptr(out)))
        return out

    # ---- End2End post-process (Head.cs:117-127, 175-196; Ops.cs:258-267)
    def e2e_topk(self, pred, max_det=300, extra=0):
        """Detect.postprocess on pred [B, 4+nc+extra, A] fp32: (rows [B, k, 6+extra] = (box, score, class, the anchor's `extra` trailing channels)
        ordered by score, anchor [B, k] int64), k = min(max_det, A); equal scores keep the lower index first (include/yolosharp_hip.h ys_e2e_topk /
        ys_e2e_topk_ex).  extra = nm is Segment.postprocess (Head.cs:321-339)."""
        p = np.ascontiguousarray(pred, np.float32)
        B, Cc, A = p.shape
        extra = int(extra)
        k = min(int(max_det), A)
        rows = np.zeros((B, k, 6 + extra), np.float32)
        anchor = np.zeros((B, k), np.int64)
        if extra:
            _lib.check(self.lib, self.lib.ys_e2e_topk_ex(self.ctx, _ptr(p), 0, B, Cc - 4 - extra, extra, A, int(max_det), _ptr(rows), _ptr(anchor)))
        else:
            _lib.check(self.lib, self.lib.ys_e2e_topk(self.ctx, _ptr(p), 0, B, Cc - 4, A, int(max_det), _ptr(rows), _ptr(anchor)))
        return rows, anchor

    def e2e_select(self, rows, conf_thres=0.25, max_det=300):
        """non_max_suppression(end2end: true): the number of leading rows of rows [B, k, 6 (+ extra)] with score > conf_thres, at most max_det -> int32 [B]."""
        r = np.ascontiguousarray(rows, np.float32)
        B, k, rl = r.shape
        assert rl >= 6, r.shape
        cnt = np.zeros((B,), np.int32)
        if rl == 6:
            _lib.check(self.lib, self.lib.ys_e2e_select(self.ctx, _ptr(r), 0, B, k, float(conf_thres), int(max_det), _ptr(cnt)))
        else:
            _lib.check(self.lib, self.lib.ys_e2e_select_ex(self.ctx, _ptr(r), 0, B, k, rl, float(conf_thres), int(max_det), _ptr(cnt)))
        return cnt

    def tal_keep_best(self, align, mask_pos, gt_count):
        """The assigner's second stage (tal_topk2 = 1, Tal.cs:242-250) on align [B, G, A] fp32, mask_pos [B, G, A] (bool / uint8), gt_count [B]: the
        pruned mask as uint8 -- every row below gt_count[b] keeps only the first anchor in (align * mask_pos descending, index ascending) order."""
        al = np.ascontiguousarray(align, np.float32)
        mp = np.ascontiguousarray(np.asarray(mask_pos).astype(np.uint8))
        gc = np.ascontiguousarray(gt_count, np.int32)
        B, G, A = al.shape
        assert mp.shape == al.shape and gc.shape == (B,), (mp.shape, gc.shape)
        _lib.check(self.lib, self.lib.ys_tal_keep_best(self.ctx, _ptr(al), _ptr(mp), _ptr(gc), 0, B, G, A))
        return mp

    # ---- validation (Detector.cs:103-120): box_iou + match_predictions per image, batched on the device
    def box_iou(self, box1, box2, eps=1e-7):
        """Metrics.box_iou (Metrics.cs:16-34): xyxy [n,4] x [m,4] -> [n,m] fp32."""
        b1 = np.ascontiguousarray(box1, np.float32).reshape(-1, 4)
        b2 = np.ascontiguousarray(box2, np.float32).reshape(-1, 4)
        out = np.zeros((b1.shape[0], b2.shape[0]), np.float32)
        _lib.check(self.lib, self.lib.ys_box_iou(self.ctx, _ptr(b1), b1.shape[0], _ptr(b2), b2.shape[0], eps, 0, _ptr(out)))
        return out

    def kpt_iou(self, kpt1, kpt2, area, eps=1e-7):
        """Metrics.kpt_iou (Metrics.cs:186-212): gt keypoints [n,K,3] x predicted keypoints [m,K,D], area [n] -> OKS [n,m] fp32."""
        k1 = np.ascontiguousarray(kpt1, np.float32)
        k2 = np.ascontiguousarray(kpt2, np.float32)
        ar = np.ascontiguousarray(area, np.float32).reshape(-1)
        n, K = k1.shape[0], k1.shape[1]
        assert k1.shape == (n, K, 3) and k2.ndim == 3 and k2.shape[1] == K and ar.shape[0] == n, (k1.shape, k2.shape, ar.shape)
        out = np.zeros((n, k2.shape[0]), np.float32)
        _lib.check(self.lib, self.lib.ys_kpt_iou(self.ctx, _ptr(k1), n, _ptr(k2), k2.shape[0], _ptr(ar), K, k2.shape[2], eps, 0, _ptr(out)))
        return out

    def val_match_call(self, fn, rows, count, on_device, shape, mid, labels, label_ptrs, img_w, img_h, correct):
        """THE call of the three batched matching entry points, which share their argument order: (ctx, rows, count, on_device, B, max_det, row_stride, *mid,
        label arrays [, their keypoint width], n_labels, img_w, img_h, one `correct` per metric).  shape = (B, max_det, row_stride); labels = the
        flatten_labels tuple (for the sizes); rows / count / label_ptrs / correct: host or device pointers, as on_device says."""
        tail = ((labels[3].shape[2],) if len(labels) > 3 else ()) + (labels[0].shape[0], float(img_w), float(img_h))
        _lib.check(self.lib, fn(self.ctx, rows, count, int(on_device), *shape, *mid, *label_ptrs, *tail, *correct))

    def _val_match(self, fn, rows, count, labels, mid, img_w, img_h, metrics=1, on_device=False):
        """rows [B,max_det,stride] / count [B] through val_match_call -> per metric a list of bool [count[b], 10]; on_device: on device copies of every argument."""
        rows = np.ascontiguousarray(rows, np.float32)
        count = np.ascontiguousarray(count, np.int32)
        cors = [np.zeros(rows.shape[:2] + (10,), np.uint8) for _ in range(metrics)]
        if not on_device:
            self.val_match_call(fn, _ptr(rows), _ptr(count), 0, rows.shape, mid, labels, [_ptr(a) for a in labels], img_w, img_h, [_ptr(c) for c in cors])
        else:
            dev = []
            try:
                for a in (rows, count) + tuple(labels):
                    dev.append(self.to_device(a) if a.size else self.malloc(4))
                for c in cors:
                    dev.append(self.malloc(c.size))
                nl = 2 + len(labels)
                self.val_match_call(fn, dev[0], dev[1], 1, rows.shape, mid, labels, dev[2:nl], img_w, img_h, dev[nl:])
                cors = [self.from_device(p_, c.shape, np.uint8) for p_, c in zip(dev[nl:], cors)]
            finally:
                for p_ in dev:
                    self.free(p_)
        return [[c[b, :count[b]].astype(bool) for b in range(rows.shape[0])] for c in cors]

    def val_match(self, rows, count, batch, img_w, img_h):
        """rows [B,max_det,6+extra] / count [B]: the padded NMS outputs (x1,y1,x2,y2,conf,cls,...); batch = collate dict
        (batch_idx, cls, bboxes normalised cxcywh).  Returns a list of bool [count[b], 10] (match_predictions per image)."""
        return self._val_match(self.lib.ys_val_match_batched, rows, count, flatten_labels(batch), (), img_w, img_h)[0]

    def val_match_rotated(self, rows, count, batch, img_w, img_h, angle_col=6):
        """Obber.Val's per-image part (Obber.cs:102-114) in one launch: rows [B,max_det,7+] / count [B] = oriented rows (cx,cy,w,h,conf,cls,angle);
        batch = collate dict (batch_idx, cls, bboxes [N,5] normalised cxcywh + angle).  Returns a list of bool [count[b], 10]: match_predictions on
        Metrics.batch_probiou(GT, prediction) per image, bit for bit what batch_probiou + match_predictions below give (ys_val_match_rotated_batched)."""
        return self._val_match(self.lib.ys_val_match_rotated_batched, rows, count, flatten_labels(batch, 5), (int(angle_col),), img_w, img_h)[0]

    def val_match_pose(self, rows, count, batch, img_w, img_h, kpt_num, kpt_dim, kpt_col=6, on_device=False):
        """PoseDetector.Val's per-image part (PoseDetector.cs:131-165) in one launch: rows [B,max_det,6+K*D] / count [B] = rows (x1,y1,x2,y2,conf,cls,
        keypoints); batch = collate dict (batch_idx, cls, bboxes [N,4] normalised cxcywh, keypoints [N,K,2|3] normalised).  Returns two lists of bool
        [count[b], 10]: match_predictions on Metrics.box_iou and on Metrics.kpt_iou (area = w * h * 0.53) per image, bit for bit what box_iou / kpt_iou +
        match_predictions give (ys_val_match_pose_batched).  on_device: the same call on device copies of every argument."""
        return tuple(self._val_match(self.lib.ys_val_match_pose_batched, rows, count, flatten_labels(batch, 4, kpt_num),
                                     (int(kpt_col), int(kpt_num), int(kpt_dim)), img_w, img_h, metrics=2, on_device=on_device))

    def mask_iou(self, gt_ids, nl, pred_masks, eps=1e-7):
        """Metrics.mask_iou (Metrics.cs:120-125) on (gt_ids == k+1), k < nl, vs pred_masks bool/uint8 [n, h, w] -> [nl, n] fp32."""
        ids = np.ascontiguousarray(gt_ids, np.float32).reshape(-1)
        pm = np.ascontiguousarray(np.asarray(pred_masks).astype(np.uint8)).reshape(-1, ids.shape[0]) if len(pred_masks) else np.zeros((0, ids.shape[0]), np.uint8)
        out = np.zeros((nl, pm.shape[0]), np.float32)
        _lib.check(self.lib, self.lib.ys_mask_iou(self.ctx, _ptr(ids), nl, _ptr(pm), pm.shape[0], ids.shape[0], eps, 0, _ptr(out)))
        return out

    def match_predictions(self, pred_classes, true_classes, iou):
        """YoloBaseTaskModel.match_predictions (:377-446): iou [nl, n] -> bool [n, 10]."""
        pc = np.ascontiguousarray(pred_classes, np.float32).reshape(-1)
        tc = np.ascontiguousarray(true_classes, np.float32).reshape(-1)
        iou = np.ascontiguousarray(iou, np.float32).reshape(tc.shape[0], pc.shape[0])
        cor = np.zeros((pc.shape[0], 10), np.uint8)
        _lib.check(self.lib, self.lib.ys_match_predictions(self.ctx, _ptr(pc), pc.shape[0], _ptr(tc), tc.shape[0], _ptr(iou), 0, _ptr(cor)))
        return cor.astype(bool)

    # ---- Augment.LetterBox / Augment.Rectangle (Data/Augment.cs:698-857)
    def letterbox(self, img, resized_width=640, resized_height=640, color=114, rectangle_shape=None):
        """img: uint8 or float32 [C,h,w].  LetterBox(resized_width, resized_height, color) -> (out [C,H,W], pad_l, pad_u); with
        rectangle_shape=(w, h) it is Augment.Rectangle (fit box = the resized shape, canvas = the rectangle shape)."""
        x = np.ascontiguousarray(img)
        is_float = x.dtype != np.uint8
        if is_float:
            x = np.ascontiguousarray(x, np.float32)
        Cc, h, w = x.shape
        ow, oh = rectangle_shape if rectangle_shape is not None else (resized_width, resized_height)
        out = np.empty((Cc, oh, ow), x.dtype)
        pl, pu = C.c_int32(), C.c_int32()
        _lib.check(self.lib, self.lib.ys_letterbox(self.ctx, _ptr(x), int(is_float), 0, Cc, h, w, resized_width, resized_height, ow, oh, int(color),
                                                   _ptr(out), C.byref(pl), C.byref(pu)))
        return out, pl.value, pu.value

    # ---- Mosaic4 + RandomPerspective + flips + Normalize + collate (Data/Augment.cs:158-274, 315-695, 860-966) on host arrays; the
    #      device-resident form is augment.MosaicAugmenter
    def augment_mosaic(self, arena, srcs, items, imgsz, mask_ratio=4, perspective=False, with_masks=False):
        from . import augment
        return augment.augment_mosaic(self, arena, srcs, items, imgsz, mask_ratio, perspective, with_masks)

    def augment_labels(self, srcs, lab_off, cls, boxes, keypoints, items, imgsz, perspective=False, flags=0, capacity=None):
        from . import augment
        return augment.augment_labels(self, srcs, lab_off, cls, boxes, keypoints, items, imgsz, perspective, flags, capacity)

    # ---- Ops.process_mask (Ops.cs:462-489)
    def process_mask(self, protos, masks_in, bboxes, shape, upsample=False, cpu_crop_branch=False):
        """protos [nm,mh,mw], masks_in [n,nm], bboxes [n,4] xyxy (image pixels), shape=(ih,iw) -> bool [n,oh,ow]."""
        protos = np.ascontiguousarray(protos, np.float32)
        masks_in = np.ascontiguousarray(masks_in, np.float32).reshape(-1, protos.shape[0])
        bboxes = np.ascontiguousarray(bboxes, np.float32).reshape(-1, 4)
        n, (nm, mh, mw), (ih, iw) = masks_in.shape[0], protos.shape, shape
        assert bboxes.shape[0] == n
        out = np.zeros((n, ih, iw) if upsample else (n, mh, mw), np.uint8)
        _lib.check(self.lib, self.lib.ys_process_mask(self.ctx, _ptr(protos), _ptr(masks_in), _ptr(bboxes), 0, n, nm, mh, mw,
                                                      ih, iw, int(bool(upsample)), int(bool(cpu_crop_branch)), _ptr(out)))
        return out.astype(bool)

    # ---- Ops.non_max_suppression (Ops.cs:239-371)
    def non_max_suppression(self, prediction, conf_thres=0.25, iou_thres=0.45, agnostic=False, max_det=300, nc=0,
                            max_time_img=0.05, max_nms=30000, max_wh=7680, in_place=True, rotated=False,
                            end2end=False):
        """prediction: float32 ndarray [B, 4+nc+extra, A] (xywh, probabilities).  Returns (output, keepi):
        lists of [n_i, 6+extra] float32 rows (x1,y1,x2,y2,conf,cls,extra) and [n_i] int64 anchor indices.
        Like the reference, `prediction[:, 0:4]` is converted to xyxy in place when in_place=True, the
        `agnostic` flag is accepted but ignored (Ops.cs:345), and invalid thresholds raise (YsError status 1).
        rotated=True (Ops.cs:286,349-353): oriented boxes, angle = last channel, boxes stay xywh, Ops.nms_rotated's
        "any earlier box overlaps" rule on Metrics.batch_probiou."""
        if end2end:        # Ops.cs:258-267: prediction [B, k, 6 (+ nm | + angle | + nk)] rows ordered by score -> rows with score > conf_thres, at most max_det; no keep indices
            rows = np.ascontiguousarray(prediction, np.float32)
            cnt = self.e2e_select(rows, conf_thres, max_det)
            return [rows[b, :cnt[b]].copy() for b in range(rows.shape[0])], [np.zeros((0,), np.float32)]
        pred = prediction if in_place else prediction.copy()
        if pred.dtype != np.float32 or not pred.flags["C_CONTIGUOUS"]:
            raise TypeError("prediction must be a C-contiguous float32 array [B, C, A]")
        B, Cc, A = pred.shape
        ncc = int(nc) if nc else Cc - 4
        extra = Cc - 4 - ncc
        rows = np.zeros((B, max_det, 6 + extra), np.float32)
        keep = np.zeros((B, max_det), np.int64)
        cnt = np.zeros((B,), np.int32)
        fn = self.lib.ys_nms_rotated_batched if rotated else self.lib.ys_nms_batched
        _lib.check(self.lib, fn(self.ctx, _ptr(pred), 0, B, Cc, A, conf_thres, iou_thres, max_det,
                                int(nc), max_nms, max_wh, _ptr(rows), _ptr(keep), _ptr(cnt)))
        output = [rows[b, :cnt[b]].copy() for b in range(B)]
        keepi = [keep[b, :cnt[b]].copy() for b in range(B)]
        return output, keepi

    # ---- Metrics.probiou / batch_probiou (Metrics.cs:137-177, 223-258): oriented boxes xywhr
    def probiou(self, obb1, obb2, CIoU=False, eps=1e-7):
        o1 = np.ascontiguousarray(obb1, np.float32).reshape(-1, 5); o2 = np.ascontiguousarray(obb2, np.float32).reshape(-1, 5)
        if o1.shape != o2.shape:
            raise ValueError("probiou: obb1 and obb2 must have the same shape [N, 5]")
        out = np.zeros((o1.shape[0],), np.float32)
        _lib.check(self.lib, self.lib.ys_probiou(self.ctx, _ptr(o1), _ptr(o2), 0, o1.shape[0], int(bool(CIoU)), eps, _ptr(out)))
        return out

    def batch_probiou(self, obb1, obb2, eps=1e-7):
        o1 = np.ascontiguousarray(obb1, np.float32).reshape(-1, 5); o2 = np.ascontiguousarray(obb2, np.float32).reshape(-1, 5)
        out = np.zeros((o1.shape[0], o2.shape[0]), np.float32)
        _lib.check(self.lib, self.lib.ys_batch_probiou(self.ctx, _ptr(o1), o1.shape[0], _ptr(o2), o2.shape[0], 0, eps, _ptr(out)))
        return out

    def nms_device(self, pred_dev, B, Cc, A, conf_thres, iou_thres, max_det, nc, rows_dev, keep_dev, cnt_dev,
                   max_nms=30000, max_wh=7680):
        """Device-resident variant (no copies, asynchronous): all pointers are HIP device pointers."""
        _lib.check(self.lib, self.lib.ys_nms_batched(self.ctx, pred_dev, 1, B, Cc, A, conf_thres, iou_thres, max_det,
                                                     nc, max_nms, max_wh, rows_dev, keep_dev, cnt_dev))

    # ---- Convs.Conv.forward (Convs.cs:36-62) / plain Conv2d with bias (Head.cs:47-50)
    def conv_bn_act(self, x, weight, k, s, bn=None, bias=None, act=True, training=True, dtype="f32", stat_mode=None, extras=None):
        """x [B,Cin,H,W], weight [Cout,Cin,k,k] float32.  bn = dict(weight, bias, running_mean, running_var)
        (running stats are updated in place when training).  Returns y [B,Cout,Ho,Wo] float32.
        stat_mode (ys_conv_bn_act_fwd_ex): 0 = statistics rows + finalize launch, 1 = fixed-point accumulators finalized inside the apply pass (what a model
        runs); extras: a dict that receives y_raw, coef [4][Cout] and stat_rows of a training-mode BatchNorm call."""
        x = np.ascontiguousarray(x, np.float32)
        w = np.ascontiguousarray(weight, np.float32)
        B, Cin, H, W = x.shape
        Cout = w.shape[0]
        p = k // 2
        Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
        y = np.empty((B, Cout, Ho, Wo), np.float32)
        dt = _dtype_code(dtype)
        g = b = rm = rv = None
        if bn is not None:
            g = np.ascontiguousarray(bn["weight"], np.float32)
            b = np.ascontiguousarray(bn["bias"], np.float32)
            rm, rv = bn["running_mean"], bn["running_var"]
            assert rm.dtype == np.float32 and rv.dtype == np.float32
        bs = np.ascontiguousarray(bias, np.float32) if bias is not None else None
        if stat_mode is None and extras is None:
            _lib.check(self.lib, self.lib.ys_conv_bn_act_fwd(self.ctx, dt, _ptr(x), B, Cin, H, W, _ptr(w), Cout, k, s,
                                                             _ptr(g), _ptr(b), _ptr(rm), _ptr(rv), _ptr(bs), int(act),
                                                             int(training), _ptr(y)))
            return y
        y_raw = coef = None
        rows = C.c_int32(0)
        if extras is not None and bn is not None and training:
            y_raw, coef = np.empty_like(y), np.empty((4, Cout), np.float32)
        _lib.check(self.lib, self.lib.ys_conv_bn_act_fwd_ex(self.ctx, dt, _ptr(x), B, Cin, H, W, _ptr(w), Cout, k, s,
                                                            _ptr(g), _ptr(b), _ptr(rm), _ptr(rv), _ptr(bs), int(act),
                                                            int(training), int(stat_mode or 0), _ptr(y), _ptr(y_raw), _ptr(coef),
                                                            C.byref(rows) if y_raw is not None else None))
        if y_raw is not None:
            extras.update(y_raw=y_raw, coef=coef, stat_rows=rows.value)
        return y

    # ---- BatchNorm training kernels in isolation (ys_bn_train_fwd / ys_bn_train_bwd / ys_colsum / ys_upsample2x / ys_copy_view); arrays channel-major [C][rows]
    def bn_train_fwd(self, problems, mode, act=True, dtype="f32"):
        """problems: dicts with y [C][rows], gamma, beta, run_mean, run_var, optional nbt, res, partial [P][2][C] (mode 1), res_pad / res_coff / z_pad / z_coff /
        res_shares_z.  Returns (status, [dict(z, coef, run_mean, run_var, nbt, part, view_intact)])."""
        f32 = lambda a: None if a is None else np.array(a, np.float32, order="C")
        cs, keep = (_lib.BnFwdCase * len(problems))(), []
        for c, p in zip(cs, problems):
            y = f32(p["y"])
            Cn, rows = y.shape
            k = dict(y=y, gamma=f32(p["gamma"]), beta=f32(p["beta"]), run_mean=f32(p["run_mean"]), run_var=f32(p["run_var"]),
                     nbt=None if p.get("nbt") is None else np.array([p["nbt"]], np.float32), res=f32(p.get("res")), partial=f32(p.get("partial")),
                     z=np.full((Cn, rows), np.nan, np.float32), coef=np.full((4, Cn), np.nan, np.float32), part_out=np.full((768, 2, Cn), np.nan, np.float32),
                     acc_out=np.zeros((8, Cn, 2), np.uint64))
            keep.append(k)
            for name, a in k.items():
                setattr(c, name, _ptr(a))
            c.rows, c.C = rows, Cn
            c.res_pad, c.res_coff, c.z_pad, c.z_coff = p.get("res_pad", 0), p.get("res_coff", 0), p.get("z_pad", 0), p.get("z_coff", 0)
            c.res_shares_z = int(p.get("res_shares_z", 0))
            c.P = 0 if k["partial"] is None else k["partial"].shape[0]
            c.nblk, c.view_intact = 0, -1
        status = self.lib.ys_bn_train_fwd(self.ctx, _dtype_code(dtype), mode, int(act), len(problems), cs)
        out = [dict(z=k["z"], coef=k["coef"], run_mean=k["run_mean"], run_var=k["run_var"], nbt=None if k["nbt"] is None else float(k["nbt"][0]),
                    part=k["part_out"][:c.nblk], acc=k["acc_out"], view_intact=c.view_intact) for c, k in zip(cs, keep)]
        return status, out

    def bn_train_bwd(self, problems, mode, act=True, dtype="f32"):
        """problems: dicts with dz, y [C][rows], coef [4][C], dgamma, dbeta, optional rg, dz_pad / dz_coff / rg_pad / rg_coff; mode 3: rows, src = [(part [nblk][2][C],
        c1), ...].  Returns (status, [dict(dy, k23, dgamma, dbeta, rg, part, view_intact)])."""
        f32 = lambda a: None if a is None else np.array(a, np.float32, order="C")
        cs, keep = (_lib.BnBwdCase * len(problems))(), []
        for c, p in zip(cs, problems):
            coef = f32(p["coef"])
            Cn = coef.shape[1]
            rows = p["rows"] if "rows" in p else np.shape(p["dz"])[1]
            k = dict(dz=f32(p.get("dz")), y=f32(p.get("y")), coef=coef, dgamma=f32(p["dgamma"]), dbeta=f32(p["dbeta"]), rg=f32(p.get("rg")),
                     dy=np.full((Cn, rows), np.nan, np.float32), k23=np.full((2, Cn), np.nan, np.float32), part_out=np.full((768, 2, Cn), np.nan, np.float32))
            for name, a in k.items():
                setattr(c, name, _ptr(a))
            src = [(f32(s_), int(c1)) for s_, c1 in p.get("src", [])]
            k["src"] = src
            keep.append(k)
            c.nsrc = len(src)
            for i, (s_, c1) in enumerate(src):
                c.src_part[i], c.src_nblk[i], c.src_c1[i] = s_.ctypes.data, s_.shape[0], c1
            c.rows, c.C = rows, Cn
            c.dz_pad, c.dz_coff, c.rg_pad, c.rg_coff = p.get("dz_pad", 0), p.get("dz_coff", 0), p.get("rg_pad", 0), p.get("rg_coff", 0)
            c.nblk, c.view_intact = 0, -1
        status = self.lib.ys_bn_train_bwd(self.ctx, _dtype_code(dtype), mode, int(act), len(problems), cs)
        out = [dict(dy=k["dy"], k23=k["k23"], dgamma=k["dgamma"], dbeta=k["dbeta"], rg=k["rg"], part=k["part_out"][:c.nblk], view_intact=c.view_intact)
               for c, k in zip(cs, keep)]
        return status, out

    # ---- fp8 path kernel by kernel (ys_f8_quant / ys_f8_scales / ys_bn_apply_q8_fwd / _bwd / ys_conv_f8_fwd / ys_conv_f8_dgrad)
    F8_KINDS = {"e4m3": 0, "e5m2": 1, "amax": 2, "weights": 3}

    def f8_amax_ways(self):
        return int(self.lib.ys_f8_amax_ways())

    def f8_quant(self, x, kind, qscale=1.0, coff=0, pad=0):
        """x [rows][C] (row-major; bf16 on the device) through one quantiser launch -> dict(q8 uint8 [rows][C] or None, amax, slots [ways], view_intact).
        kind "weights": qscale is amax_w."""
        x = np.ascontiguousarray(x, np.float32)
        rows, Cn = x.shape
        kd = self.F8_KINDS[kind]
        q8 = None if kd == 2 else np.full((rows, Cn), 0xA5, np.uint8)
        amax, ok = C.c_float(-1.0), C.c_int32(-1)
        slots = np.full(self.f8_amax_ways(), np.nan, np.float32)
        _lib.check(self.lib, self.lib.ys_f8_quant(self.ctx, kd, _ptr(x), rows, Cn, coff, pad, float(qscale), _ptr(q8), C.byref(amax), _ptr(slots), C.byref(ok)))
        return dict(q8=q8, amax=np.float32(amax.value), slots=slots, view_intact=ok.value)

    def f8_scales(self, params, layers, conv_layer, amax_x, amax_dy, scales):
        """layers = [(offset, count)]; amax_x / amax_dy [n][ways], scales [n][4] -> (amax_w [n_layers], amax_x, amax_dy, scales) after the two launches."""
        p = np.ascontiguousarray(params, np.float32)
        off = np.ascontiguousarray([l[0] for l in layers], np.int64)
        cnt = np.ascontiguousarray([l[1] for l in layers], np.int64)
        cl = np.ascontiguousarray(conv_layer, np.int32)
        ax, ag, sc = (np.array(a, np.float32, order="C") for a in (amax_x, amax_dy, scales))
        ways = self.f8_amax_ways()
        assert ax.shape == (len(cl), ways) and ag.shape == ax.shape and sc.shape == (len(cl), 4), (ax.shape, ag.shape, sc.shape)
        aw = np.full(len(layers), np.nan, np.float32)
        _lib.check(self.lib, self.lib.ys_f8_scales(self.ctx, _ptr(p), p.size, _ptr(off), _ptr(cnt), len(layers), _ptr(cl), len(cl), _ptr(ax), _ptr(ag), _ptr(sc),
                                                   _ptr(aw)))
        return aw, ax, ag, sc

    def bn_apply_q8_fwd(self, y, scale, shift, qscale, act=True, res=None, z_view=(0, 0), res_view=(0, 0), res_shares_z=False):
        """bn_act_apply_q8_kernel alone: y, res [C][rows]; views = (pad, coff) -> dict(z [C][rows], q8 uint8 [rows][C], amax, view_intact)."""
        f32 = lambda a: None if a is None else np.ascontiguousarray(a, np.float32)
        y, res, sc, sh = f32(y), f32(res), f32(scale), f32(shift)
        Cn, rows = y.shape
        z, q8 = np.full((Cn, rows), np.nan, np.float32), np.full((rows, Cn), 0xA5, np.uint8)
        amax, ok = C.c_float(-1.0), C.c_int32(-1)
        _lib.check(self.lib, self.lib.ys_bn_apply_q8_fwd(self.ctx, int(act), _ptr(y), rows, Cn, _ptr(sc), _ptr(sh), _ptr(res), res_view[0], res_view[1],
                                                         z_view[0], z_view[1], int(res_shares_z), float(qscale), _ptr(z), _ptr(q8), C.byref(amax), C.byref(ok)))
        return dict(z=z, q8=q8, amax=np.float32(amax.value), view_intact=ok.value)

    def bn_apply_q8_bwd(self, dz, y, coef, qscale, act=True, rg=None, dz_view=(0, 0), rg_view=(0, 0)):
        """bn_bwd_apply_q8_kernel alone: dz, y, rg [C][rows], coef [4][C] = scale, shift, k2, k3 -> dict(dy, rg, q8 uint8 [rows][C], amax, view_intact)."""
        f32 = lambda a: np.ascontiguousarray(a, np.float32)
        dz, y, coef = f32(dz), f32(y), f32(coef)
        rg = None if rg is None else np.array(rg, np.float32, order="C")
        Cn, rows = y.shape
        dy, q8 = np.full((Cn, rows), np.nan, np.float32), np.full((rows, Cn), 0xA5, np.uint8)
        amax, ok = C.c_float(-1.0), C.c_int32(-1)
        _lib.check(self.lib, self.lib.ys_bn_apply_q8_bwd(self.ctx, int(act), _ptr(dz), _ptr(y), rows, Cn, _ptr(coef), dz_view[0], dz_view[1], _ptr(rg), rg_view[0],
                                                         rg_view[1], float(qscale), _ptr(dy), _ptr(q8), C.byref(amax), C.byref(ok)))
        return dict(dy=dy, rg=rg, q8=q8, amax=np.float32(amax.value), view_intact=ok.value)

    def conv_f8_fwd(self, x, weight, k, s, bn=None, bias=None, act=True, training=True, prev_amax=0.0):
        """conv_bn_act(dtype="fp8") with a delayed activation scale (prev_amax = 0: current) -> dict(y, y_raw, coef, stat_rows, scales [4], amax recorded)."""
        x = np.ascontiguousarray(x, np.float32)
        w = np.ascontiguousarray(weight, np.float32)
        B, Cin, H, W = x.shape
        Cout = w.shape[0]
        p = k // 2
        y = np.empty((B, Cout, (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1), np.float32)
        g = b = rm = rv = y_raw = coef = None
        if bn is not None:
            g, b = np.ascontiguousarray(bn["weight"], np.float32), np.ascontiguousarray(bn["bias"], np.float32)
            rm, rv = bn["running_mean"], bn["running_var"]
            assert rm.dtype == np.float32 and rv.dtype == np.float32
            if training:
                y_raw, coef = np.empty_like(y), np.empty((4, Cout), np.float32)
        bs = np.ascontiguousarray(bias, np.float32) if bias is not None else None
        rows, amax, scales = C.c_int32(0), C.c_float(-1.0), np.full(4, np.nan, np.float32)
        _lib.check(self.lib, self.lib.ys_conv_f8_fwd(self.ctx, _ptr(x), B, Cin, H, W, _ptr(w), Cout, k, s, _ptr(g), _ptr(b), _ptr(rm), _ptr(rv), _ptr(bs), int(act),
                                                     int(training), float(prev_amax), _ptr(y), _ptr(y_raw), _ptr(coef),
                                                     C.byref(rows) if y_raw is not None else None, _ptr(scales), C.byref(amax)))
        return dict(y=y, y_raw=y_raw, coef=coef, stat_rows=rows.value, scales=scales, amax=np.float32(amax.value))

    def conv_f8_dgrad(self, x_shape, weight, k, s, dy, prev_amax=0.0):
        """The fp8 input gradient of conv2d(x, weight, stride s, padding k // 2) given dy, with a delayed gradient scale -> dict(dx, scales [4], amax recorded)."""
        w = np.ascontiguousarray(weight, np.float32)
        dy = np.ascontiguousarray(dy, np.float32)
        B, Cin, H, W = x_shape
        dx = np.full(x_shape, np.nan, np.float32)
        amax, scales = C.c_float(-1.0), np.full(4, np.nan, np.float32)
        _lib.check(self.lib, self.lib.ys_conv_f8_dgrad(self.ctx, B, Cin, H, W, _ptr(w), w.shape[0], k, s, _ptr(dy), float(prev_amax), _ptr(dx), _ptr(scales),
                                                       C.byref(amax)))
        return dict(dx=dx, scales=scales, amax=np.float32(amax.value))

    def stem6_fwd(self, x, weight, scale=None, shift=None, act=True, stat_mode=0):
        """Yolov5u's stem Conv(3, Cout, 6, 2, 2) on the 6x6 stem forward kernel alone (ys_stem6_fwd).  scale None: the training form -> (y as the stored bf16
        values, stats [2, Cout] float64 = the kernel's per-channel sum and sum of squares); else eval -> (act(scale * conv + shift), None)."""
        x = np.ascontiguousarray(x, np.float32)
        w = np.ascontiguousarray(weight, np.float32)
        B, _, H, W = x.shape
        Cout = w.shape[0]
        y = np.full((B, Cout, (H - 2) // 2 + 1, (W - 2) // 2 + 1), np.nan, np.float32)
        train = scale is None
        stats = np.full((2, Cout), np.nan, np.float64) if train else None
        sc = None if train else np.ascontiguousarray(scale, np.float32)
        sh = None if train else np.ascontiguousarray(shift, np.float32)
        _lib.check(self.lib, self.lib.ys_stem6_fwd(self.ctx, _ptr(x), B, H, W, _ptr(w), Cout, int(stat_mode), _ptr(sc), _ptr(sh), int(bool(act)), _ptr(y),
                                                   _ptr(stats)))
        return y, stats

    def stem6_wgrad(self, x, dy):
        """The weight gradient [Cout, 3, 6, 6] of the same convolution on the 6x6 stem weight-gradient kernel + the split reduction (ys_stem6_wgrad)."""
        x = np.ascontiguousarray(x, np.float32)
        dy = np.ascontiguousarray(dy, np.float32)
        B, _, H, W = x.shape
        Cout = dy.shape[1]
        dw = np.full((Cout, 3, 6, 6), np.nan, np.float32)
        _lib.check(self.lib, self.lib.ys_stem6_wgrad(self.ctx, _ptr(x), B, H, W, _ptr(dy), Cout, _ptr(dw)))
        return dw

    def conv_labels(self, fn):
        """fn() with the per-launch profile on -> (its result, the labels of the convolution launches it made, in order per class)."""
        import os
        import tempfile
        self.kernel_profile(True)
        try:
            out = fn()
            self.synchronize()
            fd, path = tempfile.mkstemp(suffix=".csv")
            os.close(fd)
            try:
                self.kernel_profile_dump(path)
                lines = open(path).read().splitlines()[1:]
            finally:
                os.remove(path)
        finally:
            self.kernel_profile(False)
        return out, [l.split(",")[1] for l in lines if l.startswith("conv_igemm,")]

    def colsum(self, x, grad, bstride=None, ld_pad=0, coff=0, dtype="f32"):
        """grad [C] + column sums of x [B][C][rows_per_b] -> (status, grad, view_intact)."""
        x = np.ascontiguousarray(x, np.float32)
        g = np.array(grad, np.float32)
        B, Cn, rpb = x.shape
        ok = C.c_int32(-1)
        status = self.lib.ys_colsum(self.ctx, _dtype_code(dtype), _ptr(x), B, Cn, rpb, rpb if bstride is None else bstride, ld_pad, coff, _ptr(g), C.byref(ok))
        return status, g, ok.value

    def upsample2x(self, src, H, W, backward=False, views=(None, 0, None, 0), dst=None, dtype="f32"):
        """src [B][C][H*W] -> [B][C][4*H*W], or backward src [B][C][4*H*W] -> [B][C][H*W] (dst given: accumulate into it) -> (status, dst, view_intact)."""
        src = np.ascontiguousarray(src, np.float32)
        B, Cn = src.shape[:2]
        out = np.array(dst, np.float32) if dst is not None else np.full((B, Cn, H * W if backward else 4 * H * W), np.nan, np.float32)
        sl, so, dl, do = views
        ok = C.c_int32(-1)
        status = self.lib.ys_upsample2x(self.ctx, _dtype_code(dtype), int(backward), _ptr(src), B, H, W, Cn, Cn + so if sl is None else sl, so,
                                        Cn + do if dl is None else dl, do, int(dst is not None), _ptr(out), C.byref(ok))
        return status, out, ok.value

    def copy_view(self, src, views=(None, 0, None, 0), dst=None, dtype="f32"):
        """dst view (+)= src view, src [C][rows] -> (status, dst, view_intact); dst given: accumulate into it."""
        src = np.ascontiguousarray(src, np.float32)
        Cn, rows = src.shape
        out = np.array(dst, np.float32) if dst is not None else np.full((Cn, rows), np.nan, np.float32)
        sl, so, dl, do = views
        ok = C.c_int32(-1)
        status = self.lib.ys_copy_view(self.ctx, _dtype_code(dtype), _ptr(src), rows, Cn, Cn + so if sl is None else sl, so, Cn + do if dl is None else dl, do,
                                       int(dst is not None), _ptr(out), C.byref(ok))
        return status, out, ok.value
