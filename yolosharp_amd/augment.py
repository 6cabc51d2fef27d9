"""The reference's default training input (ImageProcessType.Mosiac, Data/YoloDataset.cs:57-151) with the pixels and labels produced on the
device (csrc/augment.hip; include/yolosharp_hip.h ys_augment_mosaic / ys_augment_labels).  The host keeps what is random: per output
image it draws what Augment.Mosaic (Data/Augment.cs:153-164), RandomPerspective.affine_transform (:323-356) and FlipLR / FlipUD (:869, :926)
draw, and uploads one 68-byte item.  TorchSharp's torch.rand streams cannot be reproduced: the drawn PARAMETERS are the interface.

The close-mosaic branch -- what YoloDataset.CloseMosaic(true) builds (Data/YoloDataset.cs:378-429; the training loop calls it with
`epoch > Config.CloseMosaic`, Models/YoloBaseTaskModel.cs:180) and what ImageProcessType.Letterbox is: LetterBox + FlipLR / FlipUD -- runs on the
same uploaded arena, tables and buffers (ys_augment_letterbox / ys_augment_letterbox_labels; MosaicAugmenter.close_mosaic).  Its items carry the
primary index and the two flip decisions only.

RandomHSV (Data/Augment.cs:968-987), the last transform of both chains (Data/YoloDataset.cs:86, :416), is torchvision ColorJitter(brightness 0.4, contrast 0,
saturation 0.7, hue 0.015) on the uint8 image: MosaicAugmenter(hsv=(0.015, 0.7, 0.4)) draws one ys_aug_jitter row per image after the flips (draw_jitter follows
ColorJitter.get_params) and the gather kernels apply it in their epilogue (ys_augment_mosaic_jitter / ys_augment_letterbox_jitter); color_jitter() is the operator
on its own, contrast included (ys_color_jitter).  TorchVision.NET is not in the reference tree: torchvision's public uint8 algorithm is the contract.

OBB corner labels (Data/YoloDataset.cs:110-129, 216-244): labels that carry "obb" [n, 4, 2] pixel corners go through ys_augment_labels_obb /
ys_augment_letterbox_labels_obb -- the corners through the branch's chain, then xyxyxyxy2xywhr (the minimum-area rectangle, OpenCV >= 4.5.1's canonical form:
angle in (0, pi/2], w along the angle) and columns 0-3 / imgsz: the batch's boxes are [capacity, 5].  Quirks kept: the keep decision is made on the axis-aligned
box alone, the LetterBox pads are not scaled by ratio and that branch clips nothing.  The choice among equal-area rectangles is UNPINNED against OpenCV
(include/yolosharp_hip.h).  xyxyxyxy2xywhr() is the operator on its own.

The classification input (Data/ClassificationDataset.cs:90-131 with Auto_Augment = None): ClassifyAugmenter uploads the uint8 dataset and the class ids once;
per batch the host draws what RandomResizedCrop, the two flips, RandomErasing and ColorJitter draw (draw_classify_items; the val chain, Resize + CenterCrop,
draws nothing: draw_classify_val_items) and ys_augment_classify gathers crop, resize, flips, erase noise, all four jitter ops and mul(1 / 255) in one pass
(csrc/augment_cls.hip) -> ClassifyDeviceBatch.  Auto_Augment = AutoAugment (the reference's default, Data/Config.cs:228) / RandAugment:
ClassifyAugmenter(auto_augment=AutoAugment() / RandAugment()) draws one ys_aa_row per image between the flips and the erasing draws (draw_auto_augment: the
sub-policy, probabilities, signs and magnitudes of torchvision's get_params, the affine ops as their inverse matrix) and ys_augment_classify_aa runs the two
operator slots on the staged uint8 image (csrc/augment_aa.hip); auto_augment_ops() is the operators on their own.  Not built: AugMix.  TorchVision.NET is not
in the reference tree: nearest interpolation, smaller-edge Resize(int), CenterCrop's rounding, the crop tries' accept test, the AutoAugment policy table,
magnitude spaces and operator arithmetic are torchvision's public ones, UNPINNED.

Not built: the `rand > p` case of Augment.Mosaic (it yields images of unequal sizes).
kpt_dim = 3 only."""
import ctypes as C
import functools
import math

import numpy as np

from . import _lib

SRC_DTYPE = np.dtype([("img_off", "<i8"), ("mask_off", "<i8"), ("h", "<i4"), ("w", "<i4"), ("mh", "<i4"), ("mw", "<i4")])
ITEM_DTYPE = np.dtype([("src", "<i4", (4,)), ("xc", "<i4"), ("yc", "<i4"), ("M", "<f4", (9,)), ("flip_lr", "<i4"), ("flip_ud", "<i4")])
JITTER_DTYPE = np.dtype([("order", "<i4", (4,)), ("factor", "<f4", (4,))])
assert SRC_DTYPE.itemsize == C.sizeof(_lib.AugSrc) == 32 and ITEM_DTYPE.itemsize == C.sizeof(_lib.AugItem) == 68
assert JITTER_DTYPE.itemsize == C.sizeof(_lib.AugJitter) == 32
CLS_ITEM_DTYPE = np.dtype([(n, "<i4") for n in ("src", "top", "left", "ch", "cw", "oh", "ow", "oy", "ox", "flip_lr", "flip_ud", "er_y", "er_x", "er_h", "er_w")] +
                          [("er_seed", "<u4")])
assert CLS_ITEM_DTYPE.itemsize == C.sizeof(_lib.ClsItem) == 64
AA_ROW_DTYPE = np.dtype([("op", "<i4", (2,)), ("arg", "<f4", (2,)), ("theta", "<f4", (2, 6))])
assert AA_ROW_DTYPE.itemsize == C.sizeof(_lib.AaRow) == 64
JITTER_BRIGHTNESS, JITTER_CONTRAST, JITTER_SATURATION, JITTER_HUE = 0, 1, 2, 3      # the op ids of ColorJitter.forward
YS_AUG_SORT_FLIPPED = 1              # ys_augment_labels: write a flipped box as (min, max)
YS_AUG_FLIP_KEEP_SIZE = 2            # ys_augment_letterbox_labels: a flip leaves the cxcywh box's w / h alone (the reference writes s - w)


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def mosaic4_rects(xc, yc, shapes, s):
    """Augment.Mosaic._mosaic4's rectangles (:184-203) for the four (h, w) of `shapes`: a list of ((x1a, y1a, x2a, y2a), (x1b, y1b, x2b, y2b)) --
    canvas rectangle of the 2s x 2s image, source rectangle of the tile.  padw = x1a - x1b, padh = y1a - y1b (:211-212)."""
    out = []
    for i, (h, w) in enumerate(shapes):
        if i == 0:
            a = (max(xc - w, 0), max(yc - h, 0), xc, yc)
            b = (w - (a[2] - a[0]), h - (a[3] - a[1]), w, h)
        elif i == 1:
            a = (xc, max(yc - h, 0), min(xc + w, s * 2), yc)
            b = (0, h - (a[3] - a[1]), min(w, a[2] - a[0]), h)
        elif i == 2:
            a = (max(xc - w, 0), yc, xc, min(s * 2, yc + h))
            b = (w - (a[2] - a[0]), 0, w, min(a[3] - a[1], h))
        else:
            a = (xc, yc, min(xc + w, s * 2), min(s * 2, yc + h))
            b = (0, 0, min(w, a[2] - a[0]), min(a[3] - a[1], h))
        out.append((a, b))
    return out


def perspective_matrices(u, s, degrees=0.0, translate=0.1, scale=0.5, shear=0.0, perspective=0.0):
    """RandomPerspective.affine_transform's M (:323-356) for n images at once from their uniform draws u [n, 8] in [0, 1) -- in the reference's
    draw order: perspective x, y; angle; scale; shear x, y; translate x, y -- for the 2s x 2s mosaic canvas and the s x s output.
    M = T @ S @ R @ P @ C with C at minus half the canvas, fp32 like the reference.  -> [n, 3, 3] float32."""
    f = np.float32
    d = np.asarray(u, f).reshape(-1, 8) * f(2) - f(1)
    n = d.shape[0]
    Cm, P, R, S, T = (np.tile(np.eye(3, dtype=f), (n, 1, 1)) for _ in range(5))
    Cm[:, 0, 2] = Cm[:, 1, 2] = -(2 * s) // 2
    P[:, 2, 0] = d[:, 0] * f(perspective)
    P[:, 2, 1] = d[:, 1] * f(perspective)
    sc = f(1) + d[:, 3] * f(scale)
    rad = (d[:, 2] * f(degrees) * f(math.pi) / f(180.0)).astype(f)
    alpha, beta = np.cos(rad).astype(f) * sc, np.sin(rad).astype(f) * sc            # GetRotationMatrix2D(0, 0, a, sc), :645-662
    R[:, 0, 0], R[:, 0, 1], R[:, 1, 0], R[:, 1, 1] = alpha, beta, -beta, alpha
    S[:, 0, 1] = np.tan(d[:, 4].astype(np.float64) * shear * math.pi / 180.0)
    S[:, 1, 0] = np.tan(d[:, 5].astype(np.float64) * shear * math.pi / 180.0)
    T[:, 0, 2] = (0.5 + d[:, 6].astype(np.float64) * translate) * s
    T[:, 1, 2] = (0.5 + d[:, 7].astype(np.float64) * translate) * s
    return (T @ (S @ (R @ (P @ Cm)))).astype(f)


def random_perspective_matrix(rng, s, degrees=0.0, translate=0.1, scale=0.5, shear=0.0, perspective=0.0):
    """One matrix from eight draws of `rng` (anything with .random(), e.g. a numpy Generator) in the reference's order (perspective_matrices)."""
    u = [rng.random() for _ in range(8)]
    return perspective_matrices([u], s, degrees, translate, scale, shear, perspective)[0]


def make_items(n):
    return np.zeros((n,), ITEM_DTYPE)


def pack_sources(images_u8, masks=None):
    """One uint8 arena for the sources' RGB planes (and id masks): (arena, srcs[SRC_DTYPE])."""
    srcs = np.zeros((len(images_u8),), SRC_DTYPE)
    parts, off = [], 0
    for k, im in enumerate(images_u8):
        im = np.ascontiguousarray(im, np.uint8)
        assert im.ndim == 3 and im.shape[0] == 3, im.shape
        srcs[k]["img_off"], srcs[k]["h"], srcs[k]["w"], srcs[k]["mask_off"] = off, im.shape[1], im.shape[2], -1
        parts.append(im.reshape(-1)); off += im.size
        if masks is not None and masks[k] is not None:
            mk = np.ascontiguousarray(masks[k], np.uint8)
            assert mk.ndim == 2, mk.shape
            srcs[k]["mask_off"], srcs[k]["mh"], srcs[k]["mw"] = off, mk.shape[0], mk.shape[1]
            parts.append(mk.reshape(-1)); off += mk.size
    return np.ascontiguousarray(np.concatenate(parts)), srcs


def pack_labels(labels):
    """Per-source label dicts {cls [n], bboxes [n, 4] pixel xyxy in the source's frame, keypoints [n, K, 3] (optional)} -> (lab_off [n_src + 1],
    cls, boxes, keypoints or None).  OBB labels carry "obb" [n, 4, 2] pixel corners: see pack_obb; where "bboxes" is absent the box is the corners'
    axis-aligned one (min / max per axis, YoloDataset.cs:235-243)."""
    cnt = [int(np.asarray(l["cls"]).reshape(-1).shape[0]) for l in labels]
    lab_off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
    cls = np.concatenate([np.asarray(l["cls"], np.float32).reshape(-1) for l in labels]) if labels else np.zeros((0,), np.float32)
    boxes = np.concatenate([np.asarray(l["bboxes"], np.float32).reshape(-1, 4) if l.get("bboxes") is not None else _obb_boxes(l["obb"]) for l in labels])
    kp = None
    if labels and labels[0].get("keypoints") is not None:
        K = np.asarray(labels[0]["keypoints"]).shape[1]
        kp = np.ascontiguousarray(np.concatenate([np.asarray(l["keypoints"], np.float32).reshape(-1, K, 3) for l in labels]))
    return lab_off, np.ascontiguousarray(cls), np.ascontiguousarray(boxes), kp


def _obb_boxes(corners):
    c = np.asarray(corners, np.float32).reshape(-1, 4, 2)
    return np.concatenate([c.min(1), c.max(1)], 1).astype(np.float32).reshape(-1, 4)


def pack_obb(labels):
    """The "obb" corners [n, 4, 2] (pixels, the source's frame) of per-source label dicts as one table, or None when the labels carry none."""
    if not labels or labels[0].get("obb") is None:
        return None
    return np.ascontiguousarray(np.concatenate([np.asarray(l["obb"], np.float32).reshape(-1, 4, 2) for l in labels]))


def xyxyxyxy2xywhr(engine, corners):
    """ys_xyxyxyxy2xywhr on a HOST array: corners [n, 4, 2] -> [n, 5] = (cx, cy, w, h) in the corners' units, angle in radians in (0, pi/2]."""
    c = np.ascontiguousarray(corners, np.float32).reshape(-1, 4, 2)
    out = np.empty((c.shape[0], 5), np.float32)
    _lib.check(engine.lib, engine.lib.ys_xyxyxyxy2xywhr(engine.ctx, _ptr(c), c.shape[0], 0, _ptr(out)))
    return out


def make_jitter(n):
    """n ys_aug_jitter rows that do nothing: every slot -1, factors (1, 1, 1, 0)."""
    rows = np.zeros((n,), JITTER_DTYPE)
    rows["order"] = -1
    rows["factor"] = (1.0, 1.0, 1.0, 0.0)
    return rows


def check_jitter(rows, allow_contrast=False):
    """The library's row check (include/yolosharp_hip.h) on the host: ValueError for an invalid row, and for a contrast row where none is allowed."""
    rows = np.ascontiguousarray(rows, JITTER_DTYPE)
    for b, (order, factor) in enumerate(zip(rows["order"], rows["factor"])):
        ids = [int(i) for i in order if i != -1]
        if any(i < 0 or i > 3 for i in ids) or len(set(ids)) != len(ids):
            raise ValueError("jitter row %d: order %s must hold ids in {-1, 0..3}, none twice" % (b, order.tolist()))
        if not (np.all(np.isfinite(factor[:3])) and np.all(factor[:3] >= 0) and -0.5 <= factor[3] <= 0.5):
            raise ValueError("jitter row %d: factors %s: brightness, contrast, saturation finite and >= 0, hue in [-0.5, 0.5]" % (b, factor.tolist()))
        if JITTER_CONTRAST in ids and not allow_contrast:
            raise ValueError("jitter row %d runs contrast: the fused entries have no image mean (color_jitter does)" % b)
    return rows


def draw_jitter(rng, n, hgain, sgain, vgain, cgain=0.0):
    """n rows as torchvision ColorJitter.get_params draws them for ColorJitter(brightness=vgain, contrast=cgain, saturation=sgain, hue=hgain) -- RandomHSV's
    argument order (Data/Augment.cs:968-987).  Per image: randperm(4) first (rng.permutation), then brightness U(max(0, 1 - v), 1 + v), contrast, saturation
    likewise and hue U(-h, h), one rng.random() each, drawn ONLY for a non-zero gain.  An op with gain 0 keeps its slot of the permutation as -1."""
    gains = (float(vgain), float(cgain), float(sgain), float(hgain))
    assert all(g >= 0 for g in gains) and gains[3] <= 0.5, gains
    rows = make_jitter(n)
    for b in range(n):
        perm = rng.permutation(4)
        for op in range(4):
            if gains[op] > 0:
                lo, hi = (-gains[op], gains[op]) if op == JITTER_HUE else (max(0.0, 1.0 - gains[op]), 1.0 + gains[op])
                rows[b]["factor"][op] = lo + (hi - lo) * rng.random()
        rows[b]["order"] = [int(op) if gains[op] > 0 else -1 for op in perm]
    return rows


def color_jitter(engine, images_u8, rows, out_float=False):
    """ys_color_jitter on HOST arrays: uint8 [B, 3, h, w] through the rows' ops (all four) -> uint8, or fp32 byte * (1 / 255.0f) with out_float."""
    img = np.ascontiguousarray(images_u8, np.uint8)
    rows = np.ascontiguousarray(rows, JITTER_DTYPE)
    assert img.ndim == 4 and img.shape[1] == 3 and rows.shape == (img.shape[0],), (img.shape, rows.shape)
    out = np.empty(img.shape, np.float32 if out_float else np.uint8)
    _lib.check(engine.lib, engine.lib.ys_color_jitter(engine.ctx, _ptr(img), _ptr(rows), img.shape[0], img.shape[2], img.shape[3], 0, _ptr(out), int(bool(out_float))))
    return out


def augment_mosaic(engine, arena, srcs, items, imgsz, mask_ratio=4, perspective=False, with_masks=False, jitter=None):
    """ys_augment_mosaic (jitter rows given: ys_augment_mosaic_jitter) on HOST arrays: -> (images fp32 [B, 3, s, s], masks fp32 [B, s/r, s/r] or None)."""
    arena = np.ascontiguousarray(arena, np.uint8)
    srcs, items = np.ascontiguousarray(srcs, SRC_DTYPE), np.ascontiguousarray(items, ITEM_DTYPE)
    B, s = items.shape[0], int(imgsz)
    images = np.empty((B, 3, max(s, 0), max(s, 0)), np.float32)
    masks = np.empty((B, s // mask_ratio, s // mask_ratio), np.float32) if with_masks else None
    if jitter is None:
        _lib.check(engine.lib, engine.lib.ys_augment_mosaic(engine.ctx, _ptr(arena), _ptr(srcs), srcs.shape[0], _ptr(items), B, 0, s, int(mask_ratio),
                                                            int(bool(perspective)), _ptr(images), _ptr(masks)))
    else:
        jitter = np.ascontiguousarray(jitter, JITTER_DTYPE)
        assert jitter.shape == (B,), jitter.shape
        _lib.check(engine.lib, engine.lib.ys_augment_mosaic_jitter(engine.ctx, _ptr(arena), _ptr(srcs), srcs.shape[0], _ptr(items), B, 0, s, int(mask_ratio),
                                                                   int(bool(perspective)), _ptr(jitter), _ptr(images), _ptr(masks)))
    return images, masks


def augment_labels(engine, srcs, lab_off, cls, boxes, keypoints, items, imgsz, perspective=False, flags=0, capacity=None, kpt_dim=3):
    """ys_augment_labels on HOST arrays: -> dict(batch_idx, cls, bboxes, keypoints (or None), count), all `capacity` rows long."""
    srcs, items = np.ascontiguousarray(srcs, SRC_DTYPE), np.ascontiguousarray(items, ITEM_DTYPE)
    lab_off = np.ascontiguousarray(lab_off, np.int32)
    cls, boxes = np.ascontiguousarray(cls, np.float32), np.ascontiguousarray(boxes, np.float32)
    kp = np.ascontiguousarray(keypoints, np.float32) if keypoints is not None else None
    K = kp.shape[1] if kp is not None else 0
    cap = int(capacity if capacity is not None else max(1, int(lab_off[-1])))
    n = max(cap, 0)
    out = dict(batch_idx=np.empty((n,), np.float32), cls=np.empty((n,), np.float32), bboxes=np.empty((n, 4), np.float32),
               keypoints=np.empty((n, K, 3), np.float32) if kp is not None else None)
    cnt = C.c_int32(-1)
    _lib.check(engine.lib, engine.lib.ys_augment_labels(engine.ctx, _ptr(srcs), _ptr(lab_off), _ptr(cls), _ptr(boxes), _ptr(kp), K, int(kpt_dim), _ptr(items),
                                                        items.shape[0], 0, int(imgsz), int(bool(perspective)), int(flags), cap, _ptr(out["batch_idx"]),
                                                        _ptr(out["cls"]), _ptr(out["bboxes"]), _ptr(out["keypoints"]), C.byref(cnt)))
    out["count"] = cnt.value
    return out


def augment_labels_obb(engine, srcs, lab_off, cls, boxes, corners, items, imgsz, perspective=False, flags=0, capacity=None):
    """ys_augment_labels_obb on HOST arrays: -> dict(batch_idx, cls, bboxes [capacity, 5], count)."""
    srcs, items = np.ascontiguousarray(srcs, SRC_DTYPE), np.ascontiguousarray(items, ITEM_DTYPE)
    lab_off = np.ascontiguousarray(lab_off, np.int32)
    cls, boxes, corners = (np.ascontiguousarray(a, np.float32) for a in (cls, boxes, corners))
    cap = int(capacity if capacity is not None else max(1, int(lab_off[-1])))
    n = max(cap, 0)
    out = dict(batch_idx=np.empty((n,), np.float32), cls=np.empty((n,), np.float32), bboxes=np.empty((n, 5), np.float32))
    cnt = C.c_int32(-1)
    _lib.check(engine.lib, engine.lib.ys_augment_labels_obb(engine.ctx, _ptr(srcs), _ptr(lab_off), _ptr(cls), _ptr(boxes), _ptr(corners), _ptr(items), items.shape[0], 0,
                                                            int(imgsz), int(bool(perspective)), int(flags), cap, _ptr(out["batch_idx"]), _ptr(out["cls"]),
                                                            _ptr(out["bboxes"]), C.byref(cnt)))
    out["count"] = cnt.value
    return out


def augment_letterbox_labels_obb(engine, srcs, lab_off, cls, boxes, corners, items, imgsz, flags=0, capacity=None):
    """ys_augment_letterbox_labels_obb on HOST arrays: -> dict(batch_idx, cls, bboxes [capacity, 5], count)."""
    srcs, items = np.ascontiguousarray(srcs, SRC_DTYPE), np.ascontiguousarray(items, ITEM_DTYPE)
    lab_off = np.ascontiguousarray(lab_off, np.int32)
    assert lab_off.shape[0] == srcs.shape[0] + 1, (lab_off.shape, srcs.shape)
    cls, boxes, corners = (np.ascontiguousarray(a, np.float32) for a in (cls, boxes, corners))
    cap = int(capacity if capacity is not None else max(1, int(lab_off[-1])))
    n = max(cap, 0)
    out = dict(batch_idx=np.empty((n,), np.float32), cls=np.empty((n,), np.float32), bboxes=np.empty((n, 5), np.float32))
    cnt = C.c_int32(-1)
    _lib.check(engine.lib, engine.lib.ys_augment_letterbox_labels_obb(engine.ctx, _ptr(srcs), srcs.shape[0], _ptr(lab_off), _ptr(cls), _ptr(boxes), _ptr(corners),
                                                                      _ptr(items), items.shape[0], 0, int(imgsz), int(flags), cap, _ptr(out["batch_idx"]),
                                                                      _ptr(out["cls"]), _ptr(out["bboxes"]), C.byref(cnt)))
    out["count"] = cnt.value
    return out


def augment_letterbox(engine, arena, srcs, items, imgsz, mask_ratio=4, with_masks=False, jitter=None):
    """ys_augment_letterbox (jitter rows given: ys_augment_letterbox_jitter) on HOST arrays: -> (images fp32 [B, 3, s, s], masks fp32 [B, s/r, s/r] or None).
    Reads src[0] and the flips of an item."""
    arena = np.ascontiguousarray(arena, np.uint8)
    srcs, items = np.ascontiguousarray(srcs, SRC_DTYPE), np.ascontiguousarray(items, ITEM_DTYPE)
    B, s = items.shape[0], int(imgsz)
    images = np.empty((B, 3, max(s, 0), max(s, 0)), np.float32)
    masks = np.empty((B, s // mask_ratio, s // mask_ratio), np.float32) if with_masks else None
    if jitter is None:
        _lib.check(engine.lib, engine.lib.ys_augment_letterbox(engine.ctx, _ptr(arena), _ptr(srcs), srcs.shape[0], _ptr(items), B, 0, s, int(mask_ratio),
                                                               _ptr(images), _ptr(masks)))
    else:
        jitter = np.ascontiguousarray(jitter, JITTER_DTYPE)
        assert jitter.shape == (B,), jitter.shape
        _lib.check(engine.lib, engine.lib.ys_augment_letterbox_jitter(engine.ctx, _ptr(arena), _ptr(srcs), srcs.shape[0], _ptr(items), B, 0, s, int(mask_ratio),
                                                                      _ptr(jitter), _ptr(images), _ptr(masks)))
    return images, masks


def augment_letterbox_labels(engine, srcs, lab_off, cls, boxes, keypoints, items, imgsz, flags=0, capacity=None, kpt_dim=3):
    """ys_augment_letterbox_labels on HOST arrays: -> dict(batch_idx, cls, bboxes, keypoints (or None), count), all `capacity` rows long."""
    srcs, items = np.ascontiguousarray(srcs, SRC_DTYPE), np.ascontiguousarray(items, ITEM_DTYPE)
    lab_off = np.ascontiguousarray(lab_off, np.int32)
    assert lab_off.shape[0] == srcs.shape[0] + 1, (lab_off.shape, srcs.shape)
    cls, boxes = np.ascontiguousarray(cls, np.float32), np.ascontiguousarray(boxes, np.float32)
    kp = np.ascontiguousarray(keypoints, np.float32) if keypoints is not None else None
    K = kp.shape[1] if kp is not None else 0
    cap = int(capacity if capacity is not None else max(1, int(lab_off[-1])))
    n = max(cap, 0)
    out = dict(batch_idx=np.empty((n,), np.float32), cls=np.empty((n,), np.float32), bboxes=np.empty((n, 4), np.float32),
               keypoints=np.empty((n, K, 3), np.float32) if kp is not None else None)
    cnt = C.c_int32(-1)
    _lib.check(engine.lib, engine.lib.ys_augment_letterbox_labels(engine.ctx, _ptr(srcs), srcs.shape[0], _ptr(lab_off), _ptr(cls), _ptr(boxes), _ptr(kp), K,
                                                                  int(kpt_dim), _ptr(items), items.shape[0], 0, int(imgsz), int(flags), cap,
                                                                  _ptr(out["batch_idx"]), _ptr(out["cls"]), _ptr(out["bboxes"]), _ptr(out["keypoints"]),
                                                                  C.byref(cnt)))
    out["count"] = cnt.value
    return out


def draw_letterbox_items(rng, indices, fliplr=0.5, flipud=0.0, hsv=None):
    """The item table of one close-mosaic batch: per primary index only what FlipLR, then FlipUD draw (`rand > p -> skip`, each drawn only when its
    p > 0: YoloDataset.cs:406-415); LetterBox draws nothing.  The other fields stay zero (src[1..3] = 0: valid, unread).
    hsv = (hgain, sgain, vgain): RandomHSV follows the flips (:416) -- per image one draw_jitter row after the two flip draws; -> (items, rows)."""
    items = make_items(len(indices))
    rows = make_jitter(len(indices)) if hsv is not None else None
    for b, idx in enumerate(indices):
        flr = fliplr > 0 and not (rng.random() > fliplr)
        fud = flipud > 0 and not (rng.random() > flipud)
        items[b]["src"][0], items[b]["flip_lr"], items[b]["flip_ud"] = int(idx), int(flr), int(fud)
        if hsv is not None:
            rows[b] = draw_jitter(rng, 1, *hsv)[0]
    return items if hsv is None else (items, rows)


def draw_items(rng, indices, s, count, hyp, fliplr=0.5, flipud=0.0, hsv=None):
    """The item table of one batch: per primary index of `indices`, in the reference's per-image order, the three mixed indices as
    randint(0, count - 1) (:155), yc, then xc, in [s/2, 3s/2) (:163-164), the eight uniforms of the matrix, FlipLR then FlipUD as `rand > p -> skip`
    (drawn only when p > 0).  hyp: degrees / translate / scale / shear / perspective.  The matrices are built for the whole batch at once.
    hsv = (hgain, sgain, vgain): RandomHSV follows the flips (YoloDataset.cs:86) -- per image one draw_jitter row after the two flip draws; -> (items, rows)."""
    items = make_items(len(indices))
    rows = make_jitter(len(indices)) if hsv is not None else None
    u = np.empty((len(indices), 8), np.float64)
    for b, idx in enumerate(indices):
        mix = rng.integers(0, count - 1, size=3)
        yc = int(rng.integers(s // 2, 2 * s - s // 2))
        xc = int(rng.integers(s // 2, 2 * s - s // 2))
        u[b] = rng.random(8)
        flr = fliplr > 0 and not (rng.random() > fliplr)
        fud = flipud > 0 and not (rng.random() > flipud)
        items[b] = ((int(idx), int(mix[0]), int(mix[1]), int(mix[2])), xc, yc, 0.0, int(flr), int(fud))
        if hsv is not None:
            rows[b] = draw_jitter(rng, 1, *hsv)[0]
    items["M"] = perspective_matrices(u, s, **hyp).reshape(-1, 9)
    return items if hsv is None else (items, rows)


class DeviceBatch:
    """One collated training batch that lives in HBM: device pointers to images fp32 [B, 3, s, s], batch_idx / cls [capacity], bboxes [capacity, box_dim]
    (box_dim 4: cxcywh; 5: an OBB batch's cx, cy, w, h, angle), masks [B, s/r, s/r] and keypoints [capacity, K, 3] (None when absent) and the device int `count`.  Rows [count, capacity) carry batch_idx -1,
    which the criteria skip: n_labels = capacity, no host read.  n_input = the labels of the batch's tiles BEFORE the filters (a host number; in the
    LetterBox branch, which filters nothing, the batch's exact label count).  mode = the branch that produced it: "mosaic" or "letterbox"."""

    def __init__(self, engine, batch, imgsz, capacity, images, batch_idx, cls, bboxes, count, masks=None, keypoints=None, kpt_num=0, mask_ratio=4,
                 n_input=0, max_per_image=64, mode="mosaic", box_dim=4):
        self.mode, self.box_dim = mode, int(box_dim)
        self.engine, self.batch, self.imgsz, self.capacity = engine, batch, imgsz, capacity
        self.images, self.batch_idx, self.cls, self.bboxes, self.count = images, batch_idx, cls, bboxes, count
        self.masks, self.keypoints, self.kpt_num, self.mask_ratio, self.n_input = masks, keypoints, kpt_num, mask_ratio, n_input
        self.max_per_image = max_per_image      # upper bound of one image's label count (the criterion's per-image workspace is reserved for it)

    def to_host(self):
        """The same batch as the numpy dict the host path takes (synchronises): the first `count` rows."""
        e, s, cap = self.engine, self.imgsz, self.capacity
        n = int(e.from_device(self.count, (1,), np.int32)[0])
        if n > cap:
            raise _lib.YsError(1, "augmenter kept %d labels, capacity is %d" % (n, cap))
        out = dict(images=e.from_device(self.images, (self.batch, 3, s, s), np.float32),
                   batch_idx=e.from_device(self.batch_idx, (cap,), np.float32)[:n], cls=e.from_device(self.cls, (cap,), np.float32)[:n],
                   bboxes=e.from_device(self.bboxes, (cap, self.box_dim), np.float32)[:n])
        if self.masks is not None:
            out["masks"] = e.from_device(self.masks, (self.batch, s // self.mask_ratio, s // self.mask_ratio), np.float32)
        if self.keypoints is not None:
            out["keypoints"] = e.from_device(self.keypoints, (cap, self.kpt_num, 3), np.float32)[:n]
        return out


class MosaicAugmenter:
    """Mosaic4 + RandomPerspective + FlipLR / FlipUD + Normalize + collate per batch on the device.  The dataset -- uint8 RGB planes [3, h, w], optional
    id masks [mh, mw], per-image labels {cls, bboxes pixel xyxy, keypoints [n, K, 3]} -- is uploaded ONCE; a batch uploads its item table only.
    Draws per output image, in the reference's order, from one numpy Generator: the three mixed indices as randint(0, Count - 1) (:155: the upper bound is
    exclusive, so the LAST image is never mixed in -- kept); yc, then xc, in [s/2, 3s/2) (:163-164); the matrix (random_perspective_matrix); FlipLR then
    FlipUD as `rand > p -> skip`, drawn only when p > 0 (YoloDataset.cs:76-85).  The output buffers are reused by the next batch.
    close_mosaic(True) switches to the reference's closed pipeline (YoloDataset.CloseMosaic): LetterBox + FlipLR / FlipUD of the primary image alone, on the
    same buffers; per image it draws the two flip uniforms only.  `mode` names the branch the next batch comes from.  Of `flags`, the Mosaic branch takes
    YS_AUG_SORT_FLIPPED and the LetterBox branch YS_AUG_FLIP_KEEP_SIZE; each ignores the other's (ys_augment_labels refuses flags it does not know, so
    the LetterBox flag is not handed to it).
    hsv = (hgain, sgain, vgain) -- the reference's default is (0.015, 0.7, 0.4) -- adds RandomHSV to both branches: draw() then returns (items, rows) with
    one ColorJitter row per image, drawn after the image's two flip draws (draw_jitter), run(items, rows) uploads the rows beside the item table and calls the
    *_jitter entries.  hsv = None (the default) draws nothing more and calls the plain entries.
    OBB: labels that carry "obb" [n, 4, 2] pixel corners ("bboxes" may be left out: pack_labels) are uploaded once beside the boxes, the batch's boxes are
    [capacity, 5] and both branches call the *_obb label entries.  Those take no flags, and an OBB label has neither masks nor keypoints: each is refused."""

    def __init__(self, engine, images_u8, labels, imgsz, masks=None, mask_ratio=4, degrees=0.0, translate=0.1, scale=0.5, shear=0.0, perspective=0.0,
                 fliplr=0.5, flipud=0.0, seed=0, flags=0, max_batch=64, hsv=None):
        assert len(images_u8) == len(labels) and len(images_u8) >= 2
        self.hsv = tuple(float(g) for g in hsv) if hsv is not None else None
        assert self.hsv is None or len(self.hsv) == 3
        self.engine, self.s, self.r, self.flags = engine, int(imgsz), int(mask_ratio), int(flags)
        self.hyp = dict(degrees=degrees, translate=translate, scale=scale, shear=shear, perspective=perspective)
        self.fliplr, self.flipud = float(fliplr), float(flipud)
        self.rng = np.random.default_rng(seed)
        self.mode = "mosaic"
        arena, self.srcs = pack_sources(images_u8, masks)
        self.lab_off, cls, boxes, kp = pack_labels(labels)
        obb = pack_obb(labels)
        if obb is not None and (self.flags != 0 or masks is not None or kp is not None):
            raise ValueError("OBB labels take flags = 0 (the box-flip switches have nothing to act on) and neither masks nor keypoints")
        if obb is not None and obb.shape[0] != boxes.shape[0]:
            raise ValueError("every source's labels must carry \"obb\" corners, or none")
        self.obb, self.box_dim = obb is not None, (5 if obb is not None else 4)
        self.count = len(images_u8)
        self.with_masks, self.K = masks is not None, (kp.shape[1] if kp is not None else 0)
        e = engine
        self._static = [e.to_device(arena), e.to_device(self.srcs), e.to_device(self.lab_off), e.to_device(cls if cls.size else np.zeros(1, np.float32)),
                        e.to_device(boxes if boxes.size else np.zeros(4, np.float32))]
        self.d_arena, self.d_srcs, self.d_lab_off, self.d_cls, self.d_boxes = self._static
        self.d_kp = e.to_device(kp if kp.size else np.zeros(3, np.float32)) if kp is not None else None
        self.d_obb = e.to_device(obb if obb.size else np.zeros(8, np.float32)) if self.obb else None
        per_src = np.diff(self.lab_off)
        self.max_batch = int(max_batch)
        self.max_per_image = max(1, int(np.sort(per_src)[::-1][:4].sum()))                  # four tiles per image
        self.capacity = self.max_per_image * self.max_batch                                 # no batch can exceed it
        s, cap, B = self.s, self.capacity, self.max_batch
        self.d_items = e.malloc(B * ITEM_DTYPE.itemsize)
        self.d_jitter = e.malloc(B * JITTER_DTYPE.itemsize) if self.hsv is not None else None
        self.d_images = e.malloc(B * 3 * s * s * 4)
        self.d_masks = e.malloc(B * (s // self.r) ** 2 * 4) if self.with_masks else None
        self.d_bidx, self.d_ocls, self.d_obox, self.d_cnt = e.malloc(cap * 4), e.malloc(cap * 4), e.malloc(cap * 4 * self.box_dim), e.malloc(4)
        self.d_okp = e.malloc(cap * self.K * 12) if self.K else None

    def close(self):
        e = self.engine
        for p in self._static + [self.d_kp, self.d_obb, self.d_items, self.d_jitter, self.d_images, self.d_masks, self.d_bidx, self.d_ocls, self.d_obox, self.d_cnt, self.d_okp]:
            if p is not None:
                e.free(p)
        self._static = []
        self.d_kp = self.d_obb = self.d_items = self.d_jitter = self.d_images = self.d_masks = self.d_bidx = self.d_ocls = self.d_obox = self.d_cnt = self.d_okp = None

    def close_mosaic(self, closed):
        """YoloDataset.CloseMosaic(closed): True = the LetterBox pipeline from the next batch on, False = back to Mosaic + RandomPerspective."""
        self.mode = "letterbox" if closed else "mosaic"

    def draw(self, indices):
        """The item table for the primary dataset indices `indices` (what the data loader's shuffler hands to GetTensor); with hsv: (items, jitter rows)."""
        if self.mode == "letterbox":
            return draw_letterbox_items(self.rng, indices, self.fliplr, self.flipud, self.hsv)
        return draw_items(self.rng, indices, self.s, self.count, self.hyp, self.fliplr, self.flipud, self.hsv)

    def _upload_jitter(self, jitter, B):
        """Validate the rows on the host (the device cannot refuse them aloud) and upload them beside the item table."""
        e = self.engine
        jitter = check_jitter(jitter)
        if jitter.shape != (B,):
            raise ValueError("%d jitter rows for %d items" % (jitter.shape[0], B))
        if self.d_jitter is None:
            self.d_jitter = e.malloc(self.max_batch * JITTER_DTYPE.itemsize)
        _lib.check(e.lib, e.lib.ys_memcpy_h2d(e.ctx, self.d_jitter, _ptr(jitter), jitter.nbytes))
        return self.d_jitter

    def _run_letterbox(self, items, jitter=None):
        e, lib, B = self.engine, self.engine.lib, int(items.shape[0])
        if items["src"][:, 0].min() < 0 or items["src"][:, 0].max() >= self.count:
            raise ValueError("item source index outside [0, %d)" % self.count)
        _lib.check(lib, lib.ys_memcpy_h2d(e.ctx, self.d_items, _ptr(items), items.nbytes))
        if jitter is None:
            _lib.check(lib, lib.ys_augment_letterbox(e.ctx, self.d_arena, self.d_srcs, self.count, self.d_items, B, 1, self.s, self.r, self.d_images, self.d_masks))
        else:
            _lib.check(lib, lib.ys_augment_letterbox_jitter(e.ctx, self.d_arena, self.d_srcs, self.count, self.d_items, B, 1, self.s, self.r,
                                                            self._upload_jitter(jitter, B), self.d_images, self.d_masks))
        if self.obb:
            _lib.check(lib, lib.ys_augment_letterbox_labels_obb(e.ctx, self.d_srcs, self.count, self.d_lab_off, self.d_cls, self.d_boxes, self.d_obb, self.d_items, B, 1,
                                                                self.s, 0, self.capacity, self.d_bidx, self.d_ocls, self.d_obox, self.d_cnt))
        else:
            _lib.check(lib, lib.ys_augment_letterbox_labels(e.ctx, self.d_srcs, self.count, self.d_lab_off, self.d_cls, self.d_boxes, self.d_kp, self.K, 3, self.d_items,
                                                            B, 1, self.s, self.flags, self.capacity, self.d_bidx, self.d_ocls, self.d_obox,
                                                            self.d_okp, self.d_cnt))
        n_input = int(sum(int(self.lab_off[k + 1] - self.lab_off[k]) for k in items["src"][:, 0]))      # nothing is filtered: the exact label count
        return DeviceBatch(e, B, self.s, self.capacity, self.d_images, self.d_bidx, self.d_ocls, self.d_obox, self.d_cnt, masks=self.d_masks,
                           keypoints=self.d_okp, kpt_num=self.K, mask_ratio=self.r, n_input=n_input, max_per_image=self.max_per_image, mode="letterbox", box_dim=self.box_dim)

    def run(self, items, jitter=None):
        """Upload `items` (and the ColorJitter rows `jitter`, one per item; None = no jitter) and launch the kernels of the current branch (`mode`) on the
        engine's stream (asynchronous) -> DeviceBatch."""
        e, lib, B = self.engine, self.engine.lib, int(items.shape[0])
        assert 0 < B <= self.max_batch
        items = np.ascontiguousarray(items, ITEM_DTYPE)
        if self.mode == "letterbox":
            return self._run_letterbox(items, jitter)
        if items["src"].min() < 0 or items["src"].max() >= self.count:      # ys_augment_labels has no source count to check device items against
            raise ValueError("item source index outside [0, %d)" % self.count)
        persp = int(self.hyp["perspective"] > 0)
        _lib.check(lib, lib.ys_memcpy_h2d(e.ctx, self.d_items, _ptr(items), items.nbytes))
        if jitter is None:
            _lib.check(lib, lib.ys_augment_mosaic(e.ctx, self.d_arena, self.d_srcs, self.count, self.d_items, B, 1, self.s, self.r, persp, self.d_images, self.d_masks))
        else:
            _lib.check(lib, lib.ys_augment_mosaic_jitter(e.ctx, self.d_arena, self.d_srcs, self.count, self.d_items, B, 1, self.s, self.r, persp,
                                                         self._upload_jitter(jitter, B), self.d_images, self.d_masks))
        if self.obb:
            _lib.check(lib, lib.ys_augment_labels_obb(e.ctx, self.d_srcs, self.d_lab_off, self.d_cls, self.d_boxes, self.d_obb, self.d_items, B, 1, self.s, persp, 0,
                                                      self.capacity, self.d_bidx, self.d_ocls, self.d_obox, self.d_cnt))
        else:
            _lib.check(lib, lib.ys_augment_labels(e.ctx, self.d_srcs, self.d_lab_off, self.d_cls, self.d_boxes, self.d_kp, self.K, 3, self.d_items, B, 1, self.s, persp,
                                                  self.flags & ~YS_AUG_FLIP_KEEP_SIZE, self.capacity, self.d_bidx, self.d_ocls, self.d_obox, self.d_okp, self.d_cnt))
        n_input = int(sum(int(self.lab_off[k + 1] - self.lab_off[k]) for k in items["src"].reshape(-1)))
        return DeviceBatch(e, B, self.s, self.capacity, self.d_images, self.d_bidx, self.d_ocls, self.d_obox, self.d_cnt, masks=self.d_masks,
                           keypoints=self.d_okp, kpt_num=self.K, mask_ratio=self.r, n_input=n_input, max_per_image=self.max_per_image, box_dim=self.box_dim)

    def batch(self, indices):
        drawn = self.draw(indices)
        return self.run(*drawn) if self.hsv is not None else self.run(drawn)

    def batches(self, batch_size, shuffle=True, drop_last=True):
        """One epoch: the primary indices in (shuffled) order, `batch_size` at a time."""
        order = self.rng.permutation(self.count) if shuffle else np.arange(self.count)
        for i in range(0, self.count, batch_size):
            idx = order[i:i + batch_size]
            if len(idx) < batch_size and drop_last:
                break
            yield self.batch(idx)


# ---------------------------------------------------------------------------------------------------- the classification input
def make_classify_items(n):
    return np.zeros((n,), CLS_ITEM_DTYPE)


def check_classify_items(items, srcs, s):
    """The library's item check (include/yolosharp_hip.h ys_augment_classify) on the host: ValueError naming the first invalid item."""
    items, srcs = np.ascontiguousarray(items, CLS_ITEM_DTYPE), np.ascontiguousarray(srcs, SRC_DTYPE)
    it = {k: items[k].astype(np.int64) for k in CLS_ITEM_DTYPE.names}
    ok = (it["src"] >= 0) & (it["src"] < srcs.shape[0])
    sr = srcs[np.where(ok, it["src"], 0)] if srcs.shape[0] else np.zeros(items.shape, SRC_DTYPE)
    H, W = sr["h"].astype(np.int64), sr["w"].astype(np.int64)
    ok &= (H >= 1) & (W >= 1) & (sr["img_off"] >= 0)
    ok &= (it["ch"] >= 1) & (it["cw"] >= 1) & (it["top"] >= 0) & (it["left"] >= 0) & (it["top"] + it["ch"] <= H) & (it["left"] + it["cw"] <= W)
    ok &= (it["oh"] >= 1) & (it["ow"] >= 1) & (it["oy"] >= 0) & (it["ox"] >= 0) & (it["oy"] + s <= it["oh"]) & (it["ox"] + s <= it["ow"])
    ok &= ((it["flip_lr"] == 0) | (it["flip_lr"] == 1)) & ((it["flip_ud"] == 0) | (it["flip_ud"] == 1))
    none = (it["er_y"] == 0) & (it["er_x"] == 0) & (it["er_h"] == 0) & (it["er_w"] == 0)
    ok &= none | ((it["er_h"] >= 1) & (it["er_w"] >= 1) & (it["er_y"] >= 0) & (it["er_x"] >= 0) & (it["er_y"] + it["er_h"] <= s) & (it["er_x"] + it["er_w"] <= s))
    if not ok.all():
        b = int(np.argmin(ok))
        raise ValueError("classify item %d is invalid: %s" % (b, {k: int(items[b][k]) for k in CLS_ITEM_DTYPE.names}))
    return items


def _resized_crop_params(rng, H, W, scale, ratio):
    """torchvision RandomResizedCrop.get_params: (top, left, h, w)."""
    area = H * W
    lo, hi = math.log(ratio[0]), math.log(ratio[1])
    for _ in range(10):
        target = area * (scale[0] + (scale[1] - scale[0]) * rng.random())
        aspect = math.exp(lo + (hi - lo) * rng.random())
        w, h = int(round(math.sqrt(target * aspect))), int(round(math.sqrt(target / aspect)))
        if 0 < w <= W and 0 < h <= H:
            return int(rng.integers(0, H - h + 1)), int(rng.integers(0, W - w + 1)), h, w
    in_ratio = W / H                                                       # the centre fallback with the ratio clamp
    if in_ratio < min(ratio):
        w = W
        h = int(round(w / min(ratio)))
    elif in_ratio > max(ratio):
        h = H
        w = int(round(h * max(ratio)))
    else:
        w, h = W, H
    h, w = min(max(h, 1), H), min(max(w, 1), W)
    return (H - h) // 2, (W - w) // 2, h, w


def _erasing_params(rng, s, p, gate):
    """The reference's RandomErasing (ClassificationDataset.cs:166-226) on the s x s image: (er_y, er_x, er_h, er_w, er_seed), zeros for no erase."""
    g = rng.standard_normal() if gate == "normal" else rng.random()
    if g > p:                                                              # :218 (a NORMAL draw there)
        return 0, 0, 0, 0, 0
    lo, hi = math.log(0.3), math.log(3.3)
    for _ in range(10):
        area = s * s * (0.02 + (0.33 - 0.02) * rng.random())
        aspect = math.exp(lo + (hi - lo) * rng.random())
        h, w = int(round(math.sqrt(area * aspect))), int(round(math.sqrt(area / aspect)))      # Math.Round: half to even, like Python's
        if not (h < s and w < s):                                          # :201, strict
            continue
        seed = int(rng.integers(0, 2 ** 32, dtype=np.uint64))              # in the slot of the reference's noise tensor (:206)
        y, x = int(rng.integers(s - h + 1)), int(rng.integers(s - w + 1))
        if h < 1 or w < 1:                                                 # an empty rectangle erases nothing
            return 0, 0, 0, 0, 0
        return y, x, h, w, seed
    return 0, 0, 0, 0, 0                                                   # :213: the image erased with itself


def draw_classify_items(rng, indices, shapes, s, scale=(0.08, 1.0), ratio=(3 / 4, 4 / 3), fliplr=0.5, flipud=0.0, erasing=0.4, hsv=(0.015, 0.7, 0.4),
                        erasing_gate="normal", auto_augment=None):
    """The item table of one classification training batch (ClassificationDataset.build_transforms, :95-122, Auto_Augment = None): per index of `indices`,
    from ONE stream in the reference's order, what RandomResizedCrop.get_params draws for the source's shapes[idx] = (H, W) -- ten tries of
    target = H * W * U(scale), aspect = exp(U(log ratio)), accepted iff 0 < w <= W and 0 < h <= H, then top and left; else the centre fallback --
    RandomHorizontalFlip, then RandomVerticalFlip (each drawn only when its p > 0; flip iff rand < p), RandomErasing (only when erasing > 0; its gate is a
    NORMAL draw, `randn > p` skips: at p = 0.4 an image is erased with probability 0.655, kept; erasing_gate = "uniform" gives `rand > p`), and one
    draw_jitter row with contrast = vgain (only when hsv is not None).  -> (items, jitter rows or None).
    auto_augment = an AutoAugment / RandAugment policy object: the image's ys_aa_row (draw_auto_augment on the s x s image) is drawn in the reference's
    position, after the flips and in front of the erasing draws (:105-120) -> (items, jitter rows or None, aa rows).  None draws nothing and returns the pair."""
    assert erasing_gate in ("normal", "uniform"), erasing_gate
    s = int(s)
    items = make_classify_items(len(indices))
    rows = make_jitter(len(indices)) if hsv is not None else None
    aa = make_aa_rows(len(indices)) if auto_augment is not None else None
    for b, idx in enumerate(indices):
        H, W = (int(v) for v in shapes[int(idx)])
        top, left, ch, cw = _resized_crop_params(rng, H, W, scale, ratio)
        flr = fliplr > 0 and rng.random() < fliplr
        fud = flipud > 0 and rng.random() < flipud
        if auto_augment is not None:
            aa[b] = draw_auto_augment(rng, 1, (s, s), auto_augment)[0]
        er = _erasing_params(rng, s, erasing, erasing_gate) if erasing > 0 else (0, 0, 0, 0, 0)
        items[b] = (int(idx), top, left, ch, cw, s, s, 0, 0, int(flr), int(fud)) + er
        if hsv is not None:
            hgain, sgain, vgain = hsv
            rows[b] = draw_jitter(rng, 1, hgain, sgain, vgain, cgain=vgain)[0]
    return (items, rows) if auto_augment is None else (items, rows, aa)


def draw_classify_val_items(indices, shapes, s):
    """The val chain's items (:126-127), nothing random: torchvision Resize(int) -- the smaller edge to s, the other to int(s * long / short) -- then
    CenterCrop(s) at int(round((size - s) / 2.0)).  No flips, no erase; run them without jitter rows."""
    s = int(s)
    items = make_classify_items(len(indices))
    for b, idx in enumerate(indices):
        H, W = (int(v) for v in shapes[int(idx)])
        oh, ow = (s, int(s * W / H)) if H <= W else (int(s * H / W), s)
        items[b] = (int(idx), 0, 0, H, W, oh, ow, int(round((oh - s) / 2.0)), int(round((ow - s) / 2.0)), 0, 0, 0, 0, 0, 0, 0)
    return items


# ---------------------------------------------------------------------------------------------------- AutoAugment / RandAugment
# torchvision.transforms.AutoAugment / RandAugment (autoaugment.py) as the host's draws: the op ids are _augmentation_space's order, -1 = nothing.
AA_OPS = ("ShearX", "ShearY", "TranslateX", "TranslateY", "Rotate", "Brightness", "Color", "Contrast", "Sharpness", "Posterize", "Solarize", "AutoContrast",
          "Equalize", "Invert")
AA_ID = {name: i for i, name in enumerate(AA_OPS)}
AA_NONE = -1
AA_SIGNED = frozenset(("ShearX", "ShearY", "TranslateX", "TranslateY", "Rotate", "Brightness", "Color", "Contrast", "Sharpness"))
# AutoAugmentPolicy.IMAGENET: ((op, p, magnitude id or None), (op, p, magnitude id or None)); the last five repeat earlier rows, as in torchvision
IMAGENET_POLICY = (
    (("Posterize", 0.4, 8), ("Rotate", 0.6, 9)), (("Solarize", 0.6, 5), ("AutoContrast", 0.6, None)), (("Equalize", 0.8, None), ("Equalize", 0.6, None)),
    (("Posterize", 0.6, 7), ("Posterize", 0.6, 6)), (("Equalize", 0.4, None), ("Solarize", 0.2, 4)), (("Equalize", 0.4, None), ("Rotate", 0.8, 8)),
    (("Solarize", 0.6, 3), ("Equalize", 0.6, None)), (("Posterize", 0.8, 5), ("Equalize", 1.0, None)), (("Rotate", 0.2, 3), ("Solarize", 0.6, 8)),
    (("Equalize", 0.6, None), ("Posterize", 0.4, 6)), (("Rotate", 0.8, 8), ("Color", 0.4, 0)), (("Rotate", 0.4, 9), ("Equalize", 0.6, None)),
    (("Equalize", 0.0, None), ("Equalize", 0.8, None)), (("Invert", 0.6, None), ("Equalize", 1.0, None)), (("Color", 0.6, 4), ("Contrast", 1.0, 8)),
    (("Rotate", 0.8, 8), ("Color", 1.0, 2)), (("Color", 0.8, 8), ("Solarize", 0.8, 7)), (("Sharpness", 0.4, 7), ("Invert", 0.6, None)),
    (("ShearX", 0.6, 5), ("Equalize", 1.0, None)), (("Color", 0.4, 0), ("Equalize", 0.6, None)), (("Equalize", 0.4, None), ("Solarize", 0.2, 4)),
    (("Solarize", 0.6, 5), ("AutoContrast", 0.6, None)), (("Invert", 0.6, None), ("Equalize", 1.0, None)), (("Color", 0.6, 4), ("Contrast", 1.0, 8)),
    (("Equalize", 0.8, None), ("Equalize", 0.6, None)))
RAND_AUGMENT_OPS = ("Identity", "ShearX", "ShearY", "TranslateX", "TranslateY", "Rotate", "Brightness", "Color", "Contrast", "Sharpness", "Posterize", "Solarize",
                    "AutoContrast", "Equalize")


class AutoAugment:
    """torchvision.transforms.AutoAugment(AutoAugmentPolicy.IMAGENET), what the reference appends for Auto_Augment = AutoAugment
    (Data/ClassificationDataset.cs:105-116): one of 25 sub-policies per image, two ops each with a probability and one of 10 magnitude bins."""
    bins = 10

    def __init__(self, policy=IMAGENET_POLICY):
        self.policy = tuple(policy)
        assert all(len(row) == 2 and all(op in AA_ID and (m is None or 0 <= m < self.bins) for op, _, m in row) for row in self.policy)


class RandAugment:
    """torchvision.transforms.RandAugment(num_ops, magnitude, num_magnitude_bins): num_ops ops drawn uniformly from RAND_AUGMENT_OPS, every one at bin
    `magnitude` of `bins`.  A ys_aa_row has two slots: num_ops is 1 or 2."""

    def __init__(self, num_ops=2, magnitude=9, bins=31):
        if num_ops not in (1, 2):
            raise ValueError("RandAugment(num_ops=%r): an image has two operator slots, num_ops must be 1 or 2" % (num_ops,))
        if not 0 <= int(magnitude) < int(bins):
            raise ValueError("RandAugment(magnitude=%r, bins=%r): the magnitude is a bin index" % (magnitude, bins))
        self.num_ops, self.magnitude, self.bins = int(num_ops), int(magnitude), int(bins)


def _linspace_f32(start, end, steps):
    """torch.linspace(start, end, steps) in fp32: step = (end - start) / (steps - 1) rounded to fp32; the first half counts up from start, the second down
    from end, each value ONE fused multiply-add (the product exact, one rounding) as torch's CPU kernel computes it."""
    f = np.float32
    start, end = f(start), f(end)
    step = np.float64((end - start) / f(steps - 1))
    i = np.arange(steps)
    return np.where(i < steps // 2, np.float64(start) + step * i, np.float64(end) - step * (steps - 1 - i)).astype(f)


def aa_magnitudes(op, bins, h, w):
    """_augmentation_space(bins, (h, w))[op] as Python floats (the fp32 linspace value, then float), or None for an op without a magnitude."""
    m = _aa_magnitudes(op, int(bins), int(h), int(w))
    return list(m) if m is not None else None


@functools.lru_cache(maxsize=None)
def _aa_magnitudes(op, bins, h, w):
    if op in ("ShearX", "ShearY"):
        m = _linspace_f32(0.0, 0.3, bins)
    elif op == "TranslateX":
        m = _linspace_f32(0.0, 150.0 / 331.0 * w, bins)
    elif op == "TranslateY":
        m = _linspace_f32(0.0, 150.0 / 331.0 * h, bins)
    elif op == "Rotate":
        m = _linspace_f32(0.0, 30.0, bins)
    elif op in ("Brightness", "Color", "Contrast", "Sharpness"):
        m = _linspace_f32(0.0, 0.9, bins)
    elif op == "Posterize":
        m = 8 - np.rint(np.arange(bins, dtype=np.float32) / np.float32((bins - 1) / 4)).astype(np.int32)      # torch.round: half to even, like rint
    elif op == "Solarize":
        m = _linspace_f32(255.0, 0.0, bins)
    else:
        return None
    return tuple(float(v) for v in m)


def inverse_affine_matrix(center, angle, translate, scale, shear):
    """torchvision.transforms.functional._get_inverse_affine_matrix in Python floats: the six entries of the inverse of
    T * C * RotateScaleShear * C^-1 (angles in degrees)."""
    rot, sx, sy = math.radians(angle), math.radians(shear[0]), math.radians(shear[1])
    cx, cy = center
    tx, ty = translate
    a = math.cos(rot - sy) / math.cos(sy)
    b = -math.cos(rot - sy) * math.tan(sx) / math.cos(sy) - math.sin(rot)
    c = math.sin(rot - sy) / math.cos(sy)
    d = -math.sin(rot - sy) * math.tan(sx) / math.cos(sy) + math.cos(rot)
    m = [d, -b, 0.0, -c, a, 0.0]
    m = [x / scale for x in m]
    m[2] += m[0] * (-cx - tx) + m[1] * (-cy - ty)
    m[5] += m[3] * (-cx - tx) + m[4] * (-cy - ty)
    m[2] += cx
    m[5] += cy
    return m


def make_aa_rows(n):
    """n rows with both slots empty (op -1, identity theta)."""
    rows = np.zeros((n,), AA_ROW_DTYPE)
    rows["op"] = AA_NONE
    rows["theta"][:] = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)
    return rows


def set_aa_slot(row, k, op, magnitude, hw):
    """Slot k of one row = torchvision's _apply_op(img, op, magnitude) on an image of hw = (h, w): the op id, its argument (1 + m for the blends, the
    bits for Posterize, the threshold for Solarize) and, for the affine ops, the inverse matrix rounded to fp32.  op None / "Identity": nothing."""
    h, w = hw
    row["op"][k], row["arg"][k], row["theta"][k] = AA_NONE, 0.0, (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)
    if op is None or op == "Identity":
        return
    row["op"][k] = AA_ID[op]
    m = float(magnitude)
    if op == "ShearX":
        row["theta"][k] = inverse_affine_matrix([-w * 0.5, -h * 0.5], 0.0, [0.0, 0.0], 1.0, [math.degrees(math.atan(m)), 0.0])
    elif op == "ShearY":
        row["theta"][k] = inverse_affine_matrix([-w * 0.5, -h * 0.5], 0.0, [0.0, 0.0], 1.0, [0.0, math.degrees(math.atan(m))])
    elif op == "TranslateX":
        row["theta"][k] = inverse_affine_matrix([0.0, 0.0], 0.0, [1.0 * int(m), 0.0], 1.0, [0.0, 0.0])
    elif op == "TranslateY":
        row["theta"][k] = inverse_affine_matrix([0.0, 0.0], 0.0, [0.0, 1.0 * int(m)], 1.0, [0.0, 0.0])
    elif op == "Rotate":
        row["theta"][k] = inverse_affine_matrix([0.0, 0.0], -m, [0.0, 0.0], 1.0, [0.0, 0.0])
    elif op in ("Brightness", "Color", "Contrast", "Sharpness"):
        row["arg"][k] = 1.0 + m
    elif op == "Posterize":
        row["arg"][k] = int(m)
    elif op == "Solarize":
        row["arg"][k] = m


def check_aa_rows(rows):
    """The library's row check (include/yolosharp_hip.h ys_aa_row) on the host: ValueError naming the first invalid row."""
    rows = np.ascontiguousarray(rows, AA_ROW_DTYPE)
    ok = ((rows["op"] >= AA_NONE) & (rows["op"] <= 13)).all(axis=1) & np.isfinite(rows["arg"]).all(axis=1) & np.isfinite(rows["theta"]).all(axis=(1, 2))
    ok &= ((rows["op"] != AA_ID["Posterize"]) | ((rows["arg"] >= 0) & (rows["arg"] <= 8))).all(axis=1)
    if not ok.all():
        b = int(np.argmin(ok))
        raise ValueError("aa row %d is invalid: op %s arg %s theta %s" % (b, rows[b]["op"].tolist(), rows[b]["arg"].tolist(), rows[b]["theta"].tolist()))
    return rows


def draw_auto_augment(rng, n, hw, policy):
    """n ys_aa_row for images of hw = (h, w), per image in torchvision's draw order.  AutoAugment.get_params: one sub-policy index, two uniform
    probabilities, two sign bits; slot i runs iff prob[i] <= p; a signed magnitude is negated iff its sign bit is 0.  RandAugment.forward: per op one
    index into RAND_AUGMENT_OPS, then -- only for a signed op -- one bit; the magnitude is negated iff the bit is 1."""
    rows = make_aa_rows(n)
    for b in range(n):
        if isinstance(policy, AutoAugment):
            pid = int(rng.integers(len(policy.policy)))
            probs = rng.random(2)
            signs = rng.integers(0, 2, 2)
            for k, (op, p, mid) in enumerate(policy.policy[pid]):
                if probs[k] <= p:
                    m = _aa_magnitudes(op, policy.bins, int(hw[0]), int(hw[1]))[mid] if mid is not None else 0.0
                    if op in AA_SIGNED and int(signs[k]) == 0:
                        m *= -1.0
                    set_aa_slot(rows[b], k, op, m, hw)
        elif isinstance(policy, RandAugment):
            for k in range(policy.num_ops):
                op = RAND_AUGMENT_OPS[int(rng.integers(len(RAND_AUGMENT_OPS)))]
                mags = _aa_magnitudes(op, policy.bins, int(hw[0]), int(hw[1]))
                m = mags[policy.magnitude] if mags is not None else 0.0
                if op in AA_SIGNED and int(rng.integers(0, 2)):
                    m *= -1.0
                set_aa_slot(rows[b], k, op, m, hw)
        else:
            raise TypeError("auto_augment policy %r: pass augment.AutoAugment() or augment.RandAugment()" % (policy,))
    return rows


def auto_augment_ops(engine, images_u8, rows):
    """ys_auto_augment_ops on HOST arrays: uint8 [B, 3, h, w] through the two slots of each image's row -> uint8 [B, 3, h, w]."""
    img = np.ascontiguousarray(images_u8, np.uint8)
    rows = np.ascontiguousarray(rows, AA_ROW_DTYPE)
    assert img.ndim == 4 and img.shape[1] == 3 and rows.shape == (img.shape[0],), (img.shape, rows.shape)
    out = np.empty_like(img)
    _lib.check(engine.lib, engine.lib.ys_auto_augment_ops(engine.ctx, _ptr(img), img.shape[0], img.shape[2], img.shape[3], _ptr(rows), 0, _ptr(out)))
    return out


def augment_classify(engine, arena, srcs, src_cls, items, imgsz, jitter=None, aa=None):
    """ys_augment_classify (aa = None) / ys_augment_classify_aa (aa = the batch's ys_aa_row table) on HOST arrays: -> (images fp32 [B, 3, s, s], cls fp32 [B])."""
    arena = np.ascontiguousarray(arena, np.uint8)
    srcs, items = np.ascontiguousarray(srcs, SRC_DTYPE), np.ascontiguousarray(items, CLS_ITEM_DTYPE)
    src_cls = np.ascontiguousarray(src_cls, np.float32).reshape(-1)
    assert src_cls.shape[0] == srcs.shape[0], (src_cls.shape, srcs.shape)
    B, s = items.shape[0], int(imgsz)
    if jitter is not None:
        jitter = np.ascontiguousarray(jitter, JITTER_DTYPE)
        assert jitter.shape == (B,), jitter.shape
    images, cls = np.empty((B, 3, max(s, 0), max(s, 0)), np.float32), np.empty((B,), np.float32)
    if aa is not None:
        aa = np.ascontiguousarray(aa, AA_ROW_DTYPE)
        assert aa.shape == (B,), aa.shape
        _lib.check(engine.lib, engine.lib.ys_augment_classify_aa(engine.ctx, _ptr(arena), _ptr(srcs), srcs.shape[0], _ptr(src_cls), _ptr(items), B, 0, s, _ptr(aa),
                                                                 _ptr(jitter), _ptr(images), _ptr(cls)))
        return images, cls
    _lib.check(engine.lib, engine.lib.ys_augment_classify(engine.ctx, _ptr(arena), _ptr(srcs), srcs.shape[0], _ptr(src_cls), _ptr(items), B, 0, s, _ptr(jitter),
                                                          _ptr(images), _ptr(cls)))
    return images, cls


class ClassifyDeviceBatch:
    """One classification batch that lives in HBM: device pointers to images fp32 [batch, 3, imgsz, imgsz] and cls fp32 [batch] (one class id per image).
    mode = the chain that produced it: "train" or "val"."""

    def __init__(self, engine, batch, imgsz, images, cls, mode="train"):
        self.engine, self.batch, self.imgsz, self.images, self.cls, self.mode = engine, int(batch), int(imgsz), images, cls, mode

    def to_host(self):
        """The same batch as the numpy dict the host path takes (synchronises): images, cls and the collate's batch_idx = 0 .. batch - 1."""
        e, s = self.engine, self.imgsz
        return dict(images=e.from_device(self.images, (self.batch, 3, s, s), np.float32), cls=e.from_device(self.cls, (self.batch,), np.float32),
                    batch_idx=np.arange(self.batch, dtype=np.float32))


class ClassifyAugmenter:
    """ClassificationDataset's input on the device.  The dataset -- uint8 RGB planes [3, h, w] of any sizes and one class id per image -- is uploaded ONCE;
    a batch uploads its 64-byte items and 32-byte jitter rows only and is one fused gather (ys_augment_classify).  draw() follows draw_classify_items from
    one numpy Generator; val_batches() walks the dataset in order through the val chain.  The output buffers are reused by the next batch.
    erasing = 0 and hsv = None each skip their draws.  auto_augment: None, AutoAugment() (the reference's default) or RandAugment(...) -- a policy OBJECT,
    like the transform the reference appends; then a batch also uploads one 64-byte ys_aa_row per image and runs ys_augment_classify_aa.  A string raises
    NotImplementedError (AugMix has no object: it is not built).  close_mosaic() does nothing -- ClassificationDataset.CloseMosaic is empty -- so Trainer.fit(..., augmenter=this) works unchanged."""

    def __init__(self, engine, images_u8, classes, imgsz, scale=(0.08, 1.0), ratio=(3 / 4, 4 / 3), fliplr=0.5, flipud=0.0, erasing=0.4, hsv=(0.015, 0.7, 0.4),
                 auto_augment=None, seed=0, max_batch=64, erasing_gate="normal"):
        if auto_augment is not None and not isinstance(auto_augment, (AutoAugment, RandAugment)):
            raise NotImplementedError("auto_augment=%r: pass a policy object, augment.AutoAugment() or augment.RandAugment(num_ops, magnitude, bins); AugMix is "
                                      "not built" % (auto_augment,))
        self.auto_augment = auto_augment
        assert len(images_u8) == len(classes) and len(images_u8) >= 1
        self.engine, self.s = engine, int(imgsz)
        self.scale, self.ratio = tuple(float(v) for v in scale), tuple(float(v) for v in ratio)
        self.fliplr, self.flipud, self.erasing, self.erasing_gate = float(fliplr), float(flipud), float(erasing), erasing_gate
        self.hsv = tuple(float(g) for g in hsv) if hsv is not None else None
        assert self.hsv is None or len(self.hsv) == 3
        self.rng = np.random.default_rng(seed)
        arena, self.srcs = pack_sources(images_u8)
        self.shapes = [(int(h), int(w)) for h, w in zip(self.srcs["h"], self.srcs["w"])]
        self.classes = np.ascontiguousarray(classes, np.float32).reshape(-1)
        self.count, self.max_batch = len(images_u8), int(max_batch)
        e, s, B = engine, self.s, self.max_batch
        self.d_arena, self.d_srcs, self.d_src_cls = e.to_device(arena), e.to_device(self.srcs), e.to_device(self.classes)
        self.d_items, self.d_jitter = e.malloc(B * CLS_ITEM_DTYPE.itemsize), e.malloc(B * JITTER_DTYPE.itemsize)
        self.d_images, self.d_ocls = e.malloc(B * 3 * s * s * 4), e.malloc(B * 4)
        self.d_aa = e.malloc(B * AA_ROW_DTYPE.itemsize) if auto_augment is not None else None

    def close(self):
        for name in ("d_arena", "d_srcs", "d_src_cls", "d_items", "d_jitter", "d_aa", "d_images", "d_ocls"):
            p = getattr(self, name, None)
            if p is not None:
                self.engine.free(p)
            setattr(self, name, None)

    def close_mosaic(self, closed):
        """ClassificationDataset.CloseMosaic is empty: nothing changes."""

    def draw(self, indices):
        """(items, jitter rows or None) of one training batch for the dataset indices `indices`; with an auto_augment policy (items, rows, aa rows)."""
        return draw_classify_items(self.rng, indices, self.shapes, self.s, self.scale, self.ratio, self.fliplr, self.flipud, self.erasing, self.hsv,
                                   self.erasing_gate, self.auto_augment)

    def run(self, items, rows=None, aa=None, mode="train"):
        """Validate on the host (the device cannot refuse aloud), upload `items` (the jitter rows; None = no jitter; the AutoAugment rows `aa`; None = none)
        and launch on the engine's stream (asynchronous) -> ClassifyDeviceBatch."""
        e, lib = self.engine, self.engine.lib
        items = check_classify_items(items, self.srcs, self.s)
        B = int(items.shape[0])
        assert 0 < B <= self.max_batch
        _lib.check(lib, lib.ys_memcpy_h2d(e.ctx, self.d_items, _ptr(items), items.nbytes))
        d_jit = None
        if rows is not None:
            rows = check_jitter(rows, allow_contrast=True)
            if rows.shape != (B,):
                raise ValueError("%d jitter rows for %d items" % (rows.shape[0], B))
            _lib.check(lib, lib.ys_memcpy_h2d(e.ctx, self.d_jitter, _ptr(rows), rows.nbytes))
            d_jit = self.d_jitter
        if aa is not None:
            aa = check_aa_rows(aa)
            if aa.shape != (B,):
                raise ValueError("%d aa rows for %d items" % (aa.shape[0], B))
            if self.d_aa is None:
                self.d_aa = e.malloc(self.max_batch * AA_ROW_DTYPE.itemsize)
            _lib.check(lib, lib.ys_memcpy_h2d(e.ctx, self.d_aa, _ptr(aa), aa.nbytes))
            _lib.check(lib, lib.ys_augment_classify_aa(e.ctx, self.d_arena, self.d_srcs, self.count, self.d_src_cls, self.d_items, B, 1, self.s, self.d_aa, d_jit,
                                                       self.d_images, self.d_ocls))
            return ClassifyDeviceBatch(e, B, self.s, self.d_images, self.d_ocls, mode=mode)
        _lib.check(lib, lib.ys_augment_classify(e.ctx, self.d_arena, self.d_srcs, self.count, self.d_src_cls, self.d_items, B, 1, self.s, d_jit, self.d_images,
                                                self.d_ocls))
        return ClassifyDeviceBatch(e, B, self.s, self.d_images, self.d_ocls, mode=mode)

    def batch(self, indices):
        return self.run(*self.draw(indices))

    def batches(self, batch_size, shuffle=True, drop_last=True):
        """One training epoch: the dataset indices in (shuffled) order, `batch_size` at a time."""
        order = self.rng.permutation(self.count) if shuffle else np.arange(self.count)
        for i in range(0, self.count, batch_size):
            idx = order[i:i + batch_size]
            if len(idx) < batch_size and drop_last:
                break
            yield self.batch(idx)

    def val_batches(self, batch_size):
        """The whole dataset in order through the val chain (Resize + CenterCrop), `batch_size` at a time, the last batch short."""
        for i in range(0, self.count, batch_size):
            idx = np.arange(i, min(i + batch_size, self.count))
            yield self.run(draw_classify_val_items(idx, self.shapes, self.s), None, None, mode="val")
