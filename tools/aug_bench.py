"""Cost of the device-side training input (csrc/augment.hip) on one device: prints ONE JSON line.

  python tools/aug_bench.py [--batch 64] [--imgsz 640] [--sources 128] [--steps 20] [--warmup 5] [--repeats 3]

Four measurements, each in a child process of its own under its own time limit (a leg that fails or runs out of time ends the run):
  augment          ms per batch of ys_augment_mosaic + ys_augment_labels on a device-resident arena and item table (and of the image call alone);
                   bytes from shapes -- the fp32 batch written plus the tiles' source bytes, each read once -- over that time as a share of
                   the 6.3 TB/s this project measured for HBM.  The bound of the kernel is HBM: it is a gather with a streaming write.
  torch_augment    a torch restatement of the reference's op sequence (Data/Augment.cs:158-274, 395-538, 860-966) for the IMAGES on the same GPU:
                   per image the uint8 canvas paste and grid_sample, the flips, then the stack and mul(1/255).  Written here, not imported from tests/.
  step_static      the YOLOv8n bf16 train step (forward, criterion, backward, AdamW, zero_grad) on one fixed device batch
  step_augmented   the same step fed by MosaicAugmenter.batch() -- host draws, item upload, both kernels -- every iteration
Every figure is the median over --repeats timed blocks of --steps calls after --warmup calls, with a synchronise inside the window.

--branch letterbox measures the close-mosaic branch (ys_augment_letterbox / ys_augment_letterbox_labels, MosaicAugmenter.close_mosaic(True)) on the same
dataset instead; the default, mosaic, is the above unchanged.  Its legs: augment = the kernel pair (and the image call alone) -- the fp32 batch written
plus the sources' bytes read once, over that time; torch_augment = a torch restatement of LetterBox + flips + stack + mul(1/255) (Data/Augment.cs:698-778,
860-966) for the images; step_static / step_augmented as above with letterbox batches; and step_host = the same step through AMPWrapper.TrainStep on the
batch's host copy (images and labels copied to the device every step): what a trainer without this branch does once the mosaic is closed.

--hsv measures the ColorJitter (RandomHSV) epilogue instead, for BOTH branches, in two child processes: hsv = the image call of each branch on the same
device-resident tables through the plain entry, through the *_jitter entry with jitter = NULL (the same kernel: these two must agree) and with one drawn
row per image (draw_jitter(0.015, 0.7, 0.4), the reference's default); torch_hsv = a torch restatement of torchvision's uint8 ColorJitter, per image, on
a uint8 batch [B, 3, imgsz, imgsz] that already lives on the same GPU, with the same rows -- the extra pass a host without the epilogue would run.

--task obb measures the OBB corner labels (ys_augment_labels_obb / ys_augment_letterbox_labels_obb) on the same dataset with four rotated-rectangle
corners per label, in four child processes: obb_labels = ms per label call of each branch on device-resident tables (and of the box entries beside them);
numpy_obb_labels = a numpy restatement of the same rows on the host (keep rule, corner chain, the six-direction rectangle, vectorised over the batch's
labels; written here, not imported from tests/); step_augmented = the YOLOv8n-OBB bf16 train step fed by MosaicAugmenter.batch() every iteration, in the
branch --branch names; step_host = the same step through the host entry (AMPWrapper.TrainStep's calls) on a batch's host copy, images and labels copied
to the device every step -- the only way to train OBB without these entries.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

LEGS = ("augment", "torch_augment", "step_static", "step_augmented")
LETTERBOX_LEGS = LEGS + ("step_host",)
OBB_LEGS = ("obb_labels", "numpy_obb_labels", "step_augmented", "step_host")
HSV_LEGS = ("hsv", "torch_hsv")
HBM_TBPS = 6.3
HYP = dict(degrees=10.0, translate=0.1, scale=0.5, shear=2.0, perspective=0.0)


def _dataset(a):
    """--sources synthetic images (letterboxed-to-imgsz shapes like a resized COCO: one side = imgsz) with 8 labels each."""
    g = np.random.default_rng(0)
    S = a.imgsz
    imgs, labels = [], []
    for k in range(a.sources):
        short = int(g.integers(S // 2, S + 1))
        h, w = (S, short) if k % 2 else (short, S)
        imgs.append(g.integers(0, 256, (3, h, w), dtype=np.uint8))
        n = 8
        x1, y1 = g.random(n) * w * 0.7, g.random(n) * h * 0.7
        labels.append(dict(cls=g.integers(0, a.nc, n).astype(np.float32),
                           bboxes=np.stack([x1, y1, x1 + (0.05 + 0.25 * g.random(n)) * w, y1 + (0.05 + 0.25 * g.random(n)) * h], 1).astype(np.float32)))
        if a.task == "obb":                                           # the same rectangles, turned about their centres: "obb" corners, the box derived from them
            b, th = labels[-1].pop("bboxes").astype(np.float64), g.random(n) * np.pi
            c, hw, hh = (b[:, :2] + b[:, 2:]) / 2, (b[:, 2] - b[:, 0]) / 2, (b[:, 3] - b[:, 1]) / 2
            u, v = np.stack([np.cos(th), np.sin(th)], 1), np.stack([-np.sin(th), np.cos(th)], 1)
            labels[-1]["obb"] = np.stack([c + s1 * hw[:, None] * u + s2 * hh[:, None] * v for s1, s2 in ((-1, -1), (1, -1), (1, 1), (-1, 1))], 1).astype(np.float32)
    return imgs, labels


def _timed(fn, sync, a):
    for _ in range(a.warmup):
        fn()
    sync()
    ms = []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        for _ in range(a.steps):
            fn()
        sync()
        ms.append((time.perf_counter() - t0) * 1e3 / a.steps)
    return float(np.median(ms)), [round(v, 4) for v in ms]


def _augmenter(eng, a):
    from yolosharp_amd.augment import MosaicAugmenter
    imgs, labels = _dataset(a)
    return MosaicAugmenter(eng, imgs, labels, a.imgsz, seed=1, max_batch=a.batch, **HYP), imgs


def leg_augment(a):
    from yolosharp_amd import Engine, _lib
    from yolosharp_amd.augment import mosaic4_rects
    eng = Engine(0)
    aug, imgs = _augmenter(eng, a)
    B, S = a.batch, a.imgsz
    items = aug.draw(np.arange(B) % aug.count)
    aug.run(items)                                                    # uploads the item table; the timed calls below reuse it on the device
    lib = eng.lib

    def images():
        _lib.check(lib, lib.ys_augment_mosaic(eng.ctx, aug.d_arena, aug.d_srcs, aug.count, aug.d_items, B, 1, S, aug.r, 0, aug.d_images, None))

    def both():
        images()
        _lib.check(lib, lib.ys_augment_labels(eng.ctx, aug.d_srcs, aug.d_lab_off, aug.d_cls, aug.d_boxes, None, 0, 3, aug.d_items, B, 1, S, 0, 0, aug.capacity,
                                              aug.d_bidx, aug.d_ocls, aug.d_obox, None, aug.d_cnt))

    ms, runs = _timed(both, eng.synchronize, a)
    ms_img, runs_img = _timed(images, eng.synchronize, a)
    written = B * 3 * S * S * 4
    read = 0
    for it in items:
        shapes = [imgs[k].shape[1:] for k in it["src"]]
        read += sum(3 * (r[0][2] - r[0][0]) * (r[0][3] - r[0][1]) for r in mosaic4_rects(int(it["xc"]), int(it["yc"]), shapes, S))
    kept = int(eng.from_device(aug.d_cnt, (1,), np.int32)[0])
    aug.close()
    return {"ms_per_batch": round(ms, 4), "runs": runs, "images_only_ms": round(ms_img, 4), "images_only_runs": runs_img, "bytes_written": written,
            "bytes_read_at_most": read, "hbm_share_of_%.1f_TBps" % HBM_TBPS: round((written + read) / (ms_img * 1e-3) / (HBM_TBPS * 1e12), 4),
            "bound": "HBM (streaming fp32 write + gather)", "labels_kept": kept, "B": B, "imgsz": S, "sources": a.sources}


def leg_letterbox(a):
    from yolosharp_amd import Engine, _lib
    eng = Engine(0)
    aug, imgs = _augmenter(eng, a)
    aug.close_mosaic(True)
    B, S = a.batch, a.imgsz
    items = aug.draw(np.arange(B) % aug.count)
    aug.run(items)                                                    # uploads the item table; the timed calls below reuse it on the device
    lib = eng.lib

    def images():
        _lib.check(lib, lib.ys_augment_letterbox(eng.ctx, aug.d_arena, aug.d_srcs, aug.count, aug.d_items, B, 1, S, aug.r, aug.d_images, None))

    def both():
        images()
        _lib.check(lib, lib.ys_augment_letterbox_labels(eng.ctx, aug.d_srcs, aug.count, aug.d_lab_off, aug.d_cls, aug.d_boxes, None, 0, 3, aug.d_items, B, 1, S, 0,
                                                        aug.capacity, aug.d_bidx, aug.d_ocls, aug.d_obox, None, aug.d_cnt))

    ms, runs = _timed(both, eng.synchronize, a)
    ms_img, runs_img = _timed(images, eng.synchronize, a)
    written = B * 3 * S * S * 4
    read = sum(int(imgs[k].size) for k in items["src"][:, 0])
    kept = int(eng.from_device(aug.d_cnt, (1,), np.int32)[0])
    aug.close()
    return {"ms_per_batch": round(ms, 4), "runs": runs, "images_only_ms": round(ms_img, 4), "images_only_runs": runs_img, "bytes_written": written,
            "bytes_read_at_most": read, "hbm_share_of_%.1f_TBps" % HBM_TBPS: round((written + read) / (ms_img * 1e-3) / (HBM_TBPS * 1e12), 4),
            "labels": kept, "B": B, "imgsz": S, "sources": a.sources}


def leg_torch_letterbox(a):
    import torch
    import torch.nn.functional as F
    from yolosharp_amd.augment import draw_letterbox_items
    imgs, _ = _dataset(a)
    B, S = a.batch, a.imgsz
    items = draw_letterbox_items(np.random.default_rng(1), np.arange(B) % len(imgs), 0.5, 0.0)
    dimgs = [torch.from_numpy(im).cuda() for im in imgs]

    def one(it):
        img = dimgs[int(it["src"][0])]
        h, w = img.shape[1:]
        ratio = min(np.float32(S) / np.float32(w), np.float32(S) / np.float32(h))
        new_w, new_h = int(np.float32(w) * ratio), int(np.float32(h) * ratio)
        if (new_h, new_w) != (h, w):                                  # torchvision's resize returns the image itself at its own size
            img = F.interpolate(img[None].to(torch.float32), size=(new_h, new_w), mode="nearest")[0].to(torch.uint8)
        pl, pu = (S - new_w) // 2, (S - new_h) // 2
        out = F.pad(img, (pl, S - new_w - pl, pu, S - new_h - pu), value=114)
        if it["flip_lr"]:
            out = out.flip(-1)
        if it["flip_ud"]:
            out = out.flip(-2)
        return out[None].mul(1 / 255.0)

    def call():
        return torch.cat([one(it) for it in items], 0)

    ms, runs = _timed(call, torch.cuda.synchronize, a)
    return {"ms_per_batch": round(ms, 4), "runs": runs, "what": "images only (resize + pad per image, flips, stack, mul 1/255)"}


def leg_torch_augment(a):
    import torch
    import torch.nn.functional as F
    from yolosharp_amd.augment import draw_items, mosaic4_rects
    imgs, labels = _dataset(a)
    B, S = a.batch, a.imgsz
    items = draw_items(np.random.default_rng(1), np.arange(B) % len(imgs), S, len(imgs), HYP, 0.5, 0.0)   # same seed, same item table as the augment leg
    dimgs = [torch.from_numpy(im).cuda() for im in imgs]
    gx = torch.arange(S, dtype=torch.float32, device="cuda").view(1, S).repeat(S, 1)
    gy = torch.arange(S, dtype=torch.float32, device="cuda").view(S, 1).repeat(1, S)
    flat = torch.stack([gx, gy, torch.ones_like(gx)], 0).view(3, -1)
    border = torch.full((3, 1, 1), 114.0, device="cuda")
    Ms = [torch.from_numpy(it["M"].reshape(3, 3).copy()).cuda() for it in items]

    def one(it, M):
        img4 = torch.full((3, 2 * S, 2 * S), 114, dtype=torch.uint8, device="cuda")
        shapes = [imgs[k].shape[1:] for k in it["src"]]
        for k, (ra, rb) in zip(it["src"], mosaic4_rects(int(it["xc"]), int(it["yc"]), shapes, S)):
            img4[:, ra[1]:ra[3], ra[0]:ra[2]] = dimgs[k][:, rb[1]:rb[3], rb[0]:rb[2]]
        img = img4.to(torch.float32)
        M3 = torch.eye(3, device="cuda")
        M3[:2] = M[:2]
        sf = torch.linalg.inv(M3).mm(flat)
        src = (sf[:2] / sf[2:3]).view(2, S, S)
        grid = torch.zeros(1, S, S, 2, device="cuda")
        grid[0, :, :, 0] = src[0] / (2 * S - 1) * 2 - 1
        grid[0, :, :, 1] = src[1] / (2 * S - 1) * 2 - 1
        smp = F.grid_sample(img[None], grid, mode="bilinear", padding_mode="border", align_corners=False)[0]
        valid = (src[0] >= 0) & (src[0] <= 2 * S - 1) & (src[1] >= 0) & (src[1] <= 2 * S - 1)
        out = torch.clamp(torch.where(valid[None], smp, border.expand_as(smp)), 0, 255).to(torch.uint8)
        if it["flip_lr"]:
            out = out.flip(-1)
        if it["flip_ud"]:
            out = out.flip(-2)
        return out[None].mul(1 / 255.0)

    def call():
        return torch.cat([one(it, M) for it, M in zip(items, Ms)], 0)

    ms, runs = _timed(call, torch.cuda.synchronize, a)
    return {"ms_per_batch": round(ms, 4), "runs": runs, "what": "images only (canvas paste + grid_sample per image, flips, stack, mul 1/255)"}


def leg_obb_labels(a):
    """Per branch: the OBB label call and, beside it, the box label call on the same tables and items."""
    from yolosharp_amd import Engine, _lib
    eng = Engine(0)
    aug, _ = _augmenter(eng, a)
    B, S, lib = a.batch, a.imgsz, eng.lib
    out = {"B": B, "imgsz": S, "labels_in_tables": int(aug.lab_off[-1])}
    for branch in ("mosaic", "letterbox"):
        aug.close_mosaic(branch == "letterbox")
        aug.run(aug.draw(np.arange(B) % aug.count))                   # uploads the item table; the timed calls below reuse it on the device
        tail = (aug.d_items, B, 1, S)
        outs = (aug.capacity, aug.d_bidx, aug.d_ocls, aug.d_obox)
        if branch == "mosaic":
            calls = {"obb": lambda: lib.ys_augment_labels_obb(eng.ctx, aug.d_srcs, aug.d_lab_off, aug.d_cls, aug.d_boxes, aug.d_obb, *tail, 0, 0, *outs, aug.d_cnt),
                     "box": lambda: lib.ys_augment_labels(eng.ctx, aug.d_srcs, aug.d_lab_off, aug.d_cls, aug.d_boxes, None, 0, 3, *tail, 0, 0, *outs, None, aug.d_cnt)}
        else:
            calls = {"obb": lambda: lib.ys_augment_letterbox_labels_obb(eng.ctx, aug.d_srcs, aug.count, aug.d_lab_off, aug.d_cls, aug.d_boxes, aug.d_obb, *tail, 0,
                                                                        *outs, aug.d_cnt),
                     "box": lambda: lib.ys_augment_letterbox_labels(eng.ctx, aug.d_srcs, aug.count, aug.d_lab_off, aug.d_cls, aug.d_boxes, None, 0, 3, *tail, 0,
                                                                    *outs, None, aug.d_cnt)}
        res = {}
        for name in ("box", "obb"):                                   # obb last: the count read below is its
            ms, runs = _timed(lambda: _lib.check(lib, calls[name]()), eng.synchronize, a)
            res[name + "_ms"], res[name + "_runs"] = round(ms, 4), runs
        res["rows_kept"] = int(eng.from_device(aug.d_cnt, (1,), np.int32)[0])
        out[branch] = res
    aug.close()
    return out


def _np_min_area_rect(c):
    """corners [n, 4, 2] float64 -> [n, 5]: the six-direction rectangle of csrc/augment.hip, vectorised over the rows."""
    n = c.shape[0]
    best = np.full(n, np.inf)
    out = np.zeros((n, 5))
    out[:, :2] = c[:, 0]
    for i, j in ((0, 1), (1, 2), (2, 3), (3, 0), (0, 2), (1, 3)):
        d = c[:, j] - c[:, i]
        ln = np.hypot(d[:, 0], d[:, 1])
        ok = ln > 0
        u = d / np.where(ok, ln, 1.0)[:, None]
        neg = (u[:, 1] < 0) | ((u[:, 1] == 0) & (u[:, 0] < 0))
        u = np.where(neg[:, None], -u, u)
        flat, left = u[:, 1] == 0, u[:, 0] < 0
        u = np.where(flat[:, None], np.stack([np.zeros(n), u[:, 0]], 1), np.where(left[:, None], np.stack([u[:, 1], -u[:, 0]], 1), u))
        nv = np.stack([-u[:, 1], u[:, 0]], 1)
        t, m = np.einsum("nkc,nc->nk", c, u), np.einsum("nkc,nc->nk", c, nv)
        w, h = t.max(1) - t.min(1), m.max(1) - m.min(1)
        better = ok & (w * h < best)
        ctr = ((t.max(1) + t.min(1)) / 2)[:, None] * u + ((m.max(1) + m.min(1)) / 2)[:, None] * nv
        row = np.concatenate([ctr, w[:, None], h[:, None], np.arctan2(u[:, 1], u[:, 0])[:, None]], 1)
        out, best = np.where(better[:, None], row, out), np.where(better, w * h, best)
    return out


def leg_numpy_obb_labels(a):
    """The rows of one batch on the host, per branch, from the same tables and items (numpy, vectorised over the batch's labels)."""
    from yolosharp_amd.augment import draw_items, draw_letterbox_items, mosaic4_rects, pack_labels, pack_obb
    imgs, labels = _dataset(a)
    B, S = a.batch, a.imgsz
    lab_off, cls, boxes, _ = pack_labels(labels)
    corners = pack_obb(labels)
    f = np.float32

    def mosaic(items):
        rows = []
        for b, it in enumerate(items):
            shapes = [imgs[k].shape[1:] for k in it["src"]]
            idx, pad = [], []
            for k, (ra, rb) in zip(it["src"], mosaic4_rects(int(it["xc"]), int(it["yc"]), shapes, S)):
                idx.append(np.arange(lab_off[k], lab_off[k + 1])); pad.append(np.tile(f([ra[0] - rb[0], ra[1] - rb[1]]), (len(idx[-1]), 1)))
            idx, pad, M = np.concatenate(idx), np.concatenate(pad), it["M"].reshape(3, 3)
            bx = boxes[idx] + np.tile(pad, 2)
            org = (bx[:, 2] - bx[:, 0]) * (bx[:, 3] - bx[:, 1])
            bx = np.clip(bx, 0, 2 * S)
            area = (bx[:, 2] - bx[:, 0]) * (bx[:, 3] - bx[:, 1])
            xy = np.concatenate([bx[:, [0, 1, 2, 3, 0, 3, 2, 1]].reshape(-1, 2), np.ones((4 * len(idx), 1), f)], 1) @ M.T
            xy = xy[:, :2].reshape(-1, 4, 2)
            nb = np.clip(np.concatenate([xy.min(1), xy.max(1)], 1), 0, S)
            keep = (area > 0) & (area > f(0.7) * org) & ((nb[:, 2] - nb[:, 0]) * (nb[:, 3] - nb[:, 1]) > 0)
            c = corners[idx][keep] + pad[keep][:, None]
            c = np.clip((np.concatenate([c, np.ones(c.shape[:2] + (1,), f)], 2) @ M.T)[..., :2], 0, S)
            if it["flip_lr"]:
                c[..., 0] = S - c[..., 0]
            if it["flip_ud"]:
                c[..., 1] = S - c[..., 1]
            r = _np_min_area_rect(c.astype(np.float64)).astype(f)
            r[:, :4] /= f(S)
            rows.append(np.concatenate([np.full((len(r), 1), b, f), cls[idx][keep][:, None], r], 1))
        return np.concatenate(rows)

    def letterbox(items):
        rows = []
        for b, it in enumerate(items):
            k = int(it["src"][0])
            h, w = imgs[k].shape[1:]
            ratio = min(f(S) / f(w), f(S) / f(h))
            pad = f([(S - int(f(w) * ratio)) // 2, (S - int(f(h) * ratio)) // 2])
            c = corners[lab_off[k]:lab_off[k + 1]] + pad
            if it["flip_lr"]:
                c[..., 0] = S - c[..., 0]
            if it["flip_ud"]:
                c[..., 1] = S - c[..., 1]
            r = _np_min_area_rect(c.astype(np.float64)).astype(f)
            r[:, :4] /= f(S)
            rows.append(np.concatenate([np.full((len(r), 1), b, f), cls[lab_off[k]:lab_off[k + 1]][:, None], r], 1))
        return np.concatenate(rows)

    out = {"what": "keep rule, corner chain, six-direction rectangle and collate in numpy on the host, one batch"}
    its = {"mosaic": draw_items(np.random.default_rng(1), np.arange(B) % len(imgs), S, len(imgs), HYP, 0.5, 0.0),
           "letterbox": draw_letterbox_items(np.random.default_rng(1), np.arange(B) % len(imgs), 0.5, 0.0)}
    for branch, fn in (("mosaic", mosaic), ("letterbox", letterbox)):
        ms, runs = _timed(lambda: fn(its[branch]), lambda: None, a)
        out[branch] = {"ms_per_batch": round(ms, 4), "runs": runs, "rows": int(fn(its[branch]).shape[0])}
    return out


HSV = (0.015, 0.7, 0.4)


def leg_hsv(a):
    """Per branch: the image call without rows (plain entry; *_jitter entry with NULL) and with one drawn row per image."""
    from yolosharp_amd import Engine, _lib
    from yolosharp_amd.augment import JITTER_DTYPE, draw_jitter
    eng = Engine(0)
    aug, _ = _augmenter(eng, a)
    B, S = a.batch, a.imgsz
    lib = eng.lib
    rows = draw_jitter(np.random.default_rng(2), B, *HSV)
    d_rows = eng.to_device(np.ascontiguousarray(rows, JITTER_DTYPE))
    out = {"B": B, "imgsz": S, "hsv": list(HSV)}
    for branch in ("mosaic", "letterbox"):
        aug.close_mosaic(branch == "letterbox")
        aug.run(aug.draw(np.arange(B) % aug.count))                   # uploads the item table; the timed calls below reuse it on the device
        common = (eng.ctx, aug.d_arena, aug.d_srcs, aug.count, aug.d_items, B, 1, S, aug.r)
        if branch == "mosaic":
            calls = {"plain": lambda: lib.ys_augment_mosaic(*common, 0, aug.d_images, None),
                     "null_rows": lambda: lib.ys_augment_mosaic_jitter(*common, 0, None, aug.d_images, None),
                     "jitter": lambda: lib.ys_augment_mosaic_jitter(*common, 0, d_rows, aug.d_images, None)}
        else:
            calls = {"plain": lambda: lib.ys_augment_letterbox(*common, aug.d_images, None),
                     "null_rows": lambda: lib.ys_augment_letterbox_jitter(*common, None, aug.d_images, None),
                     "jitter": lambda: lib.ys_augment_letterbox_jitter(*common, d_rows, aug.d_images, None)}
        res = {}
        for name, fn in calls.items():
            ms, runs = _timed(lambda: _lib.check(lib, fn()), eng.synchronize, a)
            res[name + "_ms"], res[name + "_runs"] = round(ms, 4), runs
        res["jitter_extra_ms"] = round(res["jitter_ms"] - res["plain_ms"], 4)
        out[branch] = res
    eng.free(d_rows)
    aug.close()
    return out


def leg_torch_hsv(a):
    """torchvision's uint8 ColorJitter restated in torch (transforms/_functional_tensor.py), per image, on a device-resident uint8 batch."""
    import torch
    from yolosharp_amd.augment import draw_jitter
    B, S = a.batch, a.imgsz
    rows = draw_jitter(np.random.default_rng(2), B, *HSV)
    batch = torch.from_numpy(np.random.default_rng(3).integers(0, 256, (B, 3, S, S), dtype=np.uint8)).cuda()

    def blend(img, other, f):
        return (f * img + (1.0 - f) * other).clamp(0, 255).to(torch.uint8)

    def gray(img):
        r, g, b = img.unbind(0)
        return (0.2989 * r + 0.587 * g + 0.114 * b).to(torch.uint8).unsqueeze(0)

    def hue(img, f):
        x = img.to(torch.float32) / 255.0
        r, g, b = x.unbind(0)
        maxc, minc = x.max(0).values, x.min(0).values
        eqc = maxc == minc
        cr = maxc - minc
        ones = torch.ones_like(maxc)
        s = cr / torch.where(eqc, ones, maxc)
        d = torch.where(eqc, ones, cr)
        rc, gc, bc = (maxc - r) / d, (maxc - g) / d, (maxc - b) / d
        h = (maxc == r) * (bc - gc) + ((maxc == g) & (maxc != r)) * (2.0 + rc - bc) + ((maxc != g) & (maxc != r)) * (4.0 + gc - rc)
        h = (torch.fmod(h / 6.0 + 1.0, 1.0) + f) % 1.0
        i = torch.floor(h * 6.0)
        ff = h * 6.0 - i
        i = i.to(torch.int32) % 6
        p, q, t = (maxc * (1.0 - s)).clamp(0, 1), (maxc * (1.0 - s * ff)).clamp(0, 1), (maxc * (1.0 - s * (1.0 - ff))).clamp(0, 1)
        mask = (i.unsqueeze(0) == torch.arange(6, device=i.device).view(-1, 1, 1)).to(torch.float32)
        a4 = torch.stack((torch.stack((maxc, q, p, p, t, maxc)), torch.stack((t, maxc, maxc, q, p, p)), torch.stack((p, p, t, maxc, maxc, q))))
        return torch.einsum("ijk,xijk->xjk", mask, a4).mul(255.999).to(torch.uint8)

    def one(img, row):
        for op in row["order"]:
            f = float(row["factor"][op]) if op >= 0 else 0.0
            if op == 0:
                img = blend(img, torch.zeros_like(img), f)
            elif op == 1:
                img = blend(img, gray(img).to(torch.float32).mean(), f)
            elif op == 2:
                img = blend(img, gray(img), f)
            elif op == 3:
                img = hue(img, f)
        return img[None].mul(1 / 255.0)

    def call():
        return torch.cat([one(batch[b], rows[b]) for b in range(B)], 0)

    ms, runs = _timed(call, torch.cuda.synchronize, a)
    return {"ms_per_batch": round(ms, 4), "runs": runs, "what": "ColorJitter per image on a resident uint8 batch, stack, mul 1/255"}


def leg_step(a, augmented, host=False):
    from yolosharp_amd import Engine
    from yolosharp_amd.model import AMPWrapper, Yolov8, Yolov8Obb, v8DetectionLoss, v8OBBLoss
    if a.task == "obb":
        Yolov8, v8DetectionLoss = Yolov8Obb, v8OBBLoss
    eng = Engine(0)
    B, S = a.batch, a.imgsz
    aug, _ = _augmenter(eng, a)
    aug.close_mosaic(a.branch == "letterbox")
    m = Yolov8(eng, nc=a.nc, size="n", height=S, width=S, max_batch=B, dtype="bf16")
    m.init_weights(1)
    m.reserve_labels(aug.max_per_image)
    crit, amp = v8DetectionLoss(m), AMPWrapper(m)
    m.train()
    db = aug.batch(np.arange(B) % aug.count)
    state = {"i": 0}
    hb = db.to_host() if host else None

    def step():
        if host:                                                      # images and labels travel to the device every step (TrainStep without its loss read)
            m.forward(hb["images"], fetch=False)
            crit.forward(None, hb, read=False)
            return amp.Step()
        d = db
        if augmented:
            state["i"] += 1
            d = aug.batch((np.arange(B) + state["i"] * B) % aug.count)
        m.forward_device(d.images, B)
        crit.forward_device(d.batch_idx, d.cls, d.bboxes, d.capacity)
        amp.Step()

    ms, runs = _timed(step, eng.synchronize, a)
    _, items = crit.read()
    t0 = time.perf_counter()
    for _ in range(5):
        aug.draw(np.arange(B))
    draw_ms = (time.perf_counter() - t0) * 1e3 / 5
    m.close(); aug.close()
    return {"ms_per_step": round(ms, 4), "runs": runs, "loss_items": [float(v) for v in items], "label_rows": db.capacity, "host_draw_ms": round(draw_ms, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--imgsz", type=int, default=640)
    ap.add_argument("--sources", type=int, default=128)
    ap.add_argument("--nc", type=int, default=80)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--leg-timeout", type=int, default=240, help="seconds per child process")
    ap.add_argument("--branch", choices=("mosaic", "letterbox"), default="mosaic", help="the pipeline to measure (letterbox = the close-mosaic branch)")
    ap.add_argument("--hsv", action="store_true", help="measure the ColorJitter epilogue of both branches and its torch restatement instead")
    ap.add_argument("--task", choices=("detect", "obb"), default="detect", help="obb: the OBB corner-label entries and the YOLOv8n-OBB step")
    ap.add_argument("--leg", choices=LETTERBOX_LEGS + HSV_LEGS + OBB_LEGS[:2], help="run one measurement in this process (what the driver starts)")
    a = ap.parse_args()
    lb = a.branch == "letterbox"
    if a.leg:
        out = {"obb_labels": lambda: leg_obb_labels(a), "numpy_obb_labels": lambda: leg_numpy_obb_labels(a), "hsv": lambda: leg_hsv(a), "torch_hsv": lambda: leg_torch_hsv(a), "augment": lambda: leg_letterbox(a) if lb else leg_augment(a), "torch_augment": lambda: leg_torch_letterbox(a) if lb else leg_torch_augment(a),
               "step_static": lambda: leg_step(a, False), "step_augmented": lambda: leg_step(a, True), "step_host": lambda: leg_step(a, False, host=True)}[a.leg]()
        print(json.dumps(out))
        return 0
    res = {"metric": "augment_cost", "model": "yolov8n", "dtype": "bf16", "batch": a.batch, "imgsz": a.imgsz, "sources": a.sources}
    if lb and not a.hsv:
        res["branch"] = "letterbox"
    if a.hsv:
        res["metric"] = "color_jitter_cost"
    if a.task == "obb":
        res.update(metric="obb_label_cost", model="yolov8n-obb", branch=a.branch)
    fwd = [x for kv in (("--batch", a.batch), ("--imgsz", a.imgsz), ("--sources", a.sources), ("--nc", a.nc), ("--steps", a.steps), ("--warmup", a.warmup),
                        ("--repeats", a.repeats), ("--branch", a.branch), ("--task", a.task)) for x in (kv[0], str(kv[1]))]
    for leg in (OBB_LEGS if a.task == "obb" else HSV_LEGS if a.hsv else LETTERBOX_LEGS if lb else LEGS):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", leg] + fwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                               text=True, timeout=a.leg_timeout, stdin=subprocess.DEVNULL)
        except subprocess.TimeoutExpired:
            res["failed"] = {"leg": leg, "why": "time limit of %d s" % a.leg_timeout}
            break                                   # nothing more is started on the device after a leg that hung
        if r.returncode != 0:
            res["failed"] = {"leg": leg, "rc": r.returncode, "stderr": r.stderr[-2000:]}
            break                                   # ... or that failed
        res[leg] = json.loads(r.stdout.strip().splitlines()[-1])
    if "hsv" in res and "torch_hsv" in res:
        for branch in ("mosaic", "letterbox"):
            res["torch_over_epilogue_" + branch] = round(res["torch_hsv"]["ms_per_batch"] / max(res["hsv"][branch]["jitter_extra_ms"], 1e-4), 2)
    if "augment" in res and "torch_augment" in res:
        res["torch_over_augment_images"] = round(res["torch_augment"]["ms_per_batch"] / res["augment"]["images_only_ms"], 2)
    if "step_static" in res and "step_augmented" in res:
        res["augment_extra_ms_per_step"] = round(res["step_augmented"]["ms_per_step"] - res["step_static"]["ms_per_step"], 4)
        res["augment_extra_share_of_step"] = round(res["augment_extra_ms_per_step"] / res["step_static"]["ms_per_step"], 4)
    if "obb_labels" in res and "numpy_obb_labels" in res:
        for branch in ("mosaic", "letterbox"):
            res["numpy_over_kernel_" + branch] = round(res["numpy_obb_labels"][branch]["ms_per_batch"] / max(res["obb_labels"][branch]["obb_ms"], 1e-4), 1)
    if a.task == "obb" and "step_augmented" in res and "step_host" in res:
        res["host_batch_extra_ms_per_step"] = round(res["step_host"]["ms_per_step"] - res["step_augmented"]["ms_per_step"], 4)
    if "step_static" in res and "step_host" in res:
        res["host_batch_extra_ms_per_step"] = round(res["step_host"]["ms_per_step"] - res["step_static"]["ms_per_step"], 4)
    print(json.dumps(res))
    return 1 if "failed" in res else 0


if __name__ == "__main__":
    sys.exit(main())
