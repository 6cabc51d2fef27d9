"""Device-side Mosaic4 + RandomPerspective + flips + Normalize + collate (csrc/augment.hip: ys_augment_mosaic / ys_augment_labels, yolosharp_amd/augment.py)
against tests/aug_ref.py, the torch restatement of Data/Augment.cs:158-274, 315-695, 860-966 with the dtype as a parameter.

Images (and masks) are judged as BYTES against the float64 restatement: no byte differs by more than one level, and per image the share of
bytes (image and mask bytes together) that differ by one level is at most 3x the share by which the float32 restatement -- the reference's own
arithmetic -- differs from float64 on the same input; the test computes that share itself.  The factor 3 covers another operation order (the
engine inverts M, evaluates the source position and blends in double, as a nested interpolation).  No pixel is exempted: the inputs keep every source position
at least 1e-3 px from the validity edge (asserted; change the seed rather than add an exemption).
Labels: the float64 restatement computes every label's decision margins; labels whose keep decisions are closer than 1e-3 to a threshold (0.7, 0)
or that carry a keypoint closer than 1e-3 px to a bound are removed from the input (at least 80 % must remain).  Then count, kept set, order,
batch_idx and cls are exact and coordinates agree within 2e-5 normalised: about 8 fp32 roundings at magnitude <= 128 px are 6e-5 px, 1e-6 after
/ 64; the tolerance leaves 20x."""
import functools

import numpy as np
import pytest
import torch

import aug_ref as R
from conftest import BACKENDS

S, RATIO = 64, 4
SHAPES = [(64, 48), (40, 64), (64, 64), (33, 64), (64, 17), (8, 8)]         # (h, w): full, narrow, short, odd, thin, tiny


def _sources(shapes, seed, ratio=RATIO):
    """uint8 RGB planes = seeded noise + a smooth ramp, and id masks (blocks of small ids)."""
    g = np.random.default_rng(seed)
    imgs, masks = [], []
    for h, w in shapes:
        yy, xx = np.mgrid[0:h, 0:w]
        ramp = (xx * 97.0 / max(w - 1, 1) + yy * 89.0 / max(h - 1, 1))[None] + np.array([0.0, 20.0, 40.0])[:, None, None]
        imgs.append(np.clip(ramp + g.integers(0, 70, (3, h, w)), 0, 255).astype(np.uint8))
        masks.append(g.integers(0, 6, (max(h // ratio, 1), max(w // ratio, 1))).astype(np.uint8))
    return imgs, masks


def _matrix(s, angle=0.0, scale=1.0, shear=(0.0, 0.0), persp=(0.0, 0.0), trans=(0.5, 0.5)):
    """M = T @ S @ R @ P @ C of affine_transform (:323-356) from explicit parameters, fp32."""
    f = np.float32
    Cm, P, Rm, Sm, T = (np.eye(3, dtype=f) for _ in range(5))
    Cm[0, 2] = Cm[1, 2] = -s
    P[2, 0], P[2, 1] = persp
    rad = f(angle) * f(np.pi) / f(180.0)
    a, b = f(np.cos(rad)) * f(scale), f(np.sin(rad)) * f(scale)
    Rm[0, :2], Rm[1, :2] = (a, b), (-b, a)
    Sm[0, 1], Sm[1, 0] = np.tan(shear[0] * np.pi / 180), np.tan(shear[1] * np.pi / 180)
    T[0, 2], T[1, 2] = trans[0] * s, trans[1] * s
    return (T @ (Sm @ (Rm @ (P @ Cm)))).astype(f)


def _item_list(s, perspective):
    """(src[4], xc, yc, M, flip_lr, flip_ud): centres at both ends of [s/2, 3s/2) and in the middle, all four flip combinations per matrix kind."""
    lo, mid, hi = s // 2, s, 2 * s - s // 2 - 1
    centres = [(lo, lo), (hi, hi), (mid, mid), (lo, hi), (hi, mid), (mid, lo)]
    if perspective:
        kinds = [dict(angle=4.0, scale=0.9, persp=(5e-4, -5e-4), trans=(0.47, 0.55)), dict(scale=1.13, persp=(-5e-4, 3e-4), trans=(0.52, 0.44))]
    else:
        kinds = [dict(scale=0.83, trans=(0.53, 0.46)), dict(angle=10.0, scale=1.07, shear=(2.0, -2.0), trans=(0.45, 0.57))]
    items, k = [], 0
    for kind in kinds:
        for flr, fud in ((0, 0), (1, 0), (0, 1), (1, 1)):
            src = [(k + j) % len(SHAPES) for j in (0, 2, 3, 5)] if k % 2 else [(k + j) % len(SHAPES) for j in (1, 2, 4, 0)]
            xc, yc = centres[k % len(centres)]
            items.append((src, xc, yc, _matrix(s, **kind), flr, fud))
            k += 1
    items.append(([5, 5, 4, 5], mid, lo, _matrix(s, **kinds[0]), 1, 0))       # small sources only: most of the canvas is the 114 fill
    return items


def _pack_items(lst):
    from yolosharp_amd import augment as A
    it = A.make_items(len(lst))
    for b, (src, xc, yc, M, flr, fud) in enumerate(lst):
        it[b]["src"], it[b]["xc"], it[b]["yc"], it[b]["M"], it[b]["flip_lr"], it[b]["flip_ud"] = src, xc, yc, np.asarray(M, np.float32).reshape(9), flr, fud
    return it


def _ref_bytes(imgs, masks, item, s, r, perspective, dtype):
    src, xc, yc, M, flr, fud = item
    ti = [torch.from_numpy(imgs[k]) for k in src]
    tm = [torch.from_numpy(masks[k]) for k in src]
    out, om = R.image_sample(ti, tm, xc, yc, M, flr, fud, s, r, perspective, dtype)
    return out.numpy(), om.numpy()


@functools.lru_cache(maxsize=None)
def _image_case(perspective):
    """Sources, items and both restatements of the small image case, computed once and never modified."""
    imgs, masks = _sources(SHAPES, seed=11)
    items = _item_list(S, perspective)
    ref64 = [_ref_bytes(imgs, masks, it, S, RATIO, perspective, torch.float64) for it in items]
    ref32 = [_ref_bytes(imgs, masks, it, S, RATIO, perspective, torch.float32) for it in items]
    edge = min(R.edge_distance([torch.from_numpy(imgs[k]) for k in it[0]], it[1], it[2], it[3], S, perspective) for it in items)
    return imgs, masks, items, ref64, ref32, edge


def _judge(images, mks, ref64, ref32):
    """The two conditions of the module docstring for every image of a batch; returns the figures."""
    figs = []
    by = images * np.float32(255.0)
    bytes_ = np.rint(by).astype(np.int64)
    assert np.array_equal(images, bytes_.astype(np.float32) * np.float32(1 / 255.0))              # bytes * (1 / 255.0f), bit for bit
    assert bytes_.min() >= 0 and bytes_.max() <= 255
    for b in range(images.shape[0]):
        r64 = np.concatenate([ref64[b][0].reshape(-1), ref64[b][1].reshape(-1)]).astype(np.int64)
        r32 = np.concatenate([ref32[b][0].reshape(-1), ref32[b][1].reshape(-1)]).astype(np.int64)
        got = np.concatenate([bytes_[b].reshape(-1), mks[b].reshape(-1).astype(np.int64)])
        assert np.array_equal(mks[b], np.rint(mks[b]))                                               # masks are whole ids
        d, d32 = np.abs(got - r64), np.abs(r32 - r64)
        share, share32 = float(np.mean(d == 1)), float(np.mean(d32 == 1))
        print("image %d: max diff %d, share of one-level bytes %.5f (float32 restatement %.5f)" % (b, d.max(), share, share32))
        figs.append((int(d.max()), share, share32))
        assert d.max() <= 1, (b, int(d.max()))
        assert share <= 3 * share32, (b, share, share32)
    return figs


# ---------------------------------------------------------------------------------------------------- images
@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("perspective", [0, 1])
def test_image_parity(backend, engine, perspective):
    from yolosharp_amd import augment as A
    imgs, masks, items, ref64, ref32, edge = _image_case(perspective)
    assert edge >= 1e-3, edge                                        # no source position near the validity edge: nothing is exempted
    assert max(np.abs(a[0].astype(int) - b[0].astype(int)).max() for a, b in zip(ref32, ref64)) <= 1
    arena, srcs = A.pack_sources(imgs, masks)
    for i0 in range(0, len(items), 3):                               # B = 3
        chunk = items[i0:i0 + 3]
        images, mks = A.augment_mosaic(engine, arena, srcs, _pack_items(chunk), S, RATIO, perspective, with_masks=True)
        assert images.shape == (len(chunk), 3, S, S) and mks.shape == (len(chunk), S // RATIO, S // RATIO)
        _judge(images, mks, ref64[i0:i0 + 3], ref32[i0:i0 + 3])
    # a second call with the same items is bit-identical; images without masks are the same images
    it = _pack_items(items[:3])
    a1, m1 = A.augment_mosaic(engine, arena, srcs, it, S, RATIO, perspective, with_masks=True)
    a2, m2 = A.augment_mosaic(engine, arena, srcs, it, S, RATIO, perspective, with_masks=True)
    a3, m3 = A.augment_mosaic(engine, arena, srcs, it, S, RATIO, perspective, with_masks=False)
    assert np.array_equal(a1, a2) and np.array_equal(m1, m2) and np.array_equal(a1, a3) and m3 is None


@pytest.mark.parametrize("backend", BACKENDS)
def test_label_free_sample_is_still_warped(backend, engine):
    """A MosaicAugmenter over a dataset WITHOUT labels: its batch holds the s x s WARPED images (RandomPerspective.Apply would hand back the
    unwarped 2s x 2s canvas for such a sample, Augment.cs:666-669 -- a documented deviation) and no label row."""
    from yolosharp_amd import augment as A
    imgs, masks, items, ref64, ref32, _ = _image_case(0)
    empty = [dict(cls=np.zeros((0,), np.float32), bboxes=np.zeros((0, 4), np.float32)) for _ in imgs]
    aug = A.MosaicAugmenter(engine, imgs, empty, S, masks=masks, mask_ratio=RATIO, seed=0, max_batch=3)
    db = aug.run(_pack_items(items[3:6]))
    host = db.to_host()
    assert db.n_input == 0 and len(host["cls"]) == 0 and host["images"].shape == (3, 3, S, S)
    _judge(host["images"], host["masks"], ref64[3:6], ref32[3:6])
    canvas = R.mosaic4([torch.from_numpy(imgs[k]) for k in items[3][0]], None, items[3][1], items[3][2], S, RATIO)[0].numpy()
    assert not np.array_equal(np.rint(host["images"][0] * 255).astype(np.uint8), canvas[:, :S, :S])        # ... and not a crop of the canvas
    aug.close()


@pytest.mark.parametrize("backend", BACKENDS)
def test_image_odd_width_and_canvas_fill(backend, engine):
    """imgsz that is no multiple of 4 (scalar stores, a partial last quad) and the identity-like placement whose canvas has untouched 114 regions."""
    from yolosharp_amd import augment as A
    s = 30
    imgs, masks = _sources([(30, 22), (9, 30), (30, 30), (5, 7)], seed=3, ratio=2)
    arena, srcs = A.pack_sources(imgs, masks)
    lst = [([0, 1, 2, 3], 15, 44, _matrix(s, angle=-7.0, scale=0.9, trans=(0.51, 0.48)), 1, 1), ([3, 3, 1, 0], 29, 20, _matrix(s, scale=0.6, trans=(0.5, 0.52)), 0, 0)]
    images, mks = A.augment_mosaic(engine, arena, srcs, _pack_items(lst), s, 2, 0, with_masks=True)
    r64 = [_ref_bytes(imgs, masks, it, s, 2, 0, torch.float64) for it in lst]
    r32 = [_ref_bytes(imgs, masks, it, s, 2, 0, torch.float32) for it in lst]
    _judge(images, mks, r64, r32)
    assert (r64[1][0] == 114).mean() > 0.3                            # the fill is really there


@pytest.mark.gpu
def test_image_parity_large():
    """s = 640, B = 2: one affine and one perspective item through the perspective form; the same two conditions."""
    from yolosharp_amd import Engine
    from yolosharp_amd import augment as A
    s = 640
    shapes = [(640, 480), (427, 640), (640, 640), (333, 500), (480, 171), (80, 80)]
    imgs, masks = _sources(shapes, seed=5)
    arena, srcs = A.pack_sources(imgs, masks)
    lst = [([0, 1, 2, 3], 400, 700, _matrix(s, angle=10.0, scale=1.07, shear=(2.0, -2.0), trans=(0.45, 0.57)), 1, 0),
           ([4, 2, 5, 1], 930, 345, _matrix(s, angle=4.0, scale=0.9, persp=(5e-4, -5e-4), trans=(0.47, 0.55)), 0, 1)]
    images, mks = A.augment_mosaic(Engine(), arena, srcs, _pack_items(lst), s, RATIO, 1, with_masks=True)
    r64 = [_ref_bytes(imgs, masks, it, s, RATIO, 1, torch.float64) for it in lst]
    r32 = [_ref_bytes(imgs, masks, it, s, RATIO, 1, torch.float32) for it in lst]
    assert min(R.edge_distance([torch.from_numpy(imgs[k]) for k in it[0]], it[1], it[2], it[3], s, 1) for it in lst) >= 1e-3
    _judge(images, mks, r64, r32)


# ---------------------------------------------------------------------------------------------------- labels
KPT = 5
FAR = dict(scale=0.9, trans=(7.5, 0.5))                                # everything lands right of the output: the image loses all its labels


def _label_items(perspective):
    p = (5e-4, -4e-4) if perspective else (0.0, 0.0)
    return [([0, 1, 2, 3], 32, 40, _matrix(S, angle=6.0, scale=0.8, shear=(1.5, -1.0), persp=p, trans=(0.5, 0.48)), 0, 0),
            ([2, 3, 0, 4], 90, 70, _matrix(S, angle=-9.0, scale=0.7, persp=p, trans=(0.46, 0.53)), 1, 0),
            ([1, 5, 3, 2], 60, 60, _matrix(S, persp=p, **FAR), 0, 0),
            ([4, 0, 1, 2], 50, 88, _matrix(S, angle=3.0, scale=0.75, persp=p, trans=(0.55, 0.5)), 1, 1)]


def _raw_labels(seed, per_source=10):
    g = np.random.default_rng(seed)
    labels, uid = [], 0
    for h, w in SHAPES:
        x1, y1 = g.random(per_source) * w * 0.8, g.random(per_source) * h * 0.8
        bw, bh = (0.08 + g.random(per_source) * 0.5) * w, (0.08 + g.random(per_source) * 0.5) * h
        boxes = np.stack([x1, y1, np.minimum(x1 + bw, w), np.minimum(y1 + bh, h)], 1).astype(np.float32)
        kp = np.concatenate([boxes[:, None, :2] + g.random((per_source, KPT, 2)) * (boxes[:, None, 2:] - boxes[:, None, :2]),
                             g.integers(0, 3, (per_source, KPT, 1))], 2).astype(np.float32)
        labels.append(dict(cls=np.arange(uid, uid + per_source, dtype=np.float32), bboxes=boxes, keypoints=kp))   # cls = a unique id: the kept SET is visible
        uid += per_source
    return labels


def _restate_labels(labels, items, perspective, dtype, sort_flipped=False):
    samples, margins = [], []
    for src, xc, yc, M, flr, fud in items:
        _, _, pads = R.mosaic4([torch.zeros((3,) + SHAPES[k], dtype=torch.uint8) for k in src], None, xc, yc, S, RATIO)
        tiles = [dict(cls=labels[k]["cls"], boxes=labels[k]["bboxes"], kpts=labels[k]["keypoints"]) for k in src]
        smp, mg = R.labels_sample(tiles, pads, M, flr, fud, S, perspective, dtype, sort_flipped)
        samples.append(smp); margins.append((src, mg))
    return samples, margins


@functools.lru_cache(maxsize=None)
def _label_case(perspective):
    """Labels with every decision at least 1e-3 from its threshold (module docstring), the items, and the float64 restatement of the batch."""
    items = _label_items(perspective)
    raw = _raw_labels(seed=21)
    _, margins = _restate_labels(raw, items, perspective, torch.float64)
    n_src = len(SHAPES)
    ok = [np.ones(len(l["cls"]), bool) for l in raw]
    for src, mg in margins:                                           # a source label is judged in every tile it appears in
        near = (mg["ratio"].abs() < 1e-3) | ((mg["area1"] > 0) & (mg["area1"] < 1e-3)) | ((mg["area2"] > 0) & (mg["area2"] < 1e-3)) | (mg["kmargin"] < 1e-3)
        near = near.numpy()
        o = 0
        for k in src:
            n = len(raw[k]["cls"])
            ok[k] &= ~near[o:o + n]
            o += n
    total, kept = sum(len(o) for o in ok), sum(int(o.sum()) for o in ok)
    labels = [dict(cls=l["cls"][o], bboxes=l["bboxes"][o], keypoints=l["keypoints"][o]) for l, o in zip(raw, ok)]
    ref = {sf: _restate_labels(labels, items, perspective, torch.float64, sf) for sf in (False, True)}
    return items, labels, ref, kept / total, n_src


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("perspective", [0, 1])
def test_label_parity(backend, engine, perspective):
    from yolosharp_amd import augment as A
    items, labels, ref, survive, n_src = _label_case(perspective)
    assert survive >= 0.8, survive
    samples, margins = ref[False]
    g1 = torch.cat([m["good1"] for _, m in margins]); g = torch.cat([m["good"] for _, m in margins])
    a1 = torch.cat([m["area1"] for _, m in margins]); ratio = torch.cat([m["ratio"] for _, m in margins])
    assert len(g) >= 4 * 35                                            # about 40 labels per image over the four tiles
    assert bool(((a1 > 0) & (ratio < 0)).any()) and bool((a1 <= 0).any()) and bool(g1.any())       # rule 1: dropped by the ratio, by the area, kept
    assert bool((g1 & ~g).any()) and bool(g.any())                                                 # rule 2: dropped, kept
    assert any(len(smp["cls"]) == 0 for smp in samples) and any(len(smp["cls"]) > 0 for smp in samples)   # one image loses all its labels
    imgs, _ = _sources(SHAPES, seed=11)
    _, srcs = A.pack_sources(imgs)
    lab_off, cls, boxes, kp = A.pack_labels(labels)
    it = _pack_items(items)
    cap = int(lab_off[-1]) * 4 + 7
    flipped_negative = False
    for sort_flipped in (False, True):
        want = {k: v.numpy() if v is not None else None for k, v in R.collate(ref[sort_flipped][0]).items()}
        n = len(want["cls"])
        out = A.augment_labels(engine, srcs, lab_off, cls, boxes, kp, it, S, perspective, A.YS_AUG_SORT_FLIPPED if sort_flipped else 0, cap)
        assert out["count"] == n and 0 < n < cap
        assert np.array_equal(out["batch_idx"][:n], want["batch_idx"]) and np.array_equal(out["cls"][:n], want["cls"])      # kept set, order, image
        assert np.all(out["batch_idx"][n:] == -1) and not out["cls"][n:].any() and not out["bboxes"][n:].any() and not out["keypoints"][n:].any()
        err = np.abs(out["bboxes"][:n].astype(np.float64) - want["bboxes"]).max()
        kerr = np.abs(out["keypoints"][:n, :, :2].astype(np.float64) - want["keypoints"][..., :2]).max()
        print("sort_flipped %d: %d rows, box error %.3g, keypoint error %.3g" % (sort_flipped, n, err, kerr))
        assert err <= 2e-5 and kerr <= 2e-5, (err, kerr)
        assert np.array_equal(out["keypoints"][:n, :, 2], want["keypoints"][..., 2].astype(np.float32))                      # visibility
        assert (out["keypoints"][:n, :, 2] == 0).any() and (out["keypoints"][:n, :, 2] > 0).any()
        if sort_flipped:
            assert np.all(out["bboxes"][:n, 2:] > 0)
        else:
            flipped_negative = bool((out["bboxes"][:n, 2] < 0).any() and (out["bboxes"][:n, 3] < 0).any())
        # bit-identical on a second call
        again = A.augment_labels(engine, srcs, lab_off, cls, boxes, kp, it, S, perspective, A.YS_AUG_SORT_FLIPPED if sort_flipped else 0, cap)
        assert all(np.array_equal(out[k], again[k]) for k in ("batch_idx", "cls", "bboxes", "keypoints")) and again["count"] == n
    assert flipped_negative                                            # the reference's un-swapped flip: negative w and h after cxcywh
    # without keypoints: the same rows
    out = A.augment_labels(engine, srcs, lab_off, cls, boxes, None, it, S, perspective, 0, cap)
    want = R.collate(ref[False][0])
    assert out["keypoints"] is None and np.array_equal(out["cls"][:out["count"]], want["cls"].numpy())


@pytest.mark.parametrize("backend", BACKENDS)
def test_labels_more_than_one_chunk(backend, engine):
    """An image with more labels than the workgroup has threads (the scan runs in chunks of 256): 4 x 150 labels, compacted in order."""
    from yolosharp_amd import augment as A
    g = np.random.default_rng(4)
    shapes = [(64, 64)] * 4
    labels = []
    for k in range(4):
        x1, y1 = g.random(150) * 50, g.random(150) * 50
        labels.append(dict(cls=np.arange(150 * k, 150 * k + 150, dtype=np.float32),
                           bboxes=np.stack([x1, y1, x1 + 3 + g.random(150) * 10, y1 + 3 + g.random(150) * 10], 1).astype(np.float32), keypoints=None))
    items = [([0, 1, 2, 3], 64, 64, _matrix(S, scale=0.9, trans=(0.5, 0.5)), 0, 0), ([3, 2, 1, 0], 50, 70, _matrix(S, scale=0.7, trans=(0.52, 0.5)), 0, 1)]
    samples = []
    for src, xc, yc, M, flr, fud in items:
        _, _, pads = R.mosaic4([torch.zeros((3, 64, 64), dtype=torch.uint8)] * 4, None, xc, yc, S, RATIO)
        smp, mg = R.labels_sample([dict(cls=labels[k]["cls"], boxes=labels[k]["bboxes"], kpts=None) for k in src], pads, M, flr, fud, S, 0, torch.float64)
        assert float(torch.minimum(mg["ratio"].abs(), torch.where(mg["area2"] > 0, mg["area2"], torch.ones_like(mg["area2"]))).min()) > 1e-4
        samples.append(smp)
    want = R.collate(samples)
    _, srcs = A.pack_sources([np.zeros((3, 64, 64), np.uint8)] * 4)
    lab_off, cls, boxes, _ = A.pack_labels(labels)
    out = A.augment_labels(engine, srcs, lab_off, cls, boxes, None, _pack_items(items), S, 0, 0, 1200)
    n = len(want["cls"])
    assert n > 2 * 256 and out["count"] == n
    assert np.array_equal(out["cls"][:n], want["cls"].numpy()) and np.array_equal(out["batch_idx"][:n], want["batch_idx"].numpy())
    assert np.abs(out["bboxes"][:n] - want["bboxes"].numpy()).max() <= 2e-5 and np.all(out["batch_idx"][n:] == -1)


@pytest.mark.parametrize("backend", BACKENDS)
def test_labels_more_images_than_one_scan_chunk(backend, engine):
    """B = 300 images: the exclusive scan over the per-image counts runs in chunks of 256 with a carry.  The rows equal those of the same items in three
    calls of 100 images (one chunk each), shifted by their image offset."""
    from yolosharp_amd import augment as A
    imgs, _ = _sources(SHAPES, seed=11)
    _, srcs = A.pack_sources(imgs)
    lab_off, cls, boxes, kp = A.pack_labels(_raw_labels(seed=1, per_source=3))
    base = _label_items(0)
    items = _pack_items([base[(i * 7) % 4][:1] + ((32 + (i * 5) % 64), (32 + (i * 11) % 64)) + base[(i * 7) % 4][3:] for i in range(300)])
    whole = A.augment_labels(engine, srcs, lab_off, cls, boxes, kp, items, S, 0, 0, 3600)
    parts = [A.augment_labels(engine, srcs, lab_off, cls, boxes, kp, items[i:i + 100], S, 0, 0, 1200) for i in (0, 100, 200)]
    n = whole["count"]
    assert n == sum(p["count"] for p in parts) and n > 300
    assert np.array_equal(whole["batch_idx"][:n], np.concatenate([p["batch_idx"][:p["count"]] + 100 * i for i, p in enumerate(parts)]))
    for k in ("cls", "bboxes", "keypoints"):
        assert np.array_equal(whole[k][:n], np.concatenate([p[k][:p["count"]] for p in parts])), k
    assert np.all(whole["batch_idx"][n:] == -1)


# ---------------------------------------------------------------------------------------------------- criterion on padded labels
def _tiny_dataset(seed, n=6, s=32):
    g = np.random.default_rng(seed)
    shapes = [(s, s), (s, 24), (20, s), (s, s), (28, 30), (s, s)][:n]
    imgs, _ = _sources(shapes, seed=seed)
    labels = []
    for h, w in shapes:
        k = 3
        x1, y1 = g.random(k) * w * 0.5, g.random(k) * h * 0.5
        labels.append(dict(cls=g.integers(0, 5, k).astype(np.float32),
                           bboxes=np.stack([x1, y1, x1 + (0.25 + 0.25 * g.random(k)) * w, y1 + (0.25 + 0.25 * g.random(k)) * h], 1).astype(np.float32)))
    return imgs, labels


@pytest.mark.parametrize("backend", BACKENDS)
def test_criterion_on_padded_labels(backend, engine):
    """ys_loss_detect on the compacted device labels with n_labels = capacity returns the same items, bit for bit, as on the first out_count rows alone."""
    from yolosharp_amd import augment as A
    from yolosharp_amd import model as M
    imgs, labels = _tiny_dataset(2)
    aug = A.MosaicAugmenter(engine, imgs, labels, 32, degrees=5.0, seed=3, max_batch=2)
    m = M.Yolov8(engine, nc=5, size="n", height=32, width=32, max_batch=2, dtype="f32")
    m.init_weights(1)
    m.train()
    db = aug.batch([0, 3])
    n = int(engine.from_device(db.count, (1,), np.int32)[0])
    assert 0 < n < db.capacity
    m.reserve_labels(db.max_per_image)
    m.forward_device(db.images, db.batch)
    crit = M.v8DetectionLoss(m)
    crit.forward_device(db.batch_idx, db.cls, db.bboxes, db.capacity)
    _, padded = crit.read()
    crit.forward_device(db.batch_idx, db.cls, db.bboxes, n)
    _, exact = crit.read()
    host = db.to_host()
    _, viahost = crit.forward(None, host)
    assert np.all(np.isfinite(padded)) and padded[0] > 0
    assert np.array_equal(padded, exact) and np.array_equal(padded, viahost), (padded, exact, viahost)
    m.close(); aug.close()


# ---------------------------------------------------------------------------------------------------- trainer
@pytest.mark.parametrize("backend", BACKENDS)
def test_trainer_device_batches(backend, engine):
    """Three train_epoch steps on DeviceBatches from a seeded MosaicAugmenter equal, step for step, the same batches fed through the numpy path."""
    from yolosharp_amd import augment as A
    from yolosharp_amd import model as M
    from yolosharp_amd import trainer as T
    imgs, labels = _tiny_dataset(5)
    order = [[0, 1], [2, 3], [4, 5]]
    got = {}
    for mode in ("device", "host"):
        aug = A.MosaicAugmenter(engine, imgs, labels, 32, degrees=5.0, shear=1.0, seed=9, max_batch=2)
        m = M.Yolov8(engine, nc=5, size="n", height=32, width=32, max_batch=2, dtype="f32")
        m.init_weights(1)
        tr = T.Trainer(m, epochs=1, nb=3, lr0=2e-3, warmup_bias_lr=2e-3)
        steps = []
        for idx in order:                                            # one step per call: the per-step items, not only their sum
            batches = (aug.batch(i) if mode == "device" else aug.batch(i).to_host() for i in [idx])
            steps.append(tr.train_epoch(batches, 1))
            assert tr.steps_run == 1
        got[mode] = np.stack(steps)
        m.close(); aug.close()
    assert got["device"].shape == (3, 3) and np.all(np.isfinite(got["device"])) and np.all(got["device"][:, 1] > 0) and got["device"][:, 0].any()
    assert np.array_equal(got["device"], got["host"]), (got["device"], got["host"])


@pytest.mark.parametrize("backend", BACKENDS)
def test_trainer_skips_a_device_batch_without_input_labels(backend, engine):
    from yolosharp_amd import augment as A
    from yolosharp_amd import model as M
    from yolosharp_amd import trainer as T
    imgs, labels = _tiny_dataset(5)
    empty = [dict(cls=np.zeros((0,), np.float32), bboxes=np.zeros((0, 4), np.float32)) for _ in labels]
    aug = A.MosaicAugmenter(engine, imgs, empty, 32, seed=1, max_batch=2)
    m = M.Yolov8(engine, nc=5, size="n", height=32, width=32, max_batch=2, dtype="f32")
    m.init_weights(1)
    tr = T.Trainer(m, epochs=1, nb=1)
    db = aug.batch([0, 1])
    assert db.n_input == 0 and int(engine.from_device(db.count, (1,), np.int32)[0]) == 0
    assert not tr.train_epoch([db], 1).any() and tr.steps_run == 0
    m.close(); aug.close()


def test_augmenter_draws():
    """random_perspective_matrix's draw order and composition, mosaic4_rects, and the augmenter's index / centre / flip draws (no kernel involved)."""
    from yolosharp_amd import augment as A

    class Seq:                                                       # a generator that hands out a fixed sequence
        def __init__(self, v):
            self.v = list(v)

        def random(self):
            return self.v.pop(0)
    u = [0.9, 0.2, 0.75, 0.6, 0.3, 0.8, 0.55, 0.35]                  # P x, P y, angle, scale, shear x, shear y, translate x, translate y
    M = A.random_perspective_matrix(Seq(u), 64, degrees=10.0, translate=0.1, scale=0.5, shear=2.0, perspective=5e-4)
    d = [2 * x - 1 for x in u]
    Cm, P, Rm, Sm, Tm = (np.eye(3) for _ in range(5))
    Cm[0, 2] = Cm[1, 2] = -64
    P[2, 0], P[2, 1] = d[0] * 5e-4, d[1] * 5e-4
    a, sc = np.deg2rad(d[2] * 10.0), 1 + d[3] * 0.5
    Rm[:2, :2] = [[np.cos(a) * sc, np.sin(a) * sc], [-np.sin(a) * sc, np.cos(a) * sc]]
    Sm[0, 1], Sm[1, 0] = np.tan(np.deg2rad(d[4] * 2.0)), np.tan(np.deg2rad(d[5] * 2.0))
    Tm[0, 2], Tm[1, 2] = (0.5 + d[6] * 0.1) * 64, (0.5 + d[7] * 0.1) * 64
    assert M.dtype == np.float32 and np.allclose(M, Tm @ Sm @ Rm @ P @ Cm, rtol=1e-5, atol=1e-4)
    for i, (h, w) in enumerate([(40, 64), (64, 17), (8, 8), (64, 64)]):
        for xc, yc in ((32, 95), (64, 64), (95, 32)):
            assert A.mosaic4_rects(xc, yc, [(h, w)] * 4, 64)[i] == R.rects(i, xc, yc, h, w, 64)


@pytest.mark.parametrize("backend", BACKENDS)
def test_augmenter_draw_ranges(backend, engine):
    from yolosharp_amd import augment as A
    imgs, labels = _tiny_dataset(5)
    aug = A.MosaicAugmenter(engine, imgs, labels, 32, fliplr=0.5, flipud=0.0, seed=0, max_batch=64)
    it = np.concatenate([aug.draw(list(range(6)) * 10) for _ in range(4)])
    assert it["src"][:, 1:].max() == len(imgs) - 2 and it["src"][:, 1:].min() == 0      # randint(0, Count - 1): the last image is never mixed in
    assert it["xc"].min() == 16 and it["xc"].max() == 47 and it["yc"].min() == 16 and it["yc"].max() == 47
    assert 0.3 < it["flip_lr"].mean() < 0.7 and not it["flip_ud"].any()
    aug.close()


# ---------------------------------------------------------------------------------------------------- boundaries
@pytest.mark.parametrize("backend", BACKENDS)
def test_boundaries(backend, engine):
    from yolosharp_amd import YsError
    from yolosharp_amd import augment as A
    imgs, masks = _sources(SHAPES, seed=11)
    arena, srcs = A.pack_sources(imgs, masks)
    labels = _raw_labels(seed=1, per_source=3)
    lab_off, cls, boxes, kp = A.pack_labels(labels)
    good = ([0, 1, 2, 3], 40, 50, _matrix(S, scale=0.9), 0, 1)

    def bad(**kw):
        src, xc, yc, M, flr, fud = good
        d = dict(src=src, xc=xc, yc=yc, M=M)
        d.update(kw)
        return _pack_items([(d["src"], d["xc"], d["yc"], d["M"], flr, fud)])
    singular = np.array([[1, 2, 3], [2, 4, 6], [0, 0, 1]], np.float32)
    cases = [dict(items=bad(src=[0, 1, 2, len(SHAPES)])), dict(items=bad(src=[-1, 1, 2, 3])), dict(items=bad(xc=2 * S + 1)), dict(items=bad(yc=-1)),
             dict(items=bad(M=singular)), dict(items=bad(M=np.zeros((3, 3), np.float32))), dict(imgsz=63), dict(imgsz=0)]
    for c in cases:
        with pytest.raises(YsError) as e:
            A.augment_mosaic(engine, arena, srcs, c.get("items", _pack_items([good])), c.get("imgsz", S), RATIO, 0, with_masks=True)
        assert e.value.status == 1, c
    with pytest.raises(YsError) as e:                                # mask_ratio that does not divide imgsz
        A.augment_mosaic(engine, arena, srcs, _pack_items([good]), S, 5, 0, with_masks=True)
    assert e.value.status == 1
    lcases = [dict(items=bad(src=[-1, 1, 2, 3])), dict(items=bad(xc=2 * S + 1)), dict(items=bad(M=singular)), dict(imgsz=63), dict(imgsz=0),
              dict(capacity=11), dict(kpt_dim=2), dict(flags=2)]   # 4 x 3 labels need 12 rows
    for c in lcases:
        with pytest.raises(YsError) as e:
            A.augment_labels(engine, srcs, lab_off, cls, boxes, kp, c.get("items", _pack_items([good])), c.get("imgsz", S), 0, c.get("flags", 0),
                             c.get("capacity", 12), kpt_dim=c.get("kpt_dim", 3))
        assert e.value.status == 1, c
    # the singularity test carries the matrix's own scale: a sound half-scale matrix for imgsz 8192 (translation of thousands of pixels) is accepted
    big = _pack_items([([5, 5, 5, 5], 8192, 8192, _matrix(8192, scale=0.5), 0, 0)])
    assert A.augment_labels(engine, srcs, lab_off, cls, boxes, kp, big, 8192, 0, 0, 12)["count"] >= 0
    with pytest.raises(YsError):
        A.augment_labels(engine, srcs, lab_off, cls, boxes, kp, _pack_items([([5, 5, 5, 5], 8192, 8192, singular * 4096, 0, 0)]), 8192, 0, 0, 12)
    out = A.augment_labels(engine, srcs, lab_off, cls, boxes, kp, _pack_items([good]), S, 0, 0, 12)      # exactly enough
    assert 0 <= out["count"] <= 12


@pytest.mark.parametrize("backend", BACKENDS)
def test_host_and_device_pointers_agree(backend, engine):
    """on_device = 0 (the calls above) and on_device = 1 (MosaicAugmenter.run: resident arena, label tables and items) give the same bytes; a refused
    DEVICE item yields an all-114 image and no labels."""
    from yolosharp_amd import augment as A
    imgs, masks = _sources(SHAPES, seed=11)
    labels = _raw_labels(seed=1, per_source=4)
    items = _pack_items(_label_items(0))
    aug = A.MosaicAugmenter(engine, imgs, labels, S, masks=masks, mask_ratio=RATIO, seed=0, max_batch=4)
    dev = aug.run(items).to_host()
    arena, srcs = A.pack_sources(imgs, masks)
    lab_off, cls, boxes, kp = A.pack_labels(labels)
    images, mks = A.augment_mosaic(engine, arena, srcs, items, S, RATIO, 0, with_masks=True)
    out = A.augment_labels(engine, srcs, lab_off, cls, boxes, kp, items, S, 0, 0, aug.capacity)
    n = out["count"]
    assert np.array_equal(dev["images"], images) and np.array_equal(dev["masks"], mks)
    assert len(dev["cls"]) == n and all(np.array_equal(dev[k], out[k][:n]) for k in ("batch_idx", "cls", "bboxes", "keypoints"))
    broken = items.copy()
    broken[1]["xc"] = -5                                            # a device item the host does not read
    host = aug.run(broken).to_host()
    assert np.array_equal(host["images"][1], np.full((3, S, S), 114, np.float32) * np.float32(1 / 255.0)) and not host["masks"][1].any()
    assert not (host["batch_idx"] == 1).any() and np.array_equal(host["images"][0], images[0]) and (host["batch_idx"] == 0).any()
    aug.close()
