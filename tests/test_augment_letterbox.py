"""The LetterBox (close-mosaic) branch of the device training input (csrc/augment.hip: ys_augment_letterbox / ys_augment_letterbox_labels,
yolosharp_amd/augment.py MosaicAugmenter.close_mosaic, Trainer.fit(augmenter=...)) against tests/aug_letterbox_ref.py, the torch restatement of
Data/Augment.cs:698-778, 860-966, Data/YoloDataset.cs:102-151 and Data/Struct.cs:99-121.

Images and masks: nothing is blended in this branch, so they are judged BIT FOR BIT -- every output float equals byte * (1 / 255.0f) of the
restatement's byte, every mask id is equal; no pixel is exempted and there is no tolerance.
Labels: nothing is filtered, so count, order, batch_idx, cls and visibility are exact.  Coordinates agree within 2e-6 normalised with the float64
restatement fed the same fp32 xyxy tables: the chain is at most four fp32 roundings at magnitude <= 2s (the sum, the pad add, s - x, the multiply by
the rounded 1 / s), under 2e-7 normalised at s = 64 and at s = 640; the tolerance leaves 10x."""
import functools

import numpy as np
import pytest
import torch

import aug_letterbox_ref as R
from conftest import BACKENDS

S, RATIO, KPT, TOL = 64, 4, 5, 2e-6
# (h, w): three identity resizes; odd height (mask pads off the image grid); odd width (every later source starts at an odd arena offset); 8x up-sampling;
# neither side equals s (ratio 1.333...); ratio < 1
SHAPES = [(64, 48), (40, 64), (64, 64), (33, 64), (64, 17), (8, 8), (33, 48), (96, 80)]
FLIPS = [(0, 0), (1, 0), (0, 1), (1, 1)]


def _sources(shapes, seed, ratio=RATIO):
    """uint8 RGB planes = seeded noise + a smooth ramp, and id masks (blocks of small ids) of the size the dataset builds them at (h / r, w / r)."""
    g = np.random.default_rng(seed)
    imgs, masks = [], []
    for h, w in shapes:
        yy, xx = np.mgrid[0:h, 0:w]
        ramp = (xx * 97.0 / max(w - 1, 1) + yy * 89.0 / max(h - 1, 1))[None] + np.array([0.0, 20.0, 40.0])[:, None, None]
        imgs.append(np.clip(ramp + g.integers(0, 70, (3, h, w)), 0, 255).astype(np.uint8))
        masks.append(g.integers(1, 7, (max(h // ratio, 1), max(w // ratio, 1))).astype(np.uint8))
    return imgs, masks


def _raw_labels(shapes, seed, per_source=10, kpt=KPT):
    g = np.random.default_rng(seed)
    labels, uid = [], 0
    for (h, w), n in zip(shapes, per_source if isinstance(per_source, (list, tuple)) else [per_source] * len(shapes)):
        x1, y1 = g.random(n) * w * 0.8, g.random(n) * h * 0.8
        bw, bh = (0.08 + g.random(n) * 0.5) * w, (0.08 + g.random(n) * 0.5) * h
        boxes = np.stack([x1, y1, np.minimum(x1 + bw, w), np.minimum(y1 + bh, h)], 1).astype(np.float32).reshape(n, 4)
        kp = None
        if kpt:
            kp = np.concatenate([boxes[:, None, :2] + g.random((n, kpt, 2)) * (boxes[:, None, 2:] - boxes[:, None, :2]),
                                 g.integers(0, 3, (n, kpt, 1))], 2).astype(np.float32)
        labels.append(dict(cls=np.arange(uid, uid + n, dtype=np.float32), bboxes=boxes, keypoints=kp))     # cls = a unique id: set and order are visible
        uid += n
    return labels


def _pack_items(lst):
    """(src, flip_lr, flip_ud) -> item table.  The fields this branch must ignore carry values the Mosaic entries refuse."""
    from yolosharp_amd import augment as A
    it = A.make_items(len(lst))
    for b, (k, flr, fud) in enumerate(lst):
        it[b]["src"], it[b]["xc"], it[b]["yc"], it[b]["flip_lr"], it[b]["flip_ud"] = (k, -1, 10 ** 6, -7), -3, 10 ** 6, flr, fud
    return it


def _pack_odd(imgs, masks=None):
    """pack_sources behind one leading byte: a source behind even-sized ones (3 * h * w and mh * mw are even for most shapes used here) starts at an
    ODD arena offset, and the rows of an odd-width source alternate between odd and even addresses."""
    from yolosharp_amd import augment as A
    arena, srcs = A.pack_sources(imgs, masks)
    srcs["img_off"] += 1
    srcs["mask_off"][srcs["mask_off"] >= 0] += 1
    assert sum(int(o) % 2 for o in srcs["img_off"]) >= 2
    return np.ascontiguousarray(np.concatenate([np.array([201], np.uint8), arena])), srcs


def _ref_images(imgs, masks, lst, s, r):
    """(images fp32 [B, 3, s, s], bytes uint8, masks fp32 [B, s/r, s/r] or None) of the restatement."""
    outs = [R.image_sample(torch.from_numpy(imgs[k]), torch.from_numpy(masks[k]) if masks is not None else None, flr, fud, s, r) for k, flr, fud in lst]
    by = torch.stack([o[0] for o in outs])
    mk = torch.stack([o[1] for o in outs]).to(torch.float32).numpy() if masks is not None else None
    return R.to_float(by).numpy(), by.numpy(), mk


def _assert_images(images, mks, want):
    wf, wb, wm = want
    assert images.dtype == np.float32 and images.shape == wf.shape
    assert np.array_equal(np.rint(images * np.float32(255.0)).astype(np.int64), wb.astype(np.int64))       # the bytes are the restatement's
    assert images.tobytes() == wf.tobytes()                                                              # and the floats byte * (1 / 255.0f), bit for bit
    if wm is None:
        assert mks is None
    else:
        assert mks.shape == wm.shape and mks.tobytes() == wm.tobytes()


def _ref_labels(labels, shapes, lst, s, dtype, keep_size):
    return {k: (v.numpy() if v is not None else None) for k, v in
            R.collate([R.labels_sample(labels[k], shapes[k][0], shapes[k][1], flr, fud, s, dtype, keep_size) for k, flr, fud in lst]).items()}


def _assert_labels(out, want, cap, tol=TOL):
    n = len(want["cls"])
    assert out["count"] == n
    assert np.array_equal(out["batch_idx"][:n], want["batch_idx"]) and np.array_equal(out["cls"][:n], want["cls"])
    assert np.all(out["batch_idx"][n:cap] == -1) and not out["cls"][n:cap].any() and not out["bboxes"][n:cap].any()
    err = np.abs(out["bboxes"][:n].astype(np.float64) - want["bboxes"]).max() if n else 0.0
    kerr = 0.0
    if want.get("keypoints") is not None:
        assert not out["keypoints"][n:cap].any()
        if n:
            kerr = np.abs(out["keypoints"][:n, :, :2].astype(np.float64) - want["keypoints"][..., :2]).max()
            assert np.array_equal(out["keypoints"][:n, :, 2], want["keypoints"][..., 2].astype(np.float32))         # visibility untouched
    print("%d rows: box error %.3g, keypoint error %.3g (bound %.1g)" % (n, err, kerr, tol))
    assert err <= tol and kerr <= tol, (err, kerr)


@functools.lru_cache(maxsize=None)
def _small_case():
    """Sources, the 32 items (every source under every flip combination) and the restatement's images, computed once and never modified."""
    imgs, masks = _sources(SHAPES, seed=11)
    lst = [(k, flr, fud) for k in range(len(SHAPES)) for flr, fud in FLIPS]
    return imgs, masks, lst, _ref_images(imgs, masks, lst, S, RATIO)


# ---------------------------------------------------------------------------------------------------- images
def test_restatement_resize_agrees_with_aten():
    """The formula the restatement resizes with and ATen's interpolate(mode="nearest") on fp32 give the same planes on every shape used here, and the
    geometry is what the issue's table says it is."""
    shapes = [(s, h, w) for s in (S,) for h, w in SHAPES] + [(S // RATIO, max(h // RATIO, 1), max(w // RATIO, 1)) for h, w in SHAPES]
    shapes += [(62, 62, 47), (62, 31, 62), (62, 9, 7), (62, 80, 100), (640, 427, 640), (640, 639, 480), (640, 1, 1), (160, 106, 160), (160, 159, 120)]
    g = np.random.default_rng(0)
    for out, h, w in shapes:
        new_w, new_h, pad_l, pad_u = R.geometry(h, w, out)
        assert 0 < new_w <= out and 0 < new_h <= out and max(new_w, new_h) == out and pad_l >= 0 and pad_u >= 0, (out, h, w)
        img = torch.from_numpy(g.integers(0, 256, (2, h, w)).astype(np.uint8))
        assert torch.equal(R.resize_nearest(img, new_h, new_w), R.resize_nearest_aten(img, new_h, new_w)), (out, h, w)
    assert R.geometry(33, 64, 64) == (64, 33, 0, 15) and R.geometry(8, 16, 16) == (16, 8, 0, 4)          # 15 / 4 != 4: mask pads off the image grid
    assert R.geometry(33, 48, 64) == (64, 44, 0, 10) and R.geometry(96, 80, 64) == (53, 64, 5, 0) and R.geometry(8, 8, 64) == (64, 64, 0, 0)


@pytest.mark.parametrize("backend", BACKENDS)
def test_image_and_mask_bit_exact(backend, engine):
    from yolosharp_amd import augment as A
    imgs, masks, lst, want = _small_case()
    arena, srcs = _pack_odd(imgs, masks)
    for i0 in range(0, len(lst), 3):                                 # B = 3 per call
        items = _pack_items(lst[i0:i0 + 3])
        sl = tuple(w[i0:i0 + 3] for w in want)
        images, mks = A.augment_letterbox(engine, arena, srcs, items, S, RATIO, with_masks=True)
        _assert_images(images, mks, sl)
        images2, none = A.augment_letterbox(engine, arena, srcs, items, S, RATIO, with_masks=False)      # without masks: the same images
        _assert_images(images2, none, (sl[0], sl[1], None))
    items = _pack_items(lst[9:12])
    a1, m1 = A.augment_letterbox(engine, arena, srcs, items, S, RATIO, with_masks=True)
    a2, m2 = A.augment_letterbox(engine, arena, srcs, items, S, RATIO, with_masks=True)
    assert a1.tobytes() == a2.tobytes() and m1.tobytes() == m2.tobytes()                                  # a second call is bit-identical
    assert (want[1] == 114).mean() > 0.1 and (want[2] == 0).mean() > 0.1                                  # the padding is really there


@pytest.mark.parametrize("backend", BACKENDS)
def test_image_scalar_store_path(backend, engine):
    """imgsz = 62 (no multiple of 4: scalar stores, a partial last quad), images only."""
    from yolosharp_amd import augment as A
    s, shapes = 62, [(62, 47), (31, 62), (62, 62), (9, 7), (80, 100)]
    imgs, _ = _sources(shapes, seed=3)
    arena, srcs = _pack_odd(imgs)
    lst = [(k, flr, fud) for k in range(len(shapes)) for flr, fud in FLIPS][:18]
    want = _ref_images(imgs, None, lst, s, 1)
    for i0 in range(0, len(lst), 3):
        images, none = A.augment_letterbox(engine, arena, srcs, _pack_items(lst[i0:i0 + 3]), s, RATIO, with_masks=False)
        _assert_images(images, none, (want[0][i0:i0 + 3], want[1][i0:i0 + 3], None))


# ---------------------------------------------------------------------------------------------------- labels
@pytest.mark.parametrize("backend", BACKENDS)
def test_label_parity(backend, engine):
    from yolosharp_amd import augment as A
    imgs, _, lst, _ = _small_case()
    labels = _raw_labels(SHAPES, seed=21)
    _, srcs = A.pack_sources(imgs)
    lab_off, cls, boxes, kp = A.pack_labels(labels)
    items = _pack_items(lst)
    total = 10 * len(lst)
    cap = total + 7
    widths = np.concatenate([labels[k]["bboxes"][:, 2] - labels[k]["bboxes"][:, 0] for k, _, _ in lst]).astype(np.float64)
    heights = np.concatenate([labels[k]["bboxes"][:, 3] - labels[k]["bboxes"][:, 1] for k, _, _ in lst]).astype(np.float64)
    flr = np.repeat([f for _, f, _ in lst], 10).astype(bool)
    fud = np.repeat([f for _, _, f in lst], 10).astype(bool)
    for flags in (0, A.YS_AUG_FLIP_KEEP_SIZE, A.YS_AUG_FLIP_KEEP_SIZE | A.YS_AUG_SORT_FLIPPED, A.YS_AUG_SORT_FLIPPED):
        keep = bool(flags & A.YS_AUG_FLIP_KEEP_SIZE)                 # YS_AUG_SORT_FLIPPED is ignored by this entry
        want = _ref_labels(labels, SHAPES, lst, S, torch.float64, keep)
        out = A.augment_letterbox_labels(engine, srcs, lab_off, cls, boxes, kp, items, S, flags, cap)
        assert out["count"] == total                                 # no label is removed: there are no thresholds in this branch
        _assert_labels(out, want, cap)
        # the reference's flip rewrites column 2 (3) of a cxcywh box as s - value: a flipped box's width is s - w by default, w under the flag
        w_out, h_out = out["bboxes"][:total, 2].astype(np.float64) * S, out["bboxes"][:total, 3].astype(np.float64) * S
        assert np.abs(w_out - np.where(flr & ~np.bool_(keep), S - widths, widths)).max() <= TOL * S
        assert np.abs(h_out - np.where(fud & ~np.bool_(keep), S - heights, heights)).max() <= TOL * S
        assert flr.any() and (~flr).any() and np.abs((S - widths) - widths).min() > 1e-3                  # the two readings differ on every flipped row
        again = A.augment_letterbox_labels(engine, srcs, lab_off, cls, boxes, kp, items, S, flags, cap)
        assert all(out[k].tobytes() == again[k].tobytes() for k in ("batch_idx", "cls", "bboxes", "keypoints")) and again["count"] == total
    vis = out["keypoints"][:total, :, 2]
    assert (vis == 0).any() and (vis == 2).any()
    # the fp32 restatement -- the reference's own arithmetic -- is matched to the last bit
    want32 = _ref_labels(labels, SHAPES, lst, S, torch.float32, False)
    out = A.augment_letterbox_labels(engine, srcs, lab_off, cls, boxes, kp, items, S, 0, cap)
    assert np.array_equal(out["bboxes"][:total], want32["bboxes"]) and np.array_equal(out["keypoints"][:total], want32["keypoints"])
    # without keypoints: the same rows
    nok = A.augment_letterbox_labels(engine, srcs, lab_off, cls, boxes, None, items, S, 0, cap)
    assert nok["keypoints"] is None and nok["count"] == total and np.array_equal(nok["bboxes"], out["bboxes"]) and np.array_equal(nok["cls"], out["cls"])


@pytest.mark.parametrize("backend", BACKENDS)
def test_labels_more_than_one_chunk(backend, engine):
    """One image with 300 labels (the workgroup walks them in chunks of 256) between two small ones: offsets 0, 5, 305; order and tail exact."""
    from yolosharp_amd import augment as A
    shapes = [(64, 64), (40, 64)]
    labels = _raw_labels(shapes, seed=4, per_source=[300, 5])
    _, srcs = A.pack_sources([np.zeros((3,) + hw, np.uint8) for hw in shapes])
    lab_off, cls, boxes, kp = A.pack_labels(labels)
    lst = [(1, 0, 0), (0, 1, 0), (1, 0, 1)]
    out = A.augment_letterbox_labels(engine, srcs, lab_off, cls, boxes, kp, _pack_items(lst), S, 0, 400)
    _assert_labels(out, _ref_labels(labels, shapes, lst, S, torch.float64, False), 400)
    assert out["count"] == 310 and np.array_equal(np.flatnonzero(np.diff(out["batch_idx"][:310])), [4, 304])
    assert np.array_equal(out["cls"][5:305], labels[0]["cls"])


@pytest.mark.parametrize("backend", BACKENDS)
def test_labels_more_images_than_one_scan_chunk(backend, engine):
    """B = 300 images at s = 8: the exclusive scan over the per-image counts runs in chunks of 256 with a carry."""
    from yolosharp_amd import augment as A
    s, shapes = 8, [(8, 8), (8, 5), (3, 8), (8, 8), (6, 7)]
    counts = [2, 0, 3, 1, 4]
    labels = _raw_labels(shapes, seed=6, per_source=counts)
    imgs, _ = _sources(shapes, seed=6)
    arena, srcs = A.pack_sources(imgs)
    lab_off, cls, boxes, kp = A.pack_labels(labels)
    lst = [((i * 7) % 5, i % 2, (i // 2) % 2) for i in range(300)]
    total = sum(counts[k] for k, _, _ in lst)
    out = A.augment_letterbox_labels(engine, srcs, lab_off, cls, boxes, kp, _pack_items(lst), s, 0, total + 50)
    _assert_labels(out, _ref_labels(labels, shapes, lst, s, torch.float64, False), total + 50)
    offs = np.concatenate([[0], np.cumsum([counts[k] for k, _, _ in lst])])
    assert out["count"] == total == offs[-1] and total > 256
    for b in (0, 1, 255, 256, 257, 299):
        assert np.array_equal(np.flatnonzero(out["batch_idx"][:total] == b), np.arange(offs[b], offs[b + 1]))
    images, _ = A.augment_letterbox(engine, arena, srcs, _pack_items(lst), s, 2, with_masks=False)
    _assert_images(images, None, _ref_images(imgs, None, lst, s, 1))


# ---------------------------------------------------------------------------------------------------- boundaries
def _device_call(engine, A, imgs, masks, labels, items, s, r, cap, sentinel=None):
    """Both entries on DEVICE pointers -> (images, masks, dict of label arrays `cap` + 1 rows long, count).  The output buffers are filled with `sentinel`
    beforehand and are one row longer than the capacity the library is told."""
    import ctypes as C
    from yolosharp_amd import _lib
    e, lib = engine, engine.lib
    arena, srcs = A.pack_sources(imgs, masks)
    lab_off, cls, boxes, kp = A.pack_labels(labels)
    B, K, n_src = len(items), kp.shape[1], len(imgs)
    fill = np.float32(sentinel if sentinel is not None else 0)
    host = dict(images=np.full((B, 3, s, s), fill, np.float32), masks=np.full((B, s // r, s // r), fill, np.float32),
                batch_idx=np.full((cap + 1,), fill, np.float32), cls=np.full((cap + 1,), fill, np.float32), bboxes=np.full((cap + 1, 4), fill, np.float32),
                keypoints=np.full((cap + 1, K, 3), fill, np.float32), count=np.full((1,), -5, np.int32))
    ins = [e.to_device(a) for a in (arena, srcs, lab_off, cls if cls.size else np.zeros(1, np.float32), boxes if boxes.size else np.zeros(4, np.float32),
                                    kp if kp.size else np.zeros(3, np.float32), np.ascontiguousarray(items))]
    d = {k: e.to_device(v) for k, v in host.items()}
    try:
        _lib.check(lib, lib.ys_augment_letterbox(e.ctx, ins[0], ins[1], n_src, ins[6], B, 1, s, r, d["images"], d["masks"]))
        _lib.check(lib, lib.ys_augment_letterbox_labels(e.ctx, ins[1], n_src, ins[2], ins[3], ins[4], ins[5], K, 3, ins[6], B, 1, s, 0, cap, d["batch_idx"], d["cls"],
                                                        d["bboxes"], d["keypoints"], d["count"]))
        return {k: e.from_device(d[k], v.shape, v.dtype) for k, v in host.items()}
    finally:
        for p in ins + list(d.values()):
            e.free(p)


@pytest.mark.parametrize("backend", BACKENDS)
def test_boundaries(backend, engine):
    from yolosharp_amd import YsError
    from yolosharp_amd import augment as A
    imgs, masks, _, _ = _small_case()
    arena, srcs = A.pack_sources(imgs, masks)
    labels = _raw_labels(SHAPES, seed=1, per_source=3)
    lab_off, cls, boxes, kp = A.pack_labels(labels)
    good = [(0, 0, 1), (3, 1, 0)]

    def with_src(k):
        it = _pack_items(good)
        it[1]["src"][0] = k
        return it
    for c in (dict(items=with_src(len(SHAPES))), dict(items=with_src(-1)), dict(imgsz=63), dict(imgsz=0)):
        with pytest.raises(YsError) as e:
            A.augment_letterbox(engine, arena, srcs, c.get("items", _pack_items(good)), c.get("imgsz", S), RATIO, with_masks=True)
        assert e.value.status == 1, c
    with pytest.raises(YsError) as e:                                # mask_ratio that does not divide imgsz
        A.augment_letterbox(engine, arena, srcs, _pack_items(good), S, 5, with_masks=True)
    assert e.value.status == 1
    for c in (dict(items=with_src(len(SHAPES))), dict(items=with_src(-1)), dict(imgsz=63), dict(imgsz=0), dict(kpt_dim=2), dict(capacity=5), dict(flags=4)):
        with pytest.raises(YsError) as e:                            # 2 x 3 labels need 6 rows
            A.augment_letterbox_labels(engine, srcs, lab_off, cls, boxes, kp, c.get("items", _pack_items(good)), c.get("imgsz", S), c.get("flags", 0),
                                       c.get("capacity", 6), kpt_dim=c.get("kpt_dim", 3))
        assert e.value.status == 1, c
    out = A.augment_letterbox_labels(engine, srcs, lab_off, cls, boxes, kp, _pack_items(good), S, 0, 6)    # exactly enough
    assert out["count"] == 6 and np.all(out["batch_idx"] == [0, 0, 0, 1, 1, 1])


@pytest.mark.parametrize("backend", BACKENDS)
def test_label_free_source(backend, engine):
    """A source without labels between two with labels: its image is produced, it contributes no row; a batch of such sources has n_input == 0."""
    from yolosharp_amd import augment as A
    imgs, masks, _, _ = _small_case()
    labels = _raw_labels(SHAPES, seed=1, per_source=[3, 0, 2, 0, 0, 0, 0, 0])
    aug = A.MosaicAugmenter(engine, imgs, labels, S, masks=masks, mask_ratio=RATIO, seed=0, max_batch=3)
    aug.close_mosaic(True)
    lst = [(0, 0, 0), (1, 1, 0), (2, 0, 1)]
    db = aug.run(_pack_items(lst))
    host = db.to_host()
    assert db.mode == "letterbox" and db.n_input == 5 and np.array_equal(host["batch_idx"], [0, 0, 0, 2, 2])
    _assert_images(host["images"], host["masks"], _ref_images(imgs, masks, lst, S, RATIO))
    lst = [(1, 0, 0), (4, 1, 1)]
    db = aug.run(_pack_items(lst))
    host = db.to_host()
    assert db.n_input == 0 and len(host["cls"]) == 0 and int(engine.from_device(db.count, (1,), np.int32)[0]) == 0
    _assert_images(host["images"], host["masks"], _ref_images(imgs, masks, lst, S, RATIO))
    aug.close()


@pytest.mark.parametrize("backend", BACKENDS)
def test_host_and_device_pointers_agree(backend, engine):
    """on_device = 0 and on_device = 1 give the same bytes; a refused DEVICE item yields an all-114 image, a zero mask and no rows, its neighbours intact;
    a capacity one below the total reports the true total and leaves the row past capacity unwritten."""
    from yolosharp_amd import augment as A
    imgs, masks, _, _ = _small_case()
    labels = _raw_labels(SHAPES, seed=1, per_source=4)
    arena, srcs = A.pack_sources(imgs, masks)
    lab_off, cls, boxes, kp = A.pack_labels(labels)
    lst = [(3, 1, 0), (7, 0, 1), (4, 1, 1), (6, 0, 0)]
    items = _pack_items(lst)
    cap = 20
    images, mks = A.augment_letterbox(engine, arena, srcs, items, S, RATIO, with_masks=True)
    out = A.augment_letterbox_labels(engine, srcs, lab_off, cls, boxes, kp, items, S, 0, cap)
    dev = _device_call(engine, A, imgs, masks, labels, items, S, RATIO, cap, sentinel=77.0)
    assert dev["count"][0] == out["count"] == 16
    assert dev["images"].tobytes() == images.tobytes() and dev["masks"].tobytes() == mks.tobytes()
    assert all(dev[k][:cap].tobytes() == out[k].tobytes() for k in ("batch_idx", "cls", "bboxes", "keypoints"))
    assert np.all(dev["batch_idx"][cap] == 77) and np.all(dev["keypoints"][cap] == 77)                   # the row behind the buffer's capacity is untouched
    # the augmenter (resident tables) gives the same batch
    aug = A.MosaicAugmenter(engine, imgs, labels, S, masks=masks, mask_ratio=RATIO, seed=0, max_batch=4)
    aug.close_mosaic(True)
    host = aug.run(items).to_host()
    assert host["images"].tobytes() == images.tobytes() and host["masks"].tobytes() == mks.tobytes() and len(host["cls"]) == 16
    assert all(host[k].tobytes() == out[k][:16].tobytes() for k in ("batch_idx", "cls", "bboxes", "keypoints"))
    aug.close()
    # a device item the host does not read
    for bad in (len(SHAPES), -1):
        broken = items.copy()
        broken[1]["src"][0] = bad
        dev2 = _device_call(engine, A, imgs, masks, labels, broken, S, RATIO, cap, sentinel=77.0)
        assert dev2["images"][1].tobytes() == (np.full((3, S, S), 114, np.float32) * np.float32(1 / 255.0)).tobytes() and not dev2["masks"][1].any()
        assert dev2["count"][0] == 12 and not (dev2["batch_idx"][:cap] == 1).any()
        for b in (0, 2, 3):
            assert dev2["images"][b].tobytes() == images[b].tobytes() and dev2["masks"][b].tobytes() == mks[b].tobytes()
            assert dev2["bboxes"][:cap][dev2["batch_idx"][:cap] == b].tobytes() == out["bboxes"][out["batch_idx"] == b].tobytes()
    # overflow: the true total, nothing behind the capacity
    dev3 = _device_call(engine, A, imgs, masks, labels, items, S, RATIO, 15, sentinel=77.0)
    assert dev3["count"][0] == 16
    assert all(dev3[k][:15].tobytes() == out[k][:15].tobytes() for k in ("batch_idx", "cls", "bboxes", "keypoints"))
    assert all(np.all(dev3[k][15] == 77) for k in ("batch_idx", "cls", "bboxes", "keypoints"))


# ---------------------------------------------------------------------------------------------------- augmenter
def _tiny_dataset(seed, n=6, s=32, kpt=0):
    g = np.random.default_rng(seed)
    shapes = [(s, s), (s, 24), (20, s), (s, s), (28, 30), (s, s)][:n]
    imgs, masks = _sources(shapes, seed=seed)
    labels = []
    for h, w in shapes:
        k = 3
        x1, y1 = g.random(k) * w * 0.5, g.random(k) * h * 0.5
        boxes = np.stack([x1, y1, x1 + (0.25 + 0.25 * g.random(k)) * w, y1 + (0.25 + 0.25 * g.random(k)) * h], 1).astype(np.float32)
        lab = dict(cls=g.integers(0, 5, k).astype(np.float32), bboxes=boxes)
        if kpt:
            lab["keypoints"] = np.concatenate([boxes[:, None, :2] + g.random((k, kpt, 2)) * (boxes[:, None, 2:] - boxes[:, None, :2]),
                                               g.integers(1, 3, (k, kpt, 1))], 2).astype(np.float32)
        labels.append(lab)
    return shapes, imgs, masks, labels


class _Recorder:
    """A numpy Generator that counts what is drawn from it."""

    def __init__(self, seed):
        self.g, self.uniforms, self.others = np.random.default_rng(seed), 0, 0

    def random(self, size=None):
        self.uniforms += 1 if size is None else int(np.prod(size))
        return self.g.random(size)

    def integers(self, *a, **k):
        self.others += 1
        return self.g.integers(*a, **k)

    def permutation(self, *a, **k):
        self.others += 1
        return self.g.permutation(*a, **k)


@pytest.mark.parametrize("backend", BACKENDS)
def test_augmenter_close_mosaic(backend, engine):
    from yolosharp_amd import augment as A
    s = 32
    shapes, imgs, masks, labels = _tiny_dataset(5)
    hyp = dict(degrees=5.0, shear=1.0)
    # never closed: today's draws and today's bytes (a second instance that was closed and re-opened without drawing, and draw_items itself)
    a1 = A.MosaicAugmenter(engine, imgs, labels, s, masks=masks, mask_ratio=RATIO, seed=9, max_batch=4, **hyp)
    a2 = A.MosaicAugmenter(engine, imgs, labels, s, masks=masks, mask_ratio=RATIO, seed=9, max_batch=4, **hyp)
    a2.close_mosaic(True); a2.close_mosaic(False)
    assert a1.mode == a2.mode == "mosaic"
    i1, i2 = a1.draw([0, 3, 5, 1]), a2.draw([0, 3, 5, 1])
    want = A.draw_items(np.random.default_rng(9), [0, 3, 5, 1], s, len(imgs), a1.hyp, 0.5, 0.0)
    assert i1.tobytes() == i2.tobytes() == want.tobytes()
    b1, b2 = a1.run(i1), a2.run(i2)
    assert b1.mode == b2.mode == "mosaic"
    h1, h2 = b1.to_host(), b2.to_host()
    assert sorted(h1) == sorted(h2) and all(h1[k].tobytes() == h2[k].tobytes() for k in h1)
    a2.close()
    # closed: one uniform per image with fliplr = 0.5, flipud = 0, nothing else
    a1.rng = rec = _Recorder(3)
    a1.close_mosaic(True)
    idx = [4, 1, 2, 0]
    items = a1.draw(idx)
    assert a1.mode == "letterbox" and rec.uniforms == len(idx) and rec.others == 0
    u = np.random.default_rng(3).random(len(idx))
    assert np.array_equal(items["src"][:, 0], idx) and np.array_equal(items["flip_lr"], (~(u > 0.5)).astype(np.int32)) and not items["flip_ud"].any()
    both = A.draw_letterbox_items(_Recorder(3), idx, 0.5, 0.25)      # FlipLR, then FlipUD, per image
    u2 = np.random.default_rng(3).random(2 * len(idx))
    assert np.array_equal(both["flip_lr"], (~(u2[0::2] > 0.5)).astype(np.int32)) and np.array_equal(both["flip_ud"], (~(u2[1::2] > 0.25)).astype(np.int32))
    rec0 = _Recorder(3)
    assert not A.draw_letterbox_items(rec0, idx, 0.0, 0.0)["flip_lr"].any() and rec0.uniforms == 0
    # the batch equals the restatement
    db = a1.run(items)
    host = db.to_host()
    lst = [(int(k), int(f), 0) for k, f in zip(idx, items["flip_lr"])]
    assert db.mode == "letterbox" and db.n_input == 12 == len(host["cls"])
    _assert_images(host["images"], host["masks"], _ref_images(imgs, masks, lst, s, RATIO))
    want = _ref_labels([dict(l, keypoints=None) for l in labels], shapes, lst, s, torch.float64, False)
    got = dict(host, count=len(host["cls"]), keypoints=None)
    _assert_labels(got, want, len(host["cls"]))
    # ... and through batches(): one epoch of letterbox batches
    seen = list(a1.batches(2, shuffle=True))
    assert len(seen) == 3 and all(b.mode == "letterbox" for b in seen)
    # re-opened: mosaic items again
    a1.close_mosaic(False)
    it = np.concatenate([a1.draw(list(range(6)) * 10) for _ in range(2)])
    assert a1.mode == "mosaic" and it["xc"].min() >= s // 2 and it["xc"].max() < s + s // 2 and it["yc"].min() >= s // 2 and it["yc"].max() < s + s // 2
    assert it["xc"].min() == 16 and it["xc"].max() == 47
    a1.close()


# ---------------------------------------------------------------------------------------------------- criterion
@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("task", ["detect", "segment", "pose"])
def test_train_step_on_letterbox_batch(backend, engine, task):
    """AMPWrapper.TrainStepDevice on a letterbox DeviceBatch returns the same loss items, bit for bit, as TrainStep on its to_host() (the comparison
    test_criterion_on_padded_labels makes for the Mosaic branch)."""
    from yolosharp_amd import augment as A
    from yolosharp_amd import model as M
    s = 32
    kpt = 4 if task == "pose" else 0
    shapes, imgs, masks, labels = _tiny_dataset(2, kpt=kpt)
    cls_, crit_ = {"detect": (M.Yolov8, M.v8DetectionLoss), "segment": (M.Yolov8Segment, M.v8SegmentationLoss), "pose": (M.Yolov8Pose, M.v8PoseLoss)}[task]
    aug = A.MosaicAugmenter(engine, imgs, labels, s, masks=masks if task == "segment" else None, mask_ratio=RATIO, seed=3, max_batch=2,
                            flags=A.YS_AUG_FLIP_KEEP_SIZE)
    aug.close_mosaic(True)
    items = aug.draw([1, 4])
    items["flip_lr"] = [1, 0]
    db = aug.run(items)
    host = db.to_host()
    assert db.mode == "letterbox" and len(host["cls"]) == 6 < db.capacity
    got = []
    for device in (True, False):
        m = cls_(engine, nc=5, size="n", height=s, width=s, max_batch=2, dtype="f32", **(dict(kpt_num=kpt, kpt_dim=3) if kpt else {}))
        m.init_weights(1)
        amp = M.AMPWrapper(m)
        _, it = amp.TrainStepDevice(db, crit_(m)) if device else amp.TrainStep(host["images"], host, crit_(m))
        got.append(it)
        m.close()
    aug.close()
    assert np.all(np.isfinite(got[0])) and got[0][0] > 0
    assert np.array_equal(got[0], got[1]), got


# ---------------------------------------------------------------------------------------------------- trainer
@pytest.mark.parametrize("backend", BACKENDS)
def test_trainer_closes_the_mosaic(backend, engine):
    from yolosharp_amd import augment as A
    from yolosharp_amd import model as M
    from yolosharp_amd import trainer as T
    s = 32
    _, imgs, _, labels = _tiny_dataset(5)
    aug = A.MosaicAugmenter(engine, imgs, labels, s, degrees=5.0, seed=9, max_batch=2)
    m = M.Yolov8(engine, nc=5, size="n", height=s, width=s, max_batch=2, dtype="f32")
    m.init_weights(1)
    modes = []

    def train_batches():
        epoch = []
        modes.append(epoch)
        for idx in ([0, 1], [2, 3]):
            db = aug.batch(idx)
            epoch.append(db.mode)
            yield db
    tr = T.Trainer(m, epochs=2, nb=2, lr0=2e-3, warmup_bias_lr=2e-3)
    hist = tr.fit(train_batches, augmenter=aug, close_mosaic=1)
    assert modes == [["mosaic", "mosaic"], ["letterbox", "letterbox"]]
    assert len(hist) == 2 and all(np.all(np.isfinite(h["train_loss"])) and h["train_loss"][1] > 0 for h in hist)
    del modes[:]
    hist = tr.fit(train_batches, augmenter=aug)                      # Config.CloseMosaic's default 0: closed from epoch 1 on
    assert modes == [["letterbox"] * 2] * 2 and all(np.all(np.isfinite(h["train_loss"])) for h in hist)
    # without an augmenter fit runs as before: it does not touch the augmenter's state
    aug.close_mosaic(False)
    del modes[:]
    hist = T.Trainer(m, epochs=1, nb=2, lr0=2e-3, warmup_bias_lr=2e-3).fit(train_batches)
    assert modes == [["mosaic"] * 2] and aug.mode == "mosaic" and np.all(np.isfinite(hist[0]["train_loss"]))
    m.close(); aug.close()


# ---------------------------------------------------------------------------------------------------- the workload's row length
@pytest.mark.gpu
def test_large_letterbox():
    """s = 640, B = 4: the vector path at the workload's row length with odd arena offsets, masks, both flips and 50 labels per source."""
    from yolosharp_amd import Engine
    from yolosharp_amd import augment as A
    s = 640
    shapes = [(640, 480), (427, 640), (639, 480), (1, 1)]
    imgs, masks = _sources(shapes, seed=5)
    labels = _raw_labels(shapes, seed=7, per_source=50)
    arena, srcs = _pack_odd(imgs, masks)
    lab_off, cls, boxes, kp = A.pack_labels(labels)
    lst = [(0, 1, 1), (1, 1, 1), (2, 1, 1), (3, 1, 1)]
    eng = Engine()
    images, mks = A.augment_letterbox(eng, arena, srcs, _pack_items(lst), s, RATIO, with_masks=True)
    _assert_images(images, mks, _ref_images(imgs, masks, lst, s, RATIO))
    out = A.augment_letterbox_labels(eng, srcs, lab_off, cls, boxes, kp, _pack_items(lst), s, 0, 256)
    _assert_labels(out, _ref_labels(labels, shapes, lst, s, torch.float64, False), 256)
