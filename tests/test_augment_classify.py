"""The classification input on the device (csrc/augment_cls.hip: ys_augment_classify; yolosharp_amd/augment.py ClassifyAugmenter, draw_classify_items,
draw_classify_val_items; AMPWrapper.TrainStepDevice, Trainer.fit and Classifier.Val on a ClassifyDeviceBatch) against tests/cls_input_ref.py, the torch
restatement of Data/ClassificationDataset.cs:90-131 with Auto_Augment = None.

Nothing is blended in the gather, the noise is an integer function and the jitter is the bit-exact fp32 arithmetic of ys_color_jitter: images and class
ids are judged BIT FOR BIT (np.array_equal on the fp32 arrays), no pixel exempted, no tolerance.  The shapes are the smallest that can go wrong: s = 8
(16-byte stores) and s = 7 (scalar stores), sources 5x9, 13x7 and 37x23 at unaligned arena offsets, one s = 32 batch with more than one workgroup row."""
import functools
import math

import numpy as np
import pytest
import torch

import cls_input_ref as R
from conftest import BACKENDS

SHAPES = [(5, 9), (13, 7), (37, 23)]
CLASSES = [3.0, 0.0, 4.0]
FLIPS = [(0, 0), (1, 0), (0, 1), (1, 1)]
SEED = 0x1234abcd                       # the erase seed of the parity cases and of the distribution check (chosen on the CPU: see that test)
Q114 = np.float32(114.0) * np.float32(1 / 255.0)


# ---------------------------------------------------------------------------------------------------- data
@functools.lru_cache(maxsize=None)
def _sources():
    """uint8 RGB planes = seeded noise over a ramp; the arena behind one leading byte so that the sources sit at offsets 1, 136 and 409."""
    from yolosharp_amd import augment as A
    g = np.random.default_rng(5)
    imgs = []
    for h, w in SHAPES:
        yy, xx = np.mgrid[0:h, 0:w]
        ramp = (xx * 97.0 / max(w - 1, 1) + yy * 89.0 / max(h - 1, 1))[None] + np.array([0.0, 20.0, 40.0])[:, None, None]
        imgs.append(np.clip(ramp + g.integers(0, 70, (3, h, w)), 0, 255).astype(np.uint8))
    arena, srcs = A.pack_sources(imgs)
    srcs["img_off"] += 1
    arena = np.ascontiguousarray(np.concatenate([np.array([201], np.uint8), arena]))
    assert [int(o) % 4 for o in srcs["img_off"]] == [1, 0, 1]
    return imgs, arena, srcs


def _item(src, crop, s, flips=(0, 0), erase=(0, 0, 0, 0), seed=SEED, resized=None, window=(0, 0)):
    """One item: crop = (top, left, ch, cw); resized = (oh, ow), default (s, s)."""
    oh, ow = resized if resized is not None else (s, s)
    return (src,) + tuple(crop) + (oh, ow) + tuple(window) + tuple(flips) + tuple(erase) + (seed if erase != (0, 0, 0, 0) else 0,)


def _crops(k):
    H, W = SHAPES[k]
    return [(0, 0, H, W),                                   # the whole image (37x23: down-sampling; 5x9: both directions)
            (H - 1, W - 1, 1, 1),                           # 1x1 in the last row and column
            (H - 3, W - 2, 3, 2),                           # touches the bottom and the right border; up-sampling
            (1, 0, H - 1, max(W // 2, 1)),                  # touches the bottom border only
            (0, 1, max(H // 2, 1), W - 1)]                  # touches the right border only


def _erases(s):
    return [(0, 0, 0, 0),
            (0, 0, 1, 1), (0, s - 1, 1, 1), (s - 1, 0, 1, 1), (s - 1, s - 1, 1, 1),          # 1x1 at each corner
            (0, 0, s - 1, s - 1), (1, 1, s - 1, s - 1),                                       # (s - 1) x (s - 1)
            (1, 2, 2, 4)]                                                                     # columns 2 .. 5: over the boundary between two quads


def _rows(n):
    """Jitter rows cycling through: no contrast; contrast in slot 0, 1, 2, 3."""
    from yolosharp_amd import augment as A
    kinds = [((0, 2, 3, -1), (1.2, 1.0, 0.7, 0.01)), ((1, 0, 2, 3), (0.8, 1.3, 1.4, -0.012)), ((0, 1, 3, 2), (1.1, 0.6, 0.5, 0.015)),
             ((3, 2, 1, 0), (0.7, 1.4, 1.2, -0.5)), ((2, -1, 3, 1), (1.0, 0.9, 1.6, 0.5))]
    rows = A.make_jitter(n)
    for b in range(n):
        rows[b]["order"], rows[b]["factor"] = kinds[b % len(kinds)]
    return rows


@functools.lru_cache(maxsize=None)
def _case(s):
    """The items of the parity test at size s -- every crop of every source, the four flips and every erase rectangle cycling against each other so that
    each erase rectangle meets each flip -- their rows, and the restatement's batches without and with jitter, computed once and never modified."""
    from yolosharp_amd import augment as A
    imgs, _, _ = _sources()
    lst, n = [], 0
    for k in range(len(SHAPES)):
        for crop in _crops(k):
            for j in range(4):
                lst.append(_item(k, crop, s, FLIPS[(n + j) % 4], _erases(s)[(n + 2 * j) % 8]))
            n += 1
    for flips in FLIPS:                                     # each erase rectangle under each flip (it must not move with the flip)
        for er in _erases(s)[1:]:
            lst.append(_item(2, (4, 3, 20, 11), s, flips, er))
    items = A.make_classify_items(len(lst))
    for b, t in enumerate(lst):
        items[b] = t
    val = A.draw_classify_val_items([0, 1, 2], SHAPES, s)   # a wide, a tall and a large source through Resize + CenterCrop
    items = np.concatenate([items, val])
    rows = _rows(items.shape[0])
    return items, rows, R.batch(imgs, CLASSES, items, s), R.batch(imgs, CLASSES, items, s, rows)


def _chunks(n, size=60):
    return [slice(i, min(i + size, n)) for i in range(0, n, size)]


def _run_device(engine, arena, srcs, classes, items, s, rows=None):
    """ys_augment_classify on DEVICE pointers, without the Python check in front of it: -> (images, cls)."""
    from yolosharp_amd import _lib
    from yolosharp_amd import augment as A
    B = items.shape[0]
    bufs = [engine.to_device(np.ascontiguousarray(a)) for a in (arena, srcs, np.asarray(classes, np.float32), items)]
    d_rows = engine.to_device(np.ascontiguousarray(rows, A.JITTER_DTYPE)) if rows is not None else None
    d_img, d_cls = engine.malloc(B * 3 * s * s * 4), engine.malloc(B * 4)
    try:
        _lib.check(engine.lib, engine.lib.ys_augment_classify(engine.ctx, bufs[0], bufs[1], srcs.shape[0], bufs[2], bufs[3], B, 1, s, d_rows, d_img, d_cls))
        return engine.from_device(d_img, (B, 3, s, s), np.float32), engine.from_device(d_cls, (B,), np.float32)
    finally:
        for p in bufs + [d_rows, d_img, d_cls]:
            if p is not None:
                engine.free(p)


# ---------------------------------------------------------------------------------------------------- the restatement's own checks (CPU)
def test_index_formula_equals_interpolate():
    """crop -> interpolate(nearest, uint8) -> slice equals the one-line index formula, on odd sizes in both directions."""
    g = torch.Generator().manual_seed(1)
    for (H, W), (oh, ow) in (((7, 5), (4, 9)), ((5, 9), (14, 8)), ((37, 23), (8, 13)), ((1, 6), (3, 3)), ((13, 7), (13, 7))):
        img = torch.randint(0, 256, (3, H, W), generator=g, dtype=torch.uint8)
        for s in (1, 3, min(oh, ow)):
            for oy, ox in ((0, 0), (oh - s, ow - s), ((oh - s) // 2, (ow - s) // 2)):
                it = dict(top=0, left=0, ch=H, cw=W, oh=oh, ow=ow, oy=oy, ox=ox)
                assert torch.equal(R.gather(img, it, s), R.gather_by_formula(img, it, s)), ((H, W), (oh, ow), s, oy, ox)
        it = dict(top=H // 2, left=W // 3, ch=H - H // 2, cw=W - W // 3, oh=oh, ow=ow, oy=0, ox=0)       # a crop that touches both far borders
        s = min(oh, ow)
        assert torch.equal(R.gather(img, it, s), R.gather_by_formula(img, it, s))


def test_threshold_table():
    assert R.THRESHOLDS == R.thresholds_from_erf() and R.THRESHOLDS[-1] == 2 ** 32 and len(R.THRESHOLDS) == len(R.VALUES) == 13
    assert list(R.THRESHOLDS) == sorted(set(R.THRESHOLDS))


def test_noise_byte_is_atens_cast():
    """The byte of the word at cumulative probability Phi(z) equals z.to(int64).to(uint8), for z on both sides of every integer in [-6, 6] (0.25 away:
    at |z| = 6 a word is 0.9 of the whole tail, nothing finer exists there; 1e-3 away up to |z| = 4) and at ATen's four documented casts."""
    phi = lambda z: 0.5 * math.erfc(-z / math.sqrt(2.0))
    zs = [k + d for k in range(-6, 7) for d in (-0.25, 0.25)] + [k + d for k in range(-4, 5) for d in (-1e-3, 1e-3)] + [-1.3, -2.7, 0.7, 1.9]
    for z in zs:
        word = min(int(math.floor(2.0 ** 32 * phi(z))), 2 ** 32 - 1)
        want = int(torch.tensor([z], dtype=torch.float32).to(torch.int64).to(torch.uint8)[0])
        assert int(R.byte_of_word([word])[0]) == want == R.value_of_z(z) % 256, (z, word)
    assert [int(torch.tensor([z]).to(torch.int64).to(torch.uint8)[0]) for z in (-1.3, -2.7, 0.7, 1.9)] == [255, 254, 0, 1]


def test_noise_distribution():
    """65536 consecutive counters of SEED (channel 0): the bins 0, +-1, +-2 within 5 standard deviations of their expected counts."""
    n = 65536
    k = R.value_of_word(R.noise_word(SEED, 0, np.arange(n)))
    phi = lambda x: 0.5 * (1.0 + math.erf(x / math.sqrt(2.0)))
    p = {0: phi(1) - phi(-1), 1: phi(2) - phi(1), -1: phi(-1) - phi(-2), 2: phi(3) - phi(2), -2: phi(-2) - phi(-3)}
    for v, pv in p.items():
        got, sigma = int((k == v).sum()), math.sqrt(n * pv * (1 - pv))
        print("value %2d: %d, expected %.1f, sigma %.1f" % (v, got, n * pv, sigma))
        assert abs(got - n * pv) <= 5 * sigma, (v, got, n * pv, sigma)
    assert k.min() >= -6 and k.max() <= 6


# ---------------------------------------------------------------------------------------------------- kernel parity
@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("s", [8, 7])
def test_parity_host_pointers(backend, engine, s):
    """s = 8: 16-byte stores; s = 7: scalar stores.  jitter = NULL, then rows without contrast and with contrast in each of the four slots."""
    from yolosharp_amd import augment as A
    _, arena, srcs = _sources()
    items, rows, plain, jittered = _case(s)
    assert items.shape[0] >= 90
    for sl in _chunks(items.shape[0]):
        img, cls = A.augment_classify(engine, arena, srcs, CLASSES, items[sl], s)
        assert img.dtype == np.float32 and np.array_equal(img, plain[0][sl]) and np.array_equal(cls, plain[1][sl])
        img, cls = A.augment_classify(engine, arena, srcs, CLASSES, items[sl], s, jitter=rows[sl])
        assert np.array_equal(img, jittered[0][sl]) and np.array_equal(cls, jittered[1][sl])
    assert not np.array_equal(plain[0], jittered[0])


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("s", [8, 7])
def test_parity_device_pointers_and_determinism(backend, engine, s):
    """The device-pointer form (the reduction always runs) gives the same bytes; the same call twice gives identical bytes (the sums are re-zeroed)."""
    _, arena, srcs = _sources()
    items, rows, plain, jittered = _case(s)
    sl = slice(0, 60)
    a = _run_device(engine, arena, srcs, CLASSES, items[sl], s, rows[sl])
    b = _run_device(engine, arena, srcs, CLASSES, items[sl], s, rows[sl])
    assert np.array_equal(a[0], jittered[0][sl]) and np.array_equal(a[1], jittered[1][sl])
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    c = _run_device(engine, arena, srcs, CLASSES, items[sl], s, None)
    assert np.array_equal(c[0], plain[0][sl]) and np.array_equal(c[1], plain[1][sl])


@functools.lru_cache(maxsize=None)
def _mixed32():
    """s = 32, B = 3: a down-sampled crop under both flips with a quad-straddling erase and contrast first; an up-sampled 1-row crop, flipped left-right,
    erased to (s - 1)^2, contrast last; a val item of the tall source without erase, no contrast."""
    from yolosharp_amd import augment as A
    imgs, _, _ = _sources()
    s = 32
    items = A.make_classify_items(3)
    items[0] = _item(2, (5, 2, 32, 21), s, (1, 1), (3, 6, 9, 13))
    items[1] = _item(0, (4, 1, 1, 8), s, (1, 0), (1, 0, s - 1, s - 1), seed=77)
    items[2] = A.draw_classify_val_items([1], SHAPES, s)[0]
    rows = _rows(5)[[1, 4, 0]]
    return items, rows, R.batch(imgs, CLASSES, items, s), R.batch(imgs, CLASSES, items, s, rows)


@pytest.mark.parametrize("backend", BACKENDS)
def test_parity_mixed_batch_32(backend, engine):
    from yolosharp_amd import augment as A
    _, arena, srcs = _sources()
    items, rows, plain, jittered = _mixed32()
    for got, want in ((A.augment_classify(engine, arena, srcs, CLASSES, items, 32), plain),
                      (A.augment_classify(engine, arena, srcs, CLASSES, items, 32, jitter=rows), jittered),
                      (_run_device(engine, arena, srcs, CLASSES, items, 32, rows), jittered)):
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


# ---------------------------------------------------------------------------------------------------- invalid items and rows
S_BAD = 8
# one violated rule each, on a valid item of source 2 (37 x 23): crop (4, 3, 20, 11), resized 12 x 10, window (2, 1), erase (1, 2, 3, 4)
BAD = {"src_negative": dict(src=-1), "src_past_table": dict(src=3), "ch_zero": dict(ch=0), "cw_zero": dict(cw=0), "top_negative": dict(top=-1),
       "left_negative": dict(left=-1), "crop_past_bottom": dict(top=18), "crop_past_right": dict(left=13), "oh_zero": dict(oh=0, oy=0), "ow_zero": dict(ow=0, ox=0),
       "oy_negative": dict(oy=-1), "ox_negative": dict(ox=-1), "window_past_bottom": dict(oy=5), "window_past_right": dict(ox=3), "flip_lr_2": dict(flip_lr=2),
       "flip_ud_negative": dict(flip_ud=-1), "erase_h_zero": dict(er_h=0), "erase_w_zero": dict(er_w=0), "erase_y_negative": dict(er_y=-1),
       "erase_x_negative": dict(er_x=-1), "erase_past_bottom": dict(er_y=6), "erase_past_right": dict(er_x=5), "jitter_row": None}


@functools.lru_cache(maxsize=None)
def _bad_base():
    from yolosharp_amd import augment as A
    imgs, _, _ = _sources()
    items = A.make_classify_items(3)
    items[0] = _item(0, (0, 0, 5, 9), S_BAD, (1, 0), (0, 0, 2, 2))
    items[1] = _item(2, (4, 3, 20, 11), S_BAD, (0, 1), (1, 2, 3, 4), resized=(12, 10), window=(2, 1))
    items[2] = _item(1, (2, 1, 9, 5), S_BAD, (1, 1))
    rows = _rows(3)
    return items, rows, R.batch(imgs, CLASSES, items, S_BAD, rows)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("rule", sorted(BAD))
def test_invalid_item_or_row(backend, engine, rule):
    """Host pointers: YS_ERR_INVALID_ARG naming the row.  Device pointers: that image is all 114 * (1 / 255), class -1; its neighbours are unaffected."""
    from yolosharp_amd import YsError
    from yolosharp_amd import augment as A
    _, arena, srcs = _sources()
    base, base_rows, want = _bad_base()
    items, rows = base.copy(), base_rows.copy()
    if BAD[rule] is None:
        rows[1]["order"] = (1, 1, -1, -1)                  # an op id twice
    else:
        for k, v in BAD[rule].items():
            items[1][k] = v
    with pytest.raises(YsError) as ei:
        A.augment_classify(engine, arena, srcs, CLASSES, items, S_BAD, jitter=rows)
    assert ei.value.status == 1 and ("row 1" if BAD[rule] is None else "item 1") in str(ei.value), str(ei.value)
    if BAD[rule] is not None:
        with pytest.raises(ValueError):
            A.check_classify_items(items, srcs, S_BAD)
    img, cls = _run_device(engine, arena, srcs, CLASSES, items, S_BAD, rows)
    assert np.array_equal(img[1], np.full((3, S_BAD, S_BAD), Q114, np.float32)) and cls[1] == -1.0
    for b in (0, 2):
        assert np.array_equal(img[b], want[0][b]) and cls[b] == want[1][b]


# ---------------------------------------------------------------------------------------------------- draw functions (CPU)
DRAW_SHAPES = [(1, 17), (23, 1), (5, 9), (37, 23), (10, 1000), (1000, 10), (224, 224), (3, 3)]


def test_drawn_items_are_valid():
    """2000 draws over shapes with 1-pixel sides and extreme aspect ratios: every item passes the validity rules; the 10 x 1000 source reaches the
    fallback (its crop is the centred 10 x 13 = round(10 * 4 / 3) window) in a fixed share of its draws."""
    from yolosharp_amd import augment as A
    srcs = np.zeros(len(DRAW_SHAPES), A.SRC_DTYPE)
    srcs["h"], srcs["w"] = [h for h, _ in DRAW_SHAPES], [w for _, w in DRAW_SHAPES]
    rng = np.random.default_rng(7)
    fallback = 0
    for s in (7, 8, 32, 224):
        idx = np.arange(500) % len(DRAW_SHAPES)
        items, rows = A.draw_classify_items(rng, idx, DRAW_SHAPES, s, flipud=0.3)
        assert items.shape == rows.shape == (500,)
        A.check_classify_items(items, srcs, s)
        A.check_jitter(rows, allow_contrast=True)
        assert all(1 in r["order"] for r in rows)                      # contrast = vgain: always present
        assert np.all(items["oh"] == s) and np.all(items["ow"] == s) and not items["oy"].any() and not items["ox"].any()
        wide = items[items["src"] == 4]
        fb = (wide["ch"] == 10) & (wide["cw"] == 13) & (wide["top"] == 0) & (wide["left"] == (1000 - 13) // 2)
        fallback += int(fb.sum())
        A.check_classify_items(A.draw_classify_val_items(np.arange(len(DRAW_SHAPES)), DRAW_SHAPES, s), srcs, s)
    assert fallback > 0


def test_val_items():
    from yolosharp_amd import augment as A
    it = A.draw_classify_val_items([0, 1, 2], [(5, 9), (13, 7), (224, 224)], 8)
    assert [tuple(int(it[b][k]) for k in ("src", "top", "left", "ch", "cw", "oh", "ow", "oy", "ox")) for b in range(3)] == \
        [(0, 0, 0, 5, 9, 8, 14, 0, 3), (1, 0, 0, 13, 7, 14, 8, 3, 0), (2, 0, 0, 224, 224, 8, 8, 0, 0)]
    assert not any(it[k].any() for k in ("flip_lr", "flip_ud", "er_y", "er_x", "er_h", "er_w", "er_seed"))
    it = A.draw_classify_val_items([0], [(5, 8)], 7)                   # oh - s = 0, ow - s = int(7 * 8 / 5) - 7 = 4; Python's round
    assert (int(it[0]["ow"]), int(it[0]["ox"])) == (11, 2)


def test_erase_rate():
    """p = 0.4 at s = 224, fixed seed.  Normal gate (`randn > 0.4` skips, the reference's): the share of ERASED images within 5 sigma of
    P(z <= 0.4) = 0.655.  Uniform gate (`rand > 0.4` skips): the share of SKIPPED images within 5 sigma of 0.6, i.e. 0.4 are erased.  (Ten failed tries
    also leave an image alone: at s = 224 a try fails with probability < 0.1, ten in a row never happen in 4000 draws.)"""
    from yolosharp_amd import augment as A
    n = 4000
    p_normal = 0.5 * (1.0 + math.erf(0.4 / math.sqrt(2.0)))
    assert abs(p_normal - 0.655) < 5e-4
    for gate, p_erase in (("normal", p_normal), ("uniform", 1.0 - 0.6)):
        items, _ = A.draw_classify_items(np.random.default_rng(11), np.zeros(n, np.int64), [(224, 224)], 224, erasing=0.4, erasing_gate=gate)
        rate = float((items["er_h"] > 0).mean())
        sigma = math.sqrt(p_erase * (1 - p_erase) / n)
        print("%s gate: erased %.4f (skipped %.4f), expected %.4f, sigma %.4f" % (gate, rate, 1 - rate, p_erase, sigma))
        assert abs(rate - p_erase) <= 5 * sigma, (gate, rate, p_erase)
        erased = items[items["er_h"] > 0]
        assert np.all(erased["er_h"] < 224) and np.all(erased["er_w"] < 224) and len(set(erased["er_seed"].tolist())) > 0.99 * len(erased)


class _CountingRng:
    """A numpy Generator that counts what is drawn from it."""

    def __init__(self, seed):
        self.g, self.calls = np.random.default_rng(seed), []

    def __getattr__(self, name):
        fn = getattr(self.g, name)

        def wrapped(*a, **k):
            self.calls.append(name)
            return fn(*a, **k)
        return wrapped


def test_switched_off_transforms_draw_nothing():
    from yolosharp_amd import augment as A
    # a source whose whole area at scale (1, 1), ratio (1, 1) is accepted at the first try: 2 uniforms + top + left
    base = dict(scale=(1.0, 1.0), ratio=(1.0, 1.0))
    rng = _CountingRng(1)
    items, rows = A.draw_classify_items(rng, [0, 0, 0], [(16, 16)], 8, fliplr=0, flipud=0, erasing=0, hsv=None, **base)
    assert rows is None and rng.calls == ["random", "random", "integers", "integers"] * 3
    assert not any(items[k].any() for k in ("flip_lr", "flip_ud", "er_h", "er_w", "er_seed"))
    assert [tuple(int(items[b][k]) for k in ("top", "left", "ch", "cw")) for b in range(3)] == [(0, 0, 16, 16)] * 3
    rng = _CountingRng(1)
    A.draw_classify_items(rng, [0], [(16, 16)], 8, fliplr=0.5, flipud=0, erasing=0, hsv=None, **base)
    assert rng.calls == ["random", "random", "integers", "integers", "random"]                        # + the one flip draw
    rng = _CountingRng(1)
    _, rows = A.draw_classify_items(rng, [0], [(16, 16)], 8, fliplr=0, flipud=0, erasing=0, hsv=(0.015, 0.7, 0.4), **base)
    assert rng.calls == ["random", "random", "integers", "integers", "permutation"] + ["random"] * 4 and sorted(rows[0]["order"].tolist()) == [0, 1, 2, 3]
    rng = _CountingRng(1)
    A.draw_classify_items(rng, [0], [(16, 16)], 8, fliplr=0, flipud=0, erasing=0.4, hsv=None, **base)
    assert rng.calls[4] == "standard_normal"                                                          # the reference's gate is a normal draw


def test_auto_augment_is_refused():
    from yolosharp_amd import augment as A
    with pytest.raises(NotImplementedError):
        A.ClassifyAugmenter(None, [np.zeros((3, 4, 4), np.uint8)], [0], 8, auto_augment="AutoAugment")


# ---------------------------------------------------------------------------------------------------- end to end
def _dataset(n, seed=2):
    g = np.random.default_rng(seed)
    shapes = [(24 + 5 * (i % 4), 40 - 3 * (i % 5)) for i in range(n)]
    return [g.integers(0, 256, (3, h, w)).astype(np.uint8) for h, w in shapes], [float(i % 5) for i in range(n)]


@pytest.mark.parametrize("backend", BACKENDS)
def test_augmenter_batches(backend, engine):
    """ClassifyAugmenter's device batch is the restatement of its own drawn items, train and val."""
    from yolosharp_amd import augment as A
    imgs, classes = _dataset(6)
    s = 16
    aug = A.ClassifyAugmenter(engine, imgs, classes, s, seed=4, max_batch=4, flipud=0.5)
    items, rows = aug.draw([5, 0, 3])
    db = aug.run(items, rows)
    host = db.to_host()
    want = R.batch(imgs, classes, items, s, rows)
    assert (db.mode, db.batch, db.imgsz) == ("train", 3, s) and sorted(host) == ["batch_idx", "cls", "images"]
    assert np.array_equal(host["images"], want[0]) and np.array_equal(host["cls"], want[1]) and host["batch_idx"].tolist() == [0, 1, 2]
    sizes = []
    for k, vb in enumerate(aug.val_batches(4)):
        h = vb.to_host()
        idx = np.arange(4 * k, min(4 * k + 4, 6))
        want = R.batch(imgs, classes, A.draw_classify_val_items(idx, aug.shapes, s), s)
        assert vb.mode == "val" and np.array_equal(h["images"], want[0]) and np.array_equal(h["cls"], want[1])
        sizes.append(vb.batch)
    assert sizes == [4, 2]
    assert [b.batch for b in aug.batches(4)] == [4] and [b.batch for b in aug.batches(4, drop_last=False)] == [4, 2]
    with pytest.raises(ValueError):
        bad = items.copy()
        bad[1]["ch"] = 1000
        aug.run(bad, rows)
    aug.close()


@pytest.mark.parametrize("backend", BACKENDS)
def test_train_step_on_classify_batch(backend, engine):
    """Yolov8n-cls, 32 px, B = 4, nc = 5, fp32: TrainStepDevice on a ClassifyDeviceBatch returns the same loss item, bit for bit, as TrainStep on its
    to_host(); mismatched pairs of batch kind and model task are refused."""
    from yolosharp_amd import augment as A
    from yolosharp_amd import model as M
    s, B = 32, 4
    imgs, classes = _dataset(6)
    aug = A.ClassifyAugmenter(engine, imgs, classes, s, seed=3, max_batch=B)
    db = aug.batch([1, 4, 2, 5])
    host = db.to_host()
    assert host["cls"].tolist() == [1.0, 4.0, 2.0, 0.0]
    got = []
    for device in (True, False):
        m = M.Yolov8Classify(engine, nc=5, size="n", height=s, width=s, max_batch=B, dtype="f32")
        m.init_weights(1)
        amp, crit = M.AMPWrapper(m), M.v8ClassificationLoss(m)
        _, it = amp.TrainStepDevice(db, crit) if device else amp.TrainStep(host["images"], host, crit)
        got.append(it)
        m.close()
    assert got[0].shape == (1,) and np.isfinite(got[0][0]) and got[0][0] > 0
    assert np.array_equal(got[0], got[1]), got
    # a detect model given a classify batch, and a classify model given a DeviceBatch
    d = M.Yolov8(engine, nc=5, size="n", height=s, width=s, max_batch=B, dtype="f32")
    with pytest.raises(ValueError):
        M.AMPWrapper(d).TrainStepDevice(db, M.v8DetectionLoss(d))
    d.close()
    labels = [dict(cls=np.zeros(1, np.float32), bboxes=np.array([[2.0, 2.0, 20.0, 20.0]], np.float32)) for _ in imgs]
    maug = A.MosaicAugmenter(engine, imgs, labels, s, seed=1, max_batch=B)
    mdb = maug.batch([0, 1, 2, 3])
    c = M.Yolov8Classify(engine, nc=5, size="n", height=s, width=s, max_batch=B, dtype="f32")
    with pytest.raises(ValueError):
        M.AMPWrapper(c).TrainStepDevice(mdb, M.v8ClassificationLoss(c))
    c.close(); maug.close(); aug.close()


@pytest.mark.parametrize("backend", BACKENDS)
def test_trainer_and_validator_on_device_batches(backend, engine):
    """Two epochs of Trainer.fit(..., augmenter=aug) on device batches with device validation; Classifier.Val on val_batches returns the same top-1 /
    top-5 (and loss) as on the host copies of the same batches."""
    from yolosharp_amd import augment as A
    from yolosharp_amd import model as M
    from yolosharp_amd import trainer as T
    from yolosharp_amd.detector import Classifier
    s, B = 32, 4
    imgs, classes = _dataset(10)
    aug = A.ClassifyAugmenter(engine, imgs, classes, s, seed=8, max_batch=B)
    m = M.Yolov8Classify(engine, nc=5, size="n", height=s, width=s, max_batch=B, dtype="f32")
    m.init_weights(1)
    tr = T.Trainer(m, epochs=2, nb=2, lr0=2e-3, warmup_bias_lr=2e-3)
    hist = tr.fit(lambda: aug.batches(B), lambda: aug.val_batches(B), augmenter=aug)
    assert len(hist) == 2 and tr.steps_run == 2
    for h in hist:
        assert h["train_loss"].shape == (1,) and np.isfinite(h["train_loss"][0]) and h["train_loss"][0] > 0
        assert np.isfinite(h["val_loss"][0]) and 0.0 <= h["metrics"][0] <= h["metrics"][1] <= 1.0
    loss_d, acc_d = Classifier(m).Val(aug.val_batches(B))
    hosts = [vb.to_host() for vb in aug.val_batches(B)]
    assert [h["images"].shape[0] for h in hosts] == [4, 4, 2]
    loss_h, acc_h = Classifier(m).Val(hosts)
    assert acc_d == acc_h and np.array_equal(loss_d, loss_h)
    m.close(); aug.close()
