"""AutoAugment / RandAugment on the device classification input (csrc/augment_aa.hip: ys_auto_augment_ops, ys_augment_classify_aa; yolosharp_amd/augment.py
AutoAugment, RandAugment, draw_auto_augment, ClassifyAugmenter(auto_augment=...)) against tests/aa_ref.py, the restatement of torchvision's public tensor /
uint8 operators with torch's own grid_sample, conv2d, bincount / cumsum and the blend of color_jitter_ref.

Everything is judged BIT FOR BIT (np.array_equal / torch.equal), no pixel exempted, no tolerance.  The shapes are the smallest that can go wrong: 5 x 9 and
13 x 7 (non-square, byte stores), 8 x 8 (4-byte loads and stores), 7 x 7, 2 x 6 (no interior for the sharpness stencil), one 64 x 64 constant image (one
histogram bin takes every count; more than one quad per thread of the statistics launch); the classification chain at s = 8, s = 7 and one s = 32 batch.

The one case left out, on the CPU side only: ShearY, magnitude id 6, negated, at 13 x 7.  Its source coordinates sit EXACTLY on rounding ties (aa_ref.tie_distance
== 0, asserted) and the explicit index formula and the bmm + grid_sample pipeline of the torch build the tests run on resolve three of them differently; the other 499
cases, 37 more with exact ties among them, agree in every pixel, which is what is asserted of them.  The kernels are held to the formula in ALL 500."""
import functools
import hashlib

import numpy as np
import pytest
import torch

import aa_ref as AR
import test_augment_classify as TC
from conftest import BACKENDS

OPS_SHAPES = [(5, 9), (13, 7), (8, 8), (7, 7), (2, 6)]
AFFINE = ("ShearX", "ShearY", "TranslateX", "TranslateY", "Rotate")
BLENDS = ("Brightness", "Color", "Contrast", "Sharpness")
PAIRS = (("Rotate", "Equalize"), ("Equalize", "Equalize"), ("Color", "Contrast"), ("Invert", "Equalize"), ("ShearX", "AutoContrast"))
Q114 = TC.Q114
# the ImageNet policy by op id: (op, p, magnitude id) x 2 per row
POLICY_IDS = [((9, .4, 8), (4, .6, 9)), ((10, .6, 5), (11, .6, None)), ((12, .8, None), (12, .6, None)), ((9, .6, 7), (9, .6, 6)), ((12, .4, None), (10, .2, 4)),
              ((12, .4, None), (4, .8, 8)), ((10, .6, 3), (12, .6, None)), ((9, .8, 5), (12, 1., None)), ((4, .2, 3), (10, .6, 8)), ((12, .6, None), (9, .4, 6)),
              ((4, .8, 8), (6, .4, 0)), ((4, .4, 9), (12, .6, None)), ((12, .0, None), (12, .8, None)), ((13, .6, None), (12, 1., None)), ((6, .6, 4), (7, 1., 8)),
              ((4, .8, 8), (6, 1., 2)), ((6, .8, 8), (10, .8, 7)), ((8, .4, 7), (13, .6, None)), ((0, .6, 5), (12, 1., None)), ((6, .4, 0), (12, .6, None)),
              ((12, .4, None), (10, .2, 4)), ((10, .6, 5), (11, .6, None)), ((13, .6, None), (12, 1., None)), ((6, .6, 4), (7, 1., 8)), ((12, .8, None), (12, .6, None))]


# ---------------------------------------------------------------------------------------------------- data
def _image(h, w, seed):
    """uint8 [3, h, w]: seeded noise over a ramp, like the sources of test_augment_classify."""
    g = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    ramp = (xx * 97.0 / max(w - 1, 1) + yy * 89.0 / max(h - 1, 1))[None] + np.array([0.0, 20.0, 40.0])[:, None, None]
    return np.clip(ramp + g.integers(0, 70, (3, h, w)), 0, 255).astype(np.uint8)


def _slot(row, k, op, mid, sign, hw, bins=10):
    """Slot k = op at magnitude id `mid` (None: no magnitude) of `bins`, negated for sign < 0."""
    from yolosharp_amd import augment as A
    m = A.aa_magnitudes(op, bins, *hw)[mid] if mid is not None else 0.0
    A.set_aa_slot(row, k, op, -m if sign < 0 and op in A.AA_SIGNED else m, hw)


def _single_rows(hw):
    """Every op alone at every magnitude id and sign: even rows in slot 0, odd rows in slot 1."""
    from yolosharp_amd import augment as A
    cases = [(op, mid, sg) for op in AFFINE + BLENDS for mid in range(10) for sg in (1, -1)]
    cases += [(op, mid, 1) for op in ("Posterize", "Solarize") for mid in range(10)] + [(op, None, 1) for op in ("AutoContrast", "Equalize", "Invert")]
    rows = A.make_aa_rows(len(cases))
    for b, (op, mid, sg) in enumerate(cases):
        _slot(rows[b], b % 2, op, mid, sg, hw)
    assert len(cases) == 203 and sorted(set(rows["op"].reshape(-1).tolist())) == list(range(-1, 14))
    return rows


def _policy_rows(hw):
    """All 25 policy rows with both slots forced on, under both sign bits, then the pairs whose second statistics depend on the first op."""
    from yolosharp_amd import augment as A
    lst = [(row, sg) for row in A.IMAGENET_POLICY for sg in (1, -1)] + [(((a, 1.0, 5), (b, 1.0, 7)), sg) for a, b in PAIRS for sg in (1, -1)]
    rows = A.make_aa_rows(len(lst))
    for b, (row, sg) in enumerate(lst):
        for k, (op, _, mid) in enumerate(row):
            _slot(rows[b], k, op, mid if A.aa_magnitudes(op, 10, *hw) is not None else None, sg, hw)
    assert (rows["op"] >= 0).all()
    return rows


@functools.lru_cache(maxsize=None)
def _ops_case(hw):
    """(images, rows, the restatement's output) of one shape, computed once."""
    rows = np.concatenate([_single_rows(hw), _policy_rows(hw)])
    base = [_image(hw[0], hw[1], 20 + k) for k in range(3)]
    images = np.stack([base[b % 3] for b in range(rows.shape[0])])
    return images, rows, AR.ops_batch(images, rows)


def _run_ops_device(engine, images, rows):
    """ys_auto_augment_ops on DEVICE pointers, without the Python check in front of it."""
    from yolosharp_amd import _lib
    from yolosharp_amd import augment as A
    B, _, H, W = images.shape
    d_in, d_rows = engine.to_device(np.ascontiguousarray(images)), engine.to_device(np.ascontiguousarray(rows, A.AA_ROW_DTYPE))
    d_out = engine.malloc(images.nbytes)
    try:
        _lib.check(engine.lib, engine.lib.ys_auto_augment_ops(engine.ctx, d_in, B, H, W, d_rows, 1, d_out))
        return engine.from_device(d_out, images.shape, np.uint8)
    finally:
        for p in (d_in, d_rows, d_out):
            engine.free(p)


def _run_classify_device(engine, arena, srcs, classes, items, s, rows, aa):
    """ys_augment_classify_aa on DEVICE pointers (aa / rows None = NULL): -> (images, cls)."""
    from yolosharp_amd import _lib
    from yolosharp_amd import augment as A
    B = items.shape[0]
    bufs = [engine.to_device(np.ascontiguousarray(a)) for a in (arena, srcs, np.asarray(classes, np.float32), items)]
    d_rows = engine.to_device(np.ascontiguousarray(rows, A.JITTER_DTYPE)) if rows is not None else None
    d_aa = engine.to_device(np.ascontiguousarray(aa, A.AA_ROW_DTYPE)) if aa is not None else None
    d_img, d_cls = engine.malloc(B * 3 * s * s * 4), engine.malloc(B * 4)
    try:
        _lib.check(engine.lib, engine.lib.ys_augment_classify_aa(engine.ctx, bufs[0], bufs[1], srcs.shape[0], bufs[2], bufs[3], B, 1, s, d_aa, d_rows, d_img, d_cls))
        return engine.from_device(d_img, (B, 3, s, s), np.float32), engine.from_device(d_cls, (B,), np.float32)
    finally:
        for p in bufs + [d_rows, d_aa, d_img, d_cls]:
            if p is not None:
                engine.free(p)


# ---------------------------------------------------------------------------------------------------- the restatement against independent yardsticks (CPU)
TIE_DROPPED = ((13, 7), "ShearY", 6, -1)


def test_index_formula_equals_grid_sample():
    """The explicit index formula equals linspace base grid -> bmm with the rescaled theta -> grid_sample(nearest, zeros, align_corners = False) for all five
    affine ops, ten magnitude ids, both signs at 7 x 7, 8 x 8, 32 x 32, 5 x 9 and 13 x 7: every pixel of 499 cases; TIE_DROPPED is an exact tie (module docstring)."""
    from yolosharp_amd import augment as A
    g = torch.Generator().manual_seed(3)
    n = ties = 0
    for hw in ((7, 7), (8, 8), (32, 32), (5, 9), (13, 7)):
        img = torch.randint(0, 256, (3,) + hw, generator=g, dtype=torch.uint8)
        for op in AFFINE:
            for mid in range(10):
                for sg in (1, -1):
                    row = A.make_aa_rows(1)[0]
                    _slot(row, 0, op, mid, sg, hw)
                    if (hw, op, mid, sg) == TIE_DROPPED:
                        assert AR.tie_distance(row["theta"][0], *hw) == 0.0
                        continue
                    assert torch.equal(AR.affine_by_formula(img, row["theta"][0]), AR.affine_grid_sample(img, row["theta"][0])), (hw, op, mid, sg)
                    n += 1
                    ties += AR.tie_distance(row["theta"][0], *hw) == 0.0
    print("%d cases equal, %d of them with a source coordinate exactly on a tie" % (n, ties))
    assert n == 499 and ties >= 20


def test_integer_ops_equal_pillow():
    """Equalize, Posterize, Invert and Solarize (integer thresholds) equal PIL.ImageOps on the same bytes; so do a constant and a two-valued channel."""
    pytest.importorskip("PIL")
    from PIL import Image, ImageOps
    imgs = [_image(h, w, 30 + k) for k, (h, w) in enumerate(OPS_SHAPES + [(37, 23)])]
    flat = _image(8, 8, 40)
    flat[0], flat[1] = 77, np.where(np.arange(64).reshape(8, 8) % 3 == 0, 10, 200)
    for a in imgs + [flat]:
        pil, t = Image.fromarray(np.ascontiguousarray(a.transpose(1, 2, 0))), torch.from_numpy(a)
        back = lambda im: torch.from_numpy(np.asarray(im).transpose(2, 0, 1).copy())
        assert torch.equal(AR.equalize(t), back(ImageOps.equalize(pil))), a.shape
        assert torch.equal(AR.invert(t), back(ImageOps.invert(pil)))
        for bits in range(1, 9):                            # Pillow refuses bits = 0
            assert torch.equal(AR.posterize(t, bits), back(ImageOps.posterize(pil, bits))), bits
        for thr in (0, 1, 28, 57, 113, 114, 128, 170, 255):
            assert torch.equal(AR.solarize(t, thr), back(ImageOps.solarize(pil, thr))), thr
    assert not AR.posterize(torch.from_numpy(imgs[0]), 0).any()


def test_policy_table_and_magnitudes():
    from yolosharp_amd import augment as A
    assert len(A.IMAGENET_POLICY) == 25
    assert [tuple((A.AA_ID[op], p, m) for op, p, m in row) for row in A.IMAGENET_POLICY] == POLICY_IDS
    assert A.IMAGENET_POLICY[20:] == (A.IMAGENET_POLICY[4], A.IMAGENET_POLICY[1], A.IMAGENET_POLICY[13], A.IMAGENET_POLICY[14], A.IMAGENET_POLICY[2])
    assert A.AA_OPS == tuple(A.RAND_AUGMENT_OPS[1:6]) + tuple(A.RAND_AUGMENT_OPS[6:]) + ("Invert",) and A.RAND_AUGMENT_OPS[0] == "Identity"
    assert [int(v) for v in A.aa_magnitudes("Posterize", 10, 8, 8)] == [8, 8, 7, 7, 6, 6, 5, 5, 4, 4]
    assert A.aa_magnitudes("Posterize", 31, 8, 8) == [float(v) for v in (8 - (torch.arange(31) / ((31 - 1) / 4)).round().int()).tolist()]
    for bins in (10, 31):
        for op, (lo, hi) in (("ShearX", (0.0, 0.3)), ("ShearY", (0.0, 0.3)), ("TranslateX", (0.0, 150.0 / 331.0 * 9)), ("TranslateY", (0.0, 150.0 / 331.0 * 5)),
                             ("TranslateX", (0.0, 150.0 / 331.0 * 224)), ("Rotate", (0.0, 30.0)), ("Color", (0.0, 0.9)), ("Solarize", (255.0, 0.0))):
            hw = (5, 224) if hi == 150.0 / 331.0 * 224 else (5, 9)
            assert A.aa_magnitudes(op, bins, *hw) == [float(v) for v in torch.linspace(lo, hi, bins)], (op, bins)
    assert A.aa_magnitudes("Equalize", 10, 8, 8) is None


class _ScriptedRng:
    """Hands out a script of (method, value) draws and fails on any other order."""

    def __init__(self, script):
        self.script = list(script)

    def _next(self, name):
        assert self.script and self.script[0][0] == name, (name, self.script[:1])
        return self.script.pop(0)[1]

    def integers(self, *a, **k):
        return np.asarray(self._next("integers"))

    def random(self, *a, **k):
        return np.asarray(self._next("random"))


def test_draw_order():
    """draw_auto_augment against a hand-written expectation: AutoAugment = one policy index, two probabilities, two sign bits per image, a slot runs iff
    prob <= p, negated iff its bit is 0; RandAugment = per op an index, then one bit only for a signed op, negated iff the bit is 1."""
    from yolosharp_amd import augment as A
    hw = (8, 8)
    rng = _ScriptedRng([("integers", 10), ("random", [0.8, 0.4]), ("integers", [0, 1]),        # (Rotate .8 8, Color .4 0): prob 0.8 <= 0.8 runs, bit 0 negates
                        ("integers", 0), ("random", [0.41, 0.61]), ("integers", [1, 0]),       # (Posterize .4 8, Rotate .6 9): both fail
                        ("integers", 14), ("random", [0.0, 1.0]), ("integers", [1, 1])])       # (Color .6 4, Contrast 1.0 8): both run, not negated
    rows = A.draw_auto_augment(rng, 3, hw, A.AutoAugment())
    assert not rng.script
    m_rot, m_blend = A.aa_magnitudes("Rotate", 10, *hw), A.aa_magnitudes("Color", 10, *hw)
    want = A.make_aa_rows(3)
    A.set_aa_slot(want[0], 0, "Rotate", -m_rot[8], hw)
    A.set_aa_slot(want[0], 1, "Color", -m_blend[0], hw)
    A.set_aa_slot(want[2], 0, "Color", m_blend[4], hw)
    A.set_aa_slot(want[2], 1, "Contrast", m_blend[8], hw)
    assert rows.tobytes() == want.tobytes()
    assert rows[0]["op"].tolist() == [4, 6] and rows[1]["op"].tolist() == [-1, -1] and rows[2]["op"].tolist() == [6, 7]
    assert rows[2]["arg"].tolist() == [np.float32(1.0 + m_blend[4]), np.float32(1.0 + m_blend[8])] and m_blend[4] == float(torch.linspace(0.0, 0.9, 10)[4])
    th, ang = rows[0]["theta"][0].astype(np.float64), np.radians(30.0 * 8 / 9)      # angle = -magnitude = +26.67 degrees: the inverse matrix of that rotation
    assert np.allclose(th, [np.cos(ang), np.sin(ang), 0, -np.sin(ang), np.cos(ang), 0], atol=1e-6)
    rng = _ScriptedRng([("integers", 0),                                                       # Identity: no sign draw
                        ("integers", 13),                                                      # Equalize: unsigned, no sign draw
                        ("integers", 10),                                                      # Posterize: unsigned
                        ("integers", 5), ("integers", 1)])                                     # Rotate, bit 1: negated
    rows = A.draw_auto_augment(rng, 2, hw, A.RandAugment())
    assert not rng.script
    assert rows["op"].tolist() == [[-1, 12], [9, 4]]
    want = A.make_aa_rows(2)
    A.set_aa_slot(want[0], 1, "Equalize", 0.0, hw)
    A.set_aa_slot(want[1], 0, "Posterize", A.aa_magnitudes("Posterize", 31, *hw)[9], hw)
    A.set_aa_slot(want[1], 1, "Rotate", -A.aa_magnitudes("Rotate", 31, *hw)[9], hw)
    assert rows.tobytes() == want.tobytes() and rows[1]["arg"][0] == 7.0
    with pytest.raises(ValueError):
        A.RandAugment(num_ops=3)
    with pytest.raises(TypeError):
        A.draw_auto_augment(np.random.default_rng(0), 1, hw, "AutoAugment")


def test_draw_classify_items_without_policy_is_unchanged():
    """auto_augment = None: the pair this function returned before it had the argument, for a fixed seed (the digest was taken from that version); with a policy
    the rows are drawn after the flips and in front of the erasing draws."""
    from yolosharp_amd import augment as A
    shapes = [(5, 9), (13, 7), (37, 23), (224, 224)]
    out = A.draw_classify_items(np.random.default_rng(11), [0, 1, 2, 3, 2, 1], shapes, 8, flipud=0.3)
    assert len(out) == 2
    assert tuple(int(v) for v in out[0][0]) == (0, 1, 4, 3, 3, 8, 8, 0, 0, 1, 1, 7, 5, 1, 3, 3240284249) and out[1][0]["order"].tolist() == [1, 2, 3, 0]
    assert hashlib.sha256(out[0].tobytes() + out[1].tobytes()).hexdigest() == "87f2b8faf463938cd4b20a2c5acf78dda5cad63796663309b95a251a20ba4bda"
    rng = TC._CountingRng(1)
    items, rows, aa = A.draw_classify_items(rng, [0], [(16, 16)], 8, fliplr=0.5, flipud=0, erasing=0.4, hsv=None, scale=(1.0, 1.0), ratio=(1.0, 1.0),
                                            auto_augment=A.AutoAugment())
    assert rows is None and aa.shape == (1,)
    assert rng.calls[:9] == ["random", "random", "integers", "integers", "random", "integers", "random", "integers", "standard_normal"]
    A.check_aa_rows(aa)


def test_policy_argument():
    from yolosharp_amd import augment as A
    img = [np.zeros((3, 4, 4), np.uint8)]
    for bad in ("AutoAugment", "RandAugment", "AugMix"):
        with pytest.raises(NotImplementedError) as ei:
            A.ClassifyAugmenter(None, img, [0], 8, auto_augment=bad)
        assert "augment.AutoAugment()" in str(ei.value) and "augment.RandAugment(" in str(ei.value)
    assert not hasattr(A, "AugMix")


# ---------------------------------------------------------------------------------------------------- kernel parity: the operators on their own
@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("hw", OPS_SHAPES)
def test_ops_parity(backend, engine, hw):
    """Every op alone at every magnitude id and sign, the 25 policy rows and the dependent pairs with both slots on, under both signs: host pointers, then
    device pointers twice (the statistics rows are re-zeroed: identical bytes)."""
    from yolosharp_amd import augment as A
    images, rows, want = _ops_case(hw)
    got = A.auto_augment_ops(engine, images, rows)
    bad = [b for b in range(rows.shape[0]) if not np.array_equal(got[b], want[b])]
    assert not bad, [(b, rows[b]["op"].tolist(), rows[b]["arg"].tolist()) for b in bad[:8]]
    sl = slice(150, 263)
    a = _run_ops_device(engine, images[sl], rows[sl])
    b = _run_ops_device(engine, images[sl], rows[sl])
    assert np.array_equal(a, want[sl]) and a.tobytes() == b.tobytes()
    if hw != (2, 6):
        assert sum(not np.array_equal(want[b], images[b]) for b in range(rows.shape[0])) > 200      # the ops do something


@functools.lru_cache(maxsize=None)
def _flat_case():
    """8 x 8: channel 0 constant (AutoContrast max == min, Equalize step == 0), channel 1 two-valued, channel 2 noise; 13 x 7 likewise."""
    from yolosharp_amd import augment as A
    out = []
    for hw in ((8, 8), (13, 7)):
        img = _image(hw[0], hw[1], 50)
        img[0] = 77
        img[1] = np.where(np.arange(hw[0] * hw[1]).reshape(hw) % 3 == 0, 10, 200)
        lst = [(("AutoContrast", None), None), (("Equalize", None), None), (("Contrast", 8), None), (None, ("Equalize", None)), (("Equalize", None), ("AutoContrast", None)),
               (("Sharpness", 7), ("Equalize", None)), (("Solarize", 5), ("AutoContrast", None)), (("Invert", None), ("Contrast", 3))]
        rows = A.make_aa_rows(len(lst))
        for b, pair in enumerate(lst):
            for k, sl in enumerate(pair):
                if sl is not None:
                    _slot(rows[b], k, sl[0], sl[1], 1, hw)
        images = np.stack([img] * len(lst))
        out.append((images, rows, AR.ops_batch(images, rows)))
    return out


@pytest.mark.parametrize("backend", BACKENDS)
def test_ops_constant_and_two_valued_channels(backend, engine):
    from yolosharp_amd import augment as A
    for images, rows, want in _flat_case():
        assert np.array_equal(A.auto_augment_ops(engine, images, rows), want)
        assert np.array_equal(_run_ops_device(engine, images, rows), want)
        assert np.array_equal(want[0][0], images[0][0]) and np.array_equal(want[1][0], images[1][0])      # the constant channel is left alone
        assert sorted(set(want[0][1].reshape(-1).tolist())) == [0, 255]                                   # the two-valued one is stretched


@pytest.mark.parametrize("backend", BACKENDS)
def test_ops_constant_image_64(backend, engine):
    """64 x 64, every byte 200 in two images and noise in a third: one histogram bin takes all 4096 counts of a channel."""
    from yolosharp_amd import augment as A
    images = np.stack([np.full((3, 64, 64), 200, np.uint8), _image(64, 64, 60), np.full((3, 64, 64), 200, np.uint8)])
    rows = A.make_aa_rows(3)
    _slot(rows[0], 0, "Equalize", None, 1, (64, 64))
    _slot(rows[0], 1, "AutoContrast", None, 1, (64, 64))
    _slot(rows[1], 0, "Equalize", None, 1, (64, 64))
    _slot(rows[1], 1, "Contrast", 6, 1, (64, 64))
    _slot(rows[2], 0, "Contrast", 4, -1, (64, 64))
    _slot(rows[2], 1, "Equalize", None, 1, (64, 64))
    want = AR.ops_batch(images, rows)
    assert np.array_equal(A.auto_augment_ops(engine, images, rows), want)
    assert np.array_equal(_run_ops_device(engine, images, rows), want)
    assert np.array_equal(want[0], images[0]) and not np.array_equal(want[1], images[1])


# ---------------------------------------------------------------------------------------------------- kernel parity: the classification chain
def _aa_kinds(n, s):
    """n rows cycling through the 25 policy rows with both slots on (signs alternating), the dependent pairs, an empty row and one-slot rows."""
    from yolosharp_amd import augment as A
    hw = (s, s)
    kinds = [(row[0], row[1]) for row in A.IMAGENET_POLICY[:20]] + [((a, 1.0, 5), (b, 1.0, 7)) for a, b in PAIRS]
    kinds += [(None, None), (("ShearY", 1.0, 4), None), (None, ("TranslateX", 1.0, 9)), (("TranslateY", 1.0, 9), ("Sharpness", 1.0, 9)), (("Brightness", 1.0, 6), None)]
    rows = A.make_aa_rows(n)
    for b in range(n):
        for k, sl in enumerate(kinds[b % len(kinds)]):
            if sl is not None:
                _slot(rows[b], k, sl[0], sl[2] if A.aa_magnitudes(sl[0], 10, *hw) is not None else None, 1 if (b // len(kinds) + k) % 2 else -1, hw)
    return rows


@functools.lru_cache(maxsize=None)
def _cls_case(s):
    """The items and jitter rows of test_augment_classify's parity case at size s (crops x flips x erase rectangles, contrast in each jitter slot) with a row
    of _aa_kinds each, and the restatement's batches without and with jitter."""
    imgs, _, _ = TC._sources()
    items, rows, _, _ = TC._case(s)
    aa = _aa_kinds(items.shape[0], s)
    return items, rows, aa, AR.batch(imgs, TC.CLASSES, items, s, None, aa), AR.batch(imgs, TC.CLASSES, items, s, rows, aa)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("s", [8, 7])
def test_classify_parity(backend, engine, s):
    """s = 8: 16-byte / 4-byte stores; s = 7: scalar stores.  Host pointers without and with jitter; device pointers twice (identical bytes)."""
    from yolosharp_amd import augment as A
    _, arena, srcs = TC._sources()
    items, rows, aa, plain, jittered = _cls_case(s)
    assert items.shape[0] >= 90
    for sl in TC._chunks(items.shape[0]):
        img, cls = A.augment_classify(engine, arena, srcs, TC.CLASSES, items[sl], s, aa=aa[sl])
        bad = [b for b in range(img.shape[0]) if not np.array_equal(img[b], plain[0][sl][b])]
        assert not bad and np.array_equal(cls, plain[1][sl]), [(b, aa[sl][b]["op"].tolist()) for b in bad[:8]]
        img, cls = A.augment_classify(engine, arena, srcs, TC.CLASSES, items[sl], s, jitter=rows[sl], aa=aa[sl])
        assert np.array_equal(img, jittered[0][sl]) and np.array_equal(cls, jittered[1][sl])
    sl = slice(0, 60)
    a = _run_classify_device(engine, arena, srcs, TC.CLASSES, items[sl], s, rows[sl], aa[sl])
    b = _run_classify_device(engine, arena, srcs, TC.CLASSES, items[sl], s, rows[sl], aa[sl])
    assert np.array_equal(a[0], jittered[0][sl]) and np.array_equal(a[1], jittered[1][sl])
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    c = _run_classify_device(engine, arena, srcs, TC.CLASSES, items[sl], s, None, aa[sl])
    assert np.array_equal(c[0], plain[0][sl])
    _, _, plain_no_aa, _ = TC._case(s)
    assert not np.array_equal(plain[0], plain_no_aa[0])


@pytest.mark.parametrize("backend", BACKENDS)
def test_classify_parity_mixed_batch_32(backend, engine):
    """s = 32, more than one workgroup row per image: Rotate -> Equalize, Color -> Contrast and Sharpness -> AutoContrast under test_augment_classify's mixed items."""
    from yolosharp_amd import augment as A
    imgs, arena, srcs = TC._sources()
    items, rows, _, _ = TC._mixed32()
    aa = A.make_aa_rows(3)
    for b, (a0, a1) in enumerate((("Rotate", "Equalize"), ("Color", "Contrast"), ("Sharpness", "AutoContrast"))):
        _slot(aa[b], 0, a0, 8, -1, (32, 32))
        _slot(aa[b], 1, a1, 8 if a1 == "Contrast" else None, 1, (32, 32))
    want = AR.batch(imgs, TC.CLASSES, items, 32, rows, aa)
    for got in (A.augment_classify(engine, arena, srcs, TC.CLASSES, items, 32, jitter=rows, aa=aa),
                _run_classify_device(engine, arena, srcs, TC.CLASSES, items, 32, rows, aa)):
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("s", [8, 7])
def test_null_rows_are_the_plain_entry(backend, engine, s):
    """ys_augment_classify_aa(aa = NULL) is ys_augment_classify, in both pointer forms."""
    from yolosharp_amd import _lib
    from yolosharp_amd import augment as A
    _, arena, srcs = TC._sources()
    items, rows, _, jittered = TC._case(s)
    sl = slice(0, 60)
    want = TC._run_device(engine, arena, srcs, TC.CLASSES, items[sl], s, rows[sl])
    got = _run_classify_device(engine, arena, srcs, TC.CLASSES, items[sl], s, rows[sl], None)
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes() and np.array_equal(got[0], jittered[0][sl])
    it, jr, cl = np.ascontiguousarray(items[sl]), np.ascontiguousarray(rows[sl]), np.asarray(TC.CLASSES, np.float32)
    img, cls = np.empty((60, 3, s, s), np.float32), np.empty((60,), np.float32)
    _lib.check(engine.lib, engine.lib.ys_augment_classify_aa(engine.ctx, A._ptr(arena), A._ptr(srcs), srcs.shape[0], A._ptr(cl), A._ptr(it), 60, 0, s, None, A._ptr(jr),
                                                             A._ptr(img), A._ptr(cls)))
    assert img.tobytes() == want[0].tobytes() and cls.tobytes() == want[1].tobytes()


# ---------------------------------------------------------------------------------------------------- invalid rows
BAD_AA = {"op_14": ("op", 0, 14), "op_minus_2": ("op", 1, -2), "posterize_bits_9": ("arg", 0, 9.0), "posterize_bits_negative": ("arg", 0, -1.0),
          "arg_nan": ("arg", 1, float("nan")), "arg_inf": ("arg", 1, float("inf")), "theta_nan": ("theta", 0, float("nan")), "theta_inf": ("theta", 1, float("-inf"))}


@functools.lru_cache(maxsize=None)
def _bad_base():
    from yolosharp_amd import augment as A
    imgs, _, _ = TC._sources()
    items, rows, _ = TC._bad_base()
    aa = A.make_aa_rows(3)
    _slot(aa[0], 0, "Equalize", None, 1, (8, 8))
    _slot(aa[0], 1, "Rotate", 8, 1, (8, 8))
    _slot(aa[1], 0, "Posterize", 4, 1, (8, 8))              # row 1, the one made invalid: Posterize in slot 0, nothing in slot 1
    _slot(aa[2], 0, "Color", 4, -1, (8, 8))
    _slot(aa[2], 1, "Contrast", 8, 1, (8, 8))
    images = np.stack([_image(8, 8, 70 + k) for k in range(3)])
    return items, rows, aa, AR.batch(imgs, TC.CLASSES, items, TC.S_BAD, rows, aa), images, AR.ops_batch(images, aa)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("rule", sorted(BAD_AA))
def test_invalid_row(backend, engine, rule):
    """Host pointers: YS_ERR_INVALID_ARG naming the row.  Device pointers: that image is all 114 (* (1 / 255), class -1, in the chain); neighbours unaffected."""
    from yolosharp_amd import YsError
    from yolosharp_amd import augment as A
    _, arena, srcs = TC._sources()
    items, rows, base, want, images, want_ops = _bad_base()
    aa = base.copy()
    field, k, v = BAD_AA[rule]
    if field == "theta":
        aa[1]["theta"][k][4] = v                              # slot 1 of row 1 runs nothing: its entries are checked all the same
    else:
        aa[1][field][k] = v
    with pytest.raises(ValueError):
        A.check_aa_rows(aa)
    for call in (lambda: A.auto_augment_ops(engine, images, aa), lambda: A.augment_classify(engine, arena, srcs, TC.CLASSES, items, TC.S_BAD, jitter=rows, aa=aa)):
        with pytest.raises(YsError) as ei:
            call()
        assert ei.value.status == 1 and "row 1" in str(ei.value), str(ei.value)
    out = _run_ops_device(engine, images, aa)
    assert np.array_equal(out[1], np.full((3, 8, 8), 114, np.uint8)) and np.array_equal(out[0], want_ops[0]) and np.array_equal(out[2], want_ops[2])
    img, cls = _run_classify_device(engine, arena, srcs, TC.CLASSES, items, TC.S_BAD, rows, aa)
    assert np.array_equal(img[1], np.full((3, TC.S_BAD, TC.S_BAD), Q114, np.float32)) and cls[1] == -1.0
    for b in (0, 2):
        assert np.array_equal(img[b], want[0][b]) and cls[b] == want[1][b]


# ---------------------------------------------------------------------------------------------------- above the ABI
@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("policy", ["autoaugment", "randaugment"])
def test_augmenter_batches(backend, engine, policy):
    """ClassifyAugmenter(auto_augment = a policy object): the device batch is the restatement of its own drawn items, jitter rows and aa rows."""
    from yolosharp_amd import augment as A
    imgs, classes = TC._dataset(6)
    s = 16
    pol = A.AutoAugment() if policy == "autoaugment" else A.RandAugment()
    aug = A.ClassifyAugmenter(engine, imgs, classes, s, seed=4, max_batch=4, flipud=0.5, auto_augment=pol)
    active = 0
    for idx in ([5, 0, 3], [1, 2, 4, 0], [3, 3, 5, 1]):
        items, rows, aa = aug.draw(idx)
        host = aug.run(items, rows, aa).to_host()
        want = AR.batch(imgs, classes, items, s, rows, aa)
        assert np.array_equal(host["images"], want[0]) and np.array_equal(host["cls"], want[1])
        active += int((aa["op"] >= 0).sum())
    assert active >= 6
    assert [b.batch for b in aug.batches(4)] == [4]
    vb = next(iter(aug.val_batches(4))).to_host()             # the val chain has no rows
    want = AR.batch(imgs, classes, A.draw_classify_val_items(np.arange(4), aug.shapes, s), s)
    assert np.array_equal(vb["images"], want[0])
    with pytest.raises(ValueError):
        bad = aa.copy()
        bad[1]["op"][0] = 99
        aug.run(items, rows, bad)
    aug.close()


@pytest.mark.parametrize("backend", BACKENDS)
def test_train_step_on_auto_augment_batch(backend, engine):
    """Yolov8n-cls, 32 px, B = 4, fp32: TrainStepDevice on an AutoAugment batch returns the loss of TrainStep on its to_host() copy, bit for bit."""
    from yolosharp_amd import augment as A
    from yolosharp_amd import model as M
    s, B = 32, 4
    imgs, classes = TC._dataset(6)
    aug = A.ClassifyAugmenter(engine, imgs, classes, s, seed=3, max_batch=B, auto_augment=A.AutoAugment())
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
    aug.close()
