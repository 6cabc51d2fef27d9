"""ColorJitter (RandomHSV, Data/Augment.cs:968-987) on the device: ys_color_jitter, the jitter epilogue of ys_augment_mosaic_jitter /
ys_augment_letterbox_jitter (csrc/augment.hip) and MosaicAugmenter(hsv=...) against tests/color_jitter_ref.py, the torch restatement of torchvision's
public uint8 algorithm.

Equality means BIT equality with the float32 restatement: every step of the algorithm is one individually rounded IEEE fp32 operation (the kernels are
compiled without contraction, hipcc's fp32 division is correctly rounded, fmod / floor / trunc are exact), so a mismatch is a bug on one of the two
sides, not noise.  A float64 judge would prove nothing: over the 24 orders with random factors the float32 and the float64 restatement themselves
differ in 0.06 % of the bytes of a random 256 x 256 image (by up to 2 levels) and in 0.14 % of a photograph's (up to 4), because each op truncates
("ColorJitter / RandomHSV", has these and the re-measured figures)."""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest
import torch

import color_jitter_ref as R
from conftest import BACKENDS

PERMS = list(itertools.permutations(range(4)))
# (brightness, contrast, saturation, hue) at the ends of the ranges ColorJitter(0.4, c, 0.7, 0.015) draws from, and at the ends of the hue range the ABI admits
ENDS = [(0.6, 0.5, 0.3, -0.015), (1.4, 1.5, 1.7, 0.015), (0.6, 1.5, 1.7, 0.5), (1.4, 0.5, 0.3, -0.5)]
Q114 = (np.float32(114.0) * np.float32(1 / 255.0)).astype(np.float32)


def _rows(lst):
    from yolosharp_amd import augment as A
    rows = A.make_jitter(len(lst))
    for b, (order, factor) in enumerate(lst):
        rows[b]["order"], rows[b]["factor"] = order, factor
    return rows


def _parity_rows():
    """Each op alone at both ends; the 24 orders with the four factor sets, once with contrast and once with its slot skipped (-1); nothing at all."""
    lst = []
    for op in range(4):
        for f in sorted(set(e[op] for e in ENDS)):
            fac = [1.0, 1.0, 1.0, 0.0]
            fac[op] = f
            lst.append(((op, -1, -1, -1), tuple(fac)))
    for perm in PERMS:
        for e in ENDS:
            lst.append((perm, e))
            lst.append((tuple(-1 if op == R.CONTRAST else op for op in perm), e))
    lst.append(((-1, -1, -1, -1), (1.0, 1.0, 1.0, 0.0)))
    return lst


def _palette():
    """uint8 [3, 43, 128]: all 256 grays (the eqc branch), the corners of the cube (0, 255, primaries, secondaries), every pattern of a tie for the maximum
    channel, a 17^3 lattice of the cube; padded with zeros."""
    cols = [(v, v, v) for v in range(256)]
    cols += list(itertools.product((0, 255), repeat=3))
    for a, b in ((255, 0), (200, 199), (1, 0), (128, 37), (77, 76)):
        cols += [(a, a, b), (a, b, a), (b, a, a), (a, b, b), (b, a, b), (b, b, a), (a, a, a)]
    lat = [min(16 * k, 255) for k in range(17)]
    cols += list(itertools.product(lat, repeat=3))
    w = 128
    h = -(-len(cols) // w)
    img = np.zeros((h * w, 3), np.uint8)
    img[:len(cols)] = cols
    return np.ascontiguousarray(img.T.reshape(3, h, w))


@functools.lru_cache(maxsize=None)
def _parity_case(name):
    """(images uint8 [B, 3, h, w] -- one image repeated under every row --, rows, the restatement's bytes): computed once, never modified."""
    g = np.random.default_rng(17)
    img = {"odd": lambda: g.integers(0, 256, (3, 7, 13)).astype(np.uint8), "random": lambda: g.integers(0, 256, (3, 64, 64)).astype(np.uint8),
           "palette": _palette}[name]()
    lst = _parity_rows()
    images = np.ascontiguousarray(np.broadcast_to(img, (len(lst),) + img.shape))
    want = R.color_jitter_batch(images, lst).numpy()
    return images, _rows(lst), want


# ---------------------------------------------------------------------------------------------------- the restatement itself
def test_restatement_self_checks():
    """Factors (1, 1, 1, 0) reproduce the input bit for bit in every order (the hue round trip); an op at factor 1 / hue 0 is the identity on the palette;
    brightness 0 is black, saturation 0 is gray; hue +0.5 and -0.5 agree (the remainder wraps)."""
    pal = torch.from_numpy(_palette())
    for perm in PERMS:
        assert torch.equal(R.color_jitter(pal, perm, (1.0, 1.0, 1.0, 0.0)), pal)
    assert not R.adjust_brightness(pal, 0.0, torch.float32).any()
    gray = R.adjust_saturation(pal, 0.0, torch.float32)
    assert torch.equal(gray[0], gray[1]) and torch.equal(gray[1], gray[2]) and torch.equal(gray[:1], R.gray(pal, torch.float32))
    assert torch.equal(R.adjust_hue(pal, 0.5, torch.float32), R.adjust_hue(pal, -0.5, torch.float32))
    # the truncation between the ops is real: brightness 0.6 then 1.4 is not brightness 0.84
    assert not torch.equal(R.color_jitter(pal, (0, -1, -1, -1), (0.84, 1, 1, 0)), R.adjust_brightness(R.adjust_brightness(pal, 0.6, torch.float32), 1.4, torch.float32))


# ---------------------------------------------------------------------------------------------------- 1. ys_color_jitter
@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("name", ["odd", "random", "palette"])
def test_color_jitter_parity(backend, engine, name):
    """odd: 7 x 13 (91 pixels: the scalar path, a partial last quad); random: 64 x 64 (the vector path, 4 blocks); palette: every branch of rgb2hsv.
    Contrast sits first, in the middle and last among the 24 orders (the reduction replays what precedes it); all three shapes are <= 256 x 256, where
    the mean is exact."""
    from yolosharp_amd import augment as A
    images, rows, want = _parity_case(name)
    got = A.color_jitter(engine, images, rows)
    bad = np.flatnonzero((got != want).reshape(len(rows), -1).any(1))
    print("%s: %d rows, %d differ" % (name, len(rows), len(bad)), [(rows[b]["order"].tolist(), rows[b]["factor"].tolist()) for b in bad[:4]])
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    gotf = A.color_jitter(engine, images, rows, out_float=True)
    assert gotf.dtype == np.float32 and gotf.tobytes() == R.to_float(torch.from_numpy(want)).numpy().tobytes()
    assert np.array_equal(got[-1], images[-1])                                                            # a row of skipped slots does nothing
    assert (want != images).reshape(len(rows), -1).any(1)[:-1].all()                                      # every other row does something
    again = A.color_jitter(engine, images, rows)
    assert again.tobytes() == got.tobytes()                                                              # integer atomics: run to run identical


@pytest.mark.parametrize("backend", BACKENDS)
def test_skipped_slots_do_nothing(backend, engine):
    """Where the -1 slots sit does not matter, and a factor of an op that is not in the order is not read."""
    from yolosharp_amd import augment as A
    images, _, _ = _parity_case("random")
    e = ENDS[2]
    lst = [((2, 0, -1, -1), e), ((-1, 2, -1, 0), e), ((2, -1, 0, -1), (e[0], 7.0, e[2], 0.25)), ((-1, -1, 2, 0), e)]
    got = A.color_jitter(engine, images[:4], _rows(lst))
    assert all(np.array_equal(got[0], got[b]) for b in range(1, 4)) and not np.array_equal(got[0], images[0])


# ---------------------------------------------------------------------------------------------------- 2. the fused entries
def _sources(shapes, seed, ratio):
    g = np.random.default_rng(seed)
    imgs, masks = [], []
    for h, w in shapes:
        yy, xx = np.mgrid[0:h, 0:w]
        ramp = (xx * 97.0 / max(w - 1, 1) + yy * 89.0 / max(h - 1, 1))[None] + np.array([0.0, 20.0, 40.0])[:, None, None]
        imgs.append(np.clip(ramp + g.integers(0, 70, (3, h, w)), 0, 255).astype(np.uint8))
        masks.append(g.integers(1, 7, (max(h // ratio, 1), max(w // ratio, 1))).astype(np.uint8))
    return imgs, masks


def _bytes_of(images):
    """The bytes behind a plain entry's fp32 images (byte * (1 / 255.0f), checked)."""
    by = np.rint(images * np.float32(255.0)).astype(np.uint8)
    assert R.to_float(torch.from_numpy(by)).numpy().tobytes() == images.tobytes()
    return by


def _fused_items(A, branch, s, n_src, B, perspective, seed):
    hyp = dict(degrees=5.0, translate=0.1, scale=0.5, shear=1.0, perspective=0.0005 if perspective else 0.0)
    if branch == "mosaic":
        items = A.draw_items(np.random.default_rng(seed), [b % n_src for b in range(B)], s, n_src, hyp, 0.5, 0.5)
    else:
        items = A.make_items(B)
        items["src"][:, 0] = [b % n_src for b in range(B)]
    items["flip_lr"], items["flip_ud"] = [(1, 0, 1, 1)[b % 4] for b in range(B)], [(0, 1, 1, 0)[b % 4] for b in range(B)]      # the flips are on
    return items


def _fused_rows(B):
    """Rows without contrast: the orders of (brightness, saturation, hue, nothing), factor sets at the range ends; image 3 runs nothing."""
    perms = list(itertools.permutations((0, 2, 3, -1)))
    lst = [(perms[(5 * b + 1) % 24], ENDS[b % 4]) for b in range(B)]
    if B > 3:
        lst[3] = ((-1, -1, -1, -1), ENDS[0])
    return _rows(lst)


def _fused(A, engine, branch, arena, srcs, items, s, r, perspective, jitter):
    if branch == "mosaic":
        return A.augment_mosaic(engine, arena, srcs, items, s, r, perspective, with_masks=True, jitter=jitter)
    return A.augment_letterbox(engine, arena, srcs, items, s, r, with_masks=True, jitter=jitter)


def _fused_null(engine, branch, arena, srcs, items, s, r, perspective):
    """The *_jitter entry with jitter = NULL, on host arrays."""
    from yolosharp_amd import _lib
    B = items.shape[0]
    images, masks = np.empty((B, 3, s, s), np.float32), np.empty((B, s // r, s // r), np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    lib = engine.lib
    if branch == "mosaic":
        st = lib.ys_augment_mosaic_jitter(engine.ctx, p(arena), p(srcs), srcs.shape[0], p(items), B, 0, s, r, int(perspective), None, p(images), p(masks))
    else:
        st = lib.ys_augment_letterbox_jitter(engine.ctx, p(arena), p(srcs), srcs.shape[0], p(items), B, 0, s, r, None, p(images), p(masks))
    _lib.check(lib, st)
    return images, masks


FUSED_SHAPES = {32: [(32, 32), (32, 24), (20, 32), (28, 30), (40, 36)], 30: [(30, 30), (30, 23), (19, 30), (28, 26), (40, 36)]}


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("branch,perspective", [("mosaic", False), ("mosaic", True), ("letterbox", False)])
@pytest.mark.parametrize("s", [32, 30])
def test_fused_entries(backend, engine, s, branch, perspective):
    """s = 32: 16-byte stores; s = 30: scalar stores and a partial last quad.  The jittered output is the restatement applied to the bytes of the plain
    entry's output, times 1 / 255.0f; the masks do not move; jitter = NULL is the plain entry."""
    from yolosharp_amd import augment as A
    r, B = 2, 6
    imgs, masks = _sources(FUSED_SHAPES[s], seed=s, ratio=r)
    arena, srcs = A.pack_sources(imgs, masks)
    items = _fused_items(A, branch, s, len(imgs), B, perspective, seed=3)
    rows = _fused_rows(B)
    plain, pmask = _fused(A, engine, branch, arena, srcs, items, s, r, perspective, None)
    by = _bytes_of(plain)
    assert (by == 114).mean() > 0.02 and (by != 114).mean() > 0.3                                        # border / padding and picture are both there
    got, gmask = _fused(A, engine, branch, arena, srcs, items, s, r, perspective, rows)
    want = R.color_jitter_batch(by, rows)
    assert got.tobytes() == R.to_float(want).numpy().tobytes()
    assert gmask.tobytes() == pmask.tobytes() and pmask.any()
    assert got[3].tobytes() == plain[3].tobytes() and all(got[b].tobytes() != plain[b].tobytes() for b in (0, 1, 2, 4, 5))
    nimg, nmask = _fused_null(engine, branch, arena, srcs, items, s, r, perspective)
    assert nimg.tobytes() == plain.tobytes() and nmask.tobytes() == pmask.tobytes()


# ---------------------------------------------------------------------------------------------------- 3. boundaries
BAD_ROWS = [((0, 0, -1, -1), (1.0, 1.0, 1.0, 0.0)),            # an id twice
            ((4, -1, -1, -1), (1.0, 1.0, 1.0, 0.0)),           # an id of 4
            ((-2, 0, -1, -1), (1.0, 1.0, 1.0, 0.0)),           # an id below -1
            ((0, 2, 3, -1), (-0.1, 1.0, 1.0, 0.0)),            # a negative factor
            ((0, 2, 3, -1), (1.0, 1.0, float("nan"), 0.0)),    # NaN
            ((0, 2, 3, -1), (float("inf"), 1.0, 1.0, 0.0)),    # not finite
            ((-1, -1, -1, -1), (1.0, 1.0, 1.0, 0.6)),          # hue 0.6 (checked whether or not the op runs)
            ((3, -1, -1, -1), (1.0, 1.0, 1.0, float("nan")))]
CONTRAST_ROW = ((0, 1, 2, 3), ENDS[0])


def _on_device(engine, arrays, out_shapes, call):
    """Upload `arrays`, allocate outputs pre-filled with 77, run call(lib, ctx, inputs, outputs) and read the outputs back."""
    from yolosharp_amd import _lib
    e = engine
    ins = [e.to_device(np.ascontiguousarray(a)) for a in arrays]
    host = [np.full(shape, 77, dtype) for shape, dtype in out_shapes]
    outs = [e.to_device(h) for h in host]
    try:
        _lib.check(e.lib, call(e.lib, e.ctx, ins, outs))
        return [e.from_device(o, h.shape, h.dtype) for o, h in zip(outs, host)]
    finally:
        for p in ins + outs:
            e.free(p)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("branch", ["mosaic", "letterbox"])
def test_fused_boundaries(backend, engine, branch):
    from yolosharp_amd import YsError
    from yolosharp_amd import augment as A
    s, r, B = 32, 2, 4
    imgs, masks = _sources(FUSED_SHAPES[s], seed=5, ratio=r)
    arena, srcs = A.pack_sources(imgs, masks)
    items = _fused_items(A, branch, s, len(imgs), B, False, seed=4)
    good = _fused_rows(B)
    want, wmask = _fused(A, engine, branch, arena, srcs, items, s, r, False, good)

    def with_row(row):
        rows = good.copy()
        rows[1]["order"], rows[1]["factor"] = row
        return rows
    with pytest.raises(YsError) as e:
        _fused(A, engine, branch, arena, srcs, items, s, r, False, with_row(CONTRAST_ROW))
    assert e.value.status == 4                                       # YS_ERR_UNSUPPORTED
    for row in BAD_ROWS:
        with pytest.raises(YsError) as e:
            _fused(A, engine, branch, arena, srcs, items, s, r, False, with_row(row))
        assert e.value.status == 1, row                              # YS_ERR_INVALID_ARG

    def device(rows):
        def call(lib, ctx, i, o):
            if branch == "mosaic":
                return lib.ys_augment_mosaic_jitter(ctx, i[0], i[1], len(imgs), i[2], B, 1, s, r, 0, i[3], o[0], o[1])
            return lib.ys_augment_letterbox_jitter(ctx, i[0], i[1], len(imgs), i[2], B, 1, s, r, i[3], o[0], o[1])
        return _on_device(engine, [arena, srcs, items, rows], [((B, 3, s, s), np.float32), ((B, s // r, s // r), np.float32)], call)
    dimg, dmask = device(good)
    assert dimg.tobytes() == want.tobytes() and dmask.tobytes() == wmask.tobytes()                        # on_device = 0 and 1: the same bytes
    for row in BAD_ROWS + [CONTRAST_ROW]:
        dimg, dmask = device(with_row(row))
        assert np.all(dimg[1] == Q114), row                          # the all-114 image, not jittered
        assert all(dimg[b].tobytes() == want[b].tobytes() for b in (0, 2, 3)), row                       # the neighbours are intact
        assert dmask.tobytes() == wmask.tobytes()                    # the masks do not read the rows


@pytest.mark.parametrize("backend", BACKENDS)
def test_color_jitter_boundaries(backend, engine):
    from yolosharp_amd import YsError
    from yolosharp_amd import augment as A
    images, _, _ = _parity_case("random")
    images = images[:3]
    lst = [(PERMS[7], ENDS[0]), (PERMS[13], ENDS[1]), ((2, -1, 3, 0), ENDS[2])]
    want = A.color_jitter(engine, images, _rows(lst))
    assert np.array_equal(want, R.color_jitter_batch(images, lst).numpy())
    for row in BAD_ROWS:
        with pytest.raises(YsError) as e:
            A.color_jitter(engine, images, _rows([lst[0], row, lst[2]]))
        assert e.value.status == 1, row
    for c in (dict(h=0), dict(w=-1), dict(batch=0)):
        out = np.empty(images.shape, np.uint8)
        rows = _rows(lst)
        st = engine.lib.ys_color_jitter(engine.ctx, images.ctypes.data_as(C.c_void_p), rows.ctypes.data_as(C.c_void_p), c.get("batch", 3), c.get("h", 64),
                                        c.get("w", 64), 0, out.ctypes.data_as(C.c_void_p), 0)
        assert st == 1, c

    def device(rows, is_float):
        call = lambda lib, ctx, i, o: lib.ys_color_jitter(ctx, i[0], i[1], 3, 64, 64, 1, o[0], int(is_float))
        return _on_device(engine, [images, rows], [(images.shape, np.float32 if is_float else np.uint8)], call)[0]
    assert device(_rows(lst), False).tobytes() == want.tobytes()                                          # contrast rows through device pointers too
    assert device(_rows(lst), True).tobytes() == R.to_float(torch.from_numpy(want)).numpy().tobytes()
    for row in BAD_ROWS:
        got = device(_rows([lst[0], row, lst[2]]), False)
        assert np.all(got[1] == 114) and np.array_equal(got[0], want[0]) and np.array_equal(got[2], want[2]), row


# ---------------------------------------------------------------------------------------------------- 4. MosaicAugmenter
class _Log:
    """A numpy Generator that writes down what is drawn from it."""

    def __init__(self, seed):
        self.g, self.calls = np.random.default_rng(seed), []

    def random(self, size=None):
        self.calls.append(("random", 1 if size is None else int(np.prod(size))))
        return self.g.random(size)

    def integers(self, *a, **k):
        self.calls.append(("integers",))
        return self.g.integers(*a, **k)

    def permutation(self, n):
        self.calls.append(("permutation", n))
        return self.g.permutation(n)


def _tiny_dataset(seed, s=32):
    g = np.random.default_rng(seed)
    shapes = [(s, s), (s, 24 * s // 32), (20 * s // 32, s), (s, s), (28 * s // 32, 30 * s // 32), (s, s)]
    imgs, masks = _sources(shapes, seed=seed, ratio=4)
    labels = []
    for h, w in shapes:
        x1, y1 = g.random(3) * w * 0.5, g.random(3) * h * 0.5
        boxes = np.stack([x1, y1, x1 + (0.25 + 0.25 * g.random(3)) * w, y1 + (0.25 + 0.25 * g.random(3)) * h], 1).astype(np.float32)
        labels.append(dict(cls=g.integers(0, 5, 3).astype(np.float32), bboxes=boxes))
    return imgs, masks, labels


def test_draw_jitter_follows_get_params():
    """randperm(4) first, then brightness, contrast, saturation, hue -- a draw only for a non-zero gain, whose op keeps its slot as -1."""
    from yolosharp_amd import augment as A
    log = _Log(8)
    rows = A.draw_jitter(log, 3, 0.015, 0.7, 0.4)                    # RandomHSV's argument order: hgain, sgain, vgain
    assert log.calls == [("permutation", 4), ("random", 1), ("random", 1), ("random", 1)] * 3
    g = np.random.default_rng(8)
    for b in range(3):
        perm, ub, us, uh = g.permutation(4), g.random(), g.random(), g.random()
        assert rows[b]["order"].tolist() == [-1 if op == 1 else int(op) for op in perm]
        want = np.array([0.6 + 0.8 * ub, 1.0, 0.3 + 1.4 * us, -0.015 + 0.03 * uh], np.float32)
        assert np.allclose(rows[b]["factor"], want, rtol=1e-6, atol=1e-9)
        assert 0.6 <= rows[b]["factor"][0] <= 1.4 and 0.3 <= rows[b]["factor"][2] <= 1.7 and abs(rows[b]["factor"][3]) <= 0.015
    log = _Log(8)
    rows = A.draw_jitter(log, 2, 0.0, 0.7, 0.0, cgain=0.5)            # contrast and saturation only
    assert log.calls == [("permutation", 4), ("random", 1), ("random", 1)] * 2
    assert all(sorted(r["order"].tolist()) == [-1, -1, 1, 2] and r["factor"][0] == 1.0 and r["factor"][3] == 0.0 for r in rows)
    assert 0.5 <= rows[0]["factor"][1] <= 1.5 and A.draw_jitter(_Log(1), 1, 0.0, 0.0, 1.5)[0]["factor"][0] >= 0.0      # brightness U(max(0, 1 - v), 1 + v)
    A.check_jitter(rows, allow_contrast=True)
    with pytest.raises(ValueError):
        A.check_jitter(rows)                                         # the fused entries take no contrast row
    for row in BAD_ROWS:
        with pytest.raises(ValueError):
            A.check_jitter(_rows([row]), allow_contrast=True)


@pytest.mark.parametrize("backend", BACKENDS)
def test_augmenter_without_hsv_is_unchanged(backend, engine):
    """hsv = None (the default): the draws, the items and the bytes of an augmenter built without the argument, in both modes."""
    from yolosharp_amd import augment as A
    s = 32
    imgs, masks, labels = _tiny_dataset(5)
    kw = dict(masks=masks, mask_ratio=4, seed=9, max_batch=4, degrees=5.0, shear=1.0)
    a1, a2 = A.MosaicAugmenter(engine, imgs, labels, s, **kw), A.MosaicAugmenter(engine, imgs, labels, s, hsv=None, **kw)
    for closed in (False, True):
        a1.close_mosaic(closed); a2.close_mosaic(closed)
        a1.rng, a2.rng = _Log(3), _Log(3)
        i1, i2 = a1.draw([0, 3, 5, 1]), a2.draw([0, 3, 5, 1])
        per_image = [("random", 1)] if closed else [("integers",)] * 3 + [("random", 8), ("random", 1)]
        assert a1.rng.calls == a2.rng.calls == per_image * 4 and isinstance(i2, np.ndarray) and i1.tobytes() == i2.tobytes()
        h1, h2 = a1.run(i1).to_host(), a2.run(i2).to_host()
        assert sorted(h1) == sorted(h2) and all(h1[k].tobytes() == h2[k].tobytes() for k in h1)
        h3 = a2.batch([0, 3, 5, 1]).to_host()
        assert h3["images"].shape == h1["images"].shape
    assert a2.d_jitter is None
    a1.close(); a2.close()


@pytest.mark.parametrize("backend", BACKENDS)
def test_augmenter_with_hsv(backend, engine):
    from yolosharp_amd import augment as A
    s, idx = 32, [4, 1, 2, 0]
    imgs, masks, labels = _tiny_dataset(5)
    hsv = (0.015, 0.7, 0.4)                                          # the reference's default
    aug = A.MosaicAugmenter(engine, imgs, labels, s, masks=masks, mask_ratio=4, seed=9, max_batch=4, degrees=5.0, shear=1.0, flipud=0.25, hsv=hsv)
    jit = [("permutation", 4), ("random", 1), ("random", 1), ("random", 1)]
    for closed in (False, True):
        aug.close_mosaic(closed)
        aug.rng = log = _Log(3)
        items, rows = aug.draw(idx)
        geom = [] if closed else [("integers",)] * 3 + [("random", 8)]
        assert log.calls == (geom + [("random", 1), ("random", 1)] + jit) * 4                             # per image: ..., FlipLR, FlipUD, then the jitter
        # the same stream, image by image, through the hsv-free draw and draw_jitter
        g = np.random.default_rng(3)
        for b, k in enumerate(idx):
            it = A.draw_letterbox_items(g, [k], 0.5, 0.25) if closed else A.draw_items(g, [k], s, len(imgs), aug.hyp, 0.5, 0.25)
            assert it.tobytes() == items[b:b + 1].tobytes()
            assert A.draw_jitter(g, 1, *hsv).tobytes() == rows[b:b + 1].tobytes()
        assert all(sorted(r["order"].tolist()) == [-1, 0, 2, 3] for r in rows)
        # the batch is the restatement applied to the un-jittered batch's bytes; labels and masks do not move
        plain = aug.run(items).to_host()
        db = aug.run(items, rows)
        got = db.to_host()
        assert db.mode == ("letterbox" if closed else "mosaic")
        want = R.to_float(R.color_jitter_batch(_bytes_of(plain["images"]), rows)).numpy()
        assert got["images"].tobytes() == want.tobytes() and got["images"].tobytes() != plain["images"].tobytes()
        assert all(got[k].tobytes() == plain[k].tobytes() for k in ("masks", "batch_idx", "cls", "bboxes"))
        assert aug.batch(idx).to_host()["images"].shape == want.shape
        with pytest.raises(ValueError):                              # rows are validated on the host before the upload
            aug.run(items, _rows([CONTRAST_ROW] * 4))
        with pytest.raises(ValueError):
            aug.run(items, _rows([BAD_ROWS[0]] * 4))
    aug.close()
    # a gain of 0 draws nothing for its op and leaves its slot empty
    a0 = A.MosaicAugmenter(engine, imgs, labels, s, seed=9, max_batch=4, hsv=(0.015, 0.0, 0.4))
    a0.close_mosaic(True)
    a0.rng = log = _Log(3)
    _, rows = a0.draw(idx)
    assert log.calls == [("random", 1), ("permutation", 4), ("random", 1), ("random", 1)] * 4
    assert all(sorted(r["order"].tolist()) == [-1, -1, 0, 3] and r["factor"][2] == 1.0 for r in rows)
    a0.close()


@pytest.mark.parametrize("backend", BACKENDS)
def test_train_step_on_jittered_batch(backend, engine):
    """One detect train step on a jittered DeviceBatch (64 px): a finite loss."""
    from yolosharp_amd import augment as A
    from yolosharp_amd import model as M
    s = 64
    imgs, _, labels = _tiny_dataset(2, s=s)
    aug = A.MosaicAugmenter(engine, imgs, labels, s, seed=3, max_batch=2, hsv=(0.015, 0.7, 0.4))
    db = aug.batch([1, 4])
    m = M.Yolov8(engine, nc=5, size="n", height=s, width=s, max_batch=2, dtype="f32")
    m.init_weights(1)
    _, it = M.AMPWrapper(m).TrainStepDevice(db, M.v8DetectionLoss(m))
    m.close(); aug.close()
    assert np.all(np.isfinite(it)) and it[0] > 0


# ---------------------------------------------------------------------------------------------------- 5. the workload's sizes
CUBE_ROWS = [((0, 2, 3, -1), ENDS[0]), ((3, -1, 2, 0), ENDS[1]), ((3, -1, -1, -1), (1.0, 1.0, 1.0, 0.015)), ((-1, 3, -1, -1), (1.0, 1.0, 1.0, -0.015))]


@pytest.mark.gpu
@pytest.mark.parametrize("case", range(len(CUBE_ROWS)))
def test_whole_colour_cube(case):
    """Every one of the 2^24 colours, as one 4096 x 4096 image: brightness, saturation and hue in two orders, and hue alone at +-0.015."""
    from yolosharp_amd import Engine
    from yolosharp_amd import augment as A
    i = np.arange(1 << 24, dtype=np.uint32)
    img = np.stack([i & 255, (i >> 8) & 255, i >> 16]).astype(np.uint8).reshape(1, 3, 4096, 4096)
    got = A.color_jitter(Engine(), img, _rows([CUBE_ROWS[case]]))
    want = R.color_jitter_batch(img, [CUBE_ROWS[case]]).numpy()
    diff = got != want
    print("case %d: %d of %d bytes differ" % (case, int(diff.sum()), diff.size), np.argwhere(diff)[:4].tolist())
    assert not diff.any()


@pytest.mark.gpu
@pytest.mark.parametrize("branch", ["mosaic", "letterbox"])
def test_large_fused_batch(branch):
    """B = 4 at 640 x 640, the workload's row length, against the restatement."""
    from yolosharp_amd import Engine
    from yolosharp_amd import augment as A
    s, r, B = 640, 4, 4
    imgs, masks = _sources([(640, 480), (427, 640), (639, 480), (500, 375)], seed=5, ratio=r)
    arena, srcs = A.pack_sources(imgs, masks)
    items = _fused_items(A, branch, s, len(imgs), B, False, seed=6)
    rows = _fused_rows(B)
    eng = Engine()
    plain, pmask = _fused(A, eng, branch, arena, srcs, items, s, r, False, None)
    got, gmask = _fused(A, eng, branch, arena, srcs, items, s, r, False, rows)
    want = R.to_float(R.color_jitter_batch(_bytes_of(plain), rows)).numpy()
    assert got.tobytes() == want.tobytes() and gmask.tobytes() == pmask.tobytes()
    assert got[3].tobytes() == plain[3].tobytes() and got[0].tobytes() != plain[0].tobytes()
