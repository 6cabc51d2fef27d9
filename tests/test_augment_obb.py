"""OBB corner labels of the device training input (csrc/augment.hip: ys_xyxyxyxy2xywhr, ys_augment_labels_obb, ys_augment_letterbox_labels_obb;
yolosharp_amd/augment.py; AMPWrapper.TrainStepDevice; Trainer.fit) against tests/aug_obb_ref.py, the float64 restatement with an explicit hull.

HOW A RECTANGLE IS COMPARED (_check_rows).  Both sides become four corners.  The kernel's rectangle must coincide -- as a corner set, any starting
corner, either orientation -- with ONE of the restatement's hull-edge candidates whose area is within the slack of the minimum, and its own area
must be within that slack too.  No row is exempted.  OpenCV is not available, so WHICH of several equal-area rectangles the reference binary would
return is unpinned; the rule accepts each of them.  A collinear row (w = the span, h = 0) is held to the same rule -- it must describe the segment it
encloses -- which is why its angle is the line's own direction in (0, pi] and not a quarter-turn fold of it (include/yolosharp_hip.h).

THE BOUNDS, derived from the number formats (u = 2^-24, the unit roundoff of fp32; S = the image size, the magnitude of every coordinate):
  DIST_OP  the operator alone.  Restatement and kernel read the SAME fp32 corners; the kernel works in double (error ~1e-13) and rounds its five
           results to fp32 once.  A rebuilt corner is c +- (w/2) u(angle) +- (h/2) n(angle): the centre's two roundings move it by <= sqrt(2) u S;
           w and h (each <= sqrt(2) S) by <= sqrt(2) u S each, halved and summed sqrt(2) u S; the angle (<= pi/2) by <= u pi/2 radians on a lever
           of at most half a diagonal <= S: together (2 sqrt(2) + pi/2) u S = 4.4 u S = 1.7e-5 px at S = 64.
  rows of the label entries add (a) the division by S in fp32, undone here in double: the same budget once more, 2 DIST_OP in all; (b) the fp32
           chain in front of the rectangle, which the restatement runs in float64: EPS_IN per corner.  Mosaic: every intermediate of
           + pad, x a + y b + c is below 8 S in magnitude (coordinates <= 3 S on and around the canvas, |a|, |b| <= 1.5, |c| <= 2 S) and a coordinate
           passes at most 6 roundings (the pad add counted twice for its amplification by the matrix), the perspective divide adds 4 u S, a flip
           u S: 53 u S per coordinate, 75 u S per point.  LetterBox: a pad add and a flip at magnitude <= 2 S: 4 u S per coordinate, 6 u S per point.
           A perturbation eps of the points turns a hull edge of length L by <= 2 eps / L, which moves a corner of a point set of diameter D by
           <= (2 D / L) eps, and shifts the extents by <= 2 eps: eta = 2 DIST_OP + EPS_IN (2 + 2 D / L), L = the SHORTEST hull edge of the row's
           data (generated sides are >= 2 px; clipping can shorten an edge, and the row's own L then widens its own bound -- nothing is excluded).
  area     a rectangle whose corners move by eta changes its sides by <= 2 eta and its area by <= 2 eta (w + h) + 4 eta^2: with the largest w + h
           among the row's candidates that is the slack, i.e. delta = 2 eta (1 / w + 1 / h) relative to the minimum for a well-posed row."""
import functools
import math

import numpy as np
import pytest
import torch

import aug_letterbox_ref as LR
import aug_obb_ref as R
import aug_ref
from conftest import BACKENDS

S = 64
U = 2.0 ** -24
DIST_OP = (2 * math.sqrt(2) + math.pi / 2) * U * S
EPS_MOSAIC, EPS_LETTERBOX = 75 * U * S, 6 * U * S
HALF_PI = np.float32(np.pi / 2)
SHAPES = [(64, 48), (40, 64), (64, 64), (50, 60), (64, 64), (30, 30)]      # (h, w)


# ---------------------------------------------------------------------------------------------------- helpers
def _rot_rects(g, n, cx_lo, cx_hi, cy_lo, cy_hi, side_lo=2.0, side_hi=24.0):
    """n random rectangles, every rotation, sides in [side_lo, side_hi], as fp32 corners [n, 4, 2] in order around the rectangle."""
    c = np.stack([cx_lo + g.random(n) * (cx_hi - cx_lo), cy_lo + g.random(n) * (cy_hi - cy_lo)], 1)
    w, h, a = side_lo + g.random(n) * (side_hi - side_lo), side_lo + g.random(n) * (side_hi - side_lo), g.random(n) * 2 * np.pi
    u, v = np.stack([np.cos(a), np.sin(a)], 1), np.stack([-np.sin(a), np.cos(a)], 1)
    return np.stack([c + s1 * w[:, None] / 2 * u + s2 * h[:, None] / 2 * v for s1, s2 in ((-1, -1), (1, -1), (1, 1), (-1, 1))], 1).astype(np.float32)


def _eta(points, eps_in):
    """The corner-distance bound of one label row (module docstring) from the row's own data."""
    h = R.hull(points)
    if len(h) < 2:
        return 2 * DIST_OP + 2 * eps_in
    P = np.stack(h)
    D = max(float(np.linalg.norm(p - q)) for p in P for q in P)
    L = min(float(np.linalg.norm(P[(i + 1) % len(P)] - P[i])) for i in range(len(P)))
    return 2 * DIST_OP + eps_in * (2 + 2 * D / L)


def _check_rows(rows, points, eta_of, what):
    """rows [n, 5] in the units of points [n, 4, 2] (float64 restatement inputs); eta_of(i) = the row's distance bound.  Prints the worst figures
    before it asserts."""
    rows, worst_d, worst_a, fails = np.asarray(rows, np.float64), 0.0, 0.0, []
    for i in range(len(rows)):
        eta = eta_of(i)
        cand = R.candidates(points[i])
        amin = min(a for _, a, _ in cand)
        slack = 2 * eta * max(a + b for _, _, (a, b) in cand) + 4 * eta * eta
        area = rows[i, 2] * rows[i, 3]
        d = min(R.corner_set_distance(R.row_corners(rows[i]), c) for c, a, _ in cand if a <= amin + slack)
        worst_d, worst_a = max(worst_d, d / eta), max(worst_a, (area - amin) / slack)
        if not (d <= eta and area <= amin + slack):
            fails.append((i, d, eta, area, amin, slack))
        if rows[i, 2] != 0 or rows[i, 3] != 0 or rows[i, 4] != 0:          # (0, pi/2]; a collinear row (h == 0) carries its line's direction in (0, pi]
            assert 0 < np.float32(rows[i, 4]) <= (HALF_PI if rows[i, 3] > 0 else np.float32(np.pi)), (what, i, rows[i])
        assert np.all(np.isfinite(rows[i])) and rows[i, 2] >= 0 and rows[i, 3] >= 0, (what, i, rows[i])
    print("%s: %d rows, worst corner distance / bound %.3g, worst area excess / slack %.3g" % (what, len(rows), worst_d, worst_a))
    assert not fails, (what, fails[:5])


def _matrix(s, angle=0.0, scale=1.0, persp=(0.0, 0.0), trans=(0.5, 0.5)):
    """M = T @ R @ P @ C of affine_transform (Data/Augment.cs:323-356) from explicit parameters, fp32."""
    f = np.float32
    Cm, P, Rm, T = (np.eye(3, dtype=f) for _ in range(4))
    Cm[0, 2] = Cm[1, 2] = -s
    P[2, 0], P[2, 1] = persp
    rad = f(angle) * f(np.pi) / f(180.0)
    a, b = f(np.cos(rad)) * f(scale), f(np.sin(rad)) * f(scale)
    Rm[0, :2], Rm[1, :2] = (a, b), (-b, a)
    T[0, 2], T[1, 2] = trans[0] * s, trans[1] * s
    return (T @ (Rm @ (P @ Cm))).astype(f)


def _pack_items(lst):
    from yolosharp_amd import augment as A
    it = A.make_items(len(lst))
    for b, (src, xc, yc, M, flr, fud) in enumerate(lst):
        it[b]["src"], it[b]["xc"], it[b]["yc"], it[b]["M"], it[b]["flip_lr"], it[b]["flip_ud"] = src, xc, yc, np.asarray(M, np.float32).reshape(9), flr, fud
    return it


def _sources(shapes, seed=11):
    g = np.random.default_rng(seed)
    return [g.integers(0, 256, (3, h, w)).astype(np.uint8) for h, w in shapes]


def _raw_labels(shapes, seed, per_source=6):
    """Per source: rotated rectangles with sides in [2, 0.45 x the source], centres anywhere in the source (so corners also lie outside it), "obb"
    corners only: the axis-aligned box is what pack_labels derives.  cls = a unique id: the kept set and its order are visible."""
    g = np.random.default_rng(seed)
    labels, uid = [], 0
    for h, w in shapes:
        obb = _rot_rects(g, per_source, 0.1 * w, 0.9 * w, 0.1 * h, 0.9 * h, 2.0, 0.45 * min(h, w))
        labels.append(dict(cls=np.arange(uid, uid + per_source, dtype=np.float32), obb=obb))
        uid += per_source
    return labels


def _pads(src, xc, yc, shapes, s):
    return aug_ref.mosaic4([torch.zeros((3,) + tuple(shapes[k]), dtype=torch.uint8) for k in src], None, xc, yc, s, 4)[2]


def _restate_mosaic(labels, boxes_of, items, shapes, perspective):
    """-> (batch_idx, cls, corners [n, 4, 2] pixels float64, margins per image) of the batch, in collate order."""
    bi, cl, xy, mg = [], [], [], []
    for b, (src, xc, yc, M, flr, fud) in enumerate(items):
        tiles = [dict(cls=labels[k]["cls"], boxes=boxes_of[k], obb=labels[k]["obb"]) for k in src]
        c, p, m = R.mosaic_sample(tiles, _pads(src, xc, yc, shapes, S), M, flr, fud, S, perspective)
        bi.append(np.full(len(c), float(b), np.float32)); cl.append(c); xy.append(p); mg.append(m)
    return np.concatenate(bi), np.concatenate(cl), np.concatenate(xy), mg


def _to_pixels(bboxes):
    rows = np.asarray(bboxes, np.float64).copy()
    rows[:, :4] *= S
    return rows


# ---------------------------------------------------------------------------------------------------- 1-4: the operator
@pytest.mark.parametrize("backend", BACKENDS)
def test_operator_well_posed(backend, engine):
    """Random rectangles, every rotation, unclipped (more than one block of 256 rows): the rectangle rule; angle in (0, pi/2]; w lies along the
    angle; the rebuilt rectangle encloses its inputs."""
    from yolosharp_amd import augment as A
    pts = _rot_rects(np.random.default_rng(5), 600, 16, 48, 16, 48)
    rows = A.xyxyxyxy2xywhr(engine, pts)
    assert rows.shape == (600, 5) and rows.dtype == np.float32
    _check_rows(rows, pts.astype(np.float64), lambda i: DIST_OP, "operator")
    assert np.all(rows[:, 4] > 0) and np.all(rows[:, 4] <= HALF_PI) and rows[:, 4].min() < 0.1 and rows[:, 4].max() > 1.5
    for i in range(len(rows)):
        a = float(rows[i, 4])
        ext = pts[i].astype(np.float64) @ np.array([math.cos(a), math.sin(a)])
        assert abs((ext.max() - ext.min()) - rows[i, 2]) <= 2 * DIST_OP, (i, rows[i])                 # w is the side along the angle
        assert R.outside_distance(rows[i], pts[i]) <= DIST_OP, (i, rows[i])
    assert np.array_equal(A.xyxyxyxy2xywhr(engine, np.zeros((0, 4, 2), np.float32)), np.zeros((0, 5), np.float32))     # n = 0: a no-op


def _orders(p):
    p = np.asarray(p, np.float32)
    return [np.roll(q, k, axis=0) for q in (p, p[::-1]) for k in range(4)]


@pytest.mark.parametrize("backend", BACKENDS)
def test_operator_canonical_form(backend, engine):
    from yolosharp_amd import augment as A
    axis = [(3, 5), (11, 5), (11, 8), (3, 8)]                     # x extent 8, y extent 3
    diag = [(2, 0), (5, 3), (3, 5), (0, 2)]                       # sides 3 sqrt(2) along 45 degrees, 2 sqrt(2) across
    rows = A.xyxyxyxy2xywhr(engine, np.stack(_orders(axis) + _orders(diag)))
    # an axis-aligned rectangle is angle = pi/2 with (w, h) = (y extent, x extent); exact
    assert np.array_equal(rows[0], np.array([7, 6.5, 3, 8, HALF_PI], np.float32)), rows[0]
    assert np.array_equal(rows[8], np.array([2.5, 2.5, 3 * math.sqrt(2), 2 * math.sqrt(2), np.pi / 4], np.float32)), rows[8]
    # the 4 rotations and both orientations of the corner list: identical bits
    assert all(rows[k].tobytes() == rows[0].tobytes() for k in range(8)) and all(rows[k].tobytes() == rows[8].tobytes() for k in range(8, 16)), rows


@pytest.mark.parametrize("backend", BACKENDS)
def test_operator_ties_and_non_rectangles(backend, engine):
    """An acute triangle (one point repeated: its three edges tie exactly), a point inside the triangle of the other three, a trapezoid."""
    from yolosharp_amd import augment as A
    tri = [(0, 0), (8, 0), (4, math.sqrt(48.0)), (4, math.sqrt(48.0))]                   # equilateral to rounding
    acute = [(0, 0), (10, 0), (4, 8), (4, 8)]
    inside = [(0, 0), (10, 0), (4, 8), (4, 3)]
    trap = [(0, 0), (10, 0), (7, 4), (2, 4)]
    pts = np.array([tri, acute, acute[::-1], inside, inside[1:] + inside[:1], trap, trap[2:] + trap[:2]], np.float32) + np.float32(20)
    rows = A.xyxyxyxy2xywhr(engine, pts)
    _check_rows(rows, pts.astype(np.float64), lambda i: DIST_OP, "ties")
    assert rows.tobytes() == A.xyxyxyxy2xywhr(engine, pts).tobytes()                      # a pure function of the input
    assert len(R.candidates(pts[3])) == 3 and len(R.candidates(pts[5])) == 4


@pytest.mark.parametrize("backend", BACKENDS)
def test_operator_degenerate(backend, engine):
    """Collinear points: h == 0, w = the span, the angle = the line's direction in (0, pi]; identical points: (x, y, 0, 0, 0).  Centres are exact."""
    from yolosharp_amd import augment as A
    pts = np.array([[(0, 0), (1, 2), (2, 4), (3, 6)],             # first quadrant
                    [(0, 6), (1, 4), (2, 2), (3, 0)],             # second quadrant
                    [(0, 3), (9, 3), (2, 3), (4, 3)],             # horizontal
                    [(64, 1), (64, 9), (64, 9), (64, 30)],        # on a border
                    [(1, 1), (1, 1), (5, 4), (5, 4)],             # two distinct points
                    [(5, 7), (5, 7), (5, 7), (5, 7)]], np.float32)
    rows = A.xyxyxyxy2xywhr(engine, pts)
    assert np.all(np.isfinite(rows))
    span = np.array([math.sqrt(45.0), math.sqrt(45.0), 9, 29, 5], np.float32)
    assert np.array_equal(rows[:5, 2], span) and not rows[:5, 3].any(), rows
    assert np.array_equal(rows[:, :2], np.array([(1.5, 3), (1.5, 3), (4.5, 3), (64, 15.5), (3, 2.5), (5, 7)], np.float32)), rows
    assert np.all(rows[:5, 4] > 0) and np.all(rows[:5, 4] <= np.float32(np.pi)) and rows[2, 4] == np.float32(np.pi) and rows[3, 4] == HALF_PI
    assert abs(float(rows[0, 4]) - math.atan2(2, 1)) < 1e-6 and abs(float(rows[1, 4]) - math.atan2(2, -1)) < 1e-6 and abs(float(rows[4, 4]) - math.atan2(3, 4)) < 1e-6
    _check_rows(rows, pts.astype(np.float64), lambda i: DIST_OP, "degenerate")        # and each row describes the segment it encloses
    assert not rows[5, 2:].any()


# ---------------------------------------------------------------------------------------------------- 5: Mosaic label parity
def _collinear_case():
    """A label whose axis-aligned box is kept while every clipped corner lies on the border x = s: a thin rectangle along the diagonal of its
    box, and a matrix that turns the box: the turned box's own box reaches into the image, the label's corners do not."""
    src = [2, 2, 2, 2]
    a = 20.0
    d = np.array([[10, 48], [12, 50], [32, 30], [30, 28]], np.float32)        # a thin rectangle along the diagonal of its box that the turn does NOT push outward
    assert np.allclose([d[:, 0].min(), d[:, 1].min(), d[:, 0].max(), d[:, 1].max()], [10, 28, 32, 50])
    M0 = _matrix(S, angle=a, scale=1.0, trans=(0.5, 0.5))
    xc = yc = S                                                   # tile 3 of a 64 x 64 source: pad (64, 64)
    pts = (d.astype(np.float64) + S) @ M0[:2, :2].astype(np.float64).T + M0[:2, 2].astype(np.float64)
    M = M0.copy()
    M[0, 2] += np.float32(S + 1.0 - pts[:, 0].min())              # the leftmost corner lands 1 px right of the image
    M[1, 2] += np.float32(S / 2 - pts[:, 1].mean())
    return src, xc, yc, M, d


@functools.lru_cache(maxsize=None)
def _mosaic_case(perspective):
    """Items, labels (decisions at least 1e-3 from their thresholds: the keep rule is fp32 in the kernel and float64 here) and the restatement."""
    p = (5e-4, -4e-4) if perspective else (0.0, 0.0)
    raw = _raw_labels(SHAPES, seed=3)
    csrc, cxc, cyc, cM, cobb = _collinear_case()
    raw[2] = dict(cls=np.concatenate([raw[2]["cls"], np.array([900.0], np.float32)]), obb=np.concatenate([raw[2]["obb"], cobb[None]]))
    items = [([0, 1, 2, 3], 40, 52, _matrix(S, angle=6.0, scale=0.8, persp=p, trans=(0.5, 0.48)), 0, 0),
             ([2, 3, 0, 4], 84, 70, _matrix(S, angle=-9.0, scale=0.9, persp=p, trans=(0.46, 0.53)), 1, 0),
             ([4, 5, 3, 1], 60, 60, _matrix(S, angle=3.0, scale=1.2, persp=p, trans=(0.55, 0.5)), 0, 1),
             ([1, 0, 5, 2], 50, 88, _matrix(S, angle=12.0, scale=0.75, persp=p, trans=(0.5, 0.52)), 1, 1),
             (csrc, cxc, cyc, cM, 0, 0)]
    from yolosharp_amd import augment as A
    boxes_of = [A._obb_boxes(l["obb"]) for l in raw]
    _, _, _, mg = _restate_mosaic(raw, boxes_of, items, SHAPES, perspective)
    ok = [np.ones(len(l["cls"]), bool) for l in raw]
    for (src, *_), m in zip(items, mg):
        near = ((m["ratio"].abs() < 1e-3) | ((m["area1"] > 0) & (m["area1"] < 1e-3)) | ((m["area2"] > 0) & (m["area2"] < 1e-3))).numpy()
        o = 0
        for k in src:
            n = len(raw[k]["cls"])
            ok[k] &= ~near[o:o + n]
            o += n
    assert sum(int(o.sum()) for o in ok) >= 0.9 * sum(len(o) for o in ok) and ok[2][-1]
    labels = [dict(cls=l["cls"][o], obb=l["obb"][o]) for l, o in zip(raw, ok)]
    boxes_of = [A._obb_boxes(l["obb"]) for l in labels]
    return items, labels, boxes_of, _restate_mosaic(labels, boxes_of, items, SHAPES, perspective)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("perspective", [0, 1])
def test_mosaic_label_parity(backend, engine, perspective):
    from yolosharp_amd import augment as A
    items, labels, boxes_of, (bi, cl, xy, mg) = _mosaic_case(perspective)
    n = len(cl)
    assert {int(b) for b in bi} == set(range(len(items))) and n >= 25
    # the data holds what the case is about: clipped corners, and the label whose clipped corners are all on x = s while its box is kept
    clipped = ((xy == 0) | (xy == S)).any(axis=(1, 2))
    assert clipped.sum() >= 5 and (~clipped).sum() >= 5
    k = int(np.flatnonzero((cl == 900.0) & (bi == 4))[-1])                      # its instance in tile 3 (the source fills all four tiles)
    assert np.all(xy[k][:, 0] == S) and len(R.hull(xy[k])) == 2
    _, srcs = A.pack_sources(_sources(SHAPES))
    lab_off, cls, boxes, kp = A.pack_labels(labels)
    assert kp is None and np.array_equal(boxes, np.concatenate(boxes_of))            # derived the way YoloDataset.cs:235-243 does
    corners = A.pack_obb(labels)
    it = _pack_items(items)
    cap = 4 * int(np.diff(lab_off).max()) * len(items) + 3
    out = A.augment_labels_obb(engine, srcs, lab_off, cls, boxes, corners, it, S, perspective, 0, cap)
    assert out["count"] == n and out["bboxes"].shape == (cap, 5)
    assert np.array_equal(out["batch_idx"][:n], bi) and np.array_equal(out["cls"][:n], cl)                 # kept set, order, image
    assert np.all(out["batch_idx"][n:] == -1) and not out["cls"][n:].any() and not out["bboxes"][n:].any()
    # the same rows ys_augment_labels keeps for the same boxes
    box = A.augment_labels(engine, srcs, lab_off, cls, boxes, None, it, S, perspective, 0, cap)
    assert box["count"] == n and np.array_equal(box["batch_idx"], out["batch_idx"]) and np.array_equal(box["cls"], out["cls"])
    _check_rows(_to_pixels(out["bboxes"][:n]), xy, lambda i: _eta(xy[i], EPS_MOSAIC), "mosaic perspective=%d" % perspective)
    assert out["bboxes"][k, 3] == 0 and abs(out["bboxes"][k, 0] - 1.0) == 0 and out["bboxes"][k, 4] == HALF_PI       # the collinear row: on x = s
    again = A.augment_labels_obb(engine, srcs, lab_off, cls, boxes, corners, it, S, perspective, 0, cap)
    assert all(np.array_equal(out[key], again[key]) for key in ("batch_idx", "cls", "bboxes")) and again["count"] == n


# ---------------------------------------------------------------------------------------------------- 6: LetterBox label parity
@pytest.mark.parametrize("backend", BACKENDS)
def test_letterbox_label_parity(backend, engine):
    """Every label kept, in order; pads not scaled by ratio (sources with ratio != 1 among them); corners outside [0, s] are left where they are."""
    from yolosharp_amd import augment as A
    shapes = [(64, 48), (40, 64), (33, 48), (96, 80), (64, 64)]            # ratio 1, 1, 1.33.., 0.66.., 1
    labels = _raw_labels(shapes, seed=8, per_source=5)
    lst = [(k, flr, fud) for k in range(len(shapes)) for flr, fud in ((0, 0), (1, 0), (0, 1), (1, 1))]
    it = A.make_items(len(lst))
    for b, (k, flr, fud) in enumerate(lst):
        it[b]["src"], it[b]["xc"], it[b]["yc"], it[b]["flip_lr"], it[b]["flip_ud"] = (k, -1, 10 ** 6, -7), -3, 10 ** 6, flr, fud
    bi, cl, xy = [], [], []
    for b, (k, flr, fud) in enumerate(lst):
        _, _, pad_l, pad_u = LR.geometry(shapes[k][0], shapes[k][1], S)
        xy.append(R.letterbox_corners(labels[k]["obb"], pad_l, pad_u, S, flr, fud))
        bi.append(np.full(len(labels[k]["cls"]), float(b), np.float32)); cl.append(labels[k]["cls"])
    bi, cl, xy = np.concatenate(bi), np.concatenate(cl), np.concatenate(xy)
    assert LR.geometry(33, 48, S)[2:] == (0, 10) and LR.geometry(96, 80, S)[2:] == (5, 0)
    assert (xy > S).any() and (xy < 0).any()                               # unscaled pads and rectangles around the border: nothing is clipped
    _, srcs = A.pack_sources(_sources(shapes))
    lab_off, cls, boxes, _ = A.pack_labels(labels)
    cap = len(cl) + 5
    out = A.augment_letterbox_labels_obb(engine, srcs, lab_off, cls, boxes, A.pack_obb(labels), it, S, 0, cap)
    n = len(cl)
    assert out["count"] == n and np.array_equal(out["batch_idx"][:n], bi) and np.array_equal(out["cls"][:n], cl)
    assert np.all(out["batch_idx"][n:] == -1) and not out["cls"][n:].any() and not out["bboxes"][n:].any()
    rows = _to_pixels(out["bboxes"][:n])
    _check_rows(rows, xy, lambda i: _eta(xy[i], EPS_LETTERBOX), "letterbox")
    rebuilt = np.stack([R.row_corners(r) for r in rows])
    assert rebuilt.max() > S + 1 and rebuilt.min() < -1                    # the rows themselves reach outside the image


# ---------------------------------------------------------------------------------------------------- 7, 8: chunks, label-free
@pytest.mark.parametrize("backend", BACKENDS)
def test_more_than_one_chunk(backend, engine):
    """One image with more labels than the workgroup has threads (AUG_T = 256), both branches."""
    from yolosharp_amd import augment as A
    shapes = [(64, 64)] * 4
    g = np.random.default_rng(4)
    labels = [dict(cls=np.arange(150 * k, 150 * k + 150, dtype=np.float32), obb=_rot_rects(g, 150, 8, 56, 8, 56, 3.0, 12.0)) for k in range(4)]
    labels[1] = dict(cls=np.arange(1000, 1300, dtype=np.float32), obb=_rot_rects(g, 300, 8, 56, 8, 56, 3.0, 12.0))
    items = [([0, 1, 2, 3], 64, 64, _matrix(S, scale=0.5), 0, 0)]         # the whole canvas is visible: every label is kept
    boxes_of = [A._obb_boxes(l["obb"]) for l in labels]
    bi, cl, xy, mg = _restate_mosaic(labels, boxes_of, items, shapes, 0)
    m = mg[0]
    assert float(torch.minimum(m["ratio"].abs(), torch.where(m["area2"] > 0, m["area2"], torch.ones_like(m["area2"]))).min()) > 1e-4
    _, srcs = A.pack_sources(_sources(shapes))
    lab_off, cls, boxes, _ = A.pack_labels(labels)
    out = A.augment_labels_obb(engine, srcs, lab_off, cls, boxes, A.pack_obb(labels), _pack_items(items), S, 0, 0, 800)
    n = len(cl)
    assert n > 256 and out["count"] == n and np.array_equal(out["cls"][:n], cl) and np.all(out["batch_idx"][:n] == 0) and np.all(out["batch_idx"][n:] == -1)
    _check_rows(_to_pixels(out["bboxes"][:n]), xy, lambda i: _eta(xy[i], EPS_MOSAIC), "mosaic chunks")
    lb = A.augment_letterbox_labels_obb(engine, srcs, lab_off, cls, boxes, A.pack_obb(labels), _pack_items([([1, 0, 0, 0], 0, 0, np.eye(3), 1, 0)]), S, 0, 301)
    want = R.letterbox_corners(labels[1]["obb"], 0, 0, S, 1, 0)
    assert lb["count"] == 300 and np.array_equal(lb["cls"][:300], labels[1]["cls"]) and lb["batch_idx"][300] == -1 and not lb["bboxes"][300].any()
    _check_rows(_to_pixels(lb["bboxes"][:300]), want, lambda i: _eta(want[i], EPS_LETTERBOX), "letterbox chunks")


@pytest.mark.parametrize("backend", BACKENDS)
def test_label_free(backend, engine):
    """A label-free source beside others, and a batch without any label: tail rows are -1 / zeros, the count is 0."""
    from yolosharp_amd import augment as A
    shapes = [(64, 64)] * 4
    labels = _raw_labels(shapes, seed=2, per_source=3)
    labels[1] = dict(cls=np.zeros((0,), np.float32), obb=np.zeros((0, 4, 2), np.float32))
    _, srcs = A.pack_sources(_sources(shapes))
    lab_off, cls, boxes, _ = A.pack_labels(labels)
    corners = A.pack_obb(labels)
    M = _matrix(S, scale=0.5)                                             # the whole canvas is visible
    it = _pack_items([([1, 1, 1, 1], 64, 64, M, 0, 0), ([0, 1, 2, 3], 64, 64, M, 0, 0)])
    out = A.augment_labels_obb(engine, srcs, lab_off, cls, boxes, corners, it, S, 0, 0, 20)
    assert out["count"] == 9 and np.all(out["batch_idx"][:out["count"]] == 1) and np.all(out["batch_idx"][out["count"]:] == -1)
    lb = A.augment_letterbox_labels_obb(engine, srcs, lab_off, cls, boxes, corners, it, S, 0, 20)
    assert lb["count"] == 3 and np.array_equal(lb["batch_idx"][:3], [1, 1, 1]) and np.all(lb["batch_idx"][3:] == -1)
    empty = [dict(cls=np.zeros((0,), np.float32), obb=np.zeros((0, 4, 2), np.float32)) for _ in shapes]
    lab_off0, cls0, boxes0, _ = A.pack_labels(empty)
    for fn, extra in ((A.augment_labels_obb, (S, 0, 0, 6)), (A.augment_letterbox_labels_obb, (S, 0, 6))):
        o = fn(engine, srcs, lab_off0, np.zeros(1, np.float32), np.zeros((1, 4), np.float32), np.zeros((1, 4, 2), np.float32), it, *extra)
        assert o["count"] == 0 and np.all(o["batch_idx"] == -1) and not o["cls"].any() and not o["bboxes"].any() and boxes0.shape == (0, 4)


# ---------------------------------------------------------------------------------------------------- 9: pointers, refusals
@pytest.mark.parametrize("backend", BACKENDS)
def test_host_and_device_pointers_agree_and_refusals(backend, engine):
    from yolosharp_amd import YsError
    from yolosharp_amd import augment as A
    items, labels, _, _ = _mosaic_case(0)
    imgs = _sources(SHAPES)
    it = _pack_items(items)
    aug = A.MosaicAugmenter(engine, imgs, labels, S, degrees=5.0, seed=0, max_batch=len(items))
    _, srcs = A.pack_sources(imgs)
    lab_off, cls, boxes, _ = A.pack_labels(labels)
    corners = A.pack_obb(labels)
    for closed in (False, True):
        aug.close_mosaic(closed)
        dev = aug.run(it).to_host()
        host = (A.augment_letterbox_labels_obb(engine, srcs, lab_off, cls, boxes, corners, it, S, 0, aug.capacity) if closed else
                A.augment_labels_obb(engine, srcs, lab_off, cls, boxes, corners, it, S, 0, 0, aug.capacity))
        n = host["count"]
        assert n > 0 and dev["bboxes"].shape == (n, 5)
        assert all(dev[k].tobytes() == host[k][:n].tobytes() for k in ("batch_idx", "cls", "bboxes"))
    aug.close()
    one = it[:1]
    need = int(sum(lab_off[k + 1] - lab_off[k] for k in one["src"][0]))
    bad_src = one.copy(); bad_src["src"][0, 1] = -1
    for kw in (dict(flags=A.YS_AUG_SORT_FLIPPED), dict(flags=A.YS_AUG_FLIP_KEEP_SIZE), dict(capacity=need - 1), dict(items=bad_src)):
        with pytest.raises(YsError) as e:
            A.augment_labels_obb(engine, srcs, lab_off, cls, boxes, corners, kw.get("items", one), S, 0, kw.get("flags", 0), kw.get("capacity", need))
        assert e.value.status == 1, kw
    assert A.augment_labels_obb(engine, srcs, lab_off, cls, boxes, corners, one, S, 0, 0, need)["count"] <= need
    need = int(lab_off[one["src"][0, 0] + 1] - lab_off[one["src"][0, 0]])
    bad_src = one.copy(); bad_src["src"][0, 0] = len(SHAPES)
    for kw in (dict(flags=A.YS_AUG_SORT_FLIPPED), dict(flags=A.YS_AUG_FLIP_KEEP_SIZE), dict(capacity=need - 1), dict(items=bad_src)):
        with pytest.raises(YsError) as e:
            A.augment_letterbox_labels_obb(engine, srcs, lab_off, cls, boxes, corners, kw.get("items", one), S, kw.get("flags", 0), kw.get("capacity", need))
        assert e.value.status == 1, kw
    assert A.augment_letterbox_labels_obb(engine, srcs, lab_off, cls, boxes, corners, one, S, 0, need)["count"] == need


# ---------------------------------------------------------------------------------------------------- 10-12: augmenter, train step, trainer
def _tiny_dataset(seed, s, n=6):
    shapes = [(s, s), (s, s * 3 // 4), (s * 5 // 8, s), (s, s), (s * 7 // 8, s - 2), (s, s)][:n]
    g = np.random.default_rng(seed)
    labels = []
    for h, w in shapes:
        labels.append(dict(cls=g.integers(0, 5, 3).astype(np.float32), obb=_rot_rects(g, 3, 0.3 * w, 0.7 * w, 0.3 * h, 0.7 * h, 0.2 * s, 0.4 * s)))
    return shapes, _sources(shapes, seed), labels


@pytest.mark.parametrize("backend", BACKENDS)
def test_augmenter_with_obb_labels(backend, engine):
    from yolosharp_amd import augment as A
    shapes, imgs, labels = _tiny_dataset(2, S)
    aug = A.MosaicAugmenter(engine, imgs, labels, S, degrees=5.0, seed=3, max_batch=3)
    assert aug.obb and aug.box_dim == 5
    for closed in (False, True):
        aug.close_mosaic(closed)
        db = aug.batch([0, 1, 4])
        host = db.to_host()
        n = len(host["cls"])
        assert db.mode == ("letterbox" if closed else "mosaic") and db.box_dim == 5 and host["bboxes"].shape == (n, 5) and n > 0
        assert "keypoints" not in host and "masks" not in host and host["images"].shape == (3, 3, S, S)
        bb = host["bboxes"]
        assert np.all(bb[:, 4] > 0) and np.all(bb[bb[:, 3] > 0, 4] <= HALF_PI) and np.all(bb[:, 4] <= np.float32(np.pi))      # pi/2 < angle: collinear rows only
        if closed:
            assert n == 9 == db.n_input and np.all(host["bboxes"][:, 2:4] > 0)
    aug.close()
    with pytest.raises(ValueError):
        A.MosaicAugmenter(engine, imgs, labels, S, flags=A.YS_AUG_SORT_FLIPPED)
    with pytest.raises(ValueError):
        A.MosaicAugmenter(engine, imgs, labels, S, masks=[np.ones((h // 4, w // 4), np.uint8) for h, w in shapes])
    with pytest.raises(ValueError):
        A.MosaicAugmenter(engine, imgs, [dict(l, keypoints=np.zeros((3, 2, 3), np.float32)) for l in labels], S)
    # a plain box dataset still gives 4-column batches
    plain = A.MosaicAugmenter(engine, imgs, [dict(cls=l["cls"], bboxes=A._obb_boxes(l["obb"])) for l in labels], S, seed=3, max_batch=2)
    assert not plain.obb and plain.batch([0, 1]).to_host()["bboxes"].shape[1] == 4
    plain.close()


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("closed", [False, True])
def test_train_step_on_obb_batch(backend, engine, closed):
    """TrainStepDevice on an OBB DeviceBatch returns the same loss items, bit for bit (the comparison test_train_step_on_letterbox_batch makes), as
    TrainStep on its to_host(); a Detect model refuses the 5-column batch, an OBB model a 4-column one."""
    from yolosharp_amd import augment as A
    from yolosharp_amd import model as M
    shapes, imgs, labels = _tiny_dataset(2, S)
    aug = A.MosaicAugmenter(engine, imgs, labels, S, degrees=5.0, seed=3, max_batch=2)
    aug.close_mosaic(closed)
    db = aug.batch([1, 4])
    host = db.to_host()
    assert 0 < len(host["cls"]) < db.capacity and host["bboxes"].shape[1] == 5
    got = []
    for device in (True, False):
        m = M.Yolov8Obb(engine, nc=5, size="n", height=S, width=S, max_batch=2, dtype="f32")
        m.init_weights(1)
        amp = M.AMPWrapper(m)
        _, it = amp.TrainStepDevice(db, M.v8OBBLoss(m)) if device else amp.TrainStep(host["images"], host, M.v8OBBLoss(m))
        got.append(it)
        m.close()
    assert got[0].shape == (4,) and np.all(np.isfinite(got[0])) and got[0][0] > 0
    assert np.array_equal(got[0], got[1]), got
    if not closed:
        det = M.Yolov8(engine, nc=5, size="n", height=S, width=S, max_batch=2, dtype="f32")
        det.init_weights(1)
        with pytest.raises(ValueError):
            M.AMPWrapper(det).TrainStepDevice(db, M.v8DetectionLoss(det))
        det.close()
        plain = A.MosaicAugmenter(engine, imgs, [dict(cls=l["cls"], bboxes=A._obb_boxes(l["obb"])) for l in labels], S, seed=3, max_batch=2)
        obb = M.Yolov8Obb(engine, nc=5, size="n", height=S, width=S, max_batch=2, dtype="f32")
        obb.init_weights(1)
        with pytest.raises(ValueError):
            M.AMPWrapper(obb).TrainStepDevice(plain.batch([1, 4]), M.v8OBBLoss(obb))
        obb.close(); plain.close()
    aug.close()


@pytest.mark.parametrize("backend", BACKENDS)
def test_trainer_fit_end2end_obb(backend, engine):
    """Trainer.fit on the tiny dataset with an End2End OBB model, the augmenter and close_mosaic = 1: it runs, the mode switches, and the gain
    schedule is stepped once per epoch."""
    from yolosharp_amd import augment as A
    from yolosharp_amd import model as M
    from yolosharp_amd import trainer as T
    s = 32
    _, imgs, labels = _tiny_dataset(5, s)
    aug = A.MosaicAugmenter(engine, imgs, labels, s, degrees=5.0, seed=9, max_batch=2)
    m = M.Yolov8Obb(engine, nc=5, size="n", height=s, width=s, max_batch=2, dtype="f32")
    m.e2e_obb_init(max_det=20, epochs=2)
    m.init_weights(1)
    modes, updates, gains0 = [], [], m.e2e_gains()
    update = m.e2e_update
    m.e2e_update = lambda: (updates.append(1), update())[1]

    def train_batches():
        epoch = []
        modes.append(epoch)
        for idx in ([0, 1], [2, 3]):
            db = aug.batch(idx)
            epoch.append(db.mode)
            yield db
    hist = T.Trainer(m, epochs=2, nb=2, lr0=2e-3, warmup_bias_lr=2e-3).fit(train_batches, augmenter=aug, close_mosaic=1)
    assert modes == [["mosaic", "mosaic"], ["letterbox", "letterbox"]]
    assert len(hist) == 2 and all(h["train_loss"].shape == (4,) and np.all(np.isfinite(h["train_loss"])) and h["train_loss"][1] > 0 for h in hist)
    assert len(updates) == 2 and m.e2e_gains() != gains0
    del m.e2e_update
    m.close(); aug.close()
