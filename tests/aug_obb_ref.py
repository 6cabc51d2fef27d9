"""Float64 restatement of the OBB corner labels of the training input, written independently of csrc/augment.hip: the corner chain of the two
branches (Data/Augment.cs:227-256, 604-635, 746-749, 825-828, 908-911, 958-961; Utils/Ops.cs:191-199) and xyxyxyxy2xywhr (Utils/Ops.cs:44-54, OpenCV
MinAreaRect) as a rectangle built from an EXPLICIT convex hull: every hull edge is a candidate, and ALL candidates are returned with their areas.
The kernel searches the 6 point pairs instead; a test that finds its rectangle among these candidates also checks that argument.

OpenCV is not available here: which of several rectangles of equal area MinAreaRect returns is not restated (nobody can pin it), so the tests accept
any candidate whose area is within the rounding of the minimum."""
import math

import numpy as np

import aug_ref


# ---------------------------------------------------------------------------------------------------- the rectangle
def _cross(o, a, b):
    return (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0])


def hull(points):
    """Andrew's monotone chain on the distinct points, collinear points dropped: the hull's vertices in counter-clockwise order (1 point, 2 points
    for a segment, else >= 3)."""
    pts = sorted(set((float(x), float(y)) for x, y in np.asarray(points, np.float64).reshape(-1, 2)))
    if len(pts) <= 2:
        return [np.array(p) for p in pts]
    lower, upper = [], []
    for p in pts:
        while len(lower) >= 2 and _cross(lower[-2], lower[-1], p) <= 0:
            lower.pop()
        lower.append(p)
    for p in reversed(pts):
        while len(upper) >= 2 and _cross(upper[-2], upper[-1], p) <= 0:
            upper.pop()
        upper.append(p)
    return [np.array(p) for p in lower[:-1] + upper[:-1]]


def candidates(points):
    """Every enclosing rectangle with a side on a hull edge: a list of (corners [4, 2] in order around the rectangle, area, the two side lengths).
    A single point gives one rectangle of four equal corners, a segment (collinear input) the rectangle (a, b, b, a) of area 0."""
    h = hull(points)
    if len(h) == 1:
        return [(np.stack([h[0]] * 4), 0.0, (0.0, 0.0))]
    if len(h) == 2:
        return [(np.stack([h[0], h[1], h[1], h[0]]), 0.0, (float(np.linalg.norm(h[1] - h[0])), 0.0))]
    P = np.stack(h)
    out = []
    for i in range(len(h)):
        d = h[(i + 1) % len(h)] - h[i]
        u = d / np.linalg.norm(d)
        n = np.array([-u[1], u[0]])
        t, m = P @ u, P @ n
        corners = np.stack([t.min() * u + m.min() * n, t.max() * u + m.min() * n, t.max() * u + m.max() * n, t.min() * u + m.max() * n])
        a, b = float(t.max() - t.min()), float(m.max() - m.min())
        out.append((corners, a * b, (a, b)))
    return out


def row_corners(row):
    """(cx, cy, w, h, angle) -> corners [4, 2] in order around the rectangle: w lies along (cos angle, sin angle)."""
    cx, cy, w, h, a = (float(v) for v in row)
    u, n = np.array([math.cos(a), math.sin(a)]), np.array([-math.sin(a), math.cos(a)])
    c = np.array([cx, cy])
    return np.stack([c - w / 2 * u - h / 2 * n, c + w / 2 * u - h / 2 * n, c + w / 2 * u + h / 2 * n, c - w / 2 * u + h / 2 * n])


def corner_set_distance(A, B):
    """Largest corner distance between two rectangles given as corners in order, minimised over the 4 starting corners and both orientations."""
    best = float("inf")
    for Bo in (B, B[::-1]):
        for k in range(4):
            best = min(best, float(np.linalg.norm(A - np.roll(Bo, k, axis=0), axis=1).max()))
    return best


def outside_distance(row, points):
    """How far the farthest of `points` lies outside the rectangle of `row` (0: all enclosed)."""
    cx, cy, w, h, a = (float(v) for v in row)
    u, n = np.array([math.cos(a), math.sin(a)]), np.array([-math.sin(a), math.cos(a)])
    q = np.asarray(points, np.float64).reshape(-1, 2) - np.array([cx, cy])
    return float(max(0.0, (np.abs(q @ u) - w / 2).max(), (np.abs(q @ n) - h / 2).max()))


# ---------------------------------------------------------------------------------------------------- the corner chains
def mosaic_corners(corners, padw, padh, M, s, perspective, flip_lr, flip_ud):
    """_mosaic4's + (padw, padh) without a clip (:253-256), apply_obb_corners ((x, y, 1) . M^T, divided only when perspective > 0, :604-635),
    clip_obb_corners (clamp to [0, s]), FlipLR x <- s - x, FlipUD y <- s - y: fp32 tables in, float64 [n, 4, 2] pixels out."""
    c = np.asarray(corners, np.float32).reshape(-1, 4, 2).astype(np.float64) + np.array([padw, padh], np.float64)
    M = np.asarray(M, np.float32).reshape(3, 3).astype(np.float64)
    hom = np.concatenate([c, np.ones(c.shape[:2] + (1,))], 2) @ M.T
    xy = hom[..., :2] / hom[..., 2:3] if perspective else hom[..., :2]
    xy = np.clip(xy, 0.0, float(s))
    if flip_lr:
        xy[..., 0] = s - xy[..., 0]
    if flip_ud:
        xy[..., 1] = s - xy[..., 1]
    return xy


def letterbox_corners(corners, pad_l, pad_u, s, flip_lr, flip_ud):
    """LetterBox's + (pad_l, pad_u), not scaled by ratio and not clipped (:746-749), then the flips (:825-828)."""
    xy = np.asarray(corners, np.float32).reshape(-1, 4, 2).astype(np.float64) + np.array([pad_l, pad_u], np.float64)
    if flip_lr:
        xy[..., 0] = s - xy[..., 0]
    if flip_ud:
        xy[..., 1] = s - xy[..., 1]
    return xy


def mosaic_sample(tiles, pads, M, flip_lr, flip_ud, s, perspective):
    """One Mosaic image: tiles = four dicts {cls, boxes [n, 4] pixel xyxy, obb [n, 4, 2]}.  The keep decision is aug_ref.labels_sample's -- the
    axis-aligned boxes ALONE, in float64 -- and the kept labels' corners go through mosaic_corners.  -> (cls [k], corners [k, 4, 2] pixels, margins)."""
    _, margins = aug_ref.labels_sample([dict(cls=t["cls"], boxes=t["boxes"], kpts=None) for t in tiles], pads, M, flip_lr, flip_ud, s, perspective,
                                       __import__("torch").float64)
    good = margins["good"].numpy()
    cls = np.concatenate([np.asarray(t["cls"], np.float32).reshape(-1) for t in tiles])
    xy = np.concatenate([mosaic_corners(t["obb"], pw, ph, M, s, perspective, flip_lr, flip_ud) for t, (pw, ph) in zip(tiles, pads)])
    return cls[good], xy[good], margins
