"""Cases, reference and decision rule for Ops.process_mask (process_mask_kernel, csrc/segloss.hip): tests/test_process_mask.py and
tests/test_segment.py::test_process_mask.

Reference (ref64): the float64 product coef @ protos, the crop, the bilinear form of F.interpolate(align_corners=False).  The crop bounds are a discrete
decision the reference takes in fp32 (box * fp32(mw / iw), then ToInt32 + slices, or x1 <= col < x2), so ref64 takes them from the same fp32 products:
  truncating branch (Ops.cs:421-435, n < 50 on the CPU): masks[0:y1] = masks[y2:] = masks[:, 0:x1] = masks[:, x2:] = 0 with the reference's slice
    semantics, stated here by numpy slices themselves: a negative bound counts from the far edge;
  broadcast form (Ops.cs:437-447): x1 <= col < x2 and y1 <= row < y2 on the floats.

Decision rule: a pixel is DECIDED when every prototype cell it reads (a bilinear tap whose weight the clamp at 0 makes exactly 0 is not read) is cropped (the reference value is exactly 0 from the crop: the mask is 0) or when
|reference| exceeds the case's margin = 4 x the worst |fp32 oracle - ref64| of that case (oracle/yolo_oracle.py's crop_mask + F.interpolate in float32).
Decided pixels must match exactly; undecided ones may number at most 1 % of a case (test_reference_alone_is_decided checks that on the CPU)."""
import numpy as np
import torch

from oracle import yolo_oracle as O

# geometry: prototype (mh, mw), image (ih, iw), nm
GEOMS = {
    "x4": ((24, 40), (96, 160), 32),          # the exact 4x scale
    "ratio": ((25, 37), (96, 160), 5),        # non-integer ratios, a coefficient count that is not 32
    "down": ((24, 40), (16, 24), 32),         # the image is smaller than the prototypes
}
# boxes xyxy in pixels of a 96 x 160 image (scaled to the geometry's image); at the 4x scale a coordinate v is cell v / 4
BOXES = {
    "neg_x1y1": [[-4, 10, 50, 40], [10, -8, 60, 40], [-30, -20, 100, 90], [-170, -110, 50, 40], [-7, -9, 150, 90]],   # scaled x1 / y1 <= -1 (one below -size)
    "neg_x2y2": [[10, 10, -8, 60], [10, 10, 60, -8], [10, 10, -400, 60], [20, 30, -9, -13], [10, 10, 60, -300]],      # scaled x2 / y2 <= -1
    "frac_neg": [[-2, -3, 50, 40], [-3.5, 10, 90, 70], [10, -1, 90, 70], [-0.5, -0.5, 159, 95]],                       # scaled x1 / y1 inside (-1, 0)
    "past_edge": [[100, 50, 200, 130], [150, 90, 161, 97], [5, 5, 1000, 50], [5, 5, 50, 1000]],
    "outside": [[170, 10, 200, 40], [10, 100, 50, 130], [-50, 10, -10, 40], [10, -60, 50, -30], [-90, -70, -10, -6]],
    "degenerate": [[60, 40, 20, 10], [60, 10, 20, 40], [30, 30, 30, 30], [30.5, 20, 30.5, 60], [0, 0, 160, 96]],       # inverted, zero area, the whole image
}
SETS = ["inside"] + list(BOXES)


def make_case(geom, boxset, seed=0, n=None):
    (mh, mw), (ih, iw), nm = GEOMS[geom] if isinstance(geom, str) else geom
    gkey = sorted(GEOMS).index(geom) if isinstance(geom, str) else 7
    g = torch.Generator().manual_seed(1000 * (1 + gkey) + 10 * SETS.index(boxset) + seed)
    if boxset == "inside":
        n = 7 if n is None else n
        xy = torch.rand(n, 2, generator=g) * torch.tensor([iw * 0.6, ih * 0.6])
        wh = torch.rand(n, 2, generator=g) * torch.tensor([iw * 0.4, ih * 0.4]) + 2.0
        boxes = torch.cat((xy, xy + wh), 1)
    else:
        boxes = torch.tensor(BOXES[boxset], dtype=torch.float32) * torch.tensor([iw / 160.0, ih / 96.0] * 2)
        if n is not None:                        # n rows: the set repeated, each repeat moved by a fraction of a pixel
            reps = max(1, -(-n // len(boxes)))
            boxes = torch.cat([boxes + 0.037 * k for k in range(reps)])[:n]
    n = boxes.shape[0]
    return {"protos": torch.randn(nm, mh, mw, generator=g), "coef": torch.randn(n, nm, generator=g), "boxes": boxes.float().contiguous(),
            "shape": (ih, iw), "n": n, "nm": nm, "mh": mh, "mw": mw}


def scaled_edges(c):
    """the box edges in prototype cells as the reference forms them: fp32 box * fp32(mw / iw)"""
    ih, iw = c["shape"]
    wr, hr = np.float32(c["mw"]) / np.float32(iw), np.float32(c["mh"]) / np.float32(ih)
    return c["boxes"].numpy().astype(np.float32) * np.array([wr, hr, wr, hr], np.float32)


def keep_mask(c, cpu_crop):
    """bool [n, mh, mw]: the prototype cells the crop keeps"""
    n, mh, mw = c["n"], c["mh"], c["mw"]
    e = scaled_edges(c)
    keep = np.ones((n, mh, mw), bool)
    if cpu_crop and n < 50:
        for i in range(n):
            x1, y1, x2, y2 = (int(v) for v in e[i].tolist())          # ToInt32: toward zero
            keep[i, 0:y1] = False
            keep[i, y2:] = False
            keep[i, :, 0:x1] = False
            keep[i, :, x2:] = False
        return keep
    col, row = np.arange(mw, dtype=np.float32)[None, None, :], np.arange(mh, dtype=np.float32)[None, :, None]
    x1, y1, x2, y2 = (e[:, k][:, None, None] for k in range(4))
    return (col >= x1) & (col < x2) & (row >= y1) & (row < y2)


def _taps(dst, src):
    """F.interpolate(bilinear, align_corners=False) along one axis: (i0, i1, weight of i1, clamped) per output index, float64; clamped: the source
    coordinate was negative and became 0, so the weight of i1 is exactly 0 in every precision and i1 is not read"""
    raw = (np.arange(dst) + 0.5) * (src / dst) - 0.5
    s = np.maximum(raw, 0.0)
    i0 = np.minimum(np.floor(s).astype(np.int64), src - 1)
    i1 = np.minimum(i0 + 1, src - 1)
    return i0, i1, s - i0, raw < -1e-6


def ref64(c, upsample, cpu_crop):
    """(values float64 [n, oh, ow], cropped bool: every cell the pixel reads is cropped)"""
    n, nm, mh, mw = c["n"], c["nm"], c["mh"], c["mw"]
    keep = keep_mask(c, cpu_crop)
    v = (c["coef"].double().numpy() @ c["protos"].double().numpy().reshape(nm, -1)).reshape(n, mh, mw) * keep
    if not upsample:
        return v, ~keep
    ih, iw = c["shape"]
    y0, y1, ly, cy = _taps(ih, mh)
    x0, x1, lx, cx = _taps(iw, mw)
    ly, lx, ny, nx = ly[None, :, None], lx[None, None, :], ~cy[None, :, None], ~cx[None, None, :]
    g = lambda a, yy, xx: a[:, yy][:, :, xx]
    out = (1 - ly) * ((1 - lx) * g(v, y0, x0) + lx * g(v, y0, x1)) + ly * ((1 - lx) * g(v, y1, x0) + lx * g(v, y1, x1))
    anyk = g(keep, y0, x0) | (g(keep, y0, x1) & nx) | (g(keep, y1, x0) & ny) | (g(keep, y1, x1) & nx & ny)
    return out, ~anyk


def oracle32(c, upsample, cpu_crop):
    """the fp32 oracle's values before its `> 0` (oracle.process_mask without the threshold)"""
    nm, mh, mw = c["nm"], c["mh"], c["mw"]
    ih, iw = c["shape"]
    masks = c["coef"].matmul(c["protos"].view(nm, -1)).view(-1, mh, mw)
    db = c["boxes"].clone()
    wr, hr = float(mw) / iw, float(mh) / ih
    db[..., 0] *= wr; db[..., 2] *= wr; db[..., 3] *= hr; db[..., 1] *= hr
    masks = O.crop_mask(masks, db, cpu_crop)
    if upsample:
        masks = torch.nn.functional.interpolate(masks[None], size=(ih, iw), mode="bilinear", align_corners=False)[0]
    return masks.double().numpy()


def decide(c, upsample, cpu_crop):
    """(want bool mask, decided bool, margin): the reference's mask and which of its pixels are decided"""
    v, cropped = ref64(c, upsample, cpu_crop)
    if c["n"] == 0:
        return v > 0, cropped, 0.0
    margin = 4.0 * float(np.abs(oracle32(c, upsample, cpu_crop) - v).max())
    decided = cropped | (np.abs(v) > margin)
    assert not (v[cropped] != 0).any()
    return v > 0, decided, margin


def check(out, c, upsample, cpu_crop, tag=""):
    """the rule on an engine result `out`: shape, every decided pixel exact, at most 1 % undecided"""
    want, decided, margin = decide(c, upsample, cpu_crop)
    assert out.shape == want.shape and out.dtype == bool, (tag, out.shape, want.shape)
    und = 1.0 - decided.mean() if decided.size else 0.0
    bad = (out != want) & decided
    print("MEASURE %s margin %.3g undecided %.4f%% mismatched decided %d undecided %d" % (tag, margin, 100 * und, int(bad.sum()), int(((out != want) & ~decided).sum())))
    assert und <= 0.01, (tag, und)
    assert not bad.any(), (tag, int(bad.sum()), np.argwhere(bad)[:6].tolist())
    assert not out[decided & ~want].any()
