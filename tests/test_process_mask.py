"""Ops.process_mask (process_mask_kernel, csrc/segloss.hip) against the float64 product, crop and bilinear form, on both backends, with the decision rule of
tests/process_mask_cases.py: a pixel the crop zeroes, or whose reference magnitude exceeds 4x the fp32 oracle's own error, must match exactly; at most
1 % of a case may be undecided.  A cropped pixel is never rounding.

Geometries: the exact 4x scale (24x40 prototypes, 96x160 image, nm 32), non-integer ratios (25x37 prototypes, nm 5), a downscale (image 16x24).  Box
sets: inside the image; scaled x1 / y1 <= -1 and scaled x2 / y2 <= -1 (the truncating branch of the reference slices from the far edge there, Ops.cs:421-435);
x1 / y1 inside (-1, 0); past the right and bottom edges; fully outside; inverted, zero-area and whole-image boxes.  Both crop branches and both `upsample`
settings.  n = 0, 49 and 50 with the truncating branch: at 50 the broadcast form applies."""
import numpy as np
import pytest

import process_mask_cases as PM
from conftest import BACKENDS

_CASES = [(g, s) for g in PM.GEOMS for s in PM.SETS]
_SMALL = ((12, 20), (24, 40), 32)               # the geometry of the count cases: a 2x scale on a 12 x 20 prototype


def _premise(geom, boxset, c):
    """the box set does in this geometry what it is named for"""
    e = PM.scaled_edges(c)
    t = np.trunc(e)
    mh, mw = c["mh"], c["mw"]
    if boxset == "inside":
        assert (e >= 0).all() and (e[:, [0, 2]] <= mw).all() and (e[:, [1, 3]] <= mh).all()
    if boxset == "neg_x1y1":
        assert (t[:, 0] <= -1).any() and (t[:, 1] <= -1).any() and (t[:, 0] < -mw).any() and (t[:, 1] < -mh).any() and (t[:, 2:] > 0).all()
    if boxset == "neg_x2y2":
        assert (t[:, 2] <= -1).any() and (t[:, 3] <= -1).any() and (t[:, 2] < -mw).any() and (t[:, 3] < -mh).any() and (t[:, :2] >= 0).all()
    if boxset == "frac_neg":
        assert ((e[:, 0] > -1) & (e[:, 0] < 0)).any() and ((e[:, 1] > -1) & (e[:, 1] < 0)).any() and (e[:, :2] > -1).all()
    if boxset == "past_edge":
        assert (e[:, 2] > mw).any() and (e[:, 3] > mh).any() and (e >= 0).all()
    if boxset == "outside":
        assert ((e[:, 0] >= mw) | (e[:, 1] >= mh) | (e[:, 2] <= 0) | (e[:, 3] <= 0)).all()
        assert not PM.keep_mask(c, False).any()
    if boxset == "degenerate":
        assert (e[:, 2] < e[:, 0]).any() and (e[:, 3] < e[:, 1]).any() and ((e[:, 2] == e[:, 0]) & (e[:, 3] == e[:, 1])).any()
        assert PM.keep_mask(c, False)[-1].mean() > 0.9
    if boxset in ("neg_x1y1", "neg_x2y2"):         # where the slice semantics differ from a clamp, and from the broadcast form
        assert (PM.keep_mask(c, True) != PM.keep_mask(c, False)).any()


@pytest.mark.parametrize("geom,boxset", _CASES)
def test_reference_alone_is_decided(geom, boxset):
    """the cases themselves, on the CPU: the premise of every box set, at most 1 % of the reference's pixels undecided, and the fp32 oracle agrees with the
    reference on every decided pixel (its own crop follows the same slice semantics)"""
    c = PM.make_case(geom, boxset)
    _premise(geom, boxset, c)
    for upsample in (False, True):
        for cpu_crop in (False, True):
            want, decided, margin = PM.decide(c, upsample, cpu_crop)
            print("MEASURE %s-%s up %d crop %d margin %.3g undecided %.4f%%" % (geom, boxset, upsample, cpu_crop, margin, 100 * (1 - decided.mean())))
            assert 1 - decided.mean() <= 0.01
            o = PM.oracle32(c, upsample, cpu_crop) > 0
            assert not ((o != want) & decided).any()


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("cpu_crop", [False, True])
@pytest.mark.parametrize("upsample", [False, True])
@pytest.mark.parametrize("geom,boxset", _CASES)
def test_process_mask_cases(geom, boxset, upsample, cpu_crop, backend, engine):
    c = PM.make_case(geom, boxset)
    out = engine.process_mask(c["protos"].numpy(), c["coef"].numpy(), c["boxes"].numpy(), c["shape"], upsample=upsample, cpu_crop_branch=cpu_crop)
    PM.check(out, c, upsample, cpu_crop, "%s-%s-up%d-crop%d-%s" % (geom, boxset, upsample, cpu_crop, backend))


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("upsample", [False, True])
@pytest.mark.parametrize("n", [0, 49, 50])
def test_truncating_branch_counts(n, upsample, backend, engine):
    """the truncating branch holds for n < 50 only (Ops.cs:421): 49 rows of boxes with negative x2 / y2 follow the slices, 50 rows the broadcast form"""
    c = PM.make_case(_SMALL, "neg_x2y2", n=n)
    assert c["n"] == n
    if n:
        differs = (PM.keep_mask(c, True) != PM.keep_mask(c, False)).any()                 # against the broadcast form on the same rows
        assert differs == (n < 50)
    out = engine.process_mask(c["protos"].numpy(), c["coef"].numpy().reshape(n, c["nm"]), c["boxes"].numpy().reshape(n, 4), c["shape"], upsample=upsample,
                              cpu_crop_branch=True)
    PM.check(out, c, upsample, True, "count%d-up%d-%s" % (n, upsample, backend))
    if n == 50:                                    # and the flag changes nothing there
        assert np.array_equal(out, engine.process_mask(c["protos"].numpy(), c["coef"].numpy(), c["boxes"].numpy(), c["shape"], upsample=upsample))
