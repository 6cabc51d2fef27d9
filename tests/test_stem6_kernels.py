"""The 6x6 stem kernels of Yolov5u's model.0 = Conv(3, Cout, k 6, s 2, p 2) (csrc/conv_stem6.hip) on their own, against float64.

ys_stem6_fwd / ys_stem6_wgrad run exactly the kernels a bf16 Yolov5u model runs for model.0.  x, w and dy are rounded to bf16 first, so the float64
reference sees the operands the kernels see and every bound below is a statement about the kernels' own arithmetic:

  forward, training   |y - y64| <= 2^-8 |y64| + 108 * 2^-24 * sum_k |x_k w_k|            one bf16 rounding + fp32 accumulation over K = 108
  statistics (rows)   |S - S64(returned y)| <= M * 2^-24 * sum |y| (sum |y|^2 for the squares), M = B * Hout * Wout values per channel
  statistics (fixed)  the same fp32 sums inside a workgroup, then every workgroup's partial rounded to the accumulators' resolution 2^-20:
                      + rows * 2^-21, rows = the number of workgroups = tiles (<= 2048)
  forward, eval       z = SiLU(scale * y + shift):  1.1 * (|scale| * E_y + 2^-22 (|scale * y64| + |shift|)) + 2^-8 |z64|, E_y the training bound
                      (|SiLU'| <= 1.1; the kernel applies scale / shift to the bf16-rounded y, which E_y contains; the last term is the output rounding)
  weight gradient     |dW - dW64| <= M * 2^-24 * sum_pixels |dy * x|

Nothing is sampled: every element of every output is compared.  A wrong tap, a missing halo column or a stale LDS entry moves an element by a whole term of
its sum -- orders of magnitude above these bounds.  Shapes (the tile is 8 x 32 output pixels): exact tiles; a ragged right tile over several images; W % 4 != 0
(the element-wise patch fetch instead of the 16-byte one) with both edges ragged; odd H (one bottom padding row instead of two).
"""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import BACKENDS
from yolosharp_amd import weights_bin as WB

GOLD = os.path.join(os.path.dirname(__file__), "golden")
SHAPES = [(2, 64, 64), (3, 96, 160), (1, 70, 70), (1, 65, 132)]
CASES = [(s, c) for s in SHAPES for c in (16, 48)] + [(SHAPES[0], 80)]
U = 2.0 ** -24


def bf16r(a):
    return WB.bf16_to_f32(WB.f32_to_bf16(np.ascontiguousarray(a, np.float32))).reshape(np.shape(a))


def real_stem_weights():
    with open(os.path.join(GOLD, "yolov5n_prefix.bin"), "rb") as f:
        name, _, a = next(iter(WB.iter_bin(f, limit=1)))
    assert name == "model.0.conv.weight" and a.shape == (16, 3, 6, 6)
    return np.asarray(a, np.float32)


_inputs = {}


def inputs(shape, cout):
    """x, w, dy (bf16 values) and the float64 references, computed once per case and left unchanged."""
    key = (shape, cout)
    if key not in _inputs:
        B, H, W = shape
        rng = np.random.default_rng(1000 * cout + H)
        x = bf16r(rng.random((B, 3, H, W), dtype=np.float32))
        w = real_stem_weights() if (cout == 16 and shape == SHAPES[0]) else 0.2 * rng.standard_normal((cout, 3, 6, 6), dtype=np.float32)
        w = bf16r(w)
        xd, wd = torch.from_numpy(x).double(), torch.from_numpy(w).double()
        y64 = F.conv2d(xd, wd, stride=2, padding=2)
        ya = F.conv2d(xd.abs(), wd.abs(), stride=2, padding=2)
        dy = bf16r(rng.standard_normal(tuple(y64.shape), dtype=np.float32))
        dyd = torch.from_numpy(dy).double()
        dw64 = torch.nn.grad.conv2d_weight(xd, wd.shape, dyd, stride=2, padding=2)
        dwa = torch.nn.grad.conv2d_weight(xd.abs(), wd.shape, dyd.abs(), stride=2, padding=2)
        _inputs[key] = dict(x=x, w=w, dy=dy, y64=y64.numpy(), ya=ya.numpy(), dw64=dw64.numpy(), dwa=dwa.numpy())
    return _inputs[key]


def fwd_bound(d):
    return 2.0 ** -8 * np.abs(d["y64"]) + 108 * U * d["ya"]


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("shape,cout", CASES)
def test_stem6_forward_training(engine, backend, shape, cout):
    d = inputs(shape, cout)
    B, H, W = shape
    Ho, Wo = (H - 2) // 2 + 1, (W - 2) // 2 + 1
    M = B * Ho * Wo
    rows = min(2048, B * -(-Ho // 8) * -(-Wo // 32))
    y0 = None
    for stat_mode in (0, 1):
        y, stats = engine.stem6_fwd(d["x"], d["w"], stat_mode=stat_mode)
        assert y.shape == d["y64"].shape and np.isfinite(y).all() and np.isfinite(stats).all()
        assert np.array_equal(bf16r(y), y)                       # the stored bf16 values
        err = np.abs(y.astype(np.float64) - d["y64"])
        assert (err <= fwd_bound(d)).all(), (stat_mode, float((err - fwd_bound(d)).max()))
        yd = y.astype(np.float64)
        s1, s2 = yd.sum((0, 2, 3)), (yd * yd).sum((0, 2, 3))
        b1, b2 = M * U * np.abs(yd).sum((0, 2, 3)), M * U * s2
        if stat_mode == 1:
            b1, b2 = b1 + rows * 2.0 ** -21, b2 + rows * 2.0 ** -21
        assert (np.abs(stats[0] - s1) <= b1).all(), (stat_mode, np.abs(stats[0] - s1).max(), b1.min())
        assert (np.abs(stats[1] - s2) <= b2).all(), (stat_mode, np.abs(stats[1] - s2).max(), b2.min())
        if y0 is not None:
            assert np.array_equal(y, y0)                         # the statistics form does not touch the output
        y0 = y


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("shape,cout", CASES)
def test_stem6_forward_eval(engine, backend, shape, cout):
    d = inputs(shape, cout)
    rng = np.random.default_rng(7)
    scale = (0.5 + rng.random(cout)).astype(np.float32) * np.where(rng.random(cout) < 0.25, -1, 1).astype(np.float32)
    shift = rng.standard_normal(cout).astype(np.float32)
    sc, sh = scale.astype(np.float64)[None, :, None, None], shift.astype(np.float64)[None, :, None, None]
    u64 = sc * d["y64"] + sh
    eu = np.abs(sc) * fwd_bound(d) + 2.0 ** -22 * (np.abs(sc * d["y64"]) + np.abs(sh))
    for act in (True, False):
        z, _ = engine.stem6_fwd(d["x"], d["w"], scale=scale, shift=shift, act=act)
        z64 = u64 / (1.0 + np.exp(-u64)) if act else u64
        bound = (1.1 if act else 1.0) * eu + 2.0 ** -8 * np.abs(z64) + 2.0 ** -22
        err = np.abs(z.astype(np.float64) - z64)
        assert np.isfinite(z).all() and (err <= bound).all(), (act, float((err - bound).max()))


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("shape,cout", CASES)
def test_stem6_weight_gradient(engine, backend, shape, cout):
    d = inputs(shape, cout)
    B, H, W = shape
    M = B * ((H - 2) // 2 + 1) * ((W - 2) // 2 + 1)
    dw = engine.stem6_wgrad(d["x"], d["dy"])
    again = engine.stem6_wgrad(d["x"], d["dy"])
    assert np.isfinite(dw).all()
    err, bound = np.abs(dw.astype(np.float64) - d["dw64"]), M * U * d["dwa"]
    assert (err <= bound).all(), float((err / np.maximum(bound, 1e-300)).max())
    assert np.array_equal(dw.view(np.uint32), again.view(np.uint32))          # run to run bit-identical (an LDS reuse without a barrier is not)


@pytest.mark.parametrize("backend", BACKENDS)
def test_stem6_refuses_other_shapes(engine, backend):
    x = np.zeros((1, 3, 32, 32), np.float32)
    for cout in (8, 24, 96):
        with pytest.raises(RuntimeError) as e:
            engine.stem6_fwd(x, np.zeros((cout, 3, 6, 6), np.float32))
        assert e.value.status == 4
        with pytest.raises(RuntimeError) as e:
            engine.stem6_wgrad(x, np.zeros((1, cout, 16, 16), np.float32))
        assert e.value.status == 4
