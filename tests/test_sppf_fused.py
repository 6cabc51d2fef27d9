"""SPPF's three chained 5x5 max-pools in one launch (elementwise.hip sppf_pool3_fwd_kernel / sppf_pool3_bwd_kernel, SPPF_FUSE=1) against the three
maxpool5 launches (SPPF_FUSE=0) on the standalone SPPF block: the statement is BIT-IDENTITY -- max is exact, the argmax rule (first maximum in (kh, kw)
scan order, strict '>', clipped window) and the backward's rounding points (fp32 tap sum in scan order + old value, one rounding per stage) are kept.

The block API exposes the block output, the input gradient and the parameter gradients, not the concat buffer: the three pool outputs are compared
through cv2 (its weights are random, so a differing pool output changes the block output), the argmax planes through the gradients (a gradient routed
to a different tap changes dx and cv1's weight gradient).  The inputs are tie-heavy on purpose: x and cv1's weights are small integers, so cv1's
pre-BN output takes at most five values per channel and the BatchNorm output (an affine map per channel, then one rounding to bf16) as few -- every
5x5 window holds several equal maxima and the choice among them is what the comparison pins.

The fused kernels are templated on the storage type (a workgroup owns four 16-byte units per pixel: 32 bf16 or 16 f32 channels), so f32 gets the same
identity check, and -- independent of the project's own pool kernels -- a comparison of the f32 block against a float64 restatement built on
torch.nn.functional.max_pool2d chained three times, on tie-free random inputs, at the tolerance tests/test_blocks.py uses for its f32 SPPF case.

The gate of the fused form (elementwise.hip ys_sppf_pool3_ok): a map of at most 400 pixels (20 x 20: map + row maxima + codes fill 57.6 KB of LDS).
Larger maps run the three launches whatever the switch says; the kernel profile's launch count of class "sppf_pool3" shows which form ran."""
import numpy as np
import pytest

from conftest import BACKENDS

# (H, W, c1): c_ = c1 / 2 hidden channels; a workgroup owns 32 of them
SHAPES = [
    (20, 20, 64),      # the production map, one chunk
    (5, 7, 64),        # every window clipped on two sides
    (3, 3, 64),        # map smaller than the window
    (13, 9, 80),       # c_ = 40: a full chunk and a one-unit chunk
    (6, 5, 96),        # c_ = 48: a full chunk and a two-unit chunk
]
# f32: a workgroup owns 16 channels
SHAPES_F32 = [
    (20, 20, 32),      # one chunk
    (5, 7, 32),
    (3, 3, 32),
    (13, 9, 40),       # c_ = 20: a full chunk and a one-unit chunk
    (6, 5, 48),        # c_ = 24: a full chunk and a two-unit chunk
]
F32_TOL = 1e-3         # tests/test_blocks.py test_block_parity_f32_emu / _gpu: _block_parity(..., "f32", B, 1e-3, 1e-3), which holds its "sppf" case
B = 2


def _tie_weight(c1, seed=7):
    """cv1 weights with two +-1 entries per output channel: on inputs from {-1, 0, 1} the pre-BN output takes at most five values per channel."""
    rng = np.random.default_rng(seed)
    w = np.zeros((c1 // 2, c1, 1, 1), np.float32)
    for o in range(c1 // 2):
        w[o, rng.choice(c1, 2, replace=False), 0, 0] = rng.choice([-1.0, 1.0], 2)
    return w


def _make(engine, c1, H, W, dtype, fuse, seed=7):
    from yolosharp_amd.blocks import SPPF
    with engine.options(SPPF_FUSE=fuse):           # read when the block is created
        blk = SPPF(engine, c1, c1, height=H, width=W, max_batch=B, dtype=dtype)
    blk.init_weights(seed)
    sd = blk.state_dict()
    sd["cv1.conv.weight"] = _tie_weight(c1, seed).reshape(sd["cv1.conv.weight"].shape)
    blk.load_state_dict(sd)
    return blk


def _inputs(c1, H, W, ties):
    rng = np.random.default_rng(3)
    x = rng.integers(-1, 2, (B, c1, H, W)).astype(np.float32) if ties else rng.standard_normal((B, c1, H, W), dtype=np.float32)
    dy = rng.standard_normal((B, c1, H, W), dtype=np.float32)
    return x, dy


def _run(engine, c1, H, W, dtype, fuse, ties=True):
    """-> train-mode output, dx, parameter gradients, eval-mode output, launches of the fused class (train forward + backward + eval forward)."""
    blk = _make(engine, c1, H, W, dtype, fuse)
    x, dy = _inputs(c1, H, W, ties)
    engine.kernel_profile(True)
    blk.train()
    y = blk.forward(x)
    blk.zero_grad()
    dx = blk.backward(dy)
    g = blk.grads()
    blk.eval()
    ye = blk.forward(x)
    n = engine.kernel_profile_read("sppf_pool3")[0]
    engine.kernel_profile(False)
    blk.close()
    return y, dx, g, ye, n


def _same(a, b):
    ya, dxa, ga, yea, _ = a
    yb, dxb, gb, yeb, _ = b
    assert np.isfinite(ya).all() and np.isfinite(dxa).all()
    assert np.array_equal(ya, yb), "train-mode block output (the three pool outputs through cv2)"
    assert np.array_equal(dxa, dxb), "input gradient (the argmax planes and the backward's rounding points)"
    assert sorted(ga) == sorted(gb)
    for k in ga:
        assert np.array_equal(ga[k], gb[k]), k
    assert np.array_equal(yea, yeb), "eval-mode block output (no argmax planes)"


def _distinct_values(c1, H, W):
    """Distinct pre-BN values per channel of cv1 on the tie-heavy input (host arithmetic on the same integers)."""
    x, _ = _inputs(c1, H, W, True)
    y = np.einsum("oc,bchw->bohw", _tie_weight(c1)[:, :, 0, 0], x)
    return max(len(np.unique(y[:, o])) for o in range(y.shape[1]))


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d_c%d" % s)
def test_fused_pools_equal_three_launches_bf16(engine, backend, shape):
    H, W, c1 = shape
    fused = _run(engine, c1, H, W, "bf16", 1)
    plain = _run(engine, c1, H, W, "bf16", 0)
    assert fused[4] == 3, "fused form: one launch per train forward, backward and eval forward"
    assert plain[4] == 0
    _same(fused, plain)
    assert _distinct_values(c1, H, W) <= 5, "the input is meant to be tie-heavy"


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("shape", SHAPES_F32, ids=lambda s: "%dx%d_c%d" % s)
def test_fused_pools_equal_three_launches_f32(engine, backend, shape):
    H, W, c1 = shape
    fused = _run(engine, c1, H, W, "f32", 1)
    plain = _run(engine, c1, H, W, "f32", 0)
    assert fused[4] == 3 and plain[4] == 0
    _same(fused, plain)
    assert _distinct_values(c1, H, W) <= 5, "the input is meant to be tie-heavy"


def _sppf_float64(sd, x, dy):
    """The SPPF block in float64 from its state_dict: cv1 = 1x1 conv + train-mode BatchNorm (eps 1e-3), torch.nn.functional.max_pool2d(5, 1, 2) chained three
    times, concat, cv2 = 1x1 conv + BatchNorm + SiLU.  -> y, dx, parameter gradients."""
    import torch
    import torch.nn.functional as F
    p = {k: torch.tensor(np.asarray(v), dtype=torch.float64).requires_grad_(True) for k, v in sd.items() if k.endswith(("conv.weight", "bn.weight", "bn.bias"))}
    xt = torch.tensor(x, dtype=torch.float64).requires_grad_(True)

    def unit(t, name, act):
        t = F.conv2d(t, p[name + ".conv.weight"])
        t = F.batch_norm(t, None, None, p[name + ".bn.weight"], p[name + ".bn.bias"], training=True, eps=1e-3)
        return F.silu(t) if act else t
    ys = [unit(xt, "cv1", False)]
    for _ in range(3):
        ys.append(F.max_pool2d(ys[-1], 5, 1, 2))
    y = unit(torch.cat(ys, 1), "cv2", True)
    y.backward(torch.tensor(dy, dtype=torch.float64))
    return y.detach().numpy(), xt.grad.numpy(), {k: v.grad.numpy() for k, v in p.items()}


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("shape", [(20, 20, 32), (13, 9, 40)], ids=lambda s: "%dx%d_c%d" % s)
def test_fused_pools_f32_against_float64_max_pool2d(engine, backend, shape):
    """The reference here owes nothing to the project's kernels: float64 torch, max_pool2d three times, tie-free inputs (normal x, random weights)."""
    from test_model import relerr
    from yolosharp_amd.blocks import SPPF
    H, W, c1 = shape
    with engine.options(SPPF_FUSE=1):
        blk = SPPF(engine, c1, c1, height=H, width=W, max_batch=B, dtype="f32")
    blk.init_weights(7)
    x, dy = _inputs(c1, H, W, ties=False)
    engine.kernel_profile(True)
    blk.train()
    sd = blk.state_dict()                          # before the forward moves the running statistics (not used by the reference anyway)
    y = blk.forward(x)
    blk.zero_grad()
    dx = blk.backward(dy)
    g = blk.grads()
    assert engine.kernel_profile_read("sppf_pool3")[0] == 2, "the fused kernels must be what is compared"
    engine.kernel_profile(False)
    blk.close()
    ry, rdx, rg = _sppf_float64(sd, x, dy)
    assert relerr(y, ry) < F32_TOL
    assert relerr(dx, rdx) < F32_TOL
    # parameter gradients as tests/test_blocks.py compares them: analytically-zero ones (cv1.bn.bias: a per-channel shift commutes with the max pools and is
    # removed by cv2's batch statistics) on the scale of the largest gradient, not of their own rounding noise
    gmax = max(float(np.abs(v).max()) for v in rg.values())
    assert sorted(rg) == sorted(g)
    for k in rg:
        err = float(np.abs(g[k] - rg[k]).max() / max(float(np.abs(rg[k]).max()), 1e-3 * gmax))
        assert err < F32_TOL, (k, err)


@pytest.mark.parametrize("backend", BACKENDS)
def test_fused_pools_equal_three_launches_random_input(engine, backend):
    """Tie-poor input (normal x): the common case, 13 x 9 with a short last chunk."""
    fused = _run(engine, 80, 13, 9, "bf16", 1, ties=False)
    plain = _run(engine, 80, 13, 9, "bf16", 0, ties=False)
    assert fused[4] == 3 and plain[4] == 0
    _same(fused, plain)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("case", ["bf16_21x20", "f32_21x20"])
def test_fallback_runs_the_three_launches(engine, backend, case):
    """Outside the gate the switch changes nothing: a 21 x 20 map (420 pixels > the 400 of the LDS plan; the 40 x 40 maps of the 1280 x 1280
    configurations are the production instance) runs maxpool5_fwd_kernel / maxpool5_bwd_kernel three times each, in either storage type."""
    H, W, c1, dtype = (21, 20, 64, "bf16") if case == "bf16_21x20" else (21, 20, 32, "f32")
    on = _run(engine, c1, H, W, dtype, 1)
    off = _run(engine, c1, H, W, dtype, 0)
    assert on[4] == 0 and off[4] == 0
    _same(on, off)
