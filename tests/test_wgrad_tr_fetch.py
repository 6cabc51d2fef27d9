"""conv_wgrad_tr_kernel's operand fetch (csrc/conv_wgrad.hip): every thread derives the records of its dy and patch units once -- byte offset from the tile's
origin, packed (row, column), LDS slot -- and a tile costs an add, two compares and a select per unit; the tile coordinates advance by the decoded grid stride.
The cases are the ones in which such a record can be wrong: tiles that hang over the image on either side, an image narrower than the narrowest tile, stride 2 on an
odd size (the patch window moves by two), channel tiles that are partly outside the layer, dy / x as channel-offset views of wider buffers (a C2f block), and
persistent workgroups that walk several tiles with a short last share (the carry of the incremental walk).  bf16, through ys_conv_bwd, against torch autograd on the
bf16-rounded operands with the bounds of tests/test_conv.py::test_conv_backward; every case runs twice and the gradients must be bit-identical.  Both backends: the
interpreter plans for the 256 compute units of the MI355X, so its launch labels (tile, grid) are the device's."""
import ctypes as C
import os
import re
import tempfile

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import BACKENDS
from bf16_ref import check_elem

# (B, Cin, H, W, Cout, k, s), share: None = any; "multi" = every workgroup walks more than one tile; "uneven" = and the last workgroup fewer than the others
CASES = [
    ((1, 16, 44, 44, 16, 3, 1), None),        # 15 x 16 tiles on 44 x 44: the last tile row and column hang over the image
    ((1, 32, 20, 20, 32, 3, 1), None),        # 20 x 20
    ((1, 64, 20, 20, 64, 3, 1), None),
    ((2, 16, 9, 3, 16, 3, 1), None),          # W = 3: narrower than the narrowest (4-wide) tile
    ((1, 16, 45, 45, 32, 3, 2), None),        # stride 2, odd input: 23 x 23 outputs, the last patch row / column is padding
    ((1, 48, 12, 12, 80, 3, 1), None),        # ragged channel tiles: 3 and 5 fragments
    ((1, 80, 12, 12, 80, 3, 1), None),        # five fragments on both sides
    ((2, 48, 13, 17, 80, 1, 1), None),        # 1x1 path: ragged tiles and channels
    ((1, 80, 20, 20, 80, 1, 1), None),
    ((1, 16, 44, 44, 16, 1, 1), None),
    ((2, 16, 7, 3, 16, 1, 1), None),          # 1x1, W = 3
    ((16, 16, 128, 128, 16, 3, 1), "multi"),  # 1024 tiles on at most 512 workgroups
    ((17, 16, 128, 128, 16, 3, 1), "uneven"),  # 1088 tiles, three per workgroup, the last one two
    ((16, 64, 40, 40, 64, 3, 1), "multi"),    # 160 tiles, two channel tiles share the chip
    ((26, 64, 40, 40, 64, 3, 1), "uneven"),   # 260 tiles on 87 workgroups
    ((22, 64, 80, 80, 64, 1, 1), "uneven"),   # 1x1 path: 1100 tiles on 367 workgroups
    ((27, 80, 24, 24, 112, 3, 1), "multi"),   # ragged channel tiles AND several tiles per workgroup (six channel tiles leave few workgroups per tile list)
]


def wgrad_labels(engine, fn):
    """fn() with the per-launch profile on -> the labels of its weight-gradient launches."""
    engine.kernel_profile(True)
    try:
        fn()
        engine.synchronize()
        fd, path = tempfile.mkstemp(suffix=".csv")
        os.close(fd)
        try:
            engine.kernel_profile_dump(path)
            lines = open(path).read().splitlines()[1:]
        finally:
            os.remove(path)
    finally:
        engine.kernel_profile(False)
    return [l.split(",")[1] for l in lines if l.startswith("conv_wgrad,")]


def tiles_and_grid(label, B, Ho, Wo):
    m = re.search(r" tile(\d+)x(\d+) grid(\d+)x(\d+) ", label)
    th, tw, gx = int(m.group(1)), int(m.group(2)), int(m.group(3))
    return B * -(-Ho // th) * -(-Wo // tw), gx


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c[0])))
def test_wgrad_tr_fetch(backend, engine, case):
    from yolosharp_amd import _lib
    (B, Cin, H, W, Cout, k, s), share = case
    g = torch.Generator().manual_seed(100 + B + Cin + H)
    x = (torch.randn(B, Cin, H, W, generator=g)).bfloat16().float()
    w = (torch.randn(Cout, Cin, k, k, generator=g) * 0.2).bfloat16().float()
    x.requires_grad_(True); w.requires_grad_(True)
    y = F.conv2d(x, w, None, stride=s, padding=k // 2)
    dy = torch.randn(y.shape, generator=g).bfloat16().float()
    y.backward(dy)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    xn, wn, dyn = x.detach().numpy().copy(), w.detach().numpy().copy(), dy.numpy().copy()
    runs = []

    def run():
        dx = np.zeros(x.shape, np.float32); dw = np.zeros(w.shape, np.float32)
        _lib.check(engine.lib, engine.lib.ys_conv_bwd(engine.ctx, 1, vp(xn), B, Cin, H, W, vp(wn), Cout, k, s, vp(dyn), vp(dx), vp(dw)))
        runs.append((dx, dw))

    labels = wgrad_labels(engine, run)
    assert len(labels) == 1 and labels[0].startswith("wgrad_tr k%d s%d cin%d cout%d " % (k, s, Cin, Cout)), labels
    tiles, gx = tiles_and_grid(labels[0], B, y.shape[2], y.shape[3])
    if share:                       # workgroup i walks tiles i, i + gx, ...: at least two each, and with "uneven" the last workgroups one fewer than the first
        assert tiles >= 2 * gx, (labels[0], tiles)
        if share == "uneven":
            assert tiles % gx != 0, (labels[0], tiles)
    run()
    (dx, dw), (dx2, dw2) = runs
    assert np.array_equal(dw, dw2) and np.array_equal(dx, dx2), "two runs in one process differ"
    check_elem(dx, x.grad.numpy(), "dgrad %s" % (case[0],))
    ref = w.grad.numpy()
    err = float(np.abs(dw - ref).max())
    print("wgrad %s: max |err| %.3g, bound %.3g (%s)" % (case[0], err, 1e-4 * float(np.abs(ref).max()), labels[0]))
    assert err <= 1e-4 * np.abs(ref).max()


@pytest.mark.parametrize("backend", BACKENDS)
def test_wgrad_tr_fetch_c2f_views(backend, engine):
    """Through a C2f block handle: the Bottleneck convolutions read x and dy as 16-channel views at a channel offset inside the 48- / 64-channel concatenation
    buffer (row pitch wider than the channel tile).  Parity as tests/test_blocks.py (rounding-matched oracle) at its 24 x 24 shape -- on the device the block's
    FORWARD is bit-identical to that oracle there, which other map sizes do not give (44 x 20: 7.7 % one-ulp flips against the 3 % cap, the same with the parent
    commit's library) -- then two backward passes of one forward: bit-identical gradients."""
    from test_blocks import _block_bf16_matched
    from yolosharp_amd import blocks
    B, H, W = 2, 24, 24
    labels = wgrad_labels(engine, lambda: _block_bf16_matched(engine, "c2f_sc", B, H, W))
    assert sum(l.startswith("wgrad_tr k3 s1 cin16 cout16 ") for l in labels) == 4, labels       # two Bottlenecks x two 3x3 convolutions
    blk = blocks.C2f(engine, 32, 32, 2, True, height=H, width=W, max_batch=B, dtype="bf16")
    blk.init_weights(3); blk.train()
    rng = np.random.default_rng(8)
    y = blk.forward(rng.standard_normal((B, 32, H, W), dtype=np.float32))
    dy = rng.standard_normal(y.shape, dtype=np.float32)
    grads = []
    for _ in range(2):
        blk.zero_grad()
        dx = blk.backward(dy)
        grads.append((dx, blk.grads()))
    blk.close()
    assert np.array_equal(grads[0][0], grads[1][0])
    for name in grads[0][1]:
        assert np.isfinite(grads[0][1][name]).all() and np.array_equal(grads[0][1][name], grads[1][1][name]), name
