"""conv_wgrad_tr_kernel's ring of LDS stages (csrc/conv_wgrad.hip): the DMA variants cut a stage into 1 KB requests, keep tile t in stage t % NS, and request tile
t + NS - 1 into the stage tile t - 1 was read from, one barrier per tile and a counted wait.  What can go wrong there and nowhere else: a stage overwritten before
every wave has read it, a wait that counts the wrong tile's requests, a prologue that requests tiles that do not exist, a lane of a request that falls on a pad slot
of a row pitch (or on the zero row, the rounding rows, a filler request) and does not write zeros.  Every case reads the stage count NS, the tile and the grid from
the launch label and asserts the property it is there for, so that a plan change cannot turn it into a different test.  bf16, through ys_conv_bwd, against torch
autograd on the bf16-rounded operands with the bound of tests/test_wgrad_tr_fetch.py (1e-4 of the reference's maximum); every case runs twice and the gradients
must be bit-identical.  Both backends: the interpreter executes a request at once -- it checks the addressing, the padding lanes and the label arithmetic, and
plans for the 256 compute units of the MI355X, so its labels are the device's -- but only the device can show a stage overwritten too early.

Images are small on purpose (8 x 8 to 35 x 35): the ring's properties are counted in tiles per workgroup, and small tiles keep the operands at a few million elements."""
import ctypes as C
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import BACKENDS
from bf16_ref import check_elem
from test_wgrad_tr_fetch import tiles_and_grid, wgrad_labels

# (B, Cin, H, W, Cout, k, s), property, fewest stages the case is meant for (2 = a ring, however deep the plan makes it; 1 = whichever fetch the plan gives the shape)
#   "wrap"    every stage is reused at least twice and the last workgroups walk one tile fewer: tiles >= (2 NS + 1) gx, tiles % gx != 0
#   "single"  one tile per workgroup: nothing to overlap, so the plan gives it the register fetch.  (With the two stages the plan uses, "fewer tiles per
#             workgroup than stages" is this case and no other, so a ring prologue never meets a tile that does not exist; "exact0" is its nearest neighbour.)
#   "exact0"  exactly NS tiles per workgroup (no stage is used twice);  "exact1"  exactly NS + 1 (the first wrap)
#   "deep"    at least NS + 1 tiles per workgroup: tiles >= (NS + 1) gx
#   "multi"   at least two tiles per workgroup;  "uneven"  and the last workgroups one fewer
CASES = [
    ((71, 80, 24, 24, 112, 3, 1), "wrap", 2),      # six channel tiles leave 36 workgroups per tile list: six tiles each, the last three workgroups five
    ((281, 80, 8, 8, 112, 3, 1), "wrap", 2),       # the same layer on 8 x 8 maps: a 22 KB stage, eight tiles each
    ((1, 32, 20, 20, 32, 3, 1), "single", 1),      # three tiles on three workgroups
    ((174, 64, 8, 8, 64, 3, 1), "exact0", 2),      # 174 tiles on 87 workgroups: the prologue requests the first, the first trip the second, and that is all
    ((30, 80, 20, 20, 160, 3, 1), "exact1", 2),    # 90 tiles on 30 workgroups
    ((40, 80, 20, 20, 160, 3, 1), "deep", 2),      # 120 tiles on 30 workgroups
    # stride 2 on odd sizes: the 16 (mod 32) patch pitch puts the pad lanes elsewhere; the last patch row / column is padding.  16 -> 32 at 45 x 45 plans 23 x 8 tiles,
    # two workgroups per CU and so no ring (tests/test_wgrad_tr_fetch.py has it); at 11 x 11 the same layer rings, and 1540 images are four tiles per workgroup
    ((1540, 16, 11, 11, 32, 3, 2), "deep", 2),
    ((36, 64, 35, 35, 128, 3, 2), "deep", 2),      # 18 x 4 tiles
    ((65, 64, 29, 29, 128, 3, 2), "deep", 2),      # 15 x 4 tiles
    ((1030, 16, 8, 8, 16, 3, 1), "uneven", 2),     # 16 channels: a 32-byte pitch, no pad slot
    ((520, 32, 8, 8, 32, 3, 1), "uneven", 2),      # 32 channels: 64 bytes in a 96-byte pitch, one pad slot in three
    ((260, 64, 8, 8, 64, 3, 1), "uneven", 2),      # 64 output channels: 128 bytes in a 160-byte pitch, two pad slots in ten
    ((130, 64, 12, 12, 64, 3, 1), "multi", 2),     # the same pitches in 12 x 16 tiles that hang over the image
    ((260, 48, 8, 8, 80, 3, 1), "uneven", 2),      # ragged 48 -> 80: three and five fragments, lanes outside the layer
    ((260, 80, 8, 8, 80, 1, 1), "uneven", 1),      # the 4-wave 1x1 layout, which shares the tile walk and the K loop: 260 tiles on 87 workgroups (planned without a ring)
]


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c[0])) + "-" + c[1])
def test_wgrad_tr_ring(backend, engine, case):
    from yolosharp_amd import _lib
    (B, Cin, H, W, Cout, k, s), prop, ns_min = case
    g = torch.Generator().manual_seed(300 + B + Cin + H)
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
    m = re.search(r" lds(\d+)(?: ring(\d+))?$", labels[0])       # a ring launch ends its label in " ring<NS>"; the register fetch (one stage) has no suffix
    assert m, labels[0]
    lds, ns = int(m.group(1)), int(m.group(2) or 1)
    assert ns_min <= ns <= 3 and lds <= 150 * 1024, labels[0]
    if prop == "wrap":
        assert tiles >= (2 * ns + 1) * gx and tiles % gx != 0, (labels[0], tiles)
    elif prop == "single":
        assert tiles == gx and ns == 1, (labels[0], tiles)
    elif prop == "exact0":
        assert tiles == ns * gx, (labels[0], tiles)
    elif prop == "exact1":
        assert tiles == (ns + 1) * gx, (labels[0], tiles)
    elif prop == "deep":
        assert tiles >= (ns + 1) * gx, (labels[0], tiles)
    else:
        assert tiles >= 2 * gx, (labels[0], tiles)
        if prop == "uneven":
            assert tiles % gx != 0, (labels[0], tiles)
    run()
    (dx, dw), (dx2, dw2) = runs
    assert np.array_equal(dw, dw2) and np.array_equal(dx, dx2), "two runs in one process differ"
    check_elem(dx, x.grad.numpy(), "dgrad %s" % (case[0],))
    ref = w.grad.numpy()
    err = float(np.abs(dw - ref).max())
    print("wgrad %s: max |err| %.3g, bound %.3g (%s)" % (case[0], err, 1e-4 * float(np.abs(ref).max()), labels[0]))
    assert np.isfinite(dw).all() and err <= 1e-4 * np.abs(ref).max()
