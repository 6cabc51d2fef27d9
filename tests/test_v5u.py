"""The YOLOv5u family (Models/Yolo.cs:137-198), detect task: tensor surface pinned to the reference's shipped Yolov5n.bin, the C3 block handle, f32 parity of a
whole step (plain and End2End) against tests/v5u_ref.py, the bf16 model on both routes of model.0 (the 6x6 stem kernels of csrc/conv_stem6.hip against the
packed copy + generic kernels), and the family-agnostic host path (Trainer / MosaicAugmenter / Detector)."""
import copy
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import e2e_ref as R
import v5u_ref as V
from conftest import BACKENDS
from oracle import yolo_oracle as O
from test_model import assert_pred_blocks, relerr
from test_stem6_kernels import bf16r

GOLD = os.path.join(os.path.dirname(__file__), "golden")
U = 2.0 ** -24


def _model(engine, ref=None, **kw):
    from yolosharp_amd.model import Yolov5u
    m = Yolov5u(engine, **kw)
    if ref is not None:
        m.load_state_dict({k: v.detach().numpy() for k, v in ref.state_dict().items()})
    return m


def _np(d):
    return {k: v.numpy() for k, v in d.items()}


# ---------------------------------------------------------------------------------------------------- 1: surface
@pytest.mark.parametrize("backend", BACKENDS)
def test_surface_matches_reference_listing(backend, engine, tmp_path):
    from yolosharp_amd import weights_bin as WB
    ref = V.Yolov5u(nc=80, size="n")
    m = _model(engine, nc=80, size="n", height=64, width=64, max_batch=1, dtype="f32")
    info = m.tensor_info()
    sd = ref.state_dict()
    assert [n for n, s, p in info if p] == [k for k, _ in ref.named_parameters()]
    assert {n: tuple(s) for n, s, p in info} == {k: tuple(v.shape) if v.dim() else (1,) for k, v in sd.items()}
    assert m.num_params() == sum(p.numel() for n, p in ref.named_parameters() if "dfl" not in n)
    # the reference's shipped file: every tensor it lists under model.0 .. model.23 (trunk and neck; its model.24 is the old anchor head) exists with that shape,
    # and the engine has nothing else under those ids
    listing = [(n, tuple(s) if s else (1,)) for n, _, s in json.load(open(os.path.join(GOLD, "yolov5n_tensors.json")))]
    assert len(listing) == 348
    trunk = {n: s for n, s in listing if int(n.split(".")[1]) < 24}
    assert len(trunk) == 342
    mine = {n: tuple(s) for n, s, p in info if int(n.split(".")[1]) < 24}
    assert mine == trunk
    # ... and the file's first six tensors load and read back bit-equal
    with open(os.path.join(GOLD, "yolov5n_prefix.bin"), "rb") as f:      # the container header (348) and the first six tensors
        want = {n: np.asarray(a, np.float32) for n, _, a in WB.iter_bin(f, limit=6)}
    assert list(want)[0] == "model.0.conv.weight" and len(want) == 6
    m.load_state_dict(want, strict=False)
    back = m.state_dict()
    for k in want:
        assert np.array_equal(back[k].reshape(-1), want[k].reshape(-1)), k
    assert back["model.0.conv.weight"].shape == (16, 3, 6, 6)
    m.close()


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("size", ["s", "m", "l", "x"])
def test_sizes_create(backend, engine, size):
    ref = V.Yolov5u(nc=80, size=size)
    m = _model(engine, nc=80, size=size, height=64, width=64, max_batch=1, dtype="f32")
    assert m.num_params() == sum(p.numel() for n, p in ref.named_parameters() if "dfl" not in n)
    assert [n for n, s, p in m.tensor_info() if p] == [k for k, _ in ref.named_parameters()]
    m.close()


@pytest.mark.parametrize("backend", BACKENDS)
def test_other_tasks_and_fp8_are_refused(backend, engine):
    from yolosharp_amd import YsError, _lib
    for task, dtype in ((1, 1), (2, 1), (3, 1), (4, 1), (0, 2)):
        desc = _lib.ModelDesc(5, 0, task, 80, 16, 64, 64, 1, dtype, 0, 0, 0)
        h = C.c_void_p()
        with pytest.raises(YsError) as e:
            _lib.check(engine.lib, engine.lib.ys_model_create(engine.ctx, C.byref(desc), C.byref(h)))
        assert e.value.status == 4 and not h.value, (task, dtype)


# ---------------------------------------------------------------------------------------------------- 3: the C3 handle
C3_CASES = {"c3_n2_sc": (32, 32, 2, True), "c3_n1": (64, 32, 1, False)}


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("case", sorted(C3_CASES))
def test_c3_block_parity_f32(backend, engine, case):
    """tests/test_blocks.py's protocol (_block_parity) on C3: names, eval and train forward, dx, every parameter gradient, running statistics; 1e-3 relerr."""
    from yolosharp_amd import blocks
    c1, c2, n, sc = C3_CASES[case]
    B, H, W, tol = 2, 16, 16, 1e-3
    torch.manual_seed(11)
    ref = V.C3(c1, c2, n, sc)
    torch.manual_seed(5)
    for mod in ref.modules():
        if isinstance(mod, torch.nn.BatchNorm2d):
            mod.weight.data.uniform_(0.5, 1.5); mod.bias.data.normal_(0, 0.1)
            mod.running_mean.normal_(0, 0.1); mod.running_var.uniform_(0.5, 1.5)
    blk = blocks.C3(engine, c1, c2, n, sc, height=H, width=W, max_batch=B, dtype="f32")
    info = blk.tensor_info()
    assert [k for k, s, p in info if p] == [k for k, _ in ref.named_parameters()]
    assert {k: tuple(s) for k, s, p in info} == {k: (tuple(v.shape) if v.dim() else (1,)) for k, v in ref.state_dict().items()}
    assert dict((k, tuple(s)) for k, s, p in info)["m.0.cv1.conv.weight"] == (c2 // 2, c2 // 2, 1, 1)
    blk.load_state_dict({k: v.detach().numpy() for k, v in ref.state_dict().items()})
    x = torch.randn(B, c1, H, W, generator=torch.Generator().manual_seed(3))
    blk.eval(); ref.eval()
    with torch.no_grad():
        ry = ref(x)
    y = blk.forward(x.numpy())
    assert y.shape == tuple(ry.shape) and relerr(y, ry) < tol
    blk.train(); ref.train()
    xr = x.clone().requires_grad_(True)
    ry = ref(xr)
    y = blk.forward(x.numpy())
    assert relerr(y, ry) < tol
    dy = torch.randn(ry.shape, generator=torch.Generator().manual_seed(4))
    ry.backward(dy)
    blk.zero_grad()
    dx = blk.backward(dy.numpy())
    assert relerr(dx, xr.grad) < tol
    g = blk.grads()
    gmax = max(float(p.grad.abs().max()) for _, p in ref.named_parameters())
    for k, p in ref.named_parameters():
        b = p.grad.numpy()
        err = float(np.abs(g[k] - b).max() / max(float(np.abs(b).max()), 1e-3 * gmax))
        assert err < tol, (k, err)
    sd = blk.state_dict()
    for k, v in ref.state_dict().items():
        if "running" in k or "num_batches" in k:
            assert np.allclose(sd[k], v.numpy(), rtol=1e-3, atol=1e-4), k
    blk.close()


# ---------------------------------------------------------------------------------------------------- 4: the model in f32
@pytest.mark.parametrize("backend", BACKENDS)
def test_forward_loss_backward_adamw_f32(backend, engine):
    """tests/test_model.py::test_forward_loss_backward_adamw_f32 on Yolov5u-n: model.0 runs with pad = 2 on the generic kernels."""
    from yolosharp_amd.model import v8DetectionLoss
    B, H, W, nc = 2, 64, 64, 80
    ref = V.make_ref()
    m = _model(engine, ref, nc=nc, size="n", height=H, width=W, max_batch=B, dtype="f32")
    x = torch.rand(B, 3, H, W, generator=torch.Generator().manual_seed(3))
    batch = O.synthetic_batch(B, H, W, nc, seed=1)
    m.eval(); ref.eval()
    inf, preds = m.forward(x.numpy())
    with torch.no_grad():
        rinf, rpreds = ref(x)
    assert relerr(preds["boxes"], rpreds["boxes"]) < 1e-3 and relerr(preds["scores"], rpreds["scores"]) < 1e-3
    assert relerr(inf["boxes"], rinf["boxes"]) < 1e-3
    assert_pred_blocks(inf["boxes"], rinf["boxes"], nc, 1e-3, tag="v5un f32")
    m.train(); ref.train()
    _, preds = m.forward(x.numpy())
    _, rpreds = ref(x)
    assert relerr(preds["boxes"], rpreds["boxes"]) < 1e-3 and relerr(preds["scores"], rpreds["scores"]) < 1e-3
    loss, items = v8DetectionLoss(m)(None, _np(batch))
    rloss, ritems = O.v8DetectionLoss(nc)(rpreds, batch)
    assert np.allclose(items, ritems.numpy(), rtol=1e-3, atol=1e-5), (items, ritems)
    assert np.allclose(loss, rloss.detach().numpy(), rtol=1e-3, atol=1e-4)
    rloss.sum().backward()
    m.zero_grad(); m.backward()
    grads = m.grads()
    gscale = max(float(p.grad.abs().max()) for _, p in ref.named_parameters() if p.grad is not None)
    n_checked = 0
    for name, p in ref.named_parameters():
        if p.grad is None:
            continue
        r = p.grad.numpy()
        err = np.abs(grads[name] - r).max()
        assert err <= 1e-3 * np.abs(r).max() + 1e-6 * gscale, (name, err, np.abs(r).max())
        n_checked += 1
    assert n_checked > 150 and np.abs(grads["model.0.conv.weight"]).max() > 0
    sd = m.state_dict()
    for k, v in ref.state_dict().items():
        if "running" in k:
            assert np.allclose(sd[k], v.numpy(), rtol=1e-3, atol=1e-5), k
    assert sd["model.0.bn.num_batches_tracked"][0] == 1
    lr0 = round(0.002 * 5 / (4 + nc), 6)
    params = {n: p.detach().clone() for n, p in ref.named_parameters() if p.grad is not None}
    O.adamw_step(params, {n: p.grad for n, p in ref.named_parameters() if p.grad is not None}, {}, [lr0, lr0, lr0], step=1)
    m.adamw_step([lr0, lr0, lr0])
    after = m.state_dict()
    for n, p in params.items():
        gr = dict(ref.named_parameters())[n].grad.numpy()
        big = np.abs(gr) > max(1e-2 * np.abs(gr).max(), 1e-4 * gscale)
        d = np.abs(after[n] - p.numpy())
        assert d[big].max(initial=0.0) <= 2e-6 + 1e-4 * np.abs(p.numpy()).max(), n
        assert d.max() <= 2.5 * lr0, n
    m.close()


@pytest.mark.parametrize("backend", BACKENDS)
def test_end2end_loss_and_tower_gradients_f32(backend, engine):
    """Yolov5u(end2end=True): E2EDetectLoss items and the gradients of the aliased towers (and of the trunk) against tests/e2e_ref.py over v5u_ref."""
    from yolosharp_amd.model import v8DetectionLoss
    B, H, W, nc = 2, 64, 64, 7
    net = V.make_ref(nc=nc)
    sd0 = {k: v.detach().clone().numpy() for k, v in net.state_dict().items()}
    x = torch.rand(B, 3, H, W, generator=torch.Generator().manual_seed(3))
    batch = O.synthetic_batch(B, H, W, nc, seed=5, kmax=5)
    ref = R.E2E(net).train()
    _, rpreds = ref(x)
    rloss, ritems = R.E2EDetectLoss(nc)(rpreds, batch)
    rloss.sum().backward()
    m = _model(engine, nc=nc, size="n", height=H, width=W, max_batch=B, dtype="f32", end2end=True)
    m.load_state_dict(sd0)
    m.train(); m.zero_grad()
    _, preds = m.forward(x.numpy())
    assert set(preds) == {"one2many", "one2one"}
    assert relerr(preds["one2many"]["boxes"], rpreds["one2many"]["boxes"]) < 1e-3
    loss, items = v8DetectionLoss(m)(None, _np(batch))
    assert np.allclose(items, ritems.numpy(), rtol=1e-3, atol=1e-5), (items, ritems)
    m.backward()
    grads = m.grads()
    rg = {n: p.grad.numpy() for n, p in net.named_parameters() if p.grad is not None}
    gscale = max(float(np.abs(r).max()) for r in rg.values())
    towers = [n for n in rg if n.startswith("model.24.")]
    assert len(towers) >= 30
    for name, r in rg.items():
        err = np.abs(grads[name] - r).max()
        assert err <= 1e-3 * np.abs(r).max() + 1e-6 * gscale, (name, err, np.abs(r).max())
    m.close()


# ---------------------------------------------------------------------------------------------------- 5: bf16, both routes of model.0
def _route_step(engine, sd0, x, batch, B, H, W, nc, direct, steps=1):
    """One (or `steps`) forward + loss + backward of a bf16 Yolov5u-n with STEM_DIRECT = direct; the launches of the stem classes are counted over the first step."""
    from yolosharp_amd.model import v8DetectionLoss
    with engine.options(STEM_DIRECT=direct):             # read when the model is created
        m = _model(engine, nc=nc, size="n", height=H, width=W, max_batch=B, dtype="bf16")
    m.load_state_dict(sd0)
    m.train()
    crit = v8DetectionLoss(m)
    out = dict(sums=[])
    for s in range(steps):
        if s == 0:
            engine.kernel_profile(True)
        m.forward(x, fetch=False)
        loss, items = crit(None, batch)
        assert np.all(np.isfinite(items)), items
        out["sums"].append(float(loss.sum()))
        m.zero_grad(); m.backward()
        if s == 0:
            engine.synchronize()
            out["n_fwd"], out["n_wg"] = engine.kernel_profile_read("stem6")[0], engine.kernel_profile_read("stem6_wg")[0]
            engine.kernel_profile(False)
            out["y"], out["dy"] = m.get_output("model0_raw"), m.get_output("model0_dy")
            out["gw"] = m.grads()["model.0.conv.weight"]
        if steps > 1:
            m.adamw_step([1e-3] * 3)
    m.close()
    return out


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("shape", [(2, 64, 64), (3, 96, 160)])
def test_bf16_stem_routes(backend, engine, shape):
    """STEM_DIRECT 1 / 0 on the same bf16 model and batch.  Which route ran is counted (kernel-profile classes "stem6" / "stem6_wg": one launch each with the
    option on, none with it off -- a silent fallback fails here).  model.0's raw output on either route is within ONE bound of tests/test_stem6_kernels.py of
    the float64 convolution of the bf16 operands, so the two differ by at most two.  model.0.conv.weight.grad on either route is within one bound of the float64
    weight gradient for the dy THAT route's backward formed ("model0_dy": the two dy differ, because everything downstream of a one-ulp flip in y differs), so
    the two gradients differ by at most two bounds plus the difference of those two exact values."""
    B, H, W = shape
    nc = 7
    ref = V.make_ref(nc=nc, seed=2)
    sd0 = {k: v.detach().clone().numpy() for k, v in ref.state_dict().items()}
    x = bf16r(torch.rand(B, 3, H, W, generator=torch.Generator().manual_seed(3)).numpy())
    batch = _np(O.synthetic_batch(B, H, W, nc, seed=5, kmax=5))
    a = _route_step(engine, sd0, x, batch, B, H, W, nc, 1)
    b = _route_step(engine, sd0, x, batch, B, H, W, nc, 0)
    assert (a["n_fwd"], a["n_wg"]) == (1, 1), (a["n_fwd"], a["n_wg"])
    assert (b["n_fwd"], b["n_wg"]) == (0, 0), (b["n_fwd"], b["n_wg"])
    xd = torch.from_numpy(x).double()
    wd = torch.from_numpy(bf16r(sd0["model.0.conv.weight"])).double()
    y64 = F.conv2d(xd, wd, stride=2, padding=2).numpy()
    by = 2.0 ** -8 * np.abs(y64) + 108 * U * F.conv2d(xd.abs(), wd.abs(), stride=2, padding=2).numpy()
    for r in (a, b):
        assert (np.abs(r["y"].astype(np.float64) - y64) <= by).all()
    assert (np.abs(a["y"].astype(np.float64) - b["y"]) <= 2 * by).all()
    M = B * y64.shape[2] * y64.shape[3]
    exact, bound = [], []
    for r in (a, b):
        dyd = torch.from_numpy(r["dy"]).double()
        g64 = torch.nn.grad.conv2d_weight(xd, wd.shape, dyd, stride=2, padding=2).numpy()
        bg = M * U * torch.nn.grad.conv2d_weight(xd.abs(), wd.shape, dyd.abs(), stride=2, padding=2).numpy()
        assert np.abs(g64).max() > 0
        err = np.abs(r["gw"].astype(np.float64) - g64)
        assert (err <= bg).all(), float((err / np.maximum(bg, 1e-300)).max())
        exact.append(g64); bound.append(bg)
    assert (np.abs(a["gw"].astype(np.float64) - b["gw"]) <= bound[0] + bound[1] + np.abs(exact[0] - exact[1])).all()


@pytest.mark.parametrize("backend", BACKENDS)
def test_bf16_three_steps_descend(backend, engine):
    B, H, W, nc = 2, 64, 64, 7
    ref = V.make_ref(nc=nc, seed=2)
    sd0 = {k: v.detach().clone().numpy() for k, v in ref.state_dict().items()}
    x = torch.rand(B, 3, H, W, generator=torch.Generator().manual_seed(3)).numpy()
    batch = _np(O.synthetic_batch(B, H, W, nc, seed=5, kmax=5))
    r = _route_step(engine, sd0, x, batch, B, H, W, nc, 1, steps=3)
    assert (r["n_fwd"], r["n_wg"]) == (1, 1)
    assert np.all(np.isfinite(r["sums"])) and r["sums"][2] < r["sums"][0], r["sums"]


# ---------------------------------------------------------------------------------------------------- 6: host path
@pytest.mark.gpu
@pytest.mark.parametrize("backend", ["gpu"])
@pytest.mark.parametrize("end2end", [False, True])
def test_trainer_mosaic_detector_are_family_agnostic(backend, engine, end2end, tmp_path):
    """One Trainer.fit epoch of two batches fed by MosaicAugmenter at 64 x 64, then Detector.ImagePredict on the bus image: completes, finite rows."""
    from PIL import Image
    from test_augment import _tiny_dataset
    from yolosharp_amd import augment as A
    from yolosharp_amd import trainer as T
    from yolosharp_amd.detector import Detector
    nc, S = 5, 64
    imgs, labels = _tiny_dataset(5, s=S)
    aug = A.MosaicAugmenter(engine, imgs, labels, S, degrees=5.0, seed=9, max_batch=2)
    m = _model(engine, nc=nc, size="n", height=S, width=S, max_batch=2, dtype="bf16", end2end=end2end)
    m.init_weights(1)
    tr = T.Trainer(m, epochs=1, nb=2, lr0=2e-3, warmup_bias_lr=2e-3)
    hist = tr.fit(lambda: (aug.batch(i) for i in ([0, 1], [2, 3])), augmenter=aug, close_mosaic=1)
    assert tr.steps_run == 2 and np.all(np.isfinite(hist[0]["train_loss"])) and hist[0]["train_loss"][1] > 0
    sd = m.state_dict()
    assert all(np.isfinite(v).all() for v in sd.values())
    bus = np.asarray(Image.open(os.path.join(GOLD, "bus_480x640.jpg")).convert("RGB"), np.uint8)
    bus = np.ascontiguousarray(bus.transpose(2, 0, 1))
    p = _model(engine, nc=nc, size="n", height=(bus.shape[1] + 31) // 32 * 32, width=(bus.shape[2] + 31) // 32 * 32, max_batch=1, dtype="bf16", end2end=end2end)
    p.load_state_dict(sd)
    det = Detector(p)
    assert det.end2end == end2end
    res = det.ImagePredict(bus, predict_threshold=0.001)
    assert len(res) > 0
    for r in res:
        assert np.isfinite([r.Score, r.CenterX, r.CenterY, r.Width, r.Height]).all() and 0 <= r.ClassID < nc
    m.close(); p.close(); aug.close()
