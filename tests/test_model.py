"""End-to-end parity of the YOLOv8 detect path: forward (train/eval), v8DetectionLoss, backward, AdamW.
Oracle = oracle/yolo_oracle.py (ATen-CPU restatement of the cited C#).  Tolerance: logits/loss 1e-3 in fp32 (north star)."""
import os

import numpy as np
import pytest
import torch

from conftest import BACKENDS
from oracle import yolo_oracle as O

GOLD = os.path.join(os.path.dirname(__file__), "golden", "model_golden.npz")


def make_ref(nc=80, size="n", seed=0):
    torch.manual_seed(seed)
    ref = O.Yolov8(nc=nc, size=size)
    for mod in ref.modules():
        if isinstance(mod, torch.nn.BatchNorm2d):
            mod.weight.data.uniform_(0.5, 1.5); mod.bias.data.normal_(0, 0.1)
            mod.running_mean.normal_(0, 0.1); mod.running_var.uniform_(0.5, 1.5)
    return ref


def build(engine, ref, H, W, B, dtype, nc=80, size="n"):
    from yolosharp_amd.model import Yolov8
    m = Yolov8(engine, nc=nc, size=size, height=H, width=W, max_batch=B, dtype=dtype)
    m.load_state_dict({k: v.detach().numpy() for k, v in ref.state_dict().items()})
    return m


def relerr(a, b):
    """Per-element distance: max over elements of |a - b| / (|b| + rms(b)), i.e. `relerr(a, b) < tol` asserts |a - b| <= tol |b| + tol rms(b) for EVERY element
    (rounds 1-4 divided the largest difference by the tensor's largest magnitude, which a wrong block of small values passes)."""
    b = b.detach().numpy() if hasattr(b, "detach") else np.asarray(b)
    b = b.astype(np.float64); a = np.asarray(a).astype(np.float64)
    rms = max(float(np.sqrt((b * b).mean())), 1e-6)
    return float((np.abs(a - b) / (np.abs(b) + rms)).max())


def pred_block_errs(a, b, nc, kdim=0, tag=""):
    """relerr per block of an eval prediction [B, 4 + nc (+ extra), A]: "boxes" (pixels, in the hundreds), "probs" (class probabilities, below 1) and the extra
    channels ("extra"; a Pose head with kdim 3: "kxy" in pixels and "kvis", a sigmoid, apart).  One relerr over the whole tensor takes its rms from the pixel
    coordinates, and a class probability wrong by 0.1 passes it at 1e-3; per block it does not."""
    b = b.detach().numpy() if hasattr(b, "detach") else np.asarray(b)
    a = np.asarray(a)
    out = {"boxes": relerr(a[:, :4], b[:, :4]), "probs": relerr(a[:, 4:4 + nc], b[:, 4:4 + nc])}
    xa, xb = a[:, 4 + nc:], b[:, 4 + nc:]
    if xa.shape[1] and kdim == 3:
        vis = np.arange(xa.shape[1]) % 3 == 2
        out["kxy"], out["kvis"] = relerr(xa[:, ~vis], xb[:, ~vis]), relerr(xa[:, vis], xb[:, vis])
    elif xa.shape[1]:
        out["extra"] = relerr(xa, xb)
    print("MEASURE pred blocks %s %s" % (tag, {k: "%.3g" % v for k, v in out.items()}))
    return out


def assert_pred_blocks(a, b, nc, tol, kdim=0, tag=""):
    errs = pred_block_errs(a, b, nc, kdim, tag)
    for k, v in errs.items():
        assert v < tol, (tag, k, v, tol)


@pytest.mark.parametrize("backend", BACKENDS)
def test_state_dict_surface(backend, engine):
    """Names, shapes and parameter order equal TorchSharp/PyTorch registration order (Yolo.cs:10-39, 'model.{i}...')."""
    ref = make_ref()
    from yolosharp_amd.model import Yolov8
    m = Yolov8(engine, nc=80, size="n", height=64, width=64, max_batch=1, dtype="f32")
    info = m.tensor_info()
    sd = ref.state_dict()
    assert [n for n, s, p in info if p] == [k for k, _ in ref.named_parameters()]
    assert {n: tuple(s) for n, s, p in info if n in sd} == {k: tuple(v.shape) if v.dim() else (1,) for k, v in sd.items()}
    assert m.num_params() == sum(p.numel() for n, p in ref.named_parameters() if "dfl" not in n) == 3157184 - 0
    assert info[0][0] == "model.0.conv.weight" and info[0][1] == (16, 3, 3, 3)
    sd2 = {k: v.numpy() for k, v in sd.items()}
    m.load_state_dict(sd2)
    back = m.state_dict()
    for k in ("model.0.conv.weight", "model.22.cv2.0.2.bias", "model.9.cv1.bn.running_var", "model.22.dfl.conv.weight"):
        assert np.array_equal(back[k].reshape(-1), sd2[k].reshape(-1)), k
    m.close()


@pytest.mark.parametrize("backend", BACKENDS)
def test_forward_loss_backward_adamw_f32(backend, engine):
    B, H, W, nc = 2, 64, 64, 80
    ref = make_ref()
    m = build(engine, ref, H, W, B, "f32")
    g = np.load(GOLD)
    assert np.array_equal(g["w_model.0.conv.weight"], ref.state_dict()["model.0.conv.weight"].numpy()), "weight regeneration drifted"
    x = torch.from_numpy(g["x"])
    batch = {k: torch.from_numpy(g[k]) for k in ("batch_idx", "cls", "bboxes")}
    # ---- eval forward + decode (Head.cs:204-223)
    m.eval(); ref.eval()
    inf, preds = m.forward(x.numpy())
    with torch.no_grad():
        rinf, rpreds = ref(x)
    assert relerr(preds["boxes"], rpreds["boxes"]) < 1e-3 and relerr(preds["scores"], rpreds["scores"]) < 1e-3
    assert relerr(inf["boxes"], rinf["boxes"]) < 1e-3
    assert_pred_blocks(inf["boxes"], rinf["boxes"], nc, 1e-3, tag="v8n f32")
    assert np.abs(inf["boxes"] - g["pred_eval"].astype(np.float32)).max() < 2e-3 * np.abs(g["pred_eval"]).max()   # fp16-stored fixture
    # ---- train forward (batch statistics), loss, backward
    m.train(); ref.train()
    _, preds = m.forward(x.numpy())
    _, rpreds = ref(x)
    assert relerr(preds["boxes"], rpreds["boxes"]) < 1e-3 and relerr(preds["scores"], rpreds["scores"]) < 1e-3
    from yolosharp_amd.model import v8DetectionLoss
    loss, items = v8DetectionLoss(m)(None, {k: v.numpy() for k, v in batch.items()})
    rloss, ritems = O.v8DetectionLoss(nc)(rpreds, batch)
    assert np.allclose(items, ritems.numpy(), rtol=1e-3, atol=1e-5), (items, ritems)
    assert np.allclose(items, g["loss_items"], rtol=1e-3, atol=1e-5)
    assert np.allclose(loss, rloss.detach().numpy(), rtol=1e-3, atol=1e-4)
    rloss.sum().backward()
    m.zero_grad(); m.backward()
    grads = m.grads()
    gscale = max(float(p.grad.abs().max()) for _, p in ref.named_parameters() if p.grad is not None)
    for name, p in ref.named_parameters():
        if p.grad is None:
            continue
        r = p.grad.numpy()
        err = np.abs(grads[name] - r).max()
        assert err <= 1e-3 * np.abs(r).max() + 1e-6 * gscale, (name, err, np.abs(r).max())
    for k in ("model.0.conv.weight", "model.22.cv3.0.2.bias", "model.4.m.1.cv2.bn.weight"):
        assert np.abs(grads[k] - g["grad_" + k]).max() <= 1e-3 * np.abs(g["grad_" + k]).max() + 1e-6 * gscale
    # running statistics after one training forward (momentum 0.03, unbiased var)
    sd = m.state_dict()
    for k in ("model.0.bn.running_mean", "model.9.cv1.bn.running_var", "model.22.cv3.2.1.bn.running_var"):
        assert np.allclose(sd[k], ref.state_dict()[k].numpy(), rtol=1e-3, atol=1e-5), k
    assert sd["model.0.bn.num_batches_tracked"][0] == 1
    # ---- AdamW (fp32 master weights; lr0 = round(0.002*5/(4+nc),6), wd 5e-4)
    lr0 = round(0.002 * 5 / (4 + nc), 6)
    params = {n: p.detach().clone() for n, p in ref.named_parameters() if p.grad is not None}
    O.adamw_step(params, {n: p.grad for n, p in ref.named_parameters() if p.grad is not None}, {}, [lr0, lr0, lr0], step=1)
    m.adamw_step([lr0, lr0, lr0])
    after = m.state_dict()
    for n, p in params.items():
        # Adam's first step is lr*g/(|g|+eps) ~ lr*sign(g): where g is at rounding-noise level the sign is not
        # determined, so those elements are only bounded by 2*lr; everything else must match tightly.
        gr = dict(ref.named_parameters())[n].grad.numpy()
        big = np.abs(gr) > max(1e-2 * np.abs(gr).max(), 1e-4 * gscale)
        d = np.abs(after[n] - p.numpy())
        assert d[big].max(initial=0.0) <= 2e-6 + 1e-4 * np.abs(p.numpy()).max(), n
        assert d.max() <= 2.5 * lr0, n
    assert np.array_equal(after["model.22.dfl.conv.weight"].reshape(-1), np.arange(16, dtype=np.float32))
    m.close()


@pytest.mark.parametrize("backend", BACKENDS)
def test_loss_edge_cases(backend, engine):
    """Empty GT (n_max_boxes == 0 branch, Tal.cs:57-66), tiny boxes (inflated to 16 px, Tal.cs:206-211), multi-GT overlap."""
    B, H, W, nc = 2, 64, 64, 80
    ref = make_ref(seed=3)
    m = build(engine, ref, H, W, B, "f32")
    from yolosharp_amd.model import v8DetectionLoss
    x = torch.rand(B, 3, H, W, generator=torch.Generator().manual_seed(5))
    m.train(); ref.train()
    crit, rcrit = v8DetectionLoss(m), O.v8DetectionLoss(nc)
    batches = [
        {"batch_idx": torch.zeros(0), "cls": torch.zeros(0), "bboxes": torch.zeros(0, 4)},
        {"batch_idx": torch.tensor([1.0, 1.0, 1.0]), "cls": torch.tensor([3.0, 3.0, 7.0]),      # image 0 empty; nested boxes
         "bboxes": torch.tensor([[0.5, 0.5, 0.6, 0.6], [0.5, 0.5, 0.5, 0.5], [0.52, 0.5, 0.05, 0.04]])},
    ]
    for batch in batches:
        m.forward(x.numpy(), fetch=False)
        _, rpreds = ref(x)
        loss, items = crit(None, {k: v.numpy() for k, v in batch.items()})
        rloss, ritems = rcrit(rpreds, batch)
        assert np.allclose(items, ritems.numpy(), rtol=1e-3, atol=1e-5), (items, ritems)
    m.close()


@pytest.mark.parametrize("backend", BACKENDS)
def test_crowded_image_more_labels_than_initial_capacity(backend, engine):
    """The reference pads every image to the batch's largest label count, whatever it is (Loss.cs:363-390; mosaic batches
    exceed 64 per image).  Host labels grow the engine's workspace; device labels past the capacity are REFUSED, never truncated."""
    from yolosharp_amd import YsError
    from yolosharp_amd.model import Yolov8, v8DetectionLoss
    B, H, W, nc = 2, 64, 64, 80
    ref = make_ref(seed=5)
    m = Yolov8(engine, nc=nc, size="n", height=H, width=W, max_batch=B, dtype="f32", max_labels=8)
    m.load_state_dict({k: v.detach().numpy() for k, v in ref.state_dict().items()})
    x = torch.rand(B, 3, H, W, generator=torch.Generator().manual_seed(6))
    rng = np.random.default_rng(7)
    n0, n1 = 71, 3                                            # image 0 carries 71 labels (> 64 and > the initial 8)
    wh = rng.uniform(0.08, 0.5, (n0 + n1, 2)); c = wh / 2 + rng.uniform(0, 1, (n0 + n1, 2)) * (1 - wh)
    batch = {"batch_idx": torch.tensor([0.0] * n0 + [1.0] * n1), "cls": torch.from_numpy(rng.integers(0, nc, n0 + n1).astype(np.float32)),
             "bboxes": torch.from_numpy(np.concatenate([c, wh], 1).astype(np.float32))}
    nb = {k: v.numpy() for k, v in batch.items()}
    m.train(); ref.train()
    m.forward(x.numpy(), fetch=False)
    _, rpreds = ref(x)
    rloss, ritems = O.v8DetectionLoss(nc)(rpreds, batch)
    crit = v8DetectionLoss(m)
    loss, items = crit(None, nb)                               # host labels: workspace grows to 71 -> 80
    assert np.allclose(items, ritems.numpy(), rtol=1e-3, atol=1e-5), (items, ritems)
    rloss.sum().backward()
    m.zero_grad(); m.backward()
    g = m.grads()
    for name in ("model.22.cv3.0.2.bias", "model.22.cv2.1.2.weight", "model.0.conv.weight"):
        r = dict(ref.named_parameters())[name].grad.numpy()
        assert np.abs(g[name] - r).max() <= 2e-3 * np.abs(r).max() + 1e-7, name
    # device-resident labels: no host sync can size the workspace -> the first synchronising read refuses the truncated result
    m2 = Yolov8(engine, nc=nc, size="n", height=H, width=W, max_batch=B, dtype="f32", max_labels=8)
    m2.load_state_dict({k: v.detach().numpy() for k, v in ref.state_dict().items()})
    m2.train(); m2.forward(x.numpy(), fetch=False)
    d = [engine.to_device(nb[k]) for k in ("batch_idx", "cls", "bboxes")]
    crit2 = v8DetectionLoss(m2)
    crit2.forward_device(d[0], d[1], d[2], n0 + n1)
    with pytest.raises(YsError) as ei:
        crit2.read()
    assert ei.value.status == 1 and "71" in str(ei.value)
    m2.reserve_labels(71)
    m2.forward(x.numpy(), fetch=False)
    crit2.forward_device(d[0], d[1], d[2], n0 + n1)
    assert np.allclose(crit2.read()[1], ritems.numpy(), rtol=1e-3, atol=1e-5)
    for p in d:
        engine.free(p)
    m.close(); m2.close()


@pytest.mark.parametrize("backend", BACKENDS)
def test_out_of_range_batch_idx_rows_do_not_overflow_staging(backend, engine):
    """Label rows whose batch_idx lies outside [0, B) are ignored by the criterion (the reference matches `batch_idx == j`,
    Loss.cs:376-388) but they ARE staged: 70 rows of which 69 point at a missing image used to overrun the gcap * max_batch
    staging arrays (round-2 advisor finding).  The workspace now grows with the row count; the loss equals the in-range labels'."""
    from yolosharp_amd.model import Yolov8, v8DetectionLoss
    B, H, W, nc = 1, 64, 64, 80
    ref = make_ref(seed=5)
    m = Yolov8(engine, nc=nc, size="n", height=H, width=W, max_batch=B, dtype="f32")      # default capacity: 64 rows
    m.load_state_dict({k: v.detach().numpy() for k, v in ref.state_dict().items()})
    x = torch.rand(B, 3, H, W, generator=torch.Generator().manual_seed(6))
    rng = np.random.default_rng(11)
    n = 70
    wh = rng.uniform(0.1, 0.5, (n, 2)); c = wh / 2 + rng.uniform(0, 1, (n, 2)) * (1 - wh)
    bidx = np.full(n, 7.0, np.float32); bidx[0] = 0.0
    nb = {"batch_idx": bidx, "cls": rng.integers(0, nc, n).astype(np.float32), "bboxes": np.concatenate([c, wh], 1).astype(np.float32)}
    m.train(); ref.train()
    m.forward(x.numpy(), fetch=False)
    _, rpreds = ref(x)
    keep = {k: torch.from_numpy(v[:1].copy()) for k, v in nb.items()}
    _, ritems = O.v8DetectionLoss(nc)(rpreds, keep)
    for rows in (n, 5000):
        big = {k: np.concatenate([v] + [v[1:2]] * (rows - n), 0) if rows > n else v for k, v in nb.items()}
        _, items = v8DetectionLoss(m)(None, big)
        assert np.allclose(items, ritems.numpy(), rtol=1e-3, atol=1e-5), (rows, items, ritems)
    m.close()


def test_conv_bn_act_dtype_names():
    """engine.conv_bn_act accepts the same dtype names as the model classes and rejects anything else with a ValueError."""
    from yolosharp_amd import engine as E
    from yolosharp_amd.model import DTYPES
    for name, code in DTYPES.items():
        assert E._dtype_code(name) == code
    with pytest.raises(ValueError):
        E._dtype_code("half")


@pytest.mark.parametrize("backend", BACKENDS)
def test_bf16_path_tracks_f32(backend, engine):
    """bf16 is the performance mode: validated against the fp32 oracle within bf16 rounding (eval logits ~1%)."""
    B, H, W, nc = 2, 64, 64, 80
    ref = make_ref(seed=1)
    m = build(engine, ref, H, W, B, "bf16")
    x = torch.rand(B, 3, H, W, generator=torch.Generator().manual_seed(2))
    m.eval(); ref.eval()
    inf, preds = m.forward(x.numpy())
    with torch.no_grad():
        rinf, rpreds = ref(x)
    assert relerr(preds["boxes"], rpreds["boxes"]) < 3e-2 and relerr(preds["scores"], rpreds["scores"]) < 3e-2
    assert relerr(inf["boxes"], rinf["boxes"]) < 1e-2
    assert_pred_blocks(inf["boxes"], rinf["boxes"], nc, 1e-2, tag="v8n bf16")
    m.close()


@pytest.mark.parametrize("backend", BACKENDS)
def test_stem_reads_fp32_planes_directly_bf16(backend, engine):
    """model.0 (Conv(3, c, 3, 2): Yolo.cs:43, Convs.cs:36-62) on the bf16 path reads the fp32 NCHW image itself (csrc/conv_stem.hip) --
    forward, batch statistics and weight gradient -- instead of a packed bf16 NHWC copy.  Checked (a) against the packed-copy path of the
    same engine (YS_STEM_DIRECT=0 at model creation; same operand rounding, different summation order) on a canvas whose stem output
    (64 x 80) leaves ragged 8 x 32 tiles, and (b) against the fp32 oracle restricted to that layer with rounding-matched operands.
    (Round 6: B = 4, 128 x 160 instead of B = 2, 96 x 160.  The two paths round identically but add their BatchNorm partial sums in different orders; on the smaller
    canvas the P5 BatchNorms normalise over 30 values per channel and ONE activation whose bf16 rounding flips at the stem moves model.0's weight gradient by tens of
    per cent -- the rounding-matched and the plain ORACLE differ that much from each other there -- so the comparison said more about the tile plan of the day than
    about the stem kernels: a plan change in conv_p2_kernel turned 3e-2 into 1.08 with both paths correct layer by layer.)"""
    B, H, W, nc = 4, 128, 160, 80
    ref = make_ref(seed=3)
    x = torch.rand(B, 3, H, W, generator=torch.Generator().manual_seed(4))
    batch = O.synthetic_batch(B, H, W, nc, seed=5, kmax=5)
    from yolosharp_amd.model import v8DetectionLoss
    out = {}
    for mode in ("1", "0"):
        with engine.options(STEM_DIRECT=int(mode)):
            m = build(engine, ref, H, W, B, "bf16")
        m.eval()
        inf, _ = m.forward(x.numpy())
        m.train()
        m.forward(x.numpy())
        loss, items = v8DetectionLoss(m)(None, {k: v.numpy() for k, v in batch.items()})
        m.zero_grad(); m.backward()
        g = m.grads(); sd = m.state_dict()
        out[mode] = dict(inf=inf["boxes"].copy(), items=np.asarray(items).copy(), gw=g["model.0.conv.weight"].copy(), gg=g["model.0.bn.weight"].copy(),
                         rm=sd["model.0.bn.running_mean"].copy(), rv=sd["model.0.bn.running_var"].copy())
        m.close()
    d, p = out["1"], out["0"]
    assert relerr(d["inf"], p["inf"]) < 1e-2
    assert np.allclose(d["items"], p["items"], rtol=2e-2)
    assert np.allclose(d["rm"], p["rm"], rtol=1e-4, atol=1e-6) and np.allclose(d["rv"], p["rv"], rtol=1e-4, atol=1e-6)
    # model.0's weight gradient: the two paths either agree to the last bit (no activation of the stem flipped its bf16 rounding: then everything downstream is identical
    # and only the summation order of the two weight-gradient kernels differs) or sit one chaotic amplification apart -- measured on the MI355X over nine canvases
    # (tools/dev/r06/stem_modes.py): five bit-identical, four at cosine 0.981-0.992 / per-element 0.33-0.53, whatever the size.  A wrong weight-gradient kernel is
    # neither: it is asserted against the oracle at the headline batch (tests/test_production_routing.py, every tensor's cosine) and here against the other path.
    cos = float((d["gw"] * p["gw"]).sum() / np.sqrt((d["gw"] ** 2).sum() * (p["gw"] ** 2).sum()))
    assert cos > 0.95, cos
    if np.array_equal(d["items"], p["items"]):           # no flip: the gradients may differ by summation order only
        assert relerr(d["gw"], p["gw"]) < 3e-2 and relerr(d["gg"], p["gg"]) < 3e-2 and cos > 0.999, cos
    # (b) the layer alone: bf16-rounded image and weights, fp32 accumulation, output rounded to bf16 before the statistics
    w0 = ref.state_dict()["model.0.conv.weight"]
    y = torch.nn.functional.conv2d(x.bfloat16().float(), w0.bfloat16().float(), stride=2, padding=1).bfloat16().float()
    mean = y.mean(dim=(0, 2, 3)); var = y.var(dim=(0, 2, 3), unbiased=True)
    rm0 = ref.state_dict()["model.0.bn.running_mean"]; rv0 = ref.state_dict()["model.0.bn.running_var"]
    assert np.allclose(d["rm"], (0.97 * rm0 + 0.03 * mean).numpy(), rtol=1e-3, atol=1e-5)
    assert np.allclose(d["rv"], (0.97 * rv0 + 0.03 * var).numpy(), rtol=1e-3, atol=1e-5)


@pytest.mark.gpu
@pytest.mark.parametrize("backend", ["gpu"])
def test_full_resolution_parity_f32(backend, engine):
    """640x640 (A = 8400), B=4, v8n: forward + loss + backward vs the oracle on the GPU box's CPU."""
    B, H, W, nc = 4, 640, 640, 80
    ref = make_ref(seed=7)
    m = build(engine, ref, H, W, B, "f32")
    x = torch.rand(B, 3, H, W, generator=torch.Generator().manual_seed(0))
    batch = O.synthetic_batch(B, H, W, nc, seed=1)
    m.train(); ref.train()
    _, preds = m.forward(x.numpy())
    _, rpreds = ref(x)
    assert relerr(preds["boxes"], rpreds["boxes"]) < 1e-3 and relerr(preds["scores"], rpreds["scores"]) < 1e-3
    from yolosharp_amd.model import v8DetectionLoss
    loss, items = v8DetectionLoss(m)(None, {k: v.numpy() for k, v in batch.items()})
    rloss, ritems = O.v8DetectionLoss(nc)(rpreds, batch)
    assert np.allclose(items, ritems.numpy(), rtol=1e-3, atol=1e-5), (items, ritems)
    rloss.sum().backward()
    m.zero_grad(); m.backward()
    grads = m.grads()
    gscale = max(float(p.grad.abs().max()) for _, p in ref.named_parameters() if p.grad is not None)
    worst = 0.0
    for name, p in ref.named_parameters():
        if p.grad is None:
            continue
        r = p.grad.numpy()
        worst = max(worst, (np.abs(grads[name] - r).max()) / (np.abs(r).max() + 1e-3 * gscale))
    assert worst < 2e-3, worst
    m.close()


@pytest.mark.gpu
@pytest.mark.parametrize("backend", ["gpu"])
def test_bf16_full_size_properties(backend, engine):
    """BASELINE config 2 shape (v8n, B=64, 640x640, bf16): size-independent properties.
    (1) bf16 and f32 engines agree on eval predictions and on the loss; (2) the step is deterministic (bitwise equal
    gradients on a repeated step: fixed-order reductions, no atomics on the data path); (3) loss is finite and AdamW moves it."""
    from yolosharp_amd.model import Yolov8, v8DetectionLoss
    B, H, W, nc = 64, 640, 640, 80
    rng = np.random.default_rng(0)
    x = rng.random((B, 3, H, W), dtype=np.float32)
    batch = {k: v.numpy() for k, v in O.synthetic_batch(B, H, W, nc, seed=1).items()}
    res = {}
    for dt in ("bf16", "f32"):
        m = Yolov8(engine, nc=nc, size="n", height=H, width=W, max_batch=B, dtype=dt)
        m.init_weights(2)
        m.train()
        m.forward(x, fetch=False)
        loss, items = v8DetectionLoss(m)(None, batch)
        m.zero_grad(); m.backward()
        g1 = m.grads()
        m.forward(x, fetch=False)
        v8DetectionLoss(m)(None, batch)
        m.zero_grad(); m.backward()
        g2 = m.grads()
        assert all(np.array_equal(g1[k], g2[k]) for k in g1), "step is not deterministic"
        res[dt] = (items, g1)
        assert np.all(np.isfinite(items))
        if dt == "bf16":
            l0 = items.sum()
            for _ in range(3):
                m.adamw_step([1e-3, 1e-3, 1e-3]); m.zero_grad()
                m.forward(x, fetch=False); _, it = v8DetectionLoss(m)(None, batch); m.backward()
            assert it.sum() < l0, (it, l0)
        m.close()
    a, b = res["bf16"][0], res["f32"][0]
    assert np.allclose(a, b, rtol=5e-2), (a, b)
    ga, gb = res["bf16"][1], res["f32"][1]
    num = sum(float((ga[k].ravel() * gb[k].ravel()).sum()) for k in ga)
    den = np.sqrt(sum(float((ga[k] ** 2).sum()) for k in ga) * sum(float((gb[k] ** 2).sum()) for k in gb))
    assert num / den > 0.98, num / den


# ----------------------------------------------------------------------------- YOLOv11
def make_ref11(nc=80, size="n", seed=0):
    torch.manual_seed(seed)
    ref = O.Yolov11(nc=nc, size=size)
    for mod in ref.modules():
        if isinstance(mod, torch.nn.BatchNorm2d):
            mod.weight.data.uniform_(0.5, 1.5); mod.bias.data.normal_(0, 0.1)
            mod.running_mean.normal_(0, 0.1); mod.running_var.uniform_(0.5, 1.5)
    return ref


def _v11_parity(engine, size, B, H, W, tol_fwd, tol_grad):
    """C3k2 / C3k / C2PSA(attention + depthwise pe) / Detect(legacy=false): forward, loss and every gradient vs the oracle."""
    from yolosharp_amd.model import Yolov11, v8DetectionLoss
    nc = 80
    ref = make_ref11(size=size)
    m = Yolov11(engine, nc=nc, size=size, height=H, width=W, max_batch=B, dtype="f32")
    info = m.tensor_info()
    assert [n for n, s, p in info if p] == [k for k, _ in ref.named_parameters()]          # registration order incl. nested C3k
    assert {n: tuple(s) for n, s, p in info} == {k: (tuple(v.shape) if v.dim() else (1,)) for k, v in ref.state_dict().items()}
    m.load_state_dict({k: v.detach().numpy() for k, v in ref.state_dict().items()})
    x = torch.rand(B, 3, H, W, generator=torch.Generator().manual_seed(3))
    batch = O.synthetic_batch(B, H, W, nc, seed=1, kmax=6)
    m.eval(); ref.eval()
    inf, preds = m.forward(x.numpy())
    with torch.no_grad():
        rinf, rpreds = ref(x)
    assert relerr(preds["boxes"], rpreds["boxes"]) < tol_fwd and relerr(preds["scores"], rpreds["scores"]) < tol_fwd
    assert relerr(inf["boxes"], rinf["boxes"]) < tol_fwd
    assert_pred_blocks(inf["boxes"], rinf["boxes"], nc, tol_fwd, tag="v11%s f32" % size)
    m.train(); ref.train()
    _, preds = m.forward(x.numpy())
    _, rpreds = ref(x)
    assert relerr(preds["boxes"], rpreds["boxes"]) < tol_fwd and relerr(preds["scores"], rpreds["scores"]) < tol_fwd
    loss, items = v8DetectionLoss(m)(None, {k: v.numpy() for k, v in batch.items()})
    rloss, ritems = O.v8DetectionLoss(nc)(rpreds, batch)
    assert np.allclose(items, ritems.numpy(), rtol=1e-3, atol=1e-5), (items, ritems)
    rloss.sum().backward()
    m.zero_grad(); m.backward()
    grads = m.grads()
    gscale = max(float(p.grad.abs().max()) for _, p in ref.named_parameters() if p.grad is not None)
    for name, p in ref.named_parameters():
        if p.grad is None:
            continue
        r = p.grad.numpy()
        assert np.abs(grads[name] - r).max() <= tol_grad * np.abs(r).max() + 1e-6 * gscale, name
    m.close()


@pytest.mark.parametrize("backend", BACKENDS)
def test_yolov11n_forward_loss_backward_f32(backend, engine):
    _v11_parity(engine, "n", 2, 64, 64, 1e-3, 1e-3)


@pytest.mark.gpu
@pytest.mark.parametrize("backend", ["gpu"])
def test_yolov11m_full_resolution_f32(backend, engine):
    """c3k=True everywhere (nested C3k), 400-token attention at 640x640."""
    _v11_parity(engine, "m", 2, 640, 640, 1e-3, 2e-3)


@pytest.mark.gpu
@pytest.mark.parametrize("backend", ["gpu"])
def test_yolov11s_bf16_train_step(backend, engine):
    from yolosharp_amd.model import Yolov11, v8DetectionLoss
    B, H, W, nc = 16, 640, 640, 80
    rng = np.random.default_rng(0)
    x = rng.random((B, 3, H, W), dtype=np.float32)
    batch = {k: v.numpy() for k, v in O.synthetic_batch(B, H, W, nc, seed=1).items()}
    items = {}
    for dt in ("bf16", "f32"):
        m = Yolov11(engine, nc=nc, size="s", height=H, width=W, max_batch=B, dtype=dt)
        m.init_weights(4); m.train()
        m.forward(x, fetch=False)
        _, it = v8DetectionLoss(m)(None, batch)
        m.zero_grad(); m.backward(); m.adamw_step([1e-3] * 3)
        items[dt] = it
        m.close()
    assert np.all(np.isfinite(items["bf16"])) and np.allclose(items["bf16"], items["f32"], rtol=5e-2), items


@pytest.mark.gpu
@pytest.mark.parametrize("backend", ["gpu"])
def test_bf16_training_tracks_f32_over_40_steps(backend, engine):
    """bf16 acceptance beyond three optimizer steps.  YOLOv8n, 320x320, B=16, the same initial weights, batch
    and learning rate in both engines: 40 AdamW steps.  The bf16 loss curve must stay within 8 % of the fp32 curve at every step and
    within 3 % on average (observed drift is reported in the assertion message), both must fall by more than 10 %, and the two weight trajectories must
    point the same way (Adam moves every weight by ~lr per step whatever its gradient's size, so weights whose gradient is at
    rounding-noise level random-walk in both runs: the test is on the direction of the total update, not on a distance)."""
    from yolosharp_amd.model import Yolov8, v8DetectionLoss
    B, H, W, nc, steps = 16, 320, 320, 80, 40
    x = np.random.default_rng(0).random((B, 3, H, W), dtype=np.float32)
    batch = {k: v.numpy() for k, v in O.synthetic_batch(B, H, W, nc, seed=1, kmax=8).items()}
    curves, final, init = {}, {}, None
    for dt in ("f32", "bf16"):
        m = Yolov8(engine, nc=nc, size="n", height=H, width=W, max_batch=B, dtype=dt)
        m.init_weights(11); m.train()
        if init is None:
            init = m.state_dict()
        crit = v8DetectionLoss(m)
        rec = []
        for _ in range(steps):
            m.forward(x, fetch=False); _, items = crit(None, batch); m.zero_grad(); m.backward(); m.adamw_step([5e-4] * 3)
            rec.append(float(items.sum()))
        curves[dt] = np.array(rec)
        final[dt] = m.state_dict()
        m.close()
    a, b = curves["bf16"], curves["f32"]
    drift = np.abs(a - b) / b
    # The per-step maximum is a chaotic quantity: an A/B of two builds whose first-step box gradients differed in TWO bf16 elements
    # by one ulp (tools/dev/drift_curve.py, dump_dboxes.py) moved it from 3.75 % (mean 0.9 %) to 5.7 % (mean 2.0 %) -- bf16 gradient
    # storage re-rounds every layer's dy, Adam turns noise-level gradients into +-lr steps.  Hence a loose maximum and a mean.
    assert drift.max() < 8e-2 and drift.mean() < 3e-2, (float(drift.max()), int(drift.argmax()), float(drift.mean()))
    assert a[-1] < 0.9 * a[0] and b[-1] < 0.9 * b[0], (a[0], a[-1], b[0], b[-1])
    keys = [k for k in init if "running" not in k and "num_batches" not in k and "dfl" not in k]
    da = np.concatenate([(final["bf16"][k] - init[k]).ravel() for k in keys])
    db = np.concatenate([(final["f32"][k] - init[k]).ravel() for k in keys])
    cos = float(da @ db / np.sqrt((da @ da) * (db @ db)))
    assert cos > 0.55, cos


@pytest.mark.gpu
@pytest.mark.parametrize("backend", ["gpu"])
def test_first_step_of_a_new_model_is_deterministic(backend, engine):
    """Every gradient of the FIRST step of a freshly built model, twelve models in a row on recycled device memory, bit for bit.  Round 5: the stem weight-gradient
    kernel reused its dy rows as reduction scratch without a barrier; the race showed almost only on a model's first launch (waves of a workgroup furthest apart), as
    an occasional wrong or NaN model.0 gradient that the repeated-step checks on ONE model never saw (tools/dev/r05/det_phase.py found it: 3 of 40 models)."""
    from yolosharp_amd.model import Yolov8, v8DetectionLoss
    B, H, W, nc = 8, 640, 640, 80
    x = np.random.default_rng(0).random((B, 3, H, W), dtype=np.float32)
    batch = {k: v.numpy() for k, v in O.synthetic_batch(B, H, W, nc, seed=1).items()}
    ref = None
    for trial in range(12):
        m = Yolov8(engine, nc=nc, size="n", height=H, width=W, max_batch=B, dtype="bf16")
        m.init_weights(2); m.train()
        m.forward(x, fetch=False); _, items = v8DetectionLoss(m)(None, batch); m.zero_grad(); m.backward()
        g = m.grads()
        m.close()
        assert all(np.isfinite(v).all() for v in g.values()), trial
        if ref is None:
            ref = (items, g)
            continue
        assert np.array_equal(items, ref[0]), (trial, items, ref[0])
        bad = [k for k in g if not np.array_equal(g[k], ref[1][k])]
        assert not bad, (trial, bad[:4])
