"""End2End for Segment models (ys_model_e2e_init): aliased cv2 / cv3 / cv4 towers with Proto run once, E2ESegmentLoss (gains, tal_topk2 = 1), the
two-pass head backward, the top-k post-process with mask coefficients, Segmenter on an End2End model, the task boundary.
Oracle = tests/e2e_seg_ref.py over oracle/yolo_oracle.py (Modules/Head.cs:89-127, 245-357; Utils/Loss.cs:1179-1236; Utils/Tal.cs:242-250;
Utils/Ops.cs:258-267).  fp32 tolerance 1e-3; the post-process and the second assigner stage are compared exactly."""
import functools
import os

import numpy as np
import pytest
import torch

import e2e_seg_ref as R
from conftest import BACKENDS
from oracle import yolo_oracle as O
from test_model import assert_pred_blocks, relerr
from test_segment import make_ref

B, H, W, NC, NM = 2, 64, 64, 80, 32      # the tests/test_segment.py case: A = 84
HERE = os.path.dirname(os.path.abspath(__file__))
HEAD_KEYS = ("boxes", "scores", "mask_coefficient")


def _cls(family):
    from yolosharp_amd import model as M
    return M.Yolov8Segment if family == 8 else M.Yolov11Segment


def _engine_model(engine, sd, family, end2end=True, dtype="f32", max_det=300, h=H, w=W, b=B, epochs=100, size="n"):
    m = _cls(family)(engine, nc=NC, size=size, height=h, width=w, max_batch=b, dtype=dtype)
    if end2end:
        m.e2e_init(max_det, epochs)
    m.load_state_dict(sd)
    return m


def _np(d):
    return {k: v.numpy() for k, v in d.items()}


def _oracle_step(family, size, b, h, w):
    """One End2End Segment step of the oracle: everything the tests compare against, never modified afterwards."""
    net = make_ref(family, NC, size)
    sd0 = {k: v.detach().clone().numpy() for k, v in net.state_dict().items()}
    x = torch.rand(b, 3, h, w, generator=torch.Generator().manual_seed(3))
    batch = O.synthetic_batch(b, h, w, NC, seed=1, kmax=6)
    batch["masks"] = O.synthetic_masks(batch, b, h // 4, w // 4)
    ref = R.E2ESeg(net).train()
    _, rpreds = ref(x)
    for br in ("one2many", "one2one"):
        for k in HEAD_KEYS:
            rpreds[br][k].retain_grad()
    rpreds["one2many"]["proto"].retain_grad()
    crit = R.E2ESegmentLoss(NC)
    rloss, ritems = crit(rpreds, batch)
    rloss.sum().backward()
    dhead = {(br, k): rpreds[br][k].grad.numpy() for br in ("one2many", "one2one") for k in HEAD_KEYS}
    return dict(net=net, crit=crit, sd0=sd0, x=x, batch=batch, rpreds=rpreds, items=ritems.numpy(), loss=rloss.detach().numpy(), dhead=dhead,
                dproto=rpreds["one2many"]["proto"].grad.numpy(),
                grads={n: p.grad.numpy() for n, p in net.named_parameters() if p.grad is not None},
                sd1={k: v.detach().clone().numpy() for k, v in net.state_dict().items()})


@functools.lru_cache(maxsize=None)
def _case(family):
    ev = R.E2ESeg(make_ref(family, NC, "n")).eval()
    x = torch.rand(B, 3, H, W, generator=torch.Generator().manual_seed(3))
    with torch.no_grad():
        rinf, _ = ev(x)
    c = _oracle_step(family, "n", B, H, W)
    rp, crit = c.pop("rpreds"), c.pop("crit")
    # ---- the fixture must exercise the second assigner stage: several boxes, each pruned from more than one positive to one, no tie at the cut
    asg = crit.one2one.assigner
    before = asg.fg_before.sum().item()
    vals = asg.align_before * asg.mask_before
    rows = asg.mask_before.sum(-1) > 0
    top2 = torch.sort(vals, dim=-1, descending=True).values[..., :2][rows]
    gaps = ((top2[:, 0] - top2[:, 1]) / top2[:, 0])[asg.mask_before.sum(-1)[rows] > 1]
    with torch.no_grad():
        _, _, tg = O.v8DetectionLoss.__call__(crit.one2one, rp["one2one"], c["batch"], return_targets=True)
    after = int(tg["fg_mask"].sum())
    # the items with the gains two update() calls of a 5-epoch schedule leave (test_gains)
    c2 = R.E2ESegmentLoss(NC, epochs=5)
    c2.update(); c2.update()
    with torch.no_grad():
        _, items2 = c2({br: {k: (v.detach() if torch.is_tensor(v) else [f.detach() for f in v]) for k, v in rp[br].items()} for br in rp}, c["batch"])
    c.update(x=c["x"].numpy(), batch=_np(c["batch"]), pred=rinf["pred"].numpy(), rows=rinf["boxes"].numpy(),
             preds={k: rp["one2many"][k].detach().numpy() for k in HEAD_KEYS + ("proto",)},
             fg_before=int(before), fg_after=after, n_boxes=int(rows.sum()), min_gap=float(gaps.min()) if len(gaps) else 0.0,
             items2=items2.numpy(), gains2=(float(c2.o2m), float(c2.o2o)),
             head="model.22" if family == 8 else "model.23")
    c.pop("net")
    return c


def _step(m, c, backward="whole"):
    from yolosharp_amd.model import v8SegmentationLoss
    m.train(); m.zero_grad()
    _, preds = m.forward(c["x"])
    loss, items = v8SegmentationLoss(m)(None, c["batch"])
    if backward == "whole":
        m.backward()
    elif backward is not None:
        for seg in range(m.num_segments()):
            if backward == "async":
                m.backward_segment_async(seg); m.segment_fence(seg, 0)
            else:
                m.backward_segment(seg)
    return preds, loss, items


@pytest.mark.parametrize("family", [8, 11])
def test_fixture_exercises_the_second_stage(family):
    """A changed fixture must not silently turn the second assigner stage into a no-op."""
    c = _case(family)
    assert c["fg_before"] > c["fg_after"] == c["n_boxes"] >= 3, (c["fg_before"], c["fg_after"], c["n_boxes"])
    assert c["min_gap"] > 1e-2, c["min_gap"]          # far above fp32 noise: the kept anchor cannot flip between engine and oracle


# ---------------------------------------------------------------------------------------------------- 1: ys_tal_keep_best
@pytest.mark.parametrize("backend", BACKENDS)
def test_tal_keep_best_exact(backend, engine):
    g = torch.Generator().manual_seed(11)
    for b, gg, a, counts in ((2, 5, 84, [3, 4]), (1, 3, 1344, [2])):
        align = torch.rand(b, gg, a, generator=g)
        mask = (torch.rand(b, gg, a, generator=g) < 0.1).float()
        mask[0, 0] = 0                                                        # a live row without any positive stays empty
        want = R.keep_best(align, mask, counts).numpy().astype(np.uint8)
        got = engine.tal_keep_best(align.numpy(), mask.numpy(), counts)
        assert np.array_equal(got, want)
        for i, n in enumerate(counts):
            assert np.all(got[i, :n].sum(-1) <= 1) and got[i, 1:n].sum() > 0
            assert np.array_equal(got[i, n:], mask.numpy().astype(np.uint8)[i, n:]) and got[i, n:].sum() > got.shape[2] // 20   # rows >= gt_count: untouched
    # constructed rows, A = 300 (more than one trip of the 256-thread workgroup)
    a = 300
    align = np.zeros((1, 4, a), np.float32); mask = np.zeros((1, 4, a), np.uint8)
    align[0, 0, [7, 290]] = 0.5; mask[0, 0, [7, 290]] = 1; align[0, 0, 100] = 0.9          # equal positives: the lower index; a larger non-positive is ignored
    mask[0, 1, [5, 9]] = 1                                                                  # all metrics 0, anchor 0 not a positive: the row ends empty
    mask[0, 2, [0, 5, 9]] = 1                                                               # the same with anchor 0 positive: anchor 0 is kept
    mask[0, 3, [1, 2]] = 1; align[0, 3, [1, 2]] = (0.2, 0.3)                                # beyond gt_count: untouched
    got = engine.tal_keep_best(align, mask, [3])
    assert np.array_equal(got, R.keep_best(torch.from_numpy(align), torch.from_numpy(mask), [3]).numpy().astype(np.uint8))
    assert np.flatnonzero(got[0, 0]).tolist() == [7] and got[0, 1].sum() == 0 and np.flatnonzero(got[0, 2]).tolist() == [0]
    assert np.flatnonzero(got[0, 3]).tolist() == [1, 2]


# ---------------------------------------------------------------------------------------------------- 2: training forward, running statistics
@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("family", [8, 11])
def test_training_forward_and_running_statistics(backend, engine, family):
    c = _case(family)
    m = _engine_model(engine, c["sd0"], family)
    m.train()
    inf, preds = m.forward(c["x"])
    assert inf is None and set(preds) == {"one2many", "one2one"}
    for k in HEAD_KEYS + ("proto",):
        assert relerr(preds["one2many"][k], c["preds"][k]) < 1e-3, k
        assert np.array_equal(preds["one2one"][k], preds["one2many"][k]), k                 # same modules, same input values
    sd = m.state_dict()
    n_tower = n_proto = n_trunk = 0
    for k, r in c["sd1"].items():
        if "running" in k:
            assert np.allclose(sd[k], r, rtol=1e-3, atol=1e-5), k
        elif "num_batches_tracked" in k:
            tower = k.startswith(c["head"] + ".cv")
            assert float(sd[k].reshape(-1)[0]) == float(r) == (2.0 if tower else 1.0), k    # cv2 / cv3 / cv4: two updates; Proto and the trunk: one
            n_tower += tower; n_proto += ".proto." in k; n_trunk += not k.startswith(c["head"] + ".")
    assert n_tower >= 18 and n_proto == 3 and n_trunk > 20
    assert sum(1 for k in c["sd1"] if k.startswith(c["head"] + ".cv4.") and "num_batches_tracked" in k) == 6
    # a single update of a cv4 unit is NOT within the tolerance: the check above separates one update from two
    k = c["head"] + ".cv4.0.0.bn.running_mean"
    once = c["sd0"][k] + (c["sd1"][k] - c["sd0"][k]) / 1.97                                 # r1 from r2 = r1 + 0.97 (r1 - r0)
    assert not np.allclose(once, c["sd1"][k], rtol=1e-3, atol=1e-5)
    m.close()


# ---------------------------------------------------------------------------------------------------- 3: loss, head gradients, backward
def _check_loss_and_backward(engine, c, m, family, plain, tol):
    _, loss, items = _step(m, c)
    print("items", items, c["items"], "loss", loss, c["loss"])
    assert items.shape == (5,) and np.allclose(items, c["items"], rtol=1e-3, atol=1e-5), (items, c["items"])
    assert np.allclose(loss, c["loss"], rtol=1e-3, atol=1e-4), (loss, c["loss"])
    got = {}
    for br, pre in (("one2many", "d"), ("one2one", "one2one_d")):
        for k in HEAD_KEYS:
            r = c["dhead"][(br, k)]
            got[(br, k)] = g = m.get_output(pre + k)
            print(br, k, np.abs(g - r).max(), np.abs(r).max())
            assert np.abs(r).max() > 0 and np.abs(g - r).max() <= tol * np.abs(r).max(), (br, k, np.abs(g - r).max(), np.abs(r).max())
    g = m.get_output("dproto")
    assert np.abs(c["dproto"]).max() > 0 and np.abs(g - c["dproto"]).max() <= tol * np.abs(c["dproto"]).max()
    for k in HEAD_KEYS:                    # other assignment, other gain: the two branches' gradients differ
        d = np.abs(got[("one2one", k)] - got[("one2many", k)]).max()
        assert d > 1e-2 * np.abs(got[("one2many", k)]).max(), k
    grads = m.grads()
    gscale = max(float(np.abs(r).max()) for r in c["grads"].values())
    assert len(c["grads"]) > 100
    for name, r in c["grads"].items():
        err = np.abs(grads[name] - r).max()
        assert err <= tol * np.abs(r).max() + 1e-6 * gscale, (name, err, np.abs(r).max())
    if plain is None:
        return
    # the trunk and Proto see o2m = 0.8 times what a model without the one2one branch sends into them for the same batch ...
    _step(plain, c)
    pg = plain.grads()
    last_neck = "model.21.cv2.conv.weight" if family == 8 else "model.22.cv2.conv.weight"
    o2m = np.float32(0.8)
    for name in ("model.0.conv.weight", last_neck, c["head"] + ".proto.cv1.conv.weight"):
        assert np.abs(pg[name]).max() > 0
        assert np.abs(grads[name] - o2m * pg[name]).max() <= 1e-5 * np.abs(o2m * pg[name]).max(), name
    # ... while a cv4 tower also carries the one2one gradient
    tw = c["head"] + ".cv4.0.2.weight"
    assert np.abs(grads[tw] - o2m * pg[tw]).max() > 1e-2 * np.abs(pg[tw]).max()


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("family", [8, 11])
def test_loss_and_backward(backend, engine, family):
    c = _case(family)
    m = _engine_model(engine, c["sd0"], family)
    assert m.e2e_gains() == pytest.approx((0.8, 0.2), abs=1e-7)
    p = _engine_model(engine, c["sd0"], family, end2end=False)
    _check_loss_and_backward(engine, c, m, family, p, 1e-3)
    p.close(); m.close()


# ---------------------------------------------------------------------------------------------------- 4: gains
def _formula(updates, epochs):
    f = np.float32
    o2m = f(max(f(1) - f(updates) / f(max(epochs - 1, 1)), f(0))) * (f(0.8) - f(0.1)) + f(0.1)
    return float(o2m), float(max(f(1) - o2m, f(0)))


@pytest.mark.parametrize("backend", BACKENDS)
def test_gains(backend, engine):
    from yolosharp_amd import model as M
    from yolosharp_amd.trainer import Trainer
    c = _case(8)
    m = _engine_model(engine, c["sd0"], 8, epochs=5)
    assert m.e2e_gains() == pytest.approx((0.8, 0.2), abs=1e-7)
    done = 0
    for n in (1, 2, 4, 6):
        while done < n:
            m.e2e_update(); done += 1
        assert m.e2e_gains() == pytest.approx(_formula(n, 5), abs=1e-6), n
        if n == 2:     # the criterion uses the moved gains (preds fed through ys_model_set_preds: no forward needed)
            assert m.e2e_gains() == pytest.approx(c["gains2"], abs=1e-6) and abs(c["gains2"][0] - 0.8) > 0.1
            m.set_preds(c["preds"])
            _, items = M.v8SegmentationLoss(m)(None, c["batch"])
            assert np.allclose(items, c["items2"], rtol=1e-3, atol=1e-5), (items, c["items2"])
            assert not np.allclose(items, c["items"], rtol=1e-3, atol=1e-5)
    assert m.e2e_gains() == pytest.approx((0.1, 0.9), abs=1e-6)      # past the schedule's end
    m.close()
    # Trainer never steps the schedule of a Segment run (YoloBaseTaskModel.cs:350-353 updates E2EOBBLoss only)
    m = _engine_model(engine, c["sd0"], 8, dtype="bf16", epochs=2)
    data = dict(c["batch"]); data["images"] = c["x"]
    hist = Trainer(m, epochs=2, nb=1).fit(lambda: [data])
    assert len(hist) == 2 and all(np.all(np.isfinite(h["train_loss"])) and h["train_loss"].shape == (5,) for h in hist)
    assert m.e2e_gains() == pytest.approx((0.8, 0.2), abs=1e-7)
    m.close()
    # Detect End2End: unweighted, update() changes nothing, the items of tests/test_e2e.py's case are reproduced
    import test_e2e as TE
    d = TE._case(8)
    for init in ("ctor", "e2e_init"):
        dm = M.Yolov8(engine, nc=TE.NC, size="n", height=TE.H, width=TE.W, max_batch=TE.B, dtype="f32", end2end=init == "ctor")
        if init == "e2e_init":
            dm.e2e_init(300, 5)
        assert dm.e2e_gains() == (1.0, 1.0)
        dm.e2e_update(); dm.e2e_update()
        assert dm.e2e_gains() == (1.0, 1.0)
        dm.set_preds({"boxes": d["boxes"], "scores": d["scores"]})
        _, items = M.v8DetectionLoss(dm)(None, d["batch"])
        assert np.allclose(items, d["items"], rtol=1e-3, atol=1e-5), (init, items, d["items"])
        if init == "ctor":
            first = items.copy()
        else:
            assert np.array_equal(items, first)                        # the two entry points are one code path
        dm.close()


# ---------------------------------------------------------------------------------------------------- 5: backward forms, determinism
@pytest.mark.parametrize("backend", BACKENDS)
def test_backward_forms_agree_and_steps_repeat(backend, engine):
    c = _case(8)
    res = {}
    for mode in ("whole", "sync", "async", "again"):
        m = _engine_model(engine, c["sd0"], 8, dtype="bf16")
        _, _, items = _step(m, c, backward="whole" if mode == "again" else mode)
        res[mode] = ({k: v.copy() for k, v in m.grads().items()}, items.copy(), m.get_output("one2one_dmask_coefficient"), m.get_output("dproto"))
        m.close()
    for mode in ("sync", "async", "again"):
        for k, v in res["whole"][0].items():
            assert np.array_equal(v, res[mode][0][k]), (mode, k)
        for i in (1, 2, 3):
            assert np.array_equal(res["whole"][i], res[mode][i]), (mode, i)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("family", [8, 11])
def test_second_step_on_one_model_repeats_the_gradients(backend, engine, family):
    """Two consecutive steps on ONE model without an optimizer step (zero_grad, forward, criterion, backward): training-mode gradients do not depend on the
    running statistics, so the second step's gradients are the first's, bit for bit.  The one2one backward pass skips Proto's units; whatever it leaves
    behind from the previous step (split-reduction descriptors, partial regions) must not reach this step's Proto gradients."""
    from yolosharp_amd import YsError
    c = _case(family)
    m = _engine_model(engine, c["sd0"], family)
    _step(m, c)
    g1 = {k: v.copy() for k, v in m.grads().items()}
    for mode in ("whole", "sync"):
        _step(m, c, backward=mode)
        g2 = m.grads()
        for k, v in g1.items():
            assert np.array_equal(v, g2[k]), (mode, k, float(np.abs(v - g2[k]).max()), float(np.abs(v).max()))
    names = [c["head"] + ".proto.%s.conv.weight" % u for u in ("cv1", "cv2", "cv3")] + [c["head"] + ".proto.upsample.weight", c["head"] + ".cv4.0.2.weight"]
    gscale = max(float(np.abs(r).max()) for r in c["grads"].values())
    for k in names:                              # ... and still the oracle's
        r = c["grads"][k]
        assert np.abs(r).max() > 0 and np.abs(g2[k] - r).max() <= 1e-3 * np.abs(r).max() + 1e-6 * gscale, k
    p = _engine_model(engine, c["sd0"], family, end2end=False)
    _step(p, c)
    pg = p.grads()
    for k in names[:4]:                          # Proto on step 3 of the End2End model = 0.8 x a plain Segment model's
        assert np.abs(g2[k] - np.float32(0.8) * pg[k]).max() <= 1e-5 * np.abs(np.float32(0.8) * pg[k]).max(), k
    # ys_loss_segment is the only criterion entry of an End2End Segment model
    from yolosharp_amd.model import v8DetectionLoss
    with pytest.raises(YsError) as e:
        v8DetectionLoss(m)(None, c["batch"])
    assert e.value.status == 1 and "ys_loss_segment" in str(e.value)
    v8DetectionLoss(p)(None, c["batch"], read=False)       # a plain Segment model still takes the detect criterion alone, as before
    p.close(); m.close()


# ---------------------------------------------------------------------------------------------------- 6: ys_e2e_topk_ex
def _tie_free(b, nc, extra, a, seed):
    g = np.random.default_rng(seed)
    n = nc * a
    vals = ((np.arange(n, dtype=np.float64) + 0.5) / n).astype(np.float32)
    assert len(np.unique(vals)) == n
    pred = np.empty((b, 4 + nc + extra, a), np.float32)
    pred[:, :4] = g.random((b, 4, a), dtype=np.float32) * 640
    for i in range(b):
        pred[i, 4:4 + nc] = g.permutation(vals).reshape(nc, a)
    pred[:, 4 + nc:] = g.standard_normal((b, extra, a), dtype=np.float32) * 3      # coefficients are unbounded and signed
    return pred


def _check_topk_ex(engine, pred, nc, extra, max_det):
    rows, anchor = engine.e2e_topk(pred, max_det, extra=extra)
    rrows, ridx = R.postprocess(torch.from_numpy(pred), nc, max_det)
    k = min(max_det, pred.shape[2])
    assert rows.shape == (pred.shape[0], k, 6 + extra) and anchor.shape == (pred.shape[0], k)
    assert np.array_equal(anchor, ridx.numpy())
    assert np.array_equal(rows.view(np.uint32), rrows.numpy().view(np.uint32))       # bit-equal boxes, scores, classes and coefficients
    return rows, anchor


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("b,a,nc,extra,max_det", [(2, 1344, 7, 32, 300), (1, 84, 80, 32, 300), (2, 336, 3, 5, 17)])
def test_e2e_topk_ex_exact(backend, engine, b, a, nc, extra, max_det):
    pred = _tie_free(b, nc, extra, a, seed=a + nc)
    rows, anchor = _check_topk_ex(engine, pred, nc, extra, max_det)
    assert np.all(np.diff(rows[..., 4], axis=1) < 0)
    # extra = 0 is ys_e2e_topk bit for bit, and the leading six columns do not depend on the extra channels
    p0 = np.ascontiguousarray(pred[:, :4 + nc])
    r0, a0 = engine.e2e_topk(p0, max_det)
    rz, az = np.zeros_like(r0), np.zeros_like(a0)
    from yolosharp_amd import _lib
    from yolosharp_amd.engine import _ptr
    _lib.check(engine.lib, engine.lib.ys_e2e_topk_ex(engine.ctx, _ptr(p0), 0, b, nc, 0, a, max_det, _ptr(rz), _ptr(az)))
    assert np.array_equal(r0.view(np.uint32), rz.view(np.uint32)) and np.array_equal(a0, az)
    assert np.array_equal(rows[..., :6].view(np.uint32), r0.view(np.uint32)) and np.array_equal(anchor, a0)


@pytest.mark.parametrize("backend", BACKENDS)
def test_e2e_topk_ex_ties_carry_the_right_anchor(backend, engine):
    g = np.random.default_rng(9)
    b, a, nc, extra = 2, 336, 3, 5
    pred = np.zeros((b, 4 + nc + extra, a), np.float32)
    pred[:, :4] = g.random((b, 4, a), dtype=np.float32) * 64
    pred[:, 4:4 + nc] = g.integers(0, 6, (b, nc, a)).astype(np.float32) / 8
    pred[1, 4:4 + nc] = 0.5
    pred[:, 4 + nc:] = np.arange(a, dtype=np.float32)[None, None, :] + np.arange(extra, dtype=np.float32)[None, :, None] / 8   # channel j of anchor i = i + j / 8
    for max_det in (300, 5):
        rows, anchor = _check_topk_ex(engine, pred, nc, extra, max_det)
        assert np.array_equal(rows[..., 6:], anchor[..., None].astype(np.float32) + np.arange(extra, dtype=np.float32) / 8)
        assert np.array_equal(anchor[1], np.arange(min(max_det, 300)) // nc)          # all equal: anchors 0, 0, 0, 1, ... -- the lower index first


@pytest.mark.gpu
def test_e2e_topk_ex_exact_large():
    from yolosharp_amd import Engine
    _check_topk_ex(Engine(), _tie_free(2, 80, 32, 8400, seed=8400), 80, 32, 300)


# ---------------------------------------------------------------------------------------------------- 7: eval forward, Segmenter
def _bus(backend):
    """tests/golden/bus_480x640.jpg as uint8 [3, h, w]: the whole picture on the GPU, its 64 x 48 centre crop through the interpreter."""
    from PIL import Image
    im = np.asarray(Image.open(os.path.join(HERE, "golden", "bus_480x640.jpg")).convert("RGB"), np.uint8)
    im = np.ascontiguousarray(im.transpose(2, 0, 1))
    return im if backend == "gpu" else np.ascontiguousarray(im[:, 288:352, 216:264])


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("family", [8, 11])
def test_eval_forward(backend, engine, family):
    c = _case(family)
    m = _engine_model(engine, c["sd0"], family)
    m.eval()
    inf, preds = m.forward(c["x"])
    k = min(300, m.A)
    assert set(inf) == {"boxes", "pred", "proto"} and set(preds) == {"one2many", "one2one"}
    assert inf["pred"].shape == (B, 4 + NC + NM, m.A) and inf["boxes"].shape == (B, k, 6 + NM)
    assert relerr(inf["pred"][:, :4 + NC], c["pred"][:, :4 + NC]) < 1e-3 and relerr(inf["pred"][:, 4 + NC:], c["pred"][:, 4 + NC:]) < 1e-3
    assert_pred_blocks(inf["pred"], c["pred"], NC, 1e-3, tag="e2e seg v%d" % family)        # boxes and probabilities apart too
    assert np.all(inf["pred"][:, 2] > inf["pred"][:, 0]) and np.all(inf["pred"][:, 3] > inf["pred"][:, 1])      # xyxy
    rows, _ = engine.e2e_topk(inf["pred"], 300, extra=NM)                      # "det" IS ys_e2e_topk_ex of the engine's own pred ...
    assert np.array_equal(inf["boxes"].view(np.uint32), rows.view(np.uint32))
    rrows, _ = R.postprocess(torch.from_numpy(inf["pred"]), NC)                # ... which is the restatement's post-process, exactly
    assert np.array_equal(inf["boxes"].view(np.uint32), rrows.numpy().view(np.uint32))
    assert relerr(np.sort(inf["boxes"][..., 4], 1), np.sort(c["rows"][..., 4], 1)) < 1e-3
    for conf in (0.0, float(np.median(rows[..., 4])), 0.999):
        for max_det in (300, 17):
            want = [len(r) for r in R.select(torch.from_numpy(rows), conf, max_det)]
            assert engine.e2e_select(rows, conf, max_det).tolist() == want, (conf, max_det)
    m.close()


@pytest.mark.parametrize("backend", BACKENDS)
def test_segmenter_end2end_predict_and_val(backend, engine):
    from yolosharp_amd.detector import Segmenter, YoloResult, clip_boxes, pad_to_32
    c = _case(8)
    img = _bus(backend)
    ih, iw = img.shape[1:]
    h, w = (ih + 31) // 32 * 32, (iw + 31) // 32 * 32
    m = _engine_model(engine, c["sd0"], 8, h=h, w=w, b=1)
    seg = Segmenter(m)
    assert seg.end2end
    res = seg.ImagePredict(img, predict_threshold=0.001)
    m.eval()
    inf, _ = m.forward(pad_to_32(img.astype(np.float32))[None])
    want = R.select(R.postprocess(torch.from_numpy(inf["pred"]), NC)[0], 0.001)[0]
    assert 0 < len(want) == len(res)
    wmasks = O.process_mask(torch.from_numpy(inf["proto"][0]), want[:, 6:], want[:, :4].clone(), (h, w), upsample=True).numpy().astype(bool)[:, :ih, :iw]
    wb = want.numpy().copy()
    wb[:, :4] = clip_boxes(wb[:, :4], (ih, iw))
    mism = 0
    for (r, mk), wr, wm in zip(res, wb, wmasks):
        e = YoloResult(wr)
        assert (r.ClassID, r.Score, r.CenterX, r.CenterY, r.Width, r.Height) == (e.ClassID, e.Score, e.CenterX, e.CenterY, e.Width, e.Height)
        assert mk.shape == wm.shape == (ih, iw)
        mism += int((mk != wm).sum())
    assert mism <= 1e-3 * wmasks.size                   # '> 0' on a float sum: sign flips at rounding level only (tests/test_segment.py::test_process_mask)
    m.close()
    # ---- Val on the End2End model: thresholded head rows -> process_mask / mask_iou; finite loss items (E2ESegmentLoss on the eval preds) and metrics
    m = _engine_model(engine, c["sd0"], 8)
    data = dict(c["batch"]); data["images"] = c["x"]
    loss_items, box, mask = Segmenter(m).Val([data], conf_thres=0.001)
    assert loss_items.shape == (5,) and np.all(np.isfinite(loss_items)) and loss_items[1] > 0
    assert len(box) == len(mask) == 4 and np.all(np.isfinite(box)) and np.all(np.isfinite(mask))
    m.close()


# ---------------------------------------------------------------------------------------------------- 8: boundaries
@pytest.mark.parametrize("backend", BACKENDS)
def test_boundaries(backend, engine, tmp_path):
    from yolosharp_amd import YsError, weights_bin
    from yolosharp_amd import model as M
    for cls in (M.Yolov8Obb, M.Yolov11Pose, M.Yolov8Classify):
        mm = cls(engine, nc=NC, size="n", height=32, width=32, max_batch=1, dtype="f32")
        with pytest.raises(YsError) as e:
            mm.e2e_init()
        assert e.value.status == 4, cls                                               # YS_ERR_UNSUPPORTED
        mm.close()
    with pytest.raises(YsError) as e:                                                  # the old entry keeps refusing Segment models
        M.Yolov8Segment(engine, nc=NC, size="n", height=32, width=32, max_batch=1, dtype="f32", end2end=True)
    assert e.value.status == 4
    c = _case(8)
    e2e = _engine_model(engine, c["sd0"], 8)
    with pytest.raises(YsError) as e:
        e2e.e2e_init()                                                                # once
    assert e.value.status == 5                                                        # YS_ERR_STATE
    with pytest.raises(YsError):
        e2e.one2one_init()
    plain = M.Yolov8Segment(engine, nc=NC, size="n", height=H, width=W, max_batch=B, dtype="f32")
    assert e2e.tensor_info() == plain.tensor_info() and e2e.num_params() == plain.num_params()
    # `.bin` round trip: E2E -> plain -> E2E
    f1, f2 = str(tmp_path / "e2e.bin"), str(tmp_path / "plain.bin")
    weights_bin.save_from(e2e, f1); weights_bin.load_into(plain, f1)
    psd = plain.state_dict()
    for k, v in e2e.state_dict().items():
        assert np.array_equal(v, psd[k]), k
    e2e.init_weights(7)
    assert not np.array_equal(e2e.state_dict()["model.0.conv.weight"], psd["model.0.conv.weight"])
    weights_bin.save_from(plain, f2); weights_bin.load_into(e2e, f2)
    esd = e2e.state_dict()
    assert all(np.array_equal(v, esd[k]) for k, v in psd.items())
    # a plain Segment model behaves as before: xywh "pred", one criterion pass, the new keys refused
    plain.eval()
    inf, preds = plain.forward(c["x"])
    assert set(inf) == {"boxes", "proto"} and set(preds) == {"boxes", "scores", "mask_coefficient", "proto"}
    e2e.eval()
    einf, _ = e2e.forward(c["x"])
    xyxy = einf["pred"][:, :4]
    assert np.allclose(inf["boxes"][:, 0], (xyxy[:, 0] + xyxy[:, 2]) / 2, rtol=1e-5, atol=1e-4) and np.allclose(inf["boxes"][:, 2], xyxy[:, 2] - xyxy[:, 0], rtol=1e-5, atol=1e-4)
    assert np.array_equal(inf["boxes"][:, 4:], einf["pred"][:, 4:])
    for key in ("det", "one2one_boxes", "one2one_mask_coefficient", "one2one_dmask_coefficient"):
        with pytest.raises(YsError):
            plain.get_output(key)
    for fn in (plain.det_device, plain.e2e_gains, plain.e2e_update):
        with pytest.raises(YsError):
            fn()
    plain.set_preds(c["preds"])
    _, pitems = M.v8SegmentationLoss(plain)(None, c["batch"])
    rp = {k: torch.from_numpy(v) for k, v in c["preds"].items()}
    rp["feats"] = [torch.zeros(B, 1, H // s, W // s) for s in (8, 16, 32)]
    _, ritems = O.v8SegmentationLoss(NC)(rp, {k: torch.from_numpy(v) for k, v in c["batch"].items()})
    assert np.allclose(pitems, ritems.numpy(), rtol=1e-3, atol=1e-5), (pitems, ritems)       # one pass, unweighted
    # ys_model_set_preds feeds both branches
    e2e.set_preds(c["preds"])
    _, items = M.v8SegmentationLoss(e2e)(None, c["batch"])
    assert np.allclose(items, c["items"], rtol=1e-3, atol=1e-5), (items, c["items"])
    for k in HEAD_KEYS:
        assert np.array_equal(e2e.get_output("one2one_" + k), e2e.get_output(k))
    for m in (e2e, plain):
        m.close()


# ---------------------------------------------------------------------------------------------------- 9: bf16
@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("family", [8, 11])
def test_bf16_three_steps_descend(backend, engine, family):
    from yolosharp_amd.model import v8SegmentationLoss
    c = _case(family)
    m = _engine_model(engine, c["sd0"], family, dtype="bf16")
    m.train()
    crit = v8SegmentationLoss(m)
    sums = []
    for _ in range(3):
        m.forward(c["x"], fetch=False)
        loss, items = crit(None, c["batch"])
        assert np.all(np.isfinite(items))
        sums.append(float(loss.sum()))
        m.zero_grad(); m.backward(); m.adamw_step([1e-3] * 3)
    assert np.allclose(sums[0], c["loss"].sum(), rtol=5e-2), (sums, c["loss"].sum())
    assert sums[2] < sums[0], sums
    m.close()


# ---------------------------------------------------------------------------------------------------- 10: full resolution
@pytest.mark.gpu
@pytest.mark.parametrize("backend", ["gpu"])
def test_yolov11s_segment_e2e_full_resolution_f32(backend, engine):
    c = _oracle_step(11, "s", 2, 640, 640)
    c.update(x=c["x"].numpy(), batch=_np(c["batch"]), head="model.23")
    m = _engine_model(engine, c["sd0"], 11, h=640, w=640, size="s")
    _check_loss_and_backward(engine, c, m, 11, None, 2e-3)
    m.close()
