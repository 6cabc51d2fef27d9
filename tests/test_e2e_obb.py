"""End2End for OBB models (ys_model_e2e_obb_init): aliased cv2 / cv3 / cv4 towers, E2EOBBLoss (gains, the rotated assigner + tal_topk2 = 1), the
two-pass head backward, the top-k post-process with the angle, the gain schedule stepped by Trainer, Obber on an End2End model with the batched
ys_val_match_rotated_batched, the task boundary.
Oracle = tests/e2e_obb_ref.py over oracle/yolo_oracle.py (Modules/Head.cs:89-127, 434-469; Utils/Loss.cs:1120-1177; Utils/Tal.cs:242-310;
Models/Obber.cs:94-114).  fp32 tolerances are those of tests/test_obb_pose.py::_obb_train_parity; post-process and matching are compared exactly."""
import functools

import numpy as np
import pytest
import torch

import e2e_obb_ref as R
import e2e_seg_ref as S
from conftest import BACKENDS
from oracle import yolo_oracle as O
from test_model import assert_pred_blocks, relerr
from test_obb_pose import make_ref

B, H, W, NC = 2, 64, 64, 15               # A = 84
HEAD = (("boxes", "boxes"), ("scores", "scores"), ("angle", "angle_raw"))     # engine key, oracle key (the engine's angle gradient is w.r.t. the logit)


def _cls(family):
    from yolosharp_amd import model as M
    return M.Yolov8Obb if family == 8 else M.Yolov11Obb


def _engine_model(engine, sd, family, end2end=True, dtype="f32", max_det=300, h=H, w=W, b=B, epochs=100, size="n"):
    m = _cls(family)(engine, nc=NC, size=size, height=h, width=w, max_batch=b, dtype=dtype)
    if end2end:
        m.e2e_obb_init(max_det, epochs)
    m.load_state_dict(sd)
    return m


def _np(d):
    return {k: v.numpy() for k, v in d.items()}


def _detached(rp):
    return {br: {k: (v.detach() if torch.is_tensor(v) else [f.detach() for f in v]) for k, v in rp[br].items()} for br in rp}


def _oracle_step(family, size, b, h, w, kmax):
    """One End2End OBB step of the oracle: everything the tests compare against, never modified afterwards."""
    net = make_ref(getattr(O, f"Yolov{family}Obb"), NC, size)
    sd0 = {k: v.detach().clone().numpy() for k, v in net.state_dict().items()}
    x = torch.rand(b, 3, h, w, generator=torch.Generator().manual_seed(3))
    batch = O.synthetic_obb_batch(b, h, w, NC, seed=1, kmax=kmax)
    ref = R.E2EObb(net).train()
    _, rpreds = ref(x)
    for br in ("one2many", "one2one"):
        for _, rk in HEAD:
            rpreds[br][rk].retain_grad()
    crit = R.E2EOBBLoss(NC)
    rloss, ritems = crit(rpreds, batch)
    rloss.sum().backward()
    asg = crit.one2one.assigner
    # the second assigner stage on this fixture: positives before / after, rows pruned from several positives, the relative gap at the cut
    vals = asg.align_before * asg.mask_before
    rows = asg.mask_before.sum(-1) > 0
    top2 = torch.sort(vals, dim=-1, descending=True).values[..., :2][rows]
    gaps = ((top2[:, 0] - top2[:, 1]) / top2[:, 0])[asg.mask_before.sum(-1)[rows] > 1]
    dhead = {(br, k): rpreds[br][rk].grad.numpy() for br in ("one2many", "one2one") for k, rk in HEAD}
    return dict(net=net, crit=crit, sd0=sd0, x=x, batch=batch, rpreds=rpreds, items=ritems.numpy(), loss=rloss.detach().numpy(), dhead=dhead,
                fg_before=int(asg.fg_before.sum()), fg_after=int(asg.fg_after.sum()), n_boxes=int(rows.sum()),
                n_multi=int((asg.mask_before.sum(-1)[rows] > 1).sum()), min_gap=float(gaps.min()) if len(gaps) else 0.0,
                grads={n: p.grad.numpy() for n, p in net.named_parameters() if p.grad is not None},
                sd1={k: v.detach().clone().numpy() for k, v in net.state_dict().items()},
                head="model.22" if family == 8 else "model.23")


@functools.lru_cache(maxsize=None)
def _case(family):
    ev = R.E2EObb(make_ref(getattr(O, f"Yolov{family}Obb"), NC, "n")).eval()
    x = torch.rand(B, 3, H, W, generator=torch.Generator().manual_seed(3))
    with torch.no_grad():
        rinf, _ = ev(x)
    c = _oracle_step(family, "n", B, H, W, 8)
    rp, crit = c.pop("rpreds"), c.pop("crit")
    # the items with the gains two update() calls of a 5-epoch schedule leave (test_gains)
    c2 = R.E2EOBBLoss(NC, epochs=5)
    c2.update(); c2.update()
    with torch.no_grad():
        _, items2 = c2(_detached(rp), c["batch"])
        _, plain_items = O.v8OBBLoss(NC)(_detached(rp)["one2many"], c["batch"])
    c.update(x=c["x"].numpy(), batch=_np(c["batch"]), pred=rinf["pred"].numpy(), rows=rinf["boxes"].numpy(),
             preds={k: rp["one2many"][k].detach().numpy() for k in ("boxes", "scores", "angle")},
             items2=items2.numpy(), gains2=(float(c2.o2m), float(c2.o2o)), plain_items=plain_items.numpy())
    c.pop("net")
    return c


def _step(m, c, backward="whole"):
    from yolosharp_amd.model import v8OBBLoss
    m.train(); m.zero_grad()
    _, preds = m.forward(c["x"])
    loss, items = v8OBBLoss(m)(None, c["batch"])
    if backward == "whole":
        m.backward()
    elif backward is not None:
        for seg in range(m.num_segments()):
            if backward == "async":
                m.backward_segment_async(seg); m.segment_fence(seg, 0)
            else:
                m.backward_segment(seg)
    return preds, loss, items


# ---------------------------------------------------------------------------------------------------- 1: the fixture
@pytest.mark.parametrize("family", [8, 11])
def test_fixture_exercises_the_second_stage(family):
    """A changed fixture must not silently turn the second assigner stage into a no-op or sit on a tie."""
    c = _case(family)
    print(family, c["fg_before"], c["fg_after"], c["n_boxes"], c["n_multi"], c["min_gap"], c["items"])
    assert c["fg_before"] > c["fg_after"] == c["n_boxes"] >= 3, (c["fg_before"], c["fg_after"], c["n_boxes"])
    assert c["min_gap"] > 1e-2, c["min_gap"]          # far above fp32 noise: the kept anchor cannot flip between engine and oracle


# ---------------------------------------------------------------------------------------------------- 2: training forward, running statistics
@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("family", [8, 11])
def test_training_forward_and_running_statistics(backend, engine, family):
    c = _case(family)
    m = _engine_model(engine, c["sd0"], family)
    m.train()
    inf, preds = m.forward(c["x"])
    assert inf is None and set(preds) == {"one2many", "one2one"}
    for k in ("boxes", "scores", "angle"):
        assert relerr(preds["one2many"][k], c["preds"][k]) < 1e-3, k
        assert np.array_equal(preds["one2one"][k], preds["one2many"][k]), k                 # same modules, same input values
    sd = m.state_dict()
    n_tower = n_trunk = 0
    for k, r in c["sd1"].items():
        if "running" in k:
            assert np.allclose(sd[k], r, rtol=1e-3, atol=1e-5), k
        elif "num_batches_tracked" in k:
            tower = k.startswith(c["head"] + ".cv")
            assert float(sd[k].reshape(-1)[0]) == float(r) == (2.0 if tower else 1.0), k    # cv2 / cv3 / cv4: two updates; the trunk: one
            n_tower += tower; n_trunk += not tower
    assert n_tower >= 18 and n_trunk > 20
    assert sum(1 for k in c["sd1"] if k.startswith(c["head"] + ".cv4.") and "num_batches_tracked" in k) == 6
    # a single update of a cv4 unit is NOT within the tolerance: the check above separates one update from two
    k = c["head"] + ".cv4.0.0.bn.running_mean"
    once = c["sd0"][k] + (c["sd1"][k] - c["sd0"][k]) / 1.97                                 # r1 from r2 = r1 + 0.97 (r1 - r0)
    assert not np.allclose(once, c["sd1"][k], rtol=1e-3, atol=1e-5)
    m.close()


# ---------------------------------------------------------------------------------------------------- 3: loss, head gradients, backward
def _check_loss_and_backward(c, m, family, plain, tol):
    _, loss, items = _step(m, c)
    print("items", items, c["items"], "loss", loss, c["loss"])
    assert items.shape == (4,) and np.allclose(items, c["items"], rtol=1e-3, atol=1e-5), (items, c["items"])
    assert np.allclose(loss, c["loss"], rtol=1e-3, atol=1e-4), (loss, c["loss"])
    got = {}
    for br, pre in (("one2many", "d"), ("one2one", "one2one_d")):
        for k, _ in HEAD:
            r = c["dhead"][(br, k)]
            got[(br, k)] = g = m.get_output(pre + k)
            print(br, k, np.abs(g - r).max(), np.abs(r).max())
            assert np.abs(r).max() > 0 and np.abs(g - r).max() <= tol * np.abs(r).max(), (br, k, np.abs(g - r).max(), np.abs(r).max())
    for k, _ in HEAD:                      # other assignment, other gain: the two branches' gradients differ
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
    # the trunk sees o2m = 0.8 times what a model without the one2one branch sends into it for the same batch ...
    _step(plain, c)
    pg = plain.grads()
    last_neck = "model.21.cv2.conv.weight" if family == 8 else "model.22.cv2.conv.weight"
    o2m = np.float32(0.8)
    for name in ("model.0.conv.weight", last_neck):
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
    _check_loss_and_backward(c, m, family, p, 2e-3)
    p.close(); m.close()


# ---------------------------------------------------------------------------------------------------- 4: backward forms, determinism
@pytest.mark.parametrize("backend", BACKENDS)
def test_backward_forms_agree_and_steps_repeat(backend, engine):
    c = _case(8)
    res = {}
    for mode in ("whole", "sync", "async"):
        m = _engine_model(engine, c["sd0"], 8, dtype="bf16")
        _, _, items = _step(m, c, backward=mode)
        res[mode] = ({k: v.copy() for k, v in m.grads().items()}, items.copy(), m.get_output("one2one_dangle"), m.get_output("dangle"))
        m.close()
    for mode in ("sync", "async"):
        for k, v in res["whole"][0].items():
            assert np.array_equal(v, res[mode][0][k]), (mode, k)
        for i in (1, 2, 3):
            assert np.array_equal(res["whole"][i], res[mode][i]), (mode, i)
    # a second step on ONE model with the weights restored (the running statistics have moved; training-mode gradients do not read them)
    m = _engine_model(engine, c["sd0"], 8)
    _, _, i1 = _step(m, c)
    g1 = {k: v.copy() for k, v in m.grads().items()}
    m.load_state_dict(c["sd0"])
    for mode in ("whole", "sync"):
        _, _, i2 = _step(m, c, backward=mode)
        g2 = m.grads()
        assert np.array_equal(i1, i2)
        for k, v in g1.items():
            assert np.array_equal(v, g2[k]), (mode, k, float(np.abs(v - g2[k]).max()), float(np.abs(v).max()))
    m.close()


# ---------------------------------------------------------------------------------------------------- 5: gains
def _formula(updates, epochs):
    f = np.float32
    o2m = f(max(f(1) - f(updates) / f(max(epochs - 1, 1)), f(0))) * (f(0.8) - f(0.1)) + f(0.1)
    return float(o2m), float(max(f(1) - o2m, f(0)))


@pytest.mark.parametrize("backend", BACKENDS)
def test_gains(backend, engine):
    from yolosharp_amd import YsError
    from yolosharp_amd import model as M
    from yolosharp_amd.trainer import Trainer
    c = _case(8)
    m = _engine_model(engine, c["sd0"], 8, epochs=5)
    assert m.e2e_gains() == pytest.approx((0.8, 0.2), abs=1e-7)
    done = 0
    for n in (1, 2, 4, 6):
        while done < n:
            m.e2e_update(); done += 1
        assert m.e2e_gains() == _formula(n, 5), n                                          # the oracle's fp32 chain, exactly
        if n == 2:     # the criterion uses the moved gains (preds fed through ys_model_set_preds: no forward needed)
            assert m.e2e_gains() == c["gains2"] and abs(c["gains2"][0] - 0.8) > 0.1
            m.set_preds(c["preds"])
            _, items = M.v8OBBLoss(m)(None, c["batch"])
            assert np.allclose(items, c["items2"], rtol=1e-3, atol=1e-5), (items, c["items2"])
            assert not np.allclose(items, c["items"], rtol=1e-3, atol=1e-5)
    assert m.e2e_gains() == pytest.approx((0.1, 0.9), abs=1e-6) and m.e2e_gains()[0] == _formula(4, 5)[0]      # reached at the schedule's end, then held
    m.close()
    # Trainer steps the schedule of an End2End OBB run once per epoch (YoloBaseTaskModel.cs:350-353), also after an epoch without a trained batch
    m = _engine_model(engine, c["sd0"], 8, dtype="bf16", epochs=5)
    data = dict(c["batch"]); data["images"] = c["x"]
    tr = Trainer(m, epochs=2, nb=1)
    hist = tr.fit(lambda: [data])
    assert len(hist) == 2 and all(np.all(np.isfinite(h["train_loss"])) and h["train_loss"].shape == (4,) for h in hist)
    assert m.e2e_gains() == c["gains2"]
    tr.train_epoch([], 3)
    assert tr.steps_run == 0 and m.e2e_gains() == _formula(3, 5)
    m.close()
    # the same loop on a plain OBB model steps nothing, and the gain entries stay refused there
    p = _engine_model(engine, c["sd0"], 8, end2end=False, dtype="bf16")
    calls = []
    p.e2e_update = lambda: calls.append(1)
    hist = Trainer(p, epochs=2, nb=1).fit(lambda: [data])
    assert len(hist) == 2 and not calls
    del p.e2e_update
    for fn in (p.e2e_gains, p.e2e_update):
        with pytest.raises(YsError):
            fn()
    p.close()


# ---------------------------------------------------------------------------------------------------- 6: eval forward
@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("family", [8, 11])
def test_eval_forward(backend, engine, family):
    c = _case(family)
    p = _engine_model(engine, c["sd0"], family, end2end=False)
    p.eval()
    pinf, _ = p.forward(c["x"])
    for max_det in (300, 17):
        m = _engine_model(engine, c["sd0"], family, max_det=max_det)
        m.eval()
        inf, preds = m.forward(c["x"])
        k = min(max_det, m.A)
        assert set(inf) == {"boxes", "pred"} and set(preds) == {"one2many", "one2one"} and set(preds["one2one"]) == {"boxes", "scores", "angle"}
        assert inf["pred"].shape == (B, 4 + NC + 1, m.A) and inf["boxes"].shape == (B, k, 7)
        assert np.array_equal(inf["pred"].view(np.uint32), pinf["boxes"].view(np.uint32))       # Obb.decode_bboxes ignores end2end: xywh, bit for bit
        assert relerr(inf["pred"], c["pred"]) < 1e-3
        assert_pred_blocks(inf["pred"], c["pred"], NC, 1e-3, tag="e2e obb v%d" % family)            # boxes, probabilities and the angle each on their own
        rrows, _ = S.postprocess(torch.from_numpy(inf["pred"]), NC, max_det)
        assert np.array_equal(inf["boxes"].view(np.uint32), rrows.numpy().view(np.uint32))
        rows, _ = engine.e2e_topk(inf["pred"], max_det, extra=1)
        assert np.array_equal(inf["boxes"].view(np.uint32), rows.view(np.uint32))
        assert relerr(np.sort(inf["boxes"][..., 4], 1), np.sort(c["rows"][:, :k, 4], 1)) < 1e-3
        dptr, dk = m.det_device()
        assert dk == k and np.array_equal(engine.from_device(dptr, (B, k, 7), np.float32), inf["boxes"])
        m.close()
    p.close()


# ---------------------------------------------------------------------------------------------------- 7: ys_val_match_rotated_batched
def _match_case(max_det, seed=4):
    """B = 3 oriented rows and labels: image 0 has labels and detections (perturbed copies of its labels, two detections of one label, a class that
    no detection predicts), image 1 has no labels, image 2 has labels but count = 0."""
    g = np.random.default_rng(seed)
    Wd, Hd = 320.0, 256.0

    def boxes(n):
        return np.stack((g.uniform(0.15, 0.85, n), g.uniform(0.15, 0.85, n), g.uniform(0.08, 0.4, n), g.uniform(0.08, 0.4, n),
                         g.uniform(-np.pi / 4, 3 * np.pi / 4, n)), 1).astype(np.float32)
    lab0, lab2 = boxes(6), boxes(3)
    cls0 = np.array([0, 1, 1, 2, 3, 4], np.float32)                # class 4 is predicted by no detection
    bi = np.concatenate((np.zeros(6), np.full(3, 2.0))).astype(np.float32)
    cl = np.concatenate((cls0, np.array([0, 1, 2], np.float32)))
    bb = np.concatenate((lab0, lab2))
    rows = np.zeros((3, max_det, 7), np.float32)
    count = np.array([min(14, max_det), min(5, max_det), 0], np.int32)
    scale = np.array([Wd, Hd, Wd, Hd, 1.0], np.float32)
    src = [0, 0, 1, 2, 3, 1, 2, 0, 3, 1, 2, 3, 0, 1]                # label 0 twice up front (duplicates), every label but 5 several times
    for d in range(count[0]):
        j = src[d]
        jit = np.array([g.normal(0, 0.02), g.normal(0, 0.02), g.normal(0, 0.03), g.normal(0, 0.03), g.normal(0, 0.08)], np.float32) * (1 + d // 5)
        box = (lab0[j] + jit) * scale
        rows[0, d, :4] = box[:4]; rows[0, d, 6] = box[4]
        rows[0, d, 4] = 0.95 - 0.05 * d
        rows[0, d, 5] = cls0[j] if d != 6 else 3.0                  # one detection sits on label 2 with another class
    for b in (1, 2):                                                # image 1: detections without labels; image 2: rows beyond count are never read
        r = boxes(max(int(count[1]), 4)) * scale
        n = min(len(r), max_det)
        rows[b, :n, :4] = r[:n, :4]; rows[b, :n, 6] = r[:n, 4]; rows[b, :n, 4] = 0.9; rows[b, :n, 5] = np.arange(n) % 3
    return rows, count, {"batch_idx": bi, "cls": cl, "bboxes": bb}, Wd, Hd


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("max_det", [16, 300])
def test_val_match_rotated_batched(backend, engine, max_det):
    rows, count, batch, Wd, Hd = _match_case(max_det)
    got = engine.val_match_rotated(rows, count, batch, Wd, Hd)
    assert [g.shape for g in got] == [(int(n), 10) for n in count]
    thr = torch.linspace(0.5, 0.95, 10)
    seen = 0
    for b in range(3):
        sel = batch["batch_idx"] == b
        gt = np.concatenate((batch["bboxes"][sel, :4] * np.array([Wd, Hd, Wd, Hd], np.float32), batch["bboxes"][sel, 4:5]), 1).astype(np.float32)
        r = rows[b, :count[b]]
        pred = np.ascontiguousarray(np.concatenate((r[:, :4], r[:, 6:7]), 1), np.float32)
        # (a) the existing per-image path, bit for bit
        iou = engine.batch_probiou(gt, pred) if len(gt) and len(pred) else np.zeros((len(gt), len(pred)), np.float32)
        want = engine.match_predictions(r[:, 5], batch["cls"][sel], iou)
        assert np.array_equal(got[b], np.asarray(want).reshape(len(r), 10).astype(bool)), b
        # (b) the oracle, on a case whose IoUs keep clear of every threshold
        if len(gt) and len(pred):
            riou = O.batch_probiou(torch.from_numpy(gt), torch.from_numpy(pred))
            assert float((riou[..., None] - thr).abs().min()) > 1e-4
            rwant = O.match_predictions(torch.from_numpy(r[:, 5]), torch.from_numpy(batch["cls"][sel]), riou).numpy().astype(bool)
            assert np.array_equal(got[b], rwant), b
            seen += int(rwant.sum())
            if b == 0:
                assert rwant[:, 0].sum() >= 3 and rwant[:, 9].sum() < rwant[:, 0].sum()        # matches at 0.5, fewer at 0.95
                assert not (rwant[0].any() and rwant[1].any())                               # two detections of label 0: one is credited
        else:
            assert not got[b].any()
    assert seen > 0
    # (c) every label in ONE image: the per-image label workspace holds all n labels, so like ys_val_match_batched the call cannot run out of room --
    # both succeed, and the result is still the per-image path's
    one = dict(batch); one["batch_idx"] = np.zeros_like(batch["batch_idx"])
    got1 = engine.val_match_rotated(rows, count, one, Wd, Hd)
    engine.val_match(np.ascontiguousarray(rows[..., :6]), count, {"batch_idx": one["batch_idx"], "cls": one["cls"], "bboxes": np.ascontiguousarray(one["bboxes"][:, :4])}, Wd, Hd)
    gt = np.concatenate((one["bboxes"][:, :4] * np.array([Wd, Hd, Wd, Hd], np.float32), one["bboxes"][:, 4:5]), 1).astype(np.float32)
    r = rows[0, :count[0]]
    iou = engine.batch_probiou(gt, np.ascontiguousarray(np.concatenate((r[:, :4], r[:, 6:7]), 1), np.float32))
    assert np.array_equal(got1[0], np.asarray(engine.match_predictions(r[:, 5], one["cls"], iou)).reshape(len(r), 10).astype(bool))
    assert not got1[1].any() and got1[2].shape == (0, 10)


# ---------------------------------------------------------------------------------------------------- 8: Obber on an End2End model
@pytest.mark.parametrize("backend", BACKENDS)
def test_obber_end2end_predict_and_val(backend, engine):
    from yolosharp_amd import metrics as M
    from yolosharp_amd.detector import Obber, pad_to_32
    c = _case(8)
    m = _engine_model(engine, c["sd0"], 8, b=1)
    ob = Obber(m)
    assert ob.end2end
    img = np.ascontiguousarray((c["x"][0] * 255).astype(np.uint8))
    res = ob.ImagePredict(img, predict_threshold=0.001)
    m.eval()
    inf, _ = m.forward(pad_to_32(img.astype(np.float32))[None])
    want = S.select(S.postprocess(torch.from_numpy(inf["pred"]), NC)[0], 0.001)[0].numpy()
    assert 0 < len(want) == len(res)
    for r, w_ in zip(res, want):
        assert (r.CenterX, r.CenterY, r.Width, r.Height, r.Score, r.ClassID, r.Radian) == \
               (int(w_[0]), int(w_[1]), int(w_[2]), int(w_[3]), float(w_[4]), int(w_[5]), float(w_[6]))
    m.close()
    p = _engine_model(engine, c["sd0"], 8, end2end=False, b=1)
    with pytest.raises(ValueError):
        Obber(p, end2end=True)
    p.close()
    # ---- Val on two small batches against a host restatement: rows -> select -> batch_probiou -> match_predictions -> ap_per_class
    m = _engine_model(engine, c["sd0"], 8)
    d1 = dict(c["batch"]); d1["images"] = c["x"]
    # second batch: labels cut from the model's own rows (three exact copies and one shifted copy per image), so that the matching has something to credit
    x2 = np.ascontiguousarray(c["x"][::-1])
    m.eval()
    own = m.forward(x2)[0]["boxes"]
    bi2, cl2, bb2 = [], [], []
    for b in range(B):
        for j, r in enumerate(own[b, [0, 3, 7, 11]]):
            sh = 0.12 * r[2] if j == 3 else 0.0
            bi2.append(b); cl2.append(r[5]); bb2.append([(r[0] + sh) / W, r[1] / H, r[2] / W, r[3] / H, r[6]])
    d2 = {"batch_idx": np.array(bi2, np.float32), "cls": np.array(cl2, np.float32), "bboxes": np.array(bb2, np.float32), "images": x2}
    conf = 0.001
    loss_items, summary = Obber(m).Val([d1, d2], conf_thres=conf)
    tps, confs, pcls, tcls, ritems = [], [], [], [], None
    net = R.E2EObb(make_ref(O.Yolov8Obb, NC, "n")).eval()
    for d in (d1, d2):
        tb = {k: torch.from_numpy(np.asarray(v)) for k, v in d.items() if k != "images"}
        with torch.no_grad():
            _, rp = net(torch.from_numpy(d["images"]))
            _, it = R.E2EOBBLoss(NC)(rp, tb)
        ritems = it.numpy() if ritems is None else ritems + it.numpy()          # Obber.Val adds up the detached items
        m.eval()
        inf, _ = m.forward(d["images"])
        kept = S.select(S.postprocess(torch.from_numpy(inf["pred"]), NC)[0], conf)
        for b in range(B):
            sel = tb["batch_idx"] == b
            gt = torch.cat((tb["bboxes"][sel, :4] * torch.tensor([W, H, W, H], dtype=torch.float32), tb["bboxes"][sel, 4:5]), 1)
            r = kept[b]
            iou = O.batch_probiou(gt, torch.cat((r[:, :4], r[:, 6:7]), 1)) if len(gt) and len(r) else torch.zeros(len(gt), len(r))
            tps.append(O.match_predictions(r[:, 5], tb["cls"][sel], iou).numpy().astype(bool))
            confs.append(r[:, 4].numpy()); pcls.append(r[:, 5].numpy()); tcls.append(tb["cls"][sel].numpy())
    assert sum(len(t) for t in tps) > 50
    want = M.val_summary(M.ap_per_class(np.concatenate(tps), np.concatenate(confs), np.concatenate(pcls), np.concatenate(tcls)))
    print("val", loss_items, ritems, summary, want)
    assert loss_items.shape == (4,) and np.allclose(loss_items, ritems, rtol=1e-3, atol=1e-4), (loss_items, ritems)
    assert len(summary) == 4 and np.allclose(summary, want, rtol=0, atol=1e-9), (summary, want)
    assert want[2] > 0 and sum(int(t.any()) for t in tps) >= 2                      # the labels cut from the rows are credited
    m.close()


# ---------------------------------------------------------------------------------------------------- 9: boundaries
@pytest.mark.parametrize("backend", BACKENDS)
def test_boundaries(backend, engine, tmp_path):
    from yolosharp_amd import YsError, weights_bin
    from yolosharp_amd import blocks, heads
    from yolosharp_amd import model as M
    others = [cls(engine, nc=NC, size="n", height=32, width=32, max_batch=1, dtype="f32") for cls in (M.Yolov8, M.Yolov11Segment, M.Yolov8Pose, M.Yolov8Classify)]
    others.append(heads.Detect(engine, nc=NC, ch=(16, 32, 64), height=32, width=32))
    others.append(blocks.Conv(engine, 8, 8, 3, height=16, width=16))
    for mm in others:
        assert engine.lib.ys_model_e2e_obb_init(mm.handle, 300, 100) == 4, type(mm)          # YS_ERR_UNSUPPORTED
        mm.close()
    c = _case(8)
    e2e = _engine_model(engine, c["sd0"], 8)
    with pytest.raises(YsError) as e:
        e2e.e2e_obb_init()                                                            # once
    assert e.value.status == 5                                                        # YS_ERR_STATE
    for fn in (e2e.one2one_init, e2e.e2e_init):                                       # the other entries keep refusing OBB models
        with pytest.raises(YsError) as e:
            fn()
        assert e.value.status == 4
    plain = _cls(8)(engine, nc=NC, size="n", height=H, width=W, max_batch=B, dtype="f32")
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
    # a plain OBB model behaves as before: flat preds, one criterion pass, the new keys and entries refused
    plain.eval()
    inf, preds = plain.forward(c["x"])
    assert set(inf) == {"boxes"} and set(preds) == {"boxes", "scores", "angle"}
    for key in ("det", "one2one_boxes", "one2one_scores", "one2one_angle", "one2one_dangle"):
        with pytest.raises(YsError):
            plain.get_output(key)
    for fn in (plain.det_device, plain.e2e_gains, plain.e2e_update):
        with pytest.raises(YsError):
            fn()
    plain.set_preds(c["preds"])
    _, pitems = M.v8OBBLoss(plain)(None, c["batch"])
    assert np.allclose(pitems, c["plain_items"], rtol=1e-3, atol=1e-5), (pitems, c["plain_items"])       # one pass, unweighted
    # ys_model_set_preds feeds both branches
    e2e.set_preds(c["preds"])
    _, items = M.v8OBBLoss(e2e)(None, c["batch"])
    assert np.allclose(items, c["items"], rtol=1e-3, atol=1e-5), (items, c["items"])
    for k, _ in HEAD:
        assert np.array_equal(e2e.get_output("one2one_" + k), e2e.get_output(k))
    assert relerr(e2e.get_output("one2one_angle"), c["preds"]["angle"]) < 1e-4
    for m in (e2e, plain):
        m.close()


# ---------------------------------------------------------------------------------------------------- 10: bf16
@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("family", [8, 11])
def test_bf16_three_steps_descend(backend, engine, family):
    from yolosharp_amd.model import v8OBBLoss
    c = _case(family)
    m = _engine_model(engine, c["sd0"], family, dtype="bf16")
    m.train()
    crit = v8OBBLoss(m)
    sums = []
    for _ in range(3):
        m.forward(c["x"], fetch=False)
        loss, items = crit(None, c["batch"])
        assert np.all(np.isfinite(items))
        sums.append(float(loss.sum()))
        m.zero_grad(); m.backward(); m.adamw_step([1e-3] * 3)
    print("bf16", sums, c["loss"].sum())
    assert np.allclose(sums[0], c["loss"].sum(), rtol=5e-2), (sums, c["loss"].sum())
    assert sums[2] < sums[0], sums
    m.close()


# ---------------------------------------------------------------------------------------------------- 11: full resolution
@pytest.mark.gpu
@pytest.mark.parametrize("backend", ["gpu"])
def test_yolov11s_obb_e2e_full_resolution_f32(backend, engine):
    """The shape of tests/test_obb_pose.py::test_yolov11s_obb_loss_backward_full_resolution_f32 with its 1e-3 / 2e-3 tolerances."""
    c = _oracle_step(11, "s", 2, 640, 640, 12)
    assert c["fg_before"] > c["fg_after"] > 0, (c["fg_before"], c["fg_after"])       # the second stage prunes at this shape too
    c.update(x=c["x"].numpy(), batch=_np(c["batch"]))
    m = _engine_model(engine, c["sd0"], 11, h=640, w=640, size="s")
    _check_loss_and_backward(c, m, 11, None, 2e-3)
    m.close()
