"""End2End for Pose models (ys_model_e2e_pose_init): aliased cv2 / cv3 / cv4 towers (51 wide on the n model: padded inside), E2EPoseLoss (gains, the
keep-best stage tal_topk2 = 1 on the one2one pass only), the two-pass head backward, the top-k post-process with the keypoints, the gain schedule
Trainer does NOT step, PoseDetector on an End2End model with the batched ys_val_match_pose_batched, the task boundary.
Oracle = tests/e2e_pose_ref.py over oracle/yolo_oracle.py (Modules/Head.cs:89-127, 485-610; Utils/Loss.cs:870-1071, 1238-1295; Utils/Tal.cs:225-255;
Models/PoseDetector.cs:131-165).  fp32 tolerances are those of tests/test_obb_pose.py::_pose_train_parity (1e-3 / 2e-3); post-process and matching are
compared exactly."""
import copy
import functools

import numpy as np
import pytest
import torch

import e2e_pose_ref as R
import e2e_seg_ref as S
from conftest import BACKENDS
from oracle import yolo_oracle as O
from test_model import assert_pred_blocks, relerr
from test_obb_pose import make_ref

B, H, W = 2, 64, 64                        # A = 84
HEAD = ("boxes", "scores", "kpts")
# name -> (family, nc, kpt_num, kpt_dim, label seed, labels per image at most, weight seed): the COCO layout on both families, a second fixture with
# three classes, and 5 x 2 keypoints (sigmas = 1 / K, no visibility term).
# Weight seed.  The keypoint term is exp(-e) with e up to ~10 on random weights, and at 64 x 64 the P5 towers normalise over 2 x 2 x 2 values, so on
# some random networks fp32 rounding alone moves the keypoint gradients by more than the 2e-3 the comparison allows: with weight seed 0 the Yolov11 ORACLE
# differs from its own float64 run by 1e-3 in dkpts and 4e-3 in a cv4 weight gradient.  The seed is therefore chosen with the oracle alone: the first of
# 0, 1, 2, ... for which the fp32 oracle agrees with its float64 run to 5e-4 (a quarter of the tolerance) on both -- 0 for Yolov8, 2 for Yolov11 (seeds 0
# and 1 give 4.1e-3 and 8.4e-4).  test_fixture_exercises_the_second_stage asserts the condition.
CFG = {"v8": (8, 1, 17, 3, 1, 8, 0), "v11": (11, 1, 17, 3, 1, 8, 2), "v8nc3": (8, 3, 17, 3, 1, 8, 0), "v8k5d2": (8, 1, 5, 2, 1, 8, 0)}


def _cls(family):
    from yolosharp_amd import model as M
    return M.Yolov8Pose if family == 8 else M.Yolov11Pose


def _engine_model(engine, sd, cfg, end2end=True, dtype="f32", max_det=300, h=H, w=W, b=B, epochs=100, size="n"):
    family, nc, K, D = CFG[cfg][:4] if isinstance(cfg, str) else cfg
    m = _cls(family)(engine, nc=nc, size=size, height=h, width=w, max_batch=b, dtype=dtype, kpt_num=K, kpt_dim=D)
    if end2end:
        m.e2e_pose_init(max_det, epochs)
    m.load_state_dict(sd)
    return m


def _np(d):
    return {k: v.numpy() for k, v in d.items()}


def _detached(rp):
    return {br: {k: (v.detach() if torch.is_tensor(v) else [f.detach() for f in v]) for k, v in rp[br].items()} for br in rp}


def _labels(b, h, w, nc, K, D, seed, kmax):
    batch = O.synthetic_batch(b, h, w, nc, seed=seed, kmax=kmax)
    batch["keypoints"] = O.synthetic_keypoints(batch, K, D)               # about a quarter of the points invisible (D = 3)
    return batch


def _oracle_step(family, nc, K, D, size, b, h, w, seed, kmax, wseed=0):
    """One End2End Pose step of the oracle: everything the tests compare against, never modified afterwards."""
    net = make_ref(getattr(O, f"Yolov{family}Pose"), nc, size, seed=wseed, kpt_num=K, kpt_dim=D)
    sd0 = {k: v.detach().clone().numpy() for k, v in net.state_dict().items()}
    x = torch.rand(b, 3, h, w, generator=torch.Generator().manual_seed(3))
    batch = _labels(b, h, w, nc, K, D, seed, kmax)
    ref = R.E2EPose(net).train()
    _, rpreds = ref(x)
    for br in ("one2many", "one2one"):
        for k in HEAD:
            rpreds[br][k].retain_grad()
    crit = R.E2EPoseLoss(nc, K, D)
    rloss, ritems = crit(rpreds, batch)
    rloss.sum().backward()
    asg = crit.one2one.assigner
    # the second assigner stage on this fixture: positives before / after, rows pruned from several positives, the relative gap at the cut
    vals = asg.align_before * asg.mask_before
    rows = asg.mask_before.sum(-1) > 0
    top2 = torch.sort(vals, dim=-1, descending=True).values[..., :2][rows]
    gaps = ((top2[:, 0] - top2[:, 1]) / top2[:, 0])[asg.mask_before.sum(-1)[rows] > 1]
    dhead = {(br, k): rpreds[br][k].grad.numpy() for br in ("one2many", "one2one") for k in HEAD}
    return dict(net=net, crit=crit, sd0=sd0, x=x, batch=batch, rpreds=rpreds, items=ritems.numpy(), loss=rloss.detach().numpy(), dhead=dhead,
                fg_before=int(asg.fg_before.sum()), fg_after=int(asg.fg_after.sum()), n_boxes=int(rows.sum()),
                n_multi=int((asg.mask_before.sum(-1)[rows] > 1).sum()), min_gap=float(gaps.min()) if len(gaps) else 0.0,
                grads={n: p.grad.numpy() for n, p in net.named_parameters() if p.grad is not None},
                sd1={k: v.detach().clone().numpy() for k, v in net.state_dict().items()},
                head="model.22" if family == 8 else "model.23")


@functools.lru_cache(maxsize=None)
def _case(cfg):
    family, nc, K, D, seed, kmax, wseed = CFG[cfg]
    ev = R.E2EPose(make_ref(getattr(O, f"Yolov{family}Pose"), nc, "n", seed=wseed, kpt_num=K, kpt_dim=D)).eval()
    x = torch.rand(B, 3, H, W, generator=torch.Generator().manual_seed(3))
    with torch.no_grad():
        rinf, _ = ev(x)
    c = _oracle_step(family, nc, K, D, "n", B, H, W, seed, kmax, wseed)
    rp, crit = c.pop("rpreds"), c.pop("crit")
    # the items with the gains two update() calls of a 5-epoch schedule leave (test_gains)
    c2 = R.E2EPoseLoss(nc, K, D, epochs=5)
    c2.update(); c2.update()
    with torch.no_grad():
        _, items2 = c2(_detached(rp), c["batch"])
        _, plain_items = O.v8PoseLoss(nc, K, D)(_detached(rp)["one2many"], c["batch"])
    c.update(x=c["x"].numpy(), batch=_np(c["batch"]), pred=rinf["pred"].numpy(), rows=rinf["boxes"].numpy(),
             preds={k: rp["one2many"][k].detach().numpy() for k in HEAD},
             items2=items2.numpy(), gains2=(float(c2.o2m), float(c2.o2o)), plain_items=plain_items.numpy(), nc=nc, K=K, D=D, family=family, wseed=wseed)
    c.pop("net")
    return c


def _oracle_fp32_error(cfg):
    """The fp32 oracle against its own float64 run on this fixture: the largest relative difference of the one2many keypoint gradient and of the cv4
    parameter gradients (the quantities the exp(-e) of the keypoint term makes sensitive)."""
    family, nc, K, D, seed, kmax, wseed = CFG[cfg]
    net = make_ref(getattr(O, f"Yolov{family}Pose"), nc, "n", seed=wseed, kpt_num=K, kpt_dim=D)
    x = torch.rand(B, 3, H, W, generator=torch.Generator().manual_seed(3))
    batch = _labels(B, H, W, nc, K, D, seed, kmax)
    out = []
    for dt, n_ in ((torch.float32, net), (torch.float64, copy.deepcopy(net).double())):
        _, rp = R.E2EPose(n_).train()(x.to(dt))
        rp["one2many"]["kpts"].retain_grad()
        crit = R.E2EPoseLoss(nc, K, D)
        for c_ in (crit.one2many, crit.one2one):
            c_.sigmas = c_.sigmas.to(dt)
        crit(rp, {k: v.to(dt) for k, v in batch.items()})[0].sum().backward()
        out.append((rp["one2many"]["kpts"].grad.double().numpy(),
                    {k: p.grad.double().numpy() for k, p in n_.named_parameters() if ".cv4." in k and p.grad is not None}))
    (g32, p32), (g64, p64) = out
    return float(np.abs(g32 - g64).max() / np.abs(g64).max()), max(float(np.abs(p32[k] - p64[k]).max() / np.abs(p64[k]).max()) for k in p64)


def _step(m, c, backward="whole"):
    from yolosharp_amd.model import v8PoseLoss
    m.train(); m.zero_grad()
    _, preds = m.forward(c["x"])
    loss, items = v8PoseLoss(m)(None, c["batch"])
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
@pytest.mark.parametrize("cfg", list(CFG))
def test_fixture_exercises_the_second_stage(cfg):
    """A changed fixture must not silently turn the second assigner stage into a no-op or sit on a tie."""
    c = _case(cfg)
    print(cfg, c["fg_before"], c["fg_after"], c["n_boxes"], c["n_multi"], c["min_gap"], c["items"])
    assert c["fg_before"] > c["fg_after"] == c["n_boxes"] >= 3, (c["fg_before"], c["fg_after"], c["n_boxes"])
    assert c["n_multi"] >= 2
    assert c["min_gap"] > 1e-2, c["min_gap"]          # far above fp32 noise: the kept anchor cannot flip between engine and oracle
    assert c["items"][1] > 0 and (c["D"] == 2) == (c["items"][2] == 0)
    e_head, e_cv4 = _oracle_fp32_error(cfg)
    print(cfg, "oracle fp32 against float64: dkpts", e_head, "cv4 gradients", e_cv4)
    assert e_head < 5e-4 and e_cv4 < 5e-4, (e_head, e_cv4)      # the fixture is conditioned well enough for a 2e-3 comparison in fp32 (see CFG)
    if c["D"] == 3:
        assert (c["batch"]["keypoints"][..., 2] == 0).any() and (c["batch"]["keypoints"][..., 2] != 0).any()     # some invisible keypoints


# ---------------------------------------------------------------------------------------------------- 2: training forward, running statistics
@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("cfg", ["v8", "v11"])
def test_training_forward_and_running_statistics(backend, engine, cfg):
    c = _case(cfg)
    m = _engine_model(engine, c["sd0"], cfg)
    m.train()
    inf, preds = m.forward(c["x"])
    assert inf is None and set(preds) == {"one2many", "one2one"}
    for k in HEAD:
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
def _flat(engine, ptr_n):
    p, n = ptr_n
    return engine.from_device(p, (n,), np.float32)


def _check_loss_and_backward(engine, c, m, plain, tol, pad_rows=False):
    pad = None
    if pad_rows:
        # the rows of the padded 51-wide towers: the words of the flat parameter buffer no named tensor reaches (zero weights and BatchNorm biases; the
        # pad rows' BatchNorm weights are 1 and multiply a zero output)
        sd0 = m.state_dict()
        m.load_state_dict({k: np.ones_like(v) for k, v in sd0.items()})
        ones = _flat(engine, m.param_buffer())
        m.load_state_dict({k: np.full_like(v, 2) for k, v in sd0.items()})
        pad = np.flatnonzero(ones == _flat(engine, m.param_buffer()))
        assert m.param_buffer()[1] == m.grad_buffer()[1] and 0 < len(pad) == m.param_buffer()[1] - m.num_params()
        m.load_state_dict(sd0)
        pad0 = _flat(engine, m.param_buffer())[pad]
        assert np.count_nonzero(pad0) == 6 and np.all(pad0[pad0 != 0] == 1)          # one BatchNorm weight per padded unit (3 levels x 2)
    _, loss, items = _step(m, c)
    print("items", items, c["items"], "loss", loss, c["loss"])
    assert items.shape == (5,) and np.allclose(items, c["items"], rtol=1e-3, atol=1e-5), (items, c["items"])
    assert np.allclose(loss, c["loss"], rtol=1e-3, atol=1e-4), (loss, c["loss"])
    got = {}
    for br, pre in (("one2many", "d"), ("one2one", "one2one_d")):
        for k in HEAD:
            r = c["dhead"][(br, k)]
            got[(br, k)] = g = m.get_output(pre + k)
            print(br, k, np.abs(g - r).max(), np.abs(r).max())
            assert np.abs(r).max() > 0 and np.abs(g - r).max() <= tol * np.abs(r).max(), (br, k, np.abs(g - r).max(), np.abs(r).max())
    for k in HEAD:                         # other assignment, other gain: the two branches' gradients differ
        d = np.abs(got[("one2one", k)] - got[("one2many", k)]).max()
        assert d > 1e-2 * np.abs(got[("one2many", k)]).max(), k
    grads = m.grads()
    gscale = max(float(np.abs(r).max()) for r in c["grads"].values())
    assert len(c["grads"]) > 100
    for name, r in c["grads"].items():
        err = np.abs(grads[name] - r).max()
        assert err <= tol * np.abs(r).max() + 1e-6 * gscale, (name, err, np.abs(r).max())
    if pad is not None:
        assert not _flat(engine, m.grad_buffer())[pad].any()
        m.adamw_step([1e-3] * 3)
        flat = _flat(engine, m.param_buffer())
        # zero gradients: the zero rows stay exactly zero (the six weights of 1 only see AdamW's decoupled weight decay, as on a plain model)
        assert not flat[pad][pad0 == 0].any() and np.count_nonzero(flat) > m.num_params() // 2
    if plain is None:
        return
    # the trunk sees o2m = 0.8 times what a model without the one2one branch sends into it for the same batch ...
    _step(plain, c)
    pg = plain.grads()
    last_neck = "model.21.cv2.conv.weight" if c["family"] == 8 else "model.22.cv2.conv.weight"
    o2m = np.float32(0.8)
    for name in ("model.0.conv.weight", last_neck):
        assert np.abs(pg[name]).max() > 0
        assert np.abs(grads[name] - o2m * pg[name]).max() <= 1e-5 * np.abs(o2m * pg[name]).max(), name
    # ... while a cv4 tower also carries the one2one gradient
    tw = c["head"] + ".cv4.0.2.weight"
    assert np.abs(grads[tw] - o2m * pg[tw]).max() > 1e-2 * np.abs(pg[tw]).max()


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("cfg", list(CFG))
def test_loss_and_backward(backend, engine, cfg):
    c = _case(cfg)
    m = _engine_model(engine, c["sd0"], cfg)
    assert m.e2e_gains() == pytest.approx((0.8, 0.2), abs=1e-7)
    p = _engine_model(engine, c["sd0"], cfg, end2end=False) if cfg in ("v8", "v11") else None
    _check_loss_and_backward(engine, c, m, p, 2e-3, pad_rows=c["K"] * c["D"] == 51)
    if p is not None:
        p.close()
    m.close()


# ---------------------------------------------------------------------------------------------------- 4: backward forms, determinism
@pytest.mark.parametrize("backend", BACKENDS)
def test_backward_forms_agree_and_steps_repeat(backend, engine):
    c = _case("v8")
    res = {}
    for mode in ("whole", "sync", "async"):
        m = _engine_model(engine, c["sd0"], "v8", dtype="bf16")
        _, _, items = _step(m, c, backward=mode)
        res[mode] = ({k: v.copy() for k, v in m.grads().items()}, items.copy(), m.get_output("one2one_dkpts"), m.get_output("dkpts"))
        m.close()
    for mode in ("sync", "async"):
        for k, v in res["whole"][0].items():
            assert np.array_equal(v, res[mode][0][k]), (mode, k)
        for i in (1, 2, 3):
            assert np.array_equal(res["whole"][i], res[mode][i]), (mode, i)
    # a second step on ONE model with the weights restored (the running statistics have moved; training-mode gradients do not read them)
    m = _engine_model(engine, c["sd0"], "v8")
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
    from yolosharp_amd import model as M
    from yolosharp_amd.trainer import Trainer
    c = _case("v8")
    m = _engine_model(engine, c["sd0"], "v8", epochs=5)
    assert m.e2e_gains() == pytest.approx((0.8, 0.2), abs=1e-7)
    done = 0
    for n in (1, 2, 4, 6):
        while done < n:
            m.e2e_update(); done += 1
        assert m.e2e_gains() == _formula(n, 5), n                                          # the oracle's fp32 chain, exactly
        if n == 2:     # the criterion uses the moved gains (preds fed through ys_model_set_preds: no forward needed)
            assert m.e2e_gains() == c["gains2"] and abs(c["gains2"][0] - 0.8) > 0.1
            m.set_preds(c["preds"])
            _, items = M.v8PoseLoss(m)(None, c["batch"])
            assert np.allclose(items, c["items2"], rtol=1e-3, atol=1e-5), (items, c["items2"])
            assert not np.allclose(items, c["items"], rtol=1e-3, atol=1e-5)
    assert m.e2e_gains() == pytest.approx((0.1, 0.9), abs=1e-6) and m.e2e_gains()[0] == _formula(4, 5)[0]      # reached at the schedule's end, then held
    m.close()
    # Trainer does NOT step the schedule of an End2End Pose run: the reference's loop tests `loss is Loss.E2EOBBLoss` and E2EPoseLoss is a class of its own
    # (YoloBaseTaskModel.cs:350-353) -- the gains stay 0.8 / 0.2
    m = _engine_model(engine, c["sd0"], "v8", dtype="bf16", epochs=5)
    data = dict(c["batch"]); data["images"] = c["x"]
    tr = Trainer(m, epochs=2, nb=1)
    hist = tr.fit(lambda: [data])
    assert len(hist) == 2 and all(np.all(np.isfinite(h["train_loss"])) and h["train_loss"].shape == (5,) for h in hist)
    assert m.e2e_gains() == pytest.approx((0.8, 0.2), abs=1e-7)
    tr.train_epoch([data], 3)
    assert tr.steps_run == 1 and m.e2e_gains() == pytest.approx((0.8, 0.2), abs=1e-7)
    m.close()
    # ... while on an End2End OBB model it still does
    ob = M.Yolov8Obb(engine, nc=2, size="n", height=32, width=32, max_batch=1, dtype="bf16")
    ob.e2e_obb_init(300, 5)
    ob.init_weights(1)
    Trainer(ob, epochs=5, nb=1).train_epoch([], 1)
    assert ob.e2e_gains() == _formula(1, 5)
    ob.close()


# ---------------------------------------------------------------------------------------------------- 6: eval forward
@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("cfg", ["v8", "v11", "v8k5d2"])
def test_eval_forward(backend, engine, cfg):
    c = _case(cfg)
    nc, nk = c["nc"], c["K"] * c["D"]
    p = _engine_model(engine, c["sd0"], cfg, end2end=False)
    p.eval()
    pinf, ppreds = p.forward(c["x"])
    assert set(pinf) == {"boxes"} and set(ppreds) == {"boxes", "scores", "kpts"}
    for max_det in (300, 16):
        m = _engine_model(engine, c["sd0"], cfg, max_det=max_det)
        m.eval()
        inf, preds = m.forward(c["x"])
        k = min(max_det, m.A)
        assert set(inf) == {"boxes", "pred"} and set(preds) == {"one2many", "one2one"} and set(preds["one2one"]) == set(HEAD)
        assert inf["pred"].shape == (B, 4 + nc + nk, m.A) and inf["boxes"].shape == (B, k, 6 + nk)
        assert relerr(inf["pred"][:, :4], c["pred"][:, :4]) < 1e-3 and relerr(inf["pred"][:, 4:4 + nc], c["pred"][:, 4:4 + nc]) < 1e-3
        assert relerr(inf["pred"][:, 4 + nc:], c["pred"][:, 4 + nc:]) < 1e-3
        assert_pred_blocks(inf["pred"], c["pred"], nc, 1e-3, kdim=c["D"], tag="e2e pose %s" % (cfg,))     # keypoint xy (pixels) and the visibility sigmoid apart
        # xyxy boxes: the plain model's xywh converted; classes and decoded keypoints are the plain model's, bit for bit
        xywh = pinf["boxes"][:, :4]
        assert np.allclose(inf["pred"][:, :2], xywh[:, :2] - xywh[:, 2:4] / 2, rtol=1e-4, atol=1e-3)
        assert np.allclose(inf["pred"][:, 2:4], xywh[:, :2] + xywh[:, 2:4] / 2, rtol=1e-4, atol=1e-3)
        assert (inf["pred"][:, 2:4] >= inf["pred"][:, :2]).all() and not np.array_equal(inf["pred"][:, :4], xywh)
        assert np.array_equal(inf["pred"][:, 4:].view(np.uint32), pinf["boxes"][:, 4:].view(np.uint32))
        rrows, _ = S.postprocess(torch.from_numpy(inf["pred"]), nc, max_det)
        assert np.array_equal(inf["boxes"].view(np.uint32), rrows.numpy().view(np.uint32))        # values and order
        rows, _ = engine.e2e_topk(inf["pred"], max_det, extra=nk)
        assert np.array_equal(inf["boxes"].view(np.uint32), rows.view(np.uint32))
        assert relerr(np.sort(inf["boxes"][..., 4], 1), np.sort(c["rows"][:, :k, 4], 1)) < 1e-3
        dptr, dk = m.det_device()
        assert dk == k and np.array_equal(engine.from_device(dptr, (B, k, 6 + nk), np.float32), inf["boxes"])
        m.close()
    # a plain Pose model's "pred" is what it was: xywh boxes, against the oracle's plain eval forward
    with torch.no_grad():
        rplain, _ = make_ref(getattr(O, f"Yolov{c['family']}Pose"), nc, "n", seed=c["wseed"], kpt_num=c["K"], kpt_dim=c["D"]).eval()(torch.from_numpy(c["x"]))
    assert relerr(pinf["boxes"], rplain["boxes"].numpy()) < 1e-3
    assert_pred_blocks(pinf["boxes"], rplain["boxes"], nc, 1e-3, kdim=c["D"], tag="plain pose %s" % (cfg,))
    p.close()


# ---------------------------------------------------------------------------------------------------- 7: ys_val_match_pose_batched
def _match_case(max_det, K, D, LD, seed=4):
    """B = 3 rows and labels: image 0 has labels and detections that are perturbed copies of its labels (two detections of one label, a class no
    detection predicts, a detection of another class on a label, one detection with a good box and bad keypoints), image 1 has labels and count = 0,
    image 2 has detections and no labels."""
    g = np.random.default_rng(seed)
    Wd, Hd = 320.0, 256.0

    def boxes(n):
        return np.stack((g.uniform(0.2, 0.8, n), g.uniform(0.2, 0.8, n), g.uniform(0.15, 0.4, n), g.uniform(0.15, 0.4, n)), 1).astype(np.float32)

    def kpts(bx):
        u = g.uniform(-0.45, 0.45, (len(bx), K, 2))
        xy = (bx[:, None, :2] + u * bx[:, None, 2:4]).astype(np.float32)
        if LD == 2:
            return xy
        v = g.integers(0, 3, (len(bx), K, 1)).astype(np.float32)
        v[:, 0] = 2.0                                               # every label keeps a visible keypoint
        return np.concatenate((xy, v), 2).astype(np.float32)
    lab0, lab1 = boxes(6), boxes(3)
    kp0, kp1 = kpts(lab0), kpts(lab1)
    cls0 = np.array([0, 1, 1, 2, 3, 4], np.float32)                # class 4 is predicted by no detection
    bi = np.concatenate((np.zeros(6), np.ones(3))).astype(np.float32)
    cl = np.concatenate((cls0, np.array([0, 1, 2], np.float32)))
    bb, kp = np.concatenate((lab0, lab1)), np.concatenate((kp0, kp1))
    rl = 6 + K * D
    rows = np.zeros((3, max_det, rl), np.float32)
    count = np.array([min(14, max_det), 0, min(5, max_det)], np.int32)
    src = [0, 0, 1, 2, 3, 1, 2, 0, 3, 1, 2, 3, 0, 1]                # label 0 twice up front (duplicates), every label but 5 several times
    scale = np.array([Wd, Hd], np.float32)

    def det(box, kps, d, jit):
        c_ = (box[:2] + g.normal(0, 0.01, 2) * jit) * scale
        wh = (box[2:4] * (1 + g.normal(0, 0.04, 2) * jit)) * scale
        out = np.zeros(rl, np.float32)
        out[:2] = c_ - wh / 2; out[2:4] = c_ + wh / 2
        k_ = (kps[:, :2] + g.normal(0, 0.006, (K, 2)) * jit * box[2:4]) * scale
        if d == 3:                                                  # a good box with bad keypoints: the two results differ on this row
            k_ = k_ + 0.6 * box[2:4] * scale
        out[6:] = (np.concatenate((k_, g.uniform(0.1, 1.0, (K, 1))), 1) if D == 3 else k_).reshape(-1)
        return out
    for d in range(count[0]):
        j = src[d]
        rows[0, d] = det(lab0[j], kp0[j], d, 1 + d // 5)
        rows[0, d, 4] = 0.95 - 0.05 * d
        rows[0, d, 5] = cls0[j] if d != 6 else 3.0                  # one detection sits on label 2 with another class
    extra = boxes(max(int(count[2]), 1))
    ek = kpts(extra)
    for d in range(count[2]):                                       # image 2: detections without labels
        rows[2, d] = det(extra[d], ek[d], -1, 1)
        rows[2, d, 4] = 0.9; rows[2, d, 5] = d % 3
    for d in range(min(4, max_det)):                                # image 1: rows beyond count = 0 are never read
        rows[1, d] = det(lab1[d % 3], kp1[d % 3], -1, 1); rows[1, d, 4] = 0.9; rows[1, d, 5] = cl[6 + d % 3]
    return rows, count, {"batch_idx": bi, "cls": cl, "bboxes": bb, "keypoints": kp}, Wd, Hd


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("max_det", [16, 300])
@pytest.mark.parametrize("kd", [(17, 3, 3), (5, 2, 2)])
def test_val_match_pose_batched(backend, engine, max_det, kd):
    K, D, LD = kd
    rows, count, batch, Wd, Hd = _match_case(max_det, K, D, LD)
    thr = torch.linspace(0.5, 0.95, 10)
    res = {od: engine.val_match_pose(rows, count, batch, Wd, Hd, K, D, on_device=od) for od in (False, True)}
    gb, gp = res[False]
    for i in range(2):
        for b in range(3):
            assert np.array_equal(res[False][i][b], res[True][i][b]), (i, b)
    assert [g.shape for g in gb] == [g.shape for g in gp] == [(int(n), 10) for n in count]
    seen = [0, 0]
    for b in range(3):
        sel = batch["batch_idx"] == b
        r = rows[b, :count[b]]
        tcls = batch["cls"][sel]
        # (a) the library's per-image path (PoseDetector.Val's host loop), bit for bit
        gt = batch["bboxes"][sel] * np.array([Wd, Hd, Wd, Hd], np.float32)
        gt_xyxy = np.concatenate((gt[:, :2] - gt[:, 2:] / 2, gt[:, :2] + gt[:, 2:] / 2), 1).astype(np.float32)
        kp = batch["keypoints"][sel]
        if LD == 2:
            kp = np.concatenate((kp, np.ones(kp.shape[:2] + (1,), np.float32)), 2)
        gk = (kp * np.array([Wd, Hd, 1.0], np.float32)).astype(np.float32)
        area = ((gt_xyxy[:, 2] - gt_xyxy[:, 0]) * (gt_xyxy[:, 3] - gt_xyxy[:, 1]) * np.float32(0.53)).astype(np.float32)
        if len(r):
            wb = engine.match_predictions(r[:, 5], tcls, engine.box_iou(gt_xyxy, r[:, :4]))
            wp = engine.match_predictions(r[:, 5], tcls, engine.kpt_iou(gk, r[:, 6:].reshape(-1, K, D), area) if len(gk) else np.zeros((0, len(r)), np.float32))
            assert np.array_equal(gb[b], wb) and np.array_equal(gp[b], wp), b
        # (b) the oracle, on a case whose IoUs and OKS keep clear of every threshold
        if len(r) and sel.any():
            t = torch.from_numpy
            iou, oks, rb, rp_ = R.val_image(t(r), t(tcls), t(batch["bboxes"][sel]), t(batch["keypoints"][sel]), Wd, Hd, K, D)
            assert float((iou[..., None] - thr).abs().min()) > 1e-4 and float((oks[..., None] - thr).abs().min()) > 1e-4
            assert np.array_equal(gb[b], rb.numpy()) and np.array_equal(gp[b], rp_.numpy()), b
            seen[0] += int(rb.sum()); seen[1] += int(rp_.sum())
            if b == 0:
                rb, rp_ = rb.numpy(), rp_.numpy()
                assert rb[:, 0].sum() >= 3 and rb[:, 9].sum() < rb[:, 0].sum()                 # matches at 0.5, fewer at 0.95
                assert rp_[:, 0].sum() >= 3
                assert not (rb[0] & rb[1]).any() and not (rp_[0] & rp_[1]).any()                  # two detections of label 0: one is credited per threshold
                assert rb[3, 0] and not rp_[3].any()                                          # good box, bad keypoints
                assert not np.array_equal(rb, rp_)
        else:
            assert not gb[b].any() and not gp[b].any()
    assert seen[0] > 0 and seen[1] > 0
    assert gb[1].shape == (0, 10) and not gb[2].any() and not gp[2].any() and gb[2].shape[0] == count[2]


# ---------------------------------------------------------------------------------------------------- 8: PoseDetector on an End2End model
@pytest.mark.parametrize("backend", BACKENDS)
def test_pose_detector_end2end_predict_and_val(backend, engine):
    from yolosharp_amd import metrics as M
    from yolosharp_amd.detector import PoseDetector, pad_to_32
    c = _case("v8")
    nc, K, D = c["nc"], c["K"], c["D"]
    m = _engine_model(engine, c["sd0"], "v8", b=1)
    pdt = PoseDetector(m)
    assert pdt.end2end
    img = np.ascontiguousarray((c["x"][0] * 255).astype(np.uint8))
    res = pdt.ImagePredict(img, predict_threshold=0.001)
    m.eval()
    inf, _ = m.forward(pad_to_32(img.astype(np.float32))[None])
    want = S.select(S.postprocess(torch.from_numpy(inf["pred"]), nc)[0], 0.001)[0].numpy()
    assert 0 < len(want) == len(res)
    for r, w_ in zip(res, want):
        x, y = int(w_[0]), int(w_[1])
        rw, rh = int(w_[2]) - x, int(w_[3]) - y
        assert (r.CenterX, r.CenterY, r.Width, r.Height, r.Score, r.ClassID) == (x + rw // 2, y + rh // 2, rw, rh, float(w_[4]), int(w_[5]))
        assert len(r.KeyPoints) == K
        assert [(kp.X, kp.Y, kp.VisibilityScore) for kp in r.KeyPoints] == [tuple(float(v) for v in q) for q in w_[6:].reshape(K, D)]
    m.close()
    p = _engine_model(engine, c["sd0"], "v8", end2end=False, b=1)
    with pytest.raises(ValueError):
        PoseDetector(p, end2end=True)
    p.close()
    # ---- Val on two small batches against the host path on the same detections: rows -> select -> box_iou / kpt_iou -> match_predictions -> ap_per_class
    m = _engine_model(engine, c["sd0"], "v8")
    d1 = dict(c["batch"]); d1["images"] = c["x"]
    # second batch: labels cut from the model's own rows (three exact copies and one shifted copy per image), so that the matching has something to credit
    x2 = np.ascontiguousarray(c["x"][::-1])
    m.eval()
    own = m.forward(x2)[0]["boxes"]
    bi2, cl2, bb2, kp2 = [], [], [], []
    for b in range(B):
        for j, r in enumerate(own[b, [0, 3, 7, 11]]):
            sh = 0.12 * (r[2] - r[0]) if j == 3 else 0.0
            bi2.append(b); cl2.append(r[5])
            bb2.append([((r[0] + r[2]) / 2 + sh) / W, (r[1] + r[3]) / 2 / H, (r[2] - r[0]) / W, (r[3] - r[1]) / H])
            q = r[6:].reshape(K, D).copy()
            q[:, 0] = (q[:, 0] + sh) / W; q[:, 1] /= H; q[:, 2] = 2.0
            kp2.append(q)
    d2 = {"batch_idx": np.array(bi2, np.float32), "cls": np.array(cl2, np.float32), "bboxes": np.array(bb2, np.float32),
          "keypoints": np.array(kp2, np.float32), "images": x2}
    conf = 0.001
    loss_items, box, pose = PoseDetector(m).Val([d1, d2], conf_thres=conf)
    tps, tpps, confs, pcls, tcls, ritems = [], [], [], [], [], None
    net = R.E2EPose(make_ref(O.Yolov8Pose, nc, "n", kpt_num=K, kpt_dim=D)).eval()
    for d in (d1, d2):
        tb = {k: torch.from_numpy(np.asarray(v)) for k, v in d.items() if k != "images"}
        with torch.no_grad():
            _, rp = net(torch.from_numpy(d["images"]))
            _, it = R.E2EPoseLoss(nc, K, D)(rp, tb)
        ritems = it.numpy() if ritems is None else ritems + it.numpy()          # PoseDetector.Val adds up the detached items
        m.eval()
        inf, _ = m.forward(d["images"])
        kept = S.select(S.postprocess(torch.from_numpy(inf["pred"]), nc)[0], conf)
        for b in range(B):
            sel = tb["batch_idx"] == b
            r = kept[b]
            _, _, cb, cp = R.val_image(r, tb["cls"][sel], tb["bboxes"][sel], tb["keypoints"][sel], float(W), float(H), K, D)
            tps.append(cb.numpy()); tpps.append(cp.numpy())
            confs.append(r[:, 4].numpy()); pcls.append(r[:, 5].numpy()); tcls.append(tb["cls"][sel].numpy())
    assert sum(len(t) for t in tps) > 50
    cf, pc, tc = np.concatenate(confs), np.concatenate(pcls), np.concatenate(tcls)
    want_box = M.val_summary(M.ap_per_class(np.concatenate(tps), cf, pc, tc))
    want_pose = M.val_summary(M.ap_per_class(np.concatenate(tpps), cf, pc, tc))
    print("val", loss_items, ritems, box, want_box, pose, want_pose)
    assert loss_items.shape == (5,) and np.allclose(loss_items, ritems, rtol=1e-3, atol=1e-4), (loss_items, ritems)
    assert len(box) == 4 and np.allclose(box, want_box, rtol=0, atol=1e-9), (box, want_box)
    assert len(pose) == 4 and np.allclose(pose, want_pose, rtol=0, atol=1e-9), (pose, want_pose)
    assert want_box[2] > 0 and want_pose[2] > 0 and sum(int(t.any()) for t in tpps) >= 2      # the labels cut from the rows are credited
    m.close()


# ---------------------------------------------------------------------------------------------------- 9: boundaries
@pytest.mark.parametrize("backend", BACKENDS)
def test_boundaries(backend, engine, tmp_path):
    from yolosharp_amd import YsError, weights_bin
    from yolosharp_amd import blocks, heads
    from yolosharp_amd import model as M
    others = [cls(engine, nc=3, size="n", height=32, width=32, max_batch=1, dtype="f32") for cls in (M.Yolov8, M.Yolov11Segment, M.Yolov8Obb, M.Yolov8Classify)]
    others.append(heads.Detect(engine, nc=3, ch=(16, 32, 64), height=32, width=32))
    others.append(blocks.Conv(engine, 8, 8, 3, height=16, width=16))
    for mm in others:
        assert engine.lib.ys_model_e2e_pose_init(mm.handle, 300, 100) == 4, type(mm)         # YS_ERR_UNSUPPORTED
        mm.close()
    c = _case("v8")
    e2e = _engine_model(engine, c["sd0"], "v8")
    with pytest.raises(YsError) as e:
        e2e.e2e_pose_init()                                                           # once
    assert e.value.status == 5                                                        # YS_ERR_STATE
    for fn in (e2e.one2one_init, e2e.e2e_init, lambda: M._ObbMixin.e2e_obb_init(e2e)):       # the other entries keep refusing Pose models
        with pytest.raises(YsError) as e:
            fn()
        assert e.value.status == 4
    plain = _engine_model(engine, c["sd0"], "v8", end2end=False)
    assert e2e.tensor_info() == plain.tensor_info() and e2e.num_params() == plain.num_params()
    # `.bin` round trip: E2E -> plain -> E2E
    plain.init_weights(5)
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
    # a plain Pose model behaves as before: flat preds, one criterion pass, the new keys and entries refused
    plain.eval()
    inf, preds = plain.forward(c["x"])
    assert set(inf) == {"boxes"} and set(preds) == {"boxes", "scores", "kpts"}
    for key in ("det", "one2one_boxes", "one2one_scores", "one2one_kpts", "one2one_dkpts"):
        with pytest.raises(YsError):
            plain.get_output(key)
    for fn in (plain.det_device, plain.e2e_gains, plain.e2e_update):
        with pytest.raises(YsError):
            fn()
    plain.set_preds(c["preds"])
    _, pitems = M.v8PoseLoss(plain)(None, c["batch"])
    assert np.allclose(pitems, c["plain_items"], rtol=1e-3, atol=1e-5), (pitems, c["plain_items"])       # one pass, unweighted
    # the detection criterion alone stays refused on an End2End Pose model; ys_model_set_preds feeds both branches
    e2e.set_preds(c["preds"])
    with pytest.raises(YsError, match="ys_loss_pose"):
        M.v8DetectionLoss(e2e)(None, c["batch"])
    _, items = M.v8PoseLoss(e2e)(None, c["batch"])
    assert np.allclose(items, c["items"], rtol=1e-3, atol=1e-5), (items, c["items"])
    for k in HEAD:
        assert np.array_equal(e2e.get_output("one2one_" + k), e2e.get_output(k))
    assert relerr(e2e.get_output("one2one_kpts"), c["preds"]["kpts"]) < 1e-6
    for m in (e2e, plain):
        m.close()


# ---------------------------------------------------------------------------------------------------- 10: bf16
@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("cfg", ["v8", "v11"])
def test_bf16_three_steps_descend(backend, engine, cfg):
    from yolosharp_amd.model import v8PoseLoss
    c = _case(cfg)
    m = _engine_model(engine, c["sd0"], cfg, dtype="bf16")
    m.train()
    crit = v8PoseLoss(m)
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
def test_yolov11s_pose_e2e_full_resolution_f32(backend, engine):
    """The shape of tests/test_obb_pose.py::test_yolov11s_pose_loss_backward_full_resolution_f32 (nc = 4, kmax = 12) with its 1e-3 / 2e-3 tolerances."""
    c = _oracle_step(11, 4, 17, 3, "s", 2, 640, 640, 1, 12)            # weight seed 0, as there
    assert c["fg_before"] > c["fg_after"] > 0, (c["fg_before"], c["fg_after"])       # the second stage prunes at this shape too
    c.update(x=c["x"].numpy(), batch=_np(c["batch"]), family=11)
    m = _engine_model(engine, c["sd0"], (11, 4, 17, 3), h=640, w=640, size="s")
    _check_loss_and_backward(engine, c, m, None, 2e-3)
    m.close()
