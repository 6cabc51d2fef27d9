"""End2End detection (Config.End2End): aliased one2one towers, E2EDetectLoss, the two-pass head backward, the top-k post-process and
its thresholding, Detector(end2end=True), the task boundary.  Oracle = tests/e2e_ref.py over oracle/yolo_oracle.py
(Modules/Head.cs:89-127, 152-202; Utils/Loss.cs:1094-1118; Utils/Ops.cs:258-267).  fp32 tolerance 1e-3; the post-process is compared exactly."""
import copy
import functools
import os

import numpy as np
import pytest
import torch

import e2e_ref as R
from conftest import BACKENDS
from oracle import yolo_oracle as O
from test_model import assert_pred_blocks, make_ref, make_ref11, relerr

B, H, W, NC = 2, 64, 64, 7          # A = 84; nc = 7 is not a multiple of the 16-byte channel unit
HERE = os.path.dirname(os.path.abspath(__file__))


def _cls(family):
    from yolosharp_amd import model as M
    return M.Yolov8 if family == 8 else M.Yolov11


def _engine_model(engine, sd, family, end2end=True, dtype="f32", max_det=300, h=H, w=W, b=B):
    m = _cls(family)(engine, nc=NC, size="n", height=h, width=w, max_batch=b, dtype=dtype, end2end=end2end, max_det=max_det)
    m.load_state_dict(sd)
    return m


def _np(d):
    return {k: v.numpy() for k, v in d.items()}


@functools.lru_cache(maxsize=None)
def _case(family):
    """Everything the oracle says about one End2End step of the test shape, computed once per family and never modified."""
    net = (make_ref if family == 8 else make_ref11)(nc=NC, size="n")
    sd0 = {k: v.detach().clone().numpy() for k, v in net.state_dict().items()}
    x = torch.rand(B, 3, H, W, generator=torch.Generator().manual_seed(3))
    batch = O.synthetic_batch(B, H, W, NC, seed=5, kmax=5)
    ev = R.E2E(copy.deepcopy(net)).eval()
    with torch.no_grad():
        rinf, _ = ev(x)
    ref = R.E2E(net).train()
    _, rpreds = ref(x)
    for br in ("one2many", "one2one"):
        for k in ("boxes", "scores"):
            rpreds[br][k].retain_grad()
    rloss, ritems = R.E2EDetectLoss(NC)(rpreds, batch)
    rloss.sum().backward()
    # the one2many criterion alone on a second copy: what a model without the one2one branch sends into the trunk
    plain = (make_ref if family == 8 else make_ref11)(nc=NC, size="n").train()
    _, ppreds = plain(x)
    ploss, _ = O.v8DetectionLoss(NC)(ppreds, batch)
    ploss.sum().backward()
    return dict(sd0=sd0, x=x.numpy(), batch=_np(batch), pred=rinf["pred"].numpy(), rows=rinf["boxes"].numpy(),
                boxes=rpreds["one2many"]["boxes"].detach().numpy(), scores=rpreds["one2many"]["scores"].detach().numpy(),
                items=ritems.numpy(), loss=rloss.detach().numpy(),
                dhead={(br, k): rpreds[br][k].grad.numpy() for br in ("one2many", "one2one") for k in ("boxes", "scores")},
                grads={n: p.grad.numpy() for n, p in net.named_parameters() if p.grad is not None},
                plain_grads={n: p.grad.numpy() for n, p in plain.named_parameters() if p.grad is not None},
                sd1={k: v.detach().clone().numpy() for k, v in net.state_dict().items()},
                head="model.22" if family == 8 else "model.23")


def _step(m, c, backward="whole"):
    from yolosharp_amd.model import v8DetectionLoss
    m.train(); m.zero_grad()
    _, preds = m.forward(c["x"])
    loss, items = v8DetectionLoss(m)(None, c["batch"])
    if backward == "whole":
        m.backward()
    elif backward is not None:
        for seg in range(m.num_segments()):
            if backward == "async":
                m.backward_segment_async(seg); m.segment_fence(seg, 0)
            else:
                m.backward_segment(seg)
    return preds, loss, items


# ---------------------------------------------------------------------------------------------------- 1, 2: training forward, running statistics
@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("family", [8, 11])
def test_training_forward_and_running_statistics(backend, engine, family):
    c = _case(family)
    m = _engine_model(engine, c["sd0"], family)
    assert sorted(n for n, _, _ in m.tensor_info()) == sorted(c["sd0"])                     # one2one_init adds no tensor (the towers alias cv2 / cv3)
    m.train()
    inf, preds = m.forward(c["x"])
    assert inf is None and set(preds) == {"one2many", "one2one"}
    assert relerr(preds["one2many"]["boxes"], c["boxes"]) < 1e-3 and relerr(preds["one2many"]["scores"], c["scores"]) < 1e-3
    for k in ("boxes", "scores"):                                                    # same modules, same input values
        assert np.array_equal(preds["one2one"][k], preds["one2many"][k]), k
    sd = m.state_dict()
    n_head = n_trunk = 0
    for k, r in c["sd1"].items():
        if "running" in k:
            assert np.allclose(sd[k], r, rtol=1e-3, atol=1e-5), k
        elif "num_batches_tracked" in k:
            head = k.startswith(c["head"] + ".")
            assert float(sd[k].reshape(-1)[0]) == float(r) == (2.0 if head else 1.0), k   # towers: two updates per forward; trunk: one
            n_head += head; n_trunk += not head
    assert n_head >= 12 and n_trunk > 20
    # a single update of the towers' statistics is NOT within the tolerance: the check above separates the two
    k = c["head"] + ".cv2.0.0.bn.running_mean"
    once = c["sd0"][k] + (c["sd1"][k] - c["sd0"][k]) / 1.97                          # r1 from r2 = r1 + 0.97 (r1 - r0)
    assert not np.allclose(once, c["sd1"][k], rtol=1e-3, atol=1e-5)
    m.close()


# ---------------------------------------------------------------------------------------------------- 3, 4: loss, head gradients, backward
@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("family", [8, 11])
def test_loss_and_backward(backend, engine, family):
    c = _case(family)
    m = _engine_model(engine, c["sd0"], family)
    _, loss, items = _step(m, c)
    assert np.allclose(items, c["items"], rtol=1e-3, atol=1e-5), (items, c["items"])
    assert np.allclose(loss, c["loss"], rtol=1e-3, atol=1e-4), (loss, c["loss"])
    got = {}
    for br, pre in (("one2many", "d"), ("one2one", "one2one_d")):
        for k in ("boxes", "scores"):
            r = c["dhead"][(br, k)]
            got[(br, k)] = g = m.get_output(pre + k)
            assert np.abs(r).max() > 0 and np.abs(g - r).max() <= 1e-3 * np.abs(r).max(), (br, k, np.abs(g - r).max(), np.abs(r).max())
    for k in ("boxes", "scores"):          # topk 1 assigns fewer anchors than topk 10: the two branches' gradients differ
        d = np.abs(got[("one2one", k)] - got[("one2many", k)]).max()
        assert d > 1e-2 * np.abs(got[("one2many", k)]).max(), k
    # every parameter gradient: towers = both branches summed, trunk = one2many only
    grads = m.grads()
    gscale = max(float(np.abs(r).max()) for r in c["grads"].values())
    assert len(c["grads"]) > 100
    for name, r in c["grads"].items():
        err = np.abs(grads[name] - r).max()
        assert err <= 1e-3 * np.abs(r).max() + 1e-6 * gscale, (name, err, np.abs(r).max())
    # the trunk sees what a model without the one2one branch sends into it for the same one2many loss
    p = _engine_model(engine, c["sd0"], family, end2end=False)
    _step(p, c)
    pg = p.grads()
    last_neck = "model.21.cv2.conv.weight" if family == 8 else "model.22.cv2.conv.weight"
    for name in ("model.0.conv.weight", last_neck):
        assert np.abs(pg[name]).max() > 0
        assert np.abs(grads[name] - pg[name]).max() <= 1e-5 * np.abs(pg[name]).max(), name
        assert np.abs(grads[name] - c["plain_grads"][name]).max() <= 1e-3 * np.abs(c["plain_grads"][name]).max() + 1e-6 * gscale, name
    # ... while the towers' gradients are NOT the one2many ones
    tw = c["head"] + ".cv2.0.2.weight"
    assert np.abs(grads[tw] - pg[tw]).max() > 1e-2 * np.abs(pg[tw]).max()
    p.close(); m.close()


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("family", [8, 11])
def test_segmented_and_overlap_forms_agree(backend, engine, family):
    """ys_model_backward_segment / _segment_async and the one-stream form (ys_model_set_overlap(0)) against the one-call backward:
    the comparison tests/test_dist.py makes for the plain model -- identical gradients."""
    c = _case(family)
    res = {}
    for mode in ("whole", "sync", "async", "no_overlap"):
        m = _engine_model(engine, c["sd0"], family, dtype="bf16")
        if mode == "no_overlap":
            m.set_overlap(False)
        _step(m, c, backward="whole" if mode == "no_overlap" else mode)
        res[mode] = {k: v.copy() for k, v in m.grads().items()}
        m.close()
    for mode in ("sync", "async", "no_overlap"):
        for k, v in res["whole"].items():
            assert np.array_equal(v, res[mode][k]), (mode, k)


# ---------------------------------------------------------------------------------------------------- 5: determinism
@pytest.mark.parametrize("backend", BACKENDS)
def test_two_steps_from_the_same_state_are_bit_identical(backend, engine):
    c = _case(8)
    out = []
    for _ in range(2):
        m = _engine_model(engine, c["sd0"], 8, dtype="bf16")
        _, loss, items = _step(m, c)
        out.append((items.copy(), {k: v.copy() for k, v in m.grads().items()}, m.get_output("one2one_dscores"), m.get_output("dboxes")))
        m.close()
    assert np.array_equal(out[0][0], out[1][0])
    for k in out[0][1]:
        assert np.array_equal(out[0][1][k], out[1][1][k]), k
    assert np.array_equal(out[0][2], out[1][2]) and np.array_equal(out[0][3], out[1][3])


# ---------------------------------------------------------------------------------------------------- 6: ys_e2e_topk standalone
def _tie_free(b, nc, a, seed):
    """[b, 4+nc, a] with pairwise distinct class scores per image: a random permutation of distinct fp32 values in (0, 1)."""
    g = np.random.default_rng(seed)
    n = nc * a
    vals = ((np.arange(n, dtype=np.float64) + 0.5) / n).astype(np.float32)
    assert len(np.unique(vals)) == n and vals.min() > 0 and vals.max() < 1
    pred = np.empty((b, 4 + nc, a), np.float32)
    pred[:, :4] = g.random((b, 4, a), dtype=np.float32) * 640
    for i in range(b):
        pred[i, 4:] = g.permutation(vals).reshape(nc, a)
    return pred


def _check_topk(engine, pred, max_det):
    rows, anchor = engine.e2e_topk(pred, max_det)
    rrows, ridx = R.postprocess(torch.from_numpy(pred), max_det)
    k = min(max_det, pred.shape[2])
    assert rows.shape == (pred.shape[0], k, 6) and anchor.shape == (pred.shape[0], k)
    assert np.array_equal(anchor, ridx.numpy())
    assert np.array_equal(rows[..., 5], rrows[..., 5].numpy())
    assert np.array_equal(rows.view(np.uint32), rrows.numpy().view(np.uint32))       # bit-equal scores and boxes
    return rows


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("b,a,nc,max_det", [(2, 1344, 7, 300),      # k < A
                                            (2, 84, 7, 300),        # k = A < max_det
                                            (2, 1344, 1, 300),      # one class
                                            (2, 1344, 7, 10),       # small max_det
                                            (1, 1, 1, 1), (1, 65, 3, 64),
                                            (1, 2600, 2, 2500)])    # k > 2048: the keys are ordered by the general (global bitonic) path
def test_e2e_topk_exact(backend, engine, b, a, nc, max_det):
    rows = _check_topk(engine, _tie_free(b, nc, a, seed=a + nc), max_det)
    assert np.all(np.diff(rows[..., 4], axis=1) < 0)                 # strictly descending: the input is tie-free


@pytest.mark.parametrize("backend", BACKENDS)
def test_e2e_topk_ties_lower_index_first(backend, engine):
    """Many equal scores, equal per-anchor maxima included: stage 1 keeps the lower anchor, stage 2 the lower [stage-1 rank][class] index."""
    g = np.random.default_rng(9)
    b, a, nc = 2, 1344, 7
    pred = np.zeros((b, 4 + nc, a), np.float32)
    pred[:, :4] = g.random((b, 4, a), dtype=np.float32) * 64
    pred[:, 4:] = g.integers(0, 6, (b, nc, a)).astype(np.float32) / 8          # six distinct values: almost every maximum is shared
    pred[1, 4:] = 0.5                                                          # one image with every score equal
    for max_det in (300, 5):
        rows = _check_topk(engine, pred, max_det)
        assert np.array_equal(rows[1, :, 5], np.arange(min(max_det, 300)) % nc)  # all equal: anchors 0, 0, ..., classes 0..6 in order
    pz = pred.copy(); pz[0, 4:][pz[0, 4:] == 0] = -0.0                          # +0 and -0 are one value
    assert np.array_equal(engine.e2e_topk(pz, 1344)[1], engine.e2e_topk(pred, 1344)[1])


@pytest.mark.gpu
@pytest.mark.parametrize("b,a,nc", [(2, 8400, 80), (1, 33600, 80)])
def test_e2e_topk_exact_large(b, a, nc):
    from yolosharp_amd import Engine
    _check_topk(Engine(), _tie_free(b, nc, a, seed=a), 300)


# ---------------------------------------------------------------------------------------------------- 7: eval forward
@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("family", [8, 11])
def test_eval_forward(backend, engine, family):
    c = _case(family)
    m = _engine_model(engine, c["sd0"], family)
    m.eval()
    inf, preds = m.forward(c["x"])
    assert inf["pred"].shape == (B, 4 + NC, m.A) and inf["boxes"].shape == (B, min(300, m.A), 6)
    assert relerr(inf["pred"], c["pred"]) < 1e-3                                        # xyxy * stride | sigmoid
    assert_pred_blocks(inf["pred"], c["pred"], NC, 1e-3, tag="e2e v%d" % family)        # ... and boxes and probabilities each on their own
    assert np.all(inf["pred"][:, 2] > inf["pred"][:, 0]) and np.all(inf["pred"][:, 3] > inf["pred"][:, 1])
    # "det" = the restatement applied to the ENGINE's own pred, exactly (a 1e-3 forward difference may reorder near-equal scores)
    rrows, _ = R.postprocess(torch.from_numpy(inf["pred"]))
    assert np.array_equal(inf["boxes"].view(np.uint32), rrows.numpy().view(np.uint32))
    assert relerr(np.sort(inf["boxes"][..., 4], 1), np.sort(c["rows"][..., 4], 1)) < 1e-3
    m.close()


# ---------------------------------------------------------------------------------------------------- 8: ys_e2e_select
@pytest.mark.parametrize("backend", BACKENDS)
def test_e2e_select(backend, engine):
    from yolosharp_amd import YsError
    rows, _ = engine.e2e_topk(_tie_free(2, 7, 1344, seed=2), 300)
    rows[1, :, 4] *= 0.2                                             # an image whose scores mostly fall under the thresholds
    rows[1, 40:, 4] = 0.0
    for conf in (0.0, 0.1, 0.999):
        for max_det in (300, 17):
            want = [len(r) for r in R.select(torch.from_numpy(rows), conf, max_det)]
            assert engine.e2e_select(rows, conf, max_det).tolist() == want, (conf, max_det)
            out, keepi = engine.non_max_suppression(rows, conf, 0.7, max_det=max_det, end2end=True)
            for b in range(2):
                assert np.array_equal(out[b], R.select(torch.from_numpy(rows), conf, max_det)[b].numpy())
    assert engine.e2e_select(rows, 0.0, 300).tolist() == [300, 40]   # score > 0 is strict
    for bad in (-0.1, 1.5):
        with pytest.raises(YsError) as e:
            engine.e2e_select(rows, bad)
        assert e.value.status == 1


# ---------------------------------------------------------------------------------------------------- 9: Detector(end2end=True)
def _bus(backend):
    """tests/golden/bus_480x640.jpg as uint8 [3, h, w]: the whole picture on the GPU; its 64 x 48 centre crop through the interpreter (a
    640 x 480 forward takes it minutes) -- the same code path either way: pad to a multiple of 32 with 114, / 255, eval forward, "det", select."""
    from PIL import Image
    im = np.asarray(Image.open(os.path.join(HERE, "golden", "bus_480x640.jpg")).convert("RGB"), np.uint8)
    im = np.ascontiguousarray(im.transpose(2, 0, 1))
    return im if backend == "gpu" else np.ascontiguousarray(im[:, 288:352, 216:264])


@pytest.mark.parametrize("backend", BACKENDS)
def test_detector_end2end_predict_and_val(backend, engine):
    from yolosharp_amd.detector import Detector, YoloResult, pad_to_32
    c = _case(8)
    img = _bus(backend)
    h, w = (img.shape[1] + 31) // 32 * 32, (img.shape[2] + 31) // 32 * 32
    m = _engine_model(engine, c["sd0"], 8, h=h, w=w, b=1)
    det = Detector(m)
    assert det.end2end
    res = det.ImagePredict(img, predict_threshold=0.001)
    m.eval()
    inf, _ = m.forward(pad_to_32(img.astype(np.float32))[None])
    want = R.select(R.postprocess(torch.from_numpy(inf["pred"]))[0], 0.001)[0].numpy()
    assert 0 < len(want) and len(res) == len(want)
    for r, wr in zip(res, want):
        e = YoloResult(wr)
        assert (r.ClassID, r.Score, r.CenterX, r.CenterY, r.Width, r.Height) == (e.ClassID, e.Score, e.CenterX, e.CenterY, e.Width, e.Height)
    m.close()
    with pytest.raises(ValueError):
        p = _engine_model(engine, c["sd0"], 8, end2end=False)
        try:
            Detector(p, end2end=True)
        finally:
            p.close()
    # ---- Val: E2E loss items on the eval preds, the kept rows = the restatement's on the engine's own pred
    from yolosharp_amd import metrics as M
    m = _engine_model(engine, c["sd0"], 8)
    data = dict(c["batch"]); data["images"] = c["x"]
    loss_items, (P, Rc, m50, m5095) = Detector(m).Val([data], conf_thres=0.001)
    ev = R.E2E((make_ref)(nc=NC, size="n")).eval()
    with torch.no_grad():
        _, rpreds = ev(torch.from_numpy(c["x"]))
        _, ritems = R.E2EDetectLoss(NC)(rpreds, {k: torch.from_numpy(v) for k, v in c["batch"].items()})
    assert np.allclose(loss_items, ritems.numpy(), rtol=1e-3, atol=1e-5), (loss_items, ritems)
    inf, _ = m.forward(c["x"])
    kept = R.select(R.postprocess(torch.from_numpy(inf["pred"]))[0], 0.001)
    tb = {k: torch.from_numpy(v) for k, v in c["batch"].items()}
    tp = [O.val_match_image(kept[b], tb, b, W, H) for b in range(B)]
    stats = M.ap_per_class(np.concatenate([np.asarray(t) for t in tp]), np.concatenate([r[:, 4].numpy() for r in kept]),
                           np.concatenate([r[:, 5].numpy() for r in kept]), c["batch"]["cls"])
    assert np.allclose((P, Rc, m50, m5095), M.val_summary(stats), atol=1e-6)
    m.close()


# ---------------------------------------------------------------------------------------------------- 10: boundaries
@pytest.mark.parametrize("backend", BACKENDS)
def test_boundaries(backend, engine, tmp_path):
    from yolosharp_amd import YsError, weights_bin
    from yolosharp_amd import model as M
    for cls in (M.Yolov8Segment, M.Yolov8Obb, M.Yolov11Pose, M.Yolov8Classify):
        with pytest.raises(YsError) as e:
            cls(engine, nc=NC, size="n", height=32, width=32, max_batch=1, dtype="f32", end2end=True)
        assert e.value.status == 4, cls                                               # YS_ERR_UNSUPPORTED
    c = _case(8)
    e2e = _engine_model(engine, c["sd0"], 8)
    plain = M.Yolov8(engine, nc=NC, size="n", height=H, width=W, max_batch=B, dtype="f32")
    assert e2e.tensor_info() == plain.tensor_info() and e2e.num_params() == plain.num_params()
    # `.bin` round trip: E2E -> plain -> E2E
    f1, f2 = str(tmp_path / "e2e.bin"), str(tmp_path / "plain.bin")
    weights_bin.save_from(e2e, f1); weights_bin.load_into(plain, f1)
    psd = plain.state_dict()
    for k, v in e2e.state_dict().items():
        assert np.array_equal(v, psd[k]), k
    e2e.init_weights(7)                                                               # ... back into the End2End model, over other weights
    assert not np.array_equal(e2e.state_dict()["model.0.conv.weight"], psd["model.0.conv.weight"])
    weights_bin.save_from(plain, f2); weights_bin.load_into(e2e, f2)
    esd = e2e.state_dict()
    assert all(np.array_equal(v, esd[k]) for k, v in psd.items())
    # a model without one2one_init behaves as before: xywh "pred", one criterion pass, and the new keys are refused
    plain.eval()
    inf, preds = plain.forward(c["x"])
    assert set(inf) == {"boxes"} and set(preds) == {"boxes", "scores"}
    e2e.eval()
    einf, _ = e2e.forward(c["x"])
    xyxy = einf["pred"][:, :4]
    assert np.allclose(inf["boxes"][:, 0], (xyxy[:, 0] + xyxy[:, 2]) / 2, rtol=1e-5, atol=1e-4) and np.allclose(inf["boxes"][:, 2], xyxy[:, 2] - xyxy[:, 0], rtol=1e-5, atol=1e-4)
    assert np.array_equal(inf["boxes"][:, 4:], einf["pred"][:, 4:])
    for key in ("det", "one2one_boxes", "one2one_dscores"):
        with pytest.raises(YsError):
            plain.get_output(key)
    with pytest.raises(YsError):
        plain.det_device()
    with pytest.raises(YsError):
        e2e.one2one_init()                                                            # once
    # ys_model_set_preds feeds both branches
    from yolosharp_amd.model import v8DetectionLoss
    e2e.set_preds({"boxes": c["boxes"], "scores": c["scores"]})
    _, items = v8DetectionLoss(e2e)(None, c["batch"])
    assert np.allclose(items, c["items"], rtol=1e-3, atol=1e-5)
    assert np.array_equal(e2e.get_output("one2one_boxes"), e2e.get_output("boxes"))
    for m in (e2e, plain):
        m.close()


# ---------------------------------------------------------------------------------------------------- 11: bf16
@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("family", [8, 11])
def test_bf16_three_steps_descend(backend, engine, family):
    from yolosharp_amd.model import v8DetectionLoss
    c = _case(family)
    m = _engine_model(engine, c["sd0"], family, dtype="bf16")
    m.train()
    crit = v8DetectionLoss(m)
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
