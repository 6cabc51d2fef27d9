"""detect_decode_kernel (csrc/elementwise.hip) -- the DFL expectation, the anchor and stride geometry of three levels, the class sigmoid, Obb dist2rbox and
angle, Pose.kpts_decode, the End2End xyxy form -- and the rest of the eval tail (the Segment coefficient append, the End2End top-k) on head values the
test chooses, against a float64 restatement, on both backends, f32 and bf16.

Every case hands the head outputs to the model through Model.set_preds and runs the eval tail alone through Model.decode_preds (ys_model_decode_preds):
no convolution error enters, so each block of `pred` -- boxes, class probabilities, angle, keypoint xy, keypoint visibility -- is held by its own bound
(tests/decode_cases.py: 4x the fp32 oracle's own error against float64), the mask coefficients and the End2End rows bit for bit.  The cases:

  det_nc5_64x96 / 96x64 / 32x32   levels 8x12, 4x6, 2x3 (A = 126: with B = 3 a 64-row workgroup straddles two level boundaries and an image boundary, and
                    the last workgroup is ragged), the level widths swapped, and A = 21 (three images in one workgroup); each followed by a call
                    with batch < max_batch: the images past `batch` keep the earlier call's values in the whole `pred` buffer
  det_nc1 / nc7 / nc80            one class, a count that is no multiple of 4 or 8, one that fills the 16-byte units
  det_e2e_nc7, seg_e2e_nc5, obb_e2e_nc7, pose_e2e_nc3   End2End: xyxy boxes (Obb: unchanged xywh), "det" == Engine.e2e_topk(pred) bit for bit
  seg_nc5           pred[:, 4+nc:] == the stored coefficients bit for bit, B = 3
  obb_nc7, pose_nc3_k17d3, pose_nc1_k5d2   the angle channel behind an odd class count; kpt_dim 3 and 2 (the engine refuses every other kpt_dim)
  dfl_onehot / flat / underflow / tie   rows one-hot at +-30 at bins 0, 7, 15 (the expectation is the bin); all-equal rows (dist exactly 7.5: the centre
                    is anchor x stride and the side 15 x stride, exactly); a spread beyond exp underflow; two equal maxima
  sat_detect / obb / pose         class, angle and visibility logits 0, +-20, +-90: 0.5 exactly at 0, finite, inside [0, 1], monotone; the ends of
                    [-pi/4, 3pi/4]

The refusal boundary of ys_detect_decode_launch (its LDS image above 60 KB): nc = 169 decodes, nc = 170 is refused with YS_ERR_UNSUPPORTED."""
import math
import time

import numpy as np
import pytest

import decode_cases as DC
from conftest import BACKENDS

_DTYPES = ("f32", "bf16")


def _model(engine, c, dtype, **kw):
    from yolosharp_amd import model as M
    cls = {"detect": M.Yolov8, "segment": M.Yolov8Segment, "obb": M.Yolov8Obb, "pose": M.Yolov8Pose}[c["task"]]
    if c["task"] == "pose":
        kw.update(kpt_num=c["K"], kpt_dim=c["D"])
    m = cls(engine, nc=c["nc"], reg_max=c["reg_max"], size="n", height=c["H"], width=c["W"], max_batch=c["B"], dtype=dtype, **kw)
    if c["e2e"]:
        {"detect": m.one2one_init, "segment": getattr(m, "e2e_init", None), "obb": getattr(m, "e2e_obb_init", None),
         "pose": getattr(m, "e2e_pose_init", None)}[c["task"]](300)
    m.eval()
    return m


def test_case_table():
    assert list(DC.CASES) == list(DC.SEEDS)
    assert DC.n_anchors(64, 96) == 126 and DC.n_anchors(32, 32) == 21
    tasks = {DC.get_case(n)["task"] for n in DC.CASES}
    assert tasks == {"detect", "segment", "obb", "pose"}


def test_bounds_table_is_the_measured_one():
    """where BOUNDS comes from: the fp32 oracle against decode64, per block, over all cases.  Each constant is 4x the worst figure rounded up to a power of
    two.  fp32 library code differs a little from machine to machine, so the assertion is the rule with one binade of slack: the oracle stays inside a
    quarter of the bound, and the bound is pow2ceil(4 x worst) or, where the worst figure came out a little lower here, twice that"""
    worst = {}
    for name in DC.CASES:
        for k, v in DC.oracle32(name).items():
            print("MEASURE oracle32 %s %s = %.3g" % (name, k, v))
            worst[k] = max(worst.get(k, 0.0), v)
    assert set(worst) == set(DC.BOUNDS)
    for k, v in worst.items():
        print("WORST oracle32 %s %.3g (bound %.3g)" % (k, v, DC.BOUNDS[k]))
        assert 4 * v <= DC.BOUNDS[k], (k, v)
        assert DC.BOUNDS[k] in (DC.pow2ceil(4 * v), 2 * DC.pow2ceil(4 * v)), (k, v)


def _read(m, c):
    out = {"pred": m.get_output("pred")}
    if c["e2e"]:
        out["det"] = m.get_output("det")
    return out


def _check_blocks(c, pred, ref, tag):
    got = DC.split_pred(c, pred)
    assert np.isfinite(pred).all(), tag
    figs = DC.figures(c, got, ref)
    for k, v in figs.items():
        print("MEASURE %s %s = %.3g (bound %.3g)" % (tag, k, v, DC.BOUNDS[k]))
    for k, v in figs.items():
        assert v <= DC.BOUNDS[k], (tag, k, v, DC.BOUNDS[k])
    return got


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dtype", _DTYPES)
@pytest.mark.parametrize("name", list(DC.CASES))
def test_decode_on_chosen_preds(name, dtype, backend, engine):
    c = DC.get_case(name)
    ref = DC.get_reference(name, dtype)
    tag = "%s-%s-%s" % (name, dtype, backend)
    DC.premises(name, c, ref)
    B, nc, A = c["B"], c["nc"], c["A"]
    t0 = time.perf_counter()
    m = _model(engine, c, dtype)
    try:
        assert m.A == A
        m.set_preds(c["preds"])
        m.decode_preds()
        first = _read(m, c)
        m.decode_preds()
        again = _read(m, c)
        s = DC.stored(c, dtype)
        keys = {"boxes": "boxes", "scores": "scores"}
        if c["task"] in ("segment", "pose"):
            keys[DC.extra_key(c)] = DC.extra_key(c)
        for k, g in keys.items():                            # the reference was fed what the engine stores
            assert np.array_equal(m.get_output(g).astype(np.float64), s[k]), "stored " + k
        if c["task"] == "obb":                                # "angle" reads the stored logit back through the angle form (obb_angle_kernel, the same arithmetic):
            # saturated logits arrived unchanged.  The table's angle bound, per element
            ra = ref["angle"]
            assert (np.abs(m.get_output("angle") - ra) <= DC.BOUNDS["angle"] * (np.abs(ra) + np.abs(ra).max() / 8)).all()
        whole = None
        if c["partial"]:
            Cc = 4 + nc + m.NM
            whole = engine.from_device(m.pred_device(), (B, Cc, A), np.float32)
            c2 = DC.second_preds(c)
            m.set_preds(c2["preds"])
            m.decode_preds()
            whole2 = engine.from_device(m.pred_device(), (B, Cc, A), np.float32)
            part = m.get_output("pred")
    finally:
        m.close()
    print("TIME %s engine %.2f s" % (tag, time.perf_counter() - t0))
    pred = first["pred"]
    assert pred.shape == (B, 4 + nc + (m.NM if c["task"] != "detect" else 0), A)
    # ---- a second call: bit-identical
    for k in first:
        assert np.array_equal(first[k], again[k]), ("rerun differs", tag, k)
    # ---- every block against float64
    got = _check_blocks(c, pred, ref, tag)
    # ---- exact statements
    if c["task"] == "segment":
        assert np.array_equal(got["coef"], ref["coef"]), "mask coefficients are appended bit for bit"
    if c["e2e"]:
        rows, _ = engine.e2e_topk(pred, 300, extra=m.NM if c["task"] != "detect" else 0)
        assert first["det"].shape == rows.shape and np.array_equal(first["det"], rows), "det == e2e_topk(pred)"
    if name == "dfl_flat":
        gx, gy, st = DC.grid(c["H"], c["W"])
        assert np.array_equal(pred[:, 0], np.broadcast_to((gx + 0.5) * st, (B, A))) and np.array_equal(pred[:, 1], np.broadcast_to((gy + 0.5) * st, (B, A)))
        assert np.array_equal(pred[:, 2], np.broadcast_to(15 * st, (B, A))) and np.array_equal(pred[:, 3], np.broadcast_to(15 * st, (B, A)))
    if name.startswith("sat_"):
        sat = [(c["preds"]["scores"], got["prob"], True)] if name != "sat_pose" else []
        if name == "sat_obb":                                 # the ends of [-pi/4, 3pi/4]: the table's angle bound in its per-element form, R (|end| + max|ref| / 8)
            z = c["preds"]["angle_logit"]
            sat.append((z, got["angle"], False))
            for v, end in ((90, 0.75 * math.pi), (-90, -0.25 * math.pi)):
                assert np.abs(got["angle"][z == v] - end).max() <= DC.BOUNDS["angle"] * (abs(end) + 0.75 * math.pi / 8)
        if name == "sat_pose":
            sat.append((c["preds"]["kpts"].reshape(B, c["K"], c["D"], A)[:, :, 2], got["kvis"], True))
        for z, p, prob in sat:
            lv = [(float(p[z == v].min()), float(p[z == v].max())) for v in DC.SAT]
            assert all(lv[i][1] <= lv[i + 1][0] for i in range(4)), ("monotone", tag, lv)
            if prob:
                assert (p >= 0).all() and (p <= 1).all()
                assert (p[z == 0] == 0.5).all()
                # sigmoid(-90) = 8e-40 is below every fp32 normal: what the prob bound leaves at |ref| = 0 is R max|ref| / 8 = R / 8; 1 - 8e-40 is 1.0 in fp32
                assert lv[0][1] <= DC.BOUNDS["prob"] / 8 and lv[4][0] == 1.0
    # ---- batch < max_batch after the full call: the images past `batch` keep the earlier values, the others are the new decode
    if c["partial"]:
        assert np.array_equal(whole, pred)
        assert np.array_equal(whole2[B - 1:], whole[B - 1:]), "the image past `batch` was written"
        assert np.array_equal(whole2[:B - 1], part)
        _check_blocks(c2, part, DC.decode64(c2, DC.stored(c2, dtype)), tag + "-partial")


# ----------------------------------------------------------------------------- standalone head handles (ys_head_create) take the same entry
@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("name", ["det_nc5_64x96", "seg_nc5"])
def test_decode_on_head_handle(name, backend, engine):
    """the cases of the full models on a standalone Detect / Segment head: the same blocks, the coefficients bit for bit, and after an eval forward of the head
    decode_preds() leaves `pred` as it is"""
    from yolosharp_amd import heads
    c = DC.get_case(name)
    ref = DC.get_reference(name, "f32")
    ch = (16, 32, 64)
    m = (heads.Segment if c["task"] == "segment" else heads.Detect)(engine, nc=c["nc"], ch=ch, height=c["H"], width=c["W"], max_batch=c["B"], dtype="f32")
    try:
        m.eval()
        assert m.A == c["A"]
        m.set_preds(c["preds"])
        m.decode_preds()
        got = _check_blocks(c, m.get_output("pred"), ref, "head-%s-%s" % (name, backend))
        if c["task"] == "segment":
            assert np.array_equal(got["coef"], ref["coef"])
        m.init_weights(2)
        rng = np.random.default_rng(4)
        inf, _ = m.forward([rng.random((c["B"], k, c["H"] // s, c["W"] // s), dtype=np.float32) for k, s in zip(ch, (8, 16, 32))])
        m.decode_preds()
        assert np.isfinite(inf["boxes"]).all() and np.array_equal(inf["boxes"], m.get_output("pred"))
    finally:
        m.close()


# ----------------------------------------------------------------------------- the refusal boundary
@pytest.mark.parametrize("backend", BACKENDS)
def test_decode_nc_limit(backend, engine):
    """ys_detect_decode_launch refuses an LDS image above 60 KB: 64 anchors x ((4 * 16 + 1) + (nc | 1) + 4 + 1) floats x 4 bytes <= 61440 <=> (nc | 1) <= 170, so
    a Detect model with reg_max 16 decodes up to nc = 169 and is refused from nc = 170 on (the reference has no such limit: DESIGN.md)"""
    from yolosharp_amd import YsError
    lds = lambda nc: 64 * ((4 * 16 + 1) + (nc | 1) + 4 + 1) * 4
    assert lds(169) <= 60 * 1024 < lds(170)
    for nc in (169, 170):
        c = DC._case("detect", 32, 64, 2, nc, 5)
        m = _model(engine, c, "f32")
        try:
            m.set_preds(c["preds"])
            if nc == 169:
                m.decode_preds()
                _check_blocks(c, m.get_output("pred"), DC.decode64(c, DC.stored(c, "f32")), "nc169-" + backend)
            else:
                with pytest.raises(YsError) as ei:
                    m.decode_preds()
                assert ei.value.status == 4 and "detect decode: nc=170 reg_max=16 too large" in str(ei.value)
        finally:
            m.close()


# ----------------------------------------------------------------------------- the entry itself
@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("task", ["detect", "segment", "obb", "pose", "detect_e2e"])
def test_eval_forward_unchanged_by_decode_preds(task, backend, engine):
    """forward, read pred, decode_preds(), read pred again: equal bit for bit (the tail of the forward IS what decode_preds runs)"""
    c = DC._case(task.split("_")[0], 64, 64, 2, 3, 9, e2e=task.endswith("e2e"))
    m = _model(engine, c, "f32")
    try:
        m.init_weights(3)
        x = np.random.default_rng(1).random((2, 3, 64, 64), dtype=np.float32)
        m.forward(x, fetch=False)
        a = _read(m, c)
        m.decode_preds()
        b = _read(m, c)
    finally:
        m.close()
    for k in a:
        assert np.isfinite(a[k]).all() and np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("backend", BACKENDS)
def test_decode_preds_refusals(backend, engine):
    from yolosharp_amd import YsError
    from yolosharp_amd import model as M
    c = DC._case("detect", 32, 64, 1, 3, 5)
    m = M.Yolov8(engine, nc=3, size="n", height=32, width=64, max_batch=1, dtype="f32")
    try:
        m.eval()
        with pytest.raises(YsError, match="needs ys_model_set_preds or a forward first") as ei:
            m.decode_preds()
        assert ei.value.status == 1
        m.train()
        m.set_preds(c["preds"])
        with pytest.raises(YsError, match="training mode"):
            m.decode_preds()
        m.eval()
        m.decode_preds()
    finally:
        m.close()
    k = M.Yolov8Classify(engine, nc=3, size="n", height=32, width=64, max_batch=1, dtype="f32")
    try:
        k.eval()
        with pytest.raises(YsError, match="not a detection-family model"):
            k.decode_preds()
    finally:
        k.close()
