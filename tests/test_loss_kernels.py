"""The detection criterion (csrc/loss.hip: 8 kernels) stage by stage against the float64 oracle, on both backends, f32 and bf16.

Every case hands the criterion its predictions through Model.set_preds (no forward runs) and reads back, besides items and gradients, the ASSIGNMENT
(ys_loss_read_targets).  The assertions run in the order of the pipeline, so a failure names the stage: assignment (exact) -> target scores and their
sum -> gradients per element -> items -> a second run is bit-identical.  The cases (tests/loss_cases.py) are the smallest shapes that reach each
data-dependent branch of loss.hip:

  whole640        tal_metrics_pair's one-pass form: a whole-image box holds 8400 > TAL_LIST_CAP anchors
  fallback672     A = 9261 > TAL_REGS * TAL_T: the fallback top-k loop with s_taken (and the one-pass form again); an image of zero metrics for its tie-break
  many_pairs      ~700 live pairs: a workgroup of the flat walk does several pairs, the barrier between them; gcap grown past 64
  empty_and_stray the same with image 1 empty and a block of rows whose batch_idx names no image
  grid_form       B = 1030 > TAL_FLAT_MAXB: the [gcap][B] grid; target-score sum below 1 -> loss_tss_of's clamp
  unstaged_rank   4200 label rows > 4096: loss_prep_body's unstaged rank loop; images interleaved, slot = order of appearance
  ticket_b*       1, 15, 16, 17, 33 workgroups of tal_targets_kernel: n_act / n_sh of the two-level ticket (tss and the gradient scale consume it)
  regmax8 / 20    the run-time instances of loss_decode_kernel / loss_box_kernel; DFL targets clamped at both ends
  nc1 / 3 / 7 / 80  loss_cls_kernel's channel tail and padded row (f32: 4 elements per lane, bf16: 8)
  tiny_zero_last  boxes below stride 8 inflated to 16, a zero-area row, class nc - 1
  zero_ties       pairs with fewer than topk positive metrics: zeros tie, the lowest anchor index wins
  twin_labels     two identical labels of different class: equal overlaps, tal_resolve_kernel keeps the first maximum over all rows
  one2one         End2End Detect: the second pass (tal_topk 1) with its own gradient buffers, on many_pairs' shapes
  obb_*           the rotated criterion (v8OBBLoss): thin boxes dropped / widened, nested rotated boxes; a whole-image box at 640

What this file does not reach: the padded channels of the class-gradient buffer (no entry exposes them; a gradient written there also enters the class
item, which is held), and the one2many assignment of an End2End model (the passes share the workspaces; many_pairs holds it on a plain model)."""
import math

import numpy as np
import pytest

import loss_cases as L
from conftest import BACKENDS

HYP = (7.5, 0.5, 1.5)            # box, cls, dfl (Loss.cs:344); angle 1.0

# dtypes per case, stated here so that collection does not draw the cases (the builders say the same; test_case_table_matches holds the two together)
_BOTH = ("f32", "bf16")
_DTYPES = {"whole640": _BOTH, "fallback672": ("f32",), "many_pairs": _BOTH, "empty_and_stray": ("f32",), "grid_form": ("f32",), "unstaged_rank": ("f32",),
           "ticket_b1": ("f32",), "ticket_b45": ("f32",), "ticket_b46": ("f32",), "ticket_b49": ("f32",), "ticket_b100": ("f32",),
           "regmax8": ("f32",), "regmax20": _BOTH, "nc1": _BOTH, "nc3": _BOTH, "nc7": _BOTH, "nc80": _BOTH, "tiny_zero_last": ("f32",),
           "zero_ties": ("f32",), "twin_labels": ("f32",), "one2one": ("f32",), "obb_thin_nested": _BOTH, "obb_whole640": ("f32",)}


def _params():
    return [pytest.param(name, dt, id="%s-%s" % (name, dt)) for name in _DTYPES for dt in _DTYPES[name]]


def test_case_table_matches():
    assert list(_DTYPES) == list(L.CASES) == list(L.SEEDS)
    for name in L.CASES:
        assert tuple(L.get_case(name)["dtypes"]) == tuple(_DTYPES[name]), name


def item_bounds(c, dtype, ref_items, tss, passes=1):
    """|item - ref| allowed per item: ITEM_R relative + the accumulators' quantum, n_workgroups * 2^-21 / tss * hyp per sum and pass"""
    epl = 8 if dtype == "bf16" else 4
    rows = c["B"] * L.anchors(c["H"], c["W"]).shape[0]
    wg_cls = math.ceil(rows * math.ceil(c["nc"] / epl) / 256)
    wg_box = math.ceil(rows * 4 / 256)
    q = [wg_box * HYP[0], wg_cls * HYP[1], wg_box * HYP[2]] + ([wg_box * 1.0] if c.get("rot") else [])
    return L.ITEM_R * np.abs(ref_items) + passes * np.array(q) * 2.0 ** -21 / tss


def run_engine(engine, c, dtype):
    """one criterion call on the case's predictions -> everything the engine lets a caller read"""
    from yolosharp_amd.model import Yolov8, Yolov8Obb, v8DetectionLoss, v8OBBLoss
    rot, e2e = c.get("rot", False), c.get("e2e", False)
    cls = Yolov8Obb if rot else Yolov8
    m = cls(engine, nc=c["nc"], reg_max=c["reg_max"], size="n", height=c["H"], width=c["W"], max_batch=c["B"], dtype=dtype, end2end=e2e)
    try:
        assert m.A == L.anchors(c["H"], c["W"]).shape[0]
        p = {"boxes": c["preds"]["boxes"], "scores": c["preds"]["scores"]}
        if rot:
            p["angle"] = (1.0 / (1.0 + np.exp(-L.as_stored(c["preds"]["angle_logit"], dtype))) - 0.25) * math.pi
        crit = (v8OBBLoss if rot else v8DetectionLoss)(m)
        runs = []
        for _ in range(2):
            m.set_preds(p)
            loss, items = crit(None, c["batch"])
            gi, ts, tss = crit.read_targets()
            r = {"items": items.astype(np.float64), "loss": float(loss.sum()), "gt_idx": gi, "tscore": ts, "tss": tss,
                 "dboxes": m.get_output("dboxes"), "dscores": m.get_output("dscores")}
            if rot:
                r["dangle"] = m.get_output("dangle")
            if e2e:
                r["one2one_dboxes"] = m.get_output("one2one_dboxes"); r["one2one_dscores"] = m.get_output("one2one_dscores")
            runs.append(r)
        stored = {"boxes": m.get_output("boxes"), "scores": m.get_output("scores")}
    finally:
        m.close()
    return runs[0], runs[1], stored


WORST = {}        # stage -> (ratio, where): the figures DESIGN.md records; printed by every case (pytest -s) and by test_zz_report


def _note(stage, ratio, where):
    if ratio > WORST.get(stage, (0.0, ""))[0]:
        WORST[stage] = (float(ratio), where)


def check_grad(got, ref, dtype, what, stage, rot=False):
    """per element: |got - ref| <= GRAD_R (|ref| + max|ref| / 8) (+ one bf16 rounding of the stored value)"""
    assert np.isfinite(got).all(), what
    mx = np.abs(ref).max()
    err = np.abs(got.astype(np.float64) - ref)
    f32_term = L.GRAD_R[rot] * (np.abs(ref) + mx / 8)
    if dtype == "f32":
        ratio = (err / (np.abs(ref) + mx / 8 + 1e-300)).max()
        print("MEASURE %s %s worst |err| / (|ref| + max|ref| / 8) = %.3g" % (stage, what, ratio))
        _note(stage, ratio, what)
        bound = f32_term
    else:
        bound = f32_term + L.BF16_R * np.abs(ref)
        print("MEASURE %s %s bf16 worst |err| / bound = %.3g" % (stage, what, (err / (bound + 1e-300)).max()))
    bad = np.argwhere(err > bound)
    assert bad.size == 0, (what, len(bad), bad[:4].tolist(), [(float(got[tuple(i)]), float(ref[tuple(i)])) for i in bad[:4]], float(mx))


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("name,dtype", _params())
def test_criterion_stage_by_stage(name, dtype, backend, engine):
    c = L.get_case(name)
    e2e, rot = c.get("e2e", False), c.get("rot", False)
    ref = L.get_reference(name, dtype)                    # End2End: the one2one pass (tal_topk 1), the one whose targets can be read
    ref10 = L.get_reference(name, dtype, topk=10) if e2e else ref
    tag = "%s-%s-%s" % (name, dtype, backend)
    # ---- the case itself: its decisions are no near-ties (re-checked at run time: a seed that stopped satisfying them FAILS)
    for r in (ref, ref10):
        mg = r["margins"]
        print("MARGINS %s %s" % (tag, {k: "%.3g" % v for k, v in mg.items()}))
        assert L.margins_ok(mg), (name, mg)
    _case_premises(name, c, ref)
    got, again, stored = run_engine(engine, c, dtype)
    # the reference was fed what the engine stores
    assert np.array_equal(stored["boxes"].astype(np.float64), L.as_stored(c["preds"]["boxes"], dtype)), "stored boxes"
    assert np.array_equal(stored["scores"].astype(np.float64), L.as_stored(c["preds"]["scores"], dtype)), "stored scores"
    # ---- 1. assignment: foreground set and slot, every anchor
    diff = np.argwhere(got["gt_idx"] != ref["gt_idx"])
    assert diff.size == 0, ("assignment", tag, len(diff), [(i.tolist(), int(got["gt_idx"][tuple(i)]), int(ref["gt_idx"][tuple(i)])) for i in diff[:6]])
    fg = ref["fg"]
    # ---- 2. target scores per anchor, and their sum
    ts = got["tscore"].astype(np.float64)
    assert np.array_equal(ts[~fg], np.zeros((~fg).sum())), "background anchors carry no target score"
    if fg.any():
        err, want, cond = np.abs(ts[fg] - ref["tscore"][fg]), ref["tscore"][fg], ref["tscore_cond"][fg]
        assert np.array_equal(ts[fg][want == 0], np.zeros((want == 0).sum())), "a zero metric gives a zero score"
        live = want > 0
        if live.any():
            eps = (np.maximum(err[live] / want[live] - L.TSCORE_R, 0) / cond[live]).max()
            print("MEASURE tscore %s worst (|err| / ref - TSCORE_R) / cond = %.3g; worst relative error %.3g" % (tag, eps, (err[live] / want[live]).max()))
            if dtype == "f32":
                _note("tscore", eps, tag)
        assert (err <= want * (L.TSCORE_R + L.OV_EPS * cond)).all(), ("target scores", tag)
    print("MEASURE tss %s relative error = %.3g (tss %.6g, raw sum %.6g)" % (tag, abs(got["tss"] - ref["tss"]) / ref["tss"], ref["tss"], ref["tsum"]))
    _note("tss", abs(got["tss"] - ref["tss"]) / ref["tss"], tag)
    if ref["tsum"] < 1.0:
        assert got["tss"] == 1.0, ("tss is max(sum, 1)", got["tss"])
    assert abs(got["tss"] - ref["tss"]) <= L.TSS_R * ref["tss"], ("tss", got["tss"], ref["tss"])
    # ---- 3. gradients per element
    pre = "one2one_" if e2e else ""
    assert np.array_equal(got[pre + "dboxes"][np.broadcast_to(~fg[:, None, :], got[pre + "dboxes"].shape)], np.zeros((~fg).sum() * 4 * c["reg_max"])), \
        "background anchors: dboxes exactly 0"
    check_grad(got[pre + "dboxes"], ref["dboxes"], dtype, tag + " " + pre + "dboxes", "dboxes", rot)
    check_grad(got[pre + "dscores"], ref["dscores"], dtype, tag + " " + pre + "dscores", "dscores", rot)
    if rot:
        assert np.array_equal(got["dangle"][:, 0][~fg], np.zeros((~fg).sum())), "background anchors: dangle exactly 0"
        check_grad(got["dangle"], ref["dangle"], dtype, tag + " dangle", "dangle", rot)
    if e2e:                                               # the one2many pass keeps its own buffers
        fg10 = ref10["fg"]
        assert np.array_equal(got["dboxes"][np.broadcast_to(~fg10[:, None, :], got["dboxes"].shape)], np.zeros((~fg10).sum() * 4 * c["reg_max"]))
        check_grad(got["dboxes"], ref10["dboxes"], dtype, tag + " dboxes", "dboxes")
        check_grad(got["dscores"], ref10["dscores"], dtype, tag + " dscores", "dscores")
    # ---- 4. items
    want = ref["items"] + (ref10["items"] if e2e else 0.0)
    bound = item_bounds(c, dtype, ref["items"], ref["tss"]) + (item_bounds(c, dtype, ref10["items"], ref10["tss"]) if e2e else 0.0)
    err = np.abs(got["items"] - want)
    print("MEASURE items %s |err| / bound = %s (items %s)" % (tag, np.array2string(err / bound, precision=3), np.array2string(want, precision=6)))
    _note("items", (err / np.maximum(np.abs(want), 1e-30)).max(), tag)
    assert (err <= bound).all(), ("items", tag, got["items"].tolist(), want.tolist(), bound.tolist())
    wl = ref["loss"] + (ref10["loss"] if e2e else 0.0)
    assert abs(got["loss"] - wl) <= bound.sum() * c["B"] + 2.0 ** -22 * abs(wl), ("loss", got["loss"], wl)
    # ---- 5. a second run of the same case: bit-identical targets, gradients and items
    for k in got:
        assert np.array_equal(np.asarray(got[k]), np.asarray(again[k])), ("rerun differs", tag, k)


def _case_premises(name, c, ref):
    """what a case exists for, asserted from the REFERENCE (so a change of the generator cannot quietly lose the branch)"""
    d = ref["diag"]
    A = L.anchors(c["H"], c["W"]).shape[0]
    if name in ("whole640", "fallback672", "obb_whole640"):
        assert A == {"whole640": 8400, "fallback672": 9261, "obb_whole640": 8400}[name]
        assert int(d["mask_in_gts"][0, 0].sum()) == A > 8192                    # nin > TAL_LIST_CAP
    if name == "fallback672":                                                    # image 1: all metrics zero, the ten lowest anchors are the positives
        assert not (d["align_metric"][1] > 0).any() and ref["fg"][1, :10].all() and ref["fg"][1].sum() == 10
    if name in ("many_pairs", "empty_and_stray", "one2one"):
        assert int(d["mask_gt"].sum()) > 256 and d["mask_gt"].shape[1] > 64
    if name == "empty_and_stray":
        bi = c["batch"]["batch_idx"]
        assert not (bi == 1).any() and ((bi < 0) | (bi >= c["B"])).sum() == 60 and not ref["fg"][1].any()
    if name == "grid_form":
        bi = c["batch"]["batch_idx"]
        assert c["B"] > 1024 and len(bi) > 1400 and len(np.unique(bi)) < c["B"] - 100
        assert 0.05 < ref["tsum"] < 0.9 and ref["tss"] == 1.0
    if name == "unstaged_rank":
        bi = c["batch"]["batch_idx"]
        assert len(bi) > 4096 and (np.diff(bi) < 0).sum() > 1000                # interleaved: a slot is a rank, not a position
    if name.startswith("ticket_b"):
        assert math.ceil(c["B"] * A / 256) == {1: 1, 45: 15, 46: 16, 49: 17, 100: 33}[c["B"]]
    if name.startswith("regmax"):
        t = ref["dfl_t"]
        assert (t < 0).any() and (t > c["reg_max"] - 1.01).any(), (t.min(), t.max())     # both clamps of the DFL target
    if name == "tiny_zero_last":
        g = d["gt_bboxes"]
        w, h = g[..., 2] - g[..., 0], g[..., 3] - g[..., 1]
        valid = d["mask_gt"].bool().squeeze(-1)
        assert ((w < 8) & (h < 8) & valid).any() and (~valid[0, :7]).sum() == 1   # tiny boxes; the zero-area row holds slot 3 of image 0
        assert not valid[0, 3]
        cl = c["batch"]["cls"][c["batch"]["batch_idx"] == 0]
        assert cl[0] == c["nc"] - 1 and (ref["gt_idx"][0] == 0).any()           # the last class is assigned somewhere
    if name == "zero_ties":
        pos = (d["align_metric"] > 0).sum(-1)[d["mask_gt"].bool().squeeze(-1)]
        assert (pos < 10).any()
        zero_fg = ref["fg"] & (ref["tscore"] == 0)
        assert zero_fg[0, :10].all() and zero_fg.sum() == 10                    # anchors assigned on a zero metric: the lowest indices, inside the box
        assert (d["claims"][0, :10] > 1).sum() == 6 and (ref["gt_idx"][0, :10] == 0).sum() == 6 and not d["mask_pos"][0, 0].any()   # ... and row 0 takes the shared ones
    if name == "twin_labels":
        ov = d["overlaps"]
        n0 = int((c["batch"]["batch_idx"] == 0).sum())
        assert np.array_equal(ov[0, 1].numpy(), ov[0, n0 - 1].numpy()) and float(ov[0, 1].max()) > 0.3
        shared = (d["mask_pos"][0, 1] * d["mask_pos"][0, n0 - 1]).bool().numpy()       # (the twins' classes differ, so their top-k sets differ too)
        assert shared.sum() >= 3 and (ref["gt_idx"][0][shared] == 1).any() and not (ref["gt_idx"][0][shared] == n0 - 1).any()    # the first twin wins every shared anchor
    if name == "obb_thin_nested":
        bb = c["batch"]["bboxes"]
        assert ((bb[:, 2] * c["W"] < 2) | (bb[:, 3] * c["H"] < 2)).sum() == 2 and ((bb[:, 2] * c["W"] >= 2) & (bb[:, 2] * c["W"] < 8)).sum() == 2
        assert int(d["mask_gt"].sum()) == len(bb) - 2                           # the dropped labels take no slot
        assert (d["gt_bboxes"][..., 2] == 16).sum() == 2                        # the thin ones were widened to stride 16


def test_zz_report():
    """the worst figure per stage over the cases that ran in this process (what DESIGN.md's table records); always passes"""
    for k, (v, where) in sorted(WORST.items()):
        print("WORST %-8s %.3g  (%s)" % (k, v, where))


@pytest.mark.parametrize("backend", BACKENDS)
def test_read_targets_is_refused_without_an_assignment(backend, engine):
    """ys_loss_read_targets: before a criterion has run (also again after new predictions) and on a classify model there is nothing to read"""
    from yolosharp_amd import YsError
    from yolosharp_amd.model import Yolov8, Yolov8Classify, v8DetectionLoss
    c = L.get_case("ticket_b1")
    m = Yolov8(engine, nc=c["nc"], size="n", height=c["H"], width=c["W"], max_batch=1, dtype="f32")
    crit = v8DetectionLoss(m)
    m.set_preds({"boxes": c["preds"]["boxes"], "scores": c["preds"]["scores"]})
    with pytest.raises(YsError, match="no loss has run"):
        crit.read_targets()
    crit(None, c["batch"])
    gi, ts, tss = crit.read_targets()
    assert np.array_equal(gi, L.get_reference("ticket_b1", "f32")["gt_idx"])
    m.set_preds({"boxes": c["preds"]["boxes"], "scores": c["preds"]["scores"]})
    with pytest.raises(YsError, match="no loss has run"):
        crit.read_targets()
    m.close()
    m = Yolov8Classify(engine, nc=5, size="n", height=64, width=64, max_batch=2, dtype="f32")
    m._batch, m.A = 2, 1
    with pytest.raises(YsError, match="classify"):
        v8DetectionLoss(m).read_targets()
    m.close()
