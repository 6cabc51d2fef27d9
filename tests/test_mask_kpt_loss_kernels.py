"""The mask term (csrc/segloss.hip: seg_count / offsets / compact, seg_anchor, seg_proto_grad, seg_finalize) and the keypoint terms (csrc/poseloss.hip:
pose_entry, pose_finalize) stage by stage against the float64 oracle, on both backends, f32 and bf16.

Like tests/test_loss_kernels.py every case hands the criterion its predictions through Model.set_preds and reads back the assignment, the items and the
gradients; the assertions run in the order of the pipeline, so a failure names the stage: assignment (exact) -> background exactly 0 -> gradients per
element -> items -> a second run is bit-identical.  The cases (tests/mask_kpt_cases.py) are the smallest shapes that reach each branch:

  seg_rect         24 x 40 mask (mh != mw, 3.75 workgroups of pass 2 with 6.4 rows each): every row / column computation; > SG_ECH entries with a partly
                   filled last chunk next to an image below one chunk; crops clipped at all four borders; pass 2's uniform row skip; overlapping labels;
                   the seg item in both crop modes; f32 and bf16
  seg_wide_row     8 x 264 mask: a row wider than a workgroup (wr0 == wr1 inside a row, wr0 != wr1 across a row end), the ragged last workgroup
  seg_empty_mid    an image without foreground between two that have some (off[b] == off[b + 1]); label rows that name no image
  seg_many         more than 2048 entries: a workgroup of pass 1 walks two entries and reuses sco / sred
  seg_trunc_mixed  the truncating crop, which applies per image: one image at or above 50 foreground anchors, one below
  seg_thin_tiny    an empty crop (still counted in ntot), a box below stride 8 in both sides, a zero-area row
  seg_e2e          End2End: both passes, gains stepped off their initial values; dproto is the one2many term alone
  pose_rect        H != W, all three levels, a label without a visible keypoint (nvis == 0), e from << 1 to > 50; f32 and bf16
  pose_k5d2        K 5, D 2: no kobj term, ten raw channels in a padded row
  pose_empty_ends  images without labels at the start, in the middle and at the end: pose_entry's binary search over equal offsets
  pose_tiny        a box below stride 8, a zero-area row, exp(-e) underflowing to 0 in fp32
  pose_e2e         End2End on pose_rect's shape

Not reached, and no test is added for it: the run-time-nm instances of the two mask kernels (NMC = 0; the graph fixes nm = 32 and row pitches that are
multiples of 8, so no entry selects them); the 1024-workgroup cap of ys_loss_pose_grid (B * A > 262144); the intermediate buffers `ent` and `part`, which
no entry reads; the padded channels of the keypoint gradient rows (get_output("dkpts") returns the K * D channels only -- the launch clears the whole
row and pose_entry writes inside K * D); the truncating crop at edges at or below -1 cell (tests/mask_kpt_cases.py)."""
import time

import numpy as np
import pytest

import loss_cases as L
import mask_kpt_cases as MK
from conftest import BACKENDS
from test_loss_kernels import item_bounds

_BOTH = ("f32", "bf16")
_DTYPES = {"seg_rect": _BOTH, "seg_wide_row": ("f32",), "seg_empty_mid": ("f32",), "seg_many": ("f32",), "seg_trunc_mixed": ("f32",),
           "seg_thin_tiny": ("f32",), "seg_e2e": ("f32",), "pose_rect": _BOTH, "pose_k5d2": _BOTH, "pose_empty_ends": ("f32",), "pose_tiny": ("f32",),
           "pose_e2e": ("f32",)}


def _params():
    return [pytest.param(name, dt, id="%s-%s" % (name, dt)) for name in _DTYPES for dt in _DTYPES[name]]


def test_case_table_matches():
    assert list(_DTYPES) == list(MK.CASES) == list(MK.SEEDS)
    for name in MK.CASES:
        assert tuple(MK.get_case(name)["dtypes"]) == tuple(_DTYPES[name]), name


WORST = {}        # (key, backend) -> (figure, where): what DESIGN.md's table records; printed by every case (pytest -s) and by test_zz_report


def _note(key, fig, where):
    if fig > WORST.get(key, (-1.0, ""))[0]:
        WORST[key] = (float(fig), where)


@pytest.mark.parametrize("name", list(_DTYPES))
def test_fp32_oracle_stays_inside_the_bounds(name):
    """where the constants come from: the fp32 oracle against its float64 run, per tensor and item.  Each constant is 4x the worst figure printed here over all
    cases, rounded up to a power of two (or the floor); the assertion is that the oracle itself stays inside -- its fp32 sums depend on the thread count, so the
    4x is headroom, not something to assert"""
    c = MK.get_case(name)
    for crop in ([c["crop"], not c["crop"]] if c["task"] == "seg" and c["both_crops"] else [None]):
        for k, v in MK.oracle32(name, crop).items():
            print("MEASURE oracle32 %s crop %s %s = %.3g" % (name, crop, k, v))
            _note((k.replace("one2one_", ""), "oracle32"), v, name)
            bound = MK.ITEM_R[k] if k in MK.ITEM_R else MK.GRAD_R[k.replace("one2one_", "")]
            assert v <= bound, (name, k, v, bound)


def run_engine(engine, c, dtype):
    """the criterion on the case's predictions, twice -> everything the engine lets a caller read; then once in the other crop mode (items only)"""
    from yolosharp_amd import model as M
    seg, e2e = c["task"] == "seg", c.get("e2e", False)
    kw = {} if seg else {"kpt_num": c["K"], "kpt_dim": c["D"]}
    m = (M.Yolov8Segment if seg else M.Yolov8Pose)(engine, nc=c["nc"], reg_max=c["reg_max"], size="n", height=c["H"], width=c["W"], max_batch=c["B"],
                                                    dtype=dtype, **kw)
    try:
        assert m.A == L.anchors(c["H"], c["W"]).shape[0]
        if e2e:
            (m.e2e_init if seg else m.e2e_pose_init)(300, MK.E2E_EPOCHS)
            for _ in range(MK.E2E_UPDATES):
                m.e2e_update()
            assert m.e2e_gains() == pytest.approx(MK.gains(), abs=1e-7)
        heads = MK.HEADS[c["task"]]
        p = {k: c["preds"][k] for k in ("boxes", "scores") + heads}
        mk = (lambda crop: M.v8SegmentationLoss(m, cpu_crop_branch=crop)) if seg else (lambda crop: M.v8PoseLoss(m))
        runs = []
        crit = mk(c.get("crop", False))
        for _ in range(2):
            m.set_preds(p)
            loss, items = crit(None, c["batch"])
            gi, ts, tss = crit.read_targets()
            r = {"items": items.astype(np.float64), "loss": float(loss.sum()), "gt_idx": gi, "tss": tss}
            for k in MK.grad_keys(c):
                r[k] = m.get_output(k)
            runs.append(r)
        stored = {k: m.get_output(k) for k in ("boxes", "scores") + heads}
        other = None
        if seg and c["both_crops"]:
            m.set_preds(p)
            other = mk(not c["crop"])(None, c["batch"])[1].astype(np.float64)
    finally:
        m.close()
    return runs[0], runs[1], stored, other


def check_grad(got, ref, dtype, key, tag, backend):
    """per element: |got - ref| <= R (|ref| + max|ref| / 8) (+ one bf16 rounding of the stored value)"""
    what = tag + " " + key
    R = MK.GRAD_R[key.replace("one2one_", "")]
    assert np.isfinite(got).all(), what
    mx = np.abs(ref).max()
    err = np.abs(got.astype(np.float64) - ref)
    bound = R * (np.abs(ref) + mx / 8)
    if dtype == "f32":
        fig = MK.ratio(got.astype(np.float64), ref)
        print("MEASURE %s worst |err| / (|ref| + max|ref| / 8) = %.3g (bound %.3g)" % (what, fig, R))
        _note((key.replace("one2one_", ""), backend), fig, what)
    else:
        bound = bound + L.BF16_R * np.abs(ref)
        print("MEASURE %s bf16 worst |err| / bound = %.3g" % (what, (err / (bound + 1e-300)).max()))
    bad = np.argwhere(err > bound)
    assert bad.size == 0, (what, len(bad), bad[:4].tolist(), [(float(got[tuple(i)]), float(ref[tuple(i)])) for i in bad[:4]], float(mx))


def _bg(fg, arr):
    """the elements of a [B, C, A] gradient at background anchors"""
    return arr[np.broadcast_to(~fg[:, None, :], arr.shape)]


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("name,dtype", _params())
def test_mask_kpt_terms_stage_by_stage(name, dtype, backend, engine):
    c = MK.get_case(name)
    seg, e2e = c["task"] == "seg", c.get("e2e", False)
    B, H, W = c["B"], c["H"], c["W"]
    mh, mw = H // 4, W // 4
    ref = MK.get_reference(name, dtype)
    tag = "%s-%s-%s" % (name, dtype, backend)
    # ---- the case itself: no decision is a near-tie, no crop edge sits on an integer, the branch the case exists for is there (a seed that stopped
    # satisfying any of it FAILS)
    for r in ref["passes"]:
        print("MARGINS %s %s" % (tag, {k: "%.3g" % v for k, v in r["margins"].items()}))
        assert MK.margins_ok(r["margins"]), (name, r["margins"])
    _case_premises(name, c, ref, dtype)
    t0 = time.perf_counter()
    got, again, stored, other = run_engine(engine, c, dtype)
    print("TIME %s engine %.2f s" % (tag, time.perf_counter() - t0))
    for k in stored:                                     # the reference was fed what the engine stores
        assert np.array_equal(stored[k].astype(np.float64), L.as_stored(c["preds"][k], dtype)), "stored " + k
    # ---- 1. assignment: foreground set and slot, every anchor (End2End: of the one2one pass, the one a caller can read)
    diff = np.argwhere(got["gt_idx"] != ref["gt_idx"])
    assert diff.size == 0, ("assignment", tag, len(diff), [(i.tolist(), int(got["gt_idx"][tuple(i)]), int(ref["gt_idx"][tuple(i)])) for i in diff[:6]])
    # ---- 2. background: exactly 0
    first, last = ref["passes"][0], ref["passes"][-1]
    for key in MK.grad_keys(c):
        if key == "dproto":
            u = MK.crop_union(first, B, mh, mw, c["crop"])
            out = got["dproto"][np.broadcast_to(~u[:, None], got["dproto"].shape)]
            assert out.size > 0 and not out.any(), ("dproto outside every foreground crop", tag, int(np.count_nonzero(out)))
            continue
        ps = last if key.startswith("one2one_") else first
        assert not _bg(ps["fg"], got[key]).any(), (key + " at background anchors", tag)
        if seg:                                           # an empty crop contributes nothing (and still counts in ntot: the items and every other element)
            cb = MK.crop_bounds(ps["edges"], ps["img"], B, mh, mw, c["crop"])
            empty = (cb[:, 1] <= cb[:, 0]) | (cb[:, 3] <= cb[:, 2])
            bi, ai = np.nonzero(ps["fg"])
            assert not got[key][bi[empty], :, ai[empty]].any() and not ref[key][bi[empty], :, ai[empty]].any(), ("empty crop", tag)
    # ---- 3. gradients per element
    for key in MK.grad_keys(c):
        assert np.abs(ref[key]).max() > 0, key
        check_grad(got[key], ref[key], dtype, key, tag, backend)
    if "underflow" in ref:                                # pose_tiny: where exp(-e) is 0 in fp32 the reference gradient is below the bound
        bi, ai = np.nonzero(ref["fg"])
        n, k = np.nonzero(ref["underflow"])
        g = np.stack([ref["dkpts"][bi[n], k * c["D"] + j, ai[n]] for j in (0, 1)])
        assert (np.abs(g) < MK.GRAD_R["dkpts"] * np.abs(ref["dkpts"]).max() / 8).all()
    # ---- 4. items: the term's own against float64, box / cls / dfl with the criterion's bounds, and the loss
    want = ref["items"]
    bound = np.zeros(5)
    det = [0, 2, 3] if seg else [0, 3, 4]
    gains = ref.get("gains", (1.0,))
    for g, ps in zip(gains, ref["passes"]):
        bound[det] += g * item_bounds(c, dtype, ps["det_items"], ps["tss"])
    for k, i in MK.item_slots(c).items():
        bound[i] = MK.ITEM_R[k] * abs(want[i])
        rel = abs(got["items"][i] - want[i]) / max(abs(want[i]), 1e-300)
        print("MEASURE %s item %s relative error = %.3g (bound %.3g, item %.6g)" % (tag, k, rel, MK.ITEM_R[k], want[i]))
        if dtype == "f32":
            _note((k, backend), rel, tag)
    err = np.abs(got["items"] - want)
    assert (err <= bound).all(), ("items", tag, got["items"].tolist(), want.tolist(), bound.tolist())
    assert abs(got["loss"] - ref["loss"]) <= bound.sum() * B + 2.0 ** -22 * abs(ref["loss"]), ("loss", got["loss"], ref["loss"])
    if other is not None:                                 # the seg item in the other crop mode against the oracle's matching branch
        ro = MK.get_reference(name, dtype, crop=not c["crop"])
        assert ro["items"][1] != want[1]
        rel = abs(other[1] - ro["items"][1]) / abs(ro["items"][1])
        print("MEASURE %s item seg (cpu_crop_branch %s) relative error = %.3g" % (tag, not c["crop"], rel))
        assert rel <= MK.ITEM_R["seg"], ("seg item, other crop mode", tag, other[1], ro["items"][1])
    # ---- 5. a second run of the same case: bit-identical in every read-back array
    for k in got:
        assert np.array_equal(np.asarray(got[k]), np.asarray(again[k])), ("rerun differs", tag, k)


def _case_premises(name, c, ref, dtype):
    MK.premises(name, c, ref, dtype)


def test_zz_report():
    """the worst figure per tensor / item and backend over the cases that ran in this process (what DESIGN.md's table records); always passes"""
    for (k, where), (v, tag) in sorted(WORST.items()):
        print("WORST %-18s %-8s %.3g  (%s)" % (k, where, v, tag))
