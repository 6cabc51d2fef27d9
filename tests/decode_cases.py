"""Cases and references for tests/test_decode_kernels.py: detect_decode_kernel (csrc/elementwise.hip) on head values a test chooses, through
Model.set_preds + Model.decode_preds.

Reference: decode64, a float64 numpy restatement of Detect._inference / decode_bboxes (xywh and xyxy, Head.cs:199-223), dist2rbox with the angle
(Tal.cs:389-408, Head.cs:429), Pose.kpts_decode (Head.cs:590-605) and the Segment concatenation (Head.cs:309-313), applied to the head values as the
engine STORES them (a bf16 model rounds them once; `pred` is fp32 in both dtypes, so the reference sees what the kernel sees and no bf16 term enters
a bound).  oracle(): the same operation through oracle/yolo_oracle.py's own functions in float32 (what the bounds are measured from) or float64 (a
cross-check of decode64).

Figure per block: max |got - ref| / (|ref| + max|ref| / 8) (mask_kpt_cases.ratio), boxes and keypoint xy in grid cells (divided by the anchor's
stride, a power of two) so that stride-8 anchors are not measured against stride-32 magnitudes.

BOUNDS: 4x the worst figure of the fp32 oracle against decode64 over all cases, rounded up to a power of two.  Worst fp32-oracle figures (python
tests/decode_cases.py prints them; the CPU test test_bounds_table_is_the_measured_one re-measures):
    box 5.43e-07 -> 2^-18   prob 8.79e-08 -> 2^-21   angle 2.26e-07 -> 2^-20   kxy 5.06e-08 -> 2^-22   kvis 8.90e-08 -> 2^-21
"""
import math
import types

import numpy as np
import torch

import loss_cases as L
from mask_kpt_cases import ratio
from oracle import yolo_oracle as O

STRIDES = (8, 16, 32)
BOUNDS = {"box": 2.0 ** -18, "prob": 2.0 ** -21, "angle": 2.0 ** -20, "kxy": 2.0 ** -22, "kvis": 2.0 ** -21}
NM = 32


def pow2ceil(v):
    return 2.0 ** math.ceil(math.log2(v))


def levels(H, W):
    """(first anchor, rows, columns, stride) per level"""
    out, o = [], 0
    for s in STRIDES:
        out.append((o, H // s, W // s, s))
        o += (H // s) * (W // s)
    return out


def grid(H, W):
    """cell column, cell row, stride per anchor, float64 [A]"""
    gx, gy, st = [], [], []
    for o, h, w, s in levels(H, W):
        yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
        gx.append(xx.ravel()); gy.append(yy.ravel()); st.append(np.full(h * w, s))
    return [np.concatenate(v).astype(np.float64) for v in (gx, gy, st)]


def sig64(x):
    return 1.0 / (1.0 + np.exp(-x))          # float64: exp(90) = 1.2e39 is finite


def dfl64(boxes, R):
    B, _, A = boxes.shape
    x = boxes.reshape(B, 4, R, A)
    e = np.exp(x - x.max(2, keepdims=True))
    return (e * np.arange(R, dtype=np.float64)[None, None, :, None]).sum(2) / e.sum(2)


def extra_key(c):
    return {"detect": None, "segment": "mask_coefficient", "obb": "angle_logit", "pose": "kpts"}[c["task"]]


def stored(c, dtype, preds=None):
    """the head values after the engine has stored them, float64"""
    p = c["preds"] if preds is None else preds
    return {k: L.as_stored(v, dtype) for k, v in p.items() if k != "proto"}


def decode64(c, s):
    """blocks of `pred` in float64 from stored head values s: box [B,4,A] (pixels), prob [B,nc,A], angle [B,1,A], kxy [B,K,2,A] (pixels), kvis [B,K,A],
    coef [B,nm,A]; "dist" [B,4,A] = the DFL expectation (for premises)"""
    gx, gy, st = grid(c["H"], c["W"])
    d = dfl64(s["boxes"], c["reg_max"])
    ax, ay = gx + 0.5, gy + 0.5
    out = {"dist": d, "prob": sig64(s["scores"])}
    if c["task"] == "obb":
        ang = (sig64(s["angle_logit"][:, 0]) - 0.25) * math.pi
        xf, yf = (d[:, 2] - d[:, 0]) / 2, (d[:, 3] - d[:, 1]) / 2
        box = [xf * np.cos(ang) - yf * np.sin(ang) + ax, xf * np.sin(ang) + yf * np.cos(ang) + ay, d[:, 0] + d[:, 2], d[:, 1] + d[:, 3]]
        out["angle"] = ang[:, None]
    else:
        x1, y1, x2, y2 = ax - d[:, 0], ay - d[:, 1], ax + d[:, 2], ay + d[:, 3]
        box = [x1, y1, x2, y2] if c["e2e"] else [(x1 + x2) / 2, (y1 + y2) / 2, x2 - x1, y2 - y1]
    out["box"] = np.stack(box, 1) * st
    if c["task"] == "pose":
        K, D = c["K"], c["D"]
        k = s["kpts"].reshape(-1, K, D, gx.size)
        out["kxy"] = np.stack([(k[:, :, 0] * 2.0 + gx) * st, (k[:, :, 1] * 2.0 + gy) * st], 2)
        if D == 3:
            out["kvis"] = sig64(k[:, :, 2])
    if c["task"] == "segment":
        out["coef"] = s["mask_coefficient"]
    return out


def oracle(c, s, fd):
    """the same blocks through oracle/yolo_oracle.py's functions in dtype fd"""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(fd)
    feats = [torch.zeros(1, 1, c["H"] // q, c["W"] // q, dtype=fd) for q in STRIDES]
    with torch.no_grad():
        anc, st = O.make_anchors(feats, STRIDES, 0.5)
        anc, st = anc.transpose(0, 1), st.transpose(0, 1)
        d = O.DFL(c["reg_max"]).to(fd)(t(s["boxes"]))
        out = {"prob": t(s["scores"]).sigmoid()}
        if c["task"] == "obb":
            ang = (t(s["angle_logit"]).sigmoid() - 0.25) * math.pi
            out["box"] = O.dist2rbox(d, ang, anc.unsqueeze(0), dim=1) * st
            out["angle"] = ang
        else:
            out["box"] = O.dist2bbox(d, anc.unsqueeze(0), xywh=not c["e2e"], dim=1) * st
        if c["task"] == "pose":
            K, D = c["K"], c["D"]
            kp = O.Pose.kpts_decode(types.SimpleNamespace(keypoint_dim=D), t(s["kpts"]), anc, st).view(-1, K, D, anc.shape[1])
            out["kxy"] = kp[:, :, :2]
            if D == 3:
                out["kvis"] = kp[:, :, 2]
    return {k: v.double().numpy() for k, v in out.items()}


def split_pred(c, pred):
    """the engine's `pred` [B, 4+nc+extra, A] -> the same blocks (float64 views of the fp32 values)"""
    nc = c["nc"]
    p = np.asarray(pred, np.float64)
    out = {"box": p[:, :4], "prob": p[:, 4:4 + nc]}
    x = p[:, 4 + nc:]
    if c["task"] == "obb":
        out["angle"] = x
    elif c["task"] == "pose":
        k = x.reshape(-1, c["K"], c["D"], p.shape[2])
        out["kxy"] = k[:, :, :2]
        if c["D"] == 3:
            out["kvis"] = k[:, :, 2]
    elif c["task"] == "segment":
        out["coef"] = x
    return out


def figures(c, got, ref):
    """{block: figure} of blocks `got` against `ref` (coef, exact, is not a figure)"""
    st = grid(c["H"], c["W"])[2]
    out = {}
    for k in BOUNDS:
        if k in ref:
            q = st if k in ("box", "kxy") else 1.0
            out[k] = ratio(got[k] / q, ref[k] / q)
    return out


# ----------------------------------------------------------------------------- cases
def n_anchors(H, W):
    return sum(h * w for _, h, w, _ in levels(H, W))


def _case(task, H, W, B, nc, seed, e2e=False, K=17, D=3, **kw):
    """random head values: box logits N(0, 2), class logits N(0, 3), keypoints N(0, 2), angle logits N(0, 2), coefficients N(0, 1)"""
    rng = np.random.default_rng(seed)
    A, R = n_anchors(H, W), 16
    f = lambda sd, *shape: (rng.standard_normal(shape) * sd).astype(np.float32)
    p = {"boxes": f(2.0, B, 4 * R, A), "scores": f(3.0, B, nc, A)}
    if task == "segment":
        p["mask_coefficient"] = f(1.0, B, NM, A)
        p["proto"] = f(1.0, B, NM, H // 4, W // 4)
    elif task == "obb":
        p["angle_logit"] = f(2.0, B, 1, A)
    elif task == "pose":
        p["kpts"] = f(2.0, B, K * D, A)
    c = {"task": task, "H": H, "W": W, "B": B, "nc": nc, "reg_max": R, "e2e": e2e, "K": K, "D": D, "A": A, "preds": p, "partial": False}
    c.update(kw)
    return c


def _rows(c):
    """the box logits as [B, 4, R, A] (a view into the case)"""
    return c["preds"]["boxes"].reshape(c["B"], 4, c["reg_max"], c["A"])


def case_dfl_onehot(seed):
    c = _case("detect", 64, 96, 3, 5, seed)
    r = _rows(c)
    r[:] = -30.0
    b, s, a = np.meshgrid(np.arange(3), np.arange(4), np.arange(c["A"]), indexing="ij")
    c["bins"] = np.array([0, 15, 7])[(b + s + a) % 3]
    np.put_along_axis(r, c["bins"][:, :, None, :], 30.0, 2)
    return c


def case_dfl_flat(seed):
    c = _case("detect", 64, 96, 3, 5, seed)
    r = _rows(c)
    r[:] = np.array([0.0, 3.5, -7.0, 30.0], np.float32)[np.arange(c["A"]) % 4][None, None, None, :]      # every value exact in bf16
    return c


def case_dfl_underflow(seed):
    """one bin at 0, one at -5, the rest between -110 and -200: exp of them is below the smallest fp32 denormal"""
    c = _case("detect", 64, 96, 3, 5, seed)
    rng = np.random.default_rng(seed + 1)
    r = _rows(c)
    r[:] = -(110.0 + 90.0 * rng.random(r.shape)).astype(np.float32)
    i = rng.integers(0, 16, (3, 4, 1, c["A"]))
    j = (i + rng.integers(1, 16, i.shape)) % 16
    np.put_along_axis(r, i, 0.0, 2)
    np.put_along_axis(r, j, -5.0, 2)
    return c


def case_dfl_tie(seed):
    """two equal maxima, everything else 20 to 30 below"""
    c = _case("detect", 64, 96, 3, 5, seed)
    rng = np.random.default_rng(seed + 1)
    r = _rows(c)
    r[:] = -(20.0 + 10.0 * rng.random(r.shape)).astype(np.float32)
    i = rng.integers(0, 16, (3, 4, 1, c["A"]))
    j = (i + rng.integers(1, 16, i.shape)) % 16
    np.put_along_axis(r, i, 1.5, 2)
    np.put_along_axis(r, j, 1.5, 2)
    c["tie"] = (i[:, :, 0] + j[:, :, 0]) / 2.0
    return c


SAT = np.array([-90.0, -20.0, 0.0, 20.0, 90.0], np.float32)


def _saturate(a):
    """logits from SAT, the position moving with class and anchor so that every value meets every lane"""
    B, C, A = a.shape
    b, ch, an = np.meshgrid(np.arange(B), np.arange(C), np.arange(A), indexing="ij")
    a[:] = SAT[(b + ch + an) % 5]


def case_sat_detect(seed):
    c = _case("detect", 64, 96, 3, 7, seed)
    _saturate(c["preds"]["scores"])
    return c


def case_sat_obb(seed):
    c = _case("obb", 64, 96, 3, 7, seed)
    _saturate(c["preds"]["scores"])
    _saturate(c["preds"]["angle_logit"])
    return c


def case_sat_pose(seed):
    c = _case("pose", 64, 96, 3, 3, seed)
    k = c["preds"]["kpts"].reshape(3, 17, 3, c["A"])
    v = np.empty((3, 17, c["A"]), np.float32)
    _saturate(v)
    k[:, :, 2] = v
    return c


CASES = {
    # shapes: 64x96 (levels 8x12, 4x6, 2x3: A = 126; with B = 3 a 64-row workgroup straddles level boundaries and image boundaries and the last one is
    # ragged), 96x64 (level widths swapped), 32x32 (A = 21: three images in one workgroup); each with a batch < max_batch call after the full one
    "det_nc5_64x96": lambda s: _case("detect", 64, 96, 3, 5, s, partial=True),
    "det_nc5_96x64": lambda s: _case("detect", 96, 64, 3, 5, s, partial=True),
    "det_nc5_32x32": lambda s: _case("detect", 32, 32, 3, 5, s, partial=True),
    # class counts: one class, not a multiple of 4 or 8, one that fills the 16-byte units
    "det_nc1": lambda s: _case("detect", 64, 96, 3, 1, s),
    "det_nc7": lambda s: _case("detect", 64, 96, 3, 7, s),
    "det_nc80": lambda s: _case("detect", 64, 96, 3, 80, s),
    "det_e2e_nc7": lambda s: _case("detect", 64, 96, 3, 7, s, e2e=True),
    "seg_nc5": lambda s: _case("segment", 64, 96, 3, 5, s),
    "seg_e2e_nc5": lambda s: _case("segment", 64, 96, 2, 5, s, e2e=True),
    "obb_nc7": lambda s: _case("obb", 64, 96, 3, 7, s),
    "obb_e2e_nc7": lambda s: _case("obb", 96, 64, 2, 7, s, e2e=True),
    "pose_nc3_k17d3": lambda s: _case("pose", 64, 96, 3, 3, s),
    "pose_nc1_k5d2": lambda s: _case("pose", 96, 64, 3, 1, s, K=5, D=2),
    "pose_e2e_nc3": lambda s: _case("pose", 64, 96, 2, 3, s, e2e=True),
    # values
    "dfl_onehot": case_dfl_onehot, "dfl_flat": case_dfl_flat, "dfl_underflow": case_dfl_underflow, "dfl_tie": case_dfl_tie,
    "sat_detect": case_sat_detect, "sat_obb": case_sat_obb, "sat_pose": case_sat_pose,
}
SEEDS = {name: 1000 + 10 * i for i, name in enumerate(CASES)}

_cache = {}


def get_case(name):
    if name not in _cache:
        _cache[name] = CASES[name](SEEDS[name])
    return _cache[name]


def get_reference(name, dtype):
    """decode64 of the case as a model of `dtype` stores it; computed once and shared, callers must not write into it"""
    key = (name, dtype)
    if key not in _cache:
        c = get_case(name)
        _cache[key] = decode64(c, stored(c, dtype))
    return _cache[key]


def second_preds(c):
    """other values for the first B - 1 images: the batch < max_batch call"""
    o = _case(c["task"], c["H"], c["W"], c["B"] - 1, c["nc"], 77, e2e=c["e2e"], K=c["K"], D=c["D"])
    return o


def oracle32(name):
    """{block: figure} of the fp32 oracle against decode64 on the case's f32 values; the float64 oracle must agree with decode64 to rounding"""
    c = get_case(name)
    s = stored(c, "f32")
    ref = get_reference(name, "f32")
    for k, v in figures(c, oracle(c, s, torch.float64), ref).items():
        assert v < 1e-13, ("the float64 oracle and decode64 disagree", name, k, v)
    return figures(c, oracle(c, s, torch.float32), ref)


def premises(name, c, ref):
    """what the case exists for, asserted on the reference"""
    gx, gy, st = grid(c["H"], c["W"])
    d = ref["dist"]
    if name == "dfl_onehot":
        assert {0, 7, 15} == set(np.unique(c["bins"]).tolist())
        assert np.abs(d - c["bins"]).max() < 1e-12
    if name == "dfl_flat":
        assert (d == 7.5).all()
    if name == "dfl_underflow":
        r = _rows(c).astype(np.float64)
        assert ((np.sort(r, 2)[:, :, :14] - r.max(2, keepdims=True)) < -104.0).all()        # exp underflows to 0 even as an fp32 denormal
        assert np.ptp(d) > 10
    if name == "dfl_tie":
        r = _rows(c)
        assert ((r == r.max(2, keepdims=True)).sum(2) == 2).all() and np.abs(d - c["tie"]).max() < 1e-7
    if name.startswith("sat_"):
        z, p = c["preds"]["scores"], ref["prob"]
        if name == "sat_pose":                                     # the visibility logits
            z, p = c["preds"]["kpts"].reshape(c["B"], c["K"], c["D"], c["A"])[:, :, 2], ref["kvis"]
        for v in SAT:
            assert (z == v).any()
        assert (p[z == 0] == 0.5).all()
    if name == "sat_obb":
        z = c["preds"]["angle_logit"]
        assert np.abs(ref["angle"][z == 90] - 0.75 * math.pi).max() < 1e-15 and np.abs(ref["angle"][z == -90] + 0.25 * math.pi).max() < 1e-15
    if c["task"] == "pose":
        k = c["preds"]["kpts"].reshape(c["B"], c["K"], c["D"], c["A"])
        for o, h, w, s in levels(c["H"], c["W"]):
            a = o + w + 1                                          # second row, second column of the level: gx and gy are both nonzero
            assert gx[a] == 1 and gy[a] == 1 and st[a] == s
            assert (k[:, :, :2, a] > 0).any() and (k[:, :, :2, a] < 0).any()
    for o, h, w, s in levels(c["H"], c["W"]):
        assert h >= 1 and w >= 1


if __name__ == "__main__":
    worst = {}
    for name in CASES:
        for k, v in oracle32(name).items():
            print("oracle32 %-16s %-6s %.3g" % (name, k, v))
            worst[k] = max(worst.get(k, 0.0), v)
    for k, v in worst.items():
        print("WORST %-6s %.3g -> bound %s (table %s)" % (k, v, pow2ceil(4 * v), BOUNDS[k]))
