"""csrc/attn_dw.hip kernel by kernel against float64: the attention core (scalar and MFMA kernels, forward and the two backward passes) and the
depthwise 3x3 convolution (forward, input gradient, weight gradient), through the stateless entry points ys_attn_fwd / ys_attn_bwd /
ys_dwconv3x3_fwd / ys_dwconv3x3_bwd -- no qkv / proj / ffn convolution, BatchNorm or residual between the kernel and the comparison.

References: the formulas in torch float64 on the operands the kernel actually sees (rounded to the storage type first).
Bounds, none of them a free constant (d32 = max |float32 evaluation - float64 evaluation| of the same formula on the same inputs, per compared tensor,
measured from the references at run time):
  fp32 results (f32 outputs, P, depthwise dw)   |y - ref| <= 8 d32         (+ 2^-22 |s - rowmax| P_ref for P: the hardware exponential's argument error)
  bf16 results                                  |y - ref| <= 2^-8 |ref| + 8 d32
       MFMA kernels only                        ... + 2^-9 (|A_ref| @ |B|): the second product's A operand (P, dS) enters rounded to bf16
  P rows sum to 1 within N 2^-23; two consecutive calls are bit-identical; the sentinel around every padded view survives.
test_*_bounds_hold_for_an_emulation_of_the_rounding_points check the bounds themselves on the CPU, without the engine; the inputs of an attention case are redrawn
(up to SEED_TRIES times) until that emulation stays inside -- never the bound widened.

The nearly one-hot regime comes in two forms.  "peaked" (q ~ 6 N(0, 1) against random keys: the largest probability of a row is 0.5 .. 0.9) runs on the scalar
bf16 and the fp32 kernels.  On the MFMA route the emulation alone does not stay inside the bounds with such inputs, on any draw: 2^-9 is half of bf16's unit roundoff
(a value at the bottom of its binade rounds by up to 2^-8 of itself), so where one probability of 0.5 .. 0.9 dominates a row, the operand term plus the store term allow
1.5 x 2^-8 |P v| and correct rounding can cost 2 x 2^-8 |P v| (measured, emulation: 0.1 - 0.3 % of the elements out, worst 1.58 x, dv at N = 100).  Such a case gets
other inputs, not a wider bound: "onehot" (q = 6 x one of the keys: every row has ONE probability within 1e-4 of 1, which bf16 holds exactly enough, and
dS = P (dP - t) is pure cancellation) runs on all three routes, the MFMA kernels included.

Worst error / bound per kernel path, interpreter build:
  attention MFMA bf16      ao 0.990  P 0.152  dq 0.972  dk 0.937  dv 0.980        depthwise bf16   y 0.994  dx 0.995  dx(accumulate) 0.995  dw 0.197
  attention scalar bf16    ao 0.993  P 0.171  dq 0.991  dk 0.994  dv 0.995        depthwise fp32   y 0.304  dx 0.210  dx(accumulate) 0.194  dw 0.319
  attention scalar fp32    ao 0.146  P 0.197  dq 0.212  dk 0.241  dv 0.159
(bf16 ratios near 1 are the store rounding itself: half an ulp at the bottom of a binade is 2^-8 |ref|.)  The MI355X column of this table has not been measured yet
(the GPU cases print their ratios with pytest -s).
"""
import itertools
import os
import tempfile

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import BACKENDS

U8, U9, U22, U23 = 2.0 ** -8, 2.0 ** -9, 2.0 ** -22, 2.0 ** -23
YS_ERR_UNSUPPORTED = 4


def bf16r(a):
    """float32 array rounded to the nearest bf16 (ties to even), as float32."""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32).reshape(np.shape(a))


def store(a, dtype):
    return bf16r(a) if dtype == "bf16" else np.ascontiguousarray(a, np.float32)


# ------------------------------------------------------------------ attention: reference, bounds, emulation
def attn_formula(qkv, dao, dv_in, B, N, heads, kd, hd, dt, flip=False, round_a=None):
    """softmax(q^T k kd^-0.5), v P^T and their analytic gradients in torch dtype `dt`.  flip: walk every reduction in the opposite order (a second fp32
    summation order); round_a: applied to P / dS before the SECOND products (the MFMA kernels feed them as bf16)."""
    hs = 2 * kd + hd
    x = torch.from_numpy(qkv).to(dt).view(B, heads, hs, N)
    if flip:
        x = x.flip(2)                                             # d reversed: q . k and dO . v summed backwards
        q, k, v = x[:, :, hd + kd:], x[:, :, hd:hd + kd], x[:, :, :hd]
    else:
        q, k, v = x[:, :, :kd], x[:, :, kd:2 * kd], x[:, :, 2 * kd:]
    scale = torch.tensor(1.0 / np.sqrt(np.float32(kd)) if dt == torch.float32 else kd ** -0.5, dtype=dt)
    dO = torch.from_numpy(dao).to(dt).view(B, heads, hd, N)
    dvi = torch.from_numpy(dv_in).to(dt).view(B, heads, hd, N)
    if flip:
        dO, dvi = dO.flip(2), dvi.flip(2)
    s = (q.transpose(-2, -1) @ k) * scale                         # [n, m]
    mx = s.max(-1, keepdim=True).values
    e = torch.exp(s - mx)
    P = e / e.sum(-1, keepdim=True)
    ra = round_a if round_a is not None else (lambda t: t)
    Pa = ra(P)
    if flip:                                                      # key index reversed in the second products
        ao = v.flip(-1) @ Pa.flip(-1).transpose(-2, -1)
    else:
        ao = v @ Pa.transpose(-2, -1)                             # [d, n]
    dP = dO.transpose(-2, -1) @ v                                 # [n, m]
    t = (dP * P).sum(-1, keepdim=True)
    dS = P * (dP - t)
    dSa = ra(dS)
    if flip:
        dq = (k.flip(-1) @ dSa.flip(-1).transpose(-2, -1)) * scale
        dk = (q.flip(-1) @ dSa.flip(-2)) * scale
        dv = dvi + dO.flip(-1) @ Pa.flip(-2)
        ao, dq, dk, dv = ao.flip(2), dq.flip(2), dk.flip(2), dv.flip(2)
    else:
        dq = (k @ dSa.transpose(-2, -1)) * scale                  # [d, n]
        dk = (q @ dSa) * scale                                    # [d, m]
        dv = dvi + dO @ Pa
    out = dict(ao=ao, P=P, dq=dq, dk=dk, dv=dv, s=s, mx=mx, dS=dS)
    return {k_: v_.contiguous().numpy() for k_, v_ in out.items()}


def attn_bounds(qkv, dao, B, N, heads, kd, hd, dtype, mfma, r64, r32):
    """Per-element bounds of ao, P, dq, dk, dv (module docstring)."""
    hs = 2 * kd + hd
    d32 = {k_: float(np.abs(r32[k_].astype(np.float64) - r64[k_]).max()) for k_ in ("ao", "P", "dq", "dk", "dv")}
    bnd = {"P": 8 * d32["P"] + U22 * np.abs(r64["s"] - r64["mx"]) * r64["P"]}
    for k_ in ("ao", "dq", "dk", "dv"):
        bnd[k_] = 8 * d32[k_] + (U8 * np.abs(r64[k_]) if dtype == "bf16" else 0.0)
    if mfma:
        x = np.abs(qkv.astype(np.float64)).reshape(B, heads, hs, N)
        q, k, v = x[:, :, :kd], x[:, :, kd:2 * kd], x[:, :, 2 * kd:]
        dO = np.abs(dao.astype(np.float64)).reshape(B, heads, hd, N)
        P, dS, sc = np.abs(r64["P"]), np.abs(r64["dS"]), kd ** -0.5
        bnd["ao"] = bnd["ao"] + U9 * (v @ P.transpose(0, 1, 3, 2))
        bnd["dq"] = bnd["dq"] + U9 * sc * (k @ dS.transpose(0, 1, 3, 2))
        bnd["dk"] = bnd["dk"] + U9 * sc * (q @ dS)
        bnd["dv"] = bnd["dv"] + U9 * (dO @ P)
    return bnd, d32


def attn_inputs(B, N, heads, kd, hd, dtype, regime, seed):
    """qkv [B, heads*(2kd+hd), N], dao / dv_in [B, heads*hd, N], rounded to the storage type.  Regimes: "normal" q, k ~ N(0, 1); "peaked" q x 6 (one probability
    of 0.5 .. 0.9 per row); "onehot" q = 6 x a key (one probability ~ 1 per row: dS is pure cancellation); "offset" one extra-large common component in q and k: every score of a row sits near +60 (exp overflows without the row maximum)."""
    rng = np.random.default_rng(seed)
    hs = 2 * kd + hd
    x = rng.standard_normal((B, heads, hs, N)).astype(np.float32)
    if regime == "peaked":
        x[:, :, :kd] *= 6.0
    elif regime == "onehot":                                       # query n = 6 x key pi(n)
        pi = rng.integers(0, N, size=(B, heads, 1, N))
        x[:, :, :kd] = 6.0 * np.take_along_axis(x[:, :, kd:2 * kd], pi, axis=3)
    elif regime == "offset":
        a = np.float32(np.sqrt(60.0 * np.sqrt(kd)))
        x[:, :, 0] = a
        x[:, :, kd] = a
    qkv = store(x.reshape(B, heads * hs, N), dtype)
    dao = store(rng.standard_normal((B, heads * hd, N)).astype(np.float32), dtype)
    dv_in = store(rng.standard_normal((B, heads * hd, N)).astype(np.float32), dtype)
    return qkv, dao, dv_in


def attn_emulate(qkv, dao, dv_in, B, N, heads, kd, hd, dtype, mfma):
    """The kernels' rounding points without the engine: stored operands, fp32 arithmetic in another summation order than the reference's, P / dS rounded to bf16 in
    front of the second product (MFMA), one store rounding."""
    ra = (lambda t: torch.from_numpy(bf16r(t.contiguous().numpy()))) if mfma else None
    r = attn_formula(qkv, dao, dv_in, B, N, heads, kd, hd, torch.float32, flip=True, round_a=ra)
    return {k_: (store(r[k_], dtype) if k_ != "P" else r[k_]) for k_ in ("ao", "P", "dq", "dk", "dv")}


def split_dqkv(dqkv, B, N, heads, kd, hd):
    x = dqkv.reshape(B, heads, 2 * kd + hd, N)
    return x[:, :, :kd], x[:, :, kd:2 * kd], x[:, :, 2 * kd:]


RATIOS = {}        # worst error / bound per path, printed at the end of a run (pytest -s) -- the figures quoted in DESIGN.md


def _note(path, ratio):
    RATIOS[path] = max(RATIOS.get(path, 0.0), float(ratio))
    print("error/bound %-28s %.3f" % (path, ratio))


def check_bound(y, ref, bnd, what, path=None):
    err = np.abs(np.asarray(y, np.float64) - ref)
    assert np.isfinite(np.asarray(y)).all(), what
    bnd = np.broadcast_to(bnd, err.shape)
    pos = bnd > 0
    ratio = float((err[pos] / bnd[pos]).max()) if pos.any() else 0.0
    if path:
        _note(path, ratio)
    bad = err > bnd
    assert not bad.any(), "%s: %d of %d elements out of bound, worst %.3f x (|err| %.3g)" % (what, int(bad.sum()), bad.size, ratio, float(err.max()))
    return ratio


def attn_check_all(got, r64, bnd, B, N, heads, what, path=None):
    """All five tensors are measured before anything is asserted: a failure names every tensor that is out."""
    out = []
    for k_ in ("ao", "P", "dq", "dk", "dv"):
        try:
            check_bound(got[k_].reshape(r64[k_].shape), r64[k_], bnd[k_], "%s %s" % (what, k_), path and path + " " + k_)
        except AssertionError as e:
            out.append(str(e).splitlines()[0])
    assert not out, "; ".join(out)
    rs = got["P"].astype(np.float64).reshape(B * heads, N, N).sum(-1)
    assert np.abs(rs - 1.0).max() <= N * U23, (what, "P row sums", float(np.abs(rs - 1.0).max()))


def A(dtype, B, heads, N, kd=32, hd=64, regime="normal", pad=(0, 0), mfma=1):
    return dict(dtype=dtype, B=B, heads=heads, N=N, kd=kd, hd=hd, regime=regime, pad=pad, mfma=mfma)


def attn_routes_mfma(c):
    return c["dtype"] == "bf16" and c["kd"] == 32 and c["hd"] == 64 and c["mfma"] == 1 and c["N"] <= 416 and c["pad"][0] % 8 == 0 and c["pad"][1] % 8 == 0


MFMA_N = [1, 15, 16, 17, 31, 32, 33, 48, 63, 64, 65, 80, 100]
BH = [(1, 1), (2, 2), (1, 3), (2, 1), (1, 2), (2, 3)]
ATTN_CASES = []
for i, n in enumerate(MFMA_N):                                     # 16-key tile edge, 32-key K-step edge (np32 > np16), 64-query workgroup edge, first wave exiting early
    b, h = BH[i % len(BH)]
    ATTN_CASES.append(A("bf16", b, h, n))                          # MFMA kernels
    ATTN_CASES.append(A("bf16", b, h, n, mfma=0))                  # the scalar bf16 kernels on the same problem, against float64 (not against the MFMA form)
ATTN_CASES += [A("f32", *BH[i % len(BH)], n) for i, n in enumerate([1, 17, 33, 64, 65, 100])]
for kd_, hd_ in [(16, 32), (64, 128), (128, 256)]:                 # scalar kernels: other head sizes; (64, 128) = second attn_bwd_kv_dispatch instantiation, (128, 256) = the limit
    ATTN_CASES += [A("bf16", 1, 2, 33, kd_, hd_), A("f32", 2, 1, 70, kd_, hd_)]
for n in (33, 100):
    for regime in ("onehot", "offset"):
        ATTN_CASES += [A("bf16", 2, 2, n, regime=regime), A("bf16", 1, 2, n, regime=regime, mfma=0), A("f32", 1, 1, n, regime=regime)]
    ATTN_CASES += [A("bf16", 1, 2, n, regime="peaked", mfma=0), A("f32", 1, 1, n, regime="peaked")]      # (module docstring: not on the MFMA route)
ATTN_CASES += [A("bf16", 2, 2, 33, pad=(8, 16)), A("bf16", 1, 3, 80, pad=(24, 8)),              # padded ldq / ldo, still on the MFMA route
               A("bf16", 2, 2, 33, pad=(8, 16), mfma=0), A("f32", 1, 2, 33, pad=(4, 12)),
               A("bf16", 1, 2, 33, pad=(4, 0)), A("bf16", 2, 1, 65, pad=(8, 4))]              # padding off the 16-byte grid: must route to the scalar kernels
ATTN_CASES += [A("bf16", 1, 1, 400), A("bf16", 1, 1, 416), A("bf16", 1, 1, 417)]               # the production token count, the MFMA limit, the first scalar N by routing
ATTN_GPU_CASES = [A("bf16", 16, 2, 400), A("bf16", 16, 4, 400), A("bf16", 16, 6, 400), A("bf16", 2, 2, 1600), A("f32", 2, 2, 400)]


def case_id(c):
    return "%s-B%d-h%d-N%d-kd%d-hd%d-%s-pad%d.%d-%s" % (c["dtype"], c["B"], c["heads"], c["N"], c["kd"], c["hd"], c["regime"], c["pad"][0], c["pad"][1],
                                                      "mfma" if attn_routes_mfma(c) else "scalar")


def _vp(a):
    import ctypes as C
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def engine_attn(engine, c, qkv, dao, dv_in):
    """ys_attn_fwd + ys_attn_bwd under the kernel profile -> results, sentinel flags and the route each launch took."""
    import ctypes as C
    from yolosharp_amd import _lib
    B, N, heads, kd, hd = c["B"], c["N"], c["heads"], c["kd"], c["hd"]
    dt = 1 if c["dtype"] == "bf16" else 0
    ao = np.empty((B, heads * hd, N), np.float32)
    P = np.empty((B * heads, N, N), np.float32)
    dqkv = np.empty((B, heads * (2 * kd + hd), N), np.float32)
    ok1, ok2 = C.c_int32(-1), C.c_int32(-1)
    engine.kernel_profile(True)
    with engine.options(ATTN_MFMA=c["mfma"]):
        _lib.check(engine.lib, engine.lib.ys_attn_fwd(engine.ctx, dt, _vp(qkv), B, N, heads, kd, hd, c["pad"][0], c["pad"][1], _vp(ao), _vp(P), C.byref(ok1)))
        _lib.check(engine.lib, engine.lib.ys_attn_bwd(engine.ctx, dt, _vp(qkv), B, N, heads, kd, hd, c["pad"][0], c["pad"][1], _vp(dao), _vp(dv_in), _vp(dqkv),
                                                     C.byref(ok2)))
    routes = profile_labels(engine)
    engine.kernel_profile(False)
    dq, dk, dv = split_dqkv(dqkv, B, N, heads, kd, hd)
    return dict(ao=ao, P=P, dq=dq, dk=dk, dv=dv, dqkv=dqkv), (ok1.value, ok2.value), routes


def profile_labels(engine):
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "launches.csv")
        engine.kernel_profile_dump(path)
        return [tuple(l.split(",")[:2]) for l in open(path).read().splitlines()[1:]]


def attn_within(got, r64, bnd):
    """Elements out of bound and the worst error / bound over ao, P, dq, dk, dv."""
    nbad, worst = 0, 0.0
    for k_ in ("ao", "P", "dq", "dk", "dv"):
        err = np.abs(np.asarray(got[k_], np.float64).reshape(r64[k_].shape) - r64[k_])
        b = np.broadcast_to(bnd[k_], err.shape)
        nbad += int((err > b).sum())
        worst = max(worst, float((err[b > 0] / b[b > 0]).max()) if (b > 0).any() else 0.0)
    return nbad, worst


SEED_TRIES = 8
_prepared = {}


def prepare_attn(c):
    """Inputs, float64 reference and bounds of a case.  "Check the bound without the engine first": the inputs are the first of SEED_TRIES draws on which the
    emulation of the rounding points stays inside the bounds with zero elements out -- a draw on which a correctly rounding implementation does not stay inside is
    replaced by other inputs, never by a wider bound.  When no draw qualifies the first one is kept and the case fails (emu_bad > 0)."""
    B, N, heads, kd, hd = c["B"], c["N"], c["heads"], c["kd"], c["hd"]
    mfma = attn_routes_mfma(c)
    key = (c["dtype"], B, heads, N, kd, hd, c["regime"], mfma)
    if key in _prepared:
        return _prepared[key]
    first = None
    for t in range(SEED_TRIES):
        qkv, dao, dv_in = attn_inputs(B, N, heads, kd, hd, c["dtype"], c["regime"], seed=N * 7 + heads + 1000 * t)
        r64 = attn_formula(qkv, dao, dv_in, B, N, heads, kd, hd, torch.float64)
        r32 = attn_formula(qkv, dao, dv_in, B, N, heads, kd, hd, torch.float32)
        bnd, _ = attn_bounds(qkv, dao, B, N, heads, kd, hd, c["dtype"], mfma, r64, r32)
        emu = attn_emulate(qkv, dao, dv_in, B, N, heads, kd, hd, c["dtype"], mfma)
        nbad, worst = attn_within(emu, r64, bnd)
        rs = emu["P"].astype(np.float64).sum(-1)
        nbad += int((np.abs(rs - 1.0) > N * U23).sum())
        prep = dict(qkv=qkv, dao=dao, dv_in=dv_in, r64=r64, bnd=bnd, mfma=mfma, emu_bad=nbad, emu_worst=worst, draw=t)
        first = first or prep
        if nbad == 0:
            break
    else:
        prep = first
    if len(_prepared) >= 2:
        _prepared.clear()                                          # (the N = 1600 matrices are large)
    _prepared[key] = prep
    return prep


def poison_lds(engine, backend, c):
    """The MFMA kernels keep K / V^T / P tiles in dynamic LDS, which nothing clears between launches; what a tile's padding columns (np16 .. np32 - 1) hold
    before the kernel zero-fills them is whatever the previous kernel left there.  So that "whatever" is not benign by luck, an attention call on all-NaN
    operands runs first: more tokens than the case (another tile layout, no padding columns of its own below the case's), enough workgroups to visit every
    compute unit's LDS (every worker thread's of the interpreter).  Stale columns then reach the second product as NaN x 0."""
    n = min(416, ((c["N"] + 31) // 32) * 32 + 32)
    b, h = (16, 16) if backend == "gpu" else (2, 3)
    nan = lambda *s_: np.full(s_, np.nan, np.float32)
    engine_attn(engine, A("bf16", b, h, n), nan(b, h * 128, n), nan(b, h * 64, n), nan(b, h * 64, n))


def run_attn_case(engine, backend, c):
    B, N, heads = c["B"], c["N"], c["heads"]
    p = prepare_attn(c)
    qkv, dao, dv_in, r64, bnd, mfma = p["qkv"], p["dao"], p["dv_in"], p["r64"], p["bnd"], p["mfma"]
    if mfma:
        poison_lds(engine, backend, c)
    got, intact, routes = engine_attn(engine, c, qkv, dao, dv_in)
    want = "mfma" if mfma else "scalar"
    assert sorted(routes) == sorted([("attn_fwd", want), ("attn_fwd", want), ("attn_bwd", want)]), (routes, want)     # (ys_attn_bwd runs the forward itself)
    assert intact == (1, 1), ("a kernel wrote outside its view", intact)
    again, intact2, _ = engine_attn(engine, c, qkv, dao, dv_in)
    for k_ in ("ao", "P", "dqkv"):
        assert np.array_equal(got[k_], again[k_]), "%s differs between two consecutive calls" % k_
    path = "%s attn %s %s" % (backend, c["dtype"], want)
    attn_check_all(got, r64, bnd, B, N, heads, case_id(c), path)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("case", ATTN_CASES, ids=case_id)
def test_attention_kernels_against_float64(backend, engine, case):
    run_attn_case(engine, backend, case)


@pytest.mark.gpu
@pytest.mark.parametrize("backend", ["gpu"])
@pytest.mark.parametrize("case", ATTN_GPU_CASES, ids=case_id)
def test_attention_production_shapes(backend, engine, case):
    """N = 400 with 2 / 4 / 6 heads at B = 16 (every C2PSA of the YOLOv11 graphs at 640 x 640), N = 1600 on the scalar bf16 kernels (a 1280 x 1280 graph)."""
    run_attn_case(engine, backend, case)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("geom", [(33, 136, 64), (33, 32, 264), (1601, 32, 64)])
def test_attention_rejects_unsupported_geometry(backend, engine, geom):
    """kd > 128, hd > 256, N > 1600: YS_ERR_UNSUPPORTED from forward AND backward (ys_attn_bwd_launch had no range check), and no kernel is started."""
    import ctypes as C
    from yolosharp_amd import _lib
    N, kd, hd = geom
    qkv = np.zeros((1, 2 * kd + hd, N), np.float32)
    dao = np.zeros((1, hd, N), np.float32)
    ao = np.zeros((1, hd, N), np.float32)
    dqkv = np.zeros_like(qkv)
    engine.kernel_profile(True)
    for dt in (0, 1):
        assert engine.lib.ys_attn_fwd(engine.ctx, dt, _vp(qkv), 1, N, 1, kd, hd, 0, 0, _vp(ao), None, None) == YS_ERR_UNSUPPORTED
        assert b"outside the supported range" in engine.lib.ys_last_error()
        assert engine.lib.ys_attn_bwd(engine.ctx, dt, _vp(qkv), 1, N, 1, kd, hd, 0, 0, _vp(dao), None, _vp(dqkv), None) == YS_ERR_UNSUPPORTED
    labels = profile_labels(engine)
    engine.kernel_profile(False)
    assert labels == [], labels


# ------------------------------------------------------------------ depthwise 3x3
def dw_formula(x, w, dy, dx_in, dt):
    """F.conv2d(groups = C) and its autograd in torch dtype `dt`; dx = dx_in + the input gradient."""
    xt = torch.from_numpy(x).to(dt).requires_grad_(True)
    wt = torch.from_numpy(w).to(dt).requires_grad_(True)
    y = F.conv2d(xt, wt, None, stride=1, padding=1, groups=x.shape[1])
    y.backward(torch.from_numpy(dy).to(dt))
    return dict(y=y.detach().numpy(), dx0=xt.grad.numpy(), dx1=(torch.from_numpy(dx_in).to(dt) + xt.grad).numpy(), dw=wt.grad.numpy())


def dw_bounds(dtype, r64, r32):
    d32 = {k_: float(np.abs(r32[k_].astype(np.float64) - r64[k_]).max()) for k_ in r64}
    bnd = {k_: 8 * d32[k_] + (U8 * np.abs(r64[k_]) if dtype == "bf16" and k_ != "dw" else 0.0) for k_ in r64}     # dw stays fp32 in both modes
    return bnd, d32


def dw_inputs(B, C, H, W, dtype, seed):
    rng = np.random.default_rng(seed)
    x = store(rng.standard_normal((B, C, H, W)).astype(np.float32), dtype)
    w = (rng.standard_normal((C, 1, 3, 3)) * 0.3).astype(np.float32)       # fp32 master weights in both modes (the kernels read them as fp32)
    dy = store(rng.standard_normal((B, C, H, W)).astype(np.float32), dtype)
    dx_in = store(rng.standard_normal((B, C, H, W)).astype(np.float32), dtype)
    return x, w, dy, dx_in


def dw_emulate(x, w, dy, dx_in, dtype):
    """The kernels' arithmetic without the engine: fp32 tap by tap in the kernels' order (kh, kw), fp32 row sums for dw, one store rounding."""
    B, C, H, W = x.shape
    xp = np.zeros((B, C, H + 2, W + 2), np.float32); xp[:, :, 1:-1, 1:-1] = x
    gp = np.zeros((B, C, H + 2, W + 2), np.float32); gp[:, :, 1:-1, 1:-1] = dy
    y = np.zeros_like(x); dx = np.zeros_like(x); dw = np.zeros_like(w)
    for kh in range(3):
        for kw in range(3):
            wt = w[None, :, 0, kh, kw, None, None]
            y = (y + xp[:, :, kh:kh + H, kw:kw + W] * wt).astype(np.float32)
            dx = (dx + gp[:, :, 2 - kh:2 - kh + H, 2 - kw:2 - kw + W] * wt).astype(np.float32)
            dw[:, 0, kh, kw] = (dy * xp[:, :, kh:kh + H, kw:kw + W]).transpose(1, 0, 2, 3).reshape(C, -1).sum(1, dtype=np.float32)
    return dict(y=store(y, dtype), dx0=store(dx, dtype), dx1=store((dx_in + dx).astype(np.float32), dtype), dw=dw)


def D(dtype, B, C, H, W, padded):
    return dict(dtype=dtype, B=B, C=C, H=H, W=W, padded=padded)


DW_W, DW_H, DW_C, DW_B = [1, 3, 4, 5, 7, 8, 13], [1, 2, 9], [8, 16, 80, 96, 128, 384], [1, 3]
DW_CASES = []
for i, (w_, h_) in enumerate(itertools.product(DW_W, DW_H)):      # every (W, H) twice, with channel counts and batch sizes rotating: every C meets 7 maps per dtype
    for j in (0, 1):
        c_, b_ = DW_C[(i + 3 * j) % 6], DW_B[(i + j) % 2]
        DW_CASES += [D("bf16", b_, c_, h_, w_, (i + j) % 2 == 0), D("f32", b_, c_, h_, w_, (i + j) % 2 == 1)]
# the weight-gradient split: several workgroups (bf16 C = 128: 16 rows x 8 per workgroup; fp32 C = 384: RP = 2), fewer rows than one workgroup's RP (1 row, RP = 128 / 64)
DW_CASES += [D("bf16", 3, 128, 9, 13, True), D("f32", 3, 384, 9, 13, False), D("bf16", 1, 16, 1, 1, True), D("f32", 1, 16, 1, 1, True), D("bf16", 3, 80, 9, 13, False),
             D("bf16", 3, 96, 9, 7, True)]
DW_GPU_CASES = [D("bf16", 16, 64, 80, 80, False), D("bf16", 16, 80, 80, 80, True), D("bf16", 16, 384, 80, 80, False), D("f32", 16, 64, 80, 80, True),
                D("bf16", 64, 768, 40, 40, False)]                 # the last one reaches the 1024-workgroup cap of the weight-gradient split


def dw_id(c):
    return "%s-B%d-C%d-%dx%d-%s" % (c["dtype"], c["B"], c["C"], c["H"], c["W"], "view" if c["padded"] else "dense")


def engine_dw(engine, c, x, w, dy, dx_in):
    import ctypes as C
    from yolosharp_amd import _lib
    B, Cc, H, W = x.shape
    dt = 1 if c["dtype"] == "bf16" else 0
    xl, xo, yl, yo = (Cc + 16, 8, Cc + 24, 16) if c["padded"] else (Cc, 0, Cc, 0)
    y = np.empty_like(x); dx0 = np.empty_like(x); dx1 = dx_in.copy(); dw = np.empty_like(w); dw1 = np.empty_like(w)
    flags = [C.c_int32(-1) for _ in range(3)]
    engine.kernel_profile(True)
    _lib.check(engine.lib, engine.lib.ys_dwconv3x3_fwd(engine.ctx, dt, _vp(x), B, Cc, H, W, _vp(w), xl, xo, yl, yo, _vp(y), C.byref(flags[0])))
    _lib.check(engine.lib, engine.lib.ys_dwconv3x3_bwd(engine.ctx, dt, _vp(x), B, Cc, H, W, _vp(w), _vp(dy), xl, xo, yl, yo, 0, _vp(dx0), _vp(dw), C.byref(flags[1])))
    _lib.check(engine.lib, engine.lib.ys_dwconv3x3_bwd(engine.ctx, dt, _vp(x), B, Cc, H, W, _vp(w), _vp(dy), xl, xo, yl, yo, 1, _vp(dx1), _vp(dw1), C.byref(flags[2])))
    labels = sorted(l[0] for l in profile_labels(engine))
    engine.kernel_profile(False)
    assert labels == ["dwconv_dgrad", "dwconv_dgrad", "dwconv_fwd", "dwconv_wgrad", "dwconv_wgrad"], labels
    assert np.array_equal(dw, dw1)
    return dict(y=y, dx0=dx0, dx1=dx1, dw=dw), tuple(f.value for f in flags)


def run_dw_case(engine, backend, c):
    x, w, dy, dx_in = dw_inputs(c["B"], c["C"], c["H"], c["W"], c["dtype"], seed=c["C"] + 31 * c["W"] + c["H"])
    r64, r32 = dw_formula(x, w, dy, dx_in, torch.float64), dw_formula(x, w, dy, dx_in, torch.float32)
    bnd, _ = dw_bounds(c["dtype"], r64, r32)
    got, intact = engine_dw(engine, c, x, w, dy, dx_in)
    assert intact == (1, 1, 1), ("a kernel wrote outside its view", intact)
    for k_ in ("y", "dx0", "dx1", "dw"):
        check_bound(got[k_], r64[k_], bnd[k_], "%s %s" % (dw_id(c), k_), "%s dwconv %s %s" % (backend, c["dtype"], k_))
    again, _ = engine_dw(engine, c, x, w, dy, dx_in)
    for k_ in got:
        assert np.array_equal(got[k_], again[k_]), "%s differs between two consecutive calls" % k_


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("case", DW_CASES, ids=dw_id)
def test_depthwise_kernels_against_float64(backend, engine, case):
    """Forward, input gradient with accumulate 0 and 1 (dx1 = ONE rounding of dx_in + acc), weight gradient; padded input / output views on every other case."""
    run_dw_case(engine, backend, case)


@pytest.mark.gpu
@pytest.mark.parametrize("backend", ["gpu"])
@pytest.mark.parametrize("case", DW_GPU_CASES, ids=dw_id)
def test_depthwise_production_shapes(backend, engine, case):
    run_dw_case(engine, backend, case)


@pytest.mark.parametrize("backend", BACKENDS)
def test_depthwise_rejects_unsupported_geometry(backend, engine):
    """C not a multiple of the 16-byte vector (both passes), C / vector > 256 for the weight gradient: the launcher's YS_ERR_UNSUPPORTED, no kernel started."""
    z = lambda *s: np.zeros(s, np.float32)
    engine.kernel_profile(True)
    for dt, C_ in ((1, 12), (0, 6)):
        assert engine.lib.ys_dwconv3x3_fwd(engine.ctx, dt, _vp(z(1, C_, 2, 2)), 1, C_, 2, 2, _vp(z(C_, 1, 3, 3)), C_, 0, C_, 0, _vp(z(1, C_, 2, 2)), None) == YS_ERR_UNSUPPORTED
        assert b"must be a multiple" in engine.lib.ys_last_error()
    for dt, C_ in ((1, 2056), (0, 1028)):
        a = z(1, C_, 1, 1)
        assert engine.lib.ys_dwconv3x3_bwd(engine.ctx, dt, _vp(a), 1, C_, 1, 1, _vp(z(C_, 1, 3, 3)), _vp(a), C_, 0, C_, 0, 0, _vp(z(1, C_, 1, 1)), _vp(z(C_, 1, 3, 3)),
                                           None) == YS_ERR_UNSUPPORTED
        assert b"wgrad: unsupported" in engine.lib.ys_last_error()
    labels = profile_labels(engine)
    engine.kernel_profile(False)
    assert labels == [], labels


# ------------------------------------------------------------------ the bounds themselves, without the engine
EMU_ATTN = ATTN_CASES + [dict(c, B=1, heads=min(c["heads"], 2)) for c in ATTN_GPU_CASES]


@pytest.mark.parametrize("case", EMU_ATTN, ids=case_id)
def test_attention_bounds_hold_for_an_emulation_of_the_rounding_points(case):
    """Every attention case (the GPU-only shapes at B = 1) through a torch-fp32 emulation of the kernels' rounding points: stored operands, fp32 accumulation in a
    second summation order, P / dS rounded to bf16 in front of the second product on the MFMA route, one store rounding.  Zero elements out of bound on the inputs the
    engine tests use: the bounds are wide enough for a correct kernel there, so an engine failure is the engine's."""
    p = prepare_attn(case)
    _note("emulation attn %s %s" % (case["dtype"], "mfma" if p["mfma"] else "scalar"), p["emu_worst"])
    assert p["emu_bad"] == 0, "%s: no draw of %d keeps the emulation inside the bounds; first draw: %d elements out, worst %.3f x" % (
        case_id(case), SEED_TRIES, p["emu_bad"], p["emu_worst"])


def test_depthwise_bounds_hold_for_an_emulation_of_the_rounding_points():
    """The same for the depthwise cases: fp32 tap by tap, fp32 row sums for dw, one store rounding (dx with accumulate: ONE rounding of dx_in + acc)."""
    for c in DW_CASES + [dict(c, B=1) for c in DW_GPU_CASES]:
        x, w, dy, dx_in = dw_inputs(c["B"], c["C"], c["H"], c["W"], c["dtype"], seed=c["C"] + 31 * c["W"] + c["H"])
        r64, r32 = dw_formula(x, w, dy, dx_in, torch.float64), dw_formula(x, w, dy, dx_in, torch.float32)
        bnd, _ = dw_bounds(c["dtype"], r64, r32)
        emu = dw_emulate(x, w, dy, dx_in, c["dtype"])
        for k_ in ("y", "dx0", "dx1", "dw"):
            check_bound(emu[k_], r64[k_], bnd[k_], "emulation %s %s" % (dw_id(c), k_), "emulation dwconv %s %s" % (c["dtype"], k_))
