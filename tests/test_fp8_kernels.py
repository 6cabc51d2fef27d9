"""The fp8 convolution path kernel by kernel against exact references (recipe in csrc/f8.hip), through the stateless entries ys_f8_quant / ys_f8_scales /
ys_bn_apply_q8_fwd / ys_bn_apply_q8_bwd / ys_conv_f8_fwd / ys_conv_f8_dgrad (csrc/ops_conv.hip and ops_bn.hip: the production launchers called unchanged).

What is held.
  quantisers        every bf16 bit pattern through f8_quant_view_kernel<e4m3 / e5m2> and f8_quant_weights_kernel: the decoded bytes EQUAL
                    quant(float32(x) * float32(scale)) -- ties to even, subnormals, flush to zero, saturation at 448 / 57344, and the region past 480 / 61440
                    where the unclamped conversion instruction gives NaN / Inf.  The decode tables below are written from the OCP definitions.
  views             bytes exact, amax = max |bf16(x)| bit for bit, slots no workgroup owns stay 0, sentinels intact.
  scale bookkeeping amax_w exact, slots cleared, kept scales kept, s_x / s_g / reciprocals within 4 * 2^-24 of the float32 restatement (at most three fp32
                    operations of one ulp each).
  q8 BatchNorm      z / dy inside the bounds tests/test_bn_kernels.py holds the plain apply passes to; the fp8 image EQUALS quant(z_dev * qs) of the returned bf16
                    tensor; amax = max |z_dev|.
  convolutions      every kernel family and tile of the fp8 route, the route asserted from the per-launch profile.  Per element
                        |y - ref| <= 2^-8 |ref| + (K + 2) ACC_ULP A
                    ref = float64 convolution of the quantised operands times deq (+ bias), A = the same convolution of the absolute values, K = taps * Cin.
                    The result is stored in bf16 (8 significant bits): half an ulp is 2^-9 of the binade's top, 2^-8 |ref| at its bottom.  Products of two 4-bit
                    significands are exact in fp32; what is left is K - 1 additions, the rescale and the bias, each charged ACC_ULP: 2^-23 as derived (not 2^-24:
                    the MFMA adder's rounding is not documented as nearest even), widened to 2^-21 for what the MI355X's fp8 MFMA adder was measured to drop
                    (see ACC_ULP).
  delayed scale     a previous amax 4x (dgrad 16x) too small saturates operands, one 4096x too large flushes them to subnormals and zero: the output stays finite
                    and inside the same bound against the reference quantised with THAT scale; the amax the launch records is max |bf16(input)| whatever the
                    scale was.
Worst error / bound per path: printed after the module's last test (pytest -s); the measured tables are in DESIGN.md ("Per-kernel parity of the fp8 path").
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import BACKENDS
from test_fp8 import bf16, q_e4m3, q_e5m2
import test_bn_kernels as K

f32, f64 = np.float32, np.float64
E4M3_MAX, E5M2_MAX = 448.0, 57344.0


def _decode_table(exp_bits, man_bits, bias, fn):
    """OCP 8-bit floating point (OFP8 rev 1.0): sign, exp_bits, man_bits; exponent 0 = subnormal m 2^(1 - bias - man_bits).  fn (e4m3): no infinities, only
    S.1111.111 is NaN; e5m2 is IEEE-like: exponent 31 = Inf (m = 0) / NaN."""
    t = np.zeros(256, f64)
    for b in range(256):
        e, m = (b >> man_bits) & ((1 << exp_bits) - 1), b & ((1 << man_bits) - 1)
        if e == 0:
            v = m * 2.0 ** (1 - bias - man_bits)
        elif e == (1 << exp_bits) - 1 and (m == (1 << man_bits) - 1 if fn else True):
            v = np.nan if (fn or m) else np.inf
        else:
            v = (1 + m * 2.0 ** -man_bits) * 2.0 ** (e - bias)
        t[b] = -v if b & 0x80 else v
    return t


DEC = {"e4m3": _decode_table(4, 3, 7, True), "e5m2": _decode_table(5, 2, 15, False)}
QUANT = {"e4m3": q_e4m3, "e5m2": q_e5m2}
FMAX = {"e4m3": E4M3_MAX, "e5m2": E5M2_MAX}


def test_decode_tables():
    assert DEC["e4m3"][0x7E] == 448 and np.isnan(DEC["e4m3"][0x7F]) and DEC["e4m3"][0x01] == 2.0 ** -9 and DEC["e4m3"][0x08] == 2.0 ** -6 and DEC["e4m3"][0xB8] == -1
    assert DEC["e5m2"][0x7B] == 57344 and np.isinf(DEC["e5m2"][0x7C]) and np.isnan(DEC["e5m2"][0x7D]) and DEC["e5m2"][0x01] == 2.0 ** -16 and DEC["e5m2"][0x3C] == 1
    for fmt in DEC:           # the quantiser of test_fp8.py is the identity on every finite code point
        fin = DEC[fmt][np.isfinite(DEC[fmt])]
        assert np.array_equal(QUANT[fmt](fin.astype(f32)).astype(f64), fin)


def expect_q(x, qs, fmt):
    """quant(float32(x) * float32(qs)): the product is ONE fp32 operation (it may overflow to Inf, which saturates)."""
    with np.errstate(over="ignore"):
        return QUANT[fmt](np.asarray(x, f32) * f32(qs)).astype(f64)


def all_bf16_patterns():
    """All 65 536 bf16 bit patterns as float32 [4096][16]; the 256 NaN / Inf patterns replaced by finite values at the formats' edges."""
    u = (np.arange(65536, dtype=np.uint32) << 16)
    x = u.view(f32).copy()
    bad = ~np.isfinite(x)
    edge = np.array([448, 464, 479.9, 480, 496, 57344, 61439, 61440, 65536, 0.0009765625, 0.0029296875, 7.62939453125e-06], f32)
    fill = bf16(np.resize(np.concatenate([edge, -edge]), int(bad.sum())))
    x[bad] = fill
    assert np.isfinite(x).all() and np.array_equal(bf16(x), x)
    return x.reshape(4096, 16)


PATTERNS = all_bf16_patterns()
SCALES = [1.0, 2.0 ** -7, 2.0 ** 9, 448 / 3.7]


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("fmt", ["e4m3", "e5m2"])
def test_quant_view_every_bf16_pattern(backend, engine, fmt):
    for qs in SCALES:
        out = engine.f8_quant(PATTERNS, fmt, qscale=qs)
        got, want = DEC[fmt][out["q8"]], expect_q(PATTERNS, qs, fmt)
        bad = ~(got == want)
        assert not bad.any(), (fmt, qs, int(bad.sum()), PATTERNS[bad][:6], got[bad][:6], want[bad][:6])
        assert np.abs(want).max() == FMAX[fmt] and (np.abs(PATTERNS.astype(f64) * f64(f32(qs))) > 1.08 * FMAX[fmt]).any()      # saturation was exercised
        assert out["amax"] == np.abs(PATTERNS).max() and out["view_intact"] == 1


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("n", [65536, 65536 - 3, 5])
def test_quant_weights_every_bf16_pattern(backend, engine, n):
    flat = PATTERNS.reshape(1, -1)[:, 65536 - n:]
    for aw in (448.0, 448.0 * 128, 0.875, 3.7, 0.0):
        sw = f32(448.0) / f32(aw) if aw > 0 else f32(1.0)
        out = engine.f8_quant(flat, "weights", qscale=aw)
        got, want = DEC["e4m3"][out["q8"]], expect_q(flat, sw, "e4m3")
        bad = ~(got == want)
        assert not bad.any(), (n, aw, int(bad.sum()), flat[bad][:6], got[bad][:6], want[bad][:6])
        assert out["view_intact"] == 1, "the weight quantiser wrote behind its %d bytes" % n
        assert not out["slots"].any()


VIEWS = [(37, 32, 0, 0), (37, 48, 16, 8), (1031, 64, 64, 24), (5, 16, 8, 0)]


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("view", VIEWS, ids=lambda v: "x".join(map(str, v)))
def test_quant_and_amax_on_views(backend, engine, view):
    rows, C, coff, pad = view
    rng = np.random.default_rng(rows * 131 + C)
    x = bf16(rng.standard_normal((rows, C)) * np.exp(rng.uniform(-6, 3, (rows, C))))
    x[rng.random((rows, C)) < 0.05] = 0
    want_amax = np.abs(x).max()
    ways = engine.f8_amax_ways()
    for kind, per in (("e4m3", 16), ("e5m2", 16), ("amax", 8)):
        qs = FMAX.get(kind, 1.0) / float(np.quantile(np.abs(x), 0.9))          # a tenth of the tensor saturates
        out = engine.f8_quant(x, kind, qscale=qs, coff=coff, pad=pad)
        assert out["view_intact"] == 1, kind
        assert out["amax"].tobytes() == want_amax.tobytes() and out["amax"] < 1e6, (kind, out["amax"], want_amax)          # bit for bit; never the sentinel (8.65e8)
        grid = min(max(-(-rows * (C // per) // 1024), 1), 2048)      # four vectors per thread: the launchers' grid
        assert out["slots"].max() == out["amax"] and not out["slots"][min(grid, ways):].any() and (out["slots"] >= 0).all(), (kind, grid, out["slots"])
        if kind != "amax":
            got, want = DEC[kind][out["q8"]], expect_q(x, qs, kind)
            assert np.array_equal(got, want), (kind, int((got != want).sum()))
            assert (np.abs(want) == FMAX[kind]).mean() > 0.01
    if (coff, pad) == (0, 0):
        for kind in ("e4m3", "e5m2", "amax"):
            out = engine.f8_quant(np.zeros((rows, C), f32), kind, qscale=3.0)
            assert out["amax"] == 0 and not out["slots"].any() and out["view_intact"] == 1
            assert kind == "amax" or not DEC[kind][out["q8"]].any()


# ------------------------------------------------------------------ scale bookkeeping
def scales_ref(aw, ax, ag, prev):
    """f8_scales_kernel in float32: {s_x, 1 / (s_x s_w), s_g, 1 / (s_g s_w)}; ax / ag = maximum over the ways (0 = nothing recorded)."""
    one = f32(1)
    sw = f32(448) / aw if aw > 0 else one
    sx = f32(224) / ax if ax > 0 else prev[0]          # 0.5f * 448.f folds to 224 exactly
    sg = f32(8192) / ag if ag > 0 else prev[2]
    sx = sx if sx > 0 else one
    sg = sg if sg > 0 else one
    return np.array([sx, one / (sx * sw), sg, one / (sg * sw)], f32)


@pytest.mark.parametrize("backend", BACKENDS)
def test_scale_bookkeeping(backend, engine):
    rng = np.random.default_rng(5)
    ways = engine.f8_amax_ways()
    sizes = [1, 15, 16, 1023, 1024, 4096 + 3, 100]
    layers, chunks, off = [], [], 3
    params = [rng.standard_normal(off).astype(f32) * 50]          # parameters that belong to no layer, larger than every layer's
    for i, n in enumerate(sizes):
        w = (rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 1)).astype(f32) if i < 6 else np.zeros(n, f32)
        if n > 1000:
            w[-1] = -3 * np.abs(w).max()                             # the maximum in the last element of a chunked layer, negative
        layers.append((off, n)); params.append(w); off += n
    params.append(rng.standard_normal(5).astype(f32) * 50)
    params = np.concatenate(params)
    n = 300
    conv_layer = (np.arange(n) * 3 + 1) % 7
    ax, ag = np.zeros((n, ways), f32), np.zeros((n, ways), f32)
    prev = np.zeros((n, 4), f32)
    for c in range(n):
        state = c % 5
        one = lambda a: a.__setitem__((c, (c * 7) % ways), f32(10.0 ** rng.uniform(-3, 3)))
        many = lambda a: a.__setitem__((c, rng.choice(ways, 1 + c % 9, replace=False)), (10.0 ** rng.uniform(-3, 3, 1 + c % 9)).astype(f32))
        prev[c] = rng.uniform(0.01, 100, 4) if state != 3 else 0           # state 3: no maximum and a previous scale of 0 -> 1
        if state == 0:
            one(ax); many(ag)
        elif state == 1:
            many(ax); one(ag)
        elif state == 4:
            many(ag) if c % 2 else one(ag)                                   # a gradient maximum without an activation maximum
    aw, ax1, ag1, sc = engine.f8_scales(params, layers, conv_layer, ax, ag, prev)
    want_aw = np.array([np.abs(params[o:o + k]).max() for o, k in layers], f32)
    assert aw.tobytes() == want_aw.tobytes(), (aw, want_aw)
    assert want_aw[6] == 0
    assert not ax1.any() and not ag1.any(), "slots not cleared"
    want = np.stack([scales_ref(want_aw[conv_layer[c]], ax[c].max(), ag[c].max(), prev[c]) for c in range(n)])
    rel = np.abs(sc.astype(f64) - want) / np.abs(want.astype(f64))
    K._note("fp8 scales (4 2^-24)", rel.max() / (4 * 2.0 ** -24))
    assert np.isfinite(sc).all() and rel.max() <= 4 * 2.0 ** -24, rel.max() * 2.0 ** 24
    kept_x, kept_g = ax.max(1) == 0, ag.max(1) == 0
    assert kept_x.sum() >= 100 and kept_g.sum() >= 100
    assert np.array_equal(sc[kept_x, 0], np.where(prev[kept_x, 0] > 0, prev[kept_x, 0], 1)) and np.array_equal(sc[kept_g, 2], np.where(prev[kept_g, 2] > 0, prev[kept_g, 2], 1))
    aw2, ax2, ag2, sc2 = engine.f8_scales(params, layers, conv_layer, ax1, ag1, sc)
    assert np.array_equal(sc2, sc) and np.array_equal(aw2, aw) and not ax2.any() and not ag2.any()


# ------------------------------------------------------------------ the quantising BatchNorm passes
Q8_SHAPES = [(50, 16), (129, 40), (1500, 64)]


def _q8_common(out, t, qs, fmt, what):
    """The contract written in bn_q8_store: the image is the quantised STORED tensor, amax is its maximum."""
    t_dev = out[t]
    assert np.array_equal(K.bf16r(t_dev), t_dev), what + ": not bf16"
    got, want = DEC[fmt][out["q8"]], expect_q(np.ascontiguousarray(t_dev.T), qs, fmt)
    assert np.array_equal(got, want), "%s: %d image bytes differ from quant(stored value * qs)" % (what, int((got != want).sum()))
    assert out["amax"].tobytes() == np.abs(t_dev).max().tobytes(), (what, out["amax"], np.abs(t_dev).max())
    assert out["view_intact"] == 1, what + ": a sentinel was overwritten"


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("res", [None, "view", "shared"])
@pytest.mark.parametrize("act", [1, 0])
@pytest.mark.parametrize("shape", Q8_SHAPES, ids=lambda s: "%dx%d" % s)
def test_bn_apply_q8_forward(backend, engine, shape, act, res):
    rows, C = shape
    c = dict(dtype="bf16", C=C, rows=rows, act=act, res=res is not None, regimes=False, P=1)
    inp = K.fwd_inputs(c, seed=rows + act)
    y, r = inp["y"], inp["res"]
    y64 = y.astype(f64)
    q = K.coef_form(y64.sum(1), (y64 * y64).sum(1), rows, inp["gamma"], inp["beta"], inp["run_mean"], inp["run_var"], f64)
    sc, sh = q["scale"].astype(f32), q["shift"].astype(f32)
    z64 = K.apply_form(y, sc, sh, r, act, f64)
    qs = f32(E4M3_MAX / np.quantile(np.abs(z64), 0.95))
    assert (np.abs(K.bf16r(z64.astype(f32)) * qs) > E4M3_MAX).mean() > 0.01
    views = dict(z_view=(8, 16), res_view=(16, 8)) if res == "view" else dict(z_view=(8, 0), res_view=(0, C + 8), res_shares_z=True) if res == "shared" else dict(z_view=(16, 8))
    out = engine.bn_apply_q8_fwd(y, sc, sh, qs, act=act, res=r, **views)
    bad = []
    z32 = [K.apply_form(y, sc, sh, r, act, f32, fma) for fma in (False, True)]
    K.violation(out["z"], z64, K.tol(z64, K.d32_max(z32, z64), "bf16"), "z", "fp8 q8 fwd apply", bad)
    assert not bad, bad
    _q8_common(out, "z", qs, "e4m3", "forward %s act%d res=%s" % (shape, act, res))


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("rg", [False, True])
@pytest.mark.parametrize("act", [1, 0])
@pytest.mark.parametrize("shape", Q8_SHAPES, ids=lambda s: "%dx%d" % s)
def test_bn_apply_q8_backward(backend, engine, shape, act, rg):
    rows, C = shape
    c = dict(dtype="bf16", C=C, rows=rows, act=act, rg=rg, regimes=False)
    inp = K.bwd_inputs(c, seed=rows + act)
    y, dz = inp["y"], (inp["dz"] * f32(1e-3)).astype(f32)
    dz = K.bf16r(dz)
    sc, sh, mu, rs = inp["coef"]
    du64, du32 = K.du_form(dz, y, sc, sh, act, f64), K.du_form(dz, y, sc, sh, act, f32)
    fin = K.bwd_fin_form(du64.sum(1), (du64 * y.astype(f64)).sum(1), rows, sc, mu, rs, np.zeros(C), np.zeros(C), f64)
    k2, k3 = fin["k2"].astype(f32), fin["k3"].astype(f32)
    dy64 = K.dy_form(du64, y, sc, k2, k3, f64)
    qs = f32(E5M2_MAX / np.quantile(np.abs(dy64), 0.95))
    assert (np.abs(K.bf16r(dy64.astype(f32)) * qs) > E5M2_MAX).mean() > 0.01
    out = engine.bn_apply_q8_bwd(dz, y, np.stack([sc, sh, k2, k3]), qs, act=act, rg=inp["rg"], dz_view=(8, 16), rg_view=(24, 8))
    bad = []
    dy32 = [K.dy_form(du32, y, sc, k2, k3, f32, fma) for fma in (False, True)]
    K.violation(out["dy"], dy64, K.tol(dy64, K.d32_max(dy32, dy64), "bf16"), "dy", "fp8 q8 bwd apply", bad)
    assert not bad, bad
    if rg:
        assert np.array_equal(out["rg"], K.bf16r(inp["rg"] + dz)), "rg is not rg + dz with one rounding"
    _q8_common(out, "dy", qs, "e5m2", "backward %s act%d rg=%s" % (shape, act, rg))


# ------------------------------------------------------------------ the fp8 convolution kernels
def conv64(x, w, k, s):
    return F.conv2d(torch.from_numpy(np.ascontiguousarray(x)).double(), torch.from_numpy(np.ascontiguousarray(w)).double(), None, stride=s, padding=k // 2).numpy()


def dgrad64(shape, w, k, s, dy):
    xt = torch.zeros(shape, dtype=torch.float64, requires_grad=True)
    F.conv2d(xt, torch.from_numpy(np.ascontiguousarray(w)).double(), None, stride=s, padding=k // 2).backward(torch.from_numpy(np.ascontiguousarray(dy)).double())
    return xt.grad.numpy()


def rel_close(got, want, ulps=4):
    return abs(float(got) - float(want)) <= ulps * 2.0 ** -24 * abs(float(want))


def fwd_reference(x, w, k, s, prev_amax=0.0):
    """The recipe of f8.hip on this call's tensors: (ref, A, scales, amax) -- float64 convolution of the quantised operands times deq, the same of their absolute
    values, the float32 scales, max |bf16(x)|."""
    xb, wb = bf16(x), bf16(w)
    amax = np.abs(xb).max()
    sx = f32(224.0) / f32(prev_amax if prev_amax else amax)
    sw = f32(448.0) / np.abs(w).max()
    xq, wq = q_e4m3(xb * sx), q_e4m3(wb * sw)
    deq = f32(1.0) / (sx * sw)
    return conv64(xq, wq, k, s) * f64(deq), conv64(np.abs(xq), np.abs(wq), k, s) * f64(deq), (sx, deq), amax, (xb * sx, xq)


def dgrad_reference(shape, w, k, s, dy, prev_amax=0.0):
    dyb, wb = bf16(dy), bf16(w)
    amax = np.abs(dyb).max()
    sg = f32(8192.0) / f32(prev_amax if prev_amax else amax)
    sw = f32(448.0) / np.abs(w).max()
    with np.errstate(over="ignore"):
        dyq, wq = q_e5m2(dyb * sg), q_e4m3(wb * sw)
    deq = f32(1.0) / (sg * sw)
    return dgrad64(shape, wq, k, s, dyq) * f64(deq), dgrad64(shape, np.abs(wq), k, s, np.abs(dyq)) * f64(deq), (sg, deq), amax, (dyb * sg, dyq)


# Charge per fp32 operation of the accumulation term.  Derived: 2^-23 (one ulp per addition).  The interpreter stays inside that (worst 0.99 of the whole bound, the
# store rounding itself).  The MI355X does not, on the K = 32 case alone: 2 elements of 7920 at 1.37 x and 1.28 x, all with |ref| < 10^-2 A (cancellation), excess
# 2^-17.4 A.  Shown to be the adder of v_mfma_scale_f32_16x16x128_f8f6f4 and not an operand (tools/dev/f8_mfma_window.py): with operands 1.75 * 2^-j whose
# products lie within 3 binades the device returns bf16(exact sum) on EVERY element of four shapes / both kernels; with the same operand pattern over 11 binades --
# every partial sum of 32 still exact in fp32 in any order, and the interpreter still exact -- 2 % of the elements differ, by up to 2^-16.5 A (2^-15.4 A over 16
# binades): the instruction aligns the 128 products of a block to the largest and drops what falls below its window, independent of K.  So, as the derivation
# allows for an undocumented adder, only this factor is widened, to 2^-21: measured worst accumulation excess / ((K + 2) 2^-21 A) = 0.62 (a K = 32 layer of
# 16 x 16 maps), 0.34 on the cases below.
ACC_ULP = 2.0 ** -21


def held(y, ref, A, Kdim, what, path):
    """|y - ref| <= 2^-8 |ref| + (K + 2) ACC_ULP A on EVERY element (module docstring)."""
    y, ref = np.asarray(y, f64), np.asarray(ref, f64)
    assert np.isfinite(y).all(), what + ": not finite"
    bnd = 2.0 ** -8 * np.abs(ref) + (Kdim + 2) * ACC_ULP * A
    err = np.abs(y - ref)
    pos = bnd > 0
    ratio = float((err[pos] / bnd[pos]).max()) if pos.any() else 0.0
    K._note(path, ratio)
    assert not (err[~pos] > 0).any(), what + ": nonzero where the operands are all zero"
    assert ratio <= 1.0, "%s: %d of %d elements out of bound, worst %.3f x (|err| %.3g)" % (what, int((err > bnd).sum()), err.size, ratio, float(err.max()))


def routed(engine, opts, fn):
    with engine.options(**opts):
        return engine.conv_labels(fn)


def one_label(labels, prefix, *needles):
    """Exactly one convolution launch, on the kernel named."""
    assert len(labels) == 1 and labels[0].startswith(prefix) and all(" " + n + " " in labels[0] + " " for n in needles), (prefix, needles, labels)


def geom(k, s, cin, cout):
    return "k%d s%d div1 cin%d cout%d " % (k * 11, s, cin, cout)


# (B, Cin, H, W, Cout, k, s), kernel, label words, options
FWD_ROUTES = [
    ((2, 32, 9, 11, 40, 1, 1), "p2f8", ("wres1",), {}),                 # K = 32: a quarter K-step, masked Cout
    ((1, 32, 20, 40, 48, 3, 1), "p2f8", ("wres1",), {}),
    ((2, 96, 12, 12, 72, 3, 1), "p2f8", ("wres1",), {}),                # K = 864: 6.75 steps
    ((1, 64, 9, 11, 64, 3, 2), "p2f8", ("wres1",), {}),
    ((3, 128, 13, 7, 16, 1, 1), "p2f8", ("wres1",), {}),
    ((1, 320, 8, 8, 48, 3, 1), "p2f8", ("wres0",), {}),                 # streamed weights; Cout < 64 keeps it off the GEMM kernel
    ((1, 320, 8, 8, 96, 3, 1), "p2f8", ("wres0",), {"GEMM_MIN_CIN": 512}),
    ((1, 160, 9, 11, 80, 3, 2), "gemmf8", ("tile256x80",), {}),         # 11.25 K-tiles, stride 2
    ((2, 192, 7, 9, 64, 3, 1), "gemmf8", ("tile256x64",), {}),
    ((1, 256, 13, 10, 128, 1, 1), "gemmf8", ("tile128x128",), {}),      # two M tiles, exactly two K-tiles
    ((1, 160, 17, 9, 320, 3, 1), "gemmf8", ("tile128x160",), {}),       # two channel tiles
    ((2, 288, 6, 6, 144, 1, 1), "gemmf8", ("tile128x160",), {}),        # 2.25 K-tiles, Cout 144 of 160
]
EVAL_ROUTES = [2, 10]
fwd_id = lambda i: "x".join(map(str, FWD_ROUTES[i][0]))


def fwd_tensors(case, seed):
    B, Cin, H, W, Cout, k, s = case
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, Cin, H, W, generator=g).numpy() * 1.7
    w = (torch.randn(Cout, Cin, k, k, generator=g) / (Cin * k * k) ** 0.5).numpy()
    return x, w, torch.randn(Cout, generator=g).numpy() * 0.3, g


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("i", range(len(FWD_ROUTES)), ids=fwd_id)
def test_conv_f8_forward_bias(backend, engine, i):
    case, kern, words, opts = FWD_ROUTES[i]
    B, Cin, H, W, Cout, k, s = case
    x, w, bias, _ = fwd_tensors(case, 300 + i)
    out, labels = routed(engine, opts, lambda: engine.conv_f8_fwd(x, w, k, s, bias=bias, act=False))
    one_label(labels, kern + " " + geom(k, s, Cin, Cout), *words)
    ref, A, (sx, deq), amax, _ = fwd_reference(x, w, k, s)
    held(out["y"], ref + bias.astype(f64)[None, :, None, None], A, k * k * Cin, "forward %s" % (case,), "fp8 conv forward %s" % kern)
    assert rel_close(out["scales"][0], sx) and rel_close(out["scales"][1], deq), (out["scales"], sx, deq)
    assert out["amax"].tobytes() == amax.tobytes(), (out["amax"], amax)


def bn_tensors(Cout, g):
    return {"weight": torch.rand(Cout, generator=g) + 0.5, "bias": torch.randn(Cout, generator=g) * 0.1,
            "running_mean": torch.randn(Cout, generator=g) * 0.1, "running_var": torch.rand(Cout, generator=g) + 0.5}


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("i", range(len(FWD_ROUTES)), ids=fwd_id)
def test_conv_f8_forward_train_bn(backend, engine, i):
    """Training BatchNorm + SiLU behind the fp8 kernels (statistics rows): the rounding-matched reference of tests/test_conv.py's bf16 branch -- bf16 of the
    quantised convolution, float BatchNorm, SiLU -- at the project's bounds for the same epilogue in bf16."""
    from bf16_ref import check_elem
    case, kern, words, opts = FWD_ROUTES[i]
    B, Cin, H, W, Cout, k, s = case
    x, w, _, g = fwd_tensors(case, 400 + i)
    bn = bn_tensors(Cout, g)
    bn_np = {kk: v.numpy().copy() for kk, v in bn.items()}
    out, labels = routed(engine, opts, lambda: engine.conv_f8_fwd(x, w, k, s, bn=bn_np, act=True, training=True))
    one_label(labels, kern + " " + geom(k, s, Cin, Cout), *words)
    ref, A, _, _, _ = fwd_reference(x, w, k, s)
    held(out["y_raw"], ref, A, k * k * Cin, "raw output %s" % (case,), "fp8 conv forward %s" % kern)
    yq = torch.from_numpy(bf16(ref.astype(f32)))
    z = F.silu(F.batch_norm(yq, bn["running_mean"], bn["running_var"], bn["weight"], bn["bias"], training=True, momentum=0.03, eps=1e-3)).numpy()
    check_elem(out["y"], z, "fp8 conv + BN %s" % (case,), max_out=1e-4, out_mult=2.0)
    assert np.allclose(bn_np["running_mean"], bn["running_mean"].numpy(), rtol=2e-2, atol=2e-2)
    assert np.allclose(bn_np["running_var"], bn["running_var"].numpy(), rtol=2e-2, atol=2e-2)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("i", EVAL_ROUTES, ids=fwd_id)
def test_conv_f8_forward_eval_bn(backend, engine, i):
    """Eval BatchNorm + SiLU folded into the fp8 kernels' epilogue: scale / shift on the fp32 accumulator, SiLU, one bf16 store."""
    from bf16_ref import check_elem
    case, kern, words, opts = FWD_ROUTES[i]
    B, Cin, H, W, Cout, k, s = case
    x, w, _, g = fwd_tensors(case, 500 + i)
    bn = bn_tensors(Cout, g)
    bn_np = {kk: v.numpy().copy() for kk, v in bn.items()}
    out, labels = routed(engine, opts, lambda: engine.conv_f8_fwd(x, w, k, s, bn=bn_np, act=True, training=False))
    one_label(labels, kern + " " + geom(k, s, Cin, Cout), *words)
    ref, _, _, _, _ = fwd_reference(x, w, k, s)
    z = F.silu(F.batch_norm(torch.from_numpy(ref), bn["running_mean"].double(), bn["running_var"].double(), bn["weight"].double(), bn["bias"].double(),
                            training=False, eps=1e-3)).numpy()
    check_elem(out["y"], z, "fp8 conv + eval BN %s" % (case,), max_out=1e-4, out_mult=2.0)
    assert all(np.array_equal(bn_np[kk], bn[kk].numpy()) for kk in bn), "eval changed the BatchNorm state"


# dgrad (e5m2 input): case, {phase geometry: kernel} -- the dgrad convolution has cin = the layer's Cout, cout = the layer's Cin
DGRAD_ROUTES = [
    ((1, 64, 11, 13, 160, 3, 1), {"k33": "gemmf8"}),
    ((2, 96, 9, 9, 256, 1, 1), {"k11": "gemmf8"}),
    ((2, 64, 12, 12, 64, 3, 1), {"k33": "p2f8"}),
    ((1, 128, 6, 6, 96, 1, 1), {"k11": "p2f8"}),
    ((1, 64, 14, 10, 192, 3, 2), {"k11": "p2f8", "k12": "gemmf8", "k21": "gemmf8", "k22": "gemmf8"}),      # stride-2 phases
    ((2, 128, 9, 11, 128, 3, 2), {"k11": "p2f8", "k12": "p2f8", "k21": "p2f8", "k22": "p2f8"}),
]


def dgrad_tensors(case, seed):
    B, Cin, H, W, Cout, k, s = case
    g = torch.Generator().manual_seed(seed)
    w = (torch.randn(Cout, Cin, k, k, generator=g) / (Cin * k * k) ** 0.5).numpy()
    Ho, Wo = (H + 2 * (k // 2) - k) // s + 1, (W + 2 * (k // 2) - k) // s + 1
    return w, torch.randn(B, Cout, Ho, Wo, generator=g).numpy() * 1e-3


def dgrad_routes_ok(labels, case, want):
    B, Cin, H, W, Cout, k, s = case
    got = {}
    for l in labels:
        kern, kk, ss, div, cin, cout = l.split()[:6]
        assert (cin, cout) == ("cin%d" % Cout, "cout%d" % Cin), l
        assert kk not in got, labels
        got[kk] = kern
    assert got == want, (case, labels)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("i", range(len(DGRAD_ROUTES)), ids=lambda i: "x".join(map(str, DGRAD_ROUTES[i][0])))
def test_conv_f8_dgrad(backend, engine, i):
    case, want = DGRAD_ROUTES[i]
    B, Cin, H, W, Cout, k, s = case
    w, dy = dgrad_tensors(case, 600 + i)
    out, labels = routed(engine, {}, lambda: engine.conv_f8_dgrad((B, Cin, H, W), w, k, s, dy))
    dgrad_routes_ok(labels, case, want)
    ref, A, (sg, deq), amax, _ = dgrad_reference((B, Cin, H, W), w, k, s, dy)
    taps = (-(-k // s)) ** 2                       # a stride-2 phase sums at most 2 x 2 taps
    held(out["dx"], ref, A, taps * Cout, "dgrad %s" % (case,), "fp8 conv dgrad " + "+".join(sorted(set(want.values()))))
    assert rel_close(out["scales"][2], sg) and rel_close(out["scales"][3], deq), (out["scales"], sg, deq)
    assert out["amax"].tobytes() == amax.tobytes(), (out["amax"], amax)


# ------------------------------------------------------------------ delayed scaling
DELAYED = [((2, 64, 12, 12, 64, 3, 1), "p2f8"), ((1, 160, 10, 12, 256, 3, 1), "gemmf8")]


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("factor", [0.25, 4096.0], ids=["saturating", "flushing"])
@pytest.mark.parametrize("i", range(len(DELAYED)), ids=lambda i: DELAYED[i][1])
def test_delayed_scale_forward(backend, engine, i, factor):
    case, kern = DELAYED[i]
    B, Cin, H, W, Cout, k, s = case
    x, w, bias, _ = fwd_tensors(case, 700 + i)
    amax = np.abs(bf16(x)).max()
    prev = f32(amax * f32(factor))
    out, labels = routed(engine, {}, lambda: engine.conv_f8_fwd(x, w, k, s, bias=bias, act=False, prev_amax=prev))
    one_label(labels, kern + " " + geom(k, s, Cin, Cout))
    ref, A, (sx, deq), _, (xs, xq) = fwd_reference(x, w, k, s, prev_amax=prev)
    if factor < 1:
        assert (np.abs(xs) > E4M3_MAX).mean() > 0.01 and np.abs(xq).max() == E4M3_MAX
    else:
        assert (np.abs(xs) < 2.0 ** -6).mean() > 0.5 and (xq == 0).mean() > 0.01 and np.abs(ref).max() > 0          # e4m3 subnormals (below 2^-6) and zero
    held(out["y"], ref + bias.astype(f64)[None, :, None, None], A, k * k * Cin, "delayed forward %s x%g" % (case, factor), "fp8 delayed forward %s" % kern)
    assert rel_close(out["scales"][0], sx) and rel_close(out["scales"][1], deq), (out["scales"], sx, deq)
    assert out["amax"].tobytes() == amax.tobytes(), "the recorded amax %r is not max |bf16(x)| = %r" % (out["amax"], amax)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("i", range(len(DELAYED)), ids=lambda i: DELAYED[i][1])
def test_delayed_scale_dgrad(backend, engine, i):
    case, kern = DELAYED[i]
    B, Cin, H, W, Cout, k, s = case
    w, dy = dgrad_tensors(case, 800 + i)
    amax = np.abs(bf16(dy)).max()
    prev = f32(amax / f32(16))
    out, labels = routed(engine, {}, lambda: engine.conv_f8_dgrad((B, Cin, H, W), w, k, s, dy, prev_amax=prev))
    dgrad_routes_ok(labels, case, {"k33": kern})
    ref, A, (sg, deq), _, (ds, dq) = dgrad_reference((B, Cin, H, W), w, k, s, dy, prev_amax=prev)
    assert (np.abs(ds) > E5M2_MAX).mean() > 0.01 and np.abs(dq).max() == E5M2_MAX
    held(out["dx"], ref, A, k * k * Cout, "delayed dgrad %s" % (case,), "fp8 delayed dgrad %s" % kern)
    assert rel_close(out["scales"][2], sg) and rel_close(out["scales"][3], deq), (out["scales"], sg, deq)
    assert out["amax"].tobytes() == amax.tobytes(), "the recorded amax %r is not max |bf16(dy)| = %r" % (out["amax"], amax)


@pytest.mark.parametrize("backend", BACKENDS)
def test_recorded_amax_stride_2(backend, engine):
    """The amax recorded by a stride-2 forward launch and by the phase launches of a stride-2 dgrad, under a scale that is not the tensor's own."""
    case = (1, 64, 9, 11, 64, 3, 2)
    x, w, bias, _ = fwd_tensors(case, 900)
    out, labels = routed(engine, {}, lambda: engine.conv_f8_fwd(x, w, 3, 2, bias=bias, act=False, prev_amax=0.37))
    one_label(labels, "p2f8 " + geom(3, 2, 64, 64))
    assert out["amax"].tobytes() == np.abs(bf16(x)).max().tobytes()
    case, want = DGRAD_ROUTES[4]
    w, dy = dgrad_tensors(case, 901)
    out, labels = routed(engine, {}, lambda: engine.conv_f8_dgrad(case[:4], w, 3, 2, dy, prev_amax=0.37))
    dgrad_routes_ok(labels, case, want)
    assert out["amax"].tobytes() == np.abs(bf16(dy)).max().tobytes()


@pytest.fixture(scope="module", autouse=True)
def fp8_ratio_table():
    """After the module's last test: the worst error / bound per path (pytest -s) -- the table of DESIGN.md."""
    yield
    print()
    for path in sorted(p for p in K.RATIOS if p.startswith("fp8 ")):
        print("worst error/bound %-34s %.3f" % (path, K.RATIOS[path]))
