"""The BatchNorm training kernels of csrc/batchnorm.hip kernel by kernel against float64, through the stateless entry points ys_bn_train_fwd / ys_bn_train_bwd /
ys_colsum / ys_upsample2x / ys_copy_view / ys_conv_bn_act_fwd_ex (csrc/ops_bn.hip, ops_conv.hip: host arrays staged into sentinel-padded views, the production launchers
called unchanged) -- no convolution, block or model between the kernel and the comparison.

What is compared.  Every kernel against ITS OWN inputs, so that one kernel's allowed error is not charged to the next:
  statistics / reduction partial rows   sum over the returned rows (float64)  vs  float64 sums over the stored operands
  finalize coefficients                 scale, shift, mean, rstd, running statistics (forward); dgamma, dbeta, k2, k3 (backward)
                                        vs  the float64 formula on the sum of the RETURNED partial rows (or of the test's own rows: accumulator path, FinSrc)
  apply passes                          z  vs  act(y scale + shift) + res with the RETURNED scale / shift;  dy  vs  scale du - k2 - y k3 with the returned k2 / k3
and end to end: z and the running statistics against torch.nn.functional.batch_norm(training=True, momentum=0.03, eps=1e-3) + SiLU + residual in float64, dy /
dgamma / dbeta against float64 autograd through that same expression (not a restatement of the k2 / k3 algebra).  Operands are rounded to the storage type first;
the statistics are over the stored y.

Bounds, none of them a free constant.  d32 = max |float32 evaluation - float64 evaluation| of the same algebraic form on the same inputs, per compared tensor,
measured at run time.  "The same form" is the kernel's: var = E[y^2] - mean^2, sum(du xhat) = rstd (sum(du y) - mean sum(du)), dy = scale du - k2 - y k3 -- their
conditioning is the kernel's, not autograd's.  For per-channel sums the float32 evaluation is a SEQUENTIAL accumulation (forward and reversed order, the larger
error): the pessimistic order, the kernels sum in lanes and trees.
  fp32 results     |x - ref| <= 8 d32
  bf16 results     |x - ref| <= 2^-8 |ref| + 8 d32
FORMS.  End to end, the float32 evaluation of a pipeline is taken four times: sequential sums forward and reversed, each with the finalize step (coefficients from
the sums) in float32 and in float64 on the float32 sums -- the kernels finalize in double (bn_finalize_kernel, chan_finalize_kernel), and where a pure float32
finalize cancels exactly (one row: fl(du y) - fl(mean du) = 0) the float32 rounding of the sums is the form's whole error.  The apply expressions y scale + shift
and scale du - k2 - y k3 are evaluated with separate roundings and as contracted multiply-adds (the device compiler is free to contract; at one row the true dy is
0 and fma(scale, du, -fl(scale du)) is not).  d32 is the largest over these evaluations.
The SiLU of the device build uses the hardware exponential and reciprocal (1 ulp each, the exponential's argument error |u| 2^-24): below one ulp of silu(u) and of
its derivative for the |u| <= ~6 a normalised activation takes, i.e. inside d32; no extra term.
The fixed-point accumulator path (ys_stat_acc_add, bn_fin_apply_kernel) adds exactly derivable terms.  Each of the P adds per channel is rounded to the nearest
multiple of 2^-20 (the product t 2^20 is exact in fp32 for |t| < 2^32), so each of S1 = sum(y), S2 = sum(y^2) is off by at most e = P 2^-21; with n = rows:
  mean = S1 / n                           d_mean  = e / n
  var = max(S2 / n - mean^2, 0)           d_var   = e / n + 2 |mean| d_mean + d_mean^2                 (the clamp is 1-Lipschitz)
  rstd = (var + eps)^-1/2                 d_rstd  = (max(var - d_var, 0) + eps)^-1/2 - rstd            (decreasing and convex: the left end is the larger step)
  scale = gamma rstd                      d_scale = |gamma| d_rstd
  shift = beta - mean gamma rstd          d_shift = |gamma| (|mean| d_rstd + rstd d_mean + d_mean d_rstd)
  run_mean += 0.03 (mean - run_mean)      0.03 d_mean;        run_var: 0.03 d_var n / (n - 1)
P is the test's own row count, or for a convolution the row count the entry returns (ys_conv_grid_m).  The accumulators themselves are compared EXACTLY: shard
s of channel c holds sum over rows r = s (mod 8) of rint(t 2^20), plus bit 62 of the sum-of-squares word for a partial that is NaN, Inf or >= 2^32 in either word.
Exact statements (array_equal): upsample2x forward, copy_view without accumulate, rg + dz, two consecutive calls of every entry, a grouped launch against the
single-problem launches of the same problems, num_batches_tracked + 1, every sentinel and guard.
test_bounds_hold_for_an_emulation_of_the_rounding_points runs an emulation of the kernels' rounding points (float32 sums in another order than the reference's,
float64 finalize rounded to float32, float32 apply, one store rounding, partials rounded to 2^-20) through the same checks on the CPU, without the engine; the
inputs of a case are redrawn (up to SEED_TRIES times) until the emulation stays inside -- never the bound widened.

Worst error / bound per kernel path, interpreter build (single launches / grouped launches; the module prints the table after its last test with pytest -s):
  forward   statistics rows 0.188 / 0.675   finalize 0.125 / 0.133   accumulator finalize 0.830   apply fp32 0.175 / 0.125   apply bf16 0.995   end to end 0.987
  backward  reduction rows 0.135 / 0.142    finalize 0.125 / 0.205   FinSrc finalize 0.153        apply fp32 0.125 / 0.125   apply bf16 0.995   end to end 0.995
  column sums 0.125   upsample2x backward 0.996   copy_view accumulate 0.996   convolution: accumulators 0.140, statistics rows 0.140, apply 0.993
The same on the MI355X (gfx950 build):
  forward   statistics rows 0.188 / 0.675   finalize 0.184 / 0.193   accumulator finalize 0.830   apply fp32 0.115 / 0.125   apply bf16 0.995   end to end 0.987
  backward  reduction rows 0.125 / 0.142    finalize 0.125 / 0.205   FinSrc finalize 0.125        apply fp32 0.111 / 0.125   apply bf16 0.995   end to end 0.995
  column sums 0.125   upsample2x backward 0.996   copy_view accumulate 0.996   convolution: accumulators 0.154, statistics rows 0.131, apply 0.993
(bf16 ratios near 1 are the store rounding itself: half an ulp at the bottom of a binade is 2^-8 |ref|; 0.125 is a result equal to the float32 evaluation.)
The statistics epilogue of the fp8 convolution kernels (test_conv_epilogue_statistics_fp8, statistics rows only): rows 0.125, apply 0.985 on both builds.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import BACKENDS

U8 = 2.0 ** -8
EPS, MOM = 1e-3, 0.03
FIX = 2.0 ** 20
YS_ERR_INVALID_ARG, YS_ERR_UNSUPPORTED = 1, 4
SEED_TRIES = 4
f32, f64 = np.float32, np.float64


def bf16r(a):
    """float32 array rounded to the nearest bf16 (ties to even), as float32."""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32).reshape(np.shape(a))


def store(a, dtype):
    return bf16r(a) if dtype == "bf16" else np.ascontiguousarray(a, np.float32)


RATIOS = {}
QUIET = ("emulation ", "negative ")        # paths of the CPU-side emulation: not part of the table


def _note(path, ratio):
    RATIOS[path] = max(RATIOS.get(path, 0.0), float(ratio))


@pytest.fixture(scope="module", autouse=True)
def ratio_table():
    """After the module's last test: the worst error / bound per kernel path (pytest -s) -- the table of the module docstring and of DESIGN.md."""
    yield
    print()
    for path in sorted(RATIOS):
        print("worst error/bound %-34s %.3f" % (path, RATIOS[path]))


def violation(x, ref, bnd, what, path, out):
    """Appends a message to `out` when |x - ref| > bnd somewhere (or x is not finite where ref is); notes the worst error / bound of the path."""
    x, ref = np.asarray(x, f64), np.asarray(ref, f64)
    bnd = np.broadcast_to(np.asarray(bnd, f64), ref.shape)
    if not np.isfinite(x).all():
        out.append("%s: not finite" % what)
        return
    err = np.abs(x - ref)
    pos = bnd > 0
    ratio = float((err[pos] / bnd[pos]).max()) if pos.any() else 0.0
    if (err[~pos] > 0).any():
        ratio = float("inf")
    if path and not path.startswith(QUIET):
        _note(path, ratio)
    bad = err > bnd
    if bad.any():
        out.append("%s: %d of %d out of bound, worst %.3f x (|err| %.3g)" % (what, int(bad.sum()), bad.size, ratio, float(err.max())))


def d32_of(a32, a64):
    return float(np.abs(np.asarray(a32, f64) - np.asarray(a64, f64)).max())


def tol(ref, d32, dtype):
    return 8.0 * d32 + (U8 * np.abs(ref) if dtype == "bf16" else 0.0)


def seq32(terms):
    """Sequential float32 accumulation along axis 1 of float32 terms, forward and reversed."""
    t = np.ascontiguousarray(terms, f32)
    return np.cumsum(t, axis=1, dtype=f32)[:, -1], np.cumsum(t[:, ::-1], axis=1, dtype=f32)[:, -1]


def sums_d32(terms32, s64):
    a, b = seq32(terms32)
    return max(d32_of(a, s64), d32_of(b, s64))


# ------------------------------------------------------------------ the kernels' algebraic forms, in float32 or float64
def coef_form(S1, S2, n, g, bt, rm, rv, ft):
    S1, S2, g, bt, rm, rv = (np.asarray(a).astype(ft) for a in (S1, S2, g, bt, rm, rv))
    nn, one = ft(n), ft(1)
    mean = S1 / nn
    var = np.maximum(S2 / nn - mean * mean, ft(0))
    rstd = one / np.sqrt(var + ft(EPS))
    unb = var * nn / (nn - one) if n > 1 else var
    return dict(scale=g * rstd, shift=bt - mean * g * rstd, mean=mean, rstd=rstd, var=var,
                run_mean=(one - ft(MOM)) * rm + ft(MOM) * mean, run_var=(one - ft(MOM)) * rv + ft(MOM) * unb)


def silu_form(u, ft):
    return u / (ft(1) + np.exp(-u))


def mul_add(a, b, c, ft, fma):
    """a * b + c in ft; fma (float32 only): one rounding, as a contracted multiply-add gives (the product of two float32 is exact in float64)."""
    if fma and ft is f32:
        return (a.astype(f64) * b.astype(f64) + c.astype(f64)).astype(f32)
    return a.astype(ft) * b.astype(ft) + c.astype(ft)


def apply_form(y, sc, sh, res, act, ft, fma=False):
    u = mul_add(y, np.asarray(sc)[:, None], np.asarray(sh)[:, None], ft, fma)
    if act:
        u = silu_form(u, ft)
    return u + res.astype(ft) if res is not None else u


def du_form(dz, y, sc, sh, act, ft):
    if not act:
        return dz.astype(ft)
    u = y.astype(ft) * np.asarray(sc).astype(ft)[:, None] + np.asarray(sh).astype(ft)[:, None]
    s = ft(1) / (ft(1) + np.exp(-u))
    return dz.astype(ft) * (s * (ft(1) + u * (ft(1) - s)))


def bwd_fin_form(S1, S2y, n, sc, mu, rs, g0, g1, ft):
    S1, S2y, sc, mu, rs, g0, g1 = (np.asarray(a).astype(ft) for a in (S1, S2y, sc, mu, rs, g0, g1))
    s2 = rs * (S2y - mu * S1)
    m1, m2 = S1 / ft(n), s2 / ft(n)
    return dict(dgamma=g0 + s2, dbeta=g1 + S1, k2=sc * (m1 - mu * rs * m2), k3=sc * rs * m2)


def dy_form(du, y, sc, k2, k3, ft, fma=False):
    c = lambda a: np.asarray(a)[:, None]
    return mul_add(-y, c(k3), mul_add(c(sc), du, -c(k2), ft, fma), ft, fma)


def d32_max(forms32, ref64):
    return max(d32_of(a, ref64) for a in forms32)


def torch_bn(ty, trm, trv, tg, tb):
    """torch's training-mode BatchNorm in float64 on ty [rows][C] (running statistics updated in place).  torch refuses a single value per channel; the engine's
    count-1 rule (biased = unbiased variance = 0) is then written out with the same tensor operations, so that autograd still runs through it."""
    if ty.shape[0] > 1:
        return F.batch_norm(ty, trm, trv, tg, tb, training=True, momentum=MOM, eps=EPS)
    mean, var = ty.mean(0), ty.var(0, unbiased=False)
    if trm is not None:
        trm.mul_(1 - MOM).add_(MOM * mean.detach())
        trv.mul_(1 - MOM).add_(MOM * var.detach())
    return (ty - mean) / torch.sqrt(var + EPS) * tg + tb


def acc_terms(S1, S2, n, g, P):
    """The accumulator path's share of each coefficient's bound (module docstring)."""
    e = P * 2.0 ** -21
    c = coef_form(S1, S2, n, g, 0 * g, 0 * g, 0 * g, f64)
    d_mean = e / n
    d_var = e / n + 2 * np.abs(c["mean"]) * d_mean + d_mean ** 2
    d_rstd = (np.maximum(c["var"] - d_var, 0) + EPS) ** -0.5 - c["rstd"]
    ag = np.abs(np.asarray(g, f64))
    return dict(mean=d_mean, rstd=d_rstd, scale=ag * d_rstd, shift=ag * (np.abs(c["mean"]) * d_rstd + c["rstd"] * d_mean + d_mean * d_rstd),
                run_mean=MOM * d_mean, run_var=MOM * d_var * (n / (n - 1.0) if n > 1 else 1.0))


def chunk_partials(y, P):
    """[P][2][C] float32 partial (sum, sum of squares) rows of y [C][rows]: the rows split into P consecutive chunks (empty chunks give zeros)."""
    C, rows = y.shape
    part = np.zeros((P, 2, C), f32)
    edges = np.linspace(0, rows, P + 1).astype(int)
    y64 = y.astype(f64)
    for k in range(P):
        seg = y64[:, edges[k]:edges[k + 1]]
        part[k, 0], part[k, 1] = seg.sum(1), (seg * seg).sum(1)
    return part


def expected_acc(part):
    """The accumulators after pushing part [P][2][C] through ys_stat_acc_add, as uint64 [8][C][2]."""
    P, _, C = part.shape
    acc = np.zeros((8, C, 2), np.uint64)
    for r in range(P):
        for w in range(2):
            t = part[r, w].astype(f64)
            bad = ~(np.abs(t) < 2.0 ** 32)
            q = np.rint(np.where(bad, 0.0, t) * FIX).astype(np.int64)
            acc[r & 7, :, w] += q.astype(np.uint64)
            acc[r & 7, :, 1] |= np.where(bad, np.uint64(1) << np.uint64(62), np.uint64(0))
    return acc


# ------------------------------------------------------------------ forward: inputs, checks, emulation
def fwd_inputs(c, seed):
    rng = np.random.default_rng(seed)
    C, rows, dt = c["C"], c["rows"], c["dtype"]
    mean = rng.standard_normal((C, 1))
    std = rng.uniform(0.5, 2.0, (C, 1))
    y = rng.standard_normal((C, rows)) * std + mean
    if c["regimes"]:
        y[0] = 8.0 + 0.5 * rng.standard_normal(rows)        # mean >> spread
        y[1] = 0.75                                            # constant: the variance clamps at 0
        y[2] = 1e-3 * rng.standard_normal(rows)               # below the fixed point's resolution per element, not per partial
    inp = dict(y=store(y, dt), gamma=rng.uniform(0.5, 1.5, C).astype(f32), beta=(0.1 * rng.standard_normal(C)).astype(f32),
               run_mean=(0.1 * rng.standard_normal(C)).astype(f32), run_var=rng.uniform(0.5, 1.5, C).astype(f32), nbt=float(rng.integers(0, 1000)),
               res=store(rng.standard_normal((C, rows)), dt) if c["res"] else None)
    inp["partial"] = chunk_partials(inp["y"], c["P"])
    return inp


def fwd_problem(c, inp, mode):
    p = dict(y=inp["y"], gamma=inp["gamma"], beta=inp["beta"], run_mean=inp["run_mean"], run_var=inp["run_var"], nbt=inp["nbt"], res=inp["res"],
             z_pad=c["z"][0], z_coff=c["z"][1], res_pad=c["rv"][0], res_coff=c["rv"][1], res_shares_z=c["share"])
    if mode == 1:
        p["partial"] = inp["partial"]
    return p


def fwd_violations(c, inp, out, mode, tag):
    """Every bound of one forward result (engine or emulation) -> list of messages."""
    bad = []
    dt, act, n = c["dtype"], c["act"], c["rows"]
    y, g, bt, rm, rv, res = inp["y"], inp["gamma"], inp["beta"], inp["run_mean"], inp["run_var"], inp["res"]
    y64 = y.astype(f64)
    S1, S2 = y64.sum(1), (y64 * y64).sum(1)
    names = ("scale", "shift", "mean", "rstd")
    coef = dict(zip(names, out["coef"]))
    if mode == 1:
        part = inp["partial"]
        extra = acc_terms(part[:, 0].astype(f64).sum(0), part[:, 1].astype(f64).sum(0), n, g, c["P"])
        if out.get("acc") is not None and not np.array_equal(out["acc"], expected_acc(part)):
            bad.append("accumulators differ from sum of rint(t 2^20) per shard")
    else:
        part = out["part"]
        extra = dict.fromkeys(names + ("run_mean", "run_var"), 0.0)
        violation(part[:, 0].astype(f64).sum(0), S1, 8 * sums_d32(y, S1), "sum y", tag + "fwd statistics rows", bad)
        violation(part[:, 1].astype(f64).sum(0), S2, 8 * sums_d32(y * y, S2), "sum y^2", tag + "fwd statistics rows", bad)
    # finalize against its own inputs: the sums of the partial rows it read
    P1, P2 = part[:, 0].astype(f64).sum(0), part[:, 1].astype(f64).sum(0)
    r64, r32 = coef_form(P1, P2, n, g, bt, rm, rv, f64), coef_form(P1, P2, n, g, bt, rm, rv, f32)
    path = tag + ("fwd accumulator finalize" if mode == 1 else "fwd finalize")
    for k in names:
        violation(coef[k], r64[k], 8 * d32_of(r32[k], r64[k]) + extra[k], k, path, bad)
    for k in ("run_mean", "run_var"):
        violation(out[k], r64[k], 8 * d32_of(r32[k], r64[k]) + extra[k], k, path, bad)
    # apply against its own inputs: the returned scale / shift
    z64 = apply_form(y, coef["scale"], coef["shift"], res, act, f64)
    z32 = [apply_form(y, coef["scale"], coef["shift"], res, act, f32, fma) for fma in (False, True)]
    violation(out["z"], z64, tol(z64, d32_max(z32, z64), dt), "z", tag + "fwd apply " + dt, bad)
    if mode != 1:
        # end to end against torch's BatchNorm in float64; d32 from the whole form in float32 with sequential sums in both orders
        trm, trv = torch.from_numpy(rm.astype(f64)), torch.from_numpy(rv.astype(f64))
        t = torch_bn(torch.from_numpy(y64.T.copy()), trm, trv, torch.from_numpy(g.astype(f64)), torch.from_numpy(bt.astype(f64)))
        t = (F.silu(t) if act else t).numpy().T
        ref = t + res.astype(f64) if res is not None else t
        dz, dm, dv = 0.0, 0.0, 0.0
        for k, ft in ((0, f32), (1, f32), (0, f64), (1, f64)):         # ft: the finalize arithmetic (FORMS)
            q = coef_form(seq32(y)[k], seq32(y * y)[k], n, g, bt, rm, rv, ft)
            dz = max(dz, d32_max([apply_form(y, q["scale"].astype(f32), q["shift"].astype(f32), res, act, f32, fma) for fma in (False, True)], ref))
            dm, dv = max(dm, d32_of(q["run_mean"], trm.numpy())), max(dv, d32_of(q["run_var"], trv.numpy()))
        violation(out["z"], ref, tol(ref, dz, dt), "z end to end", tag + "fwd end to end", bad)
        violation(out["run_mean"], trm.numpy(), 8 * dm, "run_mean end to end", tag + "fwd end to end", bad)
        violation(out["run_var"], trv.numpy(), 8 * dv, "run_var end to end", tag + "fwd end to end", bad)
    return bad


def lane_partials(terms32, nblk):
    """float32 partial rows the way a reduction launch forms them, in another order than seq32: nblk contiguous row ranges, numpy's pairwise sum inside each."""
    C, rows = terms32.shape
    per = -(-rows // nblk)
    return np.stack([terms32[:, k * per:min(rows, (k + 1) * per)].sum(1, dtype=f32) for k in range(nblk)])


def fwd_emulate(c, inp, mode):
    dt, act, n = c["dtype"], c["act"], c["rows"]
    y, res = inp["y"], inp["res"]
    if mode == 1:
        part = inp["partial"]
        S = [np.rint(part[:, w].astype(f64) * FIX).sum(0) / FIX for w in range(2)]
    else:
        nb = max(1, min(768, -(-n // 64)))
        part = np.stack([lane_partials(y, nb), lane_partials(y * y, nb)], axis=1)
        S = [part[:, w].astype(f64).sum(0) for w in range(2)]
    q = coef_form(S[0], S[1], n, inp["gamma"], inp["beta"], inp["run_mean"], inp["run_var"], f64)
    g32 = inp["gamma"]
    rstd = q["rstd"].astype(f32)
    coef = np.stack([g32 * rstd, inp["beta"] - q["mean"].astype(f32) * g32 * rstd, q["mean"].astype(f32), rstd])
    unb = q["var"] * n / (n - 1.0) if n > 1 else q["var"]
    run_mean = (f32(1) - f32(MOM)) * inp["run_mean"] + f32(MOM) * q["mean"].astype(f32)
    run_var = (f32(1) - f32(MOM)) * inp["run_var"] + f32(MOM) * unb.astype(f32)
    z = store(apply_form(y, coef[0], coef[1], res, act, f32), dt)
    return dict(z=z, coef=coef, run_mean=run_mean, run_var=run_var, part=part, acc=expected_acc(part) if mode == 1 else None)


_drawn = {}


def drawn(kind, c, make, emulate_ok):
    """The inputs of case c: redrawn until the emulation stays inside the bounds (at most SEED_TRIES draws)."""
    key = (kind, repr(sorted(c.items())))
    if key not in _drawn:
        msgs = None
        for t in range(SEED_TRIES):
            inp = make(c, 1000 * t + c["seed"])
            msgs = emulate_ok(c, inp)
            if not msgs:
                _drawn[key] = inp
                break
        assert key in _drawn, "no draw of %r keeps the emulation inside the bounds: %s" % (c, msgs)
    return _drawn[key]


def fwd_emulation_msgs(c, inp):
    return [m for mode in (0, 1) for m in fwd_violations(c, inp, fwd_emulate(c, inp, mode), mode, "emulation ")]


def Fw(dtype, C, rows, act=1, res=False, z=(0, 0), rv=(0, 0), share=0, regimes=False, P=8, seed=0):
    return dict(dtype=dtype, C=C, rows=rows, act=act, res=res, z=z, rv=rv, share=share, regimes=regimes, P=P, seed=seed)


FWD_CASES = [
    Fw("bf16", 80, 1003, res=True, z=(8, 16), rv=(16, 8), regimes=True, P=9),          # 10 vectors per row: 25 row lanes, 6 idle threads; the last workgroup's range is short
    Fw("f32", 24, 333, res=True, z=(4, 8), rv=(0, 40), share=1, regimes=True, P=8),     # 6 vectors: 42 row lanes, 4 idle; res and z are views of one buffer
    Fw("bf16", 8, 700, z=(0, 8), P=768),                                                # one vector per row: 256 row lanes; rows not a multiple of 256 x 2
    Fw("f32", 4, 100, act=0, res=True, rv=(4, 4), P=1),                                 # rows below one pass of row lanes; no activation
    Fw("bf16", 2048, 37, act=0, P=9),                                                   # 256 vectors per row, the limit: one row lane, the tree loop does nothing
    Fw("f32", 1024, 13, z=(4, 0), P=8),
    Fw("bf16", 16, 1, res=True, z=(8, 8), rv=(8, 0), P=1),                              # rows = 1: count 1, the unbiased-variance guard
    Fw("f32", 8, 1, act=0, P=9),
    Fw("f32", 32, 1999, res=True, z=(4, 4), rv=(8, 4), regimes=True, P=768),
    Fw("bf16", 32, 1999, act=0, res=True, z=(8, 40), rv=(0, 0), share=1, regimes=True, P=768),
    Fw("bf16", 16, 7, regimes=True, P=8),                                               # a handful of rows: n / (n - 1) = 7 / 6 in run_var
    Fw("f32", 16, 5, regimes=True, res=True, P=9),
]


def fid(c):
    return "%s-C%d-r%d-act%d-P%d" % (c["dtype"], c["C"], c["rows"], c["act"], c["P"])


def same_outputs(a, b, keys):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in keys if a.get(k) is not None)


FWD_KEYS = ("z", "coef", "run_mean", "run_var", "part", "acc")


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("case", FWD_CASES, ids=fid)
def test_bn_forward_kernels(backend, engine, case):
    """chan_reduce_kernel MODE 2 -> bn_finalize_kernel -> bn_act_apply_kernel (mode 0), and ys_stat_acc_add -> bn_fin_apply_kernel (mode 1)."""
    c = case
    inp = drawn("fwd", c, fwd_inputs, fwd_emulation_msgs)
    bad = []
    for mode in (0, 1):
        st, (out,) = engine.bn_train_fwd([fwd_problem(c, inp, mode)], mode, act=c["act"], dtype=c["dtype"])
        assert st == 0, (mode, st)
        assert out["view_intact"] == 1, "mode %d: a kernel wrote outside its view or workspace" % mode
        assert out["nbt"] == inp["nbt"] + 1
        bad += ["mode %d %s" % (mode, m) for m in fwd_violations(c, inp, out, mode, "")]
        st, (again,) = engine.bn_train_fwd([fwd_problem(c, inp, mode)], mode, act=c["act"], dtype=c["dtype"])
        assert st == 0 and same_outputs(out, again, FWD_KEYS), "mode %d: two consecutive calls differ" % mode
    assert not bad, "; ".join(bad)


def group_problems(dtype, n):
    """n problems of different C and rows; the first has EXACTLY 256 x k apply vectors (its last workgroup is full: the pick boundary), the second fills a single
    workgroup partly."""
    epl = 8 if dtype == "bf16" else 4
    shapes = [(4 * epl, 128), (2 * epl, 9), (10 * epl, 77), (epl, 256), (3 * epl, 1), (6 * epl, 300), (epl, 5), (8 * epl, 64), (2 * epl, 511)][:n]
    return [Fw(dtype, C, rows, res=bool(i % 2), z=(epl * (i % 3), epl * (i % 2)), rv=(epl, epl), seed=10 + i) for i, (C, rows) in enumerate(shapes)]


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("n", [1, 2, 9])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_bn_forward_group_matches_single_launches(backend, engine, dtype, n):
    """bn_finalize_group_kernel + bn_act_apply_group_kernel over n problems: bit for bit the single-problem launches of the same problems."""
    cs = group_problems(dtype, n)
    inps = [fwd_inputs(c, c["seed"]) for c in cs]
    for act in (1, 0):
        st, outs = engine.bn_train_fwd([fwd_problem(c, i, 2) for c, i in zip(cs, inps)], 2, act=act, dtype=dtype)
        assert st == 0
        for c, i, o in zip(cs, inps, outs):
            st, (single,) = engine.bn_train_fwd([fwd_problem(c, i, 0)], 0, act=act, dtype=dtype)
            assert st == 0 and o["view_intact"] == 1 and o["nbt"] == i["nbt"] + 1
            assert same_outputs(o, single, FWD_KEYS), "problem C=%d rows=%d differs from its single launch" % (c["C"], c["rows"])
    bad = [m for c, i, o in zip(cs, inps, outs) for m in fwd_violations(dict(c, act=0), i, o, 2, "group ")]
    assert not bad, "; ".join(bad)


@pytest.mark.parametrize("backend", BACKENDS)
def test_group_of_ten_and_wide_rows_are_refused(backend, engine):
    for dtype in ("f32", "bf16"):
        epl = 8 if dtype == "bf16" else 4
        c = Fw(dtype, epl, 3)
        i = fwd_inputs(c, 0)
        st, _ = engine.bn_train_fwd([fwd_problem(c, i, 2)] * 10, 2, dtype=dtype)
        assert st == YS_ERR_INVALID_ARG
        b = bwd_inputs(Bw(dtype, epl, 3), 0)
        st, _ = engine.bn_train_bwd([bwd_problem(Bw(dtype, epl, 3), b)] * 10, 2, dtype=dtype)
        assert st == YS_ERR_INVALID_ARG
        wide = Fw(dtype, 257 * epl, 2)                     # one vector per row past the launchers' limit
        i = fwd_inputs(wide, 0)
        for mode in (0, 2):
            st, _ = engine.bn_train_fwd([fwd_problem(wide, i, mode)], mode, dtype=dtype)
            assert st == YS_ERR_UNSUPPORTED
        wb = Bw(dtype, 257 * epl, 2)
        st, _ = engine.bn_train_bwd([bwd_problem(wb, bwd_inputs(wb, 0))], 0, dtype=dtype)
        assert st == YS_ERR_UNSUPPORTED
        st, _, _ = engine.colsum(np.zeros((1, 256 * epl + 1, 2), f32), np.zeros(256 * epl + 1, f32), dtype=dtype)
        assert st == YS_ERR_UNSUPPORTED


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_stat_acc_poison_and_rounding(backend, engine, dtype):
    """A partial that is NaN, Inf or >= 2^32 in either word gives NaN mean / rstd / running statistics and NaN z in THAT channel only; 2^32 - 256 (the largest
    float32 below the limit) is summed; partials of 0.75 x 2^-20 are rounded UP to one unit each (truncation would drop them)."""
    c = Fw(dtype, 16, 40, P=9, seed=3)
    inp = fwd_inputs(c, c["seed"])
    part = inp["partial"]
    part[3, 0, 2], part[5, 1, 5], part[0, 0, 7], part[8, 1, 9], part[2, 1, 12] = np.nan, np.inf, 2.0 ** 32, -2.0 ** 32, -np.inf
    part[4, 1, 11] = 2.0 ** 32 - 256
    part[:, 0, 14] = 0.75 / FIX
    part[:, 1, 14] = 1.0
    poisoned = [2, 5, 7, 9, 12]
    clean = [k for k in range(16) if k not in poisoned]
    st, (out,) = engine.bn_train_fwd([fwd_problem(c, inp, 1)], 1, dtype=dtype)
    assert st == 0 and out["view_intact"] == 1
    assert np.array_equal(out["acc"], expected_acc(part))
    for k in (out["coef"][2], out["coef"][3], out["run_mean"], out["run_var"]):
        assert np.isnan(k[poisoned]).all() and np.isfinite(k[clean]).all()
    assert np.isnan(out["z"][poisoned]).all() and np.isfinite(out["z"][clean]).all()
    assert out["coef"][2][14] == f32(9.0 / FIX / 40)          # nine partials of 0.75 units -> nine units
    sel = lambda a: None if a is None else a[clean]
    sub = dict(c, C=len(clean))
    inp_c = dict(inp, y=sel(inp["y"]), gamma=sel(inp["gamma"]), beta=sel(inp["beta"]), run_mean=sel(inp["run_mean"]), run_var=sel(inp["run_var"]),
                 partial=np.ascontiguousarray(part[:, :, clean]))
    out_c = dict(z=out["z"][clean], coef=out["coef"][:, clean], run_mean=out["run_mean"][clean], run_var=out["run_var"][clean], acc=None)
    bad = fwd_violations(sub, inp_c, out_c, 1, "poison ")
    assert not bad, "; ".join(bad)


# ------------------------------------------------------------------ backward
def Bw(dtype, C, rows, act=1, rg=False, dzv=(0, 0), rgv=(0, 0), regimes=False, seed=0):
    return dict(dtype=dtype, C=C, rows=rows, act=act, rg=rg, dzv=dzv, rgv=rgv, regimes=regimes, seed=seed)


def bwd_inputs(c, seed):
    rng = np.random.default_rng(seed + 77)
    C, rows, dt = c["C"], c["rows"], c["dtype"]
    f = fwd_inputs(dict(c, res=False, P=1), seed)
    y = f["y"]
    y64 = y.astype(f64)
    q = coef_form(y64.sum(1), (y64 * y64).sum(1), rows, f["gamma"], f["beta"], f["run_mean"], f["run_var"], f64)
    coef = np.stack([q["scale"], q["shift"], q["mean"], q["rstd"]]).astype(f32)
    return dict(y=y, gamma=f["gamma"], beta=f["beta"], coef=coef, dz=store(rng.standard_normal((C, rows)), dt),
                rg=store(rng.standard_normal((C, rows)), dt) if c["rg"] else None,
                dgamma=rng.standard_normal(C).astype(f32), dbeta=rng.standard_normal(C).astype(f32))


def bwd_problem(c, inp):
    return dict(dz=inp["dz"], y=inp["y"], coef=inp["coef"], dgamma=inp["dgamma"], dbeta=inp["dbeta"], rg=inp["rg"],
                dz_pad=c["dzv"][0], dz_coff=c["dzv"][1], rg_pad=c["rgv"][0], rg_coff=c["rgv"][1])


def bwd_violations(c, inp, out, tag):
    bad = []
    dt, act, n = c["dtype"], c["act"], c["rows"]
    y, dz, coef = inp["y"], inp["dz"], inp["coef"]
    sc, sh, mu, rs = coef
    du64, du32 = du_form(dz, y, sc, sh, act, f64), du_form(dz, y, sc, sh, act, f32)
    S1, S2y = du64.sum(1), (du64 * y.astype(f64)).sum(1)
    part = out["part"]
    P1, P2 = part[:, 0].astype(f64).sum(0), part[:, 1].astype(f64).sum(0)
    violation(P1, S1, 8 * sums_d32(du32, S1), "sum du", tag + "bwd reduction rows", bad)
    violation(P2, S2y, 8 * sums_d32(du32 * y, S2y), "sum du y", tag + "bwd reduction rows", bad)
    r64 = bwd_fin_form(P1, P2, n, sc, mu, rs, inp["dgamma"], inp["dbeta"], f64)
    r32 = bwd_fin_form(P1, P2, n, sc, mu, rs, inp["dgamma"], inp["dbeta"], f32)
    got = dict(dgamma=out["dgamma"], dbeta=out["dbeta"], k2=out["k23"][0], k3=out["k23"][1])
    for k in ("dgamma", "dbeta", "k2", "k3"):
        violation(got[k], r64[k], 8 * d32_of(r32[k], r64[k]), k, tag + "bwd finalize", bad)
    y64r = dy_form(du64, y, sc, got["k2"], got["k3"], f64)
    y32r = [dy_form(du32, y, sc, got["k2"], got["k3"], f32, fma) for fma in (False, True)]
    violation(out["dy"], y64r, tol(y64r, d32_max(y32r, y64r), dt), "dy", tag + "bwd apply " + dt, bad)
    if inp["rg"] is not None and not np.array_equal(out["rg"], store(inp["rg"] + dz, dt)):
        bad.append("rg is not rg + dz with one rounding")
    # end to end: float64 autograd through BatchNorm + SiLU; gamma = scale / rstd
    g64 = inp["gamma"].astype(f64)
    ty = torch.from_numpy(y.astype(f64).T.copy()).requires_grad_(True)
    tg, tb = torch.from_numpy(g64.copy()).requires_grad_(True), torch.from_numpy(inp["beta"].astype(f64)).requires_grad_(True)
    t = torch_bn(ty, None, None, tg, tb)
    t = F.silu(t) if act else t
    (t * torch.from_numpy(dz.astype(f64).T.copy())).sum().backward()
    ref = dict(dy=ty.grad.numpy().T, dgamma=inp["dgamma"].astype(f64) + tg.grad.numpy(), dbeta=inp["dbeta"].astype(f64) + tb.grad.numpy())
    d = dict.fromkeys(ref, 0.0)
    for k, ft in ((0, f32), (1, f32), (0, f64), (1, f64)):             # ft: the finalize arithmetic (FORMS)
        q = bwd_fin_form(seq32(du32)[k], seq32(du32 * y)[k], n, sc, mu, rs, inp["dgamma"], inp["dbeta"], ft)
        full = dict(dy=[dy_form(du32, y, sc, q["k2"].astype(f32), q["k3"].astype(f32), f32, fma) for fma in (False, True)], dgamma=[q["dgamma"].astype(f32)],
                    dbeta=[q["dbeta"].astype(f32)])
        d = {kk: max(d[kk], d32_max(full[kk], ref[kk])) for kk in ref}
    violation(out["dy"], ref["dy"], tol(ref["dy"], d["dy"], dt), "dy end to end", tag + "bwd end to end", bad)
    violation(out["dgamma"], ref["dgamma"], 8 * d["dgamma"], "dgamma end to end", tag + "bwd end to end", bad)
    violation(out["dbeta"], ref["dbeta"], 8 * d["dbeta"], "dbeta end to end", tag + "bwd end to end", bad)
    return bad


def bwd_emulate(c, inp):
    dt, act, n = c["dtype"], c["act"], c["rows"]
    y, dz = inp["y"], inp["dz"]
    sc, sh, mu, rs = inp["coef"]
    du32 = du_form(dz, y, sc, sh, act, f32)
    nb = max(1, min(768, -(-n // 64)))
    part = np.stack([lane_partials(du32, nb), lane_partials(du32 * y, nb)], axis=1)
    q = bwd_fin_form(part[:, 0].astype(f64).sum(0), part[:, 1].astype(f64).sum(0), n, sc, mu, rs, 0 * sc, 0 * sc, f64)
    s2, s1 = q["dgamma"], q["dbeta"]
    m1, m2 = (s1 / n).astype(f32), (s2 / n).astype(f32)
    k2, k3 = sc * (m1 - mu * rs * m2), sc * rs * m2
    return dict(part=part, dgamma=inp["dgamma"] + s2.astype(f32), dbeta=inp["dbeta"] + s1.astype(f32), k23=np.stack([k2, k3]),
                dy=store(dy_form(du32, y, sc, k2, k3, f32), dt), rg=None if inp["rg"] is None else store(inp["rg"] + dz, dt))


def bwd_emulation_msgs(c, inp):
    return bwd_violations(c, inp, bwd_emulate(c, inp), "emulation ")


BWD_CASES = [
    Bw("bf16", 80, 1003, rg=True, dzv=(8, 16), rgv=(16, 8), regimes=True),
    Bw("f32", 24, 333, rg=True, dzv=(4, 8), rgv=(0, 4), regimes=True),
    Bw("bf16", 8, 700, dzv=(0, 8)),
    Bw("f32", 4, 100, act=0, rg=True, rgv=(4, 4)),
    Bw("bf16", 2048, 37, act=0, rg=True, rgv=(8, 0)),
    Bw("f32", 1024, 13, dzv=(4, 0)),
    Bw("bf16", 16, 1, rg=True, dzv=(8, 8), rgv=(8, 8)),
    Bw("f32", 8, 1, act=0),
    Bw("f32", 32, 1999, rg=True, dzv=(4, 4), rgv=(8, 4), regimes=True),
    Bw("bf16", 32, 1999, act=0, rg=True, dzv=(8, 40), rgv=(0, 16), regimes=True),
    Bw("bf16", 16, 7, regimes=True),
    Bw("f32", 16, 5, regimes=True, rg=True, rgv=(0, 12)),
]
BWD_KEYS = ("dy", "k23", "dgamma", "dbeta", "rg", "part")


def bid(c):
    return "%s-C%d-r%d-act%d-rg%d" % (c["dtype"], c["C"], c["rows"], c["act"], int(c["rg"]))


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("case", BWD_CASES, ids=bid)
def test_bn_backward_kernels(backend, engine, case):
    """chan_reduce_kernel MODE 0 (with and without the rg add and SiLU) -> chan_finalize_kernel -> bn_bwd_apply_kernel; mode 1 moves the rg add into the apply
    pass: the same numbers bit for bit."""
    c = case
    inp = drawn("bwd", c, bwd_inputs, bwd_emulation_msgs)
    outs = []
    for mode in (0, 1):
        st, (out,) = engine.bn_train_bwd([bwd_problem(c, inp)], mode, act=c["act"], dtype=c["dtype"])
        assert st == 0 and out["view_intact"] == 1, (mode, st, out["view_intact"])
        st, (again,) = engine.bn_train_bwd([bwd_problem(c, inp)], mode, act=c["act"], dtype=c["dtype"])
        assert st == 0 and same_outputs(out, again, BWD_KEYS), "mode %d: two consecutive calls differ" % mode
        outs.append(out)
    bad = bwd_violations(c, inp, outs[0], "")
    assert not bad, "; ".join(bad)
    assert same_outputs(outs[0], outs[1], BWD_KEYS), "the rg add in the apply pass changes a result"


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("n", [1, 2, 9])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_bn_backward_group_matches_single_launches(backend, engine, dtype, n):
    """chan_finalize_group_kernel + bn_bwd_apply_group_kernel (which carries rg) over n problems against mode 1 of each problem."""
    epl = 8 if dtype == "bf16" else 4
    cs = [Bw(dtype, f["C"], f["rows"], rg=bool(i % 2), dzv=(epl * (i % 3), epl * (i % 2)), rgv=(epl, epl * (i % 4)), seed=20 + i) for i, f in enumerate(group_problems(dtype, n))]
    inps = [bwd_inputs(c, c["seed"]) for c in cs]
    for act in (1, 0):
        st, outs = engine.bn_train_bwd([bwd_problem(c, i) for c, i in zip(cs, inps)], 2, act=act, dtype=dtype)
        assert st == 0
        for c, i, o in zip(cs, inps, outs):
            st, (single,) = engine.bn_train_bwd([bwd_problem(c, i)], 1, act=act, dtype=dtype)
            assert st == 0 and o["view_intact"] == 1
            assert same_outputs(o, single, BWD_KEYS), "problem C=%d rows=%d differs from its single launch" % (c["C"], c["rows"])
    bad = [m for c, i, o in zip(cs, inps, outs) for m in bwd_violations(dict(c, act=0), i, o, "group ")]
    assert not bad, "; ".join(bad)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("nsrc", [2, 3])
def test_bn_backward_finalize_from_several_sources(backend, engine, nsrc):
    """chan_finalize_kernel with a multi-source FinSrc: channel c reads the partial rows of the source that covers it -- boundaries at channel 8 and C - 8, sources
    with 1 and with many rows; the rows of the OTHER sources hold a value that ruins any channel read from the wrong one."""
    C, n = 40, 500
    rng = np.random.default_rng(nsrc)
    bounds = [8, C] if nsrc == 2 else [8, C - 8, C]
    nblks = [1, 300] if nsrc == 2 else [300, 1, 17]
    sc, mu, rs = rng.uniform(0.5, 2, C).astype(f32), rng.standard_normal(C).astype(f32), rng.uniform(0.5, 2, C).astype(f32)
    coef = np.stack([sc, 0 * sc, mu, rs])
    g0, g1 = rng.standard_normal(C).astype(f32), rng.standard_normal(C).astype(f32)
    src, P1, P2, lo = [], np.zeros(C), np.zeros(C), 0
    for nb, hi in zip(nblks, bounds):
        p = np.full((nb, 2, C), 1e6, f32)
        p[:, :, lo:hi] = rng.standard_normal((nb, 2, hi - lo))
        P1[lo:hi], P2[lo:hi] = p[:, 0, lo:hi].astype(f64).sum(0), p[:, 1, lo:hi].astype(f64).sum(0)
        src.append((p, hi))
        lo = hi
    st, (out,) = engine.bn_train_bwd([dict(coef=coef, dgamma=g0, dbeta=g1, rows=n, src=src)], 3)
    assert st == 0 and out["view_intact"] == 1
    r64, r32 = bwd_fin_form(P1, P2, n, sc, mu, rs, g0, g1, f64), bwd_fin_form(P1, P2, n, sc, mu, rs, g0, g1, f32)
    got, bad = dict(dgamma=out["dgamma"], dbeta=out["dbeta"], k2=out["k23"][0], k3=out["k23"][1]), []
    for k in got:
        violation(got[k], r64[k], 8 * d32_of(r32[k], r64[k]), k, "bwd FinSrc finalize", bad)
    assert not bad, "; ".join(bad)
    st, (again,) = engine.bn_train_bwd([dict(coef=coef, dgamma=g0, dbeta=g1, rows=n, src=src)], 3)
    assert st == 0 and same_outputs(out, again, ("k23", "dgamma", "dbeta"))


# ------------------------------------------------------------------ column sums, up-sample, view copy
COLSUM_CASES = [("bf16", 2, 65, 150, 150, 8, 8), ("bf16", 3, 65, 100, 140, 0, 16), ("f32", 2, 7, 333, 400, 4, 4), ("f32", 1, 144, 50, 50, 0, 8),
                ("bf16", 2, 80, 1, 3, 8, 0), ("f32", 4, 1, 499, 500, 0, 4)]


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("case", COLSUM_CASES, ids=lambda c: "%s-B%d-C%d-r%d-bs%d" % c[:5])
def test_colsum(backend, engine, case):
    """chan_reduce_kernel MODE 1 + chan_finalize_kernel MODE 1: a view with coff != 0, dense and with rows_per_b < bstride (the rows between the images hold the
    sentinel), C not a multiple of the vector over zeroed padding channels; grad accumulates."""
    dtype, B, C, rpb, bstride, ld_pad, coff = case
    rng = np.random.default_rng(C + rpb)
    x = store(rng.standard_normal((B, C, rpb)) + rng.standard_normal((1, C, 1)), dtype)
    g0 = rng.standard_normal(C).astype(f32)
    st, g, ok = engine.colsum(x, g0, bstride=bstride, ld_pad=ld_pad, coff=coff, dtype=dtype)
    assert st == 0 and ok == 1
    cols = np.ascontiguousarray(x.transpose(1, 0, 2).reshape(C, B * rpb))
    ref = g0.astype(f64) + cols.astype(f64).sum(1)
    d = max(d32_of(g0 + s, ref) for s in seq32(cols))
    bad = []
    violation(g, ref, 8 * d, "grad", "column sums", bad)
    assert not bad, "; ".join(bad)
    st, g2, ok = engine.colsum(x, g0, bstride=bstride, ld_pad=ld_pad, coff=coff, dtype=dtype)
    assert st == 0 and ok == 1 and np.array_equal(g, g2)


UPS_CASES = [("bf16", 2, 3, 5, 16, (24, 8, 32, 16)), ("f32", 1, 4, 4, 8, (12, 4, 8, 0)), ("bf16", 1, 1, 1, 8, (8, 0, 16, 8)), ("f32", 3, 7, 2, 20, (24, 4, 28, 8)),
             ("bf16", 1, 9, 6, 40, (40, 0, 48, 0))]


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("case", UPS_CASES, ids=lambda c: "%s-B%d-%dx%d-C%d" % c[:5])
def test_upsample2x(backend, engine, case):
    """upsample2x_fwd_kernel exactly; upsample2x_bwd_kernel (2 x 2 sum, accumulate 0 and 1) within the bounds; both operands in padded views."""
    dtype, B, H, W, C, views = case
    rng = np.random.default_rng(H * W + C)
    x = store(rng.standard_normal((B, C, H * W)), dtype)
    st, up, ok = engine.upsample2x(x, H, W, views=views, dtype=dtype)
    ref = np.repeat(np.repeat(x.reshape(B, C, H, W), 2, axis=2), 2, axis=3).reshape(B, C, 4 * H * W)
    assert st == 0 and ok == 1 and np.array_equal(up, ref)
    dy = store(rng.standard_normal((B, C, 4 * H * W)), dtype)
    dx0 = store(rng.standard_normal((B, C, H * W)), dtype)
    q = dy.reshape(B, C, H, 2, W, 2)
    quad = [q[:, :, :, a, :, b].reshape(B, C, H * W) for a in (0, 1) for b in (0, 1)]
    bviews = (views[2], views[3], views[0], views[1])
    for acc in (0, 1):
        terms = quad + ([dx0] if acc else [])
        r64 = sum(t.astype(f64) for t in terms)
        fwd = terms[0].copy()
        for t in terms[1:]:
            fwd = fwd + t
        rev = terms[-1].copy()
        for t in terms[-2::-1]:
            rev = rev + t
        d = max(d32_of(fwd, r64), d32_of(rev, r64))
        st, dx, ok = engine.upsample2x(dy, H, W, backward=True, views=bviews, dst=dx0 if acc else None, dtype=dtype)
        assert st == 0 and ok == 1
        bad = []
        violation(dx, r64, tol(r64, d, dtype), "dx accumulate=%d" % acc, "upsample2x backward", bad)
        assert not bad, "; ".join(bad)
        st, dx2, ok = engine.upsample2x(dy, H, W, backward=True, views=bviews, dst=dx0 if acc else None, dtype=dtype)
        assert st == 0 and np.array_equal(dx, dx2)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("case", [("bf16", 16, 300, (24, 8, 32, 16)), ("f32", 24, 77, (28, 4, 24, 0)), ("bf16", 8, 1, (8, 0, 16, 8)), ("f32", 4, 1000, (8, 4, 12, 8))],
                         ids=lambda c: "%s-C%d-r%d" % c[:3])
def test_copy_view(backend, engine, case):
    """copy_view_kernel: exact without accumulate; dst + src with one rounding with it."""
    dtype, C, rows, views = case
    rng = np.random.default_rng(C + rows)
    src, dst0 = store(rng.standard_normal((C, rows)), dtype), store(rng.standard_normal((C, rows)), dtype)
    st, out, ok = engine.copy_view(src, views=views, dtype=dtype)
    assert st == 0 and ok == 1 and np.array_equal(out, src)
    st, out, ok = engine.copy_view(src, views=views, dst=dst0, dtype=dtype)
    r64 = src.astype(f64) + dst0.astype(f64)
    bad = []
    violation(out, r64, tol(r64, d32_of(src + dst0, r64), dtype), "dst + src", "copy_view accumulate", bad)
    assert st == 0 and ok == 1 and not bad, "; ".join(bad)
    st, out2, ok = engine.copy_view(src, views=views, dst=dst0, dtype=dtype)
    assert st == 0 and np.array_equal(out, out2)


# ------------------------------------------------------------------ the statistics of a convolution's own epilogue, both paths
CONV_CASES = [(2, 16, 12, 12, 32, 3, 1), (1, 48, 8, 8, 24, 1, 1), (2, 80, 19, 13, 80, 3, 1), (1, 128, 9, 11, 80, 3, 2), (2, 128, 17, 16, 128, 3, 1)]


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("case", CONV_CASES, ids=lambda c: "x".join(map(str, c)))
def test_conv_epilogue_statistics(backend, engine, dtype, case):
    """ys_conv_bn_act_fwd_ex on the patch, 1x1, streamed-weight, blocked-GEMM and halo kernels: the coefficients of both statistics paths against the float64
    statistics of the convolution output the entry returns (the accumulator path with its P 2^-21 terms, P = the returned row count), z against the returned
    coefficients, and two consecutive calls bit-identical (accumulators that are not cleared between calls add up)."""
    conv_epilogue_statistics(engine, dtype, case, (1, 0))


# the fp8 kernels' statistics epilogue sums y = acc / (s_x s_w) AFTER that rescale (statistics of the raw accumulator would be off by the factor BatchNorm mostly
# hides): one conv_p2_kernel<F8> and one conv_gemm_kernel<F8 = 1> shape of tests/test_fp8_kernels.py, statistics rows only (the mode the fp8 path keeps)
F8_CONV_CASES = [((2, 96, 12, 12, 72, 3, 1), "p2f8"), ((1, 160, 9, 11, 80, 3, 2), "gemmf8")]


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("case", F8_CONV_CASES, ids=lambda c: c[1])
def test_conv_epilogue_statistics_fp8(backend, engine, case):
    """test_conv_epilogue_statistics with dtype "fp8", at its bf16 bounds; the kernel asserted from the per-launch profile."""
    (B, Cin, H, W, Cout, k, s), kern = case
    _, labels = engine.conv_labels(lambda: conv_epilogue_statistics(engine, "fp8", case[0], (0,)))
    assert len(labels) == 2 and all(l.startswith("%s k%d s%d div1 cin%d cout%d " % (kern, k * 11, s, Cin, Cout)) for l in labels), labels


def conv_epilogue_statistics(engine, dtype, case, modes):
    B, Cin, H, W, Cout, k, s = case
    rng = np.random.default_rng(Cin + Cout)
    x = rng.standard_normal((B, Cin, H, W)).astype(f32)
    w = (rng.standard_normal((Cout, Cin, k, k)) / np.sqrt(Cin * k * k)).astype(f32)
    g, bt = rng.uniform(0.5, 1.5, Cout).astype(f32), (0.1 * rng.standard_normal(Cout)).astype(f32)
    rm0, rv0 = (0.1 * rng.standard_normal(Cout)).astype(f32), rng.uniform(0.5, 1.5, Cout).astype(f32)
    names = ("scale", "shift", "mean", "rstd")
    for mode in modes:
        runs = []
        for _ in range(2):
            bn = dict(weight=g, bias=bt, running_mean=rm0.copy(), running_var=rv0.copy())
            ex = {}
            z = engine.conv_bn_act(x, w, k, s, bn=bn, act=True, training=True, dtype=dtype, stat_mode=mode, extras=ex)
            runs.append((z, ex["y_raw"], ex["coef"], bn["running_mean"], bn["running_var"]))
        assert all(np.array_equal(a, b) for a, b in zip(*runs)), "stat_mode %d: two consecutive calls differ" % mode
        z, y_raw, coef, rm, rv = runs[0]
        store_dt = "bf16" if dtype == "fp8" else dtype       # the storage type: the fp8 path is held to the bf16 bounds
        y = np.ascontiguousarray(y_raw.transpose(1, 0, 2, 3).reshape(Cout, -1))
        n = y.shape[1]
        y64 = y.astype(f64)
        S1, S2 = y64.sum(1), (y64 * y64).sum(1)
        r64 = coef_form(S1, S2, n, g, bt, rm0, rv0, f64)
        extra = acc_terms(S1, S2, n, g, ex["stat_rows"]) if mode == 1 else dict.fromkeys(names + ("run_mean", "run_var"), 0.0)
        d = dict.fromkeys(r64, 0.0)
        for o in range(2):
            q = coef_form(seq32(y)[o], seq32(y * y)[o], n, g, bt, rm0, rv0, f32)
            d = {kk: max(d[kk], d32_of(q[kk], r64[kk])) for kk in r64}
        bad, path = [], ("fp8 " if dtype == "fp8" else "") + ("convolution accumulators" if mode == 1 else "convolution statistics rows")
        for kk, got in zip(names + ("run_mean", "run_var"), list(coef) + [rm, rv]):
            violation(got, r64[kk], 8 * d[kk] + extra[kk], kk, path, bad)
        zt = np.ascontiguousarray(z.transpose(1, 0, 2, 3).reshape(Cout, -1))
        z64 = apply_form(y, coef[0], coef[1], None, 1, f64)
        violation(zt, z64, tol(z64, d32_max([apply_form(y, coef[0], coef[1], None, 1, f32, fma) for fma in (False, True)], z64), store_dt), "z", path + " apply", bad)
        assert not bad, "stat_mode %d: %s" % (mode, "; ".join(bad))


# ------------------------------------------------------------------ the bounds themselves, on the CPU
def test_bounds_hold_for_an_emulation_of_the_rounding_points():
    """Every forward and backward case: an emulation of the kernels' rounding points stays inside the bounds the engine is held to (inputs redrawn up to
    SEED_TRIES times, as for the engine tests, which then use the draw that passed)."""
    for c in FWD_CASES:
        drawn("fwd", c, fwd_inputs, fwd_emulation_msgs)
    for c in BWD_CASES:
        drawn("bwd", c, bwd_inputs, bwd_emulation_msgs)


def test_bounds_reject_a_dropped_row_and_a_wrong_k2():
    """The checks can fail: an emulation that drops the last row of the reduction, or that forgets `- mean * sum(du)`, is outside."""
    c = dict(FWD_CASES[0], res=False)
    inp = fwd_inputs(c, c["seed"])
    out = fwd_emulate(c, dict(inp, y=np.ascontiguousarray(inp["y"][:, :-1])), 0)
    out["z"] = np.concatenate([out["z"], out["z"][:, -1:]], axis=1)
    assert fwd_violations(c, inp, out, 0, "negative ")
    b = BWD_CASES[0]
    binp = bwd_inputs(b, b["seed"])
    wrong = bwd_emulate(b, dict(binp, coef=np.stack([binp["coef"][0], binp["coef"][1], 0 * binp["coef"][2], binp["coef"][3]])))
    assert bwd_violations(b, binp, wrong, "negative ")
