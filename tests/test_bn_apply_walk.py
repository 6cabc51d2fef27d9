"""The grid-stride loops of bn_fin_apply_kernel, bn_act_apply_q8_kernel and bn_bwd_apply_q8_kernel (csrc/batchnorm.hip) walk (row, channel vector) incrementally:
divided once for the thread's first vector, then advanced by (stride / CG, stride % CG) with a carry.  The walk can only go wrong where the stride is not a multiple of
CG and a thread makes several trips, so the shapes here have C = 24 or 48 (CG = 3, 6 in bf16 and 6, 12 in f32) and enough rows for two to four trips -- up to the
bounded grid of 2048 workgroups, where the stride is 2^19 vectors -- plus the single-trip shape with a ragged only workgroup.  References and bounds are those of
tests/test_bn_kernels.py (forward, production statistics path) and tests/test_fp8_kernels.py (the quantising passes), called unchanged.

  kernel                 vectors per thread   shape (rows x C)        vectors    workgroups   stride mod CG   trips
  bn_fin_apply bf16      2                    1700 x 24               5100       10           1               2
  bn_fin_apply f32       2                    900 x 24                5400       11           2               2
  bn_fin_apply bf16      2                    100001 x 48             600006     1172         2               2, rows * CG beyond 2048 x 256 threads
  bn_fin_apply f32       2                    175001 x 24             1050006    2048 (cap)   2               3, the last one ragged
  bn_fin_apply bf16      2                    50 x 24                 150        1            --              1, 150 of 256 threads
  q8 forward / backward  4                    1700 x 24               5100       5            2               4
  q8 forward / backward  4                    180400 x 24             541200     529          1               4, rows * CG beyond 2048 x 256 threads
  q8 forward / backward  4                    50 x 48                 300        1            4               2, ragged
  q8 forward / backward  4                    30 x 24                 90         1            --              1, 90 of 256 threads
"""
import pytest

from conftest import BACKENDS
import test_bn_kernels as K
import test_fp8_kernels as F8

FWD_CASES = [
    K.Fw("bf16", 24, 1700, res=True, z=(8, 16), rv=(16, 8), P=8, seed=1),
    K.Fw("f32", 24, 900, res=True, z=(4, 8), rv=(0, 40), share=1, P=9, seed=2),
    K.Fw("bf16", 48, 100001, act=1, z=(8, 8), P=8, seed=3),
    K.Fw("f32", 24, 175001, act=1, res=True, rv=(4, 4), P=8, seed=4),
    K.Fw("bf16", 24, 50, res=True, z=(0, 8), rv=(8, 0), P=1, seed=5),
]


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("case", FWD_CASES, ids=K.fid)
def test_bn_fin_apply_walk(backend, engine, case):
    """ys_bn_train_fwd on the production statistics path (mode 1: ys_stat_acc_add -> bn_fin_apply_kernel) against float64, twice with identical outputs."""
    c = case
    inp = K.fwd_inputs(c, c["seed"])
    st, (out,) = engine.bn_train_fwd([K.fwd_problem(c, inp, 1)], 1, act=c["act"], dtype=c["dtype"])
    assert st == 0 and out["view_intact"] == 1
    bad = K.fwd_violations(c, inp, out, 1, "")
    assert not bad, "; ".join(bad)
    st, (again,) = engine.bn_train_fwd([K.fwd_problem(c, inp, 1)], 1, act=c["act"], dtype=c["dtype"])
    assert st == 0 and K.same_outputs(out, again, K.FWD_KEYS), "two consecutive calls differ"


Q8_SHAPES = [(1700, 24), (180400, 24), (50, 48), (30, 24)]


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("res", [None, "view"])
@pytest.mark.parametrize("shape", Q8_SHAPES, ids=lambda s: "%dx%d" % s)
def test_bn_apply_q8_forward_walk(backend, engine, shape, res):
    F8.test_bn_apply_q8_forward(backend, engine, shape, 1, res)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("rg", [False, True])
@pytest.mark.parametrize("shape", Q8_SHAPES, ids=lambda s: "%dx%d" % s)
def test_bn_apply_q8_backward_walk(backend, engine, shape, rg):
    F8.test_bn_apply_q8_backward(backend, engine, shape, 1, rg)
