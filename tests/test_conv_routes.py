"""Which kernels a convolution runs on, per route of conv_route (csrc/conv.hip): every launch of one public call -- forward with training statistics,
backward, fp8 forward, fp8 input gradient -- as its (class, label) pair of the per-launch profile, in launch order per class, against a recording.  The labels
carry the kernel family, the variant and the grid, so they pin the route; one case per branch of the routing.

tests/golden/conv_routes.json was recorded by THIS test body (`python tests/test_conv_routes.py --record emu|gpu [file]`) at commit 2951f29, the last one whose
launch and its four row / route queries were separate hand-written decision trees.  It is never regenerated from a tree whose routing is in question: a pull
request that moves a launch on purpose re-records it and says so.  Layout: {case: {"emu": [[class, label], ...], "gpu": [...]}}.

For the cases that take training statistics the row count the call reports (ys_conv_grid_m sized the statistics rows with it) must be the number of rows the
launch named by the label writes: one per workgroup, or per tile / pixel block for the two dtype-generic kernels."""
import ctypes as C
import json
import os
import re
import sys
import tempfile

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":
    sys.path[:0] = [os.path.dirname(HERE), HERE]

from conftest import BACKENDS

GOLDEN = os.path.join(HERE, "golden", "conv_routes.json")
# the size gates tests/conftest.py lowers for the whole suite, stated here because the routes below depend on them
GATES = dict(F8_MIN_CIN=32, F8_MIN_TAPS=1, GEMM_MIN_M=1, HALO_MIN_FILL=1)
# name: (call, dtype, (B, Cin, H, W, Cout, k, s), options) -- shapes from the tables of test_conv.py, test_fp8.py and test_fp8_kernels.py
CASES = {
    "f32_3x3_s1_chunked_patch":        ("fwd", "f32", (2, 16, 12, 12, 32, 3, 1), {}),
    "f32_1x1_generic":                 ("fwd", "f32", (1, 48, 8, 8, 24, 1, 1), {}),
    "f32_3x3_s2_generic":              ("fwd", "f32", (1, 16, 9, 11, 16, 3, 2), {}),
    "bf16_p2_3x3_s1":                  ("fwd", "bf16", (2, 32, 20, 40, 48, 3, 1), {}),
    "bf16_p2_1x1":                     ("fwd", "bf16", (1, 48, 8, 8, 24, 1, 1), {}),
    "bf16_p2_3x3_s2":                  ("fwd", "bf16", (2, 16, 18, 36, 16, 3, 2), {}),
    "bf16_3x3_cin320_cout48_off_p2":   ("fwd", "bf16", (1, 320, 8, 8, 48, 3, 1), {}),
    "bf16_halo_128_160":               ("fwd", "bf16", (1, 128, 12, 12, 160, 3, 1), {}),
    "bf16_gemm_3x3_s2":                ("fwd", "bf16", (1, 128, 9, 11, 80, 3, 2), {}),
    "bf16_gemm_1x1":                   ("fwd", "bf16", (1, 256, 13, 10, 128, 1, 1), {}),
    "f32_bwd_3x3_s2":                  ("bwd", "f32", (1, 32, 9, 7, 80, 3, 2), {}),
    "bf16_bwd_3x3_s1_p2":              ("bwd", "bf16", (2, 16, 8, 8, 32, 3, 1), {}),
    "bf16_bwd_s2_phases_grouped":      ("bwd", "bf16", (1, 64, 14, 10, 128, 3, 2), {}),
    "bf16_bwd_s2_phases_ungrouped":    ("bwd", "bf16", (1, 64, 14, 10, 128, 3, 2), {"GROUP": 0}),
    "bf16_bwd_s2_phases_on_gemm":      ("bwd", "bf16", (1, 64, 14, 10, 192, 3, 2), {}),
    "f8_p2_resident":                  ("f8fwd", "fp8", (2, 64, 12, 12, 64, 3, 1), {}),
    "f8_p2_streamed_320_48":           ("f8fwd", "fp8", (1, 320, 8, 8, 48, 3, 1), {}),
    "f8_gemm_quantised_first_320_96":  ("f8fwd", "fp8", (1, 320, 8, 8, 96, 3, 1), {}),
    "f8_gemm_1x1":                     ("f8fwd", "fp8", (1, 256, 13, 10, 128, 1, 1), {}),
    "f8_declined_min_taps_1x1_gemm":   ("f8fwd", "fp8", (1, 256, 13, 10, 128, 1, 1), {"F8_MIN_TAPS": 4}),
    "f8_declined_min_taps_1x1_p2":     ("f8fwd", "fp8", (2, 32, 9, 11, 40, 1, 1), {"F8_MIN_TAPS": 4}),
    "f8_refused_min_cin_64":           ("f8fwd", "fp8", (2, 64, 12, 12, 64, 3, 1), {"F8_MIN_CIN": 128}),
    "f8_dgrad_e5m2_gemm":              ("f8dgrad", "fp8", (1, 64, 11, 13, 160, 3, 1), {}),
    "f8_dgrad_e5m2_p2":                ("f8dgrad", "fp8", (2, 64, 12, 12, 64, 3, 1), {}),
    "f8_dgrad_s2_mixed_phases":        ("f8dgrad", "fp8", (1, 64, 14, 10, 192, 3, 2), {}),
    "f8_dgrad_s2_p2_phases":           ("f8dgrad", "fp8", (2, 128, 9, 11, 128, 3, 2), {}),
    "f8_bwd_cout80_falls_to_bf16":     ("f8bwd", "fp8", (1, 256, 6, 6, 80, 1, 1), {}),
}


def run_case(engine, name):
    """-> ([[class, label], ...] of every launch of the call, the statistics rows it reported or None)"""
    from yolosharp_amd import _lib
    call, dtype, (B, Cin, H, W, Cout, k, s), opts = CASES[name]
    rng = np.random.default_rng(len(name) + Cin + Cout)
    x = rng.standard_normal((B, Cin, H, W), dtype=np.float32)
    w = rng.standard_normal((Cout, Cin, k, k), dtype=np.float32) / np.float32((Cin * k * k) ** 0.5)
    Ho, Wo = (H + 2 * (k // 2) - k) // s + 1, (W + 2 * (k // 2) - k) // s + 1
    dy = rng.standard_normal((B, Cout, Ho, Wo), dtype=np.float32) * np.float32(1e-3)
    bn = lambda: dict(weight=np.ones(Cout, np.float32), bias=np.zeros(Cout, np.float32), running_mean=np.zeros(Cout, np.float32), running_var=np.ones(Cout, np.float32))
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    rows = None
    with engine.options(**dict(GATES, **opts)):
        engine.kernel_profile(True)
        try:
            if call == "fwd":
                extras = {}
                engine.conv_bn_act(x, w, k, s, bn=bn(), act=True, training=True, dtype=dtype, stat_mode=0, extras=extras)
                rows = extras["stat_rows"]
            elif call == "f8fwd":
                rows = engine.conv_f8_fwd(x, w, k, s, bn=bn(), act=True, training=True)["stat_rows"]
            elif call == "f8dgrad":
                engine.conv_f8_dgrad((B, Cin, H, W), w, k, s, dy)
            else:
                dx, dw = np.zeros_like(x), np.zeros_like(w)
                _lib.check(engine.lib, engine.lib.ys_conv_bwd(engine.ctx, {"f32": 0, "bf16": 1, "fp8": 2}[dtype], vp(x), B, Cin, H, W, vp(w), Cout, k, s, vp(dy), vp(dx), vp(dw)))
            engine.synchronize()
            fd, path = tempfile.mkstemp(suffix=".csv")
            os.close(fd)
            try:
                engine.kernel_profile_dump(path)
                lines = open(path).read().splitlines()
            finally:
                os.remove(path)
        finally:
            engine.kernel_profile(False)
    assert lines[0] == "class,label,us"
    return [[l.split(",", 1)[0], l.split(",", 1)[1].rsplit(",", 1)[0]] for l in lines[1:]], rows


def rows_of_label(label, case):
    """Statistics rows the launch named by a conv_igemm label writes."""
    B, Cin, H, W, Cout, k, s = case
    Ho, Wo = (H + 2 * (k // 2) - k) // s + 1, (W + 2 * (k // 2) - k) // s + 1
    fam = label.split()[0]
    if fam in ("p2", "p2f8", "gemm", "gemmf8", "halo"):              # persistent grids: one row per workgroup column
        return int(re.search(r" grid(\d+)x\d+", label).group(1))
    if fam == "patch":                                               # one row per tile
        th, tw = map(int, re.search(r" tile(\d+)x(\d+) ", label).groups())
        return B * -(-Ho // th) * -(-Wo // tw)
    assert fam == "direct", label                                    # one row per block of 64 * mr pixels
    return -(-(B * Ho * Wo) // (64 * int(re.search(r" mr(\d+) ", label).group(1))))


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("name", list(CASES))
def test_conv_route_matches_the_recorded_one(backend, engine, name):
    want = json.load(open(GOLDEN))[name][backend]
    got, rows = run_case(engine, name)
    assert got == want, "\n".join(["launches now:"] + ["  %s  %s" % tuple(g) for g in got] + ["recorded:"] + ["  %s  %s" % tuple(g) for g in want])
    if rows is not None:
        conv = [label for cls, label in got if cls == "conv_igemm"]
        assert len(conv) == 1, conv
        assert rows == rows_of_label(conv[0], CASES[name][2]), (rows, conv[0])


if __name__ == "__main__":
    # --record emu|gpu [file]: (re)write that backend's entries of the golden (or of `file`, which starts as a copy of the golden) from the tree this runs in
    assert len(sys.argv) in (3, 4) and sys.argv[1] == "--record" and sys.argv[2] in ("emu", "gpu"), "usage: test_conv_routes.py --record emu|gpu [file]"
    from yolosharp_amd import Engine, build as build_mod
    eng = Engine(lib_path=build_mod.build_emu()) if sys.argv[2] == "emu" else Engine()
    gold = json.load(open(GOLDEN)) if os.path.exists(GOLDEN) else {}
    for c in CASES:
        gold.setdefault(c, {})[sys.argv[2]] = run_case(eng, c)[0]
    with open(sys.argv[3] if len(sys.argv) == 4 else GOLDEN, "w") as f:
        f.write("{\n" + ",\n".join(json.dumps(c) + ": {" + ",\n  ".join(json.dumps(b) + ": " + json.dumps(gold[c][b]) for b in sorted(gold[c])) + "}" for c in CASES) + "\n}\n")
