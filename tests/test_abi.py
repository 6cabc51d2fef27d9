"""The C-ABI library loads and exports exactly the symbols include/yolosharp_hip.h declares (no compute calls)."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    txt = open(os.path.join(ROOT, "include", "yolosharp_hip.h")).read()
    return sorted(set(re.findall(r"YS_API\s+[\w\s\*]+?\b(ys_\w+)\s*\(", txt)))


def exported_ys_symbols(path):
    """The defined dynamic symbols matching ^ys_ of a shared library: llvm-readelf --dyn-syms of the ROCm toolchain, nm -D --defined-only where that is absent."""
    readelf = "/opt/rocm/lib/llvm/bin/llvm-readelf"
    if os.path.exists(readelf):
        out = subprocess.run([readelf, "--dyn-syms", "-W", path], check=True, stdout=subprocess.PIPE, text=True).stdout
        # Num: Value Size Type Bind Vis Ndx Name -- Ndx UND = imported, not exported
        rows = [l.split() for l in out.splitlines()]
        names = [r[7] for r in rows if len(r) >= 8 and r[0].endswith(":") and r[6] != "UND" and r[4] in ("GLOBAL", "WEAK")]
    else:
        out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, stdout=subprocess.PIPE, text=True).stdout
        names = [l.split()[-1] for l in out.splitlines() if l.split()]
    return sorted(set(n.split("@")[0] for n in names if re.match(r"^ys_", n)))


def test_header_declares_symbols():
    syms = declared_symbols()
    assert len(syms) >= 35 and "ys_nms_batched" in syms and "ys_model_forward" in syms


def test_device_library_exports_every_declared_symbol():
    from yolosharp_amd import build
    path = build.build_device()           # hipcc cross-compiles for gfx950 without a GPU
    lib = ctypes.CDLL(path)
    missing = [s for s in declared_symbols() if not hasattr(lib, s)]
    assert not missing, missing
    # ... and nothing else: the header IS the boundary (triage hooks live in build/libyolosharp_hip_triage.so only)
    assert exported_ys_symbols(path) == declared_symbols()
    lib.ys_is_device_build.restype = ctypes.c_int
    assert lib.ys_is_device_build() == 1


def test_binding_covers_header():
    from yolosharp_amd import _lib
    assert sorted(_lib.PROTOTYPES) == declared_symbols()


def test_no_cpu_fallback_without_device():
    """The product library must fail loudly when no HIP device exists (this container has none)."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    from yolosharp_amd import Engine, YsError
    with pytest.raises((YsError, OSError)):
        Engine()


def test_missing_library_fails_loudly(tmp_path):
    from yolosharp_amd import _lib
    with pytest.raises(ImportError):
        _lib.load(str(tmp_path / "nope.so"))


def _run_smoke(exe):
    import subprocess
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    return r.returncode, r.stdout + r.stderr


def test_c_consumer_runs_on_interpreter_build():
    """tests/c/abi_smoke.c -- plain C, compiled with -Wall -Wextra -Werror against the public header only -- drives the whole hot
    path (create, state_dict listing, train step, AdamW, eval, NMS) through the same ABI on the test-only interpreter build."""
    from yolosharp_amd import build
    assert exported_ys_symbols(build.build_emu()) == declared_symbols()
    dev, emu = build.build_abi_smoke()
    rc, out = _run_smoke(emu)
    assert rc == 0 and "abi_smoke OK: device_build=0" in out, out
    import torch
    if not torch.cuda.is_available():
        rc, out = _run_smoke(dev)                  # the product library without a device: refuses loudly (exit 77), never a CPU path
        assert rc == 77 and "no HIP device" in out, out


@pytest.mark.gpu
def test_c_consumer_runs_on_device():
    from yolosharp_amd import build
    dev, _ = build.build_abi_smoke()
    rc, out = _run_smoke(dev)
    assert rc == 0 and "abi_smoke OK: device_build=1" in out, out


def test_sentinel_checker_can_say_no():
    """tests/c/sentinel_check.cpp -- a stand-alone host program on csrc/sentinel_check.h alone: the predicate behind every `view_intact` reports a byte changed before a
    view, behind it, between two views of a shared buffer and in the last row, for element sizes 1, 2 and 4 (every other test only ever sees it answer 1)."""
    from yolosharp_amd import build
    r = subprocess.run([build.build_sentinel_check()], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    assert r.returncode == 0 and "sentinel_check OK" in r.stdout, r.stdout


def test_csharp_shim_binds_only_exported_symbols():
    """bindings/csharp/YoloSharpHip.cs (the P/Invoke file a YoloSharp maintainer drops in): every
    `static extern` it declares must be a symbol of the header -- there is no dotnet here to compile it, so at least the names are pinned."""
    txt = open(os.path.join(ROOT, "bindings", "csharp", "YoloSharpHip.cs")).read()
    names = re.findall(r"static\s+extern\s+[\w\[\]]+\s+(ys_\w+)\s*\(", txt)
    assert len(names) >= 40
    declared = set(declared_symbols())
    unknown = [n for n in names if n not in declared]
    assert not unknown, unknown
    for must in ("ys_model_forward", "ys_loss_detect", "ys_model_backward", "ys_optim_adamw_step", "ys_nms_batched", "ys_dist_init"):
        assert must in names, must


def test_options_context_restores_what_was_there(emu_lib_path):
    """Engine.options must put back the PREVIOUS entry of the table, not delete it: tests/conftest.py seeds size gates through the environment at library load
    (YS_GEMM_MIN_M=1 ...), and a test that changed one of them temporarily used to leave the rest of its process on the production gate (round 5: two chaotic
    training-curve checks flipped when a new test ran before them)."""
    import os
    from yolosharp_amd import Engine
    eng = Engine(lib_path=emu_lib_path)
    assert os.environ.get("YS_GEMM_MIN_M") == "1" and eng.get_option("GEMM_MIN_M") == 1.0      # seeded from the environment
    assert eng.get_option("WGEMM_KT") is None
    with eng.options(GEMM_MIN_M=4096, WGEMM_KT=32):
        assert eng.get_option("GEMM_MIN_M") == 4096.0 and eng.get_option("YS_WGEMM_KT") == 32.0
        with eng.options(GEMM_MIN_M=7):
            assert eng.get_option("GEMM_MIN_M") == 7.0
        assert eng.get_option("GEMM_MIN_M") == 4096.0
    assert eng.get_option("GEMM_MIN_M") == 1.0 and eng.get_option("WGEMM_KT") is None
    # round 6: the keys are a registered list -- a typo is an error, not a silent no-op, and leaves the table untouched
    with pytest.raises(Exception) as ei:
        eng.set_option("NO_SUCH_KEY_R06", 3)
    assert "unknown key" in str(ei.value)
    assert eng.get_option("NO_SUCH_KEY_R06") is None
