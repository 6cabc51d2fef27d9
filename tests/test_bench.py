"""bench.py's own contract: a plain run prints the headline line and nothing it had to measure separately; --dump-outputs writes what the
last timed step computed; --steps sets the number of timed steps."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def test_bench_rejects_bad_arguments():
    """No GPU needed: argument checks run before anything is set up."""
    for args, msg in ((["--steps", "0"], "--steps must be >= 1"), (["--dump-launches", "x.csv"], "add --full")):
        r = subprocess.run([sys.executable, BENCH] + args, capture_output=True, text=True, timeout=120)
        assert r.returncode == 2 and msg in r.stderr, (args, r.returncode, r.stderr[-500:])


@pytest.mark.gpu
def test_plain_run_and_dump_outputs(tmp_path):
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, BENCH, "--steps", "3", "--warmup", "1", "--batch", "8", "--dump-outputs", str(out)],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in line, k
    assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0 and line["value"] > 0
    assert not any(k in line for k in ("roofline", "infer", "nms", "cpu_baseline", "dist")), sorted(line)
    files = sorted(os.listdir(out))
    assert files == ["boxes.npy", "loss_items.npy", "scores.npy", "state.npy"], files
    assert sum(os.path.getsize(out / f) for f in files) <= 64 << 20
    d = {f[:-4]: np.load(out / f) for f in files}
    assert all(a.dtype == np.float32 and np.all(np.isfinite(a)) for a in d.values())
    assert np.allclose(d["loss_items"], line["loss_items"], rtol=1e-4)
    assert d["boxes"].size == 8 * 64 * 8400 and d["scores"].size == 8 * 80 * 8400        # below the per-array cap: whole arrays
    assert d["state"].size > 3_000_000                                                     # YOLOv8n parameters + BatchNorm statistics
