"""YOLOv5u-n train / eval throughput on one device and the cost of its first layer on both routes: prints ONE JSON line.

  python tools/v5u_bench.py [--batch 64] [--size 640] [--steps 20] [--warmup 5] [--profile-steps 20]

A YOLOv5u-n bf16 train step -- forward, v8DetectionLoss, backward, AdamW, zero_grad -- on synthetic device-resident images and labels, and the eval forward,
with model.0 = Conv(3, 16, 6, 2, 2) on the 6x6 stem kernels (STEM_DIRECT = 1: csrc/conv_stem6.hip reads the fp32 image) and on the generic route
(STEM_DIRECT = 0: pack pass + generic forward + generic weight gradient on the packed bf16 copy), both in this process.  Per route: median and min of the
timed steps (every step synchronised), eval images/s, and from further profiled steps (weight-gradient stream off, so durations do not inflate) the median
and min per launch of the kernel-profile classes of model.0, with the share of the 6.3 TB/s HBM rate of DESIGN.md that the layer's compulsory bytes reach.
The pack pass of the generic route has no profile class: it shows in the step time only.  As a ruler the same classes of YOLOv8n's 3x3 stem (the same
bytes; STEM_BNB_FUSE = 0 so that its weight gradient is the plain kernel) from the same run.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 6.3e12       # the float4-copy rate this project measured


def _launches(eng, fn, n):
    """n profiled calls of fn -> {(class, first word of the label): [us per launch]}."""
    eng.kernel_profile(True)
    for _ in range(n):
        fn()
    eng.synchronize()
    fd, path = tempfile.mkstemp(suffix=".csv")
    os.close(fd)
    try:
        eng.kernel_profile_dump(path)
        rows = [l.split(",") for l in open(path).read().splitlines()[1:]]
    finally:
        os.remove(path)
    eng.kernel_profile(False)
    out = {}
    for r in rows:
        if len(r) >= 3:
            out.setdefault((r[0], " ".join(r[1].split()[:2])), []).append(float(r[-1]))
    return out


def _stat(us, nbytes):
    if not us:
        return None
    med = statistics.median(us)
    return {"launches": len(us), "median_us": round(med, 2), "min_us": round(min(us), 2), "hbm_share_at_median": round(nbytes / (med * 1e-6) / HBM_BYTES_PER_S, 3)}


def synthetic_labels(B, nc, rng, per_image=8):
    """batch_idx [N], cls [N], bboxes [N, 4] normalised cxcywh: per_image boxes inside every image."""
    n = B * per_image
    wh = rng.uniform(0.08, 0.5, (n, 2))
    c = wh / 2 + rng.uniform(0, 1, (n, 2)) * (1 - wh)
    return (np.repeat(np.arange(B), per_image).astype(np.float32), rng.integers(0, nc, n).astype(np.float32), np.concatenate([c, wh], 1).astype(np.float32))


def run_model(eng, cls, a, direct, picks, options=None):
    from yolosharp_amd.model import AMPWrapper, v8DetectionLoss
    B, S, nc = a.batch, a.size, 80
    opts = dict(STEM_DIRECT=direct)
    opts.update(options or {})
    with eng.options(**opts):                    # read when the model is created
        m = cls(eng, nc=nc, size="n", height=S, width=S, max_batch=B, dtype="bf16")
    m.init_weights(1)
    rng = np.random.default_rng(0)
    x_dev = eng.to_device(rng.random((B, 3, S, S), np.float32))
    bidx, lcls, box = synthetic_labels(B, nc, rng)
    d = [eng.to_device(v) for v in (bidx, lcls, box)]
    m.reserve_labels(int(np.bincount(bidx.astype(np.int64), minlength=B).max()))
    crit = v8DetectionLoss(m)
    amp = AMPWrapper(m)

    def step():
        m.forward_device(x_dev, B)
        crit.forward_device(d[0], d[1], d[2], len(bidx))
        amp.Step()

    def timed(fn, n):
        ts = []
        for _ in range(n):
            eng.synchronize()
            t0 = time.perf_counter()
            fn()
            eng.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return ts

    m.train()
    for _ in range(a.warmup):
        step()
    ts = timed(step, a.steps)
    _, items = crit.read()
    m.eval()
    for _ in range(a.warmup):
        m.forward_device(x_dev, B)
    es = timed(lambda: m.forward_device(x_dev, B), a.steps)
    m.set_overlap(False)
    m.train()
    prof = _launches(eng, step, max(1, a.profile_steps))
    m.eval()
    eprof = _launches(eng, lambda: m.forward_device(x_dev, B), max(1, a.profile_steps))
    px = B * 3 * S * S * 4                                   # the fp32 image
    act = B * (S // 2) * (S // 2) * 16 * 2                   # model.0's bf16 output (raw, or dy)
    packed = B * S * S * 8 * 2                               # the packed bf16 copy the generic route reads instead of the image
    xin = px if direct else packed
    out = {"stem_direct": direct, "train_ms_median": round(statistics.median(ts), 3), "train_ms_min": round(min(ts), 3),
           "eval_ms_median": round(statistics.median(es), 3), "eval_images/s": round(B * 1e3 / statistics.median(es), 1),
           "loss_items": [float(v) for v in items],
           "model0_fwd_train": _stat(prof.get(picks[0]), xin + act), "model0_wgrad": _stat(prof.get(picks[1]), xin + act),
           "model0_fwd_eval": _stat(eprof.get(picks[0]), xin + act)}
    for p in d:
        eng.free(p)
    eng.free(x_dev)
    m.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--profile-steps", type=int, default=20)
    a = ap.parse_args()
    from yolosharp_amd import Engine
    from yolosharp_amd.model import Yolov5u, Yolov8
    eng = Engine(0)
    direct = run_model(eng, Yolov5u, a, 1, (("stem6", "stem6 k66"), ("stem6_wg", "wstem6 k6")))
    generic = run_model(eng, Yolov5u, a, 0, (("conv_igemm", "direct k6"), ("conv_wgrad", "wgrad k6")))
    ruler = run_model(eng, Yolov8, a, 1, (("conv_igemm", "stem k33"), ("conv_wgrad", "wstem k3")), options=dict(STEM_BNB_FUSE=0))
    print(json.dumps({"metric": "v5u_train_step", "model": "yolov5un", "dtype": "bf16", "batch": a.batch, "imgsz": a.size, "steps": a.steps,
                      "ms_per_step": direct["train_ms_median"], "images/s": round(a.batch * 1e3 / direct["train_ms_median"], 1),
                      "direct": direct, "generic": generic, "ruler_yolov8n_stem3x3": ruler}))


if __name__ == "__main__":
    main()
