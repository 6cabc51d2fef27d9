"""Classification train / eval throughput on one device: prints ONE JSON line.

  python tools/cls_bench.py [--family 8|11] [--batch 256] [--size 224] [--nc 1000] [--steps 20] [--warmup 5]

A YOLOv8n-cls (or, with --family 11, YOLOv11n-cls) bf16 train step -- forward, v8ClassificationLoss, backward, AdamW, zero_grad -- on
synthetic device-resident images and labels, then the eval forward (softmax) and ys_cls_topk(k = 5).  The line holds ms_per_step,
images/s, eval images/s and, from a few further profiled (untimed) steps, the per-launch time of every classify kernel class.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

KERNELS = ("cls_pool", "cls_pool_bwd", "cls_xent", "cls_softmax", "cls_topk", "conv_igemm")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--family", type=int, default=8, choices=(8, 11))
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--nc", type=int, default=1000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--profile-steps", type=int, default=3)
    a = ap.parse_args()

    from yolosharp_amd import Engine
    from yolosharp_amd.model import AMPWrapper, Yolov8Classify, Yolov11Classify, v8ClassificationLoss
    eng = Engine(0)
    B, S, nc = a.batch, a.size, a.nc
    m = (Yolov8Classify if a.family == 8 else Yolov11Classify)(eng, nc=nc, size="n", height=S, width=S, max_batch=B, dtype="bf16")
    m.init_weights(1)
    rng = np.random.default_rng(0)
    x_dev = eng.to_device(rng.random((B, 3, S, S), np.float32))
    y_dev = eng.to_device(rng.integers(0, nc, B).astype(np.float32))
    crit = v8ClassificationLoss(m)
    amp = AMPWrapper(m)

    def step():
        m.forward_device(x_dev, B)
        crit.forward_device(y_dev, B)
        amp.Step()

    m.train()
    for _ in range(a.warmup):
        step()
    eng.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        step()
    eng.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / a.steps
    _, items = crit.read()

    # eval: forward (folded BN, softmax) + top-5 on the device probabilities
    m.eval()
    probs_dev = m.pred_device()
    idx_dev = eng.malloc(B * 5 * 4)
    import ctypes as C
    from yolosharp_amd import _lib

    def eval_step():
        m.forward_device(x_dev, B)
        _lib.check(eng.lib, eng.lib.ys_cls_topk(eng.ctx, probs_dev, 1, B, nc, 5, idx_dev))

    for _ in range(a.warmup):
        eval_step()
    eng.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        eval_step()
    eng.synchronize()
    ems = (time.perf_counter() - t0) * 1e3 / a.steps

    # per-kernel-class times (profiled steps, not timed above; the weight-gradient stream is switched off so durations do not inflate)
    m.set_overlap(False)
    eng.kernel_profile(True)
    n = max(1, a.profile_steps)
    for _ in range(n):
        m.train(); step()
        m.eval(); eval_step()
    eng.synchronize()
    prof = {}
    for k in KERNELS:
        try:
            cnt, tot = eng.kernel_profile_read(k)
        except Exception:
            cnt, tot = 0, 0.0
        prof[k] = {"launches_per_step": cnt / n, "us_per_step": round(tot * 1e3 / n, 2)}
    eng.kernel_profile(False)
    out = {"metric": "cls_train_step", "model": "yolov%dn-cls" % a.family, "dtype": "bf16", "batch": B, "imgsz": S, "nc": nc,
           "ms_per_step": round(ms, 3), "images/s": round(B * 1e3 / ms, 1), "eval_ms": round(ems, 3), "eval_images/s": round(B * 1e3 / ems, 1),
           "loss": float(items[0]), "kernels": prof}
    print(json.dumps(out))
    eng.free(idx_dev); eng.free(x_dev); eng.free(y_dev)
    m.close()


if __name__ == "__main__":
    main()
