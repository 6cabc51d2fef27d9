"""Classification train / eval throughput on one device: prints ONE JSON line.

  python tools/cls_bench.py [--family 8|11] [--batch 256] [--size 224] [--nc 1000] [--steps 20] [--warmup 5] [--input resident|device]
                             [--auto-augment autoaugment|randaugment]

A YOLOv8n-cls (or, with --family 11, YOLOv11n-cls) bf16 train step -- forward, v8ClassificationLoss, backward, AdamW, zero_grad -- on
synthetic device-resident images and labels, then the eval forward (softmax) and ys_cls_topk(k = 5).  The line holds ms_per_step,
images/s, eval images/s and, from a few further profiled (untimed) steps, the per-launch time of every classify kernel class.

--input device adds the classification input on the device (augment.ClassifyAugmenter over a synthetic uint8 dataset; ys_augment_classify): under
"device_input" the ms per ys_augment_classify call with and without contrast rows (items and rows uploaded once, outside the timed loop), the bytes it
writes per second against the 6.3 TB/s this project measured for HBM, the train step fed from it (draws on the host, upload of items and rows, the gather,
then the step) beside the resident-tensor step of the same process, and the torch-on-CPU restatement's ms per batch for scale.
--auto-augment autoaugment | randaugment (with --input device) gives the augmenter that policy (ys_augment_classify_aa): "augment_ms_aa" is the call with the
drawn ys_aa_row table and contrast rows, "augment_ms_aa_empty_rows" the same call with every slot empty (staging, two copies and the statistics launches that
leave at once), "aa_active_slots" the share of slots that run an op; the fed train step then includes the policy's draws.
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
    ap.add_argument("--input", default="resident", choices=("resident", "device"))
    ap.add_argument("--dataset", type=int, default=512, help="--input device: images of the synthetic uint8 dataset")
    ap.add_argument("--auto-augment", default=None, choices=("autoaugment", "randaugment"), help="--input device: the augmenter's Auto_Augment policy")
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
    if a.input == "device":
        out["device_input"] = device_input(a, eng, m, crit, amp, ms)
    print(json.dumps(out))
    eng.free(idx_dev); eng.free(x_dev); eng.free(y_dev)
    m.close()


HBM_BYTES_PER_S = 6.3e12       # the float4-copy rate this project measured


def _hue(im, f):
    """torchvision's adjust_hue on a uint8 image [3, h, w] (its public algorithm: / 255, _rgb2hsv, (h + f) % 1, _hsv2rgb, * 255.999 truncated)."""
    import torch
    x = im.float() / 255.0
    r, g, b = x.unbind(0)
    maxc, minc = x.max(0).values, x.min(0).values
    eqc = maxc == minc
    cr = maxc - minc
    ones = torch.ones_like(maxc)
    s = cr / torch.where(eqc, ones, maxc)
    d = torch.where(eqc, ones, cr)
    rc, gc, bc = (maxc - r) / d, (maxc - g) / d, (maxc - b) / d
    h = (maxc == r) * (bc - gc) + ((maxc == g) & (maxc != r)) * (2.0 + rc - bc) + ((maxc != g) & (maxc != r)) * (4.0 + gc - rc)
    h = torch.remainder(torch.fmod(h / 6.0 + 1.0, 1.0) + f, 1.0)
    i = torch.floor(h * 6.0)
    ff = h * 6.0 - i
    i = (i.to(torch.int64) % 6)[None]
    p, q, t = (maxc * (1.0 - s)).clamp(0, 1), (maxc * (1.0 - s * ff)).clamp(0, 1), (maxc * (1.0 - s * (1.0 - ff))).clamp(0, 1)
    v = maxc
    pick = lambda c: torch.gather(torch.stack(c), 0, i)[0]
    out = torch.stack((pick((v, q, p, p, t, v)), pick((t, v, v, q, p, p)), pick((p, p, t, v, v, q))))
    return (out * 255.999).to(torch.uint8)


def _cpu_restatement_ms(imgs, items, rows, s):
    """ms per batch of the same chain in torch on the CPU: crop, nearest interpolate, flip, ColorJitter's four ops on uint8 (torchvision's public algorithm, written here, not
    imported from tests/; the erase rectangle is filled with torch.randn cast to uint8, as the reference does), mul(1 / 255)."""
    import torch
    t0 = time.perf_counter()
    out = []
    for it, row in zip(items, rows):
        im = torch.from_numpy(imgs[int(it["src"])])[:, it["top"]:it["top"] + it["ch"], it["left"]:it["left"] + it["cw"]]
        im = torch.nn.functional.interpolate(im[None], size=(s, s), mode="nearest")[0]
        if it["flip_lr"]:
            im = im.flip(-1)
        if it["er_h"] > 0:
            im = im.clone()
            im[:, it["er_y"]:it["er_y"] + it["er_h"], it["er_x"]:it["er_x"] + it["er_w"]] = torch.randn(3, int(it["er_h"]), int(it["er_w"])).to(torch.int64).to(torch.uint8)
        for op in row["order"]:
            f = float(row["factor"][op]) if op >= 0 else 0.0
            if op in (0, 1, 2):
                g = ((0.2989 * im[0].float() + 0.587 * im[1].float()) + 0.114 * im[2].float()).to(torch.uint8).float()
                other = torch.zeros(()) if op == 0 else (g.mean() if op == 1 else g[None])
                im = (f * im.float() + (1.0 - f) * other).clamp(0, 255).to(torch.uint8)
            elif op == 3:
                im = _hue(im, f)
        out.append(im.float() * (1 / 255.0))
    torch.stack(out)
    return (time.perf_counter() - t0) * 1e3


def device_input(a, eng, m, crit, amp, resident_ms):
    from yolosharp_amd import _lib
    from yolosharp_amd import augment as A
    B, S, nc = a.batch, a.size, a.nc
    g = np.random.default_rng(1)
    # sources like a resized ImageNet sample: short side about 256, aspect ratios 3:4 .. 4:3 .. 16:9
    shapes = [(256, 256), (256, 341), (341, 256), (256, 384), (288, 512), (300, 400)]
    imgs = [g.integers(0, 256, (3,) + shapes[i % len(shapes)], dtype=np.uint8) for i in range(a.dataset)]
    classes = g.integers(0, nc, a.dataset).astype(np.float32)
    policy = {None: None, "autoaugment": A.AutoAugment(), "randaugment": A.RandAugment()}[a.auto_augment]
    aug = A.ClassifyAugmenter(eng, imgs, classes, S, seed=0, max_batch=B, auto_augment=policy)
    idx = g.integers(0, a.dataset, B)
    drawn = aug.draw(idx)
    items, rows, aa = drawn if policy is not None else drawn + (None,)
    plain = rows.copy()
    plain["order"][plain["order"] == A.JITTER_CONTRAST] = -1           # the same rows without their contrast op: one launch

    def time_calls(r, aa_rows=None):
        aug.run(items, r, aa_rows)                                     # uploads items and rows
        d_jit = aug.d_jitter if r is not None else None

        def call():
            if aa_rows is not None:
                _lib.check(eng.lib, eng.lib.ys_augment_classify_aa(eng.ctx, aug.d_arena, aug.d_srcs, aug.count, aug.d_src_cls, aug.d_items, B, 1, S, aug.d_aa, d_jit,
                                                                   aug.d_images, aug.d_ocls))
                return
            _lib.check(eng.lib, eng.lib.ys_augment_classify(eng.ctx, aug.d_arena, aug.d_srcs, aug.count, aug.d_src_cls, aug.d_items, B, 1, S, d_jit, aug.d_images,
                                                            aug.d_ocls))
        for _ in range(a.warmup):
            call()
        eng.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            call()
        eng.synchronize()
        return (time.perf_counter() - t0) * 1e3 / a.steps

    ms_contrast, ms_plain, ms_none = time_calls(rows), time_calls(plain), time_calls(None)
    aa_out = {}
    if policy is not None:
        aa_out = {"auto_augment": a.auto_augment, "augment_ms_aa": round(time_calls(rows, aa), 4),
                  "augment_ms_aa_empty_rows": round(time_calls(rows, A.make_aa_rows(B)), 4), "aa_active_slots": round(float((aa["op"] >= 0).mean()), 3)}
    written = B * 3 * S * S * 4

    def step():
        db = aug.batch(g.integers(0, a.dataset, B))
        m.forward_device(db.images, B)
        crit.forward_device(db.cls, B)
        amp.Step()

    m.set_overlap(True)
    m.train()
    for _ in range(a.warmup):
        step()
    eng.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        step()
    eng.synchronize()
    step_ms = (time.perf_counter() - t0) * 1e3 / a.steps
    t0 = time.perf_counter()
    for _ in range(3):
        aug.draw(idx)
    draw_ms = (time.perf_counter() - t0) * 1e3 / 3
    cpu_ms = _cpu_restatement_ms(imgs, items, rows, S)
    aug.close()
    return {**aa_out, "augment_ms_contrast": round(ms_contrast, 4), "augment_ms_no_contrast": round(ms_plain, 4), "augment_ms_no_jitter": round(ms_none, 4),
            "bytes_written": written, "write_GB/s_contrast": round(written / ms_contrast / 1e6, 1), "write_GB/s_no_contrast": round(written / ms_plain / 1e6, 1),
            "hbm_fraction_contrast": round(written / (ms_contrast * 1e-3) / HBM_BYTES_PER_S, 4),
            "hbm_fraction_no_contrast": round(written / (ms_plain * 1e-3) / HBM_BYTES_PER_S, 4),
            "host_draw_ms": round(draw_ms, 3), "step_ms_device_input": round(step_ms, 3), "step_ms_resident": round(resident_ms, 3),
            "cpu_torch_ms_per_batch": round(cpu_ms, 1)}


if __name__ == "__main__":
    main()
