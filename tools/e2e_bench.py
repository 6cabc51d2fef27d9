"""End2End cost on one device: prints ONE JSON line.

  python tools/e2e_bench.py [--task detect|segment|obb|pose] [--batch 64] [--imgsz 640] [--nc 80] [--steps 20] [--warmup 5] [--repeats 3]

Four measurements, each in a child process of its own under its own time limit (a leg that fails or runs out of time ends the run):
  step_off / step_on   ms per train step of YOLOv8n bf16 (forward, criterion, backward, AdamW, zero_grad; device-resident images and labels)
                       without and with End2End on the same build -- the difference is one criterion pass (tal_topk 1), the one2one pass
                       through the head towers' backward and the towers' second running-statistics update
  topk                 ys_e2e_topk on a device-resident [B, 4+nc, A] tensor (A = the model's anchors at --imgsz), max_det 300
  torch_topk           a torch restatement of Detect.get_topk_index + gather (Modules/Head.cs:117-127, 175-196) on the same tensor and GPU
--task segment measures the YOLOv11m-seg bf16 step at --batch 32 by default (BASELINE config 4's shape) with model.e2e_init() off and on -- the
difference is the second criterion pass (tal_topk 7 + the keep-best stage + the one2one mask term without its prototype gradient), the one2one pass
through the cv2 / cv3 / cv4 backward and the towers' second statistics update -- and ys_e2e_topk_ex (extra = 32 mask coefficients) against a torch
restatement of Segment.postprocess (Head.cs:321-339).
--task obb measures the YOLOv8n-obb bf16 step at --batch 64, nc 15 with model.e2e_obb_init() off and on -- the difference is the second criterion pass
(the rotated assigner with tal_topk 7 + the keep-best stage), the one2one pass through the cv2 / cv3 / cv4 backward and the towers' second statistics
update -- ys_e2e_topk_ex (extra = 1, the angle) against a torch restatement of Obb.postprocess (Head.cs:439-452), and one more leg, val_match: the
per-image part of Obber.Val on the End2End rows of a B = 16 eval forward, as the one launch ys_val_match_rotated_batched and as the per-image
ys_batch_probiou + ys_match_predictions loop (median of 20 calls each; both include fetching the rows, which Val needs anyway).
--task pose measures the YOLOv8n-pose bf16 step at --batch 64, nc 1, 17 x 3 keypoints with model.e2e_pose_init() off and on -- the difference is the
second criterion pass (tal_topk 7 + the keep-best stage + the second keypoint term), the one2one pass through the cv2 / cv3 / cv4 backward and the
towers' second statistics update -- ys_e2e_topk_ex (extra = 51) against a torch restatement of Pose.postprocess (Head.cs:550-563), and val_match: the
per-image part of PoseDetector.Val on the End2End rows of a B = 64 eval forward (about 8 labels per image), as the one launch
ys_val_match_pose_batched and as the per-image ys_box_iou / ys_kpt_iou + two ys_match_predictions calls.  The step legs also report criterion_ms: the
criterion's launches of one untimed step between events (its difference between the legs is the second criterion pass).
Every figure is the median over --repeats timed blocks of --steps calls after --warmup calls.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

LEGS = ("step_off", "step_on", "topk", "torch_topk")
OBB_LEGS = LEGS + ("val_match",)
EXTRA = {"detect": 0, "segment": 32, "obb": 1, "pose": 51}      # trailing channels of a "det" row: mask coefficients / the angle / 17 x 3 keypoints
KPT = (17, 3)


def _labels(B, nc, rng, kmax=16):
    bi, cl, bb = [], [], []
    for b in range(B):
        k = int(rng.integers(1, kmax + 1))
        wh = rng.random((k, 2)) * 0.57 + 0.03
        c = wh / 2 + rng.random((k, 2)) * (1 - wh)
        bi.append(np.full(k, b)); cl.append(rng.integers(0, nc, k)); bb.append(np.concatenate((c, wh), 1))
    return np.concatenate(bi).astype(np.float32), np.concatenate(cl).astype(np.float32), np.concatenate(bb).astype(np.float32)


def _timed(fn, sync, a):
    for _ in range(a.warmup):
        fn()
    sync()
    ms = []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        for _ in range(a.steps):
            fn()
        sync()
        ms.append((time.perf_counter() - t0) * 1e3 / a.steps)
    return float(np.median(ms)), [round(v, 4) for v in ms]


def _anchors(S):
    return (S // 8) ** 2 + (S // 16) ** 2 + (S // 32) ** 2


def _pred(B, nc, A, rng, extra=0):
    p = rng.random((B, 4 + nc + extra, A), dtype=np.float32)
    p[:, 4:4 + nc] = p[:, 4:4 + nc] ** 8           # most scores small, a few large: the shape of sigmoid outputs early in training
    return p


def _masks(bi, bb, B, mh, mw):
    """Overlap-encoded instance masks [B, H/4, W/4] (YoloDataset.cs:265-267): every label's box painted with its 1-based per-image index."""
    masks = np.zeros((B, mh, mw), np.float32)
    per = [0] * B
    for j in range(len(bi)):
        b = int(bi[j]); per[b] += 1
        cx, cy, w, h = bb[j] * np.array([mw, mh, mw, mh], np.float32)
        masks[b, max(int(cy - h / 2), 0):int(cy + h / 2) + 1, max(int(cx - w / 2), 0):int(cx + w / 2) + 1] = per[b]
    return masks


def _keypoints(bb, rng, K=KPT[0]):
    """Normalised keypoints [N, K, 3] inside each label's box, visibility 0 / 1 / 2 with about a quarter unlabelled."""
    u = rng.random((len(bb), K, 2)) - 0.5
    xy = np.clip(bb[:, None, :2] + u * bb[:, None, 2:4], 0.0, 1.0)
    v = np.minimum(rng.integers(0, 4, (len(bb), K, 1)), 2)
    return np.concatenate((xy, v), 2).astype(np.float32)


def leg_step(a, end2end):
    from yolosharp_amd import Engine
    from yolosharp_amd.model import AMPWrapper, Yolov8, Yolov8Obb, Yolov8Pose, Yolov11Segment, v8DetectionLoss, v8OBBLoss, v8PoseLoss, v8SegmentationLoss
    eng = Engine(0)
    B, S, nc = a.batch, a.imgsz, a.nc
    seg, obb, pose = a.task == "segment", a.task == "obb", a.task == "pose"
    if pose:
        m = Yolov8Pose(eng, nc=nc, size="n", height=S, width=S, max_batch=B, dtype="bf16", kpt_num=KPT[0], kpt_dim=KPT[1])
        if end2end:
            m.e2e_pose_init()
    elif obb:
        m = Yolov8Obb(eng, nc=nc, size="n", height=S, width=S, max_batch=B, dtype="bf16")
        if end2end:
            m.e2e_obb_init()
    elif seg:
        m = Yolov11Segment(eng, nc=nc, size="m", height=S, width=S, max_batch=B, dtype="bf16")
        if end2end:
            m.e2e_init()
    else:
        m = Yolov8(eng, nc=nc, size="n", height=S, width=S, max_batch=B, dtype="bf16", end2end=end2end)
    m.init_weights(1)
    rng = np.random.default_rng(0)
    x_dev = eng.to_device(rng.random((B, 3, S, S), dtype=np.float32))
    bi, cl, bb = _labels(B, nc, rng)
    if obb:                                         # oriented labels: + an angle in [-pi/4, 3pi/4)
        bb = np.concatenate((bb, (rng.random((len(bb), 1)) * np.pi - np.pi / 4)), 1).astype(np.float32)
    m.reserve_labels(16)
    d = [eng.to_device(v) for v in (bi, cl, bb)]
    if seg:
        d.append(eng.to_device(_masks(bi, bb, B, S // 4, S // 4)))
    if pose:
        d.append(eng.to_device(_keypoints(bb, rng)))
    crit, amp = (v8PoseLoss if pose else v8OBBLoss if obb else v8SegmentationLoss if seg else v8DetectionLoss)(m), AMPWrapper(m)
    m.train()

    def step():
        m.forward_device(x_dev, B)
        crit.forward_device(d[0], d[1], d[2], bi.shape[0], *d[3:])
        amp.Step()

    ms, runs = _timed(step, eng.synchronize, a)
    _, items = crit.read()
    # launches the library's own profiler sees per step (untimed; the weight-gradient stream off so that the order is the issue order)
    m.set_overlap(False)
    eng.kernel_profile(True)
    step(); eng.synchronize()
    path = os.path.join(a.tmp, "e2e_bench_launches_%d.csv" % int(end2end))
    eng.kernel_profile_dump(path)
    eng.kernel_profile(False)
    with open(path) as f:
        launches = max(0, sum(1 for _ in f) - 1)
    os.remove(path)
    # the criterion's launches of one more untimed step between events on the stream (the context's timers: detect part + the task's own term)
    eng.profile(True)
    step(); eng.synchronize()
    crit_ms = eng.last_ms("loss") + (eng.last_ms("loss_seg") if seg else eng.last_ms("loss_pose") if pose else 0.0)
    eng.profile(False)
    for p in d + [x_dev]:
        eng.free(p)
    m.close()
    return {"ms_per_step": round(ms, 4), "runs": runs, "loss_items": [float(v) for v in items], "profiled_launches_per_step": launches,
            "criterion_ms": round(crit_ms, 4)}


def leg_topk(a):
    from yolosharp_amd import Engine, _lib
    eng = Engine(0)
    B, nc, A = a.batch, a.nc, _anchors(a.imgsz)
    extra = EXTRA[a.task]
    k = min(300, A)
    p_dev = eng.to_device(_pred(B, nc, A, np.random.default_rng(1), extra))
    rows, anc = eng.malloc(B * k * (6 + extra) * 4), eng.malloc(B * k * 8)

    def call():
        if extra:
            _lib.check(eng.lib, eng.lib.ys_e2e_topk_ex(eng.ctx, p_dev, 1, B, nc, extra, A, 300, rows, anc))
        else:
            _lib.check(eng.lib, eng.lib.ys_e2e_topk(eng.ctx, p_dev, 1, B, nc, A, 300, rows, anc))

    ms, runs = _timed(call, eng.synchronize, a)
    eng.kernel_profile(True)
    call(); eng.synchronize()
    n, kernel_ms = eng.kernel_profile_read("e2e_topk")
    eng.kernel_profile(False)
    for p in (p_dev, rows, anc):
        eng.free(p)
    # kernels_ms: the two launches alone, between HIP events on the stream
    return {"ms_per_call": round(ms, 4), "runs": runs, "kernels_ms": round(kernel_ms / max(n, 1), 4), "B": B, "A": A, "nc": nc, "extra": extra, "k": k}


def leg_torch_topk(a):
    import torch
    B, nc, A = a.batch, a.nc, _anchors(a.imgsz)
    extra = EXTRA[a.task]
    pred = torch.from_numpy(_pred(B, nc, A, np.random.default_rng(1), extra)).cuda()
    k = min(300, A)
    ar = torch.arange(B, device="cuda")[:, None]

    def call():
        p = pred.permute(0, 2, 1)
        boxes, scores, mc = p.split((4, nc, extra), dim=-1)
        ori = scores.amax(-1).topk(k).indices.unsqueeze(-1)
        sc = scores.gather(1, ori.expand(-1, -1, nc))
        sc, index = sc.flatten(1).topk(k)
        idx = ori[ar, torch.div(index, nc, rounding_mode="floor")]
        bx = boxes.gather(1, idx.expand(-1, -1, 4))
        out = [bx, sc[..., None], (index % nc)[..., None].float()]
        if extra:                                   # Segment / Obb.postprocess: the coefficients / the angle by the same anchor index
            out.append(mc.gather(1, idx.expand(-1, -1, extra)))
        return torch.cat(out, -1)

    ms, runs = _timed(call, torch.cuda.synchronize, a)
    return {"ms_per_call": round(ms, 4), "runs": runs}


def leg_val_match(a):
    """The per-image part of Obber.Val on the End2End rows of one eval forward (B = 16): one launch against the per-image loop."""
    from yolosharp_amd import Engine, _lib
    from yolosharp_amd.model import Yolov8Obb
    eng = Engine(0)
    B, S, nc = 16, a.imgsz, a.nc
    m = Yolov8Obb(eng, nc=nc, size="n", height=S, width=S, max_batch=B, dtype="bf16")
    m.e2e_obb_init()
    m.init_weights(1)
    rng = np.random.default_rng(0)
    m.eval()
    m.forward(rng.random((B, 3, S, S), dtype=np.float32), fetch=False)
    d_det, k = m.det_device()
    bi, cl, bb = _labels(B, nc, rng)
    bb = np.concatenate((bb, (rng.random((len(bb), 1)) * np.pi - np.pi / 4)), 1).astype(np.float32)
    d_cnt, d_cor = eng.malloc(B * 4), eng.malloc(B * k * 10)
    d_lab = [eng.to_device(v) for v in (bi, cl, bb)]
    _lib.check(eng.lib, eng.lib.ys_e2e_select_ex(eng.ctx, d_det, 1, B, k, 7, 0.001, 300, d_cnt))
    cnt = eng.from_device(d_cnt, (B,), np.int32)
    scale = np.array([S, S, S, S], np.float32)
    out = {}

    def batched():
        _lib.check(eng.lib, eng.lib.ys_val_match_rotated_batched(eng.ctx, d_det, d_cnt, 1, B, k, 7, 6, d_lab[0], d_lab[1], d_lab[2], bi.shape[0],
                                                                 float(S), float(S), d_cor))
        rows = eng.from_device(d_det, (B, k, 7), np.float32)
        cor = eng.from_device(d_cor, (B, k, 10), np.uint8)
        out["batched"] = [cor[b, :cnt[b]].astype(bool) for b in range(B)]
        return rows

    def per_image():
        rows = eng.from_device(d_det, (B, k, 7), np.float32)
        res = []
        for b in range(B):
            sel = bi == b
            r = rows[b, :cnt[b]]
            gt = np.concatenate((bb[sel, :4] * scale, bb[sel, 4:5]), 1).astype(np.float32)
            pred = np.concatenate((r[:, :4], r[:, 6:7]), 1).astype(np.float32)
            iou = eng.batch_probiou(gt, pred) if len(gt) and len(pred) else np.zeros((len(gt), len(pred)), np.float32)
            res.append(eng.match_predictions(r[:, 5], cl[sel], iou))
        out["per_image"] = res

    a.steps, a.repeats = 1, 20                       # median of 20 single calls
    ms_b, _ = _timed(batched, eng.synchronize, a)
    ms_p, _ = _timed(per_image, eng.synchronize, a)
    same = all(np.array_equal(x, y) for x, y in zip(out["batched"], out["per_image"]))
    for p in d_lab + [d_cnt, d_cor]:
        eng.free(p)
    m.close()
    return {"batched_ms": round(ms_b, 4), "per_image_ms": round(ms_p, 4), "identical": bool(same), "B": B, "k": k, "rows_kept": int(cnt.sum()),
            "labels": int(bi.shape[0])}


def leg_val_match_pose(a):
    """The per-image part of PoseDetector.Val on the End2End rows of one eval forward: one launch against the four calls per image."""
    from yolosharp_amd import Engine, _lib
    from yolosharp_amd.model import Yolov8Pose
    eng = Engine(0)
    B, S, nc, (K, D) = a.batch, a.imgsz, a.nc, KPT
    rl = 6 + K * D
    m = Yolov8Pose(eng, nc=nc, size="n", height=S, width=S, max_batch=B, dtype="bf16", kpt_num=K, kpt_dim=D)
    m.e2e_pose_init()
    m.init_weights(1)
    rng = np.random.default_rng(0)
    m.eval()
    m.forward(rng.random((B, 3, S, S), dtype=np.float32), fetch=False)
    d_det, k = m.det_device()
    bi, cl, bb = _labels(B, nc, rng)
    kp = _keypoints(bb, rng)
    d_cnt, d_cob, d_cop = eng.malloc(B * 4), eng.malloc(B * k * 10), eng.malloc(B * k * 10)
    d_lab = [eng.to_device(v) for v in (bi, cl, bb, kp)]
    _lib.check(eng.lib, eng.lib.ys_e2e_select_ex(eng.ctx, d_det, 1, B, k, rl, 0.001, 300, d_cnt))
    cnt = eng.from_device(d_cnt, (B,), np.int32)
    out = {}

    def batched():
        _lib.check(eng.lib, eng.lib.ys_val_match_pose_batched(eng.ctx, d_det, d_cnt, 1, B, k, rl, 6, K, D, d_lab[0], d_lab[1], d_lab[2], d_lab[3], 3,
                                                              bi.shape[0], float(S), float(S), d_cob, d_cop))
        eng.from_device(d_det, (B, k, rl), np.float32)
        cob, cop = eng.from_device(d_cob, (B, k, 10), np.uint8), eng.from_device(d_cop, (B, k, 10), np.uint8)
        out["batched"] = [c_[b, :cnt[b]].astype(bool) for c_ in (cob, cop) for b in range(B)]

    def per_image():
        rows = eng.from_device(d_det, (B, k, rl), np.float32)
        rb, rp = [], []
        for b in range(B):
            sel = bi == b
            r = rows[b, :cnt[b]]
            gt = bb[sel] * np.array([S, S, S, S], np.float32)
            xyxy = np.concatenate((gt[:, :2] - gt[:, 2:] / 2, gt[:, :2] + gt[:, 2:] / 2), 1).astype(np.float32)
            gk = (kp[sel] * np.array([S, S, 1.0], np.float32)).astype(np.float32)
            area = ((xyxy[:, 2] - xyxy[:, 0]) * (xyxy[:, 3] - xyxy[:, 1]) * np.float32(0.53)).astype(np.float32)
            rb.append(eng.match_predictions(r[:, 5], cl[sel], eng.box_iou(xyxy, r[:, :4])))
            rp.append(eng.match_predictions(r[:, 5], cl[sel], eng.kpt_iou(gk, r[:, 6:].reshape(-1, K, D), area)))
        out["per_image"] = rb + rp

    a.steps, a.repeats = 1, 10                       # median of 10 single calls
    ms_b, _ = _timed(batched, eng.synchronize, a)
    ms_p, _ = _timed(per_image, eng.synchronize, a)
    same = all(np.array_equal(x, y) for x, y in zip(out["batched"], out["per_image"]))
    for p in d_lab + [d_cnt, d_cob, d_cop]:
        eng.free(p)
    m.close()
    return {"batched_ms": round(ms_b, 4), "per_image_ms": round(ms_p, 4), "identical": bool(same), "B": B, "k": k, "rows_kept": int(cnt.sum()),
            "labels": int(bi.shape[0]), "launches_batched": 1, "launches_per_image": 4 * B}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--task", choices=("detect", "segment", "obb", "pose"), default="detect")
    ap.add_argument("--batch", type=int, default=0, help="0 = 64 (detect, YOLOv8n; obb, YOLOv8n-obb; pose, YOLOv8n-pose) / 32 (segment, YOLOv11m-seg: config 4's shape)")
    ap.add_argument("--imgsz", type=int, default=640)
    ap.add_argument("--nc", type=int, default=0, help="0 = 80 (detect, segment) / 15 (obb) / 1 (pose)")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--leg-timeout", type=int, default=240, help="seconds per child process")
    ap.add_argument("--tmp", default=os.environ.get("TMPDIR", "/tmp"))
    ap.add_argument("--leg", choices=OBB_LEGS, help="run one measurement in this process (what the driver starts)")
    a = ap.parse_args()
    if a.batch <= 0:
        a.batch = 32 if a.task == "segment" else 64
    if a.nc <= 0:
        a.nc = 15 if a.task == "obb" else 1 if a.task == "pose" else 80
    if a.leg:
        out = {"step_off": lambda: leg_step(a, False), "step_on": lambda: leg_step(a, True), "topk": lambda: leg_topk(a),
               "torch_topk": lambda: leg_torch_topk(a), "val_match": lambda: (leg_val_match_pose if a.task == "pose" else leg_val_match)(a)}[a.leg]()
        print(json.dumps(out))
        return 0
    res = {"metric": "e2e_cost", "task": a.task, "model": {"segment": "yolov11m-seg", "obb": "yolov8n-obb", "pose": "yolov8n-pose"}.get(a.task, "yolov8n"), "dtype": "bf16", "batch": a.batch,
           "imgsz": a.imgsz, "nc": a.nc}
    fwd = [x for kv in (("--task", a.task), ("--batch", a.batch), ("--imgsz", a.imgsz), ("--nc", a.nc), ("--steps", a.steps), ("--warmup", a.warmup),
                        ("--repeats", a.repeats), ("--tmp", a.tmp)) for x in (kv[0], str(kv[1]))]
    for leg in (OBB_LEGS if a.task in ("obb", "pose") else LEGS):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", leg] + fwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                               text=True, timeout=a.leg_timeout, stdin=subprocess.DEVNULL)
        except subprocess.TimeoutExpired:
            res["failed"] = {"leg": leg, "why": "time limit of %d s" % a.leg_timeout}
            break                                   # nothing more is started on the device after a leg that hung
        if r.returncode != 0:
            res["failed"] = {"leg": leg, "rc": r.returncode, "stderr": r.stderr[-2000:]}
            break                                   # ... or that failed
        res[leg] = json.loads(r.stdout.strip().splitlines()[-1])
    if "step_off" in res and "step_on" in res:
        res["e2e_extra_ms"] = round(res["step_on"]["ms_per_step"] - res["step_off"]["ms_per_step"], 4)
        res["e2e_extra_launches"] = res["step_on"]["profiled_launches_per_step"] - res["step_off"]["profiled_launches_per_step"]
        res["e2e_extra_criterion_ms"] = round(res["step_on"]["criterion_ms"] - res["step_off"]["criterion_ms"], 4)
    print(json.dumps(res))
    return 1 if "failed" in res else 0


if __name__ == "__main__":
    sys.exit(main())
