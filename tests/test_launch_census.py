"""Launch census: which kernels a training step launches, per kernel class, for five small graphs that together reach every branch of
run_conv_fwd / run_conv_bwd / backward_range (csrc/model.hip) and of the planner (csrc/plan.hip).

tests/golden/launch_census.json was recorded by THIS test body (`python tests/test_launch_census.py --record emu|gpu`) at commit 3d473b8,
the last one with the whole model in a single translation unit; the split into graph / plan / step / ABI units and the helper folding that
followed must not move a single launch.  It is never regenerated from a tree whose launches are in question: a pull request that changes
the launches on purpose re-records it and says so.  The `us` column of the profile dump is ignored -- only (class, label) multisets count.

Golden layout (the configurations share most of their labels, and so do the two backends): "labels" = every "class<TAB>label" once; per configuration
"rows" = indices into it and, under the two backend keys "emu" and "gpu", the launch count of each row."""
import collections
import json
import os
import sys
import tempfile

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":
    sys.path[:0] = [os.path.dirname(HERE), HERE]

from conftest import BACKENDS
from oracle import yolo_oracle as O

GOLDEN = os.path.join(HERE, "golden", "launch_census.json")
B, H, W = 2, 64, 64          # 8 x 8, 4 x 4 and 2 x 2 head maps: SPPF's fused form (at most 400 pixels) is taken
SEED = 3
CONFIGS = ["v8n_detect_bf16", "v11n_segment_e2e_bf16", "v8n_pose_e2e_bf16", "v8n_classify_f32", "v8n_detect_fp8"]


def _np(d):
    return {k: v.numpy() for k, v in d.items()}


def build(engine, cfg):
    """(model, criterion, batch) of a configuration: the constructors and synthetic batches of test_model / test_segment / test_e2e_pose /
    test_classify / test_fp8, weights from init_weights with a fixed seed."""
    import torch
    from yolosharp_amd import model as M
    kw = dict(size="n", height=H, width=W, max_batch=B)
    if cfg == "v8n_detect_bf16" or cfg == "v8n_detect_fp8":
        # stem direct path, fused stem BN backward, grouped head, fused SPPF, fused BN-backward reduction | fp8: bootstrap pass, then fp8 forward / dgrad
        m = M.Yolov8(engine, nc=80, dtype="fp8" if cfg.endswith("fp8") else "bf16", **kw)
        crit, batch = M.v8DetectionLoss(m), _np(O.synthetic_batch(B, H, W, 80, seed=1, kmax=6))
    elif cfg == "v11n_segment_e2e_bf16":
        # C3k2 / C2PSA / attention / depthwise, Proto with ConvTranspose, the one2one backward pass that skips Proto's descriptors
        m = M.Yolov11Segment(engine, nc=80, dtype="bf16", **kw)
        m.e2e_init(300, 100)
        tb = O.synthetic_batch(B, H, W, 80, seed=1, kmax=6)
        tb["masks"] = O.synthetic_masks(tb, B, H // 4, W // 4)
        crit, batch = M.v8SegmentationLoss(m), _np(tb)
    elif cfg == "v8n_pose_e2e_bf16":
        # padded towers: cout > cout_real
        m = M.Yolov8Pose(engine, nc=1, dtype="bf16", kpt_num=17, kpt_dim=3, **kw)
        m.e2e_pose_init(300, 100)
        tb = O.synthetic_batch(B, H, W, 1, seed=1, kmax=8)
        tb["keypoints"] = O.synthetic_keypoints(tb, 17, 3)
        crit, batch = M.v8PoseLoss(m), _np(tb)
    elif cfg == "v8n_classify_f32":
        # pool_next / OP_POOL, the non-bf16 plain routes
        m = M.Yolov8Classify(engine, nc=7, dtype="f32", **kw)
        y = torch.randint(0, 7, (B,), generator=torch.Generator().manual_seed(4)).float()
        crit, batch = M.v8ClassificationLoss(m), {"cls": y.numpy()}
    else:
        raise KeyError(cfg)
    m.init_weights(SEED)
    return m, crit, batch


def run_steps(engine, cfg):
    """Two training steps (forward, criterion, zero_grad, backward, AdamW) and one eval forward with the per-launch profile on.
    Returns (census, arrays): census = {class: {label: launches}}; arrays = the loss items of both steps, every gradient after step two's
    backward and the state_dict after step two's AdamW (what a bit-identity comparison of two builds needs)."""
    m, crit, batch = build(engine, cfg)
    x = np.random.default_rng(0).random((B, 3, H, W), dtype=np.float32)
    arrays = {}
    engine.kernel_profile(True)
    try:
        for step in range(2):
            m.train()
            m.forward(x, fetch=False)
            _, items = crit(None, batch)
            arrays["items%d" % step] = np.asarray(items, np.float32)
            m.zero_grad()
            m.backward()
            if step == 1:
                arrays.update(("grad/" + k, v) for k, v in m.grads().items())
            m.adamw_step([1e-3] * 3)
        arrays.update(("state/" + k, v) for k, v in m.state_dict().items())
        m.eval()
        m.forward(x, fetch=False)
        engine.synchronize()
        with tempfile.NamedTemporaryFile(suffix=".csv", delete=False) as f:
            path = f.name
        engine.kernel_profile_dump(path)
    finally:
        engine.kernel_profile(False)
    census = collections.defaultdict(collections.Counter)
    with open(path) as f:
        assert f.readline().strip() == "class,label,us"
        for line in f:
            cls, rest = line.rstrip("\n").split(",", 1)
            census[cls][rest.rsplit(",", 1)[0]] += 1
    os.remove(path)
    m.close()
    return {c: dict(sorted(census[c].items())) for c in sorted(census)}, arrays


def load_golden():
    """{cfg: {backend: {class: {label: launches}}}} from the table form of the file."""
    raw = json.load(open(GOLDEN))
    out = {}
    for cfg, e in raw["configs"].items():
        for backend in ("emu", "gpu"):
            census = out.setdefault(cfg, {}).setdefault(backend, {}) if backend in e else None
            for row, n in zip(e["rows"], e.get(backend, [])):
                cls, label = raw["labels"][row].split("\t", 1)
                if n:
                    census.setdefault(cls, {})[label] = n
    return out


def save_golden(gold):
    labels = sorted({cls + "\t" + label for e in gold.values() for census in e.values() for cls, d in census.items() for label in d})
    at = {l: i for i, l in enumerate(labels)}
    with open(GOLDEN, "w") as f:
        f.write('{"labels": [\n' + ",\n".join(json.dumps(l) for l in labels) + '],\n"configs": {\n')
        rows_of = lambda e: sorted({at[cls + "\t" + label] for census in e.values() for cls, d in census.items() for label in d})
        items = []
        for cfg in sorted(gold):
            rows = rows_of(gold[cfg])
            ent = {"rows": rows}
            for backend in sorted(gold[cfg]):
                ent[backend] = [gold[cfg][backend].get(labels[r].split("\t", 1)[0], {}).get(labels[r].split("\t", 1)[1], 0) for r in rows]
            items.append(json.dumps(cfg) + ": {" + ",\n ".join(json.dumps(k) + ": " + json.dumps(v, separators=(",", ":")) for k, v in ent.items()) + "}")
        f.write(",\n".join(items) + "}}\n")


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("cfg", CONFIGS)
def test_launch_census_matches_the_recorded_one(backend, engine, cfg):
    want = load_golden()[cfg][backend]
    got, _ = run_steps(engine, cfg)
    assert sorted(got) == sorted(want), (sorted(set(got) ^ set(want)))
    for cls in want:
        diff = {k: (got[cls].get(k, 0), want[cls].get(k, 0)) for k in set(got[cls]) | set(want[cls]) if got[cls].get(k, 0) != want[cls].get(k, 0)}
        assert not diff, (cls, diff)     # label: (launches now, launches recorded)


if __name__ == "__main__":
    # --record emu|gpu: (re)write that backend's entries of the golden from the tree this runs in
    assert len(sys.argv) == 3 and sys.argv[1] == "--record" and sys.argv[2] in ("emu", "gpu"), "usage: test_launch_census.py --record emu|gpu"
    from yolosharp_amd import Engine, build as build_mod
    eng = Engine(lib_path=build_mod.build_emu()) if sys.argv[2] == "emu" else Engine()
    gold = load_golden() if os.path.exists(GOLDEN) else {}
    for c in CONFIGS:
        gold.setdefault(c, {})[sys.argv[2]] = run_steps(eng, c)[0]
    save_golden(gold)
