"""The key table of ys_model_get_output, pinned through ys_model_set_preds: what a caller hands in as head outputs is what every forward key
returns (fp32: exactly; bf16: rounded once to the storage format), the one2one keys of an End2End model return the one2many arrays (aliased
towers, Head.cs:152-167), and a key of another task, a gradient key before a criterion has run and "det" in training mode are refused.
No convolution runs: the head buffers are written by the pack kernel and read back by the unpack kernel only."""
import numpy as np
import pytest
import torch

from bf16_ref import bf16r
from conftest import BACKENDS
from test_model import relerr

B, H, W, NC = 2, 64, 64, 3                # A = 84 (64 + 16 + 4): C x rows differs between any two keys of a task
TASKS = {"detect": ("Yolov8", None), "segment": ("Yolov8Segment", "mask_coefficient"), "obb": ("Yolov8Obb", "angle"), "pose": ("Yolov8Pose", "kpts")}
FORWARD = {"detect": ("boxes", "scores"), "segment": ("boxes", "scores", "mask_coefficient", "proto"),
           "obb": ("boxes", "scores", "angle"), "pose": ("boxes", "scores", "kpts")}
GRADS = {"detect": ("dboxes", "dscores"), "segment": ("dboxes", "dscores", "dmask_coefficient", "dproto"),
         "obb": ("dboxes", "dscores", "dangle"), "pose": ("dboxes", "dscores", "dkpts")}
O2O_EXTRA = {"detect": (), "segment": ("mask_coefficient",), "obb": ("angle",)}     # one2one keys next to one2one_boxes / one2one_scores
CLASSIFY = ("cls", "logits", "dcls")
CASES = [(t, e) for t in TASKS for e in (False, True) if not (e and t == "pose")]


def _one2one(task):
    vals = ("boxes", "scores") + O2O_EXTRA.get(task, ())
    return tuple("one2one_" + k for k in vals), tuple("one2one_d" + k for k in vals)


def _all_keys():
    keys = set(CLASSIFY)
    for t in TASKS:
        keys |= set(FORWARD[t]) | set(GRADS[t])
        if t in O2O_EXTRA:
            keys |= set(_one2one(t)[0]) | set(_one2one(t)[1])
    return keys


def _end2end(m, task):
    if task == "detect":
        m.one2one_init()
    elif task == "segment":
        m.e2e_init()
    else:
        m.e2e_obb_init()


def _refused(m, key):
    """A key this model does not have is refused for what it is, before its count is looked at (Model.get_output has no shape for such a key)."""
    from yolosharp_amd import YsError, _lib
    from yolosharp_amd.engine import _ptr
    a = np.empty(1, np.float32)
    with pytest.raises(YsError) as e:
        _lib.check(m.lib, m.lib.ys_model_get_output(m.handle, key.encode(), _ptr(a), a.size))
    assert "expected" not in str(e.value), (key, str(e.value))


def _set_preds(m, task, p):
    """Model.set_preds takes an OBB model's angle in radians and inverts it; the logits themselves go through the library's entry."""
    if task != "obb":
        return m.set_preds(p)
    from yolosharp_amd import _lib
    from yolosharp_amd.engine import _ptr
    _lib.check(m.lib, m.lib.ys_model_set_preds(m.handle, B, _ptr(p["boxes"]), _ptr(p["scores"]), _ptr(p["angle"]), None))
    m._batch = B


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("task,end2end", CASES)
def test_set_preds_round_trip(backend, engine, task, end2end, dtype):
    from yolosharp_amd import YsError
    from yolosharp_amd import model as M
    cls, extra = TASKS[task]
    m = getattr(M, cls)(engine, nc=NC, size="n", height=H, width=W, max_batch=B, dtype=dtype)
    if end2end:
        _end2end(m, task)
    A, nm = m.A, m.NM
    assert A == 84
    g = torch.Generator().manual_seed(11)
    draw = lambda *s: torch.randn(*s, generator=g).numpy()
    p = {"boxes": draw(B, 4 * m.reg_max, A), "scores": draw(B, NC, A)}
    if extra:
        p[extra] = draw(B, nm, A)                                  # obb: the angle LOGITS
    if task == "segment":
        p["proto"] = draw(B, nm, H // 4, W // 4)
    _set_preds(m, task, p)
    stored = {k: (v if dtype == "f32" else bf16r(torch.from_numpy(v)).numpy()) for k, v in p.items()}

    # ---- forward keys: what went in comes out
    got = {k: m.get_output(k) for k in FORWARD[task]}
    for k in FORWARD[task]:
        if k == "angle":                                           # Head.cs:429 on the stored logit; the tolerance of test_obb_pose._head_parity
            ref = (1.0 / (1.0 + np.exp(-stored[k].astype(np.float64))) - 0.25) * np.pi
            assert got[k].shape == ref.shape and relerr(got[k], ref) < 1e-3, k
        else:
            assert got[k].shape == stored[k].shape and np.array_equal(got[k], stored[k]), k

    # ---- one2one value keys: the one2many arrays
    o2o_vals, o2o_grads = _one2one(task) if task in O2O_EXTRA else ((), ())
    if end2end:
        for k in o2o_vals:
            assert np.array_equal(m.get_output(k), got[k[len("one2one_"):]]), k

    # ---- refusals
    own = set(FORWARD[task]) | set(GRADS[task]) | (set(o2o_vals) | set(o2o_grads) if end2end else set())
    for k in sorted(_all_keys() - own):                            # another task's key, or a one2one key of a model that is not End2End
        _refused(m, k)
    for k in GRADS[task] + (o2o_grads if end2end else ()):         # no criterion has run on these preds
        with pytest.raises(YsError):
            m.get_output(k)
    assert m.training
    with pytest.raises(YsError):                                   # set_preds leaves the mode alone: "det" belongs to an eval forward
        m.get_output("det")
    m.close()
