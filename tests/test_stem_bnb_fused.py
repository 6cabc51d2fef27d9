"""model.0's BatchNorm (+ SiLU) backward inside its weight-gradient kernel (conv_stem.hip stem_wgrad_kernel, FUSE; STEM_BNB_FUSE=1) against the separate
bn_bwd_apply pass (STEM_BNB_FUSE=0): the kernel forms the same bf16 dy numbers from dz and y with the same expression and feeds them to the same MFMA
order, so the statement is BIT-IDENTITY of every parameter gradient (the one that can move is model.0.conv.weight; model.0's BatchNorm gradients come
from the finalize launch, which both forms run).

Sizes: 64 x 64, B = 2 -- the stem output is 32 x 32, exact 8 x 32 tiles; 96 x 160, B = 3 -- 48 x 80, a ragged right tile (its units outside the
image must stay zero, not -k2).

Which form ran is asserted, not assumed: the fused launch records the kernel-profile class "stem_bnb" (conv_stem.hip ys_stem_wgrad_launch), so a model that quietly
fell back to the separate pass -- and would pass every comparison against itself -- fails the launch count."""
import numpy as np
import pytest

from conftest import BACKENDS

NC = 80
SIZES = [(64, 64, 2), (96, 160, 3)]


def _labels(B, seed=1):
    import bench
    return bench.synth_labels(B, NC, seed=seed, kmax=4)


def _model(engine, H, W, B, fuse, dtype="bf16", overlap=True):
    from yolosharp_amd.model import Yolov8, v8DetectionLoss
    with engine.options(STEM_BNB_FUSE=fuse):          # read when the model is created
        m = Yolov8(engine, nc=NC, size="n", height=H, width=W, max_batch=B, dtype=dtype)
    m.init_weights(2)
    m.train()
    if not overlap:
        m.set_overlap(False)
    return m, v8DetectionLoss(m)


def _image(H, W, B):
    return np.random.default_rng(0).random((B, 3, H, W), dtype=np.float32)


def _grads_after(engine, H, W, B, fuse, overlap, passes=1, segments=False):
    """`passes` x (forward -> loss -> backward) on device-resident inputs, nothing read and nothing synchronised in between; then every gradient.
    segments: the backward as ys_model_backward_segment_async calls (the data-parallel step's form: model.0's weight gradient goes to the second stream)."""
    m, crit = _model(engine, H, W, B, fuse, overlap=overlap)
    bi, cl, bb = _labels(B)
    d_img = engine.to_device(_image(H, W, B))
    d_lab = (engine.to_device(bi), engine.to_device(cl), engine.to_device(bb), len(bi))
    m.zero_grad()
    engine.kernel_profile(True)                      # event records on the launch streams: nothing waits on them until the read below
    for _ in range(passes):
        m.forward_device(d_img, B)
        crit.forward_device(*d_lab)
        if segments:
            for sg in range(m.num_segments()):
                m.backward_segment_async(sg)
        else:
            m.backward()
    g = m.grads()
    items = crit.read()[1]
    n_fused = engine.kernel_profile_read("stem_bnb")[0]
    engine.kernel_profile(False)
    assert n_fused == (passes if fuse else 0), "fused stem launches: %d in %d passes with STEM_BNB_FUSE=%d" % (n_fused, passes, fuse)
    m.close()
    for p in (d_img,) + d_lab[:3]:
        engine.free(p)
    return g, items


def _equal(ga, gb):
    assert sorted(ga) == sorted(gb)
    for k in ga:
        assert np.isfinite(ga[k]).all(), k
        assert np.array_equal(ga[k], gb[k]), (k, float(np.abs(ga[k] - gb[k]).max()))
    assert np.abs(ga["model.0.conv.weight"]).max() > 0


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("overlap", [True, False], ids=["overlap", "one_stream"])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d_b%d" % s)
def test_fused_stem_bn_backward_gives_the_same_gradients(engine, backend, size, overlap):
    H, W, B = size
    (gf, itf), (gp, itp) = _grads_after(engine, H, W, B, 1, overlap), _grads_after(engine, H, W, B, 0, overlap)
    assert np.array_equal(itf, itp)
    _equal(gf, gp)


@pytest.mark.parametrize("backend", BACKENDS)
def test_back_to_back_steps_without_optimizer_or_sync(engine, backend):
    """The ordering the fused form needs: wherever its weight-gradient launch runs on the second stream it reads model.0's raw output and the gradient
    map of its output after the backward call has returned, so the next forward (which rewrites the first) and the next backward's dgrad of model.1
    (which rewrites the second) must be ordered behind it -- they join the stream (model.hip forward_impl, model_api.hip ys_model_backward).  Two passes with no optimizer
    step, no read and no synchronisation in between accumulate two identical gradient contributions; the result must equal the same sequence with
    the separate pass, and two fresh models must agree with each other.  (A pass does not prove the ordering -- the join in the code does; a
    missing one has a chance to show here.)"""
    H, W, B = 64, 64, 2
    a, _ = _grads_after(engine, H, W, B, 1, True, passes=2)
    b, _ = _grads_after(engine, H, W, B, 1, True, passes=2)
    p, _ = _grads_after(engine, H, W, B, 0, True, passes=2)
    _equal(a, b)
    _equal(a, p)


@pytest.mark.parametrize("backend", BACKENDS)
def test_segmented_backward_hands_the_fused_launch_to_the_second_stream(engine, backend):
    """ys_model_backward runs the fused launch on the main stream (backward_range: the stem is the step's tail and that stream has nothing else left); the
    per-segment calls queue it for the second stream like every other weight gradient.  Two passes back to back, as above."""
    H, W, B = 64, 64, 2
    a, _ = _grads_after(engine, H, W, B, 1, True, passes=2, segments=True)
    p, _ = _grads_after(engine, H, W, B, 0, True, passes=2, segments=True)
    _equal(a, p)


@pytest.mark.parametrize("backend", BACKENDS)
def test_packed_input_step_takes_the_separate_pass(engine, backend):
    """A training forward fed with uint8 planes packs its input: the stem kernels have no fp32 image to read, so a model planned for the fused form runs the
    generic weight-gradient kernel behind the separate apply pass (the unit's dy goes to the shared scratch buffer: no buffer of its own was planned) -- the
    gradients of STEM_BNB_FUSE=0."""
    H, W, B = 64, 64, 2
    img = (np.random.default_rng(0).random((B, 3, H, W)) * 255).astype(np.uint8)
    bi, cl, bb = _labels(B)
    out = []
    for fuse in (1, 0):
        m, crit = _model(engine, H, W, B, fuse)
        m.zero_grad()
        engine.kernel_profile(True)
        m.forward_u8(img)
        crit.forward(None, {"batch_idx": bi, "cls": cl, "bboxes": bb})
        m.backward()
        out.append(m.grads())
        assert engine.kernel_profile_read("stem_bnb")[0] == 0, "a packed-input step has no fp32 image for the fused launch"
        engine.kernel_profile(False)
        m.close()
    _equal(out[0], out[1])


@pytest.mark.parametrize("backend", BACKENDS)
def test_fp8_train_steps_are_unchanged(engine, backend):
    """fp8 mode keeps model.0 on the bf16 kernels (its BatchNorm backward never writes an e5m2 image), so the fused form runs there as well: two
    train steps -- the second one's loss sees the first one's stem weight gradient through AdamW -- give the same loss items with the switch on and off."""
    from yolosharp_amd.model import AMPWrapper
    H, W, B = 64, 64, 2
    bi, cl, bb = _labels(B)
    batch = {"batch_idx": bi, "cls": cl, "bboxes": bb}
    out = []
    for fuse in (1, 0):
        m, crit = _model(engine, H, W, B, fuse, dtype="fp8")
        amp = AMPWrapper(m)
        engine.kernel_profile(True)
        out.append([np.asarray(amp.TrainStep(_image(H, W, B), batch, crit)[1]).copy() for _ in range(2)])
        assert engine.kernel_profile_read("stem_bnb")[0] == (2 if fuse else 0)
        engine.kernel_profile(False)
        m.close()
    for s in range(2):
        assert np.isfinite(out[0][s]).all()
        assert np.array_equal(out[0][s], out[1][s]), (s, out[0][s], out[1][s])
