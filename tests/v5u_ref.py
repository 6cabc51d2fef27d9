"""Yolov5u oracle (TEST INFRASTRUCTURE): a torch restatement of the reference's Yolov5u graph and its C3 block, built from oracle/yolo_oracle.py's Conv, SPPF,
Detect and v8DetectionLoss where their signatures fit.  Own pieces: the stem Conv2d(3, c, 6, 2, 2) (the oracle's Conv only knows autopad k // 2) and
Bottleneck(k = (1, 3)).

  Models/Yolo.cs:137-198   class Yolov5u : Yolov8
    :139      outputIndexs {4, 6, 10, 14, 17, 20, 23}; concatIndex is Yolov8's {1, 0, 3, 2} (:14)
    :147-155  (depth_multiple, width_multiple) per size: n (0.34, 0.25)  s (0.34, 0.5)  m (0.67, 0.75)  l (1.0, 1.0)  x (1.34, 1.25)
    :157      widths = int(w * width_multiple) for {64, 128, 256, 512, 1024} -- NO max_channels clamp
    :158      depths = int(d * depth_multiple) for {3, 6, 9}, in float arithmetic
    :163-172  backbone: Conv(3, w0, 6, 2, 2), Conv(w0, w1, 3, 2), C3(w1, w1, d0), Conv(w1, w2, 3, 2), C3(w2, w2, d1), Conv(w2, w3, 3, 2), C3(w3, w3, d2),
              Conv(w3, w4, 3, 2), C3(w4, w4, d0), SPPF(w4, w4, 5)
    :175-191  head: Conv(w4, w3, 1, 1), Upsample, Concat, C3(w4, w3, d0, false), Conv(w3, w2, 1, 1), Upsample, Concat, C3(w3, w2, d0, false),
              Conv(w2, w2, 3, 2), Concat, C3(w3, w3, d0, false), Conv(w3, w3, 3, 2), Concat, C3(w4, w4, d0, false)
    :193      Detect(nc, ch = (w2, w3, w4)) as model.24
  Modules/Block.cs:404-442  class C3
    :424      c_ = int(c2 * e), e = 0.5
    :425-427  cv1 = Conv(c1, c_, 1, 1), cv2 = Conv(c1, c_, 1, 1), cv3 = Conv(2 c_, c2, 1)
    :429      m = Sequential(n x Bottleneck(c_, c_, k = (1, 3), shortcut, e = 1.0))
    :440      cv3(cat(m(cv1(x)), cv2(x)))
  Modules/Block.cs:572-608  class Bottleneck: cv1 = Conv(c1, c_, k[0], 1), cv2 = Conv(c_, c2, k[1], 1), add = shortcut and c1 == c2
  Models/Detector.cs:17     never passes yoloSize for Yolov5u: a reference v5u detector is always size n.  The size parameter is kept here and in the engine.
"""
import numpy as np
import torch
import torch.nn as nn

from oracle import yolo_oracle as O

SIZES5 = {"n": (0.34, 0.25), "s": (0.34, 0.5), "m": (0.67, 0.75), "l": (1.0, 1.0), "x": (1.34, 1.25)}     # Yolo.cs:147-155


def _f32mul(a, m):
    return int(np.float32(a) * np.float32(m))       # the reference multiplies in float (Yolo.cs:157-158)


class StemConv(O.Conv):
    """Convs.Conv(3, c2, 6, 2, 2) (Yolo.cs:163): the oracle's Conv unit with the explicit padding 2 instead of autopad's 6 // 2."""

    def __init__(self, c1, c2):
        super().__init__(c1, c2, 6, 2)
        self.conv = nn.Conv2d(c1, c2, 6, 2, 2, bias=False)


class Bottleneck13(nn.Module):
    """Block.Bottleneck(c1, c2, shortcut, k = (1, 3), e) (Block.cs:572-608 as C3 builds it, :429)."""

    def __init__(self, c1, c2, shortcut=True, e=1.0):
        super().__init__()
        c_ = int(c2 * e)
        self.cv1 = O.Conv(c1, c_, 1, 1)
        self.cv2 = O.Conv(c_, c2, 3, 1)
        self.add = shortcut and c1 == c2

    def forward(self, x):
        return x + self.cv2(self.cv1(x)) if self.add else self.cv2(self.cv1(x))


class C3(nn.Module):
    """Block.cs:404-442; registration order cv1, cv2, cv3, m."""

    def __init__(self, c1, c2, n=1, shortcut=True, e=0.5):
        super().__init__()
        c_ = int(c2 * e)
        self.cv1 = O.Conv(c1, c_, 1, 1)
        self.cv2 = O.Conv(c1, c_, 1, 1)
        self.cv3 = O.Conv(2 * c_, c2, 1)
        self.m = nn.Sequential(*(Bottleneck13(c_, c_, shortcut, e=1.0) for _ in range(n)))

    def forward(self, x):
        return self.cv3(torch.cat((self.m(self.cv1(x)), self.cv2(x)), 1))


class Yolov5u(O.Yolov8):
    """Models/Yolo.cs:137-198.  forward is the oracle Yolov8's router (Yolo.cs:92-134) over this list."""

    def __init__(self, nc=80, reg_max=16, size="n"):
        nn.Module.__init__(self)
        dm, wm = SIZES5[size]
        w = [_f32mul(x, wm) for x in (64, 128, 256, 512, 1024)]
        d = [_f32mul(x, dm) for x in (3, 6, 9)]
        up = lambda: nn.Upsample(scale_factor=2, mode="nearest")
        self.model = nn.ModuleList([
            StemConv(3, w[0]), O.Conv(w[0], w[1], 3, 2), C3(w[1], w[1], d[0]), O.Conv(w[1], w[2], 3, 2),
            C3(w[2], w[2], d[1]), O.Conv(w[2], w[3], 3, 2), C3(w[3], w[3], d[2]), O.Conv(w[3], w[4], 3, 2),
            C3(w[4], w[4], d[0]), O.SPPF(w[4], w[4], 5),
            O.Conv(w[4], w[3], 1, 1), up(), nn.Identity(), C3(w[4], w[3], d[0], False),
            O.Conv(w[3], w[2], 1, 1), up(), nn.Identity(), C3(w[3], w[2], d[0], False),
            O.Conv(w[2], w[2], 3, 2), nn.Identity(), C3(w[3], w[3], d[0], False),
            O.Conv(w[3], w[3], 3, 2), nn.Identity(), C3(w[4], w[4], d[0], False),
            O.Detect(nc, reg_max, (w[2], w[3], w[4]))])
        self.cat_layers = (12, 16, 19, 22)
        self.output_idx = (4, 6, 10, 14, 17, 20, 23)     # Yolo.cs:139
        self.concat_idx = (1, 0, 3, 2)                   # Yolo.cs:14


def make_ref(nc=80, size="n", seed=0):
    """A Yolov5u with PyTorch-default weights from `seed` and randomised BatchNorm affine / running statistics (test_model.make_ref's recipe)."""
    torch.manual_seed(seed)
    ref = Yolov5u(nc=nc, size=size)
    for mod in ref.modules():
        if isinstance(mod, nn.BatchNorm2d):
            mod.weight.data.uniform_(0.5, 1.5); mod.bias.data.normal_(0, 0.1)
            mod.running_mean.normal_(0, 0.1); mod.running_var.uniform_(0.5, 1.5)
    return ref
