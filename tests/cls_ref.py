"""Classification oracle (TEST INFRASTRUCTURE): Yolov8Classify / Yolov11Classify built from oracle.yolo_oracle's graphs.

  Yolov8Classify  = Yolov8(...).model[:9]  (model.0-8, no SPPF; Models/Yolo.cs:537-554) + Classify(widths[4], nc) as model.9
  Yolov11Classify = Yolov11(...).model[:11] (model.0-10, SPPF and C2PSA kept; Yolo.cs:556-573) + Classify as model.11
  Classify        = Conv(c1, 1280, 1) -> AdaptiveAvgPool2d(1) -> flatten -> Dropout(0) -> Linear(1280, nc) (Modules/Head.cs:612-644)
  loss            = F.cross_entropy(logits, cls, mean) (Utils/Loss.cs:1073-1091)
The backbones have no skip routing before the neck, so a plain sequential forward is the reference's Yolo.forward for these lists.
"""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle import yolo_oracle as O


class Classify(nn.Module):
    def __init__(self, c1, nc):
        super().__init__()
        c_ = 1280
        self.conv = O.Conv(c1, c_, 1, 1)
        self.pool = nn.AdaptiveAvgPool2d(1)
        self.drop = nn.Dropout(p=0.0)
        self.linear = nn.Linear(c_, nc)

    def forward(self, x):
        x = self.linear(self.drop(self.pool(self.conv(x)).flatten(1)))
        return (None, {"cls": x}) if self.training else ({"cls": x.softmax(1)}, {"cls": x})


class _ClassifyNet(nn.Module):
    def forward(self, x):
        for mod in self.model[:-1]:
            x = mod(x)
        return self.model[-1](x)


class Yolov8Classify(_ClassifyNet):
    def __init__(self, nc=80, size="n"):
        super().__init__()
        base = O.Yolov8(nc=nc, size=size)
        c1 = base.model[8].cv2.conv.out_channels
        self.model = nn.ModuleList(list(base.model[:9]) + [Classify(c1, nc)])


class Yolov11Classify(_ClassifyNet):
    def __init__(self, nc=80, size="n"):
        super().__init__()
        base = O.Yolov11(nc=nc, size=size)
        c1 = base.model[10].cv2.conv.out_channels
        self.model = nn.ModuleList(list(base.model[:11]) + [Classify(c1, nc)])


def make_ref(family, nc, size, seed=0):
    """The oracle with non-trivial BatchNorm parameters and running statistics (like the other task tests)."""
    torch.manual_seed(seed)
    ref = (Yolov8Classify if family == 8 else Yolov11Classify)(nc=nc, size=size)
    for mod in ref.modules():
        if isinstance(mod, nn.BatchNorm2d):
            mod.weight.data.uniform_(0.5, 1.5); mod.bias.data.normal_(0, 0.1)
            mod.running_mean.normal_(0, 0.1); mod.running_var.uniform_(0.5, 1.5)
    return ref


def val_reference(prob_batches, target_batches, nc):
    """Classifier.Val's metric (Classifier.cs:95-118) restated in numpy: top-min(nc, 5) of argsort descending, then top-1 / top-5."""
    n5 = min(nc, 5)
    pred = np.concatenate([np.argsort(-p, axis=1, kind="stable")[:, :n5] for p in prob_batches])
    tgt = np.concatenate([np.asarray(t, np.float32).reshape(-1) for t in target_batches])
    correct = (tgt[:, None] == pred).astype(np.float32)
    return float(correct[:, 0].mean()), float(correct.max(1).mean())


def loss(logits, cls):
    return F.cross_entropy(logits, torch.as_tensor(np.asarray(cls), dtype=torch.long).view(-1), reduction="mean")
