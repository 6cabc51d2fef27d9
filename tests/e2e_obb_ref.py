"""End2End OBB oracle (TEST INFRASTRUCTURE) on top of oracle.yolo_oracle's Obb graphs, tests/e2e_ref.py and tests/e2e_seg_ref.py.

  towers      Obb.one2one_init (Modules/Head.cs:454-469) puts the SAME cv2 / cv3 / cv4 Sequentials into the one2one lists: the one2one branch is the
              head's three towers run a second time on [xi.detach()] (Head.cs:89-106).  There is no Proto.  Every BatchNorm of the towers moves its
              running statistics twice per training forward.
  assigner    RotatedTaskAlignedAssigner with tal_topk2 = 1 (Utils/Tal.cs:242-250, 260-310): RotKeep = the keep-best stage of e2e_seg_ref on the
              rotated in-box test and probiou overlaps.  The thin-box widening (Tal.cs:283-287) edits the padded GT in place; each criterion pads its own.
  loss        E2EOBBLoss (Utils/Loss.cs:1120-1177) = o2m * v8OBBLoss(tal_topk 10)(one2many) + o2o * v8OBBLoss(tal_topk 7, tal_topk2 1)(one2one);
              o2m = 0.8, o2o = 0.2 until update() moves them -- the one criterion whose update() the reference's loop calls (YoloBaseTaskModel.cs:350-353).
  inference   Obb.decode_bboxes ignores end2end (Head.cs:434-437): pred = (xywh of dist2rbox * stride, sigmoid scores, angle), then Obb.postprocess
              (Head.cs:439-452) = get_topk_index on the class scores and a gather of the box AND the angle by the same anchor index: rows
              (cx, cy, w, h, score, class, angle) -- e2e_seg_ref.postprocess with one extra channel.
"""
import numpy as np
import torch
import torch.nn as nn

import e2e_seg_ref as S
from oracle import yolo_oracle as O


class RotKeep(S.KeepBestAssigner, O.RotatedTaskAlignedAssigner):
    """RotatedTaskAlignedAssigner(topk, topk2 = 1).  KeepBestAssigner names TaskAlignedAssigner.forward / select_highest_overlaps explicitly; both
    reach select_candidates_in_gts and iou_calculation through self, so the MRO gives them the rotated versions."""

    def select_highest_overlaps(self, mask_pos, overlaps):
        out = S.KeepBestAssigner.select_highest_overlaps(self, mask_pos, overlaps)
        self.fg_after = out[1]
        return out


def obb_loss(nc, topk, topk2=None, **kw):
    crit = O.v8OBBLoss(nc, tal_topk=topk, **kw)
    if topk2 is not None:
        assert topk2 == 1
        crit.assigner = RotKeep(topk=topk, num_classes=nc, alpha=0.5, beta=6.0, stride=crit.stride)
    return crit


class E2EOBBLoss:
    def __init__(self, nc, epochs=100):
        self.one2many = obb_loss(nc, 10)
        self.one2one = obb_loss(nc, 7, 1)
        self.updates, self.epochs = 0, epochs
        self.o2m = np.float32(0.8)
        self.o2o = np.float32(1.0) - self.o2m

    def __call__(self, preds, batch):
        l1, i1 = self.one2many(preds["one2many"], batch)
        l2, i2 = self.one2one(preds["one2one"], batch)
        return l1 * float(self.o2m) + l2 * float(self.o2o), i2 * float(self.o2o) + i1 * float(self.o2m)

    def update(self):
        f = np.float32
        self.updates += 1
        self.o2m = f(max(f(1) - f(self.updates) / f(max(self.epochs - 1, 1)), f(0))) * (f(0.8) - f(0.1)) + f(0.1)
        self.o2o = f(max(f(1.0) - self.o2m, f(0)))


class E2EObb(nn.Module):
    """Wraps an oracle Yolov8Obb / Yolov11Obb.  forward(x) -> (inference, {"one2many": preds, "one2one": preds}); inference (eval only) =
    {"pred": [B, 4+nc+1, A] (the one2one branch's plain Obb inference tensor), "boxes": postprocess(pred) [B, k, 7]}."""

    def __init__(self, net, max_det=300):
        super().__init__()
        self.net, self.max_det = net, max_det

    def forward(self, x):
        head = self.net.model[-1]
        seen = {}
        hook = head.register_forward_pre_hook(lambda mod, inp: seen.setdefault("feats", inp[0]))
        try:
            _, one2many = self.net(x)                                       # cv2 / cv3 / cv4 on x
        finally:
            hook.remove()
        feats = [f.detach() for f in seen["feats"]]                         # Head.cs:94
        inf, one2one = O.Obb.forward(head, feats)                           # the three towers again
        preds = {"one2many": one2many, "one2one": one2one}
        if head.training:
            return None, preds
        rows, _ = S.postprocess(inf["boxes"], head.nc, self.max_det)
        return {"pred": inf["boxes"], "boxes": rows}, preds
