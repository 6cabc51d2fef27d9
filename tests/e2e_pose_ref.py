"""End2End Pose oracle (TEST INFRASTRUCTURE) on top of oracle.yolo_oracle's Pose graphs, tests/e2e_ref.py and tests/e2e_seg_ref.py.

  towers      Pose.one2one_init (Modules/Head.cs:565-580) puts the SAME cv2 / cv3 / cv4 Sequentials into the one2one lists: the one2one branch is the
              head's three towers run a second time on [xi.detach()] (Head.cs:89-106).  There is no Proto.  Every BatchNorm of the towers moves its
              running statistics twice per training forward.
  assigner    TaskAlignedAssigner with tal_topk2 = 1 (Utils/Tal.cs:242-250) = e2e_seg_ref.KeepBestAssigner, for the one2one criterion only: the
              one2many v8PoseLoss is built with tal_topk2 = tal_topk = 10 and Tal.cs:242 runs the stage only `if (topk2 != topk)`.
  loss        E2EPoseLoss (Utils/Loss.cs:1238-1295) = o2m * v8PoseLoss(tal_topk 10)(one2many) + o2o * v8PoseLoss(tal_topk 7, tal_topk2 1)(one2one);
              o2m = 0.8, o2o = 0.2 until update() moves them (the reference's loop never calls it for this class, YoloBaseTaskModel.cs:350-353).
  inference   Detect.decode_bboxes under end2end gives xyxy (Head.cs:201), Pose._inference appends kpts_decode (Head.cs:526-530): pred = (xyxy *
              stride, sigmoid scores, decoded keypoints); Pose.postprocess (Head.cs:550-563) = get_topk_index on the class scores and a gather of the
              box AND the nk keypoint values by the same anchor index -- e2e_seg_ref.postprocess with nk extra channels.
  validation  PoseDetector.Val per image (Models/PoseDetector.cs:131-165): box_iou / kpt_iou (area = w * h * 0.53) + match_predictions twice.
"""
import numpy as np
import torch
import torch.nn as nn

import e2e_seg_ref as S
from oracle import yolo_oracle as O


class Keep(S.KeepBestAssigner):
    def select_highest_overlaps(self, mask_pos, overlaps):
        out = S.KeepBestAssigner.select_highest_overlaps(self, mask_pos, overlaps)
        self.fg_after = out[1]
        return out


def pose_loss(nc, kpt_num, kpt_dim, topk, topk2=None, **kw):
    crit = O.v8PoseLoss(nc, kpt_num, kpt_dim, tal_topk=topk, **kw)
    if topk2 is not None:
        assert topk2 == 1
        crit.assigner = Keep(topk=topk, num_classes=nc, alpha=0.5, beta=6.0, stride=crit.stride)
    return crit


class E2EPoseLoss:
    def __init__(self, nc, kpt_num=17, kpt_dim=3, epochs=100):
        self.one2many = pose_loss(nc, kpt_num, kpt_dim, 10)
        self.one2one = pose_loss(nc, kpt_num, kpt_dim, 7, 1)
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


class E2EPose(nn.Module):
    """Wraps an oracle Yolov8Pose / Yolov11Pose.  forward(x) -> (inference, {"one2many": preds, "one2one": preds}); inference (eval only) =
    {"pred": [B, 4+nc+nk, A] xyxy * stride | sigmoid scores | decoded keypoints, "boxes": postprocess(pred) [B, k, 6+nk]}."""

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
        bs = feats[0].shape[0]
        _, one2one = O.Detect.forward(head, feats)                          # cv2 / cv3 again
        one2one["kpts"] = torch.cat([head.cv4[i](feats[i]).view(bs, head.nk, -1) for i in range(head.nl)], 2)   # cv4 again
        preds = {"one2many": one2many, "one2one": one2one}
        if head.training:
            return None, preds
        anchors, strides = O.make_anchors(one2one["feats"], head.stride, 0.5)
        dbox = O.dist2bbox(head.dfl(one2one["boxes"]), anchors.transpose(0, 1).unsqueeze(0), xywh=False, dim=1) * strides.transpose(0, 1)
        kp = head.kpts_decode(one2one["kpts"], anchors.transpose(0, 1), strides.transpose(0, 1))
        pred = torch.cat((dbox, one2one["scores"].sigmoid(), kp), 1)
        rows, _ = S.postprocess(pred, head.nc, self.max_det)
        return {"pred": pred, "boxes": rows}, preds


def val_image(rows, cls, bboxes, keypoints, img_w, img_h, kpt_num, kpt_dim):
    """PoseDetector.cs:133-158 for one image: rows [n, 6+nk] (kept detections), the image's labels -> (iou [nl, n], oks [nl, n], correct_box [n, 10],
    correct_pose [n, 10]).  All tensors fp32."""
    scale = torch.tensor([img_w, img_h, img_w, img_h], dtype=torch.float32)
    gt = O.xywh2xyxy(bboxes * scale)
    iou = O.box_iou(gt, rows[:, :4])
    kp = keypoints
    if kp.shape[-1] == 2:                                                   # :142-146, the "seen" column
        kp = torch.cat((kp, torch.ones(kp.shape[0], kp.shape[1], 1)), -1)
    kp = kp * torch.tensor([img_w, img_h, 1.0])
    area = O.xyxy2xywh(gt)[:, 2:].prod(1) * 0.53
    oks = O.kpt_iou(kp, rows[:, 6:].reshape(-1, kpt_num, kpt_dim), area)
    return iou, oks, O.match_predictions(rows[:, 5], cls, iou), O.match_predictions(rows[:, 5], cls, oks)
