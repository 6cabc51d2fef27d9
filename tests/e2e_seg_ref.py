"""End2End Segment oracle (TEST INFRASTRUCTURE) on top of oracle.yolo_oracle's Segment graphs.

  towers      Segment.one2one_init (Modules/Head.cs:245-357) puts the SAME cv2 / cv3 / cv4 Sequentials into the one2one lists: the one2one branch
              is the head's three towers run a second time on [xi.detach()] (Head.cs:89-106, 283-307).  Proto runs ONCE; one2many["proto"] = proto,
              one2one["proto"] = proto.detach().  Every BatchNorm of the towers moves its running statistics twice per training forward, Proto's once.
  assigner    TaskAlignedAssigner with tal_topk2 = 1 (Utils/Tal.cs:242-250): after select_highest_overlaps, align_metric * mask_pos, topk(1) over the
              anchors of every (image, box) row, mask_pos *= scatter(index).
  loss        E2ESegmentLoss (Utils/Loss.cs:1179-1236) = o2m * v8SegmentationLoss(tal_topk 10)(one2many) + o2o * v8SegmentationLoss(tal_topk 7,
              tal_topk2 1)(one2one); o2m = 0.8, o2o = 0.2 until update() moves them.
  inference   _inference on the one2one branch with xyxy boxes, cat the mask coefficients (Head.cs:107-127, 309-313), then Segment.postprocess:
              get_topk_index on the class scores and a gather of the boxes AND the nm coefficients by the same anchor index (Head.cs:321-339).
ATen's topk leaves the order among equal values open; the rule fixed for this build is (value descending, index ascending), which a stable
descending sort implements -- the restatement uses stable sorts throughout.
"""
import numpy as np
import torch
import torch.nn as nn

from e2e_ref import topk_stable
from oracle import yolo_oracle as O


def keep_best(align, mask_pos, gt_count=None):
    """Tal.cs:244-248 with topk2 = 1 and a stable descending sort: align [B, G, A], mask_pos [B, G, A] (0 / 1) -> the pruned mask.
    Rows at or beyond gt_count[b] (when given) are returned as they came."""
    mp = mask_pos.to(align.dtype)
    idx = torch.sort(align * mp, dim=-1, descending=True, stable=True).indices[..., :1]
    out = mp * torch.zeros_like(mp).scatter_(-1, idx, 1.0)
    if gt_count is not None:
        live = torch.arange(mp.shape[1])[None, :, None] < torch.as_tensor(gt_count).view(-1, 1, 1)
        out = torch.where(live, out, mp)
    return out


class KeepBestAssigner(O.TaskAlignedAssigner):
    """TaskAlignedAssigner(topk, topk2 = 1): the second stage runs inside select_highest_overlaps, after the multi-box resolution
    (Tal.cs:231-250); everything downstream (target_gt_idx, pos_align, pos_overlaps, the normalised scores) reads the pruned mask."""

    @torch.no_grad()
    def forward(self, pd_scores, pd_bboxes, anc_points, gt_labels, gt_bboxes, mask_gt):
        self.bs, self.n_max = pd_scores.shape[0], gt_bboxes.shape[1]
        if self.n_max == 0:
            return O.TaskAlignedAssigner.forward(self, pd_scores, pd_bboxes, anc_points, gt_labels, gt_bboxes, mask_gt)
        mask_in_gts = self.select_candidates_in_gts(anc_points, gt_bboxes, mask_gt)
        self._align, _ = self.get_box_metrics(pd_scores, pd_bboxes, gt_labels, gt_bboxes, mask_in_gts * mask_gt)
        return O.TaskAlignedAssigner.forward(self, pd_scores, pd_bboxes, anc_points, gt_labels, gt_bboxes, mask_gt)

    def select_highest_overlaps(self, mask_pos, overlaps):
        _, _, mask_pos = O.TaskAlignedAssigner.select_highest_overlaps(self, mask_pos, overlaps)
        self.fg_before = mask_pos.sum(-2)
        self.mask_before, self.align_before = mask_pos.clone(), self._align.clone()
        mask_pos = keep_best(self._align, mask_pos)
        return mask_pos.argmax(-2), mask_pos.sum(-2), mask_pos


def seg_loss(nc, topk, topk2=None, **kw):
    crit = O.v8SegmentationLoss(nc, tal_topk=topk, **kw)
    if topk2 is not None:
        assert topk2 == 1
        crit.assigner = KeepBestAssigner(topk=topk, num_classes=nc, alpha=0.5, beta=6.0, stride=crit.stride)
    return crit


class E2ESegmentLoss:
    def __init__(self, nc, epochs=100):
        self.one2many = seg_loss(nc, 10)
        self.one2one = seg_loss(nc, 7, 1)
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


class E2ESeg(nn.Module):
    """Wraps an oracle Yolov8Segment / Yolov11Segment.  forward(x) -> (inference, {"one2many": preds, "one2one": preds}); inference (eval only) =
    {"pred": [B, 4+nc+nm, A] xyxy * stride | sigmoid scores | raw coefficients, "boxes": postprocess(pred) [B, k, 6+nm], "proto"}."""

    def __init__(self, net, max_det=300):
        super().__init__()
        self.net, self.max_det = net, max_det

    def forward(self, x):
        head = self.net.model[-1]
        seen = {}
        hook = head.register_forward_pre_hook(lambda mod, inp: seen.setdefault("feats", inp[0]))
        try:
            _, one2many = self.net(x)                                       # the three towers + Proto (Head.cs:283-290)
        finally:
            hook.remove()
        feats = [f.detach() for f in seen["feats"]]                         # Head.cs:94
        bs = feats[0].shape[0]
        _, one2one = O.Detect.forward(head, feats)                          # cv2 / cv3 again
        one2one["mask_coefficient"] = torch.cat([head.cv4[i](feats[i]).view(bs, head.nm, -1) for i in range(head.nl)], 2)   # cv4 again
        one2one["proto"] = one2many["proto"].detach()                       # Proto ran once (Head.cs:297)
        preds = {"one2many": one2many, "one2one": one2one}
        if head.training:
            return None, preds
        anchors, strides = O.make_anchors(one2one["feats"], head.stride, 0.5)
        dbox = O.dist2bbox(head.dfl(one2one["boxes"]), anchors.transpose(0, 1).unsqueeze(0), xywh=False, dim=1) * strides.transpose(0, 1)
        pred = torch.cat((dbox, one2one["scores"].sigmoid(), one2one["mask_coefficient"]), 1)
        rows, _ = postprocess(pred, head.nc, self.max_det)
        return {"pred": pred, "boxes": rows, "proto": one2one["proto"]}, preds


def postprocess(pred, nc, max_det=300):
    """pred [B, 4+nc+extra, A] -> (rows [B, k, 6+extra] = (box, score, class, extra channels of the anchor), anchor index [B, k])."""
    B, C, A = pred.shape
    extra = C - 4 - nc
    boxes, scores, mc = pred.permute(0, 2, 1).split((4, nc, extra), dim=-1)
    k = min(int(max_det), A)
    _, ori = topk_stable(scores.amax(-1), k)
    gathered = scores.gather(1, ori.unsqueeze(-1).expand(-1, -1, nc))
    sc, index = topk_stable(gathered.flatten(1), k)
    idx = ori.gather(1, torch.div(index, nc, rounding_mode="floor"))
    rows = torch.cat((boxes.gather(1, idx.unsqueeze(-1).expand(-1, -1, 4)), sc.unsqueeze(-1), (index % nc).unsqueeze(-1).to(pred.dtype),
                      mc.gather(1, idx.unsqueeze(-1).expand(-1, -1, extra))), -1)
    return rows, idx


def select(rows, conf_thres, max_det=300):
    """Ops.cs:258-267 per image: pred[pred[:, 4] > conf_thres][:max_det]."""
    return [r[r[:, 4] > conf_thres][:max_det] for r in rows]
