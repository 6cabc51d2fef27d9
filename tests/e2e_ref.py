"""End2End oracle (TEST INFRASTRUCTURE): Detect with end2end = true on top of oracle.yolo_oracle's graphs.

  towers      Detect.one2one_init (Modules/Head.cs:152-167) puts the SAME cv2 / cv3 Sequentials into the one2one lists, so the one2one branch
              is the head's own modules run a second time on [xi.detach()] (Head.cs:89-106): shared parameters, every BatchNorm of the towers
              updated twice per training forward, no gradient from the one2one branch into the feature maps.
  loss        E2EDetectLoss (Utils/Loss.cs:1094-1118) = v8DetectionLoss(tal_topk 10)(one2many) + v8DetectionLoss(tal_topk 1)(one2one), unweighted.
  inference   _inference on the one2one branch with dist2bbox(xywh = false) (Head.cs:199-223), then postprocess / get_topk_index with
              agnostic_nms = false (Head.cs:117-127, 175-196) -> [B, k, 6], and Ops.non_max_suppression(end2end: true) (Utils/Ops.cs:258-267).
ATen's topk leaves the order among equal values open; the rule fixed for this build is (value descending, index ascending), which a stable
descending sort implements -- the restatement below uses stable sorts throughout.
"""
import torch
import torch.nn as nn

from oracle import yolo_oracle as O


class E2E(nn.Module):
    """Wraps an oracle Yolov8 / Yolov11 detect model.  forward(x) -> (inference, {"one2many": preds, "one2one": preds});
    inference (eval only) = {"pred": [B, 4+nc, A] xyxy * stride | sigmoid scores, "boxes": postprocess(pred) [B, k, 6]}."""

    def __init__(self, net, max_det=300):
        super().__init__()
        self.net, self.max_det = net, max_det

    def forward(self, x):
        head = self.net.model[-1]
        seen = {}
        hook = head.register_forward_pre_hook(lambda mod, inp: seen.setdefault("feats", inp[0]))
        try:
            _, one2many = self.net(x)                                       # forward_head(x, one2many) (Head.cs:91)
        finally:
            hook.remove()
        training = head.training
        _, one2one = head([f.detach() for f in seen["feats"]])              # same modules, detached input (Head.cs:94-96)
        preds = {"one2many": one2many, "one2one": one2one}
        if training:
            return None, preds
        anchors, strides = O.make_anchors(one2one["feats"], head.stride, 0.5)
        dbox = O.dist2bbox(head.dfl(one2one["boxes"]), anchors.transpose(0, 1).unsqueeze(0), xywh=False, dim=1) * strides.transpose(0, 1)
        pred = torch.cat((dbox, one2one["scores"].sigmoid()), 1)
        rows, _ = postprocess(pred, self.max_det)
        return {"pred": pred, "boxes": rows}, preds


class E2EDetectLoss:
    def __init__(self, nc):
        self.one2many = O.v8DetectionLoss(nc, tal_topk=10)
        self.one2one = O.v8DetectionLoss(nc, tal_topk=1)

    def __call__(self, preds, batch):
        l1, i1 = self.one2many(preds["one2many"], batch)
        l2, i2 = self.one2one(preds["one2one"], batch)
        return l1 + l2, i1 + i2


def topk_stable(v, k):
    """The k first entries along the last dim in (value descending, index ascending) order: (values, indices)."""
    order = torch.sort(v, dim=-1, descending=True, stable=True).indices[..., :k]
    return v.gather(-1, order), order


def postprocess(pred, max_det=300):
    """pred [B, 4+nc, A] -> (rows [B, k, 6] = (box, score, class), anchor index [B, k]), k = min(max_det, A)."""
    B, C, A = pred.shape
    nc = C - 4
    boxes, scores = pred.permute(0, 2, 1).split((4, nc), dim=-1)
    k = min(int(max_det), A)
    _, ori = topk_stable(scores.amax(-1), k)                                               # [B, k]
    gathered = scores.gather(1, ori.unsqueeze(-1).expand(-1, -1, nc))                      # [B, k, nc]
    sc, index = topk_stable(gathered.flatten(1), k)
    idx = ori.gather(1, torch.div(index, nc, rounding_mode="floor"))
    rows = torch.cat((boxes.gather(1, idx.unsqueeze(-1).expand(-1, -1, 4)), sc.unsqueeze(-1), (index % nc).unsqueeze(-1).to(pred.dtype)), -1)
    return rows, idx


def select(rows, conf_thres, max_det=300):
    """Ops.cs:258-267 per image: pred[pred[:, 4] > conf_thres][:max_det] -> list of [n_i, 6]."""
    return [r[r[:, 4] > conf_thres][:max_det] for r in rows]
