"""Restatement of the reference's default training input in torch, with the dtype as a parameter (float32 = what the reference computes,
float64 = the judge of tests/test_augment.py): Augment.Mosaic._mosaic4 (Data/Augment.cs:158-274), RandomPerspective's
Warp{Affine,Perspective}WithGridSample (:395-538), apply_bboxes (:546-568), apply_keypoints (:581-601), Apply (:664-695), Ops.clip_boxes /
clip_keypoints (Utils/Ops.cs:150-183), FlipLR / FlipUD (:860-966), box_convert + Normalize + mul(1/255) (Data/YoloDataset.cs:102-151,
Data/Struct.cs:99-121) and the collate (Data/YoloDataLoader.cs:18-44).  The canvas IS materialised and torch.nn.functional.grid_sample IS
called, as the reference does.  The random draws are arguments (xc, yc, M, flips): TorchSharp's streams cannot be reproduced.

Two documented deviations of the engine are restated here too: a label-free sample is still warped (Apply returns the unwarped canvas,
:666-669), and where the mask slice of :209 would run past the source mask (the reference throws) the missing part reads 0."""
import torch
import torch.nn.functional as F


def rects(i, xc, yc, h, w, s):
    """:184-203 -> (x1a, y1a, x2a, y2a), (x1b, y1b, x2b, y2b)"""
    if i == 0:
        x1a, y1a, x2a, y2a = max(xc - w, 0), max(yc - h, 0), xc, yc
        x1b, y1b, x2b, y2b = w - (x2a - x1a), h - (y2a - y1a), w, h
    elif i == 1:
        x1a, y1a, x2a, y2a = xc, max(yc - h, 0), min(xc + w, s * 2), yc
        x1b, y1b, x2b, y2b = 0, h - (y2a - y1a), min(w, x2a - x1a), h
    elif i == 2:
        x1a, y1a, x2a, y2a = max(xc - w, 0), yc, xc, min(s * 2, yc + h)
        x1b, y1b, x2b, y2b = w - (x2a - x1a), 0, w, min(y2a - y1a, h)
    else:
        x1a, y1a, x2a, y2a = xc, yc, min(xc + w, s * 2), min(s * 2, yc + h)
        x1b, y1b, x2b, y2b = 0, 0, min(w, x2a - x1a), min(y2a - y1a, h)
    return (x1a, y1a, x2a, y2a), (x1b, y1b, x2b, y2b)


def mosaic4(imgs, masks, xc, yc, s, r):
    """imgs: four uint8 [3, h, w]; masks: four uint8 [mh, mw] or None entries.  -> img4 uint8 [3, 2s, 2s], mask4 uint8 [1, 2s/r, 2s/r], pads [(padw, padh)] * 4"""
    img4 = torch.full((3, 2 * s, 2 * s), 114, dtype=torch.uint8)
    mask4 = torch.zeros((1, 2 * s // r, 2 * s // r), dtype=torch.uint8)
    pads = []
    for i in range(4):
        img = imgs[i]
        h, w = img.shape[1:]
        (x1a, y1a, x2a, y2a), (x1b, y1b, x2b, y2b) = rects(i, xc, yc, h, w, s)
        img4[..., y1a:y2a, x1a:x2a] = img[..., y1b:y2b, x1b:x2b]
        if masks is not None and masks[i] is not None:
            xl, yl = y2a // r - y1a // r, x2a // r - x1a // r
            src = masks[i][None][..., y1b // r:y1b // r + xl, x1b // r:x1b // r + yl]
            dst = mask4[..., y1a // r:y2a // r, x1a // r:x2a // r]
            dst.zero_()
            dst[..., :src.shape[-2], :src.shape[-1]] = src        # deviation: the part past the source mask reads 0 (the reference throws)
        pads.append((x1a - x1b, y1a - y1b))
    return img4, mask4, pads


def warp(img, M, out_w, out_h, border, perspective, dtype, with_src=False):
    """:395-538.  img: uint8 [C, H, W]; M: 3x3 (any float dtype, used in `dtype`).  perspective: all of M; else rows 0-1 over (0, 0, 1)."""
    img = img.to(dtype)
    c, in_h, in_w = img.shape
    M = M.to(dtype)
    if not perspective:
        M3 = torch.eye(3, dtype=dtype)
        M3[:2] = M[:2]
        M = M3
    M_inv = torch.linalg.inv(M)
    gx = torch.arange(out_w, dtype=dtype).view(1, out_w).repeat(out_h, 1)
    gy = torch.arange(out_h, dtype=dtype).view(out_h, 1).repeat(1, out_w)
    flat = torch.stack([gx, gy, torch.ones_like(gx)], 0).view(3, -1)
    sf = M_inv.mm(flat)
    src = (sf[:2] / sf[2:3]).view(2, out_h, out_w)
    grid = torch.zeros(1, out_h, out_w, 2, dtype=dtype)
    grid[0, :, :, 0] = src[0] / (in_w - 1) * 2 - 1
    grid[0, :, :, 1] = src[1] / (in_h - 1) * 2 - 1
    sampled = F.grid_sample(img[None], grid, mode="bilinear", padding_mode="border", align_corners=False)
    valid = (src[0] >= 0) & (src[0] <= in_w - 1) & (src[1] >= 0) & (src[1] <= in_h - 1)
    bt = torch.tensor(border, dtype=dtype).view(c, 1, 1)
    res = torch.where(valid[None], sampled[0], bt.expand_as(sampled[0]))
    res = torch.clamp(res, 0, 255).to(torch.uint8)
    return (res, src) if with_src else res


def mask_matrix(M, r, dtype):
    """:373-376"""
    S = torch.diag(torch.tensor([r, r, 1], dtype=dtype))
    S_inv = torch.diag(torch.tensor([1.0 / r, 1.0 / r, 1], dtype=dtype))
    return S_inv.mm(M.to(dtype)).mm(S)


def image_sample(imgs, masks, xc, yc, M, flip_lr, flip_ud, s, r, perspective, dtype):
    """One output image as uint8 bytes [3, s, s] and its mask bytes [s/r, s/r] (None without masks): mosaic, warp, flips."""
    img4, mask4, _ = mosaic4(imgs, masks, xc, yc, s, r)
    M = torch.as_tensor(M, dtype=torch.float32).view(3, 3)
    out = warp(img4, M, s, s, [114, 114, 114], perspective, dtype)
    om = None
    if masks is not None:
        om = warp(mask4, mask_matrix(M, r, dtype), s // r, s // r, [0], perspective, dtype)[0]
    if flip_lr:
        out = out.flip(-1)
        om = om.flip(-1) if om is not None else None
    if flip_ud:
        out = out.flip(-2)
        om = om.flip(-2) if om is not None else None
    return out, om


def edge_distance(imgs, xc, yc, M, s, perspective):
    """Smallest distance (pixels, float64) of a source position from the validity edge 0 / in - 1 over the output pixels of one image."""
    img4, _, _ = mosaic4(imgs, None, xc, yc, s, 1)
    _, src = warp(img4, torch.as_tensor(M, dtype=torch.float32).view(3, 3), s, s, [114, 114, 114], perspective, torch.float64, with_src=True)
    return float(torch.minimum(src.abs(), (src - (2 * s - 1)).abs()).min())


def labels_sample(tiles, pads, M, flip_lr, flip_ud, s, perspective, dtype, sort_flipped=False):
    """tiles: four dicts {cls [n], boxes [n, 4] pixel xyxy in the source frame, kpts [n, K, 3] or None}.  Returns the kept rows of one image
    (cls, bboxes cxcywh / s, keypoints / s or None) and the decision margins of EVERY input label: ratio = area / org_area - 0.7, area1, area2
    (clipped areas before / after the matrix) and kmargin = the smallest distance of one of its keypoints from 0 / s (inf without keypoints)."""
    M = torch.as_tensor(M, dtype=torch.float32).view(3, 3).to(dtype)
    has_k = tiles[0]["kpts"] is not None
    bb, kk, cc = [], [], []
    for t, (padw, padh) in zip(tiles, pads):
        bb.append(torch.as_tensor(t["boxes"], dtype=torch.float32).view(-1, 4).to(dtype) + torch.tensor([padw, padh, padw, padh], dtype=dtype))
        cc.append(torch.as_tensor(t["cls"], dtype=torch.float32).view(-1))
        if has_k:
            k = torch.as_tensor(t["kpts"], dtype=torch.float32).to(dtype).clone()
            k[..., :2] = k[..., :2] + torch.tensor([padw, padh], dtype=dtype)
            kk.append(k)
    boxes, cls = torch.cat(bb), torch.cat(cc)
    kpts = torch.cat(kk) if has_k else None
    n = boxes.shape[0]
    area_of = lambda b: (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    org = area_of(boxes)
    boxes = boxes.clip(0, 2 * s)
    area1 = area_of(boxes)
    good1 = (area1 > 0) & (area1 > 0.7 * org)                                              # :245
    # apply_bboxes on every label (the reference applies it to the kept ones: the rows are independent)
    xy = torch.ones(n * 4, 3, dtype=dtype)
    xy[:, :2] = boxes[:, [0, 1, 2, 3, 0, 3, 2, 1]].reshape(n * 4, 2)
    xy = xy.mm(M.T)
    xy = (xy[:, :2] / xy[:, 2:3] if perspective else xy[:, :2]).reshape(n, 8)
    x, y = xy[:, [0, 2, 4, 6]], xy[:, [1, 3, 5, 7]]
    nb = torch.stack([x.min(1).values, y.min(1).values, x.max(1).values, y.max(1).values], 1).clamp(0, s)   # clip_boxes
    area2 = area_of(nb)
    good = good1 & (area2 > 0)                                                              # :683-684
    kmargin = torch.full((n,), float("inf"), dtype=torch.float64)
    if has_k:
        K = kpts.shape[1]
        kxy = torch.ones(n * K, 3, dtype=dtype)
        vis = kpts[..., 2].reshape(n * K).clone()
        kxy[:, :2] = kpts[..., :2].reshape(n * K, 2)
        kxy = kxy.mm(M.T)
        kxy = kxy[:, :2] / kxy[:, 2:3]                                                      # always divides (:596)
        out = (kxy[:, 0] < 0) | (kxy[:, 1] < 0) | (kxy[:, 0] > s) | (kxy[:, 1] > s)
        vis[out] = 0
        kmargin = torch.minimum(kxy.abs(), (kxy - s).abs()).min(1).values.reshape(n, K).min(1).values.double()
        kxy = kxy.clip(0, s)                                                                # clip_keypoints (same visibility test again)
        kpts = torch.cat([kxy, vis[:, None]], 1).reshape(n, K, 3)
    if flip_lr:
        nb[:, 0] = s - nb[:, 0]; nb[:, 2] = s - nb[:, 2]                                    # no swap (:890-891)
        if has_k:
            kpts[..., 0] = s - kpts[..., 0]
    if flip_ud:
        nb[:, 1] = s - nb[:, 1]; nb[:, 3] = s - nb[:, 3]
        if has_k:
            kpts[..., 1] = s - kpts[..., 1]
    if sort_flipped:
        nb = torch.stack([torch.minimum(nb[:, 0], nb[:, 2]), torch.minimum(nb[:, 1], nb[:, 3]),
                          torch.maximum(nb[:, 0], nb[:, 2]), torch.maximum(nb[:, 1], nb[:, 3])], 1)
    cxcywh = torch.stack([(nb[:, 0] + nb[:, 2]) / 2, (nb[:, 1] + nb[:, 3]) / 2, nb[:, 2] - nb[:, 0], nb[:, 3] - nb[:, 1]], 1) * (1.0 / s)
    if has_k:
        kpts[..., :2] = kpts[..., :2] * (1.0 / s)
    margins = dict(ratio=(area1 / org - 0.7).double(), area1=area1.double(), area2=area2.double(), kmargin=kmargin, good1=good1, good=good)
    return dict(cls=cls[good], bboxes=cxcywh[good], keypoints=kpts[good] if has_k else None), margins


def collate(samples):
    """YoloDataLoader.cs:18-44 over labels_sample's row dicts."""
    bi = torch.cat([torch.full((len(smp["cls"]),), float(i)) for i, smp in enumerate(samples)])
    out = dict(batch_idx=bi, cls=torch.cat([smp["cls"] for smp in samples]), bboxes=torch.cat([smp["bboxes"] for smp in samples]))
    if samples[0]["keypoints"] is not None:
        out["keypoints"] = torch.cat([smp["keypoints"] for smp in samples])
    return out
