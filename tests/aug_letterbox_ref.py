"""Restatement of the reference's close-mosaic training input in torch, with the dtype of the label arithmetic as a parameter (float32 = what the
reference computes, float64 = the judge of tests/test_augment_letterbox.py): Augment.LetterBox (Data/Augment.cs:698-778), FlipLR / FlipUD (:860-966),
GetTensor's box_convert + Normalize + mul(1/255) (Data/YoloDataset.cs:102-151, Data/Struct.cs:99-121) and the collate (Data/YoloDataLoader.cs:18-44).
The random draws (the two flip decisions) are arguments.  The image path has no arithmetic on values: bytes are gathered, so it has no dtype.

One documented deviation of the engine is restated here too: the label tables hold pixel xyxy and are converted to the cxcywh the reference carries
through this branch with cx = (x1 + x2) / 2, w = x2 - x1 (torchvision box_convert)."""
import numpy as np
import torch
import torch.nn.functional as F


def geometry(h, w, out):
    """LetterboxImage's (:761-770) new_w, new_h, pad_l, pad_u of an h x w plane on an out x out canvas, in C#'s float arithmetic."""
    f = np.float32
    ratio = min(f(out) / f(w), f(out) / f(h))
    new_w, new_h = int(f(w) * ratio), int(f(h) * ratio)
    return new_w, new_h, (out - new_w) // 2, (out - new_h) // 2


def nearest_index(out, inp):
    """ATen's legacy nearest rule in fp32: src = min(floor(dst * (float)in / out), in - 1)."""
    scale = np.float32(inp) / np.float32(out)
    return np.minimum(np.floor(np.arange(out, dtype=np.float32) * scale).astype(np.int64), inp - 1)


def resize_nearest(img, new_h, new_w):
    """torchvision.transforms.functional.resize(img, new_h, new_w) of TorchVision.NET (default interpolation: nearest) by the formula."""
    iy, ix = torch.from_numpy(nearest_index(new_h, img.shape[-2])), torch.from_numpy(nearest_index(new_w, img.shape[-1]))
    return img[..., iy, :][..., ix]


def resize_nearest_aten(img, new_h, new_w):
    """The same through ATen: interpolate(mode="nearest") on fp32."""
    return F.interpolate(img[None].to(torch.float32), size=(new_h, new_w), mode="nearest")[0].to(img.dtype)


def letterbox_image(img, out, color, resize=resize_nearest):
    """LetterboxImage (:756-777): img uint8 [C, h, w] -> (pad_l, pad_u, uint8 [C, out, out])."""
    new_w, new_h, pad_l, pad_u = geometry(img.shape[-2], img.shape[-1], out)
    res = torch.full((img.shape[0], out, out), color, dtype=img.dtype)
    if new_w > 0 and new_h > 0:
        res[:, pad_u:pad_u + new_h, pad_l:pad_l + new_w] = resize(img, new_h, new_w)
    return pad_l, pad_u, res


def image_sample(img, mask, flip_lr, flip_ud, s, r):
    """One output image as uint8 bytes [3, s, s] and its id mask bytes [s/r, s/r] (None without a mask): LetterBox (:719-727), flips (:879-883, :936-940).
    The mask is letterboxed from its own size: its pads are not the image's pads / r."""
    _, _, out = letterbox_image(img, s, 114)
    om = letterbox_image(mask[None], s // r, 0)[2][0] if mask is not None else None
    if flip_lr:
        out = out.flip(-1)
        om = om.flip(-1) if om is not None else None
    if flip_ud:
        out = out.flip(-2)
        om = om.flip(-2) if om is not None else None
    return out, om


def to_float(img_u8):
    """label.img.mul(1 / 255.0f) (YoloDataset.cs:140)."""
    return img_u8.to(torch.float32) * torch.tensor(1 / 255.0, dtype=torch.float32)


def labels_sample(label, h, w, flip_lr, flip_ud, s, dtype, keep_size=False):
    """label: {cls [n], bboxes [n, 4] pixel xyxy in the source frame (fp32), keypoints [n, K, 3] or None} of an h x w source.  Every label is kept, in
    order: -> dict(cls, bboxes cxcywh / s, keypoints / s or None) in `dtype`."""
    _, _, pad_l, pad_u = geometry(h, w, s)
    b = torch.as_tensor(label["bboxes"], dtype=torch.float32).view(-1, 4).to(dtype)
    box = torch.stack([(b[:, 0] + b[:, 2]) / 2, (b[:, 1] + b[:, 3]) / 2, b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]], 1)      # box_convert(xyxy -> cxcywh)
    box = box + torch.tensor([pad_l, pad_u, 0, 0], dtype=dtype)                                                        # :735-738, not scaled by ratio
    kp = None
    if label.get("keypoints") is not None:
        kp = torch.as_tensor(label["keypoints"], dtype=torch.float32).to(dtype).clone()
        kp[..., :2] = kp[..., :2] + torch.tensor([pad_l, pad_u], dtype=dtype)                                          # :741-744
    if flip_lr:                                                                                                         # bbox_format != xywh: columns 0 and 2
        box[:, 0] = s - box[:, 0]
        if not keep_size:
            box[:, 2] = s - box[:, 2]
        if kp is not None:
            kp[..., 0] = s - kp[..., 0]
    if flip_ud:
        box[:, 1] = s - box[:, 1]
        if not keep_size:
            box[:, 3] = s - box[:, 3]
        if kp is not None:
            kp[..., 1] = s - kp[..., 1]
    inv = torch.tensor(np.float32(1.0) / np.float32(s) if dtype == torch.float32 else 1.0 / s, dtype=dtype)          # Normalize: mul(1f / w)
    box = box * inv
    if kp is not None:
        kp[..., :2] = kp[..., :2] * inv
    return dict(cls=torch.as_tensor(label["cls"], dtype=torch.float32).view(-1), bboxes=box, keypoints=kp)


def collate(samples):
    """YoloDataLoader.cs:18-44 over labels_sample's row dicts."""
    bi = torch.cat([torch.full((len(smp["cls"]),), float(i)) for i, smp in enumerate(samples)])
    out = dict(batch_idx=bi, cls=torch.cat([smp["cls"] for smp in samples]), bboxes=torch.cat([smp["bboxes"] for smp in samples]))
    if samples[0]["keypoints"] is not None:
        out["keypoints"] = torch.cat([smp["keypoints"] for smp in samples])
    return out
