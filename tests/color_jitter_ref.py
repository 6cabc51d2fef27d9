"""torchvision.transforms.ColorJitter on a uint8 RGB image, restated in torch with the arithmetic dtype as a parameter.

What is restated is torchvision's public uint8 algorithm (torchvision/transforms/_functional_tensor.py: _blend, rgb_to_grayscale, adjust_brightness,
adjust_contrast, adjust_saturation, adjust_hue, _rgb2hsv, _hsv2rgb, convert_image_dtype; transforms.ColorJitter.forward / get_params) -- NOT the
reference: RandomHSV (Data/Augment.cs:968-987) hands the image to TorchVision.NET, whose source is not part of the reference tree.

  * every op takes and returns a uint8 image: the truncation happens between the ops, not once at the end
  * a factor is a Python double that meets the tensor as one rounded scalar of the tensor's float type; 1.0 - factor is formed in double first
  * dtype = torch.float32 is torchvision's own arithmetic (what the kernels are held to, bit for bit); torch.float64 measures how far that arithmetic
    is from the real numbers

A row is (order, factors): order[k] = the op id run in slot k (0 brightness, 1 contrast, 2 saturation, 3 hue) or -1 for nothing; factors[id] by op id,
taken as the fp32 values the ABI carries."""
import numpy as np
import torch

BRIGHTNESS, CONTRAST, SATURATION, HUE = 0, 1, 2, 3


def _scalar(x, dtype):
    return torch.tensor(float(x), dtype=dtype)


def blend(img, other, factor, dtype):
    """_blend: (ratio * img1 + (1.0 - ratio) * img2).clamp(0, 255).to(uint8); `other` is a uint8 or a `dtype` tensor that broadcasts against img."""
    ratio = float(factor)
    return (_scalar(ratio, dtype) * img.to(dtype) + _scalar(1.0 - ratio, dtype) * other.to(dtype)).clamp(0, 255).to(torch.uint8)


def gray(img, dtype):
    """rgb_to_grayscale: (0.2989 * r + 0.587 * g + 0.114 * b).to(uint8), keeping the channel axis."""
    r, g, b = (c.to(dtype) for c in img.unbind(dim=-3))
    return ((_scalar(0.2989, dtype) * r + _scalar(0.587, dtype) * g) + _scalar(0.114, dtype) * b).to(torch.uint8).unsqueeze(-3)


def adjust_brightness(img, factor, dtype):
    return blend(img, torch.zeros_like(img), factor, dtype)


def adjust_contrast(img, factor, dtype):
    mean = gray(img, dtype).to(dtype).mean(dim=(-3, -2, -1), keepdim=True)
    return blend(img, mean, factor, dtype)


def adjust_saturation(img, factor, dtype):
    return blend(img, gray(img, dtype), factor, dtype)


def rgb2hsv(img):
    r, g, b = img.unbind(dim=-3)
    maxc, minc = torch.max(img, dim=-3).values, torch.min(img, dim=-3).values
    eqc = maxc == minc
    cr = maxc - minc
    ones = torch.ones_like(maxc)
    s = cr / torch.where(eqc, ones, maxc)
    cr_divisor = torch.where(eqc, ones, cr)
    rc, gc, bc = (maxc - r) / cr_divisor, (maxc - g) / cr_divisor, (maxc - b) / cr_divisor
    hr = (maxc == r) * (bc - gc)
    hg = ((maxc == g) & (maxc != r)) * (2.0 + rc - bc)
    hb = ((maxc != g) & (maxc != r)) * (4.0 + gc - rc)
    h = hr + hg + hb
    h = torch.fmod(h / 6.0 + 1.0, 1.0)
    return torch.stack((h, s, maxc), dim=-3)


def hsv2rgb(img):
    h, s, v = img.unbind(dim=-3)
    i = torch.floor(h * 6.0)
    f = h * 6.0 - i
    i = i.to(torch.int32)
    p = torch.clamp(v * (1.0 - s), 0.0, 1.0)
    q = torch.clamp(v * (1.0 - s * f), 0.0, 1.0)
    t = torch.clamp(v * (1.0 - (s * (1.0 - f))), 0.0, 1.0)
    i = (i % 6).to(torch.int64).unsqueeze(-3)
    # torchvision sums one-hot(i) * candidates with an einsum: one candidate plus five zeros, i.e. the candidate itself
    pick = lambda cands: torch.gather(torch.stack(cands, dim=-3), -3, i).squeeze(-3)
    return torch.stack((pick((v, q, p, p, t, v)), pick((t, v, v, q, p, p)), pick((p, p, t, v, v, q))), dim=-3)


def adjust_hue(img, factor, dtype):
    x = img.to(dtype) / 255.0                                            # convert_image_dtype(uint8 -> float): a true division
    hsv = rgb2hsv(x)
    h, s, v = hsv.unbind(dim=-3)
    h = torch.remainder(h + _scalar(float(factor), dtype), 1.0)         # (h + hue_factor) % 1.0, Python-style
    out = hsv2rgb(torch.stack((h, s, v), dim=-3))
    return out.mul(_scalar(255.0 + 1.0 - 1e-3, dtype)).to(torch.uint8)   # convert_image_dtype(float -> uint8): max + 1 - eps, truncated


OPS = {BRIGHTNESS: adjust_brightness, CONTRAST: adjust_contrast, SATURATION: adjust_saturation, HUE: adjust_hue}


def color_jitter(img, order, factors, dtype=torch.float32):
    """ColorJitter.forward on one uint8 image [3, H, W] (or a stack whose images share the row -- but then contrast's mean runs over the whole stack,
    so give contrast one image at a time): the ops of `order` in turn, -1 skipped."""
    assert img.dtype == torch.uint8 and img.shape[-3] == 3
    f32 = np.asarray(factors, np.float32)
    for op in order:
        if int(op) >= 0:
            img = OPS[int(op)](img, float(f32[int(op)]), dtype)
    return img


def color_jitter_batch(images, rows, dtype=torch.float32):
    """images uint8 [B, 3, H, W] (tensor or array), rows = a structured array / sequence of (order, factor) -> uint8 tensor [B, 3, H, W]."""
    images = torch.as_tensor(images)
    return torch.stack([color_jitter(images[b], rows[b][0], rows[b][1], dtype) for b in range(images.shape[0])])


def to_float(img_u8):
    """mul(1 / 255.0f) (Data/YoloDataset.cs:140): byte * the fp32 reciprocal."""
    return img_u8.to(torch.float32) * torch.tensor(1 / 255.0, dtype=torch.float32)
