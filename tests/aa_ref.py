"""torchvision's AutoAugment / RandAugment operators on a uint8 RGB image (tensor path, nearest interpolation, fill = None), restated with torch's own
operators: grid_sample, conv2d, bincount / cumsum and the blend of color_jitter_ref.  What is restated is torchvision's public algorithm
(transforms/autoaugment.py _apply_op; transforms/_functional_tensor.py _gen_affine_grid, _apply_grid_transform, _blurred_degenerate_image, posterize,
solarize, invert, autocontrast, _equalize_single_image) -- NOT the reference, which hands the image to TorchVision.NET (not in the reference tree), and not
torchvision itself, which is not available to these tests: parity with either is UNPINNED.  Nothing here comes from the package's kernels.

A row is the ys_aa_row of include/yolosharp_hip.h: op[2] (-1 = nothing), arg[2], theta[2][6]; the slots run in order, each on the previous one's uint8 image.
The classification chain with rows is cls_input_ref's with the slots between the flips and the erase (Data/ClassificationDataset.cs:105-120)."""
import numpy as np
import torch

import cls_input_ref as CR
import color_jitter_ref as CJ

SHEAR_X, SHEAR_Y, TRANSLATE_X, TRANSLATE_Y, ROTATE, BRIGHTNESS, COLOR, CONTRAST, SHARPNESS, POSTERIZE, SOLARIZE, AUTOCONTRAST, EQUALIZE, INVERT = range(14)
F32 = torch.float32


# ---------------------------------------------------------------------------------------------------- affine
def affine_grid_sample(img, theta):
    """The real pipeline: _gen_affine_grid (linspace base grid, bmm with the rescaled theta) + grid_sample(nearest, zeros, align_corners = False), round, uint8."""
    H, W = img.shape[-2:]
    th = torch.tensor(np.asarray(theta, np.float32)).reshape(1, 2, 3)
    base = torch.empty(1, H, W, 3, dtype=F32)
    base[..., 0].copy_(torch.linspace(-W * 0.5 + 0.5, W * 0.5 + 0.5 - 1, steps=W))
    base[..., 1].copy_(torch.linspace(-H * 0.5 + 0.5, H * 0.5 + 0.5 - 1, steps=H).unsqueeze_(-1))
    base[..., 2].fill_(1)
    rescaled = th.transpose(1, 2) / torch.tensor([0.5 * W, 0.5 * H], dtype=F32)
    grid = base.view(1, H * W, 3).bmm(rescaled).view(1, H, W, 2)
    out = torch.nn.functional.grid_sample(img[None].to(F32), grid, mode="nearest", padding_mode="zeros", align_corners=False)
    return out.round().to(torch.uint8)[0]


def affine_source(theta, H, W):
    """The explicit formula's unnormalised source coordinates (ux, uy), fp32 [H, W], every operation rounded on its own."""
    f = np.float32
    th = np.asarray(theta, f).reshape(6)
    w, h = f(W), f(H)
    r = np.concatenate([th[:3] / (f(0.5) * w), th[3:] / (f(0.5) * h)]).astype(f)
    bx = np.arange(W, dtype=f) + (-w * f(0.5) + f(0.5))
    by = np.arange(H, dtype=f) + (-h * f(0.5) + f(0.5))
    BX, BY = np.meshgrid(bx, by)
    gx = (BX * r[0] + BY * r[1]) + r[2]
    gy = (BX * r[3] + BY * r[4]) + r[5]
    return ((gx + f(1)) * w - f(1)) / f(2), ((gy + f(1)) * h - f(1)) / f(2)


def affine_by_formula(img, theta):
    """out[y][x] = in[nearbyint(uy)][nearbyint(ux)] inside the image, 0 outside: the arithmetic include/yolosharp_hip.h states for the affine ops."""
    H, W = img.shape[-2:]
    ux, uy = affine_source(theta, H, W)
    ix, iy = np.rint(ux), np.rint(uy)                                  # half to even
    inside = (ix >= 0) & (ix <= W - 1) & (iy >= 0) & (iy <= H - 1)
    jx, jy = np.where(inside, ix, 0).astype(np.int64), np.where(inside, iy, 0).astype(np.int64)
    out = img[:, torch.from_numpy(jy), torch.from_numpy(jx)]
    return torch.where(torch.from_numpy(inside)[None], out, torch.zeros_like(out))


def tie_distance(theta, H, W):
    """The smallest distance of a source coordinate from a rounding tie (k + 0.5)."""
    ux, uy = affine_source(theta, H, W)
    d = lambda u: np.abs((u.astype(np.float64) - 0.5) - np.rint(u.astype(np.float64) - 0.5))
    return float(min(d(ux).min(), d(uy).min()))


# ---------------------------------------------------------------------------------------------------- the other operators
def sharpness(img, factor):
    H, W = img.shape[-2:]
    if H <= 2 or W <= 2:
        return img
    k = torch.tensor([[1, 1, 1], [1, 5, 1], [1, 1, 1]], dtype=F32)
    k = (k / k.sum()).expand(3, 1, 3, 3)
    inner = torch.nn.functional.conv2d(img[None].to(F32), k, groups=3)[0].round().to(torch.uint8)
    deg = img.clone()
    deg[:, 1:-1, 1:-1] = inner
    return CJ.blend(img, deg, factor, F32)


def posterize(img, bits):
    return img & torch.tensor((-(1 << (8 - int(bits)))) & 255, dtype=torch.uint8)


def solarize(img, threshold):
    return torch.where(img.to(F32) >= torch.tensor(float(threshold), dtype=F32), 255 - img, img)


def invert(img):
    return 255 - img


def autocontrast(img):
    x = img.to(F32)
    mn, mx = x.amin(dim=(-2, -1), keepdim=True), x.amax(dim=(-2, -1), keepdim=True)
    scale = 255.0 / (mx - mn)
    eq = torch.isfinite(scale).logical_not()
    mn[eq] = 0
    scale[eq] = 1
    return ((x - mn) * scale).clamp(0, 255).to(torch.uint8)


def equalize_channel(ch):
    hist = torch.bincount(ch.reshape(-1).to(torch.int64), minlength=256)
    nonzero = hist[hist != 0]
    step = torch.div(nonzero[:-1].sum(), 255, rounding_mode="floor")
    if step == 0:
        return ch
    lut = torch.div(torch.cumsum(hist, 0) + torch.div(step, 2, rounding_mode="floor"), step, rounding_mode="floor")
    lut = torch.nn.functional.pad(lut, [1, 0])[:-1].clamp(0, 255)
    return lut[ch.to(torch.int64)].to(torch.uint8)


def equalize(img):
    return torch.stack([equalize_channel(img[c]) for c in range(img.shape[0])])


def apply_op(img, op, arg, theta):
    """One slot on one uint8 image [3, H, W]; arg and theta taken as the fp32 values the ABI carries."""
    op, arg = int(op), float(np.float32(arg))
    if op < 0:
        return img
    if op <= ROTATE:
        return affine_by_formula(img, theta)              # the contract of the ABI; test_auto_augment.py holds it to affine_grid_sample
    if op == BRIGHTNESS:
        return CJ.adjust_brightness(img, arg, F32)
    if op == COLOR:
        return CJ.adjust_saturation(img, arg, F32)
    if op == CONTRAST:
        return CJ.adjust_contrast(img, arg, F32)
    if op == SHARPNESS:
        return sharpness(img, arg)
    if op == POSTERIZE:
        return posterize(img, int(arg))
    if op == SOLARIZE:
        return solarize(img, arg)
    if op == AUTOCONTRAST:
        return autocontrast(img)
    if op == EQUALIZE:
        return equalize(img)
    assert op == INVERT, op
    return invert(img)


def apply_row(img, row):
    img = torch.as_tensor(img)
    for k in range(2):
        img = apply_op(img, row["op"][k], row["arg"][k], row["theta"][k])
    return img


def ops_batch(images, rows):
    """uint8 [B, 3, H, W] (array) through each image's row -> uint8 array."""
    return torch.stack([apply_row(torch.from_numpy(np.ascontiguousarray(images[b])), rows[b]) for b in range(len(rows))]).numpy()


# ---------------------------------------------------------------------------------------------------- the classification chain
def sample_bytes(img_u8, item, s, row=None, aa=None):
    """cls_input_ref.sample_bytes with the two slots between the flips and the erase."""
    it = CR.item_dict(item)
    img = CR.gather(torch.as_tensor(img_u8), it, s)
    dims = [d for d, f in ((-1, it["flip_lr"]), (-2, it["flip_ud"])) if f]
    if dims:
        img = torch.flip(img, dims)
    img = img.contiguous()
    if aa is not None:
        img = apply_row(img, aa)
    img = CR.erase(img.contiguous(), it, s)
    if row is not None:
        img = CJ.color_jitter(img, row[0], row[1])
    return img


def batch(images_u8, classes, items, s, rows=None, aa=None):
    """(images fp32 [B, 3, s, s], cls fp32 [B]) of a batch, as numpy arrays."""
    out = [CJ.to_float(sample_bytes(torch.from_numpy(np.ascontiguousarray(images_u8[int(it["src"])])), it, s, None if rows is None else rows[b],
                                    None if aa is None else aa[b])) for b, it in enumerate(items)]
    return torch.stack(out).numpy(), np.asarray([classes[int(it["src"])] for it in items], np.float32)
