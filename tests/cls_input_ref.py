"""ClassificationDataset's chain with Auto_Augment = None (Data/ClassificationDataset.cs:90-131, GetTensor :70-88), restated in torch + numpy on the
DRAWN parameters of one output image (the ys_cls_item of include/yolosharp_hip.h).  Nothing here comes from the package's kernels.

  crop [top, top + ch) x [left, left + cw)  ->  torch.nn.functional.interpolate(mode="nearest") on the uint8 crop to (oh, ow)  ->  the s x s slice at
  (oy, ox)  ->  flip  ->  erase (below)  ->  color_jitter_ref.color_jitter (torchvision's public uint8 algorithm)  ->  to_float: byte * (1 / 255.0f)

Train items have oh = ow = s, oy = ox = 0 (RandomResizedCrop); val items the whole source, the Resize(int) size and the CenterCrop offset.

Erase (the reference's RandomErasing, :166-226): the rectangle [er_y, er_y + er_h) x [er_x, er_x + er_w) of the OUTPUT frame (after the flips) takes a noise byte
per channel.  The reference writes torch.empty(c, h, w).normal_() into the uint8 image; ATen's CPU cast truncates toward zero and wraps mod 256, so the
byte is (uint8)(int64)z, z ~ N(0, 1): value k = 0 covers (-1, 1), k > 0 covers [k, k + 1), k < 0 covers (k - 1, k].  It is drawn by integer thresholds
on one 32-bit word: THRESHOLDS = round(2^32 * cumulative probability) for k = -6 .. 6, in float64 from erf, the last one 2^32 (the tails beyond +-7,
mass 2.6e-12, fold into +-6); k = -6 + the number of the first twelve thresholds with word >= threshold; byte = k mod 256.  The word is a counter-based
function of (er_seed, channel c, output pixel (y, x)), all uint32 arithmetic:
    word = mix32(mix32(er_seed ^ (c * 0x9e3779b9)) + (y * s + x))
    mix32(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16"""
import math

import numpy as np
import torch

import color_jitter_ref as CJ

THRESHOLDS = (4, 1231, 136027, 5797768, 97711073, 681419127, 3613548169, 4197256223, 4289169528, 4294831269, 4294966065, 4294967292, 4294967296)
VALUES = tuple(range(-6, 7))                  # the value k of bin i; the byte is k mod 256
ITEM_FIELDS = ("src", "top", "left", "ch", "cw", "oh", "ow", "oy", "ox", "flip_lr", "flip_ud", "er_y", "er_x", "er_h", "er_w", "er_seed")


def thresholds_from_erf():
    """round(2^32 * P(value <= k)) for k = -6 .. 6: P = Phi(k) for k < 0 (the bin is (k - 1, k], the lower tail folded into -6), Phi(k + 1) for
    0 <= k < 6 (k = 0 is (-1, 1), k > 0 is [k, k + 1)), 1 for k = 6 (the upper tail folded in)."""
    phi = lambda x: 0.5 * (1.0 + math.erf(x / math.sqrt(2.0)))
    cum = [phi(k) for k in range(-6, 0)] + [phi(k + 1) for k in range(0, 6)] + [1.0]
    return tuple(int(round(2.0 ** 32 * c)) for c in cum)


def mix32(x):
    x = np.asarray(x, np.uint32).copy()
    x ^= x >> np.uint32(16)
    x *= np.uint32(0x7feb352d)
    x ^= x >> np.uint32(15)
    x *= np.uint32(0x846ca68b)
    x ^= x >> np.uint32(16)
    return x


def noise_word(seed, c, pix):
    """The word of (er_seed, channel, pixel index y * s + x); pix may be an array."""
    with np.errstate(over="ignore"):
        a = mix32(np.uint32(seed) ^ np.uint32((int(c) * 0x9e3779b9) & 0xffffffff))
        return mix32(a + np.asarray(pix, np.uint32))


def value_of_word(u):
    """k in -6 .. 6 of a word (array)."""
    return np.searchsorted(np.asarray(THRESHOLDS[:12], np.uint64), np.asarray(u, np.uint64), side="right").astype(np.int64) - 6


def byte_of_word(u):
    return (value_of_word(u) & 255).astype(np.uint8)


def value_of_z(z):
    """The bin's value for a real z inside the table: trunc(z) (0 on (-1, 1); k on [k, k + 1); k on (k - 1, k])."""
    return int(math.trunc(z))


def index_map(n, off, size_in, size_out):
    """The general index formula of one axis, fp32: src[p] = min(floor((p + off) * ((float)size_in / (float)size_out)), size_in - 1), p = 0 .. n - 1."""
    scale = np.float32(size_in) / np.float32(size_out)
    p = (np.arange(n) + off).astype(np.float32)
    return np.minimum(np.floor(p * scale).astype(np.int64), size_in - 1)


def gather_by_formula(img, it, s):
    """crop -> resize -> slice by the index formula alone (no interpolate): uint8 [3, s, s], not flipped."""
    iy = it["top"] + index_map(s, it["oy"], it["ch"], it["oh"])
    ix = it["left"] + index_map(s, it["ox"], it["cw"], it["ow"])
    return img[:, torch.from_numpy(iy)][:, :, torch.from_numpy(ix)]


def gather(img, it, s):
    """crop -> interpolate(nearest) on uint8 -> slice: uint8 [3, s, s], not flipped."""
    crop = img[:, it["top"]:it["top"] + it["ch"], it["left"]:it["left"] + it["cw"]]
    res = torch.nn.functional.interpolate(crop[None], size=(it["oh"], it["ow"]), mode="nearest")[0]
    return res[:, it["oy"]:it["oy"] + s, it["ox"]:it["ox"] + s]


def erase(img, it, s):
    """The noise bytes over the item's rectangle of the s x s uint8 image (a copy)."""
    h, w = it["er_h"], it["er_w"]
    if h < 1 or w < 1:
        return img
    out = img.clone()
    yy, xx = np.mgrid[it["er_y"]:it["er_y"] + h, it["er_x"]:it["er_x"] + w]
    pix = (yy * s + xx).astype(np.uint32)
    for c in range(3):
        out[c, it["er_y"]:it["er_y"] + h, it["er_x"]:it["er_x"] + w] = torch.from_numpy(byte_of_word(noise_word(it["er_seed"], c, pix)))
    return out


def item_dict(item):
    """A structured-array row (or a mapping) as a dict of Python ints."""
    return {k: int(item[k]) for k in ITEM_FIELDS}


def sample_bytes(img_u8, item, s, row=None):
    """One output image as uint8 [3, s, s]: img_u8 = the source [3, H, W] (tensor), item = the drawn geometry, row = (order, factors) or None."""
    it = item_dict(item)
    img = gather(torch.as_tensor(img_u8), it, s)
    dims = [d for d, f in ((-1, it["flip_lr"]), (-2, it["flip_ud"])) if f]
    if dims:
        img = torch.flip(img, dims)
    img = erase(img.contiguous(), it, s)
    if row is not None:
        img = CJ.color_jitter(img, row[0], row[1])
    return img


def batch(images_u8, classes, items, s, rows=None):
    """(images fp32 [B, 3, s, s], cls fp32 [B]) of a batch, as numpy arrays."""
    out = [CJ.to_float(sample_bytes(torch.from_numpy(np.ascontiguousarray(images_u8[int(it["src"])])), it, s, None if rows is None else rows[b]))
           for b, it in enumerate(items)]
    return torch.stack(out).numpy(), np.asarray([classes[int(it["src"])] for it in items], np.float32)
