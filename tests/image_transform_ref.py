"""NumPy restatement of the image transforms ``mvlt_image_transform`` fuses, written from Pillow's documented 8-bit resample
rules (``precompute_coeffs`` + ``normalize_coeffs_8bpc`` + the two integer passes), not from the kernel:

* ``coeffs(in_size, out_size, filt)``: the per-axis tap tables (bounds [out, 2] = (first, count), coef [out, ksize], 22-bit fixed
  point);
* ``resize(img, out_h, out_w, filt)``: ``Image.resize`` of a uint8 HWC image -- horizontal pass, round to uint8, vertical pass;
* ``resize256_size`` / ``transform``: the three modes of the fine-tuning scripts (resize, crop, flip, ToTensor + Normalize as a
  table lookup built with the torch formula).
"""
import math

import numpy as np
import torch

PRECISION_BITS = 22
BILINEAR, BICUBIC = "bilinear", "bicubic"
IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)


def _bilinear(t):
    t = np.abs(t)
    return np.where(t < 1.0, 1.0 - t, 0.0)


def _bicubic(t):
    a = -0.5
    t = np.abs(t)
    return np.where(t < 1.0, ((a + 2.0) * t - (a + 3.0)) * t * t + 1.0,
                    np.where(t < 2.0, (((t - 5.0) * t + 8.0) * t - 4.0) * a, 0.0))


FILTERS = {BILINEAR: (_bilinear, 1.0), BICUBIC: (_bicubic, 2.0)}


def coeffs(in_size, out_size, filt):
    """(bounds int32 [out, 2], coef int32 [out, ksize]) of one axis; an unchanged axis gets the identity table."""
    if in_size == out_size:
        b = np.stack([np.arange(out_size), np.ones(out_size, dtype=np.int64)], 1).astype(np.int32)
        return b, np.full((out_size, 1), 1 << PRECISION_BITS, dtype=np.int32)
    f, S = FILTERS[filt]
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = S * fs
    ksize = int(math.ceil(support)) * 2 + 1
    center = (np.arange(out_size, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum((center - support + 0.5).astype(np.int64), 0)           # astype truncates toward zero, as C's (int)
    xmax = np.minimum((center + support + 0.5).astype(np.int64), in_size)
    n = xmax - xmin
    ss = 1.0 / fs
    w = np.zeros((out_size, ksize), dtype=np.float64)
    ww = np.zeros(out_size, dtype=np.float64)
    for x in range(ksize):                                                    # taps in order: ww is a sequential sum
        wx = np.where(x < n, f((x + xmin - center + 0.5) * ss), 0.0)
        w[:, x] = wx
        ww = ww + wx
    nz = ww != 0.0
    w[nz] = w[nz] / ww[nz, None]
    k = np.where(w < 0, -0.5 + w * (1 << PRECISION_BITS), 0.5 + w * (1 << PRECISION_BITS)).astype(np.int64)
    k[np.arange(ksize)[None, :] >= n[:, None]] = 0
    return np.stack([xmin, n], 1).astype(np.int32), k.astype(np.int32)


def _pass(img, bounds, coef):
    """Resample axis 1 of a uint8 [rows, in, C] image: out[:, xx] = clip8((2^21 + sum_i coef[xx, i] * img[:, first + i]) >> 22)."""
    rows, _, ch = img.shape
    out = np.empty((rows, len(bounds), ch), dtype=np.uint8)
    src = img.astype(np.int64)
    for xx, (first, count) in enumerate(bounds):
        acc = np.full((rows, ch), 1 << (PRECISION_BITS - 1), dtype=np.int64)
        for i in range(count):
            acc += int(coef[xx, i]) * src[:, first + i]
        out[:, xx] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return out


def resize(img, out_h, out_w, filt):
    """``Image.fromarray(img).resize((out_w, out_h), filt)`` for a uint8 [h, w, C] array."""
    h, w, _ = img.shape
    hb, hc = coeffs(w, out_w, filt)
    vb, vc = coeffs(h, out_h, filt)
    tmp = _pass(img, hb, hc)                                                  # horizontal first, rounded to uint8
    return np.ascontiguousarray(_pass(np.ascontiguousarray(tmp.transpose(1, 0, 2)), vb, vc).transpose(1, 0, 2))


def resize256_size(h, w, size=256):
    """torchvision ``Resize(size)`` of an (h, w) image: short side -> size, long side -> int(size * long / short)."""
    if (w <= h and w == size) or (h <= w and h == size):
        return h, w
    if w < h:
        return int(size * h / w), size
    return size, int(size * w / h)


def norm_table():
    """ToTensor + Normalize(ImageNet) of every byte value, with torch's own f32 arithmetic: [3, 256]."""
    rows = [torch.arange(256).float().div(255).sub(m).div(s) for m, s in zip(IMAGENET_MEAN, IMAGENET_STD)]
    return torch.stack(rows)


def to_tensor_normalize(u8_hwc):
    """The torch formula on the bytes themselves (what ToTensor + Normalize compute): f32 [3, H, W]."""
    x = torch.from_numpy(np.ascontiguousarray(u8_hwc)).permute(2, 0, 1).float().div(255)
    mean = torch.tensor(IMAGENET_MEAN).view(3, 1, 1)
    std = torch.tensor(IMAGENET_STD).view(3, 1, 1)
    return x.sub(mean).div(std)


def transform_u8(img, mode, top=0, left=0, flip=False, out=224):
    """The uint8 HWC [out, out, 3] image of one mode, before ToTensor / Normalize."""
    h, w, _ = img.shape
    if mode == "train":
        oh, ow = resize256_size(h, w)
        r = resize(img, oh, ow, BILINEAR)[top:top + out, left:left + out]
        return np.ascontiguousarray(r[:, ::-1] if flip else r)
    if mode == "eval":
        return resize(img, out, out, BILINEAR)
    if mode == "pil_resize":
        return resize(img, out, out, BICUBIC)
    raise ValueError(mode)


def transform(img, mode, top=0, left=0, flip=False, out=224):
    """What the kernel returns for one image: f32 CHW (table lookup) for 'train' / 'eval', uint8 HWC for 'pil_resize'."""
    u8 = transform_u8(img, mode, top, left, flip, out)
    if mode == "pil_resize":
        return torch.from_numpy(u8)
    lut = norm_table()
    idx = torch.from_numpy(u8.astype(np.int64)).permute(2, 0, 1)
    return torch.stack([lut[c][idx[c]] for c in range(3)])
