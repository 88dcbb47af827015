"""Input pipeline for pre-training on pre-resized / pre-tokenised shards.

The reference builds every sample on the host inside ``Dataset.__getitem__``
(``run_pretrain_rgc_roco_medicat.py:94-212``: PIL decode + resize, per-channel
``(x - mean) / var``, WordPiece tokenisation, ``_random_mask_word``, ITM negative
sampling) with 8 DataLoader workers.  At ~1.9 k pairs/s per GPU that host work is
the bottleneck, so the per-step arithmetic moves to the GPU and the per-sample
decode/tokenise work moves offline:

* ``write_shard`` / ``Shard``: uint8 HWC images already resized to 224x224, token
  ids already truncated with the reference rule (``ids[:T-1] + [END]``, :170-172)
  and the untruncated token count, as three ``.npy`` files (memory-mapped);
* ``itm_pairs``: the ITM negative sampling of ``__getitem__`` (:134-158) on indices;
* ``ShardSampler``: the index arithmetic of ``torch.utils.data.DistributedSampler``
  (one process per GPU), bit-identical to it;
* ``normalize_images`` / ``mask_captions``: ``mvlt_image_normalize`` / ``mvlt_mlm_mask``;
* ``PretrainBatches``: ties them together and yields the 5-tuple ``PretrainStep`` takes
  (the fifth element, the caption lengths, enables packed rows).

Fine-tuning and evaluation read raw-size images (``run_report_generation_cxr.py:24-36``, ``run_retrieval_iuxray.py:52-65``:
``Resize(256) -> RandomCrop(224) -> RandomHorizontalFlip -> ToTensor -> Normalize`` on the train split, ``Resize((224, 224))``
on the test split; the ``--pretrained`` branches and pre-training: PIL ``resize((224, 224))``, bicubic).  Random crops rule out
an offline resize, so the resize itself runs on the GPU, bit-identical to Pillow:

* ``write_image_store`` / ``ImageStore``: ragged uint8 HWC RGB images as one flat memory-mapped byte file + an index;
* ``resize_coeffs``: Pillow's tap tables of one axis (``precompute_coeffs`` + ``normalize_coeffs_8bpc`` restated);
* ``plan_image_transform``: sizes, crop origins, flips and the tables of the crop's 224 columns and rows for a batch;
* ``transform_images``: ``mvlt_image_transform``, one launch per batch straight from the source bytes;
* ``CaptionBatches``: the iterator for the report-generation script (one or two views per sample);
* ``PretrainBatches`` also takes a shard whose images are an ``ImageStore`` (mode ``'pil_resize'`` + ``normalize_images``).
"""
from __future__ import annotations

import ctypes as C
import functools
import math
import os
import random
from typing import Iterator, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib as L
from . import ops


# ----------------------------------------------------------------------------- GPU steps
def normalize_images(u8_hwc: torch.Tensor) -> torch.Tensor:
    """uint8 [B,H,W,3] (RGB, as PIL gives it) -> f32 [B,3,H,W], per image and channel (x - mean) / var
    (run_pretrain_rgc_roco_medicat.py:107-110 -- np.var, i.e. the variance, as the reference has it)."""
    if not u8_hwc.is_cuda:
        raise RuntimeError("mvlt_amd runs on the GPU only (no CPU fallback)")
    assert u8_hwc.dtype == torch.uint8 and u8_hwc.dim() == 4 and u8_hwc.shape[3] == 3 and u8_hwc.is_contiguous()
    B, H, W, _ = u8_hwc.shape
    out = torch.empty((B, 3, H, W), dtype=torch.float32, device=u8_hwc.device)
    L.check(L.lib().mvlt_image_normalize(ops._p(u8_hwc), ops._p(out), B, H, W, ops._stream()), "mvlt_image_normalize")
    return out


def mask_captions(ids: torch.Tensor, full_len: torch.Tensor, seed: int, vocab_size: int, mask_id: int = 103,
                  itm_label: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """``_random_mask_word`` (:188-212) for a batch of truncated id rows -> (caption_masked, caption_label)."""
    if not ids.is_cuda:
        raise RuntimeError("mvlt_amd runs on the GPU only (no CPU fallback)")
    assert ids.dtype == torch.int64 and ids.dim() == 2 and ids.is_contiguous()
    assert full_len.dtype == torch.int32 and full_len.numel() == ids.shape[0] and full_len.is_cuda
    out, labels = torch.empty_like(ids), torch.empty_like(ids)
    p = L.MvltMlmMask()
    p.B, p.T, p.vocab_size, p.mask_id = ids.shape[0], ids.shape[1], int(vocab_size), int(mask_id)
    p.ids_in, p.full_len, p.ids_out, p.labels = ops._p(ids), ops._p(full_len), ops._p(out), ops._p(labels)
    if itm_label is not None:
        assert itm_label.dtype == torch.int64 and itm_label.numel() == ids.shape[0]
        p.itm_label = ops._p(itm_label)
    p.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    L.check(L.lib().mvlt_mlm_mask(C.byref(p), ops._stream()), "mvlt_mlm_mask")
    return out, labels


# ----------------------------------------------------------------------------- host logic (pure integer work)
def truncate_ids(token_ids: Sequence[int], T: int) -> Tuple[np.ndarray, int]:
    """:166-176 -- keep the first T-1 ids and the last one ([END]); zero-pad to T.  Returns (row, full length)."""
    n = len(token_ids)
    ids = list(token_ids)
    if n > T:
        ids = ids[:T - 1] + [ids[-1]]
    row = np.zeros(T, dtype=np.int64)
    row[:len(ids)] = ids
    return row, n


def deal_balanced(items: Sequence[int], weights: Sequence[int], parts: int) -> List[List[int]]:
    """Deal ``items`` (len = parts * k) into ``parts`` lists of k items with nearly equal weight sums: heaviest first, each
    to the lightest list that still has room (longest-processing-time rule; deterministic, ties by list index).  With the
    encoder running on packed rows a rank's step time follows the SUM of its caption lengths: an unbalanced deal makes
    every rank wait at the gradient all-reduce for the one with the longest captions (8 ranks x 32 samples of U{16..79}
    tokens: the slowest rank carries ~+4.7 % rows; dealt this way the sums differ by less than one caption)."""
    k = len(items) // parts
    assert k * parts == len(items) == len(weights)
    order = sorted(range(len(items)), key=lambda i: (-int(weights[i]), i))
    out: List[List[int]] = [[] for _ in range(parts)]
    load = [0] * parts
    for i in order:
        r = min((r for r in range(parts) if len(out[r]) < k), key=lambda r: (load[r], r))
        out[r].append(items[i])
        load[r] += int(weights[i])
    return out


class ShardSampler:
    """Indices of ``torch.utils.data.DistributedSampler(dataset, num_replicas, rank, shuffle, seed, drop_last)``:
    same permutation (torch.Generator seeded with seed + epoch), same padding, same rank stride.
    ``lengths`` (caption length per dataset index) + ``batch_size``: every GLOBAL batch (the num_replicas * batch_size
    entries the ranks would draw for one step) keeps its members but is re-dealt to the ranks with ``deal_balanced`` -- the
    global-batch gradient is unchanged, the ranks' packed row counts are equalised."""

    def __init__(self, n: int, num_replicas: int = 1, rank: int = 0, shuffle: bool = True, seed: int = 0,
                 drop_last: bool = False, lengths: Optional[Sequence[int]] = None, batch_size: Optional[int] = None):
        if not 0 <= rank < num_replicas:
            raise ValueError("rank out of range")
        self.n, self.num_replicas, self.rank = n, num_replicas, rank
        self.shuffle, self.seed, self.drop_last, self.epoch = shuffle, seed, drop_last, 0
        if drop_last and n % num_replicas != 0:
            self.num_samples = -(-(n - num_replicas) // num_replicas)
        else:
            self.num_samples = -(-n // num_replicas)
        self.total_size = self.num_samples * num_replicas
        if (lengths is None) != (batch_size is None):
            raise ValueError("length balancing needs both lengths and batch_size")
        self.lengths, self.batch_size = lengths, batch_size

    def set_epoch(self, epoch: int) -> None:
        self.epoch = epoch

    def __len__(self) -> int:
        return self.num_samples

    def __iter__(self) -> Iterator[int]:
        if self.shuffle:
            g = torch.Generator()
            g.manual_seed(self.seed + self.epoch)
            idx = torch.randperm(self.n, generator=g).tolist()
        else:
            idx = list(range(self.n))
        if not self.drop_last:
            pad = self.total_size - len(idx)
            if pad > 0:
                idx += (idx * (-(-pad // len(idx))))[:pad]
        else:
            idx = idx[:self.total_size]
        if self.lengths is None or self.num_replicas == 1:
            return iter(idx[self.rank:self.total_size:self.num_replicas])
        mine: List[int] = []
        step = self.num_replicas * self.batch_size
        for s0 in range(0, self.total_size, step):
            chunk = idx[s0:s0 + step]
            if len(chunk) < step:          # ragged tail: the plain stride
                mine += chunk[self.rank::self.num_replicas]
            else:
                mine += deal_balanced(chunk, [self.lengths[i] for i in chunk], self.num_replicas)[self.rank]
        return iter(mine)


def itm_pairs(indices: Sequence[int], n_total: int, cap_id_of, rng: random.Random, itm_task: bool = True
              ) -> List[Tuple[int, int, int]]:
    """(image index, caption index, ITM label) per sample, following ``__getitem__`` (:134-158): with
    probability 1/2 the pair is kept (label 1); otherwise a random other sample with a different caption id
    replaces either the image or the caption (probability 1/2 each) and the label is 0."""
    out = []
    for i in indices:
        if rng.random() < 0.5 or not itm_task:
            out.append((i, i, 1))
            continue
        j = rng.randrange(0, n_total)
        while j == i or cap_id_of(j) == cap_id_of(i):
            j = rng.randrange(0, n_total)
        out.append((j, i, 0) if rng.random() < 0.5 else (i, j, 0))
    return out


# ----------------------------------------------------------------------------- Pillow-exact resize: host tables
PRECISION_BITS = 22                  # Pillow's fixed point for 8-bit channels
MAX_TAPS = 65                        # the kernel's cap on taps per output pixel and axis (mvlt_hip.h)
IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
_MODES = {"train": ("bilinear", L.IMGXF_F32_CHW), "eval": ("bilinear", L.IMGXF_F32_CHW), "pil_resize": ("bicubic", L.IMGXF_U8_HWC)}


def _f_bilinear(t: np.ndarray) -> np.ndarray:
    t = np.abs(t)
    return np.where(t < 1.0, 1.0 - t, 0.0)


def _f_bicubic(t: np.ndarray) -> np.ndarray:
    a = -0.5
    t = np.abs(t)
    return np.where(t < 1.0, ((a + 2.0) * t - (a + 3.0)) * t * t + 1.0,
                    np.where(t < 2.0, (((t - 5.0) * t + 8.0) * t - 4.0) * a, 0.0))


_FILTERS = {"bilinear": (_f_bilinear, 1.0), "bicubic": (_f_bicubic, 2.0)}


def resize_ksize(in_size: int, out_size: int, filter: str) -> int:
    """Taps per output pixel of ``resize_coeffs`` (the width of its table)."""
    if in_size == out_size:
        return 1
    return int(math.ceil(_FILTERS[filter][1] * max(in_size / out_size, 1.0))) * 2 + 1


@functools.lru_cache(maxsize=512)
def _resize_coeffs(in_size: int, out_size: int, filter: str) -> Tuple[np.ndarray, np.ndarray]:
    if in_size == out_size:                                  # identity: one tap of 1.0 reproduces the pixel exactly
        bounds = np.stack([np.arange(out_size), np.ones(out_size, dtype=np.int64)], 1).astype(np.int32)
        coef = np.full((out_size, 1), 1 << PRECISION_BITS, dtype=np.int32)
    else:
        f, S = _FILTERS[filter]
        scale = in_size / out_size
        fs = max(scale, 1.0)
        support = S * fs
        ksize = int(math.ceil(support)) * 2 + 1
        center = (np.arange(out_size, dtype=np.float64) + 0.5) * scale
        xmin = np.maximum((center - support + 0.5).astype(np.int64), 0)      # astype truncates toward zero, like C's (int)
        n = np.minimum((center + support + 0.5).astype(np.int64), in_size) - xmin
        ss = 1.0 / fs                                                        # Pillow multiplies by the reciprocal
        w = np.zeros((out_size, ksize), dtype=np.float64)
        ww = np.zeros(out_size, dtype=np.float64)
        for x in range(ksize):                               # tap by tap: ww is Pillow's SEQUENTIAL sum (np.sum adds pairwise)
            wx = np.where(x < n, f((x + xmin - center + 0.5) * ss), 0.0)
            w[:, x] = wx
            ww = ww + wx
        nz = ww != 0.0
        w[nz] = w[nz] / ww[nz, None]
        one = float(1 << PRECISION_BITS)
        k = np.where(w < 0, -0.5 + w * one, 0.5 + w * one).astype(np.int64)
        k[np.arange(ksize)[None, :] >= n[:, None]] = 0
        bounds, coef = np.stack([xmin, n], 1).astype(np.int32), k.astype(np.int32)
    bounds.setflags(write=False)
    coef.setflags(write=False)
    return bounds, coef


def resize_coeffs(in_size: int, out_size: int, filter: str) -> Tuple[np.ndarray, np.ndarray]:
    """Pillow's tap tables for resampling one axis of an 8-bit image from ``in_size`` to ``out_size`` with ``filter``
    ('bilinear' | 'bicubic'): (bounds int32 [out, 2] = (first source index, tap count), coef int32 [out, ksize], 22-bit fixed
    point, unused taps 0).  ``precompute_coeffs`` + ``normalize_coeffs_8bpc`` of Pillow's Resample.c restated; one pass is
    ``out = clip((2**21 + sum_i coef[i] * pixel[first + i]) >> 22, 0, 255)``.  An axis whose size does not change gets the
    identity table (one tap of 2**22).  The arrays are cached and read-only."""
    if filter not in _FILTERS:
        raise ValueError(f"filter must be 'bilinear' or 'bicubic', not {filter!r}")
    if in_size < 1 or out_size < 1:
        raise ValueError("sizes must be positive")
    return _resize_coeffs(int(in_size), int(out_size), filter)


def resize256_size(h: int, w: int, size: int = 256) -> Tuple[int, int]:
    """(h, w) after torchvision ``Resize(size)``: the short side becomes ``size``, the long side ``int(size * long / short)``;
    an image whose short side already is ``size`` is left alone."""
    if (w <= h and w == size) or (h <= w and h == size):
        return h, w
    if w < h:
        return int(size * h / w), size
    return size, int(size * w / h)


class ImageTransformPlan:
    """What ``mvlt_image_transform`` needs for one batch (``plan_image_transform``).  Host arrays: ``src_off`` int64 [B], ``hw``
    int32 [B, 2], ``bounds`` int32 [B, 2, out, 2], ``coef`` int32 [B, 2, out, kmax], ``flip`` uint8 [B]; ``top`` / ``left`` /
    ``resized`` ([B, 2] = (oh, ow)) record the draws.  ``packed()`` is the five kernel arrays as one byte buffer (one H2D copy)."""

    def __init__(self, mode, out, kmax, src_off, hw, bounds, coef, flip, top, left, resized):
        self.mode, self.out, self.kmax, self.B = mode, out, kmax, len(hw)
        self.src_off, self.hw, self.bounds, self.coef, self.flip = src_off, hw, bounds, coef, flip
        self.top, self.left, self.resized = top, left, resized
        self.out_mode = _MODES[mode][1]
        self.src_bytes = int((src_off + hw[:, 0].astype(np.int64) * hw[:, 1] * 3).max())     # the source buffer must hold this

    def packed(self) -> Tuple[np.ndarray, List[int]]:
        parts = [self.src_off, self.hw, self.bounds, self.coef, self.flip]      # int64 first, bytes last: natural alignment
        offs, at = [], 0
        for a in parts:
            offs.append(at)
            at += a.nbytes
        buf = np.empty(at, dtype=np.uint8)
        for a, o in zip(parts, offs):
            buf[o:o + a.nbytes] = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        return buf, offs


def plan_image_transform(sizes: Sequence[Tuple[int, int]], mode: str, generator: Optional[torch.Generator] = None, out: int = 224,
                         offsets: Optional[Sequence[int]] = None, crops: Optional[Sequence[Tuple[int, int]]] = None,
                         flips: Optional[Sequence[bool]] = None) -> ImageTransformPlan:
    """The plan for a batch of B images of sizes ``(h, w)``:

    * ``'train'``: bilinear ``Resize(256)`` (short side), ``RandomCrop(out)`` with top ~ U{0..oh-out}, left ~ U{0..ow-out},
      ``RandomHorizontalFlip`` (p = 0.5) -> f32 CHW, ImageNet mean / std;
    * ``'eval'``: bilinear squash to out x out -> f32 CHW, ImageNet mean / std;
    * ``'pil_resize'``: bicubic squash to out x out (PIL's default filter) -> uint8 HWC, to feed ``normalize_images``.

    The draws come from ``generator`` (a seeded ``torch.Generator``; required for 'train' unless ``crops`` and ``flips`` fix
    them): statistically what torchvision does, not its RNG stream.  ``offsets``: byte offset of every image in the source
    buffer (default: packed one after the other; two entries may share one image).  Only the ``out`` columns and rows of the
    tables that the crop touches are kept.  A resize that needs more than 65 taps (a bilinear downscale beyond 32x, a bicubic one
    beyond 16x) raises ValueError; every table row is checked against the source size before anything reaches the GPU."""
    if mode not in _MODES:
        raise ValueError(f"mode must be one of {sorted(_MODES)}, not {mode!r}")
    if out < 8 or out > 224 or out % 8:
        raise ValueError("out must be a multiple of 8 in 8 .. 224")
    filt = _MODES[mode][0]
    B = len(sizes)
    if B < 1:
        raise ValueError("empty batch")
    hw = np.asarray(sizes, dtype=np.int64).reshape(B, 2)
    if (hw < 1).any():
        raise ValueError("image sizes must be positive")
    if offsets is None:
        nbytes = hw[:, 0] * hw[:, 1] * 3
        src_off = np.concatenate([[0], np.cumsum(nbytes)[:-1]]).astype(np.int64)
    else:
        src_off = np.asarray(offsets, dtype=np.int64).reshape(B)
        if (src_off < 0).any():
            raise ValueError("negative source offset")
    if mode == "train":
        resized = np.array([resize256_size(int(h), int(w), 256) for h, w in hw], dtype=np.int64).reshape(B, 2)
        if (resized < out).any():
            raise ValueError("crop larger than the resized image")
        if crops is None or flips is None:
            if generator is None:
                raise ValueError("mode 'train' draws crops and flips: pass a seeded torch.Generator")
            u = torch.rand((B, 3), generator=generator, dtype=torch.float64).numpy()
        span = resized - out + 1
        if crops is None:
            origin = np.minimum((u[:, :2] * span).astype(np.int64), span - 1)
        else:
            origin = np.asarray(crops, dtype=np.int64).reshape(B, 2)
            if (origin < 0).any() or (origin >= span).any():
                raise ValueError("crop origin out of range")
        flip = (u[:, 2] < 0.5) if flips is None else np.asarray(flips, dtype=bool).reshape(B)
    else:
        resized = np.full((B, 2), out, dtype=np.int64)
        origin = np.zeros((B, 2), dtype=np.int64)
        flip = np.zeros(B, dtype=bool)
    ks = np.array([[resize_ksize(int(hw[b, 1]), int(resized[b, 1]), filt), resize_ksize(int(hw[b, 0]), int(resized[b, 0]), filt)]
                   for b in range(B)])
    if (ks > MAX_TAPS).any():
        b = int(np.argmax(ks.max(1) > MAX_TAPS))
        raise ValueError(f"image {b} ({int(hw[b, 0])} x {int(hw[b, 1])} -> {int(resized[b, 0])} x {int(resized[b, 1])}, {filt}) needs "
                         f"{int(ks[b].max())} taps per pixel, the kernel takes {MAX_TAPS} (a bilinear downscale up to 32x, a bicubic "
                         "one up to 16x): reduce the image offline first")
    kmax = int(ks.max())
    bounds = np.zeros((B, 2, out, 2), dtype=np.int32)
    coef = np.zeros((B, 2, out, kmax), dtype=np.int32)
    for b in range(B):
        for axis, (src_n, dst_n, first) in enumerate(((hw[b, 1], resized[b, 1], origin[b, 1]), (hw[b, 0], resized[b, 0], origin[b, 0]))):
            bn, cf = resize_coeffs(int(src_n), int(dst_n), filt)             # axis 0: horizontal (columns), 1: vertical (rows)
            bounds[b, axis] = bn[first:first + out]
            coef[b, axis, :, :cf.shape[1]] = cf[first:first + out]
    # the kernel trusts the tables: a wrong row is an out-of-bounds read
    size_of = np.stack([hw[:, 1], hw[:, 0]], 1)[:, :, None]
    assert (bounds[..., 0] >= 0).all() and (bounds[..., 1] >= 1).all() and (bounds[..., 1] <= kmax).all()
    assert (bounds[..., 0].astype(np.int64) + bounds[..., 1] <= size_of).all(), "tap table reaches past the source image"
    return ImageTransformPlan(mode, out, kmax, src_off, hw.astype(np.int32), bounds, coef, flip.astype(np.uint8),
                              origin[:, 0].copy(), origin[:, 1].copy(), resized)


_NORM_TABLES: dict = {}


def imagenet_table(device) -> torch.Tensor:
    """ToTensor + Normalize(ImageNet) of every byte value, f32 [3, 256], computed once by torch itself on the host -- the kernel
    looks values up, so its f32 output is bitwise what the torch formula gives."""
    key = str(device)
    if key not in _NORM_TABLES:
        rows = [torch.arange(256).float().div(255).sub(m).div(s) for m, s in zip(IMAGENET_MEAN, IMAGENET_STD)]
        _NORM_TABLES[key] = torch.stack(rows).contiguous().to(device)
    return _NORM_TABLES[key]


def transform_images(src_u8_flat: torch.Tensor, plan: ImageTransformPlan) -> torch.Tensor:
    """``mvlt_image_transform`` on a flat uint8 CUDA buffer of ragged HWC RGB sources -> f32 [B, 3, out, out] ('train' / 'eval')
    or uint8 [B, out, out, 3] ('pil_resize').  One launch; the resized images are never materialised."""
    if not src_u8_flat.is_cuda:
        raise RuntimeError("mvlt_amd runs on the GPU only (no CPU fallback)")
    assert src_u8_flat.dtype == torch.uint8 and src_u8_flat.dim() == 1 and src_u8_flat.is_contiguous()
    if plan.src_bytes > src_u8_flat.numel():
        raise ValueError(f"the plan reads {plan.src_bytes} source bytes, the buffer holds {src_u8_flat.numel()}")
    dev, B, O = src_u8_flat.device, plan.B, plan.out
    buf, offs = plan.packed()
    tab = torch.from_numpy(buf).pin_memory().to(dev, non_blocking=True)
    base = tab.data_ptr()
    if plan.out_mode == L.IMGXF_F32_CHW:
        out = torch.empty((B, 3, O, O), dtype=torch.float32, device=dev)
        lut = ops._p(imagenet_table(dev))
    else:
        out = torch.empty((B, O, O, 3), dtype=torch.uint8, device=dev)
        lut = None
    L.check(L.lib().mvlt_image_transform(ops._p(src_u8_flat), base + offs[0], base + offs[1], base + offs[2], base + offs[3],
                                         base + offs[4], lut, ops._p(out), B, O, plan.kmax, plan.out_mode, ops._stream()),
            "mvlt_image_transform")
    return out


# ----------------------------------------------------------------------------- raw-size image store
def write_image_store(path: str, images: Sequence[np.ndarray]) -> None:
    """Ragged uint8 HWC RGB images -> ``images.bin`` (the bytes, one image after the other) + ``index.npy`` (int64 [N, 3]:
    byte offset, h, w): what a one-off decode of the dataset produces."""
    os.makedirs(path, exist_ok=True)
    index = np.zeros((len(images), 3), dtype=np.int64)
    at = 0
    with open(os.path.join(path, "images.bin"), "wb") as f:
        for i, im in enumerate(images):
            im = np.ascontiguousarray(im)
            assert im.dtype == np.uint8 and im.ndim == 3 and im.shape[2] == 3, "images are uint8 [h, w, 3]"
            index[i] = (at, im.shape[0], im.shape[1])
            f.write(im.tobytes())
            at += im.nbytes
    np.save(os.path.join(path, "index.npy"), index)


class ImageStore:
    def __init__(self, path: str):
        self.index = np.load(os.path.join(path, "index.npy"))
        self.data = np.memmap(os.path.join(path, "images.bin"), dtype=np.uint8, mode="r")
        end = self.index[:, 0] + self.index[:, 1] * self.index[:, 2] * 3
        assert len(self.index) == 0 or int(end.max()) <= len(self.data), "index.npy points past images.bin"

    def __len__(self) -> int:
        return len(self.index)

    def size(self, i: int) -> Tuple[int, int]:
        return int(self.index[i, 1]), int(self.index[i, 2])

    def image(self, i: int) -> np.ndarray:
        o, h, w = (int(v) for v in self.index[i])
        return self.data[o:o + h * w * 3].reshape(h, w, 3)

    def gather(self, idx: Sequence[int]) -> Tuple[torch.Tensor, List[Tuple[int, int]], List[int]]:
        """The bytes of images ``idx`` packed into one pinned uint8 tensor -> (buffer, sizes, byte offsets in the buffer)."""
        nbytes = [int(self.index[i, 1] * self.index[i, 2] * 3) for i in idx]
        buf = torch.empty(sum(nbytes), dtype=torch.uint8).pin_memory()
        view, at, offs = buf.numpy(), 0, []
        for i, n in zip(idx, nbytes):
            o = int(self.index[i, 0])
            view[at:at + n] = self.data[o:o + n]
            offs.append(at)
            at += n
        return buf, [self.size(i) for i in idx], offs


# ----------------------------------------------------------------------------- shards
def write_shard(path: str, images_u8_hwc: np.ndarray, id_rows: np.ndarray, full_len: np.ndarray) -> None:
    os.makedirs(path, exist_ok=True)
    assert images_u8_hwc.dtype == np.uint8 and images_u8_hwc.ndim == 4 and images_u8_hwc.shape[3] == 3
    assert id_rows.ndim == 2 and len(id_rows) == len(images_u8_hwc) == len(full_len)
    np.save(os.path.join(path, "images_u8.npy"), images_u8_hwc)
    np.save(os.path.join(path, "ids.npy"), id_rows.astype(np.int64))
    np.save(os.path.join(path, "full_len.npy"), full_len.astype(np.int32))


class Shard:
    """``images_u8.npy`` (uint8 [N, 224, 224, 3], resized offline) or, without it, an ``ImageStore`` (``images.bin`` +
    ``index.npy``) of raw-size images in the same directory; ``ids.npy``; ``full_len.npy``."""

    def __init__(self, path: str):
        if os.path.exists(os.path.join(path, "images_u8.npy")):
            self.images = np.load(os.path.join(path, "images_u8.npy"), mmap_mode="r")
        else:
            self.images = ImageStore(path)
        self.ids = np.load(os.path.join(path, "ids.npy"), mmap_mode="r")
        self.full_len = np.load(os.path.join(path, "full_len.npy"), mmap_mode="r")

    def __len__(self) -> int:
        return len(self.ids)


class PretrainBatches:
    """Iterates (image, caption_masked, caption_label, image_text_label, text_lengths) batches: gathers the uint8
    images / id rows of a batch on the host (pinned), one async H2D copy each, normalisation + masking on the GPU.
    ``text_lengths`` stays on the host (it is what ``PretrainStep`` needs for packed rows)."""

    def __init__(self, shard: Shard, batch_size: int, device, num_replicas: int = 1, rank: int = 0, seed: int = 0,
                 vocab_size: int = 30522, mask_id: int = 103, itm_task: bool = True, mlm_task: bool = True,
                 drop_last: bool = True):
        self.shard, self.B, self.device = shard, batch_size, torch.device(device)
        self.sampler = ShardSampler(len(shard), num_replicas, rank, shuffle=True, seed=seed, drop_last=drop_last)
        self.rng = random.Random(seed * 7919 + rank)
        self.seed, self.vocab_size, self.mask_id, self.itm_task, self.mlm_task = seed, vocab_size, mask_id, itm_task, mlm_task
        self.step = 0

    def set_epoch(self, epoch: int) -> None:
        self.sampler.set_epoch(epoch)

    def __iter__(self):
        idx = list(self.sampler)
        T = self.shard.ids.shape[1]
        for s in range(0, len(idx) - self.B + 1, self.B):
            pairs = itm_pairs(idx[s:s + self.B], len(self.shard), lambda k: k, self.rng, self.itm_task)
            img_i = np.fromiter((p[0] for p in pairs), dtype=np.int64)
            cap_i = np.fromiter((p[1] for p in pairs), dtype=np.int64)
            if isinstance(self.shard.images, ImageStore):       # raw sizes: PIL resize((224, 224)) on the GPU, then as before
                src, sizes, offs = self.shard.images.gather(img_i.tolist())
                u8 = transform_images(src.to(self.device, non_blocking=True), plan_image_transform(sizes, "pil_resize", offsets=offs))
            else:
                u8 = torch.from_numpy(np.ascontiguousarray(self.shard.images[img_i])).pin_memory().to(self.device, non_blocking=True)
            ids = torch.from_numpy(np.ascontiguousarray(self.shard.ids[cap_i])).pin_memory()
            flen = torch.from_numpy(np.ascontiguousarray(self.shard.full_len[cap_i]))
            itm = torch.tensor([p[2] for p in pairs], dtype=torch.int64)
            image = normalize_images(u8)
            ids_d = ids.to(self.device, non_blocking=True)
            itm_d = itm.pin_memory().to(self.device, non_blocking=True)
            if self.mlm_task:
                masked, labels = mask_captions(ids_d, flen.pin_memory().to(self.device, non_blocking=True),
                                               seed=self.seed * 1000003 + self.step, vocab_size=self.vocab_size,
                                               mask_id=self.mask_id, itm_label=itm_d)
            else:
                masked, labels = ids_d, torch.full_like(ids_d, -100)
            self.step += 1
            yield image, masked, labels, itm_d, torch.clamp(flen, max=T).to(torch.int32)


class CaptionBatches:
    """The input side of ``run_report_generation_cxr.py`` for ``MVLBertForImageCaption.forward(..., labels=)``: gathers the
    batch's raw-size source bytes into one pinned buffer, one async H2D copy, then plan + ``mvlt_image_transform`` and, on the
    train split, ``mask_captions`` (``_random_mask_word`` and the truncation rule of :154-174 are the ones it implements).

    ``store`` holds ``views`` images per sample, sample i's at ``views * i ..``; with ``views=2`` each view gets its own
    independent crop and flip, as ``__getitem__`` transforms the two images one after the other (:128-129), and the image comes
    back as [B, 2, 3, 224, 224].  ``ids`` int64 [N, T] are the truncated id rows (``truncate_ids``), ``full_len`` the
    untruncated token counts.  ``split='train'``: shuffled, whole batches, yields ``(image, caption_masked, mlm_labels)``;
    ``split='test'``: in order, the last batch may be short, no randomness, yields ``(image, caption_ids)``.
    ``pretrained=True`` is the script's ``--pretrained`` branch (:130-145): PIL ``resize((224, 224))`` + ``normalize_images``
    on either split.  Crops and flips come from the iterator's own generator (seed, rank): statistically torchvision's, not its
    RNG stream."""

    def __init__(self, store: ImageStore, ids: np.ndarray, full_len: np.ndarray, batch_size: int, device, split: str = "train",
                 views: int = 1, num_replicas: int = 1, rank: int = 0, seed: int = 0, vocab_size: int = 30522, mask_id: int = 103,
                 pretrained: bool = False):
        if split not in ("train", "test"):
            raise ValueError("split must be 'train' or 'test'")
        if views not in (1, 2):
            raise ValueError("views must be 1 or 2")
        ids = np.asarray(ids)
        if ids.ndim != 2 or len(store) != views * len(ids) or len(full_len) != len(ids):
            raise ValueError(f"{len(store)} images, {len(ids)} id rows, {len(full_len)} lengths and views={views} do not match")
        self.store, self.ids, self.full_len = store, ids.astype(np.int64), np.asarray(full_len).astype(np.int32)
        self.B, self.device, self.split, self.views, self.pretrained = batch_size, torch.device(device), split, views, pretrained
        train = split == "train"
        self.sampler = ShardSampler(len(ids), num_replicas, rank, shuffle=train, seed=seed, drop_last=train)
        self.gen = torch.Generator()
        self.gen.manual_seed(seed * 7919 + rank)
        self.seed, self.vocab_size, self.mask_id, self.step = seed, vocab_size, mask_id, 0

    def set_epoch(self, epoch: int) -> None:
        self.sampler.set_epoch(epoch)

    def _images(self, samples: Sequence[int]) -> torch.Tensor:
        src, sizes, offs = self.store.gather([self.views * i + v for i in samples for v in range(self.views)])
        mode = "pil_resize" if self.pretrained else ("train" if self.split == "train" else "eval")
        plan = plan_image_transform(sizes, mode, generator=self.gen, offsets=offs)
        image = transform_images(src.to(self.device, non_blocking=True), plan)
        if self.pretrained:
            image = normalize_images(image)
        return image.view(len(samples), 2, 3, plan.out, plan.out) if self.views == 2 else image

    def __iter__(self):
        idx = list(self.sampler)
        train = self.split == "train"
        for s in range(0, len(idx) - self.B + 1 if train else len(idx), self.B):
            samples = idx[s:s + self.B]
            image = self._images(samples)
            sel = np.asarray(samples, dtype=np.int64)
            ids_d = torch.from_numpy(self.ids[sel]).pin_memory().to(self.device, non_blocking=True)
            if not train:
                yield image, ids_d
                continue
            flen = torch.from_numpy(self.full_len[sel]).pin_memory().to(self.device, non_blocking=True)
            masked, labels = mask_captions(ids_d, flen, seed=self.seed * 1000003 + self.step, vocab_size=self.vocab_size,
                                           mask_id=self.mask_id)
            self.step += 1
            yield image, masked, labels
