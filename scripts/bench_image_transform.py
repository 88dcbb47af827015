"""The fused fine-tuning image transform (mvlt_image_transform: Pillow-exact Resize(256) -> RandomCrop(224) -> flip -> ToTensor ->
Normalize in one launch) on B = 32 sources of 512 x 620, train mode, and the views = 2 case (64 transforms per batch).
Device events around blocks of launches on an otherwise idle stream (tables uploaded before the timed region: the kernel alone),
then the whole transform_images call (plan upload + launch) the same way, the plan's host time, and a device copy of the same
byte count (source + output) as the yardstick.  Where Pillow is installed the same transform runs through Pillow + NumPy on one
core; otherwise the figure recorded in profiles/image_transform.md is quoted and marked as such.
B (32), H (512), W (620), ROUNDS (5 blocks), ITERS (50 launches per block)."""
import os, sys, time
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mvlt_amd as M  # noqa: F401
from mvlt_amd import _lib as L, ops
from mvlt_amd.data import imagenet_table, plan_image_transform, transform_images
B, H, W = int(os.environ.get("B", 32)), int(os.environ.get("H", 512)), int(os.environ.get("W", 620))
ROUNDS, ITERS = int(os.environ.get("ROUNDS", 5)), int(os.environ.get("ITERS", 50))
RECORDED_PIL_MS = 3.0          # ms per image, Pillow 12.2 on one core of the development host (profiles/image_transform.md)
rng = np.random.default_rng(0)
images = rng.integers(0, 256, size=(B, H, W, 3), dtype=np.uint8)
src = torch.from_numpy(images.reshape(-1)).cuda()


def timed(fn):
    """ms per call: ROUNDS blocks of ITERS back-to-back calls between two events; the best and the median block."""
    for _ in range(10):
        fn()
    ms = []
    for _ in range(ROUNDS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(ITERS):
            fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b) / ITERS)
    ms.sort()
    return ms[0], ms[len(ms) // 2]


for views in (1, 2):
    n = B * views
    offs = [(i // views) * H * W * 3 for i in range(n)]          # views = 2: both views read the same source bytes
    g = torch.Generator().manual_seed(0)
    t0 = time.perf_counter()
    for _ in range(20):
        plan = plan_image_transform([(H, W)] * n, "train", generator=g, offsets=offs)
    plan_ms = (time.perf_counter() - t0) * 1e3 / 20
    buf, o = plan.packed()
    tab = torch.from_numpy(buf).cuda()
    base = tab.data_ptr()
    out = torch.empty((n, 3, 224, 224), dtype=torch.float32, device="cuda")
    lut = imagenet_table(src.device)

    def kernel():
        L.check(L.lib().mvlt_image_transform(ops._p(src), base + o[0], base + o[1], base + o[2], base + o[3], base + o[4], ops._p(lut),
                                             ops._p(out), n, 224, plan.kmax, plan.out_mode, ops._stream()), "mvlt_image_transform")

    k_best, k_med = timed(kernel)
    c_best, c_med = timed(lambda: transform_images(src, plan))
    src_bytes, out_bytes = src.numel(), out.numel() * 4
    moved = src_bytes + out_bytes
    a, b = torch.empty(moved, dtype=torch.uint8, device="cuda"), torch.empty(moved, dtype=torch.uint8, device="cuda")
    y_best, _ = timed(lambda: b.copy_(a))
    print(f"views={views}: {n} transforms of {H}x{W} -> 224x224 (kmax {plan.kmax}): kernel {k_med * 1e3:.1f} us/batch (best "
          f"{k_best * 1e3:.1f}), transform_images {c_med * 1e3:.1f} us/batch (best {c_best * 1e3:.1f}), plan on the host "
          f"{plan_ms * 1e3:.0f} us", flush=True)
    print(f"    source {src_bytes / 1e6:.2f} MB + output {out_bytes / 1e6:.2f} MB = {moved / 1e6:.2f} MB: {moved / k_best / 1e6:.1f} GB/s "
          f"in the kernel; a device copy of {moved / 1e6:.2f} MB takes {y_best * 1e3:.1f} us "
          f"({2 * moved / y_best / 1e6:.1f} GB/s read + write)", flush=True)

try:
    from PIL import Image
    mean = np.array((0.485, 0.456, 0.406), dtype=np.float32)
    std = np.array((0.229, 0.224, 0.225), dtype=np.float32)
    torch.set_num_threads(1)
    t0 = time.perf_counter()
    for i in range(B):
        im = Image.fromarray(images[i], "RGB")
        oh, ow = (256, int(256 * W / H)) if H <= W else (int(256 * H / W), 256)
        im = im.resize((ow, oh), Image.BILINEAR).crop((3, 5, 227, 229)).transpose(Image.FLIP_LEFT_RIGHT)
        x = ((np.asarray(im, dtype=np.float32) / 255.0 - mean) / std).transpose(2, 0, 1).copy()
    pil_ms = (time.perf_counter() - t0) * 1e3 / B
    print(f"Pillow + NumPy on one core of this host: {pil_ms:.2f} ms per image, {pil_ms * B:.1f} ms per batch of {B}", flush=True)
except ImportError:
    print(f"Pillow is not installed on this host; recorded elsewhere (one core of the development host, NOT this machine): "
          f"{RECORDED_PIL_MS:.2f} ms per image, {RECORDED_PIL_MS * B:.1f} ms per batch of {B}", flush=True)
