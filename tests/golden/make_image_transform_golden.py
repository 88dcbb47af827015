"""Writes tests/golden/image_transform.npz: Pillow's own ``Image.resize`` outputs (bilinear and bicubic) for tiny uint8 RGB
sources, so that neither the CPU tests nor a GPU host need Pillow.  Run from the repository root with Pillow installed:

    python tests/golden/make_image_transform_golden.py

Keys: ``n`` (number of cases); per case i ``src_i`` uint8 [h, w, 3], ``size_i`` = (out_h, out_w), ``bilinear_i`` / ``bicubic_i``
uint8 [out_h, out_w, 3].  The file records the Pillow version it was made with (``pillow``).
"""
import os

import numpy as np
import PIL
from PIL import Image

# (h, w) -> (out_h, out_w): downscales with factors ~1.3 .. 16, a one-axis 16x squash, upscales, identity on one / both axes
CASES = [((37, 53), (16, 23)), ((53, 37), (23, 16)), ((61, 45), (14, 14)), ((20, 15), (48, 40)), ((10, 8), (28, 28)),
         ((224, 9), (14, 14)), ((9, 224), (14, 14)), ((31, 40), (31, 25)), ((31, 40), (19, 40)), ((16, 20), (16, 20)),
         ((120, 11), (7, 11))]


def main():
    rng = np.random.default_rng(20240607)
    out = {"n": np.int64(len(CASES)), "pillow": np.array(PIL.__version__)}
    for i, ((h, w), (oh, ow)) in enumerate(CASES):
        if i == 4:
            src = (rng.integers(0, 2, size=(h, w, 3)) * 255).astype(np.uint8)       # black / white: bicubic overshoot clips
        else:
            src = rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
        im = Image.fromarray(src, "RGB")
        out[f"src_{i}"] = src
        out[f"size_{i}"] = np.array([oh, ow], dtype=np.int64)
        out[f"bilinear_{i}"] = np.asarray(im.resize((ow, oh), Image.BILINEAR))
        out[f"bicubic_{i}"] = np.asarray(im.resize((ow, oh), Image.BICUBIC))
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "image_transform.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
