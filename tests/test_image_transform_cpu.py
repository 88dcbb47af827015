"""Host side of the fused image transform (mvlt_amd.data: resize_coeffs, plan_image_transform) and its NumPy restatement
(tests/image_transform_ref.py) against Pillow: the recorded outputs of tests/golden/image_transform.npz everywhere, live Pillow
where it is installed.  Every comparison is exact -- the resize is integer arithmetic over tables computed in double."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import image_transform_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILTERS = (R.BILINEAR, R.BICUBIC)
# source (h, w) -> output (h, w): the issue's list
LIVE = [((300, 517), (256, 441)), ((517, 300), (441, 256)), ((1033, 777), (224, 224)), ((40, 30), (224, 224)),
        ((3584, 230), (224, 224)), ((230, 3584), (224, 224)), ((256, 300), (256, 300))]


def _source(h, w, seed, bw=False):
    rng = np.random.default_rng(seed)
    if bw:
        return (rng.integers(0, 2, size=(h, w, 3)) * 255).astype(np.uint8)
    return rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)


@pytest.fixture(scope="module")
def pil_golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "image_transform.npz"))


def test_restatement_equals_the_recorded_pillow_outputs(pil_golden):
    golden = pil_golden
    n = int(golden["n"])
    assert n >= 8
    for i in range(n):
        oh, ow = (int(v) for v in golden[f"size_{i}"])
        for filt in FILTERS:
            got = R.resize(golden[f"src_{i}"], oh, ow, filt)
            assert got.dtype == np.uint8 and np.array_equal(got, golden[f"{filt}_{i}"]), (i, filt)


@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("case", LIVE, ids=[f"{h}x{w}" for (h, w), _ in LIVE])
def test_restatement_equals_live_pillow(case, filt):
    PIL = pytest.importorskip("PIL")
    from PIL import Image
    (h, w), (oh, ow) = case
    src = _source(h, w, seed=h * 7 + w, bw=(h, w) == (40, 30))
    want = np.asarray(Image.fromarray(src, "RGB").resize((ow, oh), getattr(Image, filt.upper())))
    assert np.array_equal(R.resize(src, oh, ow, filt), want), PIL.__version__


def test_resize_coeffs_equal_the_restatement():
    from mvlt_amd.data import resize_coeffs, resize_ksize
    pairs = [(517, 441), (300, 256), (1033, 224), (777, 224), (40, 224), (30, 224), (3584, 224), (230, 224), (256, 256), (620, 310),
             (7168, 224), (225, 224), (224, 225)]
    for filt in FILTERS:
        for n_in, n_out in pairs:
            b, c = resize_coeffs(n_in, n_out, filt)
            rb, rc = R.coeffs(n_in, n_out, filt)
            assert b.dtype == np.int32 and c.dtype == np.int32 and b.shape == (n_out, 2)
            assert c.shape == (n_out, resize_ksize(n_in, n_out, filt))
            assert np.array_equal(b, rb) and np.array_equal(c, rc), (filt, n_in, n_out)
            assert (b[:, 0] >= 0).all() and (b[:, 0] + b[:, 1] <= n_in).all() and (b[:, 1] <= c.shape[1]).all()
    b, c = resize_coeffs(256, 256, R.BICUBIC)                                 # identity: one tap of 1.0
    assert c.shape == (256, 1) and (c == 1 << 22).all() and np.array_equal(b[:, 0], np.arange(256)) and (b[:, 1] == 1).all()
    with pytest.raises(ValueError):
        resize_coeffs(10, 5, "lanczos")


def test_resize256_size_rule():
    from mvlt_amd.data import resize256_size
    assert resize256_size(300, 517) == (256, 441)            # landscape: int(256 * 517 / 300)
    assert resize256_size(517, 300) == (441, 256)            # portrait
    assert resize256_size(400, 400) == (256, 256)            # square
    assert resize256_size(256, 300) == (256, 300)            # short side already 256: left alone
    assert resize256_size(300, 256) == (300, 256)
    assert resize256_size(512, 620) == (256, 310)
    for hw in [(300, 517), (517, 300), (400, 400), (256, 300), (1033, 777), (40, 30)]:
        assert resize256_size(*hw) == R.resize256_size(*hw)


def test_tap_cap():
    from mvlt_amd.data import MAX_TAPS, plan_image_transform
    assert MAX_TAPS == 65
    with pytest.raises(ValueError, match="image 1 .*reduce the image offline"):
        plan_image_transform([(230, 300), (224 * 17, 230)], "pil_resize")     # bicubic 17x
    p = plan_image_transform([(224 * 16, 230)], "pil_resize")                 # bicubic 16x: the edge
    assert p.kmax == 65
    p = plan_image_transform([(224 * 32, 230)], "eval")                       # bilinear 32x is accepted
    assert p.kmax == 65
    with pytest.raises(ValueError):
        plan_image_transform([(224 * 33, 230)], "eval")
    with pytest.raises(ValueError):
        plan_image_transform([(300, 400)], "train")                           # draws need a generator
    with pytest.raises(ValueError):
        plan_image_transform([(300, 400)], "other")


def test_plan_tables_are_the_crop_rows_of_the_full_tables():
    from mvlt_amd.data import plan_image_transform
    sizes = [(300, 517), (517, 300), (256, 300), (40, 30)]
    plan = plan_image_transform(sizes, "train", crops=[(0, 0), (441 - 224, 256 - 224), (5, 70), (10, 0)], flips=[0, 1, 1, 0])
    assert plan.bounds.shape == (4, 2, 224, 2) and plan.bounds.dtype == np.int32
    assert plan.coef.shape == (4, 2, 224, plan.kmax) and plan.coef.dtype == np.int32
    assert plan.kmax == 5 and plan.flip.tolist() == [0, 1, 1, 0] and plan.hw.tolist() == [list(s) for s in sizes]
    assert plan.src_off.tolist() == [0, 300 * 517 * 3, 2 * 300 * 517 * 3, 2 * 300 * 517 * 3 + 256 * 300 * 3]
    for b, (h, w) in enumerate(sizes):
        oh, ow = R.resize256_size(h, w)
        for axis, (n_in, n_out, first) in enumerate(((w, ow, plan.left[b]), (h, oh, plan.top[b]))):
            rb, rc = R.coeffs(n_in, n_out, R.BILINEAR)
            assert np.array_equal(plan.bounds[b, axis], rb[first:first + 224])
            k = rc.shape[1]
            assert np.array_equal(plan.coef[b, axis, :, :k], rc[first:first + 224]) and not plan.coef[b, axis, :, k:].any()
    ev = plan_image_transform(sizes, "eval")
    assert not ev.flip.any() and not ev.top.any() and not ev.left.any() and ev.kmax == 7      # 517 / 224 = 2.3: 3 * 2 + 1 taps


def test_plan_draws():
    from mvlt_amd.data import plan_image_transform
    n = 4096
    sizes = [(300, 517), (517, 300)] * (n // 2)                               # resized: 256 x 441 and 441 x 256
    g = torch.Generator().manual_seed(11)
    plan = plan_image_transform(sizes, "train", generator=g)
    top, left = plan.top, plan.left
    assert top[0::2].min() == 0 and top[0::2].max() == 256 - 224 and left[0::2].min() == 0 and left[0::2].max() == 441 - 224
    assert top[1::2].min() == 0 and top[1::2].max() == 441 - 224 and left[1::2].min() == 0 and left[1::2].max() == 256 - 224
    assert abs(plan.flip.mean() - 0.5) < 0.03, plan.flip.mean()
    again = plan_image_transform(sizes, "train", generator=torch.Generator().manual_seed(11))
    for name in ("top", "left", "flip", "bounds", "coef", "src_off", "hw"):
        assert np.array_equal(getattr(plan, name), getattr(again, name)), name
    other = plan_image_transform(sizes, "train", generator=torch.Generator().manual_seed(12))
    assert not np.array_equal(plan.top, other.top) and not np.array_equal(plan.flip, other.flip)
    nxt = plan_image_transform(sizes, "train", generator=g)                    # the generator moves on
    assert not np.array_equal(plan.left, nxt.left)


def test_entry_point_is_declared_bound_and_exported_without_an_abi_bump():
    import re
    import mvlt_amd
    from mvlt_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "mvlt_hip.h")).read()
    assert re.search(r"\bint\s+mvlt_image_transform\s*\(", hdr)
    assert len(_lib.SYMBOLS["mvlt_image_transform"][1]) == 13 and hasattr(_lib.lib(), "mvlt_image_transform")
    assert int(re.search(r"#define\s+MVLT_ABI_VERSION\s+(\d+)", hdr).group(1)) == 17 == _lib.ABI_VERSION
    assert re.search(r"MVLT_IMGXF_F32_CHW = 0, MVLT_IMGXF_U8_HWC = 1", hdr) and (_lib.IMGXF_F32_CHW, _lib.IMGXF_U8_HWC) == (0, 1)
    for name in ("CaptionBatches", "ImageStore", "plan_image_transform", "resize_coeffs", "transform_images", "write_image_store"):
        assert hasattr(mvlt_amd, name), name
    # scalar refusals need no GPU: nothing is launched
    L = _lib.lib()
    ok = dict(src=64, off=64, hw=64, bounds=64, coef=64, flip=64, lut=64, out=64, B=1, O=224, kmax=5, mode=0)

    def call(**kw):
        a = dict(ok, **kw)
        return L.mvlt_image_transform(a["src"], a["off"], a["hw"], a["bounds"], a["coef"], a["flip"], a["lut"], a["out"], a["B"],
                                      a["O"], a["kmax"], a["mode"], None)
    for bad in (dict(B=0), dict(kmax=0), dict(kmax=66), dict(mode=2), dict(src=None), dict(coef=None), dict(out=None),
                dict(lut=None), dict(O=0), dict(O=228), dict(O=232), dict(out=72)):
        assert call(**bad) == -1, bad


def test_image_store_round_trip(tmp_path):
    from mvlt_amd.data import ImageStore, write_image_store
    images = [_source(h, w, seed=h) for h, w in [(5, 9), (12, 3), (1, 1), (7, 7)]]
    write_image_store(str(tmp_path / "st"), images)
    st = ImageStore(str(tmp_path / "st"))
    assert len(st) == 4 and st.size(1) == (12, 3)
    for i, im in enumerate(images):
        assert np.array_equal(st.image(i), im)
    assert st.index[:, 0].tolist() == [0, 135, 243, 246]
