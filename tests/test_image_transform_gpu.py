"""mvlt_image_transform (csrc/imgxf.hip) against the NumPy restatement of Pillow's resize + torchvision's crop / flip /
ToTensor / Normalize (tests/image_transform_ref.py), and the iterators built on it end to end.  Integer arithmetic and a lookup
table leave no tolerance to choose: every kernel comparison is torch.equal / np.array_equal."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import image_transform_ref as R  # noqa: E402
from tiny_caption import tiny_caption  # noqa: E402

pytestmark = pytest.mark.gpu

# (h, w): both Resize(256) orientations, a 3x and a 4.6x squash, a black/white upscale, 16x on one axis only, identity axes
SIZES = [(300, 517), (517, 300), (1033, 777), (40, 30), (3584, 230), (230, 3584), (256, 300)]


def _source(h, w, seed, bw=False):
    rng = np.random.default_rng(seed)
    if bw:
        return (rng.integers(0, 2, size=(h, w, 3)) * 255).astype(np.uint8)
    return rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)


@pytest.fixture(scope="module")
def sources():
    return [_source(h, w, seed=31 * h + w, bw=(h, w) == (40, 30)) for h, w in SIZES]


@pytest.fixture(scope="module")
def resized256(sources):
    """Resize(256) of every source, bilinear, by the restatement: computed once, cropped by the tests."""
    return [R.resize(s, *R.resize256_size(*s.shape[:2]), R.BILINEAR) for s in sources]


def _flat(images):
    return torch.from_numpy(np.concatenate([im.reshape(-1) for im in images])).cuda()


def _f32_of(u8_hwc):
    """ToTensor + Normalize by the torch formula on the restatement's bytes."""
    return R.to_tensor_normalize(u8_hwc)


def test_train_mode_crops_and_flips_equal_the_restatement(sources, resized256):
    from mvlt_amd.data import plan_image_transform, transform_images
    src = _flat(sources)
    n = len(sources)
    alt = [b % 2 == 1 for b in range(n)]
    corner = [(r.shape[0] - 224, r.shape[1] - 224) for r in resized256]
    runs = [dict(crops=[(0, 0)] * n, flips=alt), dict(crops=corner, flips=[not f for f in alt]),
            dict(generator=torch.Generator().manual_seed(3))]
    for kw in runs:
        plan = plan_image_transform([s.shape[:2] for s in sources], "train", **kw)
        out = transform_images(src, plan)
        assert out.shape == (n, 3, 224, 224) and out.dtype == torch.float32 and out.is_cuda
        out = out.cpu()
        for b in range(n):
            t, l = int(plan.top[b]), int(plan.left[b])
            crop = resized256[b][t:t + 224, l:l + 224]
            want_u8 = np.ascontiguousarray(crop[:, ::-1] if plan.flip[b] else crop)
            assert torch.equal(out[b], _f32_of(want_u8)), (b, t, l, int(plan.flip[b]))        # bitwise: the torch formula
        assert torch.equal(out[0], R.transform(sources[0], "train", int(plan.top[0]), int(plan.left[0]), bool(plan.flip[0])))
    drawn = plan_image_transform([s.shape[:2] for s in sources], "train", generator=torch.Generator().manual_seed(3))
    assert drawn.flip.min() == 0 and drawn.flip.max() == 1                                    # the drawn run flips both ways


def test_eval_and_pil_resize_equal_the_restatement(sources):
    from mvlt_amd.data import plan_image_transform, transform_images
    src = _flat(sources)
    sizes = [s.shape[:2] for s in sources]
    plan = plan_image_transform(sizes, "eval")
    assert plan.kmax == 33                                                    # bilinear 16x
    out = transform_images(src, plan).cpu()
    assert out.shape == (len(sources), 3, 224, 224) and out.dtype == torch.float32
    for b, s in enumerate(sources):
        assert torch.equal(out[b], _f32_of(R.resize(s, 224, 224, R.BILINEAR))), b
    plan = plan_image_transform(sizes, "pil_resize")
    assert plan.kmax == 65                                                    # the bicubic 16x edge
    out = transform_images(src, plan)
    assert out.shape == (len(sources), 224, 224, 3) and out.dtype == torch.uint8 and out.is_cuda
    out = out.cpu().numpy()
    for b, s in enumerate(sources):
        assert np.array_equal(out[b], R.resize(s, 224, 224, R.BICUBIC)), b


def test_padded_tables_at_the_cap_and_a_single_image(sources):
    """A 3-tap image (bilinear upscale) beside a 65-tap one (bilinear 32x): the small image's rows are zero-padded to the cap.
    The same small image alone (B = 1, kmax = 3) gives the same result."""
    from mvlt_amd.data import plan_image_transform, transform_images
    small, big = sources[3], _source(7168, 230, seed=5)
    both = plan_image_transform([small.shape[:2], big.shape[:2]], "eval")
    alone = plan_image_transform([small.shape[:2]], "eval")
    assert both.kmax == 65 and alone.kmax == 3 and alone.B == 1
    assert not both.coef[0, :, :, 3:].any() and both.bounds[0, :, :, 1].max() <= 3
    out2 = transform_images(_flat([small, big]), both).cpu()
    out1 = transform_images(_flat([small]), alone).cpu()
    assert out1.shape == (1, 3, 224, 224)
    assert torch.equal(out2[0], _f32_of(R.resize(small, 224, 224, R.BILINEAR)))
    assert torch.equal(out2[1], _f32_of(R.resize(big, 224, 224, R.BILINEAR)))
    assert torch.equal(out1[0], out2[0])
    # B = 1 in the other output mode and with a shared source: two plan entries read one image
    twice = plan_image_transform([small.shape[:2]] * 2, "train", offsets=[0, 0], crops=[(0, 0), (50, 10)], flips=[0, 1])
    o = transform_images(_flat([small]), twice).cpu()
    assert torch.equal(o[0], R.transform(small, "train", 0, 0, False)) and torch.equal(o[1], R.transform(small, "train", 50, 10, True))
    u1 = transform_images(_flat([small]), plan_image_transform([small.shape[:2]], "pil_resize")).cpu().numpy()
    assert np.array_equal(u1[0], R.resize(small, 224, 224, R.BICUBIC))
    with pytest.raises(ValueError):
        transform_images(_flat([small])[:-1], alone)                          # a buffer shorter than the plan reads


def _store(tmp_path, n, seed):
    from mvlt_amd.data import ImageStore, write_image_store
    rng = np.random.default_rng(seed)
    shapes = [(int(rng.integers(230, 420)), int(rng.integers(230, 420))) for _ in range(n)]
    shapes[0], shapes[1] = (256, 300), (300, 256)
    images = [_source(h, w, seed=seed * 100 + i) for i, (h, w) in enumerate(shapes)]
    write_image_store(str(tmp_path / "store"), images)
    return ImageStore(str(tmp_path / "store")), images


def test_caption_batches_feed_the_caption_loss(tmp_path, specs_hash):
    import mvlt_amd as M
    from mvlt_amd.data import CaptionBatches, truncate_ids
    store, images = _store(tmp_path, 12, seed=2)
    rng = np.random.default_rng(4)
    N, T, V = 6, 12, 3000
    rows, full = zip(*[truncate_ids(list(rng.integers(1000, V, size=int(rng.integers(4, 11)))) + [104], T) for _ in range(N)])
    ids, full = np.stack(rows), np.array(full)
    model, _ = tiny_caption(M, specs_hash, torch.float32, max_length=T)
    n = 0
    for image, masked, labels in CaptionBatches(store, ids, full, 3, "cuda", split="train", views=2, seed=9, vocab_size=V):
        assert image.shape == (3, 2, 3, 224, 224) and image.dtype == torch.float32 and image.is_cuda
        assert masked.shape == (3, T) and masked.dtype == torch.int64 and labels.shape == (3, T) and labels.dtype == torch.int64
        assert int((labels >= 0).sum()) >= 3                                   # every caption has at least one masked token
        loss = model(image, masked, 0, "unilm", labels=labels)
        loss.backward()
        assert loss.dim() == 0 and bool(torch.isfinite(loss))
        n += 1
    assert n == 2
    g = model.MLM_head_seq2seq.predictions.decoder.weight.grad
    assert g is not None and bool(torch.isfinite(g).all())
    # the test split: in order, no randomness, short last batch, equal across two passes and equal to the restatement
    passes = []
    for _ in range(2):
        it = CaptionBatches(store, ids, full, 4, "cuda", split="test", views=2)
        passes.append([(im.cpu(), cap.cpu()) for im, cap in it])
    assert [p[0].shape[0] for p in passes[0]] == [4, 2]
    for (im_a, cap_a), (im_b, cap_b) in zip(*passes):
        assert torch.equal(im_a, im_b) and torch.equal(cap_a, cap_b)
    assert torch.equal(torch.cat([c for _, c in passes[0]]), torch.from_numpy(ids))
    assert torch.equal(passes[0][1][0][1, 1], R.transform(images[11], "eval"))                 # sample 5, view 1


def test_pretrain_batches_over_an_image_store(tmp_path):
    from mvlt_amd.data import PretrainBatches, Shard, normalize_images, truncate_ids, write_image_store
    rng = np.random.default_rng(8)
    N, T, V = 4, 12, 3000
    images = [_source(h, w, seed=70 + i) for i, (h, w) in enumerate([(260, 333), (517, 300), (224, 224), (100, 90)])]
    path = str(tmp_path / "s0")
    write_image_store(path, images)
    rows, full = zip(*[truncate_ids(list(rng.integers(1000, V, size=6)) + [104], T) for _ in range(N)])
    np.save(os.path.join(path, "ids.npy"), np.stack(rows).astype(np.int64))
    np.save(os.path.join(path, "full_len.npy"), np.array(full).astype(np.int32))
    want = [normalize_images(torch.from_numpy(R.resize(im, 224, 224, R.BICUBIC))[None].cuda())[0].cpu() for im in images]
    it = PretrainBatches(Shard(path), 4, "cuda", seed=1, vocab_size=V, itm_task=False)
    batches = list(it)
    assert len(batches) == 1
    image, masked, labels, itm, lengths = batches[0]
    assert image.shape == (4, 3, 224, 224) and image.dtype == torch.float32 and bool(itm.all())
    order = list(it.sampler)                                                  # itm_task=False: image i goes with caption i
    for slot, i in enumerate(order):
        ref = want[i]
        # the bound of tests/test_data_gpu.py for mvlt_image_normalize (the normalisation is that kernel); the bytes it reads
        # are bit-identical to the restatement's, so the two sides run the same kernel on the same input
        assert (image[slot].cpu() - ref).abs().max() <= 2e-5 * ref.abs().max(), i
