"""The harness the two replayed decode graphs share (decode._DecodeGraph): a call with another key replaces the model's graph, a
call with the same key reuses it, every result equals the eager loop's on a fresh model, and the graph objects pickle to None.
Tiny f32 model, max_length 8."""
import os
import pickle
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import rel_err, synth_batch  # noqa: E402
from tiny_caption import tiny_caption  # noqa: E402

pytestmark = pytest.mark.gpu

F32 = torch.float32


@pytest.fixture(scope="module")
def M():
    import mvlt_amd
    return mvlt_amd


def _count_captures(monkeypatch, cls, captures):
    orig = cls.capture
    monkeypatch.setattr(cls, "capture", lambda self: (captures.append(self.key), orig(self))[1])


def test_greedy_graph_is_replaced_and_reused_by_key(M, specs_hash, monkeypatch):
    from mvlt_amd import decode
    model, _ = tiny_caption(M, specs_hash, F32)
    fresh, _ = tiny_caption(M, specs_hash, F32)
    image, _, _, _ = synth_batch(3, 24, seed=63, vocab=3000)
    img = image.cuda()
    monkeypatch.setenv("MVLT_DECODE_GRAPH", "0")
    ref = {B: [t.cpu() for t in fresh(img[:B], None, 1, 'unilm')] for B in (3, 2)}
    assert "_mvlt_greedy_graph" not in fresh.__dict__
    monkeypatch.setenv("MVLT_DECODE_GRAPH", "1")
    captures = []
    _count_captures(monkeypatch, decode._GreedyGraph, captures)
    for n, B in enumerate((3, 2, 3), 1):
        ids, sc = model(img[:B], None, 1, 'unilm')
        gg = model.__dict__["_mvlt_greedy_graph"]
        assert len(captures) == n and gg.key == captures[-1] and gg.key[0] == B
        assert torch.equal(ids.cpu(), ref[B][0]), (B, ids, ref[B][0])
        # (the graph's pick and the eager loop's are two entry points of the f32 head: the bound of tests/test_sample_gpu.py)
        assert sc.shape == ref[B][1].shape and rel_err(sc.cpu(), ref[B][1]) < 1e-5
    assert captures[0] == captures[2] != captures[1]
    ids, _ = model(img, None, 1, 'unilm')                              # the same key again: nothing is captured
    assert len(captures) == 3 and model.__dict__["_mvlt_greedy_graph"] is gg and torch.equal(ids.cpu(), ref[3][0])
    assert pickle.loads(pickle.dumps(gg)) is None


def test_beam_graph_is_replaced_and_reused_by_key(M, specs_hash, monkeypatch):
    from mvlt_amd import decode
    model, _ = tiny_caption(M, specs_hash, F32)
    fresh, _ = tiny_caption(M, specs_hash, F32)
    image, _, _, _ = synth_batch(2, 24, seed=83, vocab=3000)
    img = image.cuda()
    monkeypatch.setenv("MVLT_BEAM_DEVICE", "1")
    monkeypatch.setenv("MVLT_DECODE_GRAPH", "0")
    ref = {nb: fresh(img, None, nb, 'unilm').cpu() for nb in (3, 2)}
    assert "_mvlt_beam_graph" not in fresh.__dict__
    monkeypatch.setenv("MVLT_DECODE_GRAPH", "1")
    captures = []
    _count_captures(monkeypatch, decode._BeamGraph, captures)
    for n, nb in ((1, 3), (2, 2), (2, 2)):
        out = model(img, None, nb, 'unilm').cpu()
        bg = model.__dict__["_mvlt_beam_graph"]
        assert len(captures) == n and bg.key == captures[-1] and bg.key[:2] == (2, nb)
        assert torch.equal(out, ref[nb]), (nb, out, ref[nb])
    assert captures[0] != captures[1]
    assert pickle.loads(pickle.dumps(bg)) is None
