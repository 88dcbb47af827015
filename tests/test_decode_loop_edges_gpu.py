"""The edges of the token loops of ``decode.greedy_search`` and ``decode.sample_many`` on the tiny f32 caption model, B = 3:
``max_length`` 1 (the replay loop runs zero times: only the tail's head launch), 2 (one replay), 8 and 9 (at and one above
SYNC_EVERY: the read-back falls on the last replay, and on the tail), and an eos that the last row reaches in the last column of a
9-token decode.  Every call runs under ``MVLT_DECODE_GRAPH=1`` and ``=0``: equal ids, equal score shapes, scores within the bound
tests/test_sample_gpu.py holds the two entry points of the f32 head to (rel_err < 1e-5) over the live entries."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import rel_err, synth_batch  # noqa: E402
from tiny_caption import tiny_caption as _tiny  # noqa: E402

pytestmark = pytest.mark.gpu

B = 3
LENGTHS = (1, 2, 8, 9)
LOW_T = 0.05          # the sampled rows follow their image's greedy row (tests/test_multi_sample_gpu.py): rows can share an eos


def _greedy(decode, model, feat, n, **kw):
    return decode.greedy_search(model, feat, max_length=n, **kw)


def _sampled(decode, model, feat, n, seed=77, **kw):
    return decode.greedy_search(model, feat, sample_mode='sample', seed=seed, max_length=n, **kw)


def _many(decode, model, feat, n, seed=77, **kw):
    return decode.sample_many(model, feat, 2, include_greedy=True, seed=seed, max_length=n, **kw)


CALLS = {"greedy": _greedy, "sampled": _sampled, "many": _many}


@pytest.fixture(scope="module")
def tiny(specs_hash):
    """(decode module, model, image features of a pool of three images [3, n_img, H]): one model and one Swin pass per module."""
    import mvlt_amd as M
    from mvlt_amd import decode
    from mvlt_amd.arena import Arena
    from mvlt_amd.runtime import compute_dtype_of
    model, _ = _tiny(M, specs_hash, torch.float32)
    image, _, _, _ = synth_batch(B, 24, seed=63, vocab=3000)
    with torch.no_grad():
        Arena.of(model, compute_dtype_of(model))
        feat = model.conv(image.cuda())
    return decode, model, feat


def _both(monkeypatch, call, *args, **kw):
    """The call under both values of the switch -> {switch: (ids, scores)} on the host."""
    outs = {}
    for graph in ("1", "0"):
        monkeypatch.setenv("MVLT_DECODE_GRAPH", graph)
        ids, sc = call(*args, **kw)
        torch.cuda.synchronize()
        outs[graph] = (ids.cpu(), sc.cpu())
    return outs


@pytest.mark.parametrize("n", LENGTHS, ids=lambda n: f"len{n}")
@pytest.mark.parametrize("name", list(CALLS))
def test_graph_loop_equals_eager_loop_at_the_edges(tiny, monkeypatch, name, n):
    decode, model, feat = tiny
    assert decode.SYNC_EVERY == 8
    outs = _both(monkeypatch, CALLS[name], decode, model, feat, n)
    (ids, sc), (eids, esc) = outs["1"], outs["0"]
    want = ((B, 3, n), (B, 3, n)) if name == "many" else ((B, n), (B * n,))          # no eos: a score per id
    print(name, n, tuple(ids.shape), tuple(sc.shape), tuple(eids.shape), tuple(esc.shape), rel_err(sc, esc))
    assert (tuple(ids.shape), tuple(sc.shape)) == want and (tuple(eids.shape), tuple(esc.shape)) == want
    assert ids.dtype == eids.dtype == torch.int64 and sc.dtype == esc.dtype == torch.float32
    assert torch.equal(ids, eids), (ids.tolist(), eids.tolist())
    assert rel_err(sc, esc) < 1e-5


def _eos_in_the_last_column(rows, pad):
    """A token every row holds whose latest first occurrence is the rows' last column, or None."""
    n = len(rows[0])
    common = set(rows[0]).intersection(*rows[1:]) - {pad}
    cands = sorted(c for c in common if max(r.index(c) for r in rows) == n - 1)
    return cands[0] if cands else None


# batches of the three pooled images: the distinct ones first, then batches whose rows share an image (and so a greedy row)
BATCHES = ((0, 1, 2), (0, 2, 0), (0, 1, 0), (1, 2, 1), (0, 0, 0), (1, 1, 1), (2, 2, 2))


@pytest.mark.parametrize("name", list(CALLS))
def test_eos_in_the_last_column_of_a_nine_token_decode(tiny, monkeypatch, name):
    """max_length 9 and an eos whose last row finishes at column 8, the column of the tail: the replay loop's one read-back (after
    column 7) sees every flag up, the tail's pick lowers the last one, and the outputs are cut at 9 ids and 8 score columns
    (``sample_many``: 9 and 9).  The eos comes from an eos-free eager run, searched in the idiom of
    test_multi_sample_gpu.test_early_stop_is_per_row_and_cut_at_the_last_finish over a few batches of the pooled images and, for
    the sampled calls (temperature 0.05), at most 8 seeds."""
    decode, model, pool = tiny
    n, pad, call = 9, model.config.pad_token_id, CALLS[name]
    monkeypatch.setenv("MVLT_DECODE_GRAPH", "0")
    kw = {} if name == "greedy" else {"temperature": LOW_T}
    found = None
    for batch in BATCHES:
        feat = pool[list(batch)].contiguous()
        for seed in ((None,) if name == "greedy" else range(8)):
            if seed is not None:
                kw["seed"] = seed
            full, _ = call(decode, model, feat, n, **kw)
            full = full.reshape(-1, n).cpu()
            eos = _eos_in_the_last_column(full.tolist(), pad)
            if eos is not None:
                found = (feat, dict(kw), eos, full)
                break
        if found:
            break
    assert found, "no batch and seed lets every row reach a common token, the last of them in column 8"
    feat, kw, eos, full = found
    R = full.shape[0]
    first = [full[r].tolist().index(eos) for r in range(R)]
    assert max(first) == n - 1
    outs = _both(monkeypatch, call, decode, model, feat, n, eos_token_id=eos, **kw)
    live = torch.zeros(R, n, dtype=torch.bool)
    for r in range(R):
        live[r, :first[r] + 1] = True
    for graph in ("1", "0"):
        ids, sc = outs[graph]
        ids = ids.reshape(R, -1)
        assert ids.shape == (R, n), (graph, ids.shape)
        for r in range(R):
            assert torch.equal(ids[r, :first[r] + 1], full[r, :first[r] + 1]) and bool((ids[r, first[r] + 1:] == pad).all()), (graph, r)
    (ids, sc), (eids, esc) = outs["1"], outs["0"]
    assert torch.equal(ids, eids) and sc.shape == esc.shape
    if name == "many":
        assert sc.shape == (B, 3, n)
        sc, esc, lv = sc.reshape(R, n), esc.reshape(R, n), live
    else:          # the score of the column that finished the decode is not appended: 8 columns, concatenated step after step
        assert sc.shape == (B * (n - 1),)
        sc, esc, lv = sc.view(n - 1, B).t(), esc.view(n - 1, B).t(), live[:, :n - 1]
    print(name, first, rel_err(sc[lv], esc[lv]))
    assert rel_err(sc[lv], esc[lv]) < 1e-5
