"""``decode.sample_many`` on the GPU -- K sampled reports per image (and the greedy report) from one decode pass -- on the tiny
caption model: against ``greedy_search``, against the oracle pick by pick (the generalised teacher-forced checker of
tests/multi_sample_ref.py), graph loop against eager loop, early stop, the graphs' coexistence, ``generate(num_return_sequences=)``
and the refusals."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import multi_sample_ref as R  # noqa: E402
import sample_ref as S  # noqa: E402
from conftest import rel_err, synth_batch  # noqa: E402
from test_sample_gpu import _tiny_oracle_cfgs  # noqa: E402
from tiny_caption import tiny_caption as _tiny  # noqa: E402

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
B = 3


@pytest.fixture(scope="module")
def M():
    import mvlt_amd
    return mvlt_amd


def _image():
    image, _, _, _ = synth_batch(B, 24, seed=63, vocab=3000)
    return image


def _many(M, model, image, *args, **kw):
    """sample_many on the image tower's output, as generate() calls it."""
    from mvlt_amd.arena import Arena
    from mvlt_amd.runtime import compute_dtype_of
    with torch.no_grad():
        Arena.of(model, compute_dtype_of(model))
        return M.sample_many(model, model.conv(image.cuda()), *args, **kw)


@pytest.mark.parametrize("graph", ["1", "0"], ids=["graph", "eager"])
def test_one_sample_without_greedy_draws_what_greedy_search_draws(M, specs_hash, monkeypatch, graph):
    monkeypatch.setenv("MVLT_DECODE_GRAPH", graph)
    model, _ = _tiny(M, specs_hash, F32)
    image = _image()
    want, _ = model.generate(image.cuda(), sample_mode='sample', seed=77)
    ids, sc = _many(M, model, image, 1, include_greedy=False, seed=77)
    assert ids.shape == (B, 1, 8) and sc.shape == (B, 1, 8) and ids.dtype == torch.int64 and sc.dtype == torch.float32
    assert torch.equal(ids[:, 0], want)


def test_three_samples_and_greedy_against_the_oracle_f32(M, specs_hash, monkeypatch):
    """K = 3 with the greedy row (R = 12), max_length 8: graph ids == eager ids; every pick teacher-forced against the oracle with
    host noise at rows b * 3 + k and none on the greedy rows (margin 2e-4 of the logits' spread, no wrong pick, near-ties <= 2 %);
    the scores are the oracle's log-probabilities; the greedy rows are greedy_search's; the samples of an image differ; column 0
    of the sampled rows is column 0 of the call without the greedy row, exactly."""
    model, sd = _tiny(M, specs_hash, F32)
    image = _image()
    outs = {}
    for graph in ("1", "0"):
        monkeypatch.setenv("MVLT_DECODE_GRAPH", graph)
        ids, sc = _many(M, model, image, 3, include_greedy=True, seed=77)
        assert ids.shape == (B, 4, 8) and sc.shape == (B, 4, 8)
        outs[graph] = (ids.cpu(), sc.cpu())
    assert torch.equal(outs["1"][0], outs["0"][0]), outs
    assert rel_err(outs["1"][1], outs["0"][1]) < 1e-5
    ids, sc = outs["1"]
    from mvlt_amd import decode
    noise_row, inv_t, _ = decode.multi_sample_tables(B, 3, True, 1.0, 8)
    assert noise_row.view(B, 4).tolist() == [[-1, 0, 1, 2], [-1, 3, 4, 5], [-1, 6, 7, 8]]
    O, scfg, bcfg = _tiny_oracle_cfgs()
    with torch.no_grad():
        exact, near, bad, logp = R.teacher_forced_rows(O, sd, scfg, bcfg, image, ids, 77, noise_row, inv_t)
    msg = f"{exact} exact, {near} near-ties, wrong {bad} of {ids.numel()} picks"
    print(msg)
    assert not bad and near <= S.NEAR_TIE_CAP * ids.numel(), msg
    assert rel_err(sc, logp) < 1e-4
    # the greedy rows against greedy_search: equal, or the first difference is a near-tie of the same margin
    monkeypatch.setenv("MVLT_DECODE_GRAPH", "1")
    greedy, _ = model.generate(image.cuda())
    greedy = greedy.cpu()
    for b in range(B):
        if torch.equal(ids[b, 0], greedy[b]):
            continue
        t = int((ids[b, 0] != greedy[b]).nonzero()[0])
        with torch.no_grad():
            feat = O.conv_layer(image[b:b + 1], sd, scfg)
            inp = torch.cat([greedy[b:b + 1, :t], torch.full((1, 1), bcfg.mask_token_id)], 1)
            x = O.mlm_head(O.mvlbert_forward(sd, bcfg, inp, feat, True)["hidden"][:, -1], sd, "MLM_head_seq2seq", bcfg).double()[0]
        gap = abs(float(x[ids[b, 0, t]] - x[greedy[b, t]]))
        assert gap <= 2e-4 * float(x.max() - x.mean()), (b, t, gap)
    for b in range(B):          # the samples of an image are not all one sequence, and not all the greedy one
        assert len({tuple(r) for r in ids[b, 1:].tolist()}) > 1, ids[b].tolist()
    # same step 0 and a row-independent pick: the first tokens do not depend on the greedy row being there
    alone, sc_alone = _many(M, model, image, 3, include_greedy=False, seed=77)
    assert alone.shape == (B, 3, 8)
    assert torch.equal(alone[:, :, 0].cpu(), ids[:, 1:, 0]) and torch.equal(sc_alone[:, :, 0].cpu(), sc[:, 1:, 0])


def test_early_stop_is_per_row_and_cut_at_the_last_finish(M, specs_hash, monkeypatch):
    """An eos that every row reaches, not all at one column: a finished row emits PAD, the outputs are cut at the column where the
    last row finished, and the graph loop agrees with the eager loop.  The tiny model's distribution at temperature 1 is so flat
    that two samples share no token, so the samples are drawn at temperature 0.05 (they follow their image's greedy row, whose
    tokens the rows of the two images that share one reach at different columns) and the eos is searched over at most 16 seeds,
    in the idiom of test_sample_gpu.test_sampled_early_stop_is_cut_like_the_eager_loop."""
    monkeypatch.setenv("MVLT_DECODE_GRAPH", "0")
    model, _ = _tiny(M, specs_hash, F32, max_length=20)
    image = _image()[[0, 2]]
    pad = model.config.pad_token_id
    T = 0.05
    eos = seed = None
    for cand_seed in range(16):
        full, _ = _many(M, model, image, 2, include_greedy=True, seed=cand_seed, temperature=T)
        assert full.shape == (2, 3, 20)
        rows = full.view(6, 20).cpu()[:, :19].tolist()
        common = set(rows[0]).intersection(*rows[1:]) - {pad}
        cands = [c for c in common if len({r.index(c) for r in rows}) > 1]
        if cands:
            eos, seed = max(cands, key=lambda c: max(r.index(c) for r in rows)), cand_seed
            break
    assert eos is not None, "no seed in 0..15 lets all six rows draw a common token at different columns"
    full = full.view(6, 20).cpu()
    first = [full[r].tolist().index(eos) for r in range(6)]
    stop = max(first) + 1
    outs = {}
    for graph in ("0", "1"):
        monkeypatch.setenv("MVLT_DECODE_GRAPH", graph)
        ids, sc = _many(M, model, image, 2, include_greedy=True, seed=seed, temperature=T, eos_token_id=eos)
        outs[graph] = (ids.cpu().view(6, -1), sc.cpu().view(6, -1))
    ids, sc = outs["0"]
    assert ids.shape == (6, stop) and sc.shape == (6, stop), (ids.shape, sc.shape, first)
    live = torch.zeros(6, stop, dtype=torch.bool)
    for r in range(6):
        assert torch.equal(ids[r, :first[r] + 1], full[r, :first[r] + 1])
        assert bool((ids[r, first[r] + 1:] == pad).all())
        live[r, :first[r] + 1] = True
    assert len(set(first)) > 1
    assert torch.equal(outs["1"][0], ids)
    assert rel_err(outs["1"][1][live], sc[live]) < 1e-5                  # (a finished row's scores are unspecified)
    gg = model.__dict__["_mvlt_multi_sample_graph"]
    assert gg.unfinished.tolist() == [0] * 6
    alive = gg.alive[:stop].tolist()
    assert alive[:stop - 1] == [1] * (stop - 1) and alive[stop - 1] == 0


def test_bf16_graph_equals_eager_and_the_seed_selects_the_draw(M, specs_hash, monkeypatch):
    model, _ = _tiny(M, specs_hash, BF16)
    image = _image()
    outs = {}
    for graph in ("1", "0"):
        monkeypatch.setenv("MVLT_DECODE_GRAPH", graph)
        outs[graph] = _many(M, model, image, 3, include_greedy=True, seed=5, temperature=1.2)
    assert torch.equal(outs["1"][0], outs["0"][0])
    monkeypatch.setenv("MVLT_DECODE_GRAPH", "1")
    again = _many(M, model, image, 3, include_greedy=True, seed=5, temperature=1.2)
    assert torch.equal(again[0], outs["1"][0]) and torch.equal(again[1], outs["1"][1])          # the same seed: the same bits
    other = _many(M, model, image, 3, include_greedy=True, seed=6, temperature=1.2)
    assert not torch.equal(other[0][:, 1:], outs["1"][0][:, 1:])
    assert torch.equal(other[0][:, 0], outs["1"][0][:, 0])                                     # the greedy rows draw nothing


def test_default_seed_follows_torch(M, specs_hash, monkeypatch):
    monkeypatch.setenv("MVLT_DECODE_GRAPH", "1")
    model, _ = _tiny(M, specs_hash, F32)
    image = _image()
    torch.manual_seed(11)
    a, _ = _many(M, model, image, 2)
    torch.manual_seed(11)
    b, _ = _many(M, model, image, 2)
    c, _ = _many(M, model, image, 2)
    assert torch.equal(a, b) and not torch.equal(a, c)


def test_the_multi_sample_graph_coexists_with_the_other_graphs(M, specs_hash, monkeypatch):
    from mvlt_amd import decode
    monkeypatch.setenv("MVLT_DECODE_GRAPH", "1")
    model, _ = _tiny(M, specs_hash, F32)
    fresh, _ = _tiny(M, specs_hash, F32)
    image = _image()
    img = image.cuda()
    ref, _ = fresh.generate(img)
    captures = []
    orig = decode._DecodeGraph.capture
    monkeypatch.setattr(decode._DecodeGraph, "capture",
                        lambda self: (captures.append((type(self).__name__, getattr(self, "mode", None))), orig(self))[1])
    a, sa = _many(M, model, image, 2, seed=3)
    g, _ = model.generate(img)
    s, _ = model.generate(img, sample_mode='sample', seed=3)
    b, sb = _many(M, model, image, 2, seed=3)
    c, _ = _many(M, model, image, 1, include_greedy=False, seed=3, temperature=0.9)          # another S: the slot's key changes
    g2, _ = model.generate(img)
    s2, _ = model.generate(img, sample_mode='sample', seed=3)
    assert captures == [("_MultiSampleGraph", None), ("_GreedyGraph", "greedy"), ("_GreedyGraph", "sample"), ("_MultiSampleGraph", None)], captures
    assert torch.equal(a, b) and torch.equal(sa, sb) and torch.equal(g, g2) and torch.equal(s, s2)
    assert torch.equal(g, ref)
    # one capture serves another temperature and another split of the same S into samples and greedy row
    d, _ = _many(M, model, image, 1, include_greedy=False, seed=3, temperature=0.5)
    assert len(captures) == 4 and d.shape == c.shape
    assert {"_mvlt_multi_sample_graph", "_mvlt_greedy_graph", "_mvlt_sample_graph"} <= set(model.__dict__)


def test_generate_returns_the_sampled_rows_of_sample_many(M, specs_hash, monkeypatch):
    monkeypatch.setenv("MVLT_DECODE_GRAPH", "1")
    model, _ = _tiny(M, specs_hash, F32)
    image = _image()
    ids, sc = model.generate(image.cuda(), sample_mode='sample', seed=9, temperature=0.8, num_return_sequences=3)
    want, wsc = _many(M, model, image, 3, include_greedy=False, seed=9, temperature=0.8)
    assert ids.shape == (B, 3, 8) and torch.equal(ids, want) and torch.equal(sc, wsc)
    one, _ = model.generate(image.cuda(), sample_mode='sample', seed=9, num_return_sequences=1)
    assert one.shape == (B, 8)                                          # K = 1 is today's call and today's shapes


def test_refusals(M, specs_hash):
    model, _ = _tiny(M, specs_hash, F32)
    img = _image().cuda()
    for kw in (dict(sample_mode='sample', top_k=5), dict(sample_mode='sample', top_p=0.9), dict(sample_mode='sample', num_beams=2),
               dict(sample_mode='greedy'), dict()):
        with pytest.raises(ValueError):
            model.generate(img, num_return_sequences=3, **kw)
    with pytest.raises(ValueError):
        model.generate(img, sample_mode='sample', num_return_sequences=0)
    image = _image()
    for bad in (dict(num_samples=0), dict(num_samples=2, temperature=0.0), dict(num_samples=2, repetition_penalty=0.0)):
        with pytest.raises(ValueError):
            _many(M, model, image, **bad)
    with pytest.raises(TypeError):
        _many(M, model, image, 2, top_k=5)                              # filters are no argument of the one-pass decode
    with pytest.raises(ValueError):                                     # the rules keep the V > max_length check
        _many(M, model, image, 2, max_length=3000, no_repeat_ngram_size=2)
    cfg = M.MVLBertConfigForImageCaption(hidden_size=256, num_hidden_layers=1, num_attention_heads=8, intermediate_size=256, vocab_size=3000)
    with pytest.raises(ValueError):                                     # head_dim 32: the beam attention has no such form
        M.sample_many(type("Stub", (), {"config": cfg})(), torch.zeros(1, 49, 256), 2)
