"""``greedy_search(input_ids=, prompt_lengths=)`` on the GPU, tiny caption model: B = 3 rows continue prompts of 0 / 2 / 5 tokens
(ids from 1000..2999), 8 new tokens.  Every pick is teacher-forced against the CPU oracle on the row's own
``[prompt_b, y_<t, MASK]`` (tests/prompt_ref.py); the replayed graph against the eager loop in every mode; a decode continued
from a prefix of its own output; uniform and empty prompts; early stop; bf16; the prompted graph's own slot; ``generate``.

Near-ties of the fixed inputs (image seed 63, prompt seed 4242), from the oracle alone on the CPU: none of the 24 greedy picks
of the prompted decode and none of the 39 picks of the 13-token unprompted decode has a top-2 gap inside the f32 margin (2e-4 of
the logits' spread), so the cap of ``sample_ref.NEAR_TIE_CAP`` (0.02 of the picks) leaves room for none and none is needed."""
import inspect
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import prompt_ref as P  # noqa: E402
import sample_ref as S  # noqa: E402
from conftest import rel_err  # noqa: E402
from tiny_caption import tiny_caption as _tiny  # noqa: E402

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
B, N = P.B, P.MAX_LENGTH
_FEAT = {}


@pytest.fixture(scope="module")
def M():
    import mvlt_amd
    return mvlt_amd


def _oracle(sd):
    """(O, bcfg, image features of the three test images): computed once, shared, never written."""
    O, scfg, bcfg = P.oracle_cfgs()
    if "feat" not in _FEAT:
        with torch.no_grad():
            _FEAT["feat"] = O.conv_layer(P.image(), sd, scfg)
    return O, bcfg, _FEAT["feat"]


def _search(M, model, image, **kw):
    """greedy_search on the image tower's output, as generate() calls it -> (ids [B, n], scores [B, n_scores]) on the CPU."""
    from mvlt_amd.arena import Arena
    from mvlt_amd.runtime import compute_dtype_of
    with torch.no_grad():
        Arena.of(model, compute_dtype_of(model))
        ids, sc = M.decode.greedy_search(model, model.conv(image.cuda()), **kw)
    return ids.cpu(), sc.cpu().view(-1, ids.shape[0]).t()          # scores are concatenated step after step


def _both_loops(M, model, image, monkeypatch, **kw):
    outs = {}
    for graph in ("1", "0"):
        monkeypatch.setenv("MVLT_DECODE_GRAPH", graph)
        outs[graph] = _search(M, model, image, **kw)
    assert torch.equal(outs["1"][0], outs["0"][0]), outs
    assert outs["1"][1].shape == outs["0"][1].shape and rel_err(outs["1"][1], outs["0"][1]) < 1e-5
    return outs["1"]


def _prompt_kw():
    return dict(input_ids=P.prompts().cuda(), prompt_lengths=list(P.LENGTHS))


def test_f32_greedy_graph_and_eager_against_the_oracle(M, specs_hash, monkeypatch):
    model, sd = _tiny(M, specs_hash, F32)
    ids, sc = _both_loops(M, model, P.image(), monkeypatch, **_prompt_kw())
    assert ids.shape == (B, N) and sc.shape == (B, N) and ids.dtype == torch.int64          # the continuation only
    O, bcfg, feat = _oracle(sd)
    with torch.no_grad():
        exact, near, bad, at = P.teacher_forced(O, sd, bcfg, feat, P.prompts(), P.LENGTHS, ids)
    msg = f"{exact} exact, {near} near-ties, wrong {bad} of {ids.numel()} picks"
    print(msg)
    assert not bad and near <= S.NEAR_TIE_CAP * ids.numel(), msg
    assert rel_err(sc, at) < 1e-4                                  # the greedy score is the logit of the pick


def test_a_decode_continues_a_prefix_of_its_own_output(M, specs_hash, monkeypatch):
    """13 tokens without a prompt, then every row is given the first 1 / 3 / 5 of its own tokens: the continuation is the rest
    (a wrong position, cache slot or prefill row would change it), or the first difference is a near-tie under the oracle."""
    monkeypatch.setenv("MVLT_DECODE_GRAPH", "1")
    model, sd = _tiny(M, specs_hash, F32)
    image = P.image()
    full, _ = _search(M, model, image, max_length=13)
    assert full.shape == (B, 13)
    lens = [1, 3, 5]
    O, bcfg, feat = _oracle(sd)
    for graph in ("1", "0"):
        monkeypatch.setenv("MVLT_DECODE_GRAPH", graph)
        ids, _ = _search(M, model, image, input_ids=full[:, :5].contiguous().cuda(), prompt_lengths=lens)
        assert ids.shape == (B, N)
        for b, n in enumerate(lens):
            with torch.no_grad():
                assert P.first_difference_is_a_near_tie(O, sd, bcfg, feat[b:b + 1], full[b, :n], ids[b], full[b, n:n + N]), \
                    (graph, b, ids[b].tolist(), full[b].tolist())
    # with these inputs no row meets a near-tie (module docstring): the last decode is the rest of the first, exactly
    assert all(torch.equal(ids[b], full[b, n:n + N]) for b, n in enumerate(lens)), (ids.tolist(), full.tolist())


def test_uniform_and_empty_prompts(M, specs_hash, monkeypatch):
    model, _ = _tiny(M, specs_hash, F32)
    image = P.image()
    for graph in ("1", "0"):
        monkeypatch.setenv("MVLT_DECODE_GRAPH", graph)
        dense, sd_ = _search(M, model, image, input_ids=P.prompts().cuda())                  # the reference's case: one length
        same, ss = _search(M, model, image, input_ids=P.prompts().cuda(), prompt_lengths=[P.P_MAX] * B)
        assert torch.equal(dense, same) and torch.equal(sd_, ss)
        plain, _ = _search(M, model, image)
        empty, _ = _search(M, model, image, input_ids=P.prompts().cuda(), prompt_lengths=torch.zeros(B, dtype=torch.int64))
        none, _ = _search(M, model, image, input_ids=torch.zeros((B, 0), dtype=torch.int64, device="cuda"))
        assert torch.equal(empty, plain) and torch.equal(none, plain), (graph, empty.tolist(), none.tolist(), plain.tolist())
        assert not torch.equal(dense, plain)


def test_sampled_picks_graph_eager_and_oracle(M, specs_hash, monkeypatch):
    model, sd = _tiny(M, specs_hash, F32)
    image = P.image()
    ids, sc = _both_loops(M, model, image, monkeypatch, sample_mode='sample', seed=77, **_prompt_kw())
    assert ids.shape == (B, N)
    O, bcfg, feat = _oracle(sd)
    with torch.no_grad():
        exact, near, bad, logp = P.teacher_forced(O, sd, bcfg, feat, P.prompts(), P.LENGTHS, ids, seed=77)
    msg = f"{exact} exact, {near} near-ties, wrong {bad} of {ids.numel()} picks"
    print(msg)
    assert not bad and near <= S.NEAR_TIE_CAP * ids.numel(), msg
    assert rel_err(sc, logp) < 1e-4
    greedy, _ = _search(M, model, image, **_prompt_kw())
    assert not torch.equal(greedy, ids)
    # the filtered pick and the logit rules: the two loops against each other
    filt, _ = _both_loops(M, model, image, monkeypatch, sample_mode='sample', seed=77, top_k=50, top_p=0.9, **_prompt_kw())
    assert filt.shape == (B, N)
    ruled, _ = _both_loops(M, model, image, monkeypatch, sample_mode='sample', seed=77, repetition_penalty=1.2,
                           no_repeat_ngram_size=3, min_length=2, **_prompt_kw())
    for row in ruled.tolist():          # the rules act on the continuation as stored: it repeats no 3-gram of itself
        grams = [tuple(row[i:i + 3]) for i in range(len(row) - 2)]
        assert len(grams) == len(set(grams)), row
    gruled, _ = _both_loops(M, model, image, monkeypatch, repetition_penalty=1.2, no_repeat_ngram_size=3, min_length=2, **_prompt_kw())
    assert gruled.shape == (B, N)


def test_early_stop_is_per_row_and_cut_at_the_last_finish(M, specs_hash, monkeypatch):
    """One image three times, prompted with the first 0 / 2 / 5 tokens of its own greedy report: the rows walk the same
    sequence from different starts, so a token of it is reached at different columns.  The eos is searched among the tokens
    all three rows emit, at different columns, in the decode without an eos (the idiom of the early-stop tests of
    test_sample_gpu.py / test_multi_sample_gpu.py)."""
    monkeypatch.setenv("MVLT_DECODE_GRAPH", "0")
    model, _ = _tiny(M, specs_hash, F32, max_length=20)
    image = P.image()[[0, 0, 0]]
    pad = model.config.pad_token_id
    own, _ = _search(M, model, image[:1], max_length=5)
    kw = dict(input_ids=own.expand(B, 5).contiguous().cuda(), prompt_lengths=list(P.LENGTHS))
    full, _ = _search(M, model, image, **kw)
    assert full.shape == (B, 20)
    rows = full[:, :19].tolist()
    common = set(rows[0]).intersection(*rows[1:]) - {pad}
    cands = [c for c in common if len({r.index(c) for r in rows}) > 1]
    assert cands, f"no token reached by all rows at different columns: {rows}"
    eos = max(cands, key=lambda c: max(r.index(c) for r in rows))
    first = [full[b].tolist().index(eos) for b in range(B)]
    stop = max(first) + 1
    outs = {}
    for graph in ("0", "1"):
        monkeypatch.setenv("MVLT_DECODE_GRAPH", graph)
        outs[graph] = _search(M, model, image, eos_token_id=eos, **kw)
    ids, sc = outs["0"]
    assert ids.shape == (B, stop) and sc.shape == (B, stop - 1), (ids.shape, sc.shape, first)
    assert len(set(first)) > 1
    for b in range(B):
        assert torch.equal(ids[b, :first[b] + 1], full[b, :first[b] + 1])
        assert bool((ids[b, first[b] + 1:] == pad).all())
    assert torch.equal(outs["1"][0], ids) and outs["1"][1].shape == sc.shape
    live = torch.zeros(B, stop - 1, dtype=torch.bool)
    for b in range(B):
        live[b, :first[b] + 1] = True
    assert rel_err(outs["1"][1][live], sc[live]) < 1e-5
    gg = model.__dict__["_mvlt_prompt_graph"]
    assert gg.unfinished.tolist() == [0] * B


def test_bf16_against_the_f32_oracle(M, specs_hash, monkeypatch):
    """The margin is that of the bf16 greedy-decode test of test_model_gpu.py (its ``tol`` default): no pick outside it.  By the
    oracle's own top-2 gaps 5 of the 24 picks of these inputs lie inside that margin, so near-ties are counted, not capped."""
    import test_model_gpu
    tol = inspect.signature(test_model_gpu._teacher_forced_picks_ok).parameters["tol"].default
    model, sd = _tiny(M, specs_hash, BF16)
    ids, _ = _both_loops(M, model, P.image(), monkeypatch, **_prompt_kw())
    assert ids.shape == (B, N)
    O, bcfg, feat = _oracle(sd)
    with torch.no_grad():
        exact, near, bad, _ = P.teacher_forced(O, sd, bcfg, feat, P.prompts(), P.LENGTHS, ids, tol=tol)
    print(f"{exact} exact, {near} near-ties, wrong {bad} of {ids.numel()} picks")
    assert not bad, (bad, ids.tolist())


def test_the_prompted_graph_lives_in_a_slot_of_its_own(M, specs_hash, monkeypatch):
    from mvlt_amd import decode
    monkeypatch.setenv("MVLT_DECODE_GRAPH", "1")
    model, _ = _tiny(M, specs_hash, F32)
    image = P.image()
    captures = []
    orig = decode._DecodeGraph.capture
    monkeypatch.setattr(decode._DecodeGraph, "capture",
                        lambda self: (captures.append((type(self).__name__, getattr(self, "row_shift", None) is not None)), orig(self))[1])
    plain, _ = _search(M, model, image)
    g0 = model.__dict__["_mvlt_greedy_graph"]
    key0 = g0.key
    a, sa = _search(M, model, image, **_prompt_kw())
    assert "_mvlt_prompt_graph" in model.__dict__ and model.__dict__["_mvlt_greedy_graph"] is g0 and g0.key == key0
    gp = model.__dict__["_mvlt_prompt_graph"]
    assert gp.key[-1] == 49 + 2 + P.P_MAX + N + 1 == gp.kc[0].shape[2]          # keyed by the cache capacity
    assert gp.row_shift.tolist() == [n - P.P_MAX for n in P.LENGTHS] and g0.row_shift is None
    again, _ = _search(M, model, image)
    assert model.__dict__["_mvlt_greedy_graph"] is g0 and torch.equal(again, plain)
    other = [5, 0, 3]          # other lengths, same shapes: the table is data of the captured graph
    b, _ = _search(M, model, image, input_ids=P.prompts().cuda(), prompt_lengths=other)
    c, sc = _search(M, model, image, **_prompt_kw())
    assert model.__dict__["_mvlt_prompt_graph"] is gp
    assert captures == [("_GreedyGraph", False), ("_GreedyGraph", True)], captures
    assert torch.equal(a, c) and torch.equal(sa, sc) and not torch.equal(a, b)
    monkeypatch.setenv("MVLT_DECODE_GRAPH", "0")
    eager, _ = _search(M, model, image, input_ids=P.prompts().cuda(), prompt_lengths=other)
    assert torch.equal(eager, b)
    monkeypatch.setenv("MVLT_DECODE_GRAPH", "1")
    longer, _ = _search(M, model, image, input_ids=torch.cat([P.prompts(), P.prompts()], 1).cuda(), prompt_lengths=list(P.LENGTHS))
    assert len(captures) == 3 and torch.equal(longer, a)          # a longer P_max is another capacity; the rows' prompts are the same


def test_generate_takes_the_prompt_and_refuses_what_has_none(M, specs_hash, monkeypatch):
    monkeypatch.setenv("MVLT_DECODE_GRAPH", "1")
    model, _ = _tiny(M, specs_hash, F32)
    image = P.image()
    want, wsc = _search(M, model, image, sample_mode='sample', seed=5, temperature=0.8, **_prompt_kw())
    ids, sc = model.generate(image.cuda(), sample_mode='sample', seed=5, temperature=0.8, prompt_ids=P.prompts().cuda(),
                             prompt_lengths=list(P.LENGTHS))
    assert torch.equal(ids.cpu(), want) and torch.equal(sc.cpu().view(-1, B).t(), wsc)
    img, pr = image.cuda(), P.prompts().cuda()
    for kw in (dict(num_beams=2), dict(sample_mode='sample', num_return_sequences=2)):
        with pytest.raises(ValueError, match="prompt"):
            model.generate(img, prompt_ids=pr, **kw)
    for kw in (dict(prompt_lengths=[0, 2, 6]), dict(prompt_lengths=[0, -1, 5]), dict(prompt_lengths=[0, 2]),
               dict(prompt_lengths=torch.tensor(P.LENGTHS, device="cuda")), dict(max_length=512 - 49 - 2 - P.P_MAX)):
        with pytest.raises(ValueError):
            model.generate(img, prompt_ids=pr, **kw)
    with pytest.raises(ValueError):
        model.generate(img, prompt_ids=pr[:2])
    ok, _ = model.generate(img, prompt_ids=pr, prompt_lengths=list(P.LENGTHS))          # and the model still decodes
    assert ok.shape == (B, N)


def test_more_than_64_rows_take_the_eager_loop(M, specs_hash, monkeypatch):
    """B = 66 (the torch picks of the eager loop): the three images and prompts 22 times over decode row for row what the batch
    of three decodes, or differ first at a near-tie."""
    monkeypatch.setenv("MVLT_DECODE_GRAPH", "1")
    model, sd = _tiny(M, specs_hash, F32)
    image, pr = P.image(), P.prompts()
    small, _ = _search(M, model, image, **_prompt_kw())
    reps = 22
    big, sc = _search(M, model, image.repeat(reps, 1, 1, 1), input_ids=pr.repeat(reps, 1).cuda(), prompt_lengths=list(P.LENGTHS) * reps)
    assert big.shape == (B * reps, N) and sc.shape == (B * reps, N) and "_mvlt_prompt_graph" in model.__dict__
    O, bcfg, feat = _oracle(sd)
    for r in range(B * reps):
        b = r % B
        if not torch.equal(big[r], small[b]):
            with torch.no_grad():
                assert P.first_difference_is_a_near_tie(O, sd, bcfg, feat[b:b + 1], pr[b, :P.LENGTHS[b]], big[r], small[b]), r
