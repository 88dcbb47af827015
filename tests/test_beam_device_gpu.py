"""The beam scorer on the device: ops.beam_step (mvlt_beam_step) step by step against decode.BeamScorer on the streams of
tests/beam_step_ref.py, its refusals, and decode.beam_search on the device-scorer route (eager loop and replayed graph) against
the host-scorer route and the oracle's recompute."""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beam_step_ref as R  # noqa: E402
from conftest import synth_batch  # noqa: E402
from test_model_gpu import _tiny_caption, _tiny_oracle_cfgs  # noqa: E402
from test_sample_gpu import _tiny  # noqa: E402

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
ERR_ARG, ERR_UNSUPPORTED = -1, -3
PAST0 = 40


@pytest.fixture(scope="module")
def M():
    import mvlt_amd
    from mvlt_amd import decode  # noqa: F401  (a submodule the package does not import by itself)
    return mvlt_amd


def _load(st, step, nb):
    scores, beams, toks = step
    st.cand[0].copy_(torch.tensor(scores, dtype=torch.float32).view(torch.int32))
    st.cand[1].copy_(torch.tensor(beams, dtype=torch.int32))
    st.cand[2].copy_(torch.tensor(toks, dtype=torch.int32))


# ------------------------------------------------------------------------------------------------ the kernel against the host scorer
@pytest.mark.parametrize("case", R.cases(), ids=[c[0] for c in R.cases()])
def test_beam_step_against_the_host_scorer(M, case):
    _, plans, nb, ml, has_eos, seed = case
    G, rows = len(plans), len(plans) * nb
    eos = R.EOS if has_eos else None
    stream = R.make_stream(plans, nb, ml, seed)
    ref = R.drive(M.decode.BeamScorer, stream, G, nb, ml, eos)
    log = torch.full((ml, G, 3, 2 * nb), -1, dtype=torch.int32, device="cuda")
    st = M.decode.BeamDeviceState(G, nb, ml, R.PAD, eos, R.MASK, torch.device("cuda"), cand_log=log)
    st.reset(PAST0)
    gen = torch.Generator().manual_seed(seed)
    slot = torch.randint(0, nb, (rows, ml), generator=gen, dtype=torch.int32)          # a random table: whole rows must travel
    st.slot.copy_(slot)
    was_done = [False] * G
    for t, step in enumerate(stream):
        _load(st, step, nb)
        M.ops.beam_step(st.struct, 1 if t == 0 else nb)
        s_l, t_l, i_l, done = ref["steps"][t]
        got_s, got_ids, got_i = st.beam_scores.cpu(), st.new_ids.cpu(), st.beam_idx.cpu()
        assert [R.f32_bits(v) for v in got_s.tolist()] == [R.f32_bits(v) for v in s_l], (t, got_s, s_l)          # also 0 for done samples
        assert got_ids[:, 0].tolist() == t_l and got_ids[:, 1].tolist() == [R.MASK] * rows, (t, got_ids, t_l)
        assert got_i.tolist() == i_l, (t, got_i, i_l)
        assert [bool(v) for v in st.done.tolist()] == done, (t, st.done, done)
        assert int(st.alive[t]) == int(not all(done)) and int(st.col) == t + 1 and int(st.past) == PAST0 + t + 1 and int(st.ticket) == 0
        # the slot table of live samples: index_select by beam_idx, then the column write; done samples keep their rows
        want = slot.index_select(0, torch.tensor(i_l))
        want[:, t] = torch.arange(rows, dtype=torch.int32) % nb
        for g in range(G):
            if was_done[g]:
                want[g * nb:(g + 1) * nb] = slot[g * nb:(g + 1) * nb]
        slot = want
        assert torch.equal(st.slot.cpu(), slot), t
        lg = log[t].cpu()
        assert lg[:, 0].view(torch.float32).tolist() == step[0] and lg[:, 1].tolist() == step[1] and lg[:, 2].tolist() == step[2], t
        was_done = list(done)
    scorer, seqs, scores = st.scorer()
    for g in range(G):
        pool = scorer.hyps[g].beams
        assert [(R.f64_bits(s), h) for s, h in pool] == [(R.f64_bits(s), h) for s, h in ref["pools"][g]], (g, pool, ref["pools"][g])
        assert R.f64_bits(scorer.hyps[g].worst_score) == R.f64_bits(ref["worst"][g])
        if not was_done[g]:
            assert seqs[g * nb:(g + 1) * nb] == ref["seqs"][g * nb:(g + 1) * nb], g
    assert scorer.finalize(seqs, scores, ml, R.PAD, eos) == ref["final"]


def test_beam_step_past_max_length_writes_nothing(M):
    nb, ml = 2, 4
    st = M.decode.BeamDeviceState(1, nb, ml, R.PAD, R.EOS, R.MASK, torch.device("cuda"))
    st.reset(PAST0)
    st.col.fill_(ml)
    _load(st, R.make_stream(("none",), nb, ml, 5)[1], nb)
    before = (st.flat.clone(), st.slot.clone(), st.new_ids.clone(), st.alive.clone())
    M.ops.beam_step(st.struct, nb)
    torch.cuda.synchronize()
    after = (st.flat, st.slot, st.new_ids, st.alive)
    assert all(torch.equal(a, b) for a, b in zip(before, after)) and int(st.past) == PAST0 and int(st.ticket) == 0


def test_beam_step_refusals_launch_nothing(M):
    from mvlt_amd import _lib as L
    G, nb, ml = 2, 2, 6
    fields = [n for n, t in L.MvltBeamStep._fields_ if t is L.vp and n not in ("past", "cand_log")]
    cases = [(f"{n} NULL", {n: None}, ERR_ARG) for n in fields] + [
        ("b NULL", None, ERR_ARG),
        ("G 0", dict(G=0), ERR_ARG),
        ("num_beams 0", dict(num_beams=0), ERR_ARG),
        ("n_cand < num_beams", dict(n_cand=1), ERR_ARG),
        ("src_beams 3", dict(src_beams=3), ERR_ARG),
        ("src_beams 0", dict(src_beams=0), ERR_ARG),
        ("max_length 0", dict(max_length=0), ERR_ARG),
        ("ld_slot < max_length", dict(ld_slot=ml - 1), ERR_ARG),
        ("num_beams 9", dict(num_beams=9, n_cand=16, src_beams=9), ERR_UNSUPPORTED),
        ("n_cand 17", dict(n_cand=17), ERR_UNSUPPORTED),
        ("staging area", dict(max_length=8192 // nb + 1, ld_slot=8192 // nb + 1), ERR_UNSUPPORTED),
    ]
    stream = R.make_stream(("eos0", "none"), nb, ml, 3)
    for what, change, code in cases:
        st = M.decode.BeamDeviceState(G, nb, ml, R.PAD, R.EOS, R.MASK, torch.device("cuda"))
        _load(st, stream[0], nb)
        bufs = [st.flat, st.slot, st.past, st.ticket, st.alive, st.new_ids, st.beam_idx]
        for b in bufs:          # poison: whatever a launch wrote would show
            b.view(torch.uint8).fill_(0x5A)
        st.col.zero_()          # (a launch would find a valid column, live samples and an armed ticket)
        st.done.zero_(); st.n_hyp.zero_(); st.ticket.zero_()
        before = [b.clone() for b in bufs]
        for k, v in (change or {}).items():
            setattr(st.struct, k, v)
        rc = L.lib().mvlt_beam_step(C.byref(st.struct) if change is not None else None, None)
        torch.cuda.synchronize()
        assert rc == code, (what, rc)
        assert all(torch.equal(a, b) for a, b in zip(before, bufs)), what


# ------------------------------------------------------------------------------------------------ decode.beam_search
def _routes(model, image, nb, monkeypatch):
    """-> (host scorer, device eager, device graph, device graph again) sequences."""
    out = []
    for dev, graph in (("0", "1"), ("1", "0"), ("1", "1"), ("1", "1")):
        monkeypatch.setenv("MVLT_BEAM_DEVICE", dev)
        monkeypatch.setenv("MVLT_DECODE_GRAPH", graph)
        out.append(model(image.cuda(), None, nb, 'unilm').cpu())
    monkeypatch.delenv("MVLT_BEAM_DEVICE")
    monkeypatch.delenv("MVLT_DECODE_GRAPH")
    return out


@pytest.mark.parametrize("num_beams,B", [(3, 2), (2, 3), (5, 2)])
def test_device_beam_search_matches_host_route_and_oracle(M, specs, monkeypatch, num_beams, B):
    model, sd = _tiny_caption(M, specs, F32)
    O, scfg, bcfg = _tiny_oracle_cfgs()
    image, _, _, _ = synth_batch(B, 24, seed=80 + num_beams, vocab=3000)
    host, eager, graph, again = _routes(model, image, num_beams, monkeypatch)
    with torch.no_grad():
        ref = O.beam_decode_recompute(sd, scfg, bcfg, image, num_beams, model.config.max_length)
    assert torch.equal(host, ref), (host, ref)
    assert torch.equal(eager, ref), (eager, ref)
    assert torch.equal(graph, ref), (graph, ref)
    bg = model.__dict__["_mvlt_beam_graph"]
    assert torch.equal(again, ref) and model.__dict__["_mvlt_beam_graph"] is bg          # the second call reused the graph
    # with [END] forced early: the most likely first token of sample 0 becomes the end token
    greedy, _ = model(image.cuda(), None, 1, 'unilm')
    old = model.config.eos_token_id
    try:
        model.config.eos_token_id = int(greedy[0, 1])
        bcfg2 = O.BertCfg(vocab_size=3000, hidden_size=256, num_hidden_layers=2, num_attention_heads=4, intermediate_size=1024,
                          eos_token_id=int(greedy[0, 1]))
        host2, eager2, graph2, again2 = _routes(model, image, num_beams, monkeypatch)
        with torch.no_grad():
            ref2 = O.beam_decode_recompute(sd, scfg, bcfg2, image, num_beams, model.config.max_length)
        assert torch.equal(host2, ref2), (host2, ref2)
        assert torch.equal(eager2, ref2), (eager2, ref2)
        assert torch.equal(graph2, ref2) and torch.equal(again2, ref2), (graph2, again2, ref2)
    finally:
        model.config.eos_token_id = old


def _replay_log(M, log, B, nb, max_length, cfg_max_length, pad, eos, mask):
    """The logged candidate lists through the HOST scorer, as beam_search's host loop would: stops where it reports all done."""
    scorer = M.decode.BeamScorer(B, nb)
    input_ids = [[mask] for _ in range(B * nb)]
    s_l = None
    for t in range(max_length):
        lg = log[t]
        s_l, t_l, i_l = scorer.process(input_ids, lg[:, 0].view(torch.float32).tolist(), lg[:, 2].tolist(), lg[:, 1].tolist(), pad, eos)
        input_ids = [[k] for k in t_l] if t == 0 else [input_ids[i] + [k] for i, k in zip(i_l, t_l)]
        if scorer.is_done:
            break
    return scorer.finalize(input_ids, s_l, cfg_max_length, pad, eos), t + 1


@pytest.mark.parametrize("graph", ["0", "1"], ids=["eager", "graph"])
@pytest.mark.parametrize("with_eos", [False, True], ids=["no-eos", "eos"])
def test_device_beam_search_bf16_replays_its_own_candidates(M, specs_hash, monkeypatch, graph, with_eos):
    """bf16: the scorer is checked on the candidates of the run itself (two bf16 runs may differ at near-ties)."""
    monkeypatch.setenv("MVLT_DECODE_GRAPH", graph)
    model, _ = _tiny(M, specs_hash, BF16, max_length=8)
    B, nb, ml = 3, 4, 8
    image, _, _, _ = synth_batch(B, 24, seed=91, vocab=3000)
    cfg = model.config
    if with_eos:
        greedy, _ = model(image.cuda(), None, 1, 'unilm')
        cfg.eos_token_id = int(greedy[0, 1])
    from mvlt_amd.arena import Arena
    from mvlt_amd.runtime import compute_dtype_of
    Arena.of(model, compute_dtype_of(model))          # what MVLBertForImageCaption.forward does before it calls the conv layer
    feat = model.conv(image.cuda())
    log = torch.full((ml, B, 3, 2 * nb), -1, dtype=torch.int32, device="cuda")
    out = M.decode.beam_search(model, feat, nb, device_scorer=True, cand_log=log).cpu()
    want, steps = _replay_log(M, log.cpu(), B, nb, ml, cfg.max_length, cfg.pad_token_id, cfg.eos_token_id, 103)
    print(f"bf16 device beam search ({'graph' if graph == '1' else 'eager'}): host replay used {steps} of {ml} logged steps")
    assert out.tolist() == want, (out, want)
    assert (graph == "1") == ("_mvlt_beam_graph" in model.__dict__)


def test_nine_beams_ignore_the_device_switch(M, specs, monkeypatch):
    model, _ = _tiny_caption(M, specs, F32)
    image, _, _, _ = synth_batch(2, 24, seed=89, vocab=3000)
    plain = model(image.cuda(), None, 9, 'unilm').cpu()
    called = []
    real = M.ops.beam_step
    monkeypatch.setattr(M.ops, "beam_step", lambda *a, **kw: (called.append(1), real(*a, **kw))[1])
    monkeypatch.setenv("MVLT_BEAM_DEVICE", "1")
    dev = model(image.cuda(), None, 9, 'unilm').cpu()
    assert not called and torch.equal(dev, plain)
    dev3 = model(image.cuda(), None, 3, 'unilm')          # (and the switch does reach the new route at a shape it covers)
    assert called and dev3.shape[0] == 2
