"""Logit rules in beam search.  Head level: the plan over int32 beam histories (mvlt_beam_rules_plan) bit for bit against
logit_rules_ref.bitmaps and the rule-aware candidate head (mvlt_gemm_beam_candidates_rules) against the float64 reference and
classify of tests/beam_rules_ref.py.  Model level: decode.beam_search with rules on its three routes against each other and against
a host recompute from the oracle's public functions, and MVLBertForImageCaption.generate."""
import ctypes as C
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beam_ref as B  # noqa: E402
import beam_rules_ref as R  # noqa: E402
import logit_rules_ref as LR  # noqa: E402
import sample_filter_ref as F  # noqa: E402
import sample_ref as S  # noqa: E402
from conftest import synth_batch  # noqa: E402
from test_model_gpu import _tiny_caption, _tiny_oracle_cfgs  # noqa: E402
from test_sample_gpu import _tiny  # noqa: E402
from tiny_caption import tiny_caption  # noqa: E402

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
ERR_ARG, ERR_UNSUPPORTED = -1, -3
OFF = (1.0, 0, 0)
JUNK = 7                      # what the history buffers hold beyond column c: a plan that read it would set its bit


@pytest.fixture(scope="module")
def M():
    import mvlt_amd
    from mvlt_amd import decode  # noqa: F401  (a submodule the package does not import by itself)
    return mvlt_amd


def _split(out):
    """(beam, tok, score) of the [3, G, n] int32 buffer of ops.gemm_beam_candidates."""
    return out[1], out[2], out[0].view(torch.float32)


def _rules(M, V, rules, eos, hist, ld):
    """ops.BeamLogitRules over a device copy of `hist` (int64 [rows, c]) in an int32 buffer [rows, ld >= c] filled with JUNK, col = c."""
    rows, c = hist.shape
    seq = torch.full((rows, ld), JUNK, dtype=torch.int32)
    seq[:, :c] = hist.to(torch.int32)
    return M.ops.BeamLogitRules(V, *rules, eos, seq.cuda(), torch.tensor([c], dtype=torch.int64, device="cuda"))


def _assert_maps(lr, hist, V, rules, eos, what):
    seen, banned = LR.bitmaps(hist, V, rules[1], rules[2], eos)
    assert torch.equal(lr.maps[0].cpu(), seen), what
    assert torch.equal(lr.maps[1].cpu(), banned), what


# ------------------------------------------------------------------------------------------------ head level
@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("G,nb", B.CASES)
def test_plan_and_candidates_against_host_reference(M, G, nb, dtype):
    A, W, bias, bs = R.case_operands(G, nb, dtype)
    V = W.shape[0]
    base = S.sample_ref(A, W, bias, 0, 0)
    ref0 = B.beam_ref(A, W, bias, bs, nb, 2 * nb)
    Ad, Wd, bd, bsd = A.cuda(), W.cuda(), bias.cuda(), bs.cuda()
    for rules in LR.RULE_SETS:
        for c, ld in ((R.C_HIST, 16), (0, 16), (R.C_HIST, R.C_HIST)):          # c = 12, c = 0 (only min_length bears), c = ld_seq
            what = f"G={G} beams={nb} {dtype} rules={rules} c={c} ld={ld}"
            hist = R.histories(ref0, c)
            ref = R.beam_rules_ref(A, W, bias, bs, nb, 2 * nb, hist, *rules, eos=R.EOS, ref0=ref0, base=base)
            lr = _rules(M, V, rules, R.EOS, hist, ld)
            lr.plan()
            _assert_maps(lr, hist, V, rules, R.EOS, what)
            out, lse = M.ops.gemm_beam_candidates(Ad, Wd, bd, bsd, nb, 2 * nb, want_lse=True, rules=lr.struct)
            _, _, worst = R.assert_lists(ref, *_split(out), what)
            assert worst <= 1.0, what
            # a banned entry stays inside lse: the one of the unprocessed row
            assert float(((lse.cpu().double() - ref0["lse"]).abs() / ref0["bound_s"].min(1).values).max()) <= 1.0, what
            lr.plan()                                                            # stateless: the same maps and lists again
            out2, _ = M.ops.gemm_beam_candidates(Ad, Wd, bd, bsd, nb, 2 * nb, rules=lr.struct)
            _assert_maps(lr, hist, V, rules, R.EOS, what)
            assert torch.equal(out, out2), what


def test_plan_rows_beyond_the_old_limit_and_a_stale_map(M):
    """160 rows in one launch (32 samples x 5 beams), a ragged last bitmap word, ids outside [0, V) and maps that start full."""
    rows, V, c = 160, 200, 9
    gen = torch.Generator().manual_seed(5)
    hist = torch.randint(0, V, (rows, c), generator=gen)
    hist[::7, 3] = V + 4
    hist[1::7, 2] = -1
    hist[:, c - 2:] = hist[:, 1:3]                       # the last bigram occurred at 1 .. 2
    for rules in ((1.5, 2, 12), (1.0, 1, 0), (1.2, 3, 9)):
        lr = _rules(M, V, rules, 11, hist, 12)
        lr.maps.fill_(-1)
        lr.plan()
        _assert_maps(lr, hist, V, rules, 11, rules)
        lr.maps.fill_(-1)
        lr.plan(37)                                      # the first 37 rows only
        seen, banned = LR.bitmaps(hist, V, rules[1], rules[2], 11)
        assert torch.equal(lr.maps[0, :37].cpu(), seen[:37]) and torch.equal(lr.maps[1, :37].cpu(), banned[:37])
        assert bool((lr.maps[:, 37:] == -1).all())


def test_candidates_with_rules_at_the_real_size(M):
    """M = 40 rows (20 samples x 2 beams), N = 30522 (a partial last bitmap word), K = 768, bf16."""
    A, W, bias, bs = R.case_operands(0, 0, BF16, big=True)
    nb, V = B.BIG["num_beams"], B.BIG["N"]
    base = S.sample_ref(A, W, bias, 0, 0)
    ref0 = B.beam_ref(A, W, bias, bs, nb, 2 * nb)
    rules = LR.RULE_SETS[2]
    hist = R.histories(ref0)
    hist[3, 5] = V - 1                                    # the last column of the vocabulary, in the partial word
    ref = R.beam_rules_ref(A, W, bias, bs, nb, 2 * nb, hist, *rules, eos=R.EOS, ref0=ref0, base=base)
    lr = _rules(M, V, rules, R.EOS, hist, 16)
    lr.plan()
    _assert_maps(lr, hist, V, rules, R.EOS, "real size")
    out, _ = M.ops.gemm_beam_candidates(A.cuda(), W.cuda(), bias.cuda(), bs.cuda(), nb, 2 * nb, rules=lr.struct)
    _, _, worst = R.assert_lists(ref, *_split(out), "real size")
    assert worst <= 1.0


def test_small_vocabulary_exactly_n_cand_and_fewer(M):
    """N = 48, 1-gram histories: sample 0 keeps exactly n_cand = 4 unbanned entries (46 distinct tokens in both rows), sample 1
    only 3 (46 and 47): its last slot is (-inf, 0, 0), and no index leaves its range."""
    N, nb, n = 48, 2, 4
    A, W, bias = F.operands(4, BF16, 301, n=N)
    bs = torch.tensor([-0.5, -1.25, -0.75, -2.0])
    gen = torch.Generator().manual_seed(9)
    hist = torch.stack([torch.randperm(N, generator=gen)[:47] for _ in range(4)])
    for m in (0, 1, 2):
        hist[m, 46] = hist[m, 0]                           # rows 0 .. 2: 46 distinct tokens, row 3: 47
    rules = (1.0, 1, 0)
    ref = R.beam_rules_ref(A, W, bias, bs, nb, n, hist, *rules)
    assert ref["valid"].tolist() == [4, 3] and int(ref["banned"].sum()) == 3 * 46 + 47
    lr = _rules(M, N, rules, None, hist, 48)
    lr.plan()
    _assert_maps(lr, hist, N, rules, None, "N = 48")
    out = torch.full((3, 2, n), -7, dtype=torch.int32, device="cuda")
    M.ops.gemm_beam_candidates(A.cuda(), W.cuda(), bias.cuda(), bs.cuda(), nb, n, out=out, rules=lr.struct)
    beam, tok, score = (v.cpu() for v in _split(out))
    exact, near, wrong, worst = R.classify(ref, beam, tok, score)
    assert not wrong and exact + near == 2 and worst <= 1.0, (wrong, beam, tok, score)
    assert score[1, 3] == -math.inf and int(beam[1, 3]) == 0 and int(tok[1, 3]) == 0
    assert bool(torch.isfinite(score[0]).all()) and bool(torch.isfinite(score[1, :3]).all())
    # every column of every row banned: four empty slots per sample
    full = torch.arange(N)[None, :].repeat(4, 1)
    lr = _rules(M, N, rules, None, full, 48)
    lr.plan()
    out.fill_(-7)
    M.ops.gemm_beam_candidates(A.cuda(), W.cuda(), bias.cuda(), bs.cuda(), nb, n, out=out, rules=lr.struct)
    beam, tok, score = (v.cpu() for v in _split(out))
    assert bool((score == -math.inf).all()) and not bool(beam.any()) and not bool(tok.any())


def test_constructed_ties_come_back_in_flat_index_order(M):
    G, nb, n = 2, 2, 4
    A, W, bias, bs = B.case_operands(3, 2, BF16)
    A, bs = A[:G * nb].clone(), bs[:G * nb].clone()
    bs[1] = -3.0
    ref0 = B.beam_ref(A, W, bias, bs, nb, n)
    N = ref0["N"]
    t = int(ref0["flat"][0, 0]) % N
    assert int(ref0["flat"][0, 0]) // N == 0 and 7 < t < N - 8
    W0, bias0 = W, bias
    W, bias = W.clone(), bias.clone()
    for j in (t - 7, t + 8):
        W[j], bias[j] = W[t], bias[t]
    dev = [v.cuda() for v in (A, W, bias, bs)]
    # (1) the three bit-equal entries of beam 0 all seen: one penalised score, three times, in index order
    # (a penalty below 1 RAISES a log-probability: the three stay at the head of the list)
    hist = torch.tensor([[t + 8, t, t - 7]] * (G * nb))
    lr = _rules(M, N, (0.75, 0, 0), None, hist, 4)
    lr.plan()
    out, _ = M.ops.gemm_beam_candidates(*dev, nb, n, rules=lr.struct)
    beam, tok, score = (v.cpu() for v in _split(out))
    ref = R.beam_rules_ref(A, W, bias, bs, nb, n, hist, 0.75)
    assert torch.equal(beam.long() * N + tok.long(), ref["flat"]), (beam, tok, ref["flat"])
    where = [i for i in range(n) if int(beam[0, i]) == 0 and int(tok[0, i]) in (t - 7, t, t + 8)]
    assert where == [0, 1, 2] and tok[0, where].tolist() == [t - 7, t, t + 8] and score[0, where[0]] == score[0, where[1]] == score[0, where[2]]
    # (2) the middle one banned (a 1-gram history of t alone in the row of beam 0): its twins lead, in index order
    hist = torch.tensor([[t], [0], [0], [0]])
    lr = _rules(M, N, (1.0, 1, 0), None, hist, 4)
    lr.plan()
    out, _ = M.ops.gemm_beam_candidates(*dev, nb, n, rules=lr.struct)
    beam, tok, score = (v.cpu() for v in _split(out))
    assert beam[0, :2].tolist() == [0, 0] and tok[0, :2].tolist() == [t - 7, t + 8] and score[0, 0] == score[0, 1]
    assert t not in tok[0][beam[0] == 0].tolist()
    ref = R.beam_rules_ref(A, W, bias, bs, nb, n, hist, 1.0, 1)
    assert torch.equal(beam.long() * N + tok.long(), ref["flat"])
    # (3) every score of a sample equal (zero activations and bias): more ties than the candidate list holds, so the
    # round-by-round form -- the first 16 UNBANNED flat indices, in order
    Z = torch.zeros(2, A.shape[1], dtype=BF16)
    hist = torch.tensor([[0, 3], [1, 1]])
    lr = _rules(M, N, (1.0, 1, 0), None, hist, 4)
    lr.plan()
    out, _ = M.ops.gemm_beam_candidates(Z.cuda(), W0.cuda(), torch.zeros_like(bias0).cuda(), torch.tensor([-1.5, -1.5]).cuda(), 2, 16,
                                        rules=lr.struct)
    beam, tok, score = (v.cpu() for v in _split(out))
    assert beam[0].tolist() == [0] * 16 and tok[0].tolist() == [1, 2] + list(range(4, 18)) and bool((score[0] == score[0, 0]).all())


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
def test_rules_off_is_the_plain_entry_bit_for_bit(M, dtype):
    for G, nb in ((3, 2), (13, 5)):
        A, W, bias, bs = (v.cuda() for v in R.case_operands(G, nb, dtype))
        V = W.shape[0]
        plain, lse0 = M.ops.gemm_beam_candidates(A, W, bias, bs, nb, 2 * nb, want_lse=True)
        hist = R.histories(B.beam_ref(*R.case_operands(G, nb, dtype), nb, 2 * nb))
        for c in (0, R.C_HIST):          # penalty 1 on seen tokens is exact; no n-gram, no min length: nothing banned
            lr = _rules(M, V, OFF, R.EOS, hist[:, :c], 16)
            lr.plan()
            assert not bool(lr.maps[1].any()) and bool(lr.maps[0].any()) == (c > 0)
            got, lse = M.ops.gemm_beam_candidates(A, W, bias, bs, nb, 2 * nb, want_lse=True, rules=lr.struct)
            assert torch.equal(got, plain) and torch.equal(lse, lse0), (G, nb, c)


def test_refusals_launch_nothing(M):
    from mvlt_amd import _lib as L
    G, nb, n = 3, 2, 4
    A, W, bias, bs = (v.cuda() for v in R.case_operands(G, nb, BF16))
    N = W.shape[0]
    rows, ldx, nw = A.shape[0], (N + 3) // 4 * 4, (N + 31) // 32
    A9 = torch.cat([A, A[:3]])
    cases = [
        ("rules NULL", "rules", None, A, ERR_ARG), ("seen NULL", "r", dict(seen=None), A, ERR_ARG),
        ("banned NULL", "r", dict(banned=None), A, ERR_ARG), ("ld_words short", "r", dict(ld_words=nw - 1), A, ERR_ARG),
        ("penalty 0", "r", dict(penalty=0.0), A, ERR_ARG), ("penalty NaN", "r", dict(penalty=math.nan), A, ERR_ARG),
        ("ngram -1", "r", dict(ngram=-1), A, ERR_ARG),
        ("beam_scores NULL", "c", dict(beam_scores=None), A, ERR_ARG), ("x NULL", "c", dict(x=None), A, ERR_ARG),
        ("cand_tok NULL", "c", dict(cand_tok=None), A, ERR_ARG), ("num_beams 0", "c", dict(num_beams=0), A, ERR_ARG),
        ("n_cand 0", "c", dict(n_cand=0), A, ERR_ARG), ("M % num_beams", "c", dict(num_beams=4), A, ERR_ARG),
        ("ldx < N", "c", dict(ldx=N - 1), A, ERR_ARG), ("num_beams 9", "c", dict(num_beams=9), A9, ERR_UNSUPPORTED),
        ("n_cand 17", "c", dict(n_cand=17), A, ERR_UNSUPPORTED), ("k-major operand", "p", dict(a_kmajor=1), A, ERR_UNSUPPORTED),
        ("K not a whole number of k-blocks", "p", dict(K=A.shape[1] - 1), A, ERR_UNSUPPORTED),
    ]
    for what, where, change, Ad, code in cases:
        r_ = Ad.shape[0]
        ws = torch.full((r_, ldx), float("nan"), device="cuda")
        score = torch.full((r_, 17), float("nan"), device="cuda")
        cb = torch.full((r_, 17), -7, dtype=torch.int32, device="cuda")
        ct = torch.full((r_, 17), -7, dtype=torch.int32, device="cuda")
        lse = torch.full((r_,), float("nan"), device="cuda")
        maps = torch.zeros((2, r_, nw), dtype=torch.int32, device="cuda")
        p, _, _ = M.ops._head_gemm(Ad, W, bias)
        c = L.MvltBeamCand()
        for k, v in dict(beam_scores=torch.zeros(r_, device="cuda"), x=ws, cand_score=score, cand_beam=cb, cand_tok=ct, lse=lse).items():
            setattr(c, k, v.data_ptr())
        c.num_beams, c.n_cand, c.ldx = nb, n, ldx
        r = L.MvltLogitRules()
        r.seen, r.banned, r.ld_words, r.penalty = maps[0].data_ptr(), maps[1].data_ptr(), nw, 1.3
        for k, v in (change or {}).items():
            setattr({"r": r, "c": c, "p": p}[where], k, v)
        rc = L.lib().mvlt_gemm_beam_candidates_rules(C.byref(p), C.byref(c), C.byref(r) if where != "rules" else None, None)
        torch.cuda.synchronize()
        assert rc == code, (what, rc)
        assert bool(torch.isnan(ws).all()) and bool(torch.isnan(score).all()) and bool(torch.isnan(lse).all()), what
        assert bool((cb == -7).all()) and bool((ct == -7).all()), what
    # the plan
    V, rows_ = 200, 5
    seq = torch.zeros((rows_, 8), dtype=torch.int32, device="cuda")
    col = torch.full((1,), 4, dtype=torch.int64, device="cuda")
    for what, change, args in [
        ("rules NULL", None, {}), ("seen NULL", dict(seen=None), {}), ("banned NULL", dict(banned=None), {}), ("col NULL", dict(col=None), {}),
        ("ld_words short", dict(ld_words=6), {}), ("penalty 0", dict(penalty=0.0), {}), ("ngram -1", dict(ngram=-1), {}),
        ("min_length -1", dict(min_length=-1), {}), ("seq NULL", {}, dict(seq=None)), ("ld_seq 0", {}, dict(ld_seq=0)),
        ("rows 0", {}, dict(rows=0)), ("V 0", {}, dict(V=0)),
    ]:
        maps = torch.full((2, rows_, 7), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        r = L.MvltLogitRules()
        r.seen, r.banned, r.ld_words, r.penalty, r.col, r.ngram = maps[0].data_ptr(), maps[1].data_ptr(), 7, 1.3, col.data_ptr(), 2
        for k, v in (change or {}).items():
            setattr(r, k, v)
        a = dict(seq=seq.data_ptr(), ld_seq=8, rows=rows_, V=V)
        a.update(args)
        rc = L.lib().mvlt_beam_rules_plan(C.byref(r) if change is not None else None, a["seq"], a["ld_seq"], a["rows"], a["V"], None)
        torch.cuda.synchronize()
        assert rc == ERR_ARG, (what, rc)
        assert bool((maps == 0x5A5A5A5A).all()), what


# ------------------------------------------------------------------------------------------------ decode.beam_search
MODEL_RULES = [(p, g, min(ml, 6)) for p, g, ml in LR.RULE_SETS]          # min_length below the tiny model's max_length = 10


def _search(M, model, image, nb, rules, monkeypatch, fused="1", device="0", graph="1"):
    monkeypatch.setenv("MVLT_BEAM_FUSED", fused)
    monkeypatch.setenv("MVLT_BEAM_DEVICE", device)
    monkeypatch.setenv("MVLT_DECODE_GRAPH", graph)
    from mvlt_amd.arena import Arena
    from mvlt_amd.runtime import compute_dtype_of
    Arena.of(model, compute_dtype_of(model))          # what MVLBertForImageCaption.forward does before it calls the conv layer
    with torch.no_grad():
        feat = model.conv(image.cuda())
    kw = dict(repetition_penalty=rules[0], no_repeat_ngram_size=rules[1], min_length=rules[2]) if rules is not None else {}
    return M.decode.beam_search(model, feat, nb, **kw).cpu()


def _all_routes(M, model, image, nb, rules, monkeypatch):
    """-> (plain, fused, device eager, device graph) sequences."""
    return [_search(M, model, image, nb, rules, monkeypatch, *sw) for sw in (("0", "0", "1"), ("1", "0", "1"), ("1", "1", "0"), ("1", "1", "1"))]


def _recompute(M, O, sd, scfg, bcfg, image, nb, max_len, cfg_max_len, rules, eos, pad=0):
    """beam_search by full-sequence recompute from the oracle's public functions (conv_layer, mvlbert_forward, mlm_head), the rules
    on the log_softmax rows by logit_rules_ref.process, the host scorer of the package (pinned by test_beam_gpu.py)."""
    feat = O.conv_layer(image, sd, scfg).repeat_interleave(nb, dim=0)
    Bn, V, mask = image.shape[0], bcfg.vocab_size, bcfg.mask_token_id
    scorer = M.decode.BeamScorer(Bn, nb)
    beam_scores = torch.zeros(Bn, nb)
    beam_scores[:, 1:] = -1e9
    beam_scores = beam_scores.view(-1)
    gen = torch.zeros(Bn * nb, 0, dtype=torch.long)
    input_ids = [[mask] for _ in range(Bn * nb)]
    for cur_len in range(max_len):
        inp = torch.cat([gen, torch.full((Bn * nb, 1), mask)], 1)
        logits = O.mlm_head(O.mvlbert_forward(sd, bcfg, inp, feat, True)["hidden"][:, -1], sd, "MLM_head_seq2seq", bcfg)
        lp = LR.process(torch.log_softmax(logits, -1), gen, *rules, eos)
        top_s, top_t = torch.topk((lp + beam_scores[:, None]).view(Bn, nb * V), 2 * nb, dim=1, largest=True, sorted=True)
        s_l, t_l, i_l = scorer.process(input_ids, top_s.tolist(), (top_t % V).tolist(), torch.div(top_t, V, rounding_mode="floor").tolist(),
                                       pad, eos)
        tok = torch.tensor(t_l)
        gen = tok[:, None] if cur_len == 0 else torch.cat([gen[torch.tensor(i_l)], tok[:, None]], 1)
        input_ids, beam_scores = gen.tolist(), torch.tensor(s_l, dtype=torch.float32)
        if scorer.is_done or cur_len + 1 >= max_len:
            break
    return torch.tensor(scorer.finalize(input_ids, beam_scores.tolist(), cfg_max_len, pad, eos), dtype=torch.int64)


def _check_properties(out, rules, eos, pad=0):
    """No g-gram twice before the padding, no eos before min_length."""
    _, g, min_length = rules
    for row in out.tolist():
        seq = row[:row.index(eos) + 1] if eos in row else row
        if eos in row:
            assert row.index(eos) >= min_length, (row, rules)
        if g >= 1:
            grams = [tuple(seq[i:i + g]) for i in range(len(seq) - g + 1)]
            assert len(grams) == len(set(grams)), (row, rules)


@pytest.mark.parametrize("num_beams,Bn", [(3, 2), (5, 2)])
def test_beam_search_with_rules_on_every_route(M, specs_hash, monkeypatch, num_beams, Bn):
    """The tiny caption model with the hash weights: its unconstrained beams repeat tokens and bigrams (the formula weights give
    one repeat-free sequence for every image, on which no rule bears)."""
    model, sd = tiny_caption(M, specs_hash, F32, max_length=10)
    O, scfg, bcfg = _tiny_oracle_cfgs()
    image, _, _, _ = synth_batch(Bn, 24, seed=80 + num_beams, vocab=3000)
    ml = model.config.max_length
    old = model.config.eos_token_id
    base = _search(M, model, image, num_beams, None, monkeypatch)
    try:
        # [END] = a token of the unconstrained best sequence of sample 0, so that it is likely early and min_length bears
        eos = model.config.eos_token_id = int(base[0, 1])
        off = _search(M, model, image, num_beams, None, monkeypatch)
        changed = 0
        for rules in MODEL_RULES:
            plain, fused, eager, graph = _all_routes(M, model, image, num_beams, rules, monkeypatch)
            with torch.no_grad():
                ref = _recompute(M, O, sd, scfg, bcfg, image, num_beams, ml, ml, rules, eos)
            print(f"beams={num_beams} rules={rules}: {fused.tolist()} (rules off: {off.tolist()})")
            assert torch.equal(fused, ref), (rules, fused, ref)
            assert torch.equal(plain, ref), (rules, plain, ref)
            assert torch.equal(eager, ref), (rules, eager, ref)
            assert torch.equal(graph, ref), (rules, graph, ref)
            _check_properties(fused, rules, eos)
            differs = fused.shape != off.shape or not torch.equal(fused, off)
            assert differs, (rules, fused, off)          # the rules bear: at least one sample is not the unconstrained one
            changed += int(differs)
        assert changed == len(MODEL_RULES)
    finally:
        model.config.eos_token_id = old


def test_beam_search_with_rules_bf16_routes_agree(M, specs_hash, monkeypatch):
    model, _ = _tiny(M, specs_hash, BF16, max_length=8)
    nb = 4
    image, _, _, _ = synth_batch(3, 24, seed=91, vocab=3000)
    base = _search(M, model, image, nb, None, monkeypatch)
    eos = model.config.eos_token_id = int(base[0, 1])
    for rules in [(p, g, min(ml, 5)) for p, g, ml in LR.RULE_SETS]:
        _, fused, eager, graph = _all_routes(M, model, image, nb, rules, monkeypatch)
        assert torch.equal(fused, eager) and torch.equal(fused, graph), (rules, fused, eager, graph)
        _check_properties(fused, rules, eos)


def test_rules_at_their_off_values_are_the_call_without_them(M, specs, monkeypatch):
    from mvlt_amd import decode
    model, _ = _tiny_caption(M, specs, F32)
    image, _, _, _ = synth_batch(2, 24, seed=83, vocab=3000)
    captures = []
    orig = decode._BeamGraph.capture
    monkeypatch.setattr(decode._BeamGraph, "capture", lambda self: (captures.append(self.key), orig(self))[1])
    called = []
    real = M.ops.beam_rules_plan
    monkeypatch.setattr(M.ops, "beam_rules_plan", lambda *a, **kw: (called.append(1), real(*a, **kw))[1])
    for sw in (("1", "0", "1"), ("1", "1", "1")):          # the fused route, the device graph
        without = _search(M, model, image, 3, None, monkeypatch, *sw)
        at_off = _search(M, model, image, 3, OFF, monkeypatch, *sw)
        assert torch.equal(without, at_off)
    assert len(captures) == 1 and "rules" not in captures[0] and not called
    with_rules = _search(M, model, image, 3, (1.0, 2, 0), monkeypatch, "1", "1", "1")
    assert len(captures) == 2 and captures[1][-4:] == ("rules", 1.0, 2, 0) and called and with_rules.shape[0] == 2


def test_generate_reaches_the_rules_and_forward_still_refuses(M, specs, monkeypatch):
    for name in ("MVLT_BEAM_FUSED", "MVLT_BEAM_DEVICE", "MVLT_DECODE_GRAPH"):
        monkeypatch.delenv(name, raising=False)
    model, _ = _tiny_caption(M, specs, F32)
    image, _, _, _ = synth_batch(2, 24, seed=83, vocab=3000)
    got = model.generate(image.cuda(), num_beams=3, no_repeat_ngram_size=2).cpu()
    want = _search(M, model, image, 3, (1.0, 2, 0), monkeypatch, "1", "0", "1")
    assert torch.equal(got, want)
    _check_properties(got, (1.0, 2, 0), model.config.eos_token_id)
    dev = model.generate(image.cuda(), num_beams=3, no_repeat_ngram_size=2, device_scorer=True).cpu()
    assert torch.equal(dev, want)
    assert torch.equal(model.generate(image.cuda(), num_beams=3).cpu(), model(image.cuda(), None, 3, 'unilm').cpu())
    ids, scores = model.generate(image.cuda(), num_beams=1, no_repeat_ngram_size=2)
    ids2, scores2 = model(image.cuda(), None, 1, 'unilm', no_repeat_ngram_size=2)
    assert torch.equal(ids, ids2) and torch.equal(scores, scores2)
    with pytest.raises(ValueError, match="generate"):
        model(image.cuda(), None, 3, 'unilm', no_repeat_ngram_size=2)
    with pytest.raises(ValueError, match="beam"):
        model.generate(image.cuda(), num_beams=3, sample_mode='sample')
