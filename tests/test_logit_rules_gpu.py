"""The logit rules on the GPU (repetition penalty, no-repeat n-grams, min length): the plan kernel's bitmaps word for word, the
rule-aware heads (mvlt_gemm_*_rules) exactly on integer operands and within per-element bounds on random ones, the refusals, and
greedy_search(repetition_penalty=, no_repeat_ngram_size=, min_length=) on the graph, eager and chunked routes against the
restatement of tests/logit_rules_ref.py.

Near-ties of the bounded head test, counted on the CPU for exactly these inputs (logit_rules_ref.at_risk over the 6 shapes x 4
rule sets = 656 picks each): greedy 4 of 656, sampled 0 of 656 reference picks lie within the sum of their two bounds; the cap
of sample_ref.NEAR_TIE_CAP allows 13."""
import ctypes as C
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import logit_rules_ref as R  # noqa: E402
import sample_filter_ref as F  # noqa: E402
import sample_ref as S  # noqa: E402
from conftest import synth_batch  # noqa: E402
from tiny_caption import tiny_caption as _tiny  # noqa: E402

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
ROWS = (1, 17, 64)
_cache = {}


@pytest.fixture(scope="module")
def M():
    import mvlt_amd
    return mvlt_amd


def _rules(M, V, rule, eos, history, cap=None):
    """ops.LogitRules over a device copy of `history` (int64 [rows, c]) with col = c, the plan already run."""
    rows, c = history.shape
    ids = torch.zeros((rows, cap or max(c, 1)), dtype=torch.int64, device="cuda")
    ids[:, :c] = history.cuda()
    lr = M.ops.LogitRules(V, rule[0], rule[1], rule[2], eos, ids, torch.full((1,), c, dtype=torch.int64, device="cuda"))
    lr.plan()
    return lr


# ------------------------------------------------------------------------------------------------ the plan
def _plan_history(V):
    """M = 5 rows x 12 tokens: a bigram / trigram pattern that repeats, one token many times (in the ragged last word), a PAD
    tail, planted repeats among random tokens, and a row that holds the eos."""
    gen = torch.Generator().manual_seed(V)
    h = torch.randint(1, V, (5, 12), generator=gen)
    h[0] = torch.tensor([7, 8, 9, 7, 8, 31, 7, 8, 32, 7, 8, 9])
    h[1] = V - 1
    h[2, 5:] = 0
    h[3, 9:] = h[3, 2:5]
    h[4, 3], h[4, 11] = R.EOS, V - 2
    return h


@pytest.mark.parametrize("V", [200, 4106])
def test_plan_bitmaps_equal_the_reference_word_for_word(M, V):
    L = M._lib
    h = _plan_history(V)
    nw = (V + 31) // 32
    ids = h.cuda()
    col = torch.zeros(1, dtype=torch.int64, device="cuda")
    for g, min_length, eos in ((0, 0, None), (1, 0, None), (2, 5, R.EOS), (3, 20, R.EOS), (4, 12, R.EOS), (2, 13, None)):
        for c in sorted({0, 1, max(g - 1, 0), 12}):
            maps = torch.full((2, 5, nw + 1), 0x5A5A5A5A, dtype=torch.int32, device="cuda")          # one guard word behind each row
            r = L.MvltLogitRules()
            r.seen, r.banned, r.ld_words, r.penalty = maps[0].data_ptr(), maps[1].data_ptr(), nw + 1, 1.5
            r.ids, r.ld_ids, r.col, r.ngram, r.min_length = ids.data_ptr(), 12, col.data_ptr(), g, min_length
            r.eos_id, r.has_eos = (eos if eos is not None else -1), int(eos is not None)
            col.fill_(c)
            for _ in range(2):          # stateless: a second run over the filled maps gives the same words
                assert L.lib().mvlt_decode_rules_plan(C.byref(r), 5, V, torch.cuda.current_stream().cuda_stream) == 0
            got = maps.cpu()
            seen, banned = R.bitmaps(h[:, :c], V, g, min_length, eos)
            assert torch.equal(got[0, :, :nw], seen) and torch.equal(got[1, :, :nw], banned), (V, g, min_length, eos, c)
            assert bool((got[:, :, nw] == 0x5A5A5A5A).all()), "guard word written"
            if c == 12 and g >= 1:
                assert int(banned.ne(0).sum()) > 0
    assert int(col) == 12 and torch.equal(ids.cpu(), h)          # the plan writes nothing but the maps


# ------------------------------------------------------------------------------------------------ greedy head, exact
def _int_operands(rows, dtype):
    """|a|, |w| <= 4, K = 64, N = 200, integer bias: every logit is an exact integer in f32 (and the operands exact in bf16).
    Columns 20 and 150 are copies of one weight row with bias + 3000: the row maximum, twice."""
    gen = torch.Generator().manual_seed(rows)
    A = torch.randint(-4, 5, (rows, 64), generator=gen).to(dtype)
    W = torch.randint(-4, 5, (200, 64), generator=gen).to(dtype)
    bias = torch.randint(-50, 51, (200,), generator=gen).float()
    W[150], bias[150] = W[20], bias[20]
    bias[20] += 3000.0
    bias[150] += 3000.0
    return A, W, bias


@pytest.mark.parametrize("dtype", [BF16, F32])
@pytest.mark.parametrize("rows", ROWS)
def test_greedy_head_is_exact_on_integer_operands(M, rows, dtype):
    A, W, bias = _int_operands(rows, dtype)
    x = A.float() @ W.float().t() + bias          # exact integers
    Ad, Wd, bd = A.cuda(), W.cuda(), bias.cuda()
    t0, v0 = M.ops.gemm_argmax(Ad, Wd, bd)
    assert bool((t0.cpu() == 20).all()) and torch.equal(v0.cpu(), x[:, 20])          # the tie goes to the first index
    second = torch.where(torch.arange(200)[None] == 20, -math.inf, torch.where(torch.arange(200)[None] == 150, -math.inf, x)).argmax(1)
    gen = torch.Generator().manual_seed(7)
    rnd = torch.randint(0, 200, (rows, 6), generator=gen)
    rnd = rnd.masked_fill((rnd == 20) | (rnd == 150), 3)
    cases = []
    cases.append(("unseen tie", (2.0, 0, 0), None, rnd))                                                    # neither twin seen: 20
    h = rnd.clone(); h[:, 2] = 20
    cases.append(("first twin penalised", (2.0, 0, 0), None, h))                                           # 150 wins
    h = rnd.clone(); h[:, 1], h[:, 4] = 20, 150
    cases.append(("both twins penalised", (2.0, 0, 0), None, h))                                           # x / 2 twice: 20 again
    cases.append(("penalty below one", (0.5, 0, 0), None, h))
    h = rnd.clone(); h[:, 0], h[:, 3], h[:, 5] = 20, 150, second
    cases.append(("banned maxima", (2.0, 1, 0), None, h))                                                  # g = 1: the top three are banned
    h = rnd.clone(); h[:, 0], h[:, 1], h[:, 5] = 9, 20, 9
    cases.append(("bigram ban + min length", (0.5, 2, 9), 150, h))                                         # 20 follows 9, 150 is the eos
    for what, rule, eos, hist in cases:
        lr = _rules(M, 200, rule, eos, hist)
        tok, val = M.ops.gemm_argmax(Ad, Wd, bd, rules=lr.struct())
        ref = R.process(x, hist, rule[0], rule[1], rule[2], eos)
        want = ref.argmax(1)          # first index of the maximum
        assert torch.equal(tok.cpu(), want), (what, tok.cpu(), want)
        assert torch.equal(val.cpu(), ref.gather(1, want[:, None]).squeeze(1)), what          # bit for bit
        assert not bool(R.sets(hist, 200, rule[1], rule[2], eos)[1].gather(1, tok.cpu()[:, None]).any()), what
    assert bool((R.process(x, cases[1][3], 2.0).argmax(1) == 150).all()) and bool((R.process(x, cases[2][3], 2.0).argmax(1) == 20).all())
    assert not bool(((want == 20) | (want == 150)).any())


# ------------------------------------------------------------------------------------------------ heads, bounded
def _case(rows, dtype):
    """Operands, the unprocessed reference and the history of one shape: computed once, shared, never changed."""
    key = (rows, dtype)
    if key not in _cache:
        A, W, bias = F.operands(rows, dtype, 100 + rows)
        base = S.sample_ref(A, W, bias, F.SEED, S.TAG0)
        _cache[key] = (A, W, bias, A.cuda(), W.cuda(), bias.cuda(), base, R.bounded_history(base))
    return _cache[key]


@pytest.mark.parametrize("dtype", [BF16, F32])
def test_greedy_and_sampled_heads_within_bounds(M, dtype):
    """N = 4106, K = 256: every pick is the reference's or a near-tie by sample_ref.classify_picks; the greedy score within the
    processed logit's bound, the sampled score within bound_lp; no banned token; the rules change the picks."""
    g_near = s_near = total = changed_g = changed_s = 0
    for rows in ROWS:
        A, W, bias, Ad, Wd, bd, base, hist = _case(rows, dtype)
        t_plain, _ = M.ops.gemm_argmax(Ad, Wd, bd)
        s_plain, _ = M.ops.gemm_sample(Ad, Wd, bd, F.SEED, S.TAG0)
        for rule in R.RULE_SETS:
            ref = R.processed(base, hist, *rule, R.EOS, F.SEED, S.TAG0)
            lr = _rules(M, F.N, rule, R.EOS, hist)
            tok, val = M.ops.gemm_argmax(Ad, Wd, bd, rules=lr.struct())
            stok, lp = M.ops.gemm_sample(Ad, Wd, bd, F.SEED, S.TAG0, rules=lr.struct())
            tok, val, stok, lp = tok.cpu(), val.cpu().double(), stok.cpu(), lp.cpu().double()
            what = f"M={rows} {dtype} {rule}"
            assert not bool(ref["banned"].gather(1, tok[:, None]).any()) and not bool(ref["banned"].gather(1, stok[:, None]).any()), what
            e, n, bad = S.classify_picks(tok, ref["x"], ref["bound_x"])
            print(f"{what}: greedy {e} exact, {n} near, {len(bad)} wrong; at risk {R.at_risk(ref, 'x')}")
            assert not bad, (what, bad[:4])
            g_near += n
            dv = (val - ref["x"].gather(1, tok[:, None]).squeeze(1)).abs() / ref["bound_x"].gather(1, tok[:, None]).squeeze(1)
            assert float(dv.max()) <= 1.0, (what, float(dv.max()))
            e, n, bad = S.classify_picks(stok, ref["y"], ref["bound_y"])
            print(f"{what}: sampled {e} exact, {n} near, {len(bad)} wrong; at risk {R.at_risk(ref, 'y')}")
            assert not bad, (what, bad[:4])
            s_near += n
            want_lp = ref["x"].gather(1, stok[:, None]).squeeze(1) - ref["lse"]
            dl = (lp - want_lp).abs() / ref["bound_lp"](stok)
            assert float(dl.max()) <= 1.0, (what, float(dl.max()))
            total += rows
            changed_g += int((tok != t_plain.cpu()).sum())
            changed_s += int((stok != s_plain.cpu()).sum())
            if rule[1] >= 1:          # the reference's own unprocessed argmax and sampled token are banned: every pick moved
                assert bool((tok != base["x"].argmax(1)).all()) and bool((stok != base["tok"]).all()), what
    print(f"{dtype}: near-ties greedy {g_near}, sampled {s_near} of {total}; picks changed by the rules: {changed_g}, {changed_s}")
    assert g_near <= S.NEAR_TIE_CAP * total and s_near <= S.NEAR_TIE_CAP * total
    assert changed_g >= total // 2 and changed_s >= total // 2


@pytest.mark.parametrize("filt", [(8, 1.0), (0, 0.9)])
def test_filtered_head_with_rules(M, filt):
    near = total = 0
    for dtype in (BF16, F32):
        for rows in ROWS:
            A, W, bias, Ad, Wd, bd, base, hist = _case(rows, dtype)
            for rule in R.RULE_SETS:
                pr = R.processed(base, hist, *rule, R.EOS, F.SEED, S.TAG0)
                ref = F.filter_ref(A, W, bias, F.SEED, S.TAG0, filt[0], filt[1], base=pr)
                lr = _rules(M, F.N, rule, R.EOS, hist)
                tok, lp = M.ops.gemm_sample_filtered(Ad, Wd, bd, F.SEED, S.TAG0, top_k=filt[0], top_p=filt[1], rules=lr.struct())
                what = f"M={rows} {dtype} {rule} {filt}"
                assert not bool(pr["banned"].gather(1, tok.cpu()[:, None]).any()), what
                exact, n, wrong, ratio = F.classify(ref, tok, lp)
                assert not wrong and ratio <= 1.0, (what, wrong[:4], ratio)
                near, total = near + n, total + rows
    print(f"{filt}: {near} near-ties of {total}")
    assert near <= S.NEAR_TIE_CAP * total


def test_top_k_above_the_number_of_unbanned_columns(M):
    """V = 48, g = 1 bans the (up to 12) seen tokens, top_k = 47 asks for more columns than are left: the threshold falls to
    -inf, every unbanned column is kept, no banned one is drawn, the score is renormalised over the unbanned columns."""
    A, W, bias = F.operands(17, BF16, 5, n=48)
    base = S.sample_ref(A, W, bias, F.SEED, S.TAG0)
    hist = torch.randint(0, 48, (17, 12), generator=torch.Generator().manual_seed(3))
    hist[:, 0], hist[:, 1] = base["x"].argmax(1), base["tok"]
    rule = (1.0, 1, 0)
    lr = _rules(M, 48, rule, None, hist)
    for tag in range(S.TAG0, S.TAG0 + 8):
        pr = R.processed(base, hist, *rule, None, F.SEED, tag)
        assert int((~pr["banned"]).sum(1).max()) < 47
        ref = F.filter_ref(A, W, bias, F.SEED, tag, 47, 1.0, base=pr)
        tok, lp = M.ops.gemm_sample_filtered(A.cuda(), W.cuda(), bias.cuda(), F.SEED, tag, top_k=47, rules=lr.struct())
        assert not bool(pr["banned"].gather(1, tok.cpu()[:, None]).any())
        _, _, wrong, ratio = F.classify(ref, tok, lp)
        assert not wrong and ratio <= 1.0, (wrong[:4], ratio)
        want = pr["x"].gather(1, tok.cpu()[:, None]).squeeze(1) - pr["lse"]
        assert float((lp.cpu().double() - want).abs().max()) < 1e-4


# ------------------------------------------------------------------------------------------------ refusals
def _raw(M, entry, rows=8, null=None, ld_words=2, penalty=1.5, ngram=2, min_length=0):
    """A direct C-ABI call (N = 64, K = 64, bf16) with NaN / -7 filled outputs, scratch and maps; returns (rc, buffers)."""
    L = M._lib
    dev = torch.device("cuda")
    A = torch.zeros((rows, 64), dtype=BF16, device=dev)
    W = torch.zeros((64, 64), dtype=BF16, device=dev)
    p = L.MvltGemm()
    p.dtype, p.M, p.N, p.K, p.A, p.lda, p.B, p.ldb = 1, rows, 64, 64, A.data_ptr(), 64, W.data_ptr(), 64
    pv = torch.full((4, rows, 4), math.nan, device=dev)
    pi = torch.full((rows, 4), -7, dtype=torch.int32, device=dev)
    ws = torch.full((rows, 64), math.nan, device=dev)
    idx = torch.full((rows,), -7, dtype=torch.int64, device=dev)
    out = torch.full((rows,), math.nan, device=dev)
    maps = torch.full((2, rows, 2), -7, dtype=torch.int32, device=dev)
    hist = torch.full((rows, 4), -7, dtype=torch.int64, device=dev)
    hcol = torch.zeros(1, dtype=torch.int64, device=dev)
    r = L.MvltLogitRules()
    r.seen, r.banned = (None if null == "seen" else maps[0].data_ptr()), (None if null == "banned" else maps[1].data_ptr())
    r.ld_words, r.penalty, r.ngram, r.min_length = ld_words, penalty, ngram, min_length
    r.ids, r.ld_ids, r.col = (None if null == "ids" else hist.data_ptr()), 4, (None if null == "col" else hcol.data_ptr())
    rp = None if null == "rules" else C.byref(r)
    st = torch.cuda.current_stream().cuda_stream
    lib = L.lib()
    if entry == "plan":
        rc = lib.mvlt_decode_rules_plan(rp, rows, 64, st)
        outs = (maps, hist, hcol)
    elif entry == "argmax":
        rc = lib.mvlt_gemm_argmax_rules(C.byref(p), pv.data_ptr(), pi.data_ptr(), idx.data_ptr(), out.data_ptr(), rp, st)
        outs = (pv, pi, idx, out, maps)
    elif entry == "sample":
        rc = lib.mvlt_gemm_sample_rules(C.byref(p), pv.data_ptr(), pi.data_ptr(), idx.data_ptr(), out.data_ptr(), 1, 2, 1.0, rp, st)
        outs = (pv, pi, idx, out, maps)
    elif entry == "filtered":
        f = L.MvltSampleFilter()
        f.top_k, f.top_p, f.x, f.ldx, f.row0 = 4, 0.9, ws.data_ptr(), 64, 0
        rc = lib.mvlt_gemm_sample_filtered_rules(C.byref(p), pv.data_ptr(), pi.data_ptr(), C.byref(f), idx.data_ptr(), out.data_ptr(), 1, 2, 1.0,
                                                 rp, st)
        outs = (pv, pi, ws, idx, out, maps)
    else:
        ids = torch.full((rows, 4), -7, dtype=torch.int64, device=dev)
        scores = torch.full((rows, 4), math.nan, device=dev)
        new_ids = torch.full((rows, 2), -7, dtype=torch.int64, device=dev)
        col = torch.zeros(1, dtype=torch.int64, device=dev)
        ticket = torch.zeros(1, dtype=torch.int32, device=dev)
        seed = torch.zeros(1, dtype=torch.int64, device=dev)
        g = L.MvltSampleState() if entry != "greedy_step" else L.MvltGreedyState()
        g.has_eos, g.col, g.ids, g.ld_ids, g.scores, g.ld_scores = 0, col.data_ptr(), ids.data_ptr(), 4, scores.data_ptr(), 4
        g.new_ids, g.ld_new, g.ticket = new_ids.data_ptr(), 2, ticket.data_ptr()
        if entry != "greedy_step":
            g.seed, g.tag0, g.inv_temperature = seed.data_ptr(), 5, 1.0
        if entry == "greedy_step":
            rc = lib.mvlt_gemm_argmax_greedy_rules(C.byref(p), pv.data_ptr(), pi.data_ptr(), C.byref(g), rp, st)
        elif entry == "sample_step":
            rc = lib.mvlt_gemm_sample_step_rules(C.byref(p), pv.data_ptr(), pi.data_ptr(), C.byref(g), rp, st)
        else:
            f = L.MvltSampleFilter()
            f.top_k, f.top_p, f.x, f.ldx, f.row0 = 4, 0.9, ws.data_ptr(), 64, 0
            rc = lib.mvlt_gemm_sample_filtered_step_rules(C.byref(p), pv.data_ptr(), pi.data_ptr(), C.byref(f), C.byref(g), rp, st)
        outs = (pv, pi, ws, ids, scores, new_ids, col, ticket, maps)
    torch.cuda.synchronize()
    return rc, outs


def _untouched(outs):
    for t in outs:
        if t.dtype.is_floating_point:
            assert bool(torch.isnan(t).all())
        elif t.numel() > 1:
            assert bool((t == -7).all())
        else:
            assert int(t) == 0


def test_refusals_write_nothing(M):
    ARG = -1
    heads = ("argmax", "greedy_step", "sample", "sample_step", "filtered", "filtered_step")
    for entry in heads + ("plan",):
        for kw in (dict(null="rules"), dict(null="seen"), dict(null="banned"), dict(ld_words=1), dict(penalty=0.0), dict(penalty=-2.0),
                   dict(penalty=math.nan), dict(ngram=-1), dict(rows=65)):
            rc, outs = _raw(M, entry, **kw)
            assert rc == ARG, (entry, kw, rc)
            _untouched(outs)
    for kw in (dict(null="ids"), dict(null="col"), dict(min_length=-1)):
        rc, outs = _raw(M, "plan", **kw)
        assert rc == ARG, kw
        _untouched(outs)
    rc, outs = _raw(M, "plan")                       # and the same calls run when nothing is wrong: col = 0, empty maps
    assert rc == 0 and bool((outs[0] == 0).all())
    for entry in heads:
        rc, outs = _raw(M, entry, penalty=1.0, ngram=0)          # (the maps hold -7: bits set, a legal input)
        assert rc == 0, entry


# ------------------------------------------------------------------------------------------------ model level
ML = 12
RULES_KW = dict(repetition_penalty=1.3, no_repeat_ngram_size=2, min_length=5)


def _model(M, specs_hash, eos=None):
    return _tiny(M, specs_hash, F32, max_length=ML, eos=eos)


def _images(n, seed=63):
    return synth_batch(n, 24, seed=seed, vocab=3000)[0]


def _run(model, img, **kw):
    ids, sc = model(img, None, 1, 'unilm', **kw)
    return ids.cpu(), sc.cpu()


def test_graph_equals_eager_and_the_graphs_coexist(M, specs_hash, monkeypatch):
    """Greedy, sampled and filtered decoding with rules: graph == eager token for token; the calls in mixed order and twice give
    the same outputs (every keyed graph recaptures in its mode's slot); the defaults are the call without the arguments."""
    model, _ = _model(M, specs_hash)
    img = _images(3).cuda()
    plain = _run(model, img)
    eos = int(plain[0][0, 0])
    model.config.eos_token_id = eos
    calls = [dict(RULES_KW), dict(sample_mode='sample', seed=5, **RULES_KW), dict(),
             dict(sample_mode='sample', seed=5, top_k=8, **RULES_KW), dict(no_repeat_ngram_size=1), dict(sample_mode='sample', seed=5),
             dict(sample_mode='sample', seed=5, top_p=0.9, repetition_penalty=2.0)]
    outs = {}
    for graph in ("1", "0"):
        monkeypatch.setenv("MVLT_DECODE_GRAPH", graph)
        first = [_run(model, img, **kw) for kw in calls]
        again = [_run(model, img, **kw) for kw in reversed(calls)][::-1]
        for kw, a, b in zip(calls, first, again):
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), kw
        outs[graph] = first
    for kw, a, b in zip(calls, outs["1"], outs["0"]):
        assert torch.equal(a[0], b[0]) and a[1].shape == b[1].shape, (kw, a[0], b[0])
        assert a[1].numel() == 0 or float((a[1] - b[1]).abs().max()) < 1e-5, kw
    first = outs["1"]
    assert not torch.equal(first[0][0], first[2][0]) and not torch.equal(first[4][0], first[2][0])          # the rules are in the key
    monkeypatch.setenv("MVLT_DECODE_GRAPH", "1")
    d = _run(model, img, repetition_penalty=1.0, no_repeat_ngram_size=0, min_length=0)
    assert torch.equal(d[0], first[2][0]) and torch.equal(d[1], first[2][1])                                # bit for bit
    d = _run(model, img, sample_mode='sample', seed=5, repetition_penalty=1.0, no_repeat_ngram_size=0, min_length=0)
    assert torch.equal(d[0], first[5][0]) and torch.equal(d[1], first[5][1])
    V = model.MLM_head_seq2seq.predictions.decoder.out_features
    for bad in (dict(repetition_penalty=0.0), dict(repetition_penalty=math.nan), dict(no_repeat_ngram_size=-1), dict(min_length=-2)):
        with pytest.raises(ValueError):
            model(img, None, 1, 'unilm', **bad)
    with pytest.raises(ValueError, match="beam"):
        model(img, None, 2, 'unilm', min_length=3)
    from mvlt_amd.decode import greedy_search
    with pytest.raises(ValueError, match="vocabulary"):
        greedy_search(model, model.conv(img), max_length=V, no_repeat_ngram_size=2)


@pytest.mark.parametrize("graph", ["1", "0"])
def test_no_repeated_bigram_and_min_length(M, specs_hash, monkeypatch, graph):
    monkeypatch.setenv("MVLT_DECODE_GRAPH", graph)
    model, _ = _model(M, specs_hash)
    img = _images(3).cuda()
    plain, _ = _run(model, img)
    grams = lambda row: list(zip(row[:-1], row[1:]))
    assert any(len(set(grams(r))) < len(grams(r)) for r in plain.tolist()), "the unconstrained decode repeats no bigram: nothing to test"
    ids, _ = _run(model, img, no_repeat_ngram_size=2)
    assert ids.shape == (3, ML)
    for r in ids.tolist():
        assert len(set(grams(r))) == len(grams(r)), r
    for mode in (dict(), dict(sample_mode='sample', seed=3)):
        ids, _ = _run(model, img, no_repeat_ngram_size=2, **mode)
        for r in ids.tolist():
            assert len(set(grams(r))) == len(grams(r)), r
    # min length: eos = the first token of the unconstrained row 0 -- without the rule row 0 finishes at column 0
    eos = int(plain[0, 0])
    model.config.eos_token_id = eos
    short, _ = _run(model, img)
    assert short.shape[1] < 6 or bool((short[0, 1:] == model.config.pad_token_id).all())
    for mode in (dict(), dict(sample_mode='sample', seed=3)):
        ids, _ = _run(model, img, min_length=5, **mode)
        assert ids.shape[1] >= 6 or ids.shape[1] == ML, ids
        assert not bool((ids[:, :5] == eos).any()), ids                                          # no row finishes before column 5


ORACLE_CASES = [(63, dict(no_repeat_ngram_size=2)), (63, dict(no_repeat_ngram_size=3)), (64, dict(repetition_penalty=1.3)),
                (64, dict(repetition_penalty=1.3, no_repeat_ngram_size=3, min_length=5))]


@pytest.mark.parametrize("seed,kw", ORACLE_CASES)
def test_greedy_with_rules_teacher_forced_against_the_oracle(M, specs_hash, monkeypatch, seed, kw):
    """Every pick of the graph loop against the CPU oracle's logits on the generated prefix with the restatement of the rules
    applied: the oracle's processed argmax, or a near-tie within SAFETY (e_ref + e_pick), e_x = 1e-4 (top - mean logit), scaled by
    max(p, 1 / p) on a penalised column -- and no more near-ties than the cap (none, at 36 picks).  The output differs from the
    unconstrained decode."""
    from test_sample_gpu import _tiny_oracle_cfgs
    monkeypatch.setenv("MVLT_DECODE_GRAPH", "1")
    model, sd = _model(M, specs_hash)
    image = _images(3, seed)
    plain, _ = _run(model, image.cuda())
    eos = None
    if kw.get("min_length"):
        eos = int(plain[0, 0])
        model.config.eos_token_id = eos
    ids, sc = _run(model, image.cuda(), **kw)
    n = ids.shape[1]
    assert not torch.equal(ids, plain[:, :n])
    sc = sc.view(-1, 3).t()
    pen, g, ml = kw.get("repetition_penalty", 1.0), kw.get("no_repeat_ngram_size", 0), kw.get("min_length", 0)
    O, scfg, bcfg = _tiny_oracle_cfgs()
    exact = near = 0
    alive = torch.ones(3, dtype=torch.bool)
    with torch.no_grad():
        feat = O.conv_layer(image, sd, scfg)
        for t in range(n):
            inp = torch.cat([ids[:, :t], torch.full((3, 1), bcfg.mask_token_id)], 1)
            x = O.mlm_head(O.mvlbert_forward(sd, bcfg, inp, feat, True)["hidden"][:, -1], sd, "MLM_head_seq2seq", bcfg).double()
            e_x = (1e-4 * (x.max(-1).values - x.mean(-1)))[:, None].expand_as(x)
            seen, _ = R.sets(ids[:, :t], x.shape[1], g, ml, eos)
            xp = R.process(x, ids[:, :t], pen, g, ml, eos)
            e = torch.where(seen, e_x * max(pen, 1.0 / pen), e_x)
            want = xp.argmax(1)
            for b in range(3):
                if not alive[b]:
                    continue                      # a finished row emits PAD
                tok = int(ids[b, t])
                assert math.isfinite(float(xp[b, tok])), (b, t, tok, "a banned token")
                gap, allowed = float(xp[b, want[b]] - xp[b, tok]), S.SAFETY * float(e[b, want[b]] + e[b, tok])
                assert gap <= allowed, (b, t, tok, int(want[b]), gap, allowed)
                exact, near = exact + (tok == int(want[b])), near + (tok != int(want[b]))
                if t < sc.shape[1]:
                    assert abs(float(sc[b, t]) - float(xp[b, tok])) <= S.SAFETY * float(e[b, tok]) + 2.0 ** -23 * abs(float(xp[b, tok]))
            if eos is not None:
                alive &= ids[:, t] != eos
    print(f"{seed} {kw}: {exact} exact, {near} near-ties")
    assert near <= S.NEAR_TIE_CAP * (exact + near)


def test_batch_of_70_runs_in_row_chunks_through_the_fused_heads(M, specs_hash, monkeypatch):
    """B = 70 with rules never reaches the torch picks: greedy goes through the fused argmax in chunks of 64, sampled through the
    filtered pick with both filters off, and the shared rows equal the B = 64 decode (graph route)."""
    model, _ = _model(M, specs_hash)
    img = _images(70).cuda()

    def boom(*a, **k):
        raise AssertionError("a torch pick on the rules route")
    monkeypatch.setattr(torch, "multinomial", boom)
    monkeypatch.setattr(M.ops, "argmax", boom)
    for mode in (dict(), dict(sample_mode='sample', seed=9)):
        kw = dict(repetition_penalty=1.3, no_repeat_ngram_size=2, **mode)
        ids70, sc70 = _run(model, img, **kw)
        ids64, sc64 = _run(model, img[:64].contiguous(), **kw)
        assert ids70.shape == (70, ML) and torch.equal(ids70[:64], ids64), mode
        # (sampled: the filtered finish sums the row in another order than the part-wise finish of the B = 64 graph)
        assert torch.allclose(sc70.view(ML, 70)[:, :64], sc64.view(ML, 64), rtol=0, atol=1e-4 if mode else 1e-5)
        for r in ids70.tolist():
            assert len(set(zip(r[:-1], r[1:]))) == ML - 1, r
