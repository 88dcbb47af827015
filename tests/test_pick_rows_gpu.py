"""The per-row MLM-head pick on the GPU (mvlt_gemm_pick_rows / _step and their _rules forms): the equivalences with the existing
heads that hold by construction, bit for bit; mixed greedy / sampled rows at three temperatures over two 64-row groups against the
float64 reference of tests/multi_sample_ref.py (whose bounds tests/test_multi_sample_cpu.py proves on these very inputs); row
independence; the step form replayed on the host; the rules form against the chunked sibling; the refusals (codes only)."""
import ctypes as C
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import multi_sample_ref as R  # noqa: E402
import sample_ref as S  # noqa: E402
from gemm_ref import check_bound  # noqa: E402

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
_cache = {}


@pytest.fixture(scope="module")
def M():
    import mvlt_amd
    return mvlt_amd


def _dev(*ts):
    return [t.cuda() for t in ts]


def _mixed(case):
    """The operands, tables and float64 reference of one of R.MIXED_CASES, computed once and left unchanged."""
    if case not in _cache:
        rows, K, N, dtype, seed = case
        A, W, bias = R.operands(rows, K, N, dtype, seed)
        noise_row, inv_t = R.mixed_tables(rows)
        _cache[case] = (A, W, bias, noise_row, inv_t, R.pick_rows_ref(A, W, bias, noise_row, inv_t, R.SEED, R.TAG))
    return _cache[case]


@pytest.mark.parametrize("dtype", [BF16, F32])
def test_sibling_equivalences_hold_bit_for_bit(M, dtype):
    """R = 40, K = 64, N = 1000 with bias (a partial row tile, a partial 16-column part).  noise_row[r] = r with a uniform inv_t:
    the tokens AND scores of mvlt_gemm_sample; noise_row = -1 with inv_t = 1: the tokens of mvlt_gemm_argmax."""
    ops = M.ops
    A, W, bias = _dev(*R.operands(40, 64, 1000, dtype, 17))
    rows = torch.arange(40, dtype=torch.int32, device="cuda")
    for T in (1.0, 0.7):
        t0, l0 = ops.gemm_sample(A, W, bias, R.SEED, R.TAG, temperature=T)
        inv_t = torch.full((40,), 1.0 / T, dtype=torch.float32, device="cuda")
        t1, l1 = ops.gemm_pick_rows(A, W, bias, rows, inv_t, R.SEED, R.TAG)
        assert torch.equal(t0, t1) and torch.equal(l0, l1), T
    g0, _ = ops.gemm_argmax(A, W, bias)
    g1, lp = ops.gemm_pick_rows(A, W, bias, torch.full_like(rows, -1), torch.ones(40, device="cuda"), R.SEED, R.TAG)
    assert torch.equal(g0, g1)
    assert bool((lp < 0).all()) and bool(torch.isfinite(lp).all())          # a log-probability, not the raw maximum logit
    assert not torch.equal(g1, t1)


@pytest.mark.parametrize("case", R.MIXED_CASES, ids=lambda c: f"R{c[0]}-K{c[1]}-N{c[2]}-{str(c[3])[6:]}")
def test_mixed_rows_against_the_f64_reference(M, case):
    """R = 70 (two groups, the second of 6 rows), every third row greedy, noise_row = (7 r + 3) % 97 elsewhere, inv_t cycling
    through 1, 1 / 0.7, 1 / 1.5: every pick the reference's or a near-tie (<= 2 %), every log-probability inside bound_lp.  The
    last case is the real head (N = 30522, K = 768, bf16)."""
    A, W, bias, noise_row, inv_t, ref = _mixed(case)
    tok, lp = M.ops.gemm_pick_rows(*_dev(A, W, bias, noise_row, inv_t), R.SEED, R.TAG)
    tok, lp = tok.cpu(), lp.cpu()
    assert bool(((tok >= 0) & (tok < case[2])).all())
    exact, near = S.assert_picks(tok, ref["y"], ref["bound_y"], f"pick_rows {case[:3]}")
    b = ref["bound_lp"](tok)
    ref_lp = R.lp_at(ref, tok)
    print(f"{case[:4]}: {exact} exact / {near} near-ties of {case[0]}; worst logprob ratio {float(((lp.double() - ref_lp).abs() / b).max()):.3f}")
    check_bound(lp.view(-1, 1), ref_lp.view(-1, 1), b.view(-1, 1), f"logprob {case[:3]}")
    # the greedy rows are the argmax of their logits, the others are not all so
    g = noise_row < 0
    assert int((tok[g] == ref["x"][g].argmax(1)).sum()) >= int(g.sum()) - 1
    assert int((tok[~g] != ref["x"][~g].argmax(1)).sum()) > 0


@pytest.mark.parametrize("case", R.MIXED_CASES[:2], ids=["bf16", "f32"])
def test_a_row_does_not_depend_on_the_other_rows(M, case):
    """Rows 64 .. 69 of the R = 70 call are bit for bit the result of a call on those 6 rows alone (another group, another
    row-tile instantiation, another R), and so are rows 10 .. 29 (inside the first group)."""
    A, W, bias, noise_row, inv_t, _ = _mixed(case)
    Ad, Wd, bd, nd, td = _dev(A, W, bias, noise_row, inv_t)
    tok, lp = M.ops.gemm_pick_rows(Ad, Wd, bd, nd, td, R.SEED, R.TAG)
    for lo, hi in ((64, 70), (10, 30)):
        t1, l1 = M.ops.gemm_pick_rows(Ad[lo:hi], Wd, bd, nd[lo:hi].contiguous(), td[lo:hi].contiguous(), R.SEED, R.TAG)
        assert torch.equal(tok[lo:hi], t1) and torch.equal(lp[lo:hi], l1), (lo, hi)


def _state(M, rows, ncol, eos, pad, tag0, past0):
    L = M._lib
    dev = torch.device("cuda")
    bufs = dict(ids=torch.full((rows, ncol), -7, dtype=torch.int64, device=dev), scores=torch.full((rows, ncol), math.nan, device=dev),
                new_ids=torch.full((rows, 2), -7, dtype=torch.int64, device=dev), col=torch.zeros(1, dtype=torch.int64, device=dev),
                past=torch.full((1,), past0, dtype=torch.int32, device=dev), ticket=torch.zeros(1, dtype=torch.int32, device=dev),
                seed=torch.full((1,), M.ops.s64(R.SEED), dtype=torch.int64, device=dev),
                unfinished=torch.ones(rows, dtype=torch.int64, device=dev), alive=torch.zeros(ncol, dtype=torch.int64, device=dev))
    g = L.MvltSampleState()
    g.has_eos, g.eos_id, g.pad_id = int(eos is not None), (eos if eos is not None else -1), pad
    g.col, g.past, g.ids, g.ld_ids, g.scores, g.ld_scores = bufs["col"].data_ptr(), bufs["past"].data_ptr(), bufs["ids"].data_ptr(), ncol, bufs["scores"].data_ptr(), ncol
    g.new_ids, g.ld_new, g.ticket, g.seed, g.tag0, g.inv_temperature = bufs["new_ids"].data_ptr(), 2, bufs["ticket"].data_ptr(), bufs["seed"].data_ptr(), tag0, 1.0
    g.unfinished, g.alive = bufs["unfinished"].data_ptr(), bufs["alive"].data_ptr()
    return g, bufs


def test_step_form_replayed_on_the_host(M):
    """R = 70, two consecutive calls of the step form with an eos that some rows draw at the first call: the ids / scores columns,
    PAD behind the eos, unfinished, alive, new_ids, col and past advanced once per call, the ticket re-armed."""
    ops = M.ops
    A, W, bias, noise_row, inv_t, _ = _mixed(R.MIXED_CASES[1])
    Ad, Wd, bd, nd, td = _dev(A, W, bias, noise_row, inv_t)
    tag0, pad = S.TAG0 + 40, 0
    picks = [ops.gemm_pick_rows(Ad, Wd, bd, nd, td, R.SEED, tag0 + c) for c in (0, 1)]
    tok1, lp1, tok2, lp2 = [t.cpu() for p in picks for t in p]
    eos = int(torch.mode(tok1).values)
    hit = tok1 == eos
    assert 1 <= int(hit.sum()) < 70
    g, b = _state(M, 70, 3, eos, pad, tag0, 11)
    for _ in range(2):
        ops.gemm_pick_rows_step(Ad, Wd, bd, g, nd, td)
    torch.cuda.synchronize()
    unf1 = (~hit).long()
    nxt2 = tok2 * unf1 + pad * (1 - unf1)
    unf2 = unf1 * (nxt2 != eos).long()
    ids, scores = b["ids"].cpu(), b["scores"].cpu()
    assert torch.equal(ids[:, 0], tok1) and torch.equal(ids[:, 1], nxt2) and bool((ids[:, 2] == -7).all())
    assert bool((ids[hit, 1] == pad).all())
    assert torch.equal(scores[:, 0], lp1) and torch.equal(scores[:, 1], lp2) and bool(torch.isnan(scores[:, 2]).all())
    assert torch.equal(b["unfinished"].cpu(), unf2)
    assert b["alive"].tolist() == [int(unf1.max()), int(unf2.max()), 0]
    assert torch.equal(b["new_ids"][:, 0].cpu(), nxt2) and bool((b["new_ids"][:, 1] == -7).all())
    assert int(b["col"]) == 2 and int(b["past"]) == 13 and int(b["ticket"]) == 0


def _history(rows, N, eos):
    """A non-trivial history [rows, 6]: random tokens, a repeated bigram (whose continuation the 2-gram rule bans), a token seen
    many times, a PAD tail, the eos inside a row."""
    gen = torch.Generator().manual_seed(rows)
    h = torch.randint(1, N, (rows, 6), generator=gen)
    h[::4, 4:] = h[::4, 0:2]                                     # ... a b x y a b  -> wait for the continuation x
    h[1::5] = h[1::5, :1]
    h[2::7, 3:] = 0
    h[3::9, 2] = eos
    return h


@pytest.mark.parametrize("dtype", [BF16, F32])
def test_rules_form_equals_the_chunked_siblings(M, dtype):
    """R = 70, penalty 1.3 + bigram ban + min length (eos banned): rows r0 .. r0 + 63 with noise_row[r] = r - r0 are what the
    chunked mvlt_gemm_sample_rules(struct(r0)) gives, tokens and scores; all rows greedy at inv_t = 1 give the tokens of the chunked
    mvlt_gemm_argmax_rules; and the rules change the result."""
    ops = M.ops
    N, eos = 1000, 77
    A, W, bias = _dev(*R.operands(70, 64, N, dtype, 23))
    hist = _history(70, N, eos)
    ids = torch.zeros((70, 8), dtype=torch.int64, device="cuda")
    ids[:, :6] = hist.cuda()
    lr = ops.LogitRules(N, 1.3, 2, 9, eos, ids, torch.full((1,), 6, dtype=torch.int64, device="cuda"))
    lr.plan()
    T = 0.7
    noise_row = (torch.arange(70, dtype=torch.int32) % 64).cuda()
    inv_t = torch.full((70,), 1.0 / T, dtype=torch.float32, device="cuda")
    tok, lp = ops.gemm_pick_rows(A, W, bias, noise_row, inv_t, R.SEED, R.TAG, rules=lr.struct())
    gtok, _ = ops.gemm_pick_rows(A, W, bias, torch.full_like(noise_row, -1), torch.ones_like(inv_t), R.SEED, R.TAG, rules=lr.struct())
    for r0 in (0, 64):
        t0, l0 = ops.gemm_sample(A[r0:r0 + 64], W, bias, R.SEED, R.TAG, temperature=T, rules=lr.struct(r0))
        assert torch.equal(tok[r0:r0 + 64], t0) and torch.equal(lp[r0:r0 + 64], l0), r0
        g0, _ = ops.gemm_argmax(A[r0:r0 + 64], W, bias, rules=lr.struct(r0))
        assert torch.equal(gtok[r0:r0 + 64], g0), r0
    plain, plp = ops.gemm_pick_rows(A, W, bias, noise_row, inv_t, R.SEED, R.TAG)
    assert not torch.equal(plp, lp)
    assert bool((tok != eos).all())                                      # min length bans the eos


# ------------------------------------------------------------------------------------------------ refusals (codes only)
def _raw(M, rows=70, Kk=64, dtype=BF16, step=False, rules=False, null=None, lda=None, alloc_rows=None, **over):
    """A direct C-ABI call on zero operands with sentinel-filled outputs; ``null``: the pointer to leave out; ``over``: MvltGemm
    fields to overwrite.  Nothing here is sized by ``rows`` when ``alloc_rows`` is given (a call that must be refused unread)."""
    L = M._lib
    dev = torch.device("cuda")
    ar = alloc_rows or rows
    A = torch.zeros((ar, 2 * Kk), dtype=dtype, device=dev)[:, :Kk]
    W = torch.zeros((64, Kk), dtype=dtype, device=dev)
    bias = torch.zeros(64, device=dev)
    noise_row = torch.arange(ar, dtype=torch.int32, device=dev)
    inv_t = torch.ones(ar, device=dev)
    p = L.MvltGemm()
    p.dtype, p.M, p.N, p.K = (1 if dtype == BF16 else 0), rows, 64, Kk
    p.A, p.lda, p.B, p.ldb = A.data_ptr(), (lda or 2 * Kk), W.data_ptr(), Kk
    p.epilogue, p.bias = L.EPI_BIAS, bias.data_ptr()
    for k, v in over.items():
        setattr(p, k, v)
    pv = torch.full((4, ar, 4), math.nan, device=dev)
    pi = torch.full((ar, 4), -7, dtype=torch.int32, device=dev)
    idx = torch.full((ar,), -7, dtype=torch.int64, device=dev)
    lp = torch.full((ar,), math.nan, device=dev)
    ptr = dict(p=C.byref(p), part_val=pv.data_ptr(), part_idx=pi.data_ptr(), noise_row=noise_row.data_ptr(), inv_t=inv_t.data_ptr(),
               out_idx=idx.data_ptr(), out_logprob=lp.data_ptr())
    outs = [pv, pi, idx, lp]
    tail = []
    if rules:
        maps = torch.zeros((2, ar, 2), dtype=torch.int32, device=dev)
        r = L.MvltLogitRules()
        r.seen, r.banned, r.ld_words, r.penalty = maps[0].data_ptr(), maps[1].data_ptr(), 2, 1.5
        for k in ("seen", "banned", "ld_words", "penalty"):
            if null == "rules." + k:
                setattr(r, k, None if k in ("seen", "banned") else 0)
        tail = [None if null == "rules" else C.byref(r)]
    st = torch.cuda.current_stream().cuda_stream
    lib = L.lib()
    if step:
        g, b = _state(M, ar, 4, None, 0, 5, 3)
        if null is not None and null.startswith("g."):
            setattr(g, null[2:], None)
        outs += [b["ids"], b["scores"], b["new_ids"]]
        counters = (b["col"], b["ticket"])
        fn = lib.mvlt_gemm_pick_rows_step_rules if rules else lib.mvlt_gemm_pick_rows_step
        args = [ptr[k] if k != null else None for k in ("p", "part_val", "part_idx", "noise_row", "inv_t")]
        rc = fn(*args, None if null == "g" else C.byref(g), *tail, st)
    else:
        counters = ()
        fn = lib.mvlt_gemm_pick_rows_rules if rules else lib.mvlt_gemm_pick_rows
        args = [ptr[k] if k != null else None for k in ("p", "part_val", "part_idx", "noise_row", "inv_t", "out_idx", "out_logprob")]
        rc = fn(*args, 1, 2, *tail, st)
    torch.cuda.synchronize()
    return rc, outs, counters


def _untouched(outs, counters):
    for t in outs:
        if t.dtype.is_floating_point:
            assert bool(torch.isnan(t).all())
        else:
            assert bool((t == -7).all())
    for t in counters:
        assert int(t) == 0


def test_refusals_return_their_code_and_write_nothing(M):
    ARG, UNSUP = -1, -3
    for step in (False, True):
        cases = [(ARG, dict(null=k)) for k in ("p", "part_val", "part_idx", "noise_row", "inv_t")]
        cases += [(ARG, dict(A=None)), (ARG, dict(B=None)), (ARG, dict(bias=None)), (ARG, dict(rows=0, alloc_rows=8)),
                  (ARG, dict(rows=-3, alloc_rows=8)), (ARG, dict(rows=1 << 26, alloc_rows=8)),          # R * N = 2^32
                  (ARG, dict(K=0)), (ARG, dict(ldb=0))]
        cases += [(UNSUP, dict(Kk=48)), (UNSUP, dict(Kk=24, dtype=F32)), (UNSUP, dict(lda=68)), (UNSUP, dict(a_kmajor=1)),
                  (UNSUP, dict(b_kmajor=1)), (UNSUP, dict(epilogue=M._lib.EPI_BIAS | M._lib.EPI_GELU))]
        if step:
            cases += [(ARG, dict(null="g"))] + [(ARG, dict(null="g." + f)) for f in ("seed", "col", "ticket", "ids", "scores", "new_ids")]
        else:
            cases += [(ARG, dict(null="out_idx")), (ARG, dict(null="out_logprob"))]
        for want, kw in cases:
            rc, outs, counters = _raw(M, step=step, **kw)
            assert rc == want, (step, kw, rc)
            _untouched(outs, counters)
        for kw in (dict(null="rules"), dict(null="rules.seen"), dict(null="rules.banned"), dict(null="rules.ld_words"), dict(null="rules.penalty")):
            rc, outs, counters = _raw(M, step=step, rules=True, **kw)
            assert rc == ARG, (step, kw, rc)
            _untouched(outs, counters)
        for rules in (False, True):          # and the same call with nothing missing runs: 70 rows, two groups
            rc, outs, counters = _raw(M, step=step, rules=rules)
            assert rc == 0, (step, rules, rc)
            if step:
                assert int(counters[0]) == 1 and int(counters[1]) == 0
                assert bool(((outs[4][:, 0] >= 0) & (outs[4][:, 0] < 64)).all()) and bool(torch.isfinite(outs[5][:, 0]).all())
            else:
                # zero operands, noise row r: the token is the argmax of the noise, the score log(1 / 64)
                assert bool(((outs[2] >= 0) & (outs[2] < 64)).all()) and bool(((outs[3] - math.log(1 / 64)).abs() < 1e-5).all())
