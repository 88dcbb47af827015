"""The filtered sampled pick on the GPU (mvlt_gemm_sample_filtered / _step: top-k, then top-p, fused behind the Gumbel-max MLM
head) against the float64 reference and rules of tests/sample_filter_ref.py, and greedy_search(top_k=, top_p=) on the graph,
eager and chunked routes."""
import ctypes as C
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sample_filter_ref as F  # noqa: E402
import sample_ref as S  # noqa: E402
from conftest import rel_err, synth_batch  # noqa: E402
from test_sample_gpu import _teacher_forced_sampled, _tiny, _tiny_oracle_cfgs  # noqa: E402,F401

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
ROWS = (1, 17, 64)
_cache = {}


@pytest.fixture(scope="module")
def M():
    import mvlt_amd
    return mvlt_amd


def _case(rows, dtype):
    """Operands (host + device) and the unfiltered reference of one shape, computed once and shared (never changed)."""
    key = (rows, dtype)
    if key not in _cache:
        A, W, bias = F.operands(rows, dtype, 100 + rows)
        _cache[key] = (A, W, bias, A.cuda(), W.cuda(), bias.cuda(), S.sample_ref(A, W, bias, F.SEED, S.TAG0))
    return _cache[key]


def _check(ref, tok, score, what):
    exact, near, wrong, ratio = F.classify(ref, tok, score)
    assert not wrong, (what, wrong[:4])
    return exact, near, ratio


@pytest.mark.parametrize("dtype", [BF16, F32])
@pytest.mark.parametrize("rows", ROWS)
def test_filters_off_is_the_unfiltered_pick(M, rows, dtype):
    """Both filters off inside mvlt_gemm_sample_filtered: the tokens of mvlt_gemm_sample bit for bit (x bit-identical, the same
    noise index), both scores within their bound of the reference."""
    A, W, bias, Ad, Wd, bd, base = _case(rows, dtype)
    for tag in (S.TAG0, S.TAG0 + 1):
        t0, l0 = M.ops.gemm_sample(Ad, Wd, bd, F.SEED, tag)
        t1, l1 = M.ops.gemm_sample_filtered(Ad, Wd, bd, F.SEED, tag, top_k=0, top_p=1.0)
        assert torch.equal(t0, t1), (t0, t1)
        ref = F.filter_ref(A, W, bias, F.SEED, tag, 0, 1.0, base=base)
        assert bool(ref["IN"].all())
        for lp in (l0, l1):
            _, _, ratio = _check(ref, t1, lp, f"off M={rows} {dtype}")
            assert ratio <= 1.0, ratio


@pytest.mark.parametrize("dtype", [BF16, F32])
def test_filtered_pick_against_host_reference(M, dtype):
    exact = near = total = 0
    worst = 0.0
    for rows in ROWS:
        A, W, bias, Ad, Wd, bd, base = _case(rows, dtype)
        for top_k, top_p in F.FILTERS:
            for tag in (S.TAG0, S.TAG0 + 1):
                ref = F.filter_ref(A, W, bias, F.SEED, tag, top_k, top_p, base=base)
                tok, lp = M.ops.gemm_sample_filtered(Ad, Wd, bd, F.SEED, tag, top_k=top_k, top_p=top_p)
                e, n, ratio = _check(ref, tok, lp, f"M={rows} k={top_k} p={top_p} tag={tag:#x}")
                assert ratio <= 1.0, (rows, top_k, top_p, ratio)
                exact, near, total, worst = exact + e, near + n, total + rows, max(worst, ratio)
        # top_k = 1 is the greedy pick wherever the top two logits are further apart than their bounds
        tok, _ = M.ops.gemm_sample_filtered(Ad, Wd, bd, F.SEED, S.TAG0, top_k=1)
        am, _ = M.ops.gemm_argmax(Ad, Wd, bd)
        top2 = torch.topk(base["x"], 2, dim=1)
        gap = top2.values[:, 0] - top2.values[:, 1]
        clear = gap > S.SAFETY * (base["e_x"].gather(1, top2.indices).sum(1))
        assert int(clear.sum()) >= rows - 1
        assert torch.equal(tok.cpu()[clear], am.cpu()[clear]) and torch.equal(tok.cpu()[clear], top2.indices[:, 0][clear])
    print(f"{dtype}: {exact} exact, {near} near-ties of {total} picks; worst score ratio {worst:.3f}")
    assert near <= S.NEAR_TIE_CAP * total, (near, total)


def test_filtered_pick_at_the_real_size(M):
    """M = 64, K = 768, N = 30522, bf16, (50, 0.9)."""
    A, W, bias = F.operands(64, BF16, 7, n=30522, k=768)
    ref = F.filter_ref(A, W, bias, F.SEED, S.TAG0 + 2, 50, 0.9)
    tok, lp = M.ops.gemm_sample_filtered(A.cuda(), W.cuda(), bias.cuda(), F.SEED, S.TAG0 + 2, top_k=50, top_p=0.9)
    exact, near, ratio = _check(ref, tok, lp, "real size")
    print(f"real size: {exact} exact, {near} near-ties of 64; worst score ratio {ratio:.3f}; kept {int(ref['keep'].sum(1).min())} .. {int(ref['keep'].sum(1).max())}")
    assert ratio <= 1.0 and near <= S.NEAR_TIE_CAP * 64


def test_constructed_ties_are_all_kept(M):
    """Bit-equal logits at the 4th place (top_k = 4 keeps five columns) and at the nucleus boundary (a triple of equal logits with
    top_p set inside its mass: all three stay).  Over 64 tags every draw is the reference's, which draws the later duplicates."""
    near = picks = later = 0
    for A1, W, bias, twins, triple in F.tied_operands(BF16):
        Ad, Wd, bd = A1.cuda(), W.cuda(), bias.cuda()
        base = S.sample_ref(A1, W, bias, F.SEED, S.TAG0)
        x = base["x"][0]
        assert float(x[twins[0]]) == float(x[twins[1]]) and float(x[triple[0]]) == float(x[triple[2]])
        w = torch.exp(x - x.max())
        p_in = float((w[x > x[triple[0]]].sum() + 0.5 * w[triple[0]]) / w.sum())          # the boundary falls inside the triple
        for top_k, top_p, dup in ((4, 1.0, twins), (0, p_in, triple)):
            for tag in range(S.TAG0, S.TAG0 + 64):
                ref = F.filter_ref(A1, W, bias, F.SEED, tag, top_k, top_p, base=base)
                assert all(bool(ref["keep"][0, j]) for j in dup) and not bool(ref["keep"][0, int(torch.argsort(x)[0])])
                tok, lp = M.ops.gemm_sample_filtered(Ad, Wd, bd, F.SEED, tag, top_k=top_k, top_p=top_p)
                _, n, _ = _check(ref, tok, lp, f"ties k={top_k} p={top_p:.4f}")
                near, picks = near + n, picks + 1
                later += int(tok[0]) in dup[1:] and int(tok[0]) == int(ref["tok"][0])
    print(f"ties: {near} near-ties of {picks} picks; a later duplicate drawn {later} times")
    assert near <= S.NEAR_TIE_CAP * picks and later >= 20, (near, picks, later)


def test_row0_makes_chunks_draw_what_one_call_draws(M):
    A, W, bias, Ad, Wd, bd, _ = _case(64, BF16)
    t, l = M.ops.gemm_sample_filtered(Ad, Wd, bd, F.SEED, S.TAG0, top_k=50, top_p=0.9)
    t, l = t.clone(), l.clone()
    t2, l2 = M.ops.gemm_sample_filtered(Ad[32:], Wd, bd, F.SEED, S.TAG0, top_k=50, top_p=0.9, row0=32)
    assert torch.equal(t[32:], t2) and torch.equal(l[32:], l2)
    t3, _ = M.ops.gemm_sample_filtered(Ad[32:], Wd, bd, F.SEED, S.TAG0, top_k=50, top_p=0.9)
    assert not torch.equal(t[32:], t3)


def test_same_call_twice_is_bit_equal(M):
    _, _, _, Ad, Wd, bd, _ = _case(64, BF16)
    for top_k, top_p in F.FILTERS:
        a = [v.clone() for v in M.ops.gemm_sample_filtered(Ad, Wd, bd, F.SEED, S.TAG0 + 3, top_k=top_k, top_p=top_p)]
        b = M.ops.gemm_sample_filtered(Ad, Wd, bd, F.SEED, S.TAG0 + 3, top_k=top_k, top_p=top_p)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def _raw(M, step=False, rows=8, top_k=4, top_p=0.9, ldx=64, row0=0, null=None):
    """A direct C-ABI call (N = 64, K = 64, bf16) with NaN / -7 filled outputs and workspace; returns (rc, buffers)."""
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
    lp = torch.full((rows,), math.nan, device=dev)
    f = L.MvltSampleFilter()
    f.top_k, f.top_p, f.x, f.ldx, f.row0 = top_k, top_p, (None if null == "x" else ws.data_ptr()), ldx, row0
    fp = None if null == "filter" else C.byref(f)
    st = torch.cuda.current_stream().cuda_stream
    if not step:
        rc = L.lib().mvlt_gemm_sample_filtered(C.byref(p), pv.data_ptr(), pi.data_ptr(), fp, idx.data_ptr(), lp.data_ptr(), 1, 2, 1.0, st)
        torch.cuda.synchronize()
        return rc, (pv, pi, ws, idx, lp)
    ids = torch.full((rows, 4), -7, dtype=torch.int64, device=dev)
    scores = torch.full((rows, 4), math.nan, device=dev)
    new_ids = torch.full((rows, 2), -7, dtype=torch.int64, device=dev)
    col = torch.zeros(1, dtype=torch.int64, device=dev)
    ticket = torch.zeros(1, dtype=torch.int32, device=dev)
    seed = torch.zeros(1, dtype=torch.int64, device=dev)
    g = L.MvltSampleState()
    g.has_eos, g.col, g.ids, g.ld_ids, g.scores, g.ld_scores = 0, col.data_ptr(), ids.data_ptr(), 4, scores.data_ptr(), 4
    g.new_ids, g.ld_new, g.ticket, g.seed, g.tag0, g.inv_temperature = new_ids.data_ptr(), 2, ticket.data_ptr(), seed.data_ptr(), 5, 1.0
    if null == "seed":
        g.seed = None
    rc = L.lib().mvlt_gemm_sample_filtered_step(C.byref(p), pv.data_ptr(), pi.data_ptr(), fp, C.byref(g), st)
    torch.cuda.synchronize()
    return rc, (pv, pi, ws, ids, scores, new_ids, col, ticket)


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
    for step in (False, True):
        for kw in (dict(null="filter"), dict(null="x"), dict(ldx=63), dict(top_k=-1), dict(top_p=0.0), dict(top_p=-0.5),
                   dict(top_p=math.nan), dict(row0=2 ** 32 // 64 - 8 + 1), dict(rows=65)):
            rc, outs = _raw(M, step=step, **kw)
            assert rc == ARG, (step, kw, rc)
            _untouched(outs)
    rc, outs = _raw(M, step=True, null="seed")
    assert rc == ARG
    _untouched(outs)
    rc, outs = _raw(M, row0=2 ** 32 // 64 - 8 - 1)                     # the largest row0 that fits runs
    assert rc == 0 and bool(((outs[3] >= 0) & (outs[3] < 64)).all()) and bool(torch.isfinite(outs[4]).all())
    assert bool(torch.isfinite(outs[2]).all())                          # and the logits went through the workspace
    rc, outs = _raw(M, step=True)
    assert rc == 0 and int(outs[6]) == 1 and bool((outs[3][:, 0] >= 0).all()) and bool(torch.isfinite(outs[4][:, 0]).all())


# ------------------------------------------------------------------------------------------------ model level
def _images(n):
    return synth_batch(n, 24, seed=63, vocab=3000)[0]


@pytest.mark.parametrize("filt", [(8, 1.0), (0, 0.9)])
def test_filtered_graph_equals_eager(M, specs_hash, monkeypatch, filt):
    """Graph == eager token for token and score for score, without an eos and with one that cuts early."""
    model, _ = _tiny(M, specs_hash, F32)
    img = _images(3).cuda()
    kw = dict(sample_mode='sample', seed=77, top_k=filt[0], top_p=filt[1])
    outs = {}
    for graph in ("1", "0"):
        monkeypatch.setenv("MVLT_DECODE_GRAPH", graph)
        ids, sc = model(img, None, 1, 'unilm', **kw)
        assert ids.shape == (3, 8) and sc.shape == (24,)
        outs[graph] = (ids.cpu(), sc.cpu())
    assert torch.equal(outs["1"][0], outs["0"][0]) and rel_err(outs["1"][1], outs["0"][1]) < 1e-5, outs
    full = outs["1"][0]
    eos = int(full[0, 2])                                               # a token the first sample draws by step 2
    first = full[0].tolist().index(eos)
    model.config.eos_token_id = eos
    cut = {}
    for graph in ("1", "0"):
        monkeypatch.setenv("MVLT_DECODE_GRAPH", graph)
        ids, sc = model(img, None, 1, 'unilm', **kw)
        cut[graph] = (ids.cpu(), sc.cpu())
    assert torch.equal(cut["1"][0], cut["0"][0]) and cut["1"][1].shape == cut["0"][1].shape, cut
    assert cut["1"][1].numel() == 0 or rel_err(cut["1"][1], cut["0"][1]) < 1e-5
    assert torch.equal(cut["1"][0][0, :first + 1], full[0, :first + 1])
    assert bool((cut["1"][0][0, first + 1:] == model.config.pad_token_id).all())


def test_filtered_unfiltered_and_greedy_graphs_coexist(M, specs_hash, monkeypatch):
    monkeypatch.setenv("MVLT_DECODE_GRAPH", "1")
    model, _ = _tiny(M, specs_hash, F32)
    img = _images(3).cuda()
    calls = [dict(sample_mode='sample', seed=5, top_k=8), dict(sample_mode='sample', seed=5), dict(),
             dict(sample_mode='sample', seed=5, top_p=0.9), dict(sample_mode='sample', seed=5, top_k=1)]
    first = [tuple(v.cpu() for v in model(img, None, 1, 'unilm', **kw)) for kw in calls]
    again = [tuple(v.cpu() for v in model(img, None, 1, 'unilm', **kw)) for kw in reversed(calls)][::-1]
    for a, b in zip(first, again):
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert not torch.equal(first[0][0], first[1][0]) and not torch.equal(first[3][0], first[1][0])     # the key includes the filter
    assert torch.equal(first[4][0], first[2][0])                        # top_k = 1 is the greedy sequence
    assert float(first[4][1].abs().max()) < 1e-5                        # ... with log-probability 0 under the one-token law
    for bad in (dict(top_k=8), dict(top_p=0.9), dict(sample_mode='sample', top_k=-1), dict(sample_mode='sample', top_p=0.0),
                dict(sample_mode='sample', top_p=math.nan)):
        with pytest.raises(ValueError):
            model(img, None, 1, 'unilm', **bad)


@pytest.mark.parametrize("filt", [(8, 1.0), (0, 0.9)])
def test_filtered_decode_teacher_forced_against_the_oracle(M, specs_hash, monkeypatch, filt):
    """Every pick of the graph loop against the CPU oracle's logits on the generated prefix with the host noise, by the pick rule;
    e_x = 1e-4 x (top - mean logit), so that SAFETY e_x is the f32 activation tolerance of test_sample_gpu.py."""
    monkeypatch.setenv("MVLT_DECODE_GRAPH", "1")
    model, sd = _tiny(M, specs_hash, F32)
    image = _images(3)
    ids, sc = model(image.cuda(), None, 1, 'unilm', sample_mode='sample', seed=77, top_k=filt[0], top_p=filt[1])
    ids, sc = ids.cpu(), sc.cpu().view(8, 3).t()
    O, scfg, bcfg = _tiny_oracle_cfgs()
    exact = near = 0
    with torch.no_grad():
        feat = O.conv_layer(image, sd, scfg)
        for t in range(8):
            inp = torch.cat([ids[:, :t], torch.full((3, 1), bcfg.mask_token_id)], 1)
            o = O.mvlbert_forward(sd, bcfg, inp, feat, True)
            x = O.mlm_head(o["hidden"][:, -1], sd, "MLM_head_seq2seq", bcfg).double()
            e_x = (1e-4 * (x.max(-1).values - x.mean(-1)))[:, None].expand_as(x)
            g = S.gumbel_ref(S.u01_ref(77, S.TAG0 + t, 3, x.shape[1]))
            y = x + g
            tp = F.p32(filt[1])
            keep = torch.stack([F.kept_ref(x[b], filt[0], tp) for b in range(3)])
            io = [F.membership(x[b], e_x[b], filt[0], tp) for b in range(3)]
            ref = dict(x=x, e_x=e_x, y=y, bound_y=S.SAFETY * (e_x + S.e_g(g) + 2.0 ** -24 * y.abs()), keep=keep,
                       IN=torch.stack([a for a, _ in io]), OUT=torch.stack([b for _, b in io]),
                       tok=torch.where(keep, y, torch.full_like(y, -math.inf)).argmax(1),
                       bound_lp=lambda tt: S.SAFETY * (2.0 * e_x[:, 0] + 1e-5))
            e, n, _ = _check(ref, ids[:, t], sc[:, t], f"step {t} {filt}")
            exact, near = exact + e, near + n
    print(f"{filt}: {exact} exact, {near} near-ties of 24 picks")
    assert near <= S.NEAR_TIE_CAP * 24


def test_batch_of_70_runs_in_row_chunks_without_multinomial(M, specs_hash, monkeypatch):
    model, _ = _tiny(M, specs_hash, F32)
    img = _images(70).cuda()

    def boom(*a, **k):
        raise AssertionError("torch.multinomial on the filtered route")
    monkeypatch.setattr(torch, "multinomial", boom)
    kw = dict(sample_mode='sample', seed=9, top_k=8, top_p=0.9)
    ids70, sc70 = model(img, None, 1, 'unilm', **kw)
    ids64, sc64 = model(img[:64].contiguous(), None, 1, 'unilm', **kw)
    assert ids70.shape == (70, 8) and torch.equal(ids70[:64], ids64)
    assert torch.allclose(sc70.view(8, 70)[:, :64], sc64.view(8, 64), rtol=0, atol=1e-5)


def test_first_token_frequencies_follow_the_renormalised_softmax(M):
    """One row of 24 logits, top_k = 5, 4096 tags: chi-square (4 degrees of freedom, significance 1e-4) against the renormalised
    softmax over K_ref, and no draw outside it (the kept set is decided: the fifth and sixth logits are far apart).  The logits
    are handed over exactly: A = e_0, W[:, 0] = the f32 logits, no bias."""
    logits, keep, p = F.frequency_case()
    l32 = logits.float()
    srt = torch.sort(l32, descending=True).values
    assert float(srt[4] - srt[5]) > 1e-3
    keep32 = F.kept_ref(l32.double(), 5, 1.0)
    p32 = torch.softmax(torch.where(keep32, l32.double(), torch.full_like(logits, -math.inf)), 0)
    A = torch.zeros(1, 16)
    A[0, 0] = 1.0
    W = torch.zeros(24, 16)
    W[:, 0] = l32
    Ad, Wd = A.cuda(), W.cuda()
    toks = [M.ops.gemm_sample_filtered(Ad, Wd, None, 99, S.TAG0 + s, top_k=5)[0] for s in range(4096)]
    toks = torch.cat(toks).cpu().tolist()
    assert all(bool(keep32[t]) for t in toks)
    chi2 = F.chi_square(toks, keep32, p32, 4096)
    print(f"chi-square over the 5 kept cells, 4096 device draws: {chi2:.2f} (critical {F.CHI2_CRIT_4DF})")
    assert chi2 < F.CHI2_CRIT_4DF
