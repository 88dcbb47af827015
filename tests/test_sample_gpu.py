"""Sampled decoding on the GPU: the fused Gumbel-max MLM head (mvlt_gemm_sample / mvlt_gemm_sample_step, mvlt_gumbel_noise) against
the float64 host reference of tests/sample_ref.py, token by token, and the sampled graph / eager decode loops against the oracle.

Every pick must be the reference's token or a near-tie (the reference's y at the device's token within the sum of the two
elements' bounds of the reference's maximum), and at most 2 % of a test's picks may be near-ties."""
import ctypes as C
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sample_ref as S  # noqa: E402
from conftest import rel_err, synth_batch  # noqa: E402
from gemm_ref import check_bound  # noqa: E402
from tiny_caption import tiny_caption as _tiny  # noqa: E402

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
V, VPAD, K = 30522, 30528, 768
SEED = 0x9E3779B97F4A7C15


@pytest.fixture(scope="module")
def M():
    import mvlt_amd
    return mvlt_amd


def _operands(rows, dtype, seed):
    """A ~ N(0, 1) in the storage the graph path hands over (row stride 2 K: the [MASK] rows of a [B, 2, K] buffer), W ~ N(0, 9 / K)
    (logit std 3) with the rows beyond the vocabulary holding NaN, bias ~ N(0, 0.01)."""
    gen = torch.Generator().manual_seed(seed)
    full = torch.randn(rows, 2, K, generator=gen).to(dtype)
    W = torch.full((VPAD, K), math.nan).to(dtype)
    W[:V] = (torch.randn(V, K, generator=gen) * (3.0 / math.sqrt(K))).to(dtype)
    bias = torch.randn(V, generator=gen) * 0.1
    fd = full.cuda()
    return full[:, 1], W, bias, fd[:, 1], W.cuda()[:V], bias.cuda()


def test_gumbel_noise_equals_the_host_noise(M):
    """mvlt_gumbel_noise against -log(-log(u01)) in float64 within e_g at every element of a 64 x 30522 draw, two steps and two
    seeds: pins the index m N + n, the tag and the 24-bit u01 construction on the device."""
    worst = 0.0
    for seed in (SEED, 12345):
        for tag in (S.TAG0, S.TAG0 + 7):
            got = M.ops.gumbel_noise(seed, tag, 64, V, torch.device("cuda")).cpu().double()
            g = S.gumbel_ref(S.u01_ref(seed, tag, 64, V))
            bound = S.e_g(g)
            worst = max(worst, float(((got - g).abs() / bound).max()))
            check_bound(got, g, bound, f"gumbel noise seed {seed:#x} tag {tag:#x}")
    print(f"device noise: worst |g - g_ref| / e_g = {worst:.3f}")


@pytest.mark.parametrize("dtype", [BF16, F32])
def test_sampled_pick_against_host_reference(M, dtype):
    """M in {1, 17, 32, 64} x 2 steps (and 8 steps x 64 rows): token = the reference's or a near-tie (<= 2 % of the picks),
    logprob within its bound."""
    ops = M.ops
    cases = [(m, S.TAG0 + s) for m in (1, 17, 32, 64) for s in (0, 1)] + [(64, S.TAG0 + s) for s in range(2, 8)]
    exact = near = total = 0
    worst_lp = 0.0
    for i, (rows, tag) in enumerate(cases):
        A, W, bias, Ad, Wd, bd = _operands(rows, dtype, 100 + rows)
        assert Ad.stride(0) == 2 * K
        ref = S.sample_ref(A, W[:V], bias, SEED, tag)
        tok, lp = ops.gemm_sample(Ad, Wd, bd, SEED, tag)
        torch.cuda.synchronize()
        tok, lp = tok.cpu(), lp.cpu()
        e, n, bad = S.classify_picks(tok, ref["y"], ref["bound_y"])
        assert not bad, (rows, tag, bad[:4])
        exact, near, total = exact + e, near + n, total + rows
        ok = (tok >= 0) & (tok < V)
        assert bool(ok.all())
        ref_lp = ref["x"].gather(1, tok.view(-1, 1)).squeeze(1) - ref["lse"]
        b = ref["bound_lp"](tok)
        worst_lp = max(worst_lp, float(((lp.double() - ref_lp).abs() / b).max()))
        check_bound(lp.view(-1, 1), ref_lp.view(-1, 1), b.view(-1, 1), f"logprob M={rows} tag={tag:#x}")
    print(f"{dtype}: {exact} exact, {near} near-ties of {total} picks; worst logprob ratio {worst_lp:.3f}")
    assert near <= S.NEAR_TIE_CAP * total, f"{near} near-ties of {total} picks ({exact} exact): more than 2 %"


@pytest.mark.parametrize("T", [0.5, 2.0])
def test_temperature_follows_the_reference(M, T):
    A, W, bias, Ad, Wd, bd = _operands(64, BF16, 7)
    ref = S.sample_ref(A, W[:V], bias, SEED, S.TAG0 + 1, T)
    tok, lp = M.ops.gemm_sample(Ad, Wd, bd, SEED, S.TAG0 + 1, temperature=T)
    tok, lp = tok.cpu(), lp.cpu()
    S.assert_picks(tok, ref["y"], ref["bound_y"], f"T={T}")
    ref_lp = ref["x"].gather(1, tok.view(-1, 1)).squeeze(1) - ref["lse"]
    check_bound(lp.view(-1, 1), ref_lp.view(-1, 1), ref["bound_lp"](tok).view(-1, 1), f"logprob T={T}")


def test_seed_and_tag_select_the_draw(M):
    _, _, _, Ad, Wd, bd = _operands(64, BF16, 8)
    ops = M.ops
    t0, l0 = ops.gemm_sample(Ad, Wd, bd, SEED, S.TAG0)
    t1, l1 = ops.gemm_sample(Ad, Wd, bd, SEED, S.TAG0)
    assert torch.equal(t0, t1) and torch.equal(l0, l1)                 # the same draw, bit for bit
    for seed, tag in ((SEED + 1, S.TAG0), (SEED, S.TAG0 + 1), (SEED ^ (1 << 40), S.TAG0)):
        t2, _ = ops.gemm_sample(Ad, Wd, bd, seed, tag)
        changed = int((t2 != t0).sum())
        assert changed > 32, (seed, tag, changed)


def _raw_sample(M, rows, Kk, dtype=BF16, step=False, null=None, lda=None):
    """A direct C-ABI call with NaN-filled outputs; returns (rc, outputs)."""
    L = M._lib
    dev = torch.device("cuda")
    A = torch.zeros((rows, 2 * Kk), dtype=dtype, device=dev)[:, :Kk]
    W = torch.zeros((64, Kk), dtype=dtype, device=dev)
    p = L.MvltGemm()
    p.dtype, p.M, p.N, p.K = (1 if dtype == BF16 else 0), rows, 64, Kk
    p.A, p.lda, p.B, p.ldb = A.data_ptr(), (lda or Kk), W.data_ptr(), Kk
    pv = torch.full((4, rows, 4), math.nan, device=dev)
    pi = torch.full((rows, 4), -7, dtype=torch.int32, device=dev)
    idx = torch.full((rows,), -7, dtype=torch.int64, device=dev)
    lp = torch.full((rows,), math.nan, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    if not step:
        rc = L.lib().mvlt_gemm_sample(C.byref(p), pv.data_ptr(), pi.data_ptr(), None if null == "out" else idx.data_ptr(), lp.data_ptr(),
                                      1, 2, 1.0, st)
        torch.cuda.synchronize()
        return rc, (pv, pi, idx, lp)
    ids = torch.full((rows, 4), -7, dtype=torch.int64, device=dev)
    scores = torch.full((rows, 4), math.nan, device=dev)
    new_ids = torch.full((rows, 2), -7, dtype=torch.int64, device=dev)
    col = torch.zeros(1, dtype=torch.int64, device=dev)
    ticket = torch.zeros(1, dtype=torch.int32, device=dev)
    seed = torch.zeros(1, dtype=torch.int64, device=dev)
    g = L.MvltSampleState()
    g.has_eos, g.col, g.ids, g.ld_ids, g.scores, g.ld_scores = 0, col.data_ptr(), ids.data_ptr(), 4, scores.data_ptr(), 4
    g.new_ids, g.ld_new, g.ticket, g.seed, g.tag0, g.inv_temperature = new_ids.data_ptr(), 2, ticket.data_ptr(), seed.data_ptr(), 5, 1.0
    if null is not None:
        setattr(g, null, None)
    rc = L.lib().mvlt_gemm_sample_step(C.byref(p), pv.data_ptr(), pi.data_ptr(), C.byref(g), st)
    torch.cuda.synchronize()
    return rc, (pv, pi, ids, scores, new_ids, col, ticket)


def _untouched(outs):
    for t in outs:
        if t.dtype.is_floating_point:
            assert bool(torch.isnan(t).all())
        elif t.numel() > 1:
            assert bool((t == -7).all())
        else:
            assert int(t) == 0


def test_refusals_write_nothing(M):
    """M > 64 and null pointers: MVLT_ERR_ARG; a K that is not a whole number of k-blocks or an unaligned row stride:
    MVLT_ERR_UNSUPPORTED -- as mvlt_gemm_argmax_greedy documents them -- and no output is written."""
    ARG, UNSUP = -1, -3
    for step in (False, True):
        rc, outs = _raw_sample(M, 65, 64, step=step)
        assert rc == ARG
        _untouched(outs)
        for dtype, kk in ((BF16, 48), (F32, 24)):
            rc, outs = _raw_sample(M, 8, kk, dtype=dtype, step=step)
            assert rc == UNSUP, (dtype, kk, rc)
            _untouched(outs)
        rc, outs = _raw_sample(M, 8, 64, step=step, lda=68)
        assert rc == UNSUP
        _untouched(outs)
    rc, outs = _raw_sample(M, 8, 64, null="out")
    assert rc == ARG
    _untouched(outs)
    for field in ("seed", "col", "ticket", "ids", "scores", "new_ids"):
        rc, outs = _raw_sample(M, 8, 64, step=True, null=field)
        assert rc == ARG, field
        _untouched(outs)
    rc, outs = _raw_sample(M, 8, 64, step=True)                       # and the same call with nothing missing runs
    assert rc == 0 and int(outs[5]) == 1 and bool((outs[2][:, 0] >= 0).all()) and bool(torch.isfinite(outs[3][:, 0]).all())


# ------------------------------------------------------------------------------------------------ model level
def _tiny_oracle_cfgs():
    from oracle import mvlt_oracle as O
    scfg = O.SwinCfg(embed_dim=32, depths=(2, 2, 2, 2), num_heads=(1, 2, 4, 8), drop_path_rate=0.2)
    bcfg = O.BertCfg(vocab_size=3000, hidden_size=256, num_hidden_layers=2, num_attention_heads=4, intermediate_size=1024)
    return O, scfg, bcfg


def _teacher_forced_sampled(O, sd, scfg, bcfg, image, ids, seed, temperature=1.0, tol=None, eos=None):
    """For every sample and step the oracle's full-sequence recompute on the GENERATED prefix gives the logits; the host noise
    of (seed, TAG0 + step, row) is added; the device's token must be that argmax or a near-tie.  The near-tie margin is
    `tol` x (top - mean logit) (the bf16 greedy margin, applied to y) or, tol = None (f32), the f32 bound of a logit that went
    through the network: 2e-4 relative to the logits' spread (the f32 activation tolerance of the model tests).
    Returns (exact, near, bad, logp [B, n] of the device's tokens under the oracle)."""
    feat = O.conv_layer(image, sd, scfg)
    B, n = ids.shape
    Vv = bcfg.vocab_size
    it = S.inv_t_f32(temperature)
    exact = near = 0
    bad, logp = [], torch.zeros(B, n, dtype=torch.float64)
    alive = torch.ones(B, dtype=torch.bool)
    for t in range(n):
        inp = torch.cat([ids[:, :t], torch.full((B, 1), bcfg.mask_token_id)], 1)
        o = O.mvlbert_forward(sd, bcfg, inp, feat, True)
        x = O.mlm_head(o["hidden"][:, -1], sd, "MLM_head_seq2seq", bcfg).double() * it
        y = x + S.gumbel_ref(S.u01_ref(seed, S.TAG0 + t, B, Vv))
        logp[:, t] = torch.log_softmax(x, -1).gather(1, ids[:, t:t + 1].clamp(0, Vv - 1)).squeeze(1)
        spread = x.max(-1).values - x.mean(-1)
        for b in range(B):
            if not alive[b]:
                continue                        # finished samples emit PAD: nothing to pin
            m = float(y[b].max() - y[b, ids[b, t]])
            if m == 0.0:
                exact += 1
            elif m <= (tol if tol is not None else 2e-4) * float(spread[b]):
                near += 1
            else:
                bad.append((b, t, m, float(spread[b])))
        if eos is not None:
            alive &= ids[:, t] != eos
    return exact, near, bad, logp


def test_sampled_graph_equals_eager_and_oracle_f32(M, specs_hash, monkeypatch):
    model, sd = _tiny(M, specs_hash, F32)
    image, _, _, _ = synth_batch(3, 24, seed=63, vocab=3000)
    outs = {}
    for graph in ("1", "0"):
        monkeypatch.setenv("MVLT_DECODE_GRAPH", graph)
        ids, sc = model(image.cuda(), None, 1, 'unilm', sample_mode='sample', seed=77)
        assert ids.shape == (3, 8) and sc.shape == (3 * 8,)
        outs[graph] = (ids.cpu(), sc.cpu())
    assert torch.equal(outs["1"][0], outs["0"][0]), outs
    assert rel_err(outs["1"][1], outs["0"][1]) < 1e-5
    O, scfg, bcfg = _tiny_oracle_cfgs()
    ids, sc = outs["1"]
    with torch.no_grad():
        exact, near, bad, logp = _teacher_forced_sampled(O, sd, scfg, bcfg, image, ids, 77)
    msg = f"{exact} exact, {near} near-ties, wrong {bad} of {ids.numel()} picks"
    assert not bad and near <= S.NEAR_TIE_CAP * ids.numel(), msg
    assert rel_err(sc.view(8, 3).t(), logp) < 1e-4                     # scores are concatenated step after step
    greedy, _ = model(image.cuda(), None, 1, 'unilm')
    assert not torch.equal(greedy.cpu(), ids)                           # and it is not the greedy sequence


def test_sampled_early_stop_is_cut_like_the_eager_loop(M, specs_hash, monkeypatch):
    """An eos the sampling reaches: ids are cut after the step at which the last sample finished (n_out columns, n_out - 1
    score steps), finished rows emit PAD, and the graph loop agrees with the eager loop."""
    monkeypatch.setenv("MVLT_DECODE_GRAPH", "0")
    model, _ = _tiny(M, specs_hash, F32, max_length=20)
    image, _, _, _ = synth_batch(2, 24, seed=63, vocab=3000)
    pad = model.config.pad_token_id
    # a seed and a token that both samples draw, at different steps: that token becomes the eos (at most 64 short decodes)
    eos = seed = None
    for cand_seed in range(64):
        full, _ = model(image.cuda(), None, 1, 'unilm', sample_mode='sample', seed=cand_seed)
        full = full.cpu()
        assert full.shape == (2, 20)
        r0, r1 = full[0, :19].tolist(), full[1, :19].tolist()
        for c in r0:
            if c != pad and c in r1 and r0.index(c) != r1.index(c):
                eos, seed = c, cand_seed
                break
        if eos is not None:
            break
    assert eos is not None, "no seed in 0..63 lets both samples draw a common token"
    first = [full[b].tolist().index(eos) for b in range(2)]
    stop = max(first) + 1
    model.config.eos_token_id = eos
    outs = {}
    for graph in ("0", "1"):
        monkeypatch.setenv("MVLT_DECODE_GRAPH", graph)
        ids, sc = model(image.cuda(), None, 1, 'unilm', sample_mode='sample', seed=seed)
        outs[graph] = (ids.cpu(), sc.cpu())
    ids, sc = outs["0"]
    assert ids.shape == (2, stop) and sc.numel() == 2 * (stop - 1), (ids.shape, sc.numel(), first)
    for b in range(2):
        assert torch.equal(ids[b, :first[b] + 1], full[b, :first[b] + 1])
        assert bool((ids[b, first[b] + 1:] == pad).all())
    assert torch.equal(outs["1"][0], ids) and outs["1"][1].shape == sc.shape and rel_err(outs["1"][1], sc) < 1e-5
    gg = model.__dict__["_mvlt_sample_graph"]
    assert gg.unfinished.tolist() == [0, 0]
    alive = gg.alive[:stop].tolist()
    assert alive[:stop - 1] == [1] * (stop - 1) and alive[stop - 1] == 0


def test_default_seed_follows_torch_and_graphs_coexist(M, specs_hash, monkeypatch):
    from mvlt_amd import decode
    monkeypatch.setenv("MVLT_DECODE_GRAPH", "1")
    model, _ = _tiny(M, specs_hash, F32)
    fresh, _ = _tiny(M, specs_hash, F32)
    image, _, _, _ = synth_batch(3, 24, seed=63, vocab=3000)
    img = image.cuda()
    captures = []
    orig = decode._GreedyGraph.capture
    monkeypatch.setattr(decode._GreedyGraph, "capture", lambda self: (captures.append(self.mode), orig(self))[1])
    torch.manual_seed(11)
    a, sa = model(img, None, 1, 'unilm', sample_mode='sample')
    g, _ = model(img, None, 1, 'unilm')
    torch.manual_seed(11)
    b, sb = model(img, None, 1, 'unilm', sample_mode='sample')
    torch.manual_seed(12)
    c, _ = model(img, None, 1, 'unilm', sample_mode='sample')
    assert torch.equal(a, b) and torch.equal(sa, sb)
    assert not torch.equal(a, c)
    assert captures == ["sample", "greedy"], captures                   # neither graph recaptured the other
    g2, _ = model(img, None, 1, 'unilm')
    assert captures == ["sample", "greedy"]
    ref, _ = fresh(img, None, 1, 'unilm')
    assert torch.equal(g, ref) and torch.equal(g2, ref)
    e, _ = model(img, None, 1, 'unilm', sample_mode='sample', seed=3)   # an explicit seed leaves torch's generator alone
    state = torch.get_rng_state()
    f, _ = model(img, None, 1, 'unilm', sample_mode='sample', seed=3)
    assert torch.equal(e, f) and torch.equal(state, torch.get_rng_state())


def test_first_step_frequencies_follow_the_softmax(M, specs_hash, monkeypatch):
    """512 draws of the first token (16 calls of B = 32 with seeds 0..15 on copies of one image) against softmax(logits), with the
    4-sigma criterion of test_model_gpu.py::test_sample_mode_decoding."""
    monkeypatch.setenv("MVLT_DECODE_GRAPH", "1")
    model, _ = _tiny(M, specs_hash, F32, max_length=2)
    image, _, _, _ = synth_batch(1, 24, seed=63, vocab=3000)
    img = image.cuda().expand(32, -1, -1, -1).contiguous()
    first = torch.cat([model(img, None, 1, 'unilm', sample_mode='sample', seed=s)[0][:, 0].cpu() for s in range(16)])
    with torch.no_grad():
        feat = model.conv(img[:1])
        mask = torch.full((1, 1), 103, device="cuda")
        out0, _ = model.MVLBert(mask, None, feat, None, use_cache=True, seq2seq_mask=True)
        logits = model.MLM_head_seq2seq(out0.last_hidden_state[:, -1:])[0, 0].float()
    p = torch.softmax(logits, -1).cpu()
    top = torch.topk(p, 5).indices
    freq = torch.stack([(first == t).float().mean() for t in top])
    assert bool(((freq - p[top]).abs() < 4 * (p[top] * (1 - p[top]) / 512).sqrt() + 1e-3).all()), (freq, p[top])


def test_sampled_decode_config4_full_size_bf16(M, monkeypatch):
    """Config #4 shapes (Swin-S + BERT-base, B = 32, bf16), 16 sampled steps on the graph path: every pick teacher-forced against
    the f32 oracle with host noise, margin = the bf16 greedy margin (2 % of top minus mean logit) applied to y.  Near-tie cap:
    2 % plus the share of near-ties that greedy bf16 decoding of the same model and images shows under the existing full-size test's
    own check (_teacher_forced_picks_ok of test_model_gpu.py, run here; both counts go into the assertion message)."""
    from oracle import mvlt_oracle as O
    monkeypatch.setenv("MVLT_DECODE_GRAPH", "1")
    cfg = M.MVLBertConfigForImageCaption()
    cfg.max_length = 16
    cfg.eos_token_id = None
    tok = type("Tok", (), {"mask_token_id": 103, "sep_token_id": 102})()
    torch.manual_seed(1)
    model = M.MVLBertForImageCaption(cfg, tokenizer=tok)
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    model = M.set_compute_dtype(model.cuda().eval(), BF16)
    image = torch.randn(32, 3, 224, 224, generator=torch.Generator().manual_seed(2))
    ids, sc = model(image.cuda(), None, 1, 'unilm', sample_mode='sample', seed=2024)
    ids2, sc2 = model(image.cuda(), None, 1, 'unilm', sample_mode='sample', seed=2024)
    assert ids.shape == (32, 16) and torch.equal(ids, ids2) and torch.equal(sc, sc2)
    NS = 8                                        # samples pinned to the CPU oracle (the recompute is quadratic on the CPU)
    with torch.no_grad():
        exact, near, bad, logp = _teacher_forced_sampled(O, sd, O.SwinCfg(), O.BertCfg(eos_token_id=-1), image[:NS], ids.cpu()[:NS],
                                                         2024, tol=0.02)
    # the greedy bf16 share, measured here on the same model, images and box with the existing test's own helper
    from test_model_gpu import _teacher_forced_picks_ok
    gids, _ = model(image.cuda(), None, 1, 'unilm')
    with torch.no_grad():
        g_exact, greedy_near, g_bad = _teacher_forced_picks_ok(O, sd, O.SwinCfg(), O.BertCfg(eos_token_id=-1), image[:NS], gids.cpu()[:NS])
    greedy_total = NS * 16
    assert not g_bad, g_bad
    cap = (S.NEAR_TIE_CAP + greedy_near / greedy_total) * NS * 16
    msg = (f"{exact} exact, {near} near-ties, {len(bad)} wrong of {NS * 16} picks; cap {cap:.1f} = 2 % + greedy bf16 "
           f"{greedy_near} / {greedy_total}; wrong: {bad[:4]}")
    print(msg)
    assert not bad and near <= cap, msg
    # NOTE the noise row of sample b is b of the WHOLE batch (index m N + n): the first NS rows are rows 0 .. NS - 1 either way
    got = sc.cpu().view(16, 32).t()[:NS].double()
    assert float((got - logp).abs().max()) < 0.15, float((got - logp).abs().max())      # bf16 logits: loose, the picks are the check
