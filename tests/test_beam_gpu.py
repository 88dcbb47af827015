"""Beam search on the fused route: the candidate head (mvlt_gemm_beam_candidates) against the float64 reference and rules of
tests/beam_ref.py, the table-driven cached attention (mvlt_attn_cached_beam) bit for bit against mvlt_attn_cached on a densely
gathered cache, and decode.beam_search against the oracle's full recompute and against the MVLT_BEAM_FUSED=0 route."""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beam_ref as R  # noqa: E402
from conftest import synth_batch  # noqa: E402
from test_model_gpu import _tiny_caption, _tiny_oracle_cfgs  # noqa: E402
from test_sample_gpu import _tiny  # noqa: E402

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
ERR_ARG, ERR_UNSUPPORTED = -1, -3


@pytest.fixture(scope="module")
def M():
    import mvlt_amd
    return mvlt_amd


def _split(out):
    """(beam, tok, score) of the [3, G, n] int32 buffer of ops.gemm_beam_candidates."""
    return out[1], out[2], out[0].view(torch.float32)


# ------------------------------------------------------------------------------------------------ candidates
@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("G,nb", R.CASES)
def test_candidates_against_host_reference(M, G, nb, dtype):
    A, W, bias, bs = R.case_operands(G, nb, dtype)
    ref = R.beam_ref(A, W, bias, bs, nb, 2 * nb)
    out, lse = M.ops.gemm_beam_candidates(A.cuda(), W.cuda(), bias.cuda(), bs.cuda(), nb, 2 * nb, want_lse=True)
    _, _, worst = R.assert_lists(ref, *_split(out), f"G={G} beams={nb} {dtype}")
    assert worst <= 1.0
    assert float(((lse.cpu().double() - ref["lse"]).abs() / ref["bound_s"].min(1).values).max()) <= 1.0
    out2, _ = M.ops.gemm_beam_candidates(A.cuda(), W.cuda(), bias.cuda(), bs.cuda(), nb, 2 * nb)
    assert torch.equal(out, out2)          # the same call twice: the same lists and scores, bit for bit


def test_candidates_at_the_real_size(M):
    """M = 40 rows (20 samples x 2 beams), N = 30522, K = 768, bf16."""
    A, W, bias, bs = R.case_operands(0, 0, BF16, big=True)
    nb = R.BIG["num_beams"]
    ref = R.beam_ref(A, W, bias, bs, nb, 2 * nb)
    out, _ = M.ops.gemm_beam_candidates(A.cuda(), W.cuda(), bias.cuda(), bs.cuda(), nb, 2 * nb)
    _, _, worst = R.assert_lists(ref, *_split(out), "real size")
    assert worst <= 1.0


def test_constructed_ties_come_back_in_flat_index_order(M):
    # (1) duplicate weight rows: bit-equal logits in every row.  The best token of sample 0 gets a twin at a LOWER and one at a
    # HIGHER index; the three entries of beam 0 must lead the list in index order with bit-equal scores
    G, nb, n = 2, 2, 4
    A, W, bias, bs = R.case_operands(3, 2, BF16)
    A, bs = A[:G * nb].clone(), bs[:G * nb].clone()
    bs[1] = -3.0                                             # (sample 0's second beam: an ordinary score here)
    ref0 = R.beam_ref(A, W, bias, bs, nb, n)
    t = int(ref0["flat"][0, 0]) % ref0["N"]
    assert int(ref0["flat"][0, 0]) // ref0["N"] == 0 and 7 < t < ref0["N"] - 8
    W0, bias0 = W, bias
    W, bias = W.clone(), bias.clone()
    for j in (t - 7, t + 8):
        W[j], bias[j] = W[t], bias[t]
    out, _ = M.ops.gemm_beam_candidates(A.cuda(), W.cuda(), bias.cuda(), bs.cuda(), nb, n)
    beam, tok, score = (v.cpu() for v in _split(out))
    assert beam[0, :3].tolist() == [0, 0, 0] and tok[0, :3].tolist() == [t - 7, t, t + 8], (beam[0], tok[0])
    assert score[0, 0] == score[0, 1] == score[0, 2]
    ref = R.beam_ref(A, W, bias, bs, nb, n)
    assert torch.equal(beam.long() * ref["N"] + tok.long(), ref["flat"])
    # (2) two identical beam rows with equal beam scores: every entry has a twin in the other beam; beam 0 comes first each time
    A2 = A[:2].clone()
    A2[1] = A2[0]
    bs2 = torch.tensor([-1.5, -1.5])
    out, _ = M.ops.gemm_beam_candidates(A2.cuda(), W0.cuda(), bias0.cuda(), bs2.cuda(), 2, 8)
    beam, tok, score = (v.cpu() for v in _split(out))
    ref = R.beam_ref(A2, W0, bias0, bs2, 2, 8)
    assert torch.equal(beam.long() * ref["N"] + tok.long(), ref["flat"]), (beam, tok, ref["flat"])
    assert beam[0].tolist() == [0, 1] * 4 and torch.equal(tok[0, 0::2], tok[0, 1::2]) and torch.equal(score[0, 0::2], score[0, 1::2])
    # (3) every score of the sample equal (zero activations, constant bias): the first n flat indices, in order -- more ties than
    # the kernel's candidate list holds, so this is its round-by-round form
    Z = torch.zeros(2, A.shape[1], dtype=BF16)
    out, _ = M.ops.gemm_beam_candidates(Z.cuda(), W.cuda(), torch.zeros_like(bias).cuda(), bs2.cuda(), 2, 16)
    beam, tok, score = (v.cpu() for v in _split(out))
    assert beam[0].tolist() == [0] * 16 and tok[0].tolist() == list(range(16)) and bool((score[0] == score[0, 0]).all())


def test_candidate_refusals_launch_nothing(M):
    from mvlt_amd import _lib as L
    G, nb, n = 3, 2, 4
    A, W, bias, bs = (v.cuda() for v in R.case_operands(G, nb, BF16))
    N = W.shape[0]
    ldx = (N + 3) // 4 * 4
    A9 = torch.cat([A, A[:3]])          # 9 rows: a multiple of 9 beams
    cases = [
        ("beam_scores NULL", dict(beam_scores=None), A, ERR_ARG),
        ("x NULL", dict(x=None), A, ERR_ARG),
        ("cand_tok NULL", dict(cand_tok=None), A, ERR_ARG),
        ("num_beams 0", dict(num_beams=0), A, ERR_ARG),
        ("n_cand 0", dict(n_cand=0), A, ERR_ARG),
        ("M % num_beams", dict(num_beams=4), A, ERR_ARG),
        ("ldx < N", dict(ldx=N - 1), A, ERR_ARG),
        ("num_beams 9", dict(num_beams=9), A9, ERR_UNSUPPORTED),
        ("n_cand 17", dict(n_cand=17), A, ERR_UNSUPPORTED),
        ("k-major operand", dict(a_kmajor=1), A, ERR_UNSUPPORTED),
        ("K not a whole number of k-blocks", dict(K=A.shape[1] - 1), A, ERR_UNSUPPORTED),
    ]
    for what, change, Ad, code in cases:
        rows = Ad.shape[0]
        ws = torch.full((rows, ldx), float("nan"), device="cuda")
        score = torch.full((rows, 17), float("nan"), device="cuda")
        cb = torch.full((rows, 17), -7, dtype=torch.int32, device="cuda")
        ct = torch.full((rows, 17), -7, dtype=torch.int32, device="cuda")
        lse = torch.full((rows,), float("nan"), device="cuda")
        bsr = torch.zeros(rows, device="cuda")
        p, _, _ = M.ops._head_gemm(Ad, W, bias)
        c = L.MvltBeamCand()
        ptr = dict(beam_scores=bsr, x=ws, cand_score=score, cand_beam=cb, cand_tok=ct, lse=lse)
        for k, v in ptr.items():
            setattr(c, k, v.data_ptr())
        c.num_beams, c.n_cand, c.ldx = nb, n, ldx
        for k, v in change.items():
            if k in ("a_kmajor", "K"):
                setattr(p, k, v)
            else:
                setattr(c, k, v.data_ptr() if torch.is_tensor(v) else v)
        rc = L.lib().mvlt_gemm_beam_candidates(C.byref(p), C.byref(c), None)
        torch.cuda.synchronize()
        assert rc == code, (what, rc)
        assert bool(torch.isnan(ws).all()) and bool(torch.isnan(score).all()) and bool(torch.isnan(lse).all()), what
        assert bool((cb == -7).all()) and bool((ct == -7).all()), what


# ------------------------------------------------------------------------------------------------ attention
G_, NB_, NH_, HD_, PREFIX_, NNEW_, CAP_ = 2, 3, 2, 64, 5, 2, 208
ROWS_ = G_ * NB_


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


def _attn_inputs(dtype, past, seed):
    gen = torch.Generator().manual_seed(seed)
    qkv = torch.randn(ROWS_ * NNEW_, 3 * NH_ * HD_, generator=gen).to(dtype).cuda()
    k = torch.randn(ROWS_, NH_, CAP_, HD_, generator=gen).to(dtype).cuda()
    v = torch.randn(ROWS_, NH_, CAP_, HD_, generator=gen).to(dtype).cuda()
    slot = torch.randint(0, NB_, (ROWS_, CAP_ - PREFIX_), generator=gen, dtype=torch.int32).cuda()
    return qkv, k, v, slot


def _past_arg(past, dev):
    return torch.tensor([past], dtype=torch.int32, device="cuda") if dev else past


def _dense(k, slot, past):
    """The cache mvlt_attn_cached would need: row r holds, position by position, what the table points at."""
    first = (torch.arange(ROWS_, device="cuda") // NB_) * NB_
    out = k.clone()
    out[:, :, :PREFIX_] = k[first, :, :PREFIX_]
    for j in range(past - PREFIX_):
        out[:, :, PREFIX_ + j] = k[first + slot[:, j].long(), :, PREFIX_ + j]
    return out


@pytest.mark.parametrize("dev", [False, True], ids=["host-past", "past_dev"])
@pytest.mark.parametrize("past", [5, 6, 70, 200])
@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
def test_attn_cached_beam(M, dtype, past, dev):
    ops = M.ops
    qkv, k, v, slot = _attn_inputs(dtype, past, 900 + past)
    scale = HD_ ** -0.5
    own = (torch.arange(ROWS_, device="cuda") % NB_).to(torch.int32)
    first = (torch.arange(ROWS_, device="cuda") // NB_) * NB_
    # ---- identity table, prefix replicated into every row: mvlt_attn_cached on the same cache, bit for bit
    ki, vi = k.clone(), v.clone()
    ki[:, :, :PREFIX_], vi[:, :, :PREFIX_] = k[first, :, :PREFIX_], v[first, :, :PREFIX_]
    ka, va, kb, vb = ki.clone(), vi.clone(), ki.clone(), vi.clone()
    want = ops.attn_cached(qkv, ka, va, _past_arg(past, dev), scale)
    ident = own[:, None].expand(ROWS_, CAP_ - PREFIX_).contiguous()
    got = ops.attn_cached_beam(qkv, kb, vb, _past_arg(past, dev), scale, NB_, PREFIX_, ident)
    assert torch.equal(_bits(got), _bits(want))
    assert torch.equal(_bits(ka), _bits(kb)) and torch.equal(_bits(va), _bits(vb))
    # ---- random table; the prefix only in each sample's first row, every cell the table does not point at is NaN
    used = torch.zeros(ROWS_, CAP_, dtype=torch.bool, device="cuda")
    used[first.unique(), :PREFIX_] = True
    for j in range(past - PREFIX_):
        used[first + slot[:, j].long(), PREFIX_ + j] = True
    nan = torch.full_like(k, float("nan"))
    ks, vs = torch.where(used[:, None, :, None], k, nan), torch.where(used[:, None, :, None], v, nan)
    kd, vd = _dense(ks, slot, past), _dense(vs, slot, past)
    want = ops.attn_cached(qkv, kd, vd, _past_arg(past, dev), scale)
    k0, v0 = ks.clone(), vs.clone()
    got = ops.attn_cached_beam(qkv, ks, vs, _past_arg(past, dev), scale, NB_, PREFIX_, slot)
    assert not bool(torch.isnan(got.float()).any()) and torch.equal(_bits(got), _bits(want))
    # ---- only the cells (r, past) and (r, past + 1) changed, and they hold the new K / V
    new = qkv.view(ROWS_, NNEW_, 3, NH_, HD_)
    for cache, before, which in ((ks, k0, 1), (vs, v0, 2)):
        changed = (_bits(cache) != _bits(before)).any(3).any(1)          # [rows, cap]
        assert not bool(changed[:, :past].any()) and not bool(changed[:, past + NNEW_:].any())
        assert torch.equal(_bits(cache[:, :, past:past + NNEW_]), _bits(new[:, :, which].permute(0, 2, 1, 3)))
    # ---- a table with values outside [0, num_beams) gives the result of the clamped table
    bad = slot.clone()
    bad[::2, ::3] = -4
    bad[1::2, 1::3] = NB_ + 6
    k1, v1, k2, v2 = (t.clone() for t in (k, v, k, v))
    a = ops.attn_cached_beam(qkv, k1, v1, _past_arg(past, dev), scale, NB_, PREFIX_, bad)
    b = ops.attn_cached_beam(qkv, k2, v2, _past_arg(past, dev), scale, NB_, PREFIX_, bad.clamp(0, NB_ - 1))
    assert torch.equal(_bits(a), _bits(b))


def test_attn_cached_beam_refusals(M):
    ops = M.ops
    qkv, k, v, slot = _attn_inputs(BF16, 6, 1)
    with pytest.raises(RuntimeError, match="MVLT_ERR_ARG"):
        ops.attn_cached_beam(qkv, k, v, 6, 0.125, 4, PREFIX_, slot)                   # rows % num_beams
    with pytest.raises(RuntimeError, match="MVLT_ERR_ARG"):
        ops.attn_cached_beam(qkv, k, v, 4, 0.125, NB_, PREFIX_, slot)                 # past < prefix
    with pytest.raises(RuntimeError, match="MVLT_ERR_ARG"):
        ops.attn_cached_beam(qkv, k, v, CAP_ - 1, 0.125, NB_, PREFIX_, slot)          # past + n_new > cap
    k32 = torch.zeros(ROWS_, NH_ * 2, CAP_, 32, dtype=BF16, device="cuda")
    with pytest.raises(RuntimeError, match="MVLT_ERR_UNSUPPORTED"):
        ops.attn_cached_beam(qkv, k32, k32.clone(), 6, 0.125, NB_, PREFIX_, slot)     # hd != 64


# ------------------------------------------------------------------------------------------------ decode.beam_search
def _both_routes(model, image, nb, monkeypatch):
    monkeypatch.setenv("MVLT_BEAM_FUSED", "1")
    fused = model(image.cuda(), None, nb, 'unilm')
    monkeypatch.setenv("MVLT_BEAM_FUSED", "0")
    plain = model(image.cuda(), None, nb, 'unilm')
    monkeypatch.setenv("MVLT_BEAM_FUSED", "1")
    return fused.cpu(), plain.cpu()


@pytest.mark.parametrize("num_beams,B", [(3, 2), (2, 3), (5, 2)])
def test_fused_beam_search_matches_oracle_and_plain_route(M, specs, monkeypatch, num_beams, B):
    model, sd = _tiny_caption(M, specs, F32)
    O, scfg, bcfg = _tiny_oracle_cfgs()
    image, _, _, _ = synth_batch(B, 24, seed=80 + num_beams, vocab=3000)
    fused, plain = _both_routes(model, image, num_beams, monkeypatch)
    with torch.no_grad():
        ref = O.beam_decode_recompute(sd, scfg, bcfg, image, num_beams, model.config.max_length)
    assert torch.equal(fused, ref), (fused, ref)
    assert torch.equal(fused, plain), (fused, plain)
    # with [END] forced early: the most likely first token of sample 0 becomes the end token
    greedy, _ = model(image.cuda(), None, 1, 'unilm')
    old = model.config.eos_token_id
    try:
        model.config.eos_token_id = int(greedy[0, 1])
        bcfg2 = O.BertCfg(vocab_size=3000, hidden_size=256, num_hidden_layers=2, num_attention_heads=4, intermediate_size=1024,
                          eos_token_id=int(greedy[0, 1]))
        fused2, plain2 = _both_routes(model, image, num_beams, monkeypatch)
        with torch.no_grad():
            ref2 = O.beam_decode_recompute(sd, scfg, bcfg2, image, num_beams, model.config.max_length)
        assert torch.equal(fused2, ref2), (fused2, ref2)
        assert torch.equal(fused2, plain2), (fused2, plain2)
    finally:
        model.config.eos_token_id = old


def test_fused_route_never_touches_the_cache_rows(M, specs, monkeypatch):
    """layers x steps table-driven attention launches, no mvlt_attn_cached, no gather of a 4-D tensor, one set of cache tensors."""
    monkeypatch.setenv("MVLT_BEAM_FUSED", "1")
    model, _ = _tiny_caption(M, specs, F32)
    ops = M.ops
    calls = dict(beam=0, plain=0, cand=0, gather4d=0)
    ptrs = set()
    real_beam, real_plain, real_cand, real_sel = ops.attn_cached_beam, ops.attn_cached, ops.gemm_beam_candidates, torch.Tensor.index_select

    def spy_beam(qkv, k, v, *a, **kw):
        calls["beam"] += 1
        ptrs.add((k.data_ptr(), v.data_ptr()))
        return real_beam(qkv, k, v, *a, **kw)

    def spy_plain(*a, **kw):
        calls["plain"] += 1
        return real_plain(*a, **kw)

    def spy_cand(*a, **kw):
        calls["cand"] += 1
        return real_cand(*a, **kw)

    def spy_sel(self, *a, **kw):
        calls["gather4d"] += int(self.dim() == 4)
        return real_sel(self, *a, **kw)

    monkeypatch.setattr(ops, "attn_cached_beam", spy_beam)
    monkeypatch.setattr(ops, "attn_cached", spy_plain)
    monkeypatch.setattr(ops, "gemm_beam_candidates", spy_cand)
    monkeypatch.setattr(torch.Tensor, "index_select", spy_sel)
    image, _, _, _ = synth_batch(2, 24, seed=83, vocab=3000)
    out = model(image.cuda(), None, 3, 'unilm')
    nl = len(model.MVLBert.encoder.layer)
    steps = calls["cand"] - 1                                # every cached forward is followed by one candidate call
    assert out.shape[0] == 2 and steps >= 1
    assert calls["beam"] == nl * steps and calls["plain"] == 0 and calls["gather4d"] == 0, calls
    assert len(ptrs) == nl, ptrs


def test_fused_beam_search_bf16_teacher_forced(M, specs_hash, monkeypatch):
    """bf16: every step's candidate lists are classified against beam_ref computed from the operands the kernel itself was given
    at that step (its own activations and beam scores), as the sampled tests do."""
    monkeypatch.setenv("MVLT_BEAM_FUSED", "1")
    model, _ = _tiny(M, specs_hash, BF16, max_length=8)
    ops = M.ops
    rec = []
    real = ops.gemm_beam_candidates

    def spy(A, W, bias, bs, nb, n, **kw):
        out, lse = real(A, W, bias, bs, nb, n, **kw)
        rec.append((A.cpu().clone(), W, bias, bs.cpu().clone(), nb, n, out.cpu().clone()))
        return out, lse

    monkeypatch.setattr(ops, "gemm_beam_candidates", spy)
    image, _, _, _ = synth_batch(3, 24, seed=91, vocab=3000)
    out = model(image.cuda(), None, 4, 'unilm')
    assert out.shape[0] == 3 and len(rec) >= 2
    exact = near = lists = 0
    worst = 0.0
    Wc, bc = rec[0][1].cpu(), rec[0][2].cpu()
    for A, _, _, bs, nb, n, res in rec:
        ref = R.beam_ref(A, Wc, bc, bs, nb, n)
        e, nr, wrong, w = R.classify(ref, *_split(res))
        assert not wrong, wrong
        exact, near, lists, worst = exact + e, near + nr, lists + ref["G"], max(worst, w)
    print(f"bf16 beam search: {exact} exact, {near} near of {lists} lists over {len(rec)} steps; worst score ratio {worst:.3f}")
    assert near <= R.NEAR_TIE_CAP * lists, (near, lists)


def test_nine_beams_take_the_plain_route(M, specs, monkeypatch):
    model, _ = _tiny_caption(M, specs, F32)
    called = []
    monkeypatch.setattr(M.ops, "attn_cached_beam", lambda *a, **kw: called.append(1))
    image, _, _, _ = synth_batch(2, 24, seed=89, vocab=3000)
    fused, plain = _both_routes(model, image, 9, monkeypatch)
    assert not called and torch.equal(fused, plain)
