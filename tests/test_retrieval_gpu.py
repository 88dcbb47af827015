"""Retrieval on the GPU: recall ranks and counts (exact, against the numpy reference), the fused scoring head (every stage per
element against the float64 reference of tests/retrieval_ref.py, from the kernel's own stored input), and the all-pairs driver
against single-pair forward calls and the oracle.  tests/test_retrieval_bound_cpu.py proves the references first.

Tolerances: ranks and counts are integers, compared exactly.  Head: the derived per-element bounds of retrieval_ref.  Driver in
f32: 2e-4 relative (Frobenius), the suite's tolerance for this head (test_model_gpu.test_retrieval_head_forward).  Driver in
bf16: nothing fixed in advance -- the test measures what the existing route (model(image, caption) in bf16) loses against f32 on
the same pairs and allows the new route twice that (one factor for the rounding points that moved)."""
import numpy as np
import pytest
import torch

import retrieval_ref as R
from conftest import rel_err, synth_batch
from gemm_ref import check_bound

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
SENTINEL = -7.0


@pytest.fixture(scope="module")
def M():
    import mvlt_amd
    return mvlt_amd


# ------------------------------------------------------------------------------------------------ ranks
@pytest.mark.parametrize("Ni,Nc", [(1, 1), (5, 7), (67, 130)])
def test_recall_ranks_equal_the_numpy_reference(M, Ni, Nc):
    from mvlt_amd import ops
    s, ig, cg = R.rank_case(Ni, Nc, 100 + Ni)
    ref_i2t, ref_t2i = R.recall_ranks_ref(s, ig, cg)
    if Ni > 2:
        assert np.isnan(s).sum() == 1 and ref_i2t[1] == Nc and ref_t2i[2] == Ni and ref_i2t[0] == 1      # the cases are in
        assert len(set(ig.tolist())) < Ni
    if Ni > 4:
        assert ref_t2i[Nc - 2] == 1
    wide = torch.full((Ni, Nc + 3), 9.0, dtype=F32)          # ld > Nc: columns beyond Nc would outrank everything
    wide[:, :Nc] = torch.from_numpy(s)
    dev = wide.cuda()[:, :Nc]
    i2t, t2i = M.recall_ranks(dev, torch.from_numpy(ig), torch.from_numpy(cg))
    assert i2t.dtype == torch.int32 and t2i.dtype == torch.int32 and i2t.is_cuda
    assert i2t.cpu().tolist() == ref_i2t.tolist()
    assert t2i.cpu().tolist() == ref_t2i.tolist()
    for rank, ref in ((i2t, ref_i2t), (t2i, ref_t2i)):
        ks = (1, 5, 10, 64)
        got = ops.recall_counts(rank.contiguous(), ks).cpu().tolist()
        assert got == [int((ref < k).sum()) for k in ks]
    assert M.evaluate(dev, ig, cg) == R.recalls_ref(ref_i2t, ref_t2i)


def test_recall_ranks_refusals(M):
    from mvlt_amd import _lib
    L = _lib.lib()
    x = torch.zeros(4, 4, device="cuda")
    g = torch.zeros(4, dtype=torch.int64, device="cuda")
    r = torch.zeros(4, dtype=torch.int32, device="cuda")
    args = lambda ld, ni, nc: (x.data_ptr(), ld, ni, nc, g.data_ptr(), g.data_ptr(), r.data_ptr(), r.data_ptr(), None)
    assert L.mvlt_recall_ranks(*args(3, 4, 4)) == -1 and L.mvlt_recall_ranks(*args(4, 0, 4)) == -1
    assert L.mvlt_recall_ranks(None, 4, 4, 4, g.data_ptr(), g.data_ptr(), r.data_ptr(), r.data_ptr(), None) == -1


# ------------------------------------------------------------------------------------------------ head kernel
def _run_head(M, H, P, p_dev=None):
    from mvlt_amd import ops
    hidden, row_start, w, out_index, n_scores = R.head_operands(H, P, 1000 + H + P)
    scores = torch.full((n_scores,), SENTINEL, dtype=F32, device="cuda")
    c = lambda t: t.cuda().contiguous()
    pd = None if p_dev is None else torch.tensor([p_dev], dtype=torch.int32, device="cuda")
    extra = ops.retrieval_head(c(hidden), c(row_start), c(w["w_pool"]), c(w["b_pool"]), c(w["w_tr"]), c(w["b_tr"]), c(w["gamma"]),
                               c(w["beta"]), w["eps"], c(w["w_out"]), c(w["b_out"]), c(out_index), scores, p_dev=pd, want=True)
    torch.cuda.synchronize()
    return hidden, row_start, w, out_index, scores.cpu(), [t.cpu() for t in extra]


@pytest.mark.parametrize("H", [256, 768])
@pytest.mark.parametrize("P", [1, 33, 70])
def test_retrieval_head_every_stage_within_its_bound(M, H, P):
    hidden, row_start, w, out_index, scores, (pooled, t1, logits) = _run_head(M, H, P)
    x = hidden[row_start.long()]
    ref, bound = R.pooled_ref(x, w["w_pool"], w["b_pool"])
    check_bound(pooled, ref, bound, "pooled")
    ref, bound = R.t1_ref(pooled, w["w_tr"], w["b_tr"])                      # from the kernel's own pooled
    check_bound(t1, ref, bound, "t1")
    t = R.tail_ref(t1, w["gamma"], w["beta"], w["eps"], w["w_out"], w["b_out"])          # from the kernel's own t1
    check_bound(logits, t["logits"], t["bound_logits"], "logits")
    got = scores[out_index]
    check_bound(got, t["prob"], t["bound_prob"], "scores")
    ref, bound = R.softmax_ref(logits)                                         # from the kernel's own logits
    check_bound(got, ref, bound, "scores against the softmax of the returned logits")
    untouched = torch.ones(scores.numel(), dtype=torch.bool)
    untouched[out_index] = False
    assert bool((scores[untouched] == SENTINEL).all()) and int(untouched.sum()) == P + 3


def test_retrieval_head_device_side_pair_count(M):
    P, live = 70, 37
    hidden, row_start, w, out_index, scores, (pooled, t1, logits) = _run_head(M, 256, P, p_dev=live)
    t = R.tail_ref(t1[:live], w["gamma"], w["beta"], w["eps"], w["w_out"], w["b_out"])
    check_bound(scores[out_index[:live]], t["prob"], t["bound_prob"], "scores of the live pairs")
    assert bool((scores[out_index[live:]] == SENTINEL).all())


def test_retrieval_head_refusals(M):
    from mvlt_amd import ops
    assert ops.retrieval_head_supported(BF16, 256) and ops.retrieval_head_supported(BF16, 1024)
    assert not ops.retrieval_head_supported(F32, 256)
    assert not ops.retrieval_head_supported(BF16, 96) and not ops.retrieval_head_supported(BF16, 1088)
    H, P = 96, 3
    z = lambda *s, dt=BF16: torch.zeros(*s, dtype=dt, device="cuda")
    scores = torch.full((P,), SENTINEL, device="cuda")
    with pytest.raises(RuntimeError, match="MVLT_ERR_UNSUPPORTED"):
        ops.retrieval_head(z(P, H), torch.arange(P, dtype=torch.int32, device="cuda"), z(H, H), z(H, dt=F32), z(H, H), z(H, dt=F32),
                           z(H, dt=F32), z(H, dt=F32), 1e-12, z(2, H), z(2, dt=F32), torch.arange(P, device="cuda"), scores)
    torch.cuda.synchronize()
    assert bool((scores == SENTINEL).all())


# ------------------------------------------------------------------------------------------------ driver
NI, NC, T = 6, 6, 24


def _tiny_model(M, cd):
    """The tiny configuration of tests/test_model_gpu.py (hidden 256, 2 layers, 4 heads, Swin embed 32, vocabulary 3000)."""
    cfg = M.MVLBertRetrieval(hidden_size=256, num_hidden_layers=2, num_attention_heads=4, intermediate_size=1024, vocab_size=3000)
    cfg.swin.update(embed_dim=32, depths=[2, 2, 2, 2], num_heads=[1, 2, 4, 8], drop_path_rate=0.2)
    torch.manual_seed(4)
    model = M.MVLBertForRetrieval(cfg)
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    return M.set_compute_dtype(model.cuda().eval(), cd), sd


def _singles(model, image, ids):
    out = torch.empty(image.shape[0], ids.shape[0])
    with torch.no_grad():
        for i in range(image.shape[0]):
            for j in range(ids.shape[0]):
                out[i, j] = model(image[i:i + 1], ids[j:j + 1])[0, 1]
    return out


@pytest.fixture(scope="module")
def data(M):
    """6 images x 6 captions of unequal length, the 36 single-pair f32 scores (computed once, shared, never changed)."""
    image, ids, _, _ = synth_batch(NI, T, seed=43, vocab=3000)
    lens = (ids != 0).sum(1).tolist()
    assert len(set(lens[:4])) > 1, lens
    model, sd = _tiny_model(M, F32)
    single = _singles(model, image.cuda(), ids.cuda())
    return dict(image=image, ids=ids, model=model, sd=sd, single=single)


@pytest.mark.parametrize("pair_chunk", [5, 12])
def test_score_all_pairs_f32_equals_single_pair_calls_and_the_oracle(M, data, pair_chunk):
    from oracle import mvlt_oracle as O
    image, ids, model, sd = data["image"][:3], data["ids"][:4], data["model"], data["sd"]
    scores = M.score_all_pairs(model, image.cuda(), ids.cuda(), pair_chunk=pair_chunk)
    assert scores.shape == (3, 4) and scores.dtype == F32 and scores.is_cuda
    err = rel_err(scores.cpu(), data["single"][:3, :4])
    print(f"pair_chunk {pair_chunk}: against the single-pair calls {err:.3g}")
    assert err < 2e-4
    with torch.no_grad():
        scfg = O.SwinCfg(embed_dim=32, depths=(2, 2, 2, 2), num_heads=(1, 2, 4, 8), drop_path_rate=0.2)
        bcfg = O.BertCfg(vocab_size=3000, hidden_size=256, num_hidden_layers=2, num_attention_heads=4, intermediate_size=1024)
        feat = O.conv_layer(image, sd, scfg)
        ii = torch.arange(12) // 4
        o = O.mvlbert_forward(sd, bcfg, ids[torch.arange(12) % 4], feat[ii], False)
        h = O._ln(torch.nn.functional.gelu(O._lin(o["pooled"], sd, "final_mlp.0.dense")), sd, "final_mlp.0.LayerNorm", 1e-12)
        ref = O._lin(h, sd, "final_mlp.1").softmax(-1)[:, 1].view(3, 4)
    err = rel_err(scores.cpu(), ref)
    print(f"pair_chunk {pair_chunk}: against the oracle {err:.3g}")
    assert err < 2e-4


def test_score_all_pairs_host_and_device_images_agree_and_training_raises(M, data):
    image, ids, model = data["image"][:3], data["ids"][:4], data["model"]
    a = M.score_all_pairs(model, image.cuda(), ids.cuda(), pair_chunk=5, image_chunk=2)
    b = M.score_all_pairs(model, image, ids, pair_chunk=5, image_chunk=2)
    assert torch.equal(a, b)
    pairs = model.score_pairs(model.encode_images(image.cuda()), ids.cuda(), torch.tensor([2, 0], device="cuda"),
                              torch.tensor([1, 3], device="cuda"))
    assert pairs.shape == (2,) and rel_err(pairs.cpu(), data["single"][[2, 0], [1, 3]]) < 2e-4
    model.train()
    try:
        with pytest.raises(ValueError, match="eval"):
            M.score_all_pairs(model, image.cuda(), ids.cuda())
        with pytest.raises(ValueError, match="eval"):
            model.encode_images(image.cuda())
    finally:
        model.eval()


@pytest.mark.parametrize("fused", [False, True])
def test_score_all_pairs_bf16_within_twice_the_existing_routes_error(M, data, monkeypatch, fused):
    """Both heads of score_pairs: the separate launches (default) and mvlt_retrieval_head (MVLT_RETRIEVAL_HEAD=1).  Measured on an
    MI355X on these 12 pairs (profiles/retrieval.md), max abs difference of the probability against f32: the existing bf16 route
    1.553e-3, score_all_pairs 2.815e-3 (separate launches) and 2.227e-3 (fused head); allowed 3.106e-3."""
    import mvlt_amd.model as model_mod
    from mvlt_amd import ops
    monkeypatch.setattr(model_mod, "_RETRIEVAL_HEAD", fused)
    image, ids = data["image"][:3].cuda(), data["ids"][:4].cuda()
    ref = data["single"][:3, :4]
    model, _ = _tiny_model(M, BF16)
    assert ops.retrieval_head_supported(BF16, 256)          # fused = True does take the kernel
    e_old = float((_singles(model, image, ids) - ref).abs().max())
    scores = M.score_all_pairs(model, image, ids, pair_chunk=5)
    e_new = float((scores.cpu() - ref).abs().max())
    print(f"bf16 against f32, max abs difference of the probability: existing route {e_old:.4g}, score_all_pairs "
          f"({'fused head' if fused else 'separate launches'}) {e_new:.4g}")
    assert e_new <= 2 * e_old


def test_evaluate_reproduces_the_recalls_of_the_single_pair_calls(M, data):
    model = data["model"]
    groups = [0, 1, 2, 1, 4, 5]                     # images 1 and 3 share a group (the reference's cap_id)
    scores = M.score_all_pairs(model, data["image"], data["ids"].cuda(), pair_chunk=16)
    got = M.evaluate(scores, groups, groups, ks=(1, 2, 5))
    i2t, t2i = R.recall_ranks_ref(data["single"].numpy(), groups, groups)
    assert got == R.recalls_ref(i2t, t2i, ks=(1, 2, 5))
    ri, rt = M.recall_ranks(scores, groups, groups)
    assert ri.cpu().tolist() == i2t.tolist() and rt.cpu().tolist() == t2i.tolist()
