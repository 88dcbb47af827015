"""Host proof of tests/beam_rules_ref.py and host side of the logit rules in beam search: the reference against the installed
transformers processors applied to log_softmax scores (the placement of HF 4.16 beam_search), an f32 emulation of the kernel's
sequence inside the bound with four wrong implementations outside it, the inputs of tests/test_beam_rules_gpu.py unambiguous in the
reference alone, the argument checks, the route table (unchanged) and the two new C symbols."""
import ctypes
import functools
import os
import re
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beam_ref as B  # noqa: E402
import beam_rules_ref as R  # noqa: E402
import logit_rules_ref as LR  # noqa: E402
import sample_ref as S  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF16, F32 = torch.bfloat16, torch.float32


def x_f32(A, W, bias):
    """f32 logits the way an f32-accumulating product forms them (f32 matmul of the stored operands, one rounded bias add)."""
    return (A.float() @ W.float().t() + bias.float()[None, :]).float()


@functools.lru_cache(maxsize=None)
def small(G, nb, dtype):
    A, W, bias, bs = R.case_operands(G, nb, dtype)
    base = S.sample_ref(A, W, bias, 0, 0)
    ref0 = B.beam_ref(A, W, bias, bs, nb, 2 * nb)
    return A, W, bias, bs, base, ref0


def ruled(G, nb, dtype, rules, c=R.C_HIST):
    A, W, bias, bs, base, ref0 = small(G, nb, dtype)
    h = R.histories(ref0, c)
    return h, R.beam_rules_ref(A, W, bias, bs, nb, 2 * nb, h, *rules, eos=R.EOS, ref0=ref0, base=base)


# ------------------------------------------------------------------------------------------------ the reference
@pytest.mark.parametrize("g", [0, 1, 2, 3])
def test_reference_equals_the_transformers_processors_on_log_softmax(g):
    from transformers import MinLengthLogitsProcessor, NoRepeatNGramLogitsProcessor, RepetitionPenaltyLogitsProcessor
    gen = torch.Generator().manual_seed(70 + g)
    V, G, nb, eos = 97, 3, 2, 11
    rows = G * nb
    for c in (0, 1, 12):
        h = torch.randint(1, V, (rows, c), generator=gen)
        if c >= 8:
            h[0, c - 2:] = h[0, 1:3]                      # a bigram that returns
            h[1, c - 3:] = h[1, 0:3]                      # a trigram that returns
            h[2, :] = 7                                   # one token, many times
        x = (torch.randn(rows, V, generator=gen) * 3).double()
        bs = -torch.rand(rows, generator=gen) * 4
        for penalty, min_length in ((1.0, 0), (1.25, 0), (0.75, 14), (2.0, c)):          # (penalties exact in f32)
            want = torch.log_softmax(x, -1)
            if penalty != 1.0:
                want = RepetitionPenaltyLogitsProcessor(penalty)(h, want)
            if g >= 1:
                want = NoRepeatNGramLogitsProcessor(g)(h, want)
            if min_length > 0:
                want = MinLengthLogitsProcessor(min_length, eos, device="cpu")(h, want)
            want = want + bs.double()[:, None]
            ref = R.beam_rules_ref(None, None, None, bs, nb, 2 * nb, h, penalty, g, min_length, eos,
                                   base=dict(x=x, e_x=torch.zeros_like(x)))
            assert torch.equal(ref["banned"], torch.isinf(want)), (g, c, penalty, min_length)
            got = torch.where(ref["banned"], torch.full_like(want, -float("inf")), ref["s"])
            fin = ~ref["banned"]
            assert float((got[fin] - want[fin]).abs().max()) < 1e-12, (g, c, penalty, min_length)
            top = torch.topk(want.view(G, nb * V), 2 * nb, dim=1).indices
            assert torch.equal(ref["flat"], top), (g, c, penalty, min_length)


@pytest.mark.parametrize("G,nb", [(3, 2), (2, 5)])
def test_rules_off_is_beam_ref(G, nb):
    A, W, bias, bs, base, ref0 = small(G, nb, BF16)
    for c in (0, R.C_HIST):
        ref = R.beam_rules_ref(A, W, bias, bs, nb, 2 * nb, R.histories(ref0, c), 1.0, 0, 0, R.EOS, base=base)
        assert torch.equal(ref["s"], ref0["s"]) and torch.equal(ref["bound_s"], ref0["bound_s"])
        assert torch.equal(ref["flat"], ref0["flat"]) and not bool(ref["banned"].any())
        assert torch.equal(R.ambiguous(ref), B.ambiguous(ref0))


def test_every_rule_set_changes_every_list():
    """The histories are built around each sample's own candidates: no rule set leaves a list (entries and scores) of the c = 12
    cases as it was."""
    for G, nb in B.CASES:
        ref0 = small(G, nb, BF16)[5]
        for rules in LR.RULE_SETS:
            _, ref = ruled(G, nb, BF16, rules)
            N = ref["N"]          # (a mild penalty may leave the ORDER of a list: then its scores moved)
            score, score0 = (r["s"].view(G, nb * N).gather(1, r["flat"]) for r in (ref, ref0))
            same = (ref["flat"] == ref0["flat"]).all(1) & (score == score0).all(1)
            assert not bool(same.any()), (G, nb, rules, same.nonzero().flatten().tolist())


def test_classify_never_accepts_a_banned_entry_and_checks_the_fill():
    G, nb = 3, 2
    h, ref = ruled(G, nb, BF16, (1.0, 2, 0))
    N, n = ref["N"], ref["n_cand"]
    flat = ref["flat"]
    score = ref["s"].view(G, nb * N).gather(1, flat).float()
    assert R.classify(ref, flat // N, flat % N, score)[:3] == (G, 0, [])
    ban = int(ref["banned"].view(G, nb * N)[0].nonzero()[0])          # a banned entry in the place of the last one, with its own score
    bad = flat.clone()
    bad[0, n - 1] = ban
    sc = score.clone()
    sc[0, n - 1] = float(ref["s"].view(G, nb * N)[0, ban])
    wrong = R.classify(ref, bad // N, bad % N, sc)[2]
    assert len(wrong) == 1 and wrong[0][0] == 0 and "banned" in wrong[0][1]
    # a sample with two unbanned entries: the other slots must hold (-inf, 0, 0)
    x = torch.arange(6, dtype=torch.float64)[None].repeat(2, 1)
    hist = torch.tensor([[0, 1, 2, 3], [0, 1, 2, 3]])
    r = R.beam_rules_ref(None, None, None, torch.zeros(2), 1, 4, hist, 1.0, 1, 0, None, base=dict(x=x, e_x=torch.full_like(x, 1e-6)))
    assert r["valid"].tolist() == [2, 2] and r["flat"][0].tolist() == [5, 4, -1, -1]
    lp = (x[0] - torch.logsumexp(x[0], 0)).float()
    good = (torch.zeros(2, 4, dtype=torch.long), torch.tensor([[5, 4, 0, 0]] * 2),
            torch.stack([torch.stack([lp[5], lp[4], torch.tensor(-float("inf")), torch.tensor(-float("inf"))])] * 2))
    assert R.classify(r, *good)[:3] == (2, 0, [])
    for what in ("tok", "score"):
        beam, tok, score2 = (v.clone() for v in good)
        if what == "tok":
            tok[1, 3] = 4
        else:
            score2[1, 2] = -1e30
        wrong = R.classify(r, beam, tok, score2)[2]
        assert len(wrong) == 1 and wrong[0][0] == 1 and "empty" in wrong[0][1], (what, wrong)


# ------------------------------------------------------------------------------------------------ the emulation
@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("G,nb", B.CASES)
def test_f32_emulation_stays_inside_the_bound(G, nb, dtype):
    A, W, bias, bs, _, _ = small(G, nb, dtype)
    x32 = x_f32(A, W, bias)
    for rules in LR.RULE_SETS:
        for c in (R.C_HIST, 0):
            h, ref = ruled(G, nb, dtype, rules, c)
            out = R.emulate(x32, bs, nb, 2 * nb, h, *rules, eos=R.EOS)
            exact, near, wrong, worst = R.classify(ref, *out)
            assert not wrong and worst <= 0.5, (rules, c, exact, near, wrong, worst)
            assert near <= int(R.ambiguous(ref).sum()), (rules, c, near)


# the rule sets on which a wrong implementation changes a list (per_occurrence: under (2.0, 3, 20) the tokens that occur twice
# are banned as well, so their penalty shows nowhere)
BEARS = {"on_logits": [(1.3, 0, 0), (2.0, 3, 20), (1.0, 2, 0)], "per_occurrence": [(1.3, 0, 0)],
         "lse_without_banned": [(1.0, 2, 0), (2.0, 3, 20), (1.0, 1, 0)], "pre_reorder": list(LR.RULE_SETS)}


@pytest.mark.parametrize("variant", R.WRONG)
def test_wrong_implementations_are_caught(variant):
    G, nb = 8, 8
    A, W, bias, bs, _, _ = small(G, nb, BF16)
    x32 = x_f32(A, W, bias)
    for rules in BEARS[variant]:
        h, ref = ruled(G, nb, BF16, rules)
        exact, near, wrong, worst = R.classify(ref, *R.emulate(x32, bs, nb, 2 * nb, h, *rules, eos=R.EOS, wrong=variant))
        print(f"{variant} {rules}: {exact} exact, {near} near, {len(wrong)} wrong, worst ratio {worst:.1f}")
        assert len(wrong) >= G // 2, (variant, rules, exact, near, wrong, worst)


def test_gpu_inputs_are_not_ambiguous():
    """No list of the GPU cases is ambiguous by the reference alone: NEAR_TIE_CAP stays the only allowance there."""
    for dtype in (BF16, F32):
        for G, nb in B.CASES:
            for rules in LR.RULE_SETS:
                for c in (R.C_HIST, 0):
                    a = R.ambiguous(ruled(G, nb, dtype, rules, c)[1])
                    assert not bool(a.any()), (G, nb, dtype, rules, c, a.nonzero().flatten().tolist())


def test_the_real_size_input_is_not_ambiguous():
    A, W, bias, bs = B.case_operands(0, 0, BF16, big=True)
    nb = B.BIG["num_beams"]
    base = S.sample_ref(A, W, bias, 0, 0)
    ref0 = B.beam_ref(A, W, bias, bs, nb, 2 * nb)
    rules = LR.RULE_SETS[2]
    ref = R.beam_rules_ref(A, W, bias, bs, nb, 2 * nb, R.histories(ref0), *rules, eos=R.EOS, ref0=ref0, base=base)
    a = R.ambiguous(ref)
    assert not bool(a.any()), a.nonzero().flatten().tolist()
    assert not bool((ref["flat"] == ref0["flat"]).all(1).any())


# ------------------------------------------------------------------------------------------------ host logic
def test_argument_checks_and_the_vocabulary_refusal():
    from mvlt_amd.decode import check_beam_rules, check_logit_rules
    assert check_beam_rules(1.0, 0, 0, 5, 10, 150) == (1.0, 0, 0)                       # all off: no limit on the vocabulary
    assert check_beam_rules(1.2, 3, 10, 5, 30522, 150) == (1.2, 3, 10)
    for bad in (dict(repetition_penalty=0.0), dict(repetition_penalty=float("nan")), dict(no_repeat_ngram_size=-1),
                dict(min_length=-1), dict(no_repeat_ngram_size=1.5)):
        args = dict(repetition_penalty=1.0, no_repeat_ngram_size=0, min_length=0)
        args.update(bad)
        with pytest.raises(ValueError):
            check_beam_rules(num_beams=3, V=3000, max_length=8, **args)
    for on in (dict(repetition_penalty=1.2), dict(no_repeat_ngram_size=2), dict(min_length=3)):
        args = dict(repetition_penalty=1.0, no_repeat_ngram_size=0, min_length=0)
        args.update(on)
        with pytest.raises(ValueError, match="vocabulary"):
            check_beam_rules(num_beams=3, V=151, max_length=150, **args)                  # max_length + 2 decides
        check_beam_rules(num_beams=3, V=152, max_length=150, **args)
        with pytest.raises(ValueError, match="vocabulary"):
            check_beam_rules(num_beams=8, V=16, max_length=4, **args)                     # 2 * num_beams + 1 decides
        check_beam_rules(num_beams=8, V=17, max_length=4, **args)
        with pytest.raises(ValueError, match="beam"):                                     # the greedy check still refuses beams
            check_logit_rules(num_beams=2, **on)


def test_model_refusals_need_no_gpu():
    import mvlt_amd as M
    cfg = M.MVLBertConfigForImageCaption(hidden_size=256, num_hidden_layers=1, num_attention_heads=4, intermediate_size=256, vocab_size=200)
    cfg.swin.update(embed_dim=32, depths=[1, 1, 1, 1], num_heads=[1, 2, 4, 8])
    cfg.max_length = 199
    model = M.MVLBertForImageCaption(cfg, tokenizer=type("Tok", (), {"mask_token_id": 103, "sep_token_id": 102})())
    from mvlt_amd.decode import beam_search
    with pytest.raises(ValueError, match="vocabulary"):
        beam_search(model, None, 3, no_repeat_ngram_size=2)                               # 200 < 199 + 2, checked before the image
    with pytest.raises(ValueError, match="repetition_penalty"):
        beam_search(model, None, 3, repetition_penalty=0.0)
    with pytest.raises(ValueError, match="generate"):
        model(None, None, 3, 'unilm', no_repeat_ngram_size=2)                             # forward still refuses, and says where to go
    for sampling in (dict(sample_mode='sample'), dict(top_k=5), dict(top_p=0.9), dict(temperature=0.7), dict(seed=3)):
        with pytest.raises(ValueError, match="beam"):
            model.generate(None, num_beams=3, **sampling)
    with pytest.raises(ValueError):
        model.generate(None, num_beams=0)


@pytest.mark.parametrize("args,route", [
    ((5, 64, 150, True, None), 'fused'), ((5, 64, 150, False, None), 'plain'), ((9, 64, 150, True, None), 'plain'),
    ((5, 32, 150, True, None), 'plain'), ((5, 64, 150, True, True), 'device'), ((5, 64, 150, True, None, True), 'device'),
    ((5, 64, 150, True, False, True), 'fused'), ((8, 64, 1025, True, True), 'fused'), ((5, 64, 150, False, True), 'plain'),
])
def test_beam_route_is_unchanged(args, route):
    from mvlt_amd import decode
    assert decode._beam_route(*args) == route


def test_new_symbols_and_unchanged_abi():
    from mvlt_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "mvlt_hip.h")).read()
    assert re.search(r"MVLT_STRUCT_LOGIT_RULES = 20, MVLT_STRUCT_COUNT = 21", hdr)
    assert int(re.search(r"#define\s+MVLT_ABI_VERSION\s+(\d+)", hdr).group(1)) == 17 == _lib.ABI_VERSION
    assert len(_lib.STRUCTS) == 21 and _lib.lib().mvlt_version() == 17
    assert _lib.lib().mvlt_sizeof(20) == ctypes.sizeof(_lib.MvltLogitRules) == 80
    assert re.search(r"int mvlt_beam_rules_plan\(const MvltLogitRules\* rules, const int32_t\* seq, int64_t ld_seq, int rows, int V, "
                     r"void\* stream\);", hdr)
    assert re.search(r"int mvlt_gemm_beam_candidates_rules\(const MvltGemm\* p, const MvltBeamCand\* c, const MvltLogitRules\* rules, "
                     r"void\* stream\);", hdr)
    for name, nargs in (("mvlt_beam_rules_plan", 6), ("mvlt_gemm_beam_candidates_rules", 4)):
        assert name in _lib.SYMBOLS and len(_lib.SYMBOLS[name][1]) == nargs and hasattr(_lib.lib(), name), name
