"""The yardsticks of tests/test_retrieval_gpu.py, proven on the host before they judge a kernel: the numpy rank reference against
np.argsort(kind="stable")[::-1], and the float64 head reference against damage it must reject and f32 arithmetic it must accept."""
import numpy as np
import pytest
import torch

import retrieval_ref as R
from gemm_ref import check_bound

H, P = 256, 37


# ------------------------------------------------------------------------------------------------ ranks
@pytest.mark.parametrize("n,levels", [(1, 1), (7, 3), (50, 4), (64, 1000000)])
def test_rank_reference_is_the_stable_sort_reversed(n, levels):
    g = np.random.default_rng(n + levels)
    for trial in range(40):
        sim = (g.integers(0, levels, size=n) / 8.0).astype(np.float32)          # few levels: ties everywhere; many: none
        match = g.random(n) < (0.0 if trial == 0 else 0.2)
        assert R.rank_line(sim, match) == R.rank_line_argsort(sim, match)


def test_rank_reference_tie_rule_and_nan():
    sim = np.array([0.5, 0.5, 0.5, 0.25], dtype=np.float32)
    assert R.rank_line(sim, [False, True, False, False]) == 1          # index 2 sorts before the match, index 0 after it
    assert R.rank_line(sim, [True, True, False, False]) == 1           # best match = the higher index of the two
    assert R.rank_line(sim, [False] * 4) == 4
    nan = np.array([np.nan, -np.inf, 0.0, -0.0], dtype=np.float32)
    assert R.rank_line(nan, [True, False, False, False]) == 3          # NaN is below -inf
    assert R.rank_line(nan, [False, True, False, False]) == 2
    assert R.rank_line(nan, [False, False, True, False]) == 1          # -0 == +0: the higher index first


def test_rank_case_holds_every_case():
    s, ig, cg = R.rank_case(67, 130, 3)
    i2t, t2i = R.recall_ranks_ref(s, ig, cg)
    assert i2t[1] == 130 and t2i[2] == 67 and np.isnan(s).sum() == 1
    assert i2t[0] == 1 and t2i[128] == 1          # one tied non-match on the high-index side of the match, others below
    assert len(set(ig.tolist())) < 67             # duplicated groups


# ------------------------------------------------------------------------------------------------ head
@pytest.fixture(scope="module")
def case():
    hidden, row_start, w, out_index, n_scores = R.head_operands(H, P, 11)
    x = hidden[row_start.long()]
    return x, w


def _check_all(x, w, pooled, t1, logits, prob):
    ref, bound = R.pooled_ref(x, w["w_pool"], w["b_pool"])
    check_bound(pooled, ref, bound, "pooled")
    ref, bound = R.t1_ref(pooled, w["w_tr"], w["b_tr"])
    check_bound(t1, ref, bound, "t1")
    t = R.tail_ref(t1, w["gamma"], w["beta"], w["eps"], w["w_out"], w["b_out"])
    check_bound(logits, t["logits"], t["bound_logits"], "logits")
    check_bound(prob, t["prob"], t["bound_prob"], "prob")
    ref, bound = R.softmax_ref(logits)
    check_bound(prob, ref, bound, "softmax of the logits")


@pytest.mark.parametrize("order", [0, 1, 2])
def test_head_reference_accepts_f32_in_three_summation_orders(case, order):
    x, w = case
    _check_all(x, w, *R.emulate_f32(x, w, order))


def test_head_reference_rejects_one_damaged_element(case):
    x, w = case
    pooled, t1, logits, prob = R.emulate_f32(x, w, 0)
    for name, good, ref in (("pooled", pooled, R.pooled_ref(x, w["w_pool"], w["b_pool"])),
                            ("t1", t1, R.t1_ref(pooled, w["w_tr"], w["b_tr"]))):
        bad = good.clone()
        r, c = divmod(int(good.float().abs().argmax()), H)
        bad[r, c] = (bad[r, c].float() * (1 + 3 * 2.0 ** -7)).to(torch.bfloat16)          # three steps of the bf16 grid
        with pytest.raises(AssertionError, match=f"{name}: 1 of"):
            check_bound(bad, ref[0], ref[1], name)


@pytest.mark.parametrize("which", ["w_pool", "w_tr"])
def test_head_reference_rejects_a_dropped_k_tile(case, which):
    x, w = case
    w2 = dict(w)
    w2[which] = w[which].clone()
    w2[which][:, 96:128] = 0                     # the product skips one 32-wide k-block
    pooled, t1, _, _ = R.emulate_f32(x, w2, 0)
    if which == "w_pool":
        ref, bound = R.pooled_ref(x, w["w_pool"], w["b_pool"])
        out, what = pooled, "pooled"
    else:
        ref, bound = R.t1_ref(pooled, w["w_tr"], w["b_tr"])
        out, what = t1, "t1"
    with pytest.raises(AssertionError, match="outside the bound"):
        check_bound(out, ref, bound, what)
    # ... and row by row: no row of the damaged product passes
    ratio = (out.double() - ref).abs() / bound
    assert bool((ratio.max(1).values > 1).all())


def test_head_reference_rejects_a_row_block_left_unwritten(case):
    x, w = case
    pooled, t1, logits, prob = R.emulate_f32(x, w, 0)
    lo, hi = R.RB, 2 * R.RB
    for name, good, ref in (("pooled", pooled, R.pooled_ref(x, w["w_pool"], w["b_pool"])),
                            ("t1", t1, R.t1_ref(pooled, w["w_tr"], w["b_tr"]))):
        bad = good.clone()
        bad[lo:hi] = 0
        with pytest.raises(AssertionError, match="outside the bound"):
            check_bound(bad, ref[0], ref[1], name)
    t = R.tail_ref(t1, w["gamma"], w["beta"], w["eps"], w["w_out"], w["b_out"])
    bad = prob.clone()
    bad[lo:hi] = -7.0                            # the sentinel of the GPU test
    with pytest.raises(AssertionError, match="outside the bound"):
        check_bound(bad, t["prob"], t["bound_prob"], "prob")


def test_tail_reference_rejects_a_dropped_column_group(case):
    x, w = case
    _, t1, _, _ = R.emulate_f32(x, w, 0)
    t = R.tail_ref(t1, w["gamma"], w["beta"], w["eps"], w["w_out"], w["b_out"])
    y = ((t1.double() - t1.double().mean(1, keepdim=True)))
    n = int((y[5].abs() * w["w_out"].double().abs().min(0).values).view(-1, 4).sum(1).argmax()) * 4
    logits, prob = R.emulate_tail_f32(t1, w, 1, drop_group=(5, n))
    with pytest.raises(AssertionError, match="logits: "):
        check_bound(logits, t["logits"], t["bound_logits"], "logits")
    ok = torch.ones(P, dtype=torch.bool)
    ok[5] = False
    check_bound(logits[ok], t["logits"][ok], t["bound_logits"][ok], "the other rows")


def test_tail_bound_is_small_next_to_the_outputs(case):
    """The derived bound is a statement about f32 arithmetic, not a tolerance: orders of magnitude below a bf16 step of the logits."""
    x, w = case
    _, t1, _, _ = R.emulate_f32(x, w, 0)
    t = R.tail_ref(t1, w["gamma"], w["beta"], w["eps"], w["w_out"], w["b_out"])
    assert float(t["bound_logits"].max()) < 2.0 ** -8 * float(t["logits"].abs().max()) / 16
    assert float(t["bound_prob"].max()) < 2.0 ** -8 / 16          # p (1 - p) <= 1 / 4 carries the logits' bound over
