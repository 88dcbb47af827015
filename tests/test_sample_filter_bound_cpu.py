"""Host proof of the rules of tests/sample_filter_ref.py (no GPU): an f32 emulation of the filtered pick's sequence -- the select on
f32 logits, 64-bit fixed-point masses, the two thresholds, the pick and the kept log-sum-exp -- run on the GPU tests' own inputs
is exact or acceptable at every pick, inside the 2 % near-tie cap, with scores at <= 0.5 of their bound; six wrong
implementations fall outside; and Gumbel-max over the kept set is the renormalised softmax."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sample_filter_ref as F  # noqa: E402
import sample_ref as S  # noqa: E402

BF16, F32 = torch.bfloat16, torch.float32


def _x32(A, W, bias):
    return A.float() @ W.float().t() + bias[None, :]                 # an f32 product in another summation order


def _outside(ref, tok, score, picks):
    _, near, wrong, _ = F.classify(ref, tok, score)
    return bool(wrong) or near > S.NEAR_TIE_CAP * picks


@pytest.mark.parametrize("dtype", [BF16, F32])
def test_emulation_of_the_device_sequence_passes_on_the_gpu_inputs(dtype):
    rows = 64
    A, W, bias = F.operands(rows, dtype, 100 + rows)
    x32 = _x32(A, W, bias)
    exact = near = total = 0
    worst = 0.0
    for top_k, top_p in F.FILTERS:
        base = S.sample_ref(A, W, bias, F.SEED, S.TAG0)
        for tag in (S.TAG0, S.TAG0 + 1):
            ref = F.filter_ref(A, W, bias, F.SEED, tag, top_k, top_p, base=base)
            if (top_k, top_p) == (0, 0.9):                              # the inputs have a body and a tail
                size = ref["keep"].sum(1)
                assert int(size.min()) >= 2 and int(size.max()) <= F.N // 2, (int(size.min()), int(size.max()))
            tok, score, _ = F.emulate(x32, F.SEED, tag, top_k, top_p)
            e, n, wrong, ratio = F.classify(ref, tok, score)
            assert not wrong, (top_k, top_p, tag, wrong[:4])
            assert ratio <= 0.5, (top_k, top_p, ratio)
            exact, near, total, worst = exact + e, near + n, total + rows, max(worst, ratio)
    print(f"{dtype}: {exact} exact, {near} near-ties of {total} picks; worst score ratio {worst:.3f}; E_MASS {F.e_mass(F.N):.2e}")
    assert near <= S.NEAR_TIE_CAP * total, (near, total)


def test_wrong_implementations_fall_outside():
    rows = 64
    A, W, bias = F.operands(rows, BF16, 100 + rows)
    x32 = _x32(A, W, bias)
    base = S.sample_ref(A, W, bias, F.SEED, S.TAG0)
    ref = F.filter_ref(A, W, bias, F.SEED, S.TAG0, 50, 0.9, base=base)
    ok = F.emulate(x32, F.SEED, S.TAG0, 50, 0.9)
    assert not _outside(ref, ok[0], ok[1], rows)
    # 1. top-k off by one (k + 1 and k - 1 columns), seen where top-k alone decides
    ref8 = F.filter_ref(A, W, bias, F.SEED, S.TAG0, 8, 1.0, base=base)
    for adj in (1, -1):
        tok, score, keep = F.emulate(x32, F.SEED, S.TAG0, 8, 1.0, k_adjust=adj)
        assert int(keep.sum(1).min()) == 8 + adj and _outside(ref8, tok, score, rows)
    # 2. top-p applied before top-k
    tok, score, _ = F.emulate(x32, F.SEED, S.TAG0, 50, 0.9, p_first=True)
    assert _outside(ref, tok, score, rows)
    # 3. the score not renormalised (log-sum-exp over the whole row)
    tok, score, _ = F.emulate(x32, F.SEED, S.TAG0, 50, 0.9, renorm=False)
    assert torch.equal(tok, ok[0]) and _outside(ref, tok, score, rows)
    # 4. the noise indexed without row0: rows 32 .. 63 of a batch drawn with the noise of rows 0 .. 31
    ref_r = F.filter_ref(A[:32], W, bias, F.SEED, S.TAG0, 50, 0.9, row0=32)
    good = F.emulate(x32[:32], F.SEED, S.TAG0, 50, 0.9, row0=32)
    assert not _outside(ref_r, good[0], good[1], 32)
    tok, score, _ = F.emulate(x32[:32], F.SEED, S.TAG0, 50, 0.9, row0=32, noise_row0=0)
    assert _outside(ref_r, tok, score, 32)


def test_strict_nucleus_rule_at_an_exact_boundary():
    """Logits 0, t, t with exp(t) = 1/2 and a tail without mass, top_p = 1/2: the mass above t EQUALS top_p S, so t is not kept;
    the rule A <= top_p S keeps it.  The boundary is exact in the reference (float64) and in the device's fixed point
    (q(t) = 2^31), where no bound is involved: the two rules are told apart by the kept set itself (between the bounds a column
    at the boundary is undecided by construction -- that is what U is for)."""
    t = -math.log(2.0)
    assert math.exp(t) == 0.5 and math.exp(-800.0) == 0.0
    x = torch.tensor([0.0, t, t] + [-800.0] * 13, dtype=torch.float64)
    assert F.kept_ref(x, 0, 0.5).tolist() == [True] + [False] * 15
    assert F.kept_ref(x, 0, 0.5, strict=False).tolist() == [True] * 3 + [False] * 13
    x32 = np.array([0.0, t, t] + [-100.0] * 13, dtype=np.float32)
    q = F.masses(x32, x32.max())
    assert [int(v) for v in q[:4]] == [1 << 32, 1 << 31, 1 << 31, 0]
    assert F.kept_f32(x32, 0, 0.5).tolist() == [True] + [False] * 15
    assert F.kept_f32(x32, 0, 0.5, strict=False).tolist() == [True] * 3 + [False] * 13
    # just inside: a top_p one f32 step above 1/2 keeps the pair under both rules
    up = float(np.nextafter(np.float32(0.5), np.float32(1.0)))
    assert F.kept_f32(x32, 0, up).tolist() == [True] * 3 + [False] * 13 and F.kept_ref(x, 0, up).tolist() == [True] * 3 + [False] * 13


def test_dropped_threshold_ties_fall_outside():
    """top_k = 4 over rows whose 4th and 5th logits are bit-equal: the reference keeps five columns; an implementation that
    keeps exactly four never draws the later twin, which the near-tie cap then rejects over 64 tags."""
    good = bad = 0
    picks = 0
    twin_wins = 0
    for A1, W, bias, twins, _ in F.tied_operands(BF16):
        x32 = _x32(A1, W, bias)
        assert float(x32[0, twins[0]]) == float(x32[0, twins[1]])
        base = S.sample_ref(A1, W, bias, F.SEED, S.TAG0)
        for tag in range(S.TAG0, S.TAG0 + 64):
            ref = F.filter_ref(A1, W, bias, F.SEED, tag, 4, 1.0, base=base)
            assert int(ref["keep"].sum()) == 5
            twin_wins += int(ref["tok"][0]) == twins[1]
            for drop in (False, True):
                tok, score, keep = F.emulate(x32, F.SEED, tag, 4, 1.0, drop_ties=drop)
                assert int(keep.sum()) == (4 if drop else 5)
                _, near, wrong, _ = F.classify(ref, tok, score)
                assert not (wrong and not drop), wrong
                if drop:
                    bad += near + len(wrong)
                else:
                    good += near
            picks += 1
    print(f"ties: the later twin wins {twin_wins} of {picks} reference draws; near-ties or wrong: kept {good}, dropped {bad}")
    assert good <= S.NEAR_TIE_CAP * picks < bad, (good, bad, picks)


def test_gumbel_max_over_the_kept_set_is_the_renormalised_softmax():
    logits, keep, p = F.frequency_case()
    n = 4096
    assert int(keep.sum()) == 5 and float(p[keep].min()) * n > 20
    xs = logits.tolist()
    toks = []
    for step in range(n):
        g = S.gumbel_host_row(99, S.TAG0 + step, 24)
        y = [a + b if bool(k) else -math.inf for a, b, k in zip(xs, g, keep)]
        toks.append(y.index(max(y)))
    chi2 = F.chi_square(toks, keep, p, n)
    print(f"chi-square over the 5 kept cells, 4096 draws: {chi2:.2f} (critical {F.CHI2_CRIT_4DF} at 1e-4)")
    assert chi2 < F.CHI2_CRIT_4DF
    q = torch.softmax(logits, 0)                                        # not renormalised: rejected, the test has power
    assert sum((sum(1 for t in toks if t == i) - n * float(q[i])) ** 2 / (n * float(q[i])) for i in range(24) if bool(keep[i])) > F.CHI2_CRIT_4DF
