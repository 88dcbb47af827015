"""Host proof of the bounds of tests/sample_ref.py (no GPU): an f32 emulation of the sampled pick's epilogue stays inside them
at a ratio <= 0.5, five ways of getting the epilogue wrong fall outside, and Gumbel-max with the host's noise is the softmax."""
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sample_ref as S  # noqa: E402
from gemm_ref import check_bound  # noqa: E402

V, VPAD, K = 30522, 30528, 768


def test_noise_bound_holds_for_every_u01():
    """All 2^24 values of u >> 8: the kernel's f32 sequence (h + l split, two logs) against -log(-log(u01)) in float64.
    numpy's f32 log is correctly rounded to <= 1 ulp where the bound allows the device's logf 2, so the ratio must be <= 0.5;
    the naive fl(k + 0.5) 2^-24 (u01 = 1 at the top) is rejected."""
    worst, naive_bad = 0.0, 0
    for lo in range(0, 1 << 24, 1 << 22):
        k = np.arange(lo, lo + (1 << 22), dtype=np.uint32)
        g = -np.log(-np.log((k.astype(np.float64) + 0.5) * 2.0 ** -24))
        bound = S.E_LOG * (3.0 + np.abs(g)) * (1.0 + 2.0 ** -10)
        got = S.gumbel_f32(k).astype(np.float64)
        assert np.isfinite(got).all()
        worst = max(worst, float((np.abs(got - g) / bound).max()))
        with np.errstate(divide="ignore"):
            u = (k.astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -24)
            naive = -np.log(-np.log(u, dtype=np.float32), dtype=np.float32).astype(np.float64)
        naive_bad += int((~(np.abs(naive - g) <= bound)).sum())
    print(f"noise: worst |g_f32 - g| / e_g over 2^24 values = {worst:.3f}; naive u01 outside the bound at {naive_bad} values")
    assert worst <= 0.5, worst
    assert naive_bad > 1000, naive_bad
    g_lo, g_hi = -math.log(-math.log(0.5 * 2.0 ** -24)), -math.log(-math.log(1.0 - 2.0 ** -25))
    assert -2.86 < g_lo < -2.85 and 17.32 < g_hi < 17.34


def _operands(M, seed):
    """Inputs of the kind the GPU test uses: A ~ N(0, 1), W ~ N(0, 9 / K) rounded to bf16 (logit std 3), bias ~ N(0, 0.01);
    the rows of W beyond the vocabulary hold NaN."""
    gen = torch.Generator().manual_seed(seed)
    A = torch.randn(M, K, generator=gen).bfloat16()
    W = torch.full((VPAD, K), math.nan).bfloat16()
    W[:V] = (torch.randn(V, K, generator=gen) * (3.0 / math.sqrt(K))).bfloat16()
    bias = torch.randn(V, generator=gen) * 0.1
    return A, W, bias


def _ratio(out, ref, bound):
    out = out.double()
    r = torch.where(torch.isfinite(out), (out - ref).abs() / bound, torch.full_like(ref, math.inf))
    return float(r.max())


def test_whole_epilogue_bound_accepts_f32_and_rejects_damage():
    M, seed, tag = 64, 0x1234567890ABCDEF, S.TAG0 + 3
    A, W, bias = _operands(M, 5)
    ref = S.sample_ref(A, W[:V], bias, seed, tag, 1.0)
    x32 = A.float() @ W[:V].float().t() + bias[None, :]                 # an f32 product in another summation order
    g32, y32, tok, lp = S.emulate_f32(x32, seed, tag, V)
    r_y, r_lp = _ratio(y32, ref["y"], ref["bound_y"]), _ratio(lp, ref["logprob"], ref["bound_lp"](tok))
    r_g = _ratio(g32, ref["g"], ref["e_g"])
    exact, near = S.assert_picks(tok, ref["y"], ref["bound_y"], "f32 emulation")
    print(f"emulation: y ratio {r_y:.3f}, logprob ratio {r_lp:.3f}, noise ratio {r_g:.3f}; picks {exact} exact / {near} near-ties; "
          f"mean bound_y {float(ref['bound_y'].mean()):.2e}, mean top prob {float(torch.exp(ref['x'].max(1).values - ref['lse']).mean()):.3f}")
    assert r_y <= 0.5 and r_lp <= 0.5 and r_g <= 0.5, (r_y, r_lp, r_g)

    def rejected_picks(t):
        _, near, bad = S.classify_picks(t, ref["y"], ref["bound_y"])
        return bool(bad) or near > S.NEAR_TIE_CAP * M

    # 1. the noise of the wrong step (tag off by one)
    g_w, y_w, tok_w, _ = S.emulate_f32(x32, seed, tag + 1, V)
    assert _ratio(g_w, ref["g"], ref["e_g"]) > 1.0 and _ratio(y_w, ref["y"], ref["bound_y"]) > 1.0 and rejected_picks(tok_w)
    # 2. the noise indexed with the padded width 30528 instead of N
    idx = (torch.arange(M)[:, None] * VPAD + torch.arange(V)[None, :]).reshape(-1)
    k = (S.rng_u32(seed, tag, idx) >> 8).numpy().astype(np.uint32)
    g_p = torch.from_numpy(S.gumbel_f32(k)).view(M, V)
    assert _ratio(g_p, ref["g"], ref["e_g"]) > 1.0 and rejected_picks((x32 + g_p).argmax(1))
    assert _ratio(g_p[:1], ref["g"][:1], ref["e_g"][:1]) <= 0.5          # (row 0 is the same either way: the test needs M > 1)
    # 3. the pick taken over x instead of y
    assert rejected_picks(x32.argmax(1))
    # 4. a log-sum-exp that includes the 6 padding columns (NaN rows of W, as in the GPU test; and rows that hold real weights)
    for fill in (math.nan, None):
        Wp = W.clone()
        if fill is None:
            Wp[V:] = W[ref["tok"][:VPAD - V]]                             # copies of rows that won a draw: real mass
        xpad = torch.cat([x32, A.float() @ Wp[V:].float().t()], 1)
        lse_bad = torch.logsumexp(xpad, 1)
        lp_bad = x32.gather(1, tok.view(-1, 1)).squeeze(1) - lse_bad
        assert _ratio(lp_bad, ref["logprob"], ref["bound_lp"](tok)) > 1.0
    # 5. the score is the perturbed y instead of x - lse
    assert _ratio(y32.gather(1, tok.view(-1, 1)).squeeze(1), ref["logprob"], ref["bound_lp"](tok)) > 1.0
    # and check_bound names such damage element by element
    try:
        check_bound(y_w, ref["y"], ref["bound_y"], "wrong step")
    except AssertionError as e:
        assert "outside the bound" in str(e)
    else:
        raise AssertionError("check_bound accepted the noise of the wrong step")


def test_temperature_enters_before_the_noise():
    A, W, bias = _operands(8, 6)
    for T in (0.5, 2.0):
        ref = S.sample_ref(A, W[:V], bias, 7, S.TAG0, T)
        it = torch.tensor(S.inv_t_f32(T), dtype=torch.float32)
        x32 = (A.float() @ W[:V].float().t() + bias[None, :]) * it
        _, y32, tok, lp = S.emulate_f32(x32, 7, S.TAG0, V)
        assert _ratio(y32, ref["y"], ref["bound_y"]) <= 0.5 and _ratio(lp, ref["logprob"], ref["bound_lp"](tok)) <= 0.5
        # scaling y instead of x (noise divided by T as well) is outside
        y_bad = (A.float() @ W[:V].float().t() + bias[None, :] + S.emulate_f32(x32, 7, S.TAG0, V)[0]) * it
        assert _ratio(y_bad, ref["y"], ref["bound_y"]) > 1.0


def test_gumbel_max_with_host_noise_is_the_softmax():
    """A fixed 16-entry logit row, 2^16 steps (tags) of host noise: the argmax counts against softmax(logits), chi-square
    goodness of fit with 15 degrees of freedom at significance 1e-4 (critical value 44.26).  A property of the host port:
    it pins the u01 construction (a 23-bit or one-sided u01, or log in place of -log(-log), fails it)."""
    gen = torch.Generator().manual_seed(3)
    logits = (torch.randn(16, generator=gen) * 1.5).double()
    p = torch.softmax(logits, 0)
    n = 1 << 16
    assert float(p.min()) * n > 20
    counts = [0] * 16
    xs = logits.tolist()
    for step in range(n):
        g = S.gumbel_host_row(99, S.TAG0 + step, 16)
        y = [a + b for a, b in zip(xs, g)]
        counts[y.index(max(y))] += 1
    chi2 = sum((c - n * float(q)) ** 2 / (n * float(q)) for c, q in zip(counts, p))
    print(f"chi-square over 16 cells, 2^16 draws: {chi2:.2f} (critical 44.26 at 1e-4)")
    assert chi2 < 44.26, (chi2, counts)
    # the same draws counted against a wrong law (logits / 2) are rejected: the test has power
    q = torch.softmax(logits / 2, 0)
    assert sum((c - n * float(v)) ** 2 / (n * float(v)) for c, v in zip(counts, q)) > 44.26
