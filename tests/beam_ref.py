"""float64 reference of the candidate step of beam search (mvlt_gemm_beam_candidates) on top of sample_ref.sample_ref, whose x
and e_x it uses (temperature 1: x = A W^T + b), with the operands of sample_filter_ref.operands.

    lse_m = logsumexp_n x[m, n]        s[m, n] = x[m, n] - lse_m + beam_score[m]
    list of sample g = the n_cand largest s over its num_beams x N entries, descending, ties by the lower flat index beam N + n

Bound of one element (first order, constants from the kernel's own arithmetic, csrc/skinny.hip beam_candidates_kernel):
  x        e_x of sample_ref (the product, the bias add; the multiplication by inv_t = 1 is exact but stays in the estimate)
  lse      moves by at most the row's largest e_x, plus its f32 evaluation: every term expf(x - max) is off by at most
           (3 d + 4) 2^-24 relative, d = max - x (rounding of the difference, of d log2 e with a rounded constant, the ex2
           approximation: the derivation above E_MASS in csrc/skinny.hip), softmax-weighted mean of d <= ln N; the additions on the
           path of a term in the summation shape the kernel builds -- 1024 threads, a thread's columns t, t + 1024, ... go
           round-robin into four accumulators (ceil(ceil(N / 1024) / 4) additions), two to combine them, six levels of the wave's
           xor tree, 15 to add the 16 wave sums in order -- each 2^-24:
               lse_sum(N) = 3 ln N + 4 + ceil(ceil(N / 1024) / 4) + 23            (66 at N = 30522, 54 at N = 4106)
           then logf of the sum (E_LOG |lse - max|) and the addition of the maximum (2^-24 |lse|)
  s        the two roundings of (x - lse) + beam_score: 2^-24 |x - lse| + 2^-24 |s|
bound_s = SAFETY times the sum, as sample_ref.bound_lp (a correct kernel sits at <= 1/2; tests/test_beam_bound_cpu.py).

`classify` labels a returned list: exact (the reference list), near (a valid sorted top-n_cand once every score may move by its
bound: distinct in-range entries, no returned pair out of order by more than the sum of its bounds, no entry left out that beats
a returned one by more than the sum of theirs), wrong otherwise."""
import math

import numpy as np
import torch

import sample_filter_ref as F
import sample_ref as S
from gemm_ref import U32

NEAR_TIE_CAP = S.NEAR_TIE_CAP
THREADS = 1024                # BEAM_THREADS of the kernel
CASES = [(1, 1), (3, 2), (2, 5), (8, 8), (13, 5)]          # (G, num_beams); 13 x 5 = 65 rows crosses the 64-row chunk of the product
# operand seeds per case (bf16, f32), picked so that the reference alone leaves no list ambiguous (test_beam_bound_cpu.py)
SEEDS = {(1, 1): (101, 1101), (3, 2): (101, 1101), (2, 5): (101, 1101), (8, 8): (103, 1102), (13, 5): (106, 1104)}
# M = 40 rows of the real head, bf16.  20 x 2 and not 8 x 5: the product bound at K = 768 is 2.7e-3 against gaps of ~0.08 among the
# first 11 of 152,610 scores, which leaves every second list of 10 candidates ambiguous whatever the seed; lists of 4 are not
BIG = dict(G=20, num_beams=2, N=30522, K=768, seed=108)


def lse_sum(n):
    return 3.0 * math.log(n) + 4.0 + math.ceil(math.ceil(n / THREADS) / 4) + 23.0


def beam_scores(G, nb):
    """Descending negatives a few units apart, different per sample; the last beam of sample 0 sits at -1e9 (nb >= 2): the
    reference's way of switching a beam off (model.py:681-682)."""
    b = -(0.25 + 2.75 * torch.arange(nb, dtype=torch.float32)[None, :] + 0.375 * torch.arange(G, dtype=torch.float32)[:, None])
    if nb >= 2:
        b[0, nb - 1] = -1e9
    return b.reshape(-1).contiguous()


def case_operands(G, nb, dtype, big=False):
    if big:
        A, W, bias = F.operands(BIG["G"] * BIG["num_beams"], dtype, BIG["seed"], n=BIG["N"], k=BIG["K"])
        return A, W, bias, beam_scores(BIG["G"], BIG["num_beams"])
    A, W, bias = F.operands(G * nb, dtype, SEEDS[(G, nb)][1 if dtype == torch.float32 else 0])
    return A, W, bias, beam_scores(G, nb)


def beam_ref(A, W, bias, bs, nb, n_cand):
    """A [M, K], W [N, K], bias f32 [N] or None, bs f32 [M] -> dict: s, bound_s [M, N] float64; lse [M]; flat [G, n_cand] int64
    (beam N + tok), score [G, n_cand]."""
    base = S.sample_ref(A, W, bias, 0, 0)
    x, e_x = base["x"], base["e_x"]
    M, N = x.shape
    lse = torch.logsumexp(x, 1)
    d = x - lse[:, None]
    s = d + bs.double()[:, None]
    xmax = x.max(1).values
    e_lse = lse_sum(N) * U32 + S.E_LOG * (lse - xmax).abs() + U32 * lse.abs()
    bound_s = S.SAFETY * (e_x + e_x.max(1).values[:, None] + e_lse[:, None] + U32 * d.abs() + U32 * s.abs())
    G = M // nb
    sg = s.view(G, nb * N)
    order = torch.sort(sg, dim=1, descending=True, stable=True).indices[:, :n_cand + 1]
    return dict(s=s, bound_s=bound_s, lse=lse, flat=order[:, :n_cand].contiguous(), score=sg.gather(1, order[:, :n_cand]),
                next=order, nb=nb, n_cand=n_cand, N=N, G=G)


def ambiguous(ref):
    """bool [G]: a gap among the first n_cand + 1 sorted reference scores is below the sum of the two bounds."""
    G, N, nb = ref["G"], ref["N"], ref["nb"]
    sg, bg = ref["s"].view(G, nb * N), ref["bound_s"].view(G, nb * N)
    o = ref["next"]
    sv, bv = sg.gather(1, o), bg.gather(1, o)
    return ((sv[:, :-1] - sv[:, 1:]) < (bv[:, :-1] + bv[:, 1:])).any(1)


def classify(ref, beam, tok, score):
    """beam, tok int [G, n_cand], score f32 [G, n_cand] -> (exact, near, wrong [(sample, why)], worst score ratio)."""
    G, N, nb, n = ref["G"], ref["N"], ref["nb"], ref["n_cand"]
    beam, tok, score = beam.cpu().long(), tok.cpu().long(), score.cpu().double()
    sg, bg = ref["s"].view(G, nb * N), ref["bound_s"].view(G, nb * N)
    exact = near = 0
    wrong = []
    worst = 0.0
    for g in range(G):
        if bool(((beam[g] < 0) | (beam[g] >= nb) | (tok[g] < 0) | (tok[g] >= N)).any()):
            wrong.append((g, "out of range"))
            continue
        flat = beam[g] * N + tok[g]
        sv, bv = sg[g, flat], bg[g, flat]
        ratio = float(((score[g] - sv).abs() / bv).max()) if bool(torch.isfinite(score[g]).all()) else math.inf
        worst = max(worst, ratio)
        if ratio > 1.0:
            wrong.append((g, f"score off by {ratio:.2f} bounds"))
            continue
        if torch.equal(flat, ref["flat"][g]):
            exact += 1
            continue
        if flat.unique().numel() != n:
            wrong.append((g, "an entry twice"))
            continue
        if bool(((sv[:-1] + bv[:-1]) < (sv[1:] - bv[1:])).any()):
            wrong.append((g, "not sorted"))
            continue
        rest_lo = (sg[g] - bg[g]).clone()
        rest_lo[flat] = -math.inf
        if float((sv + bv).min()) < float(rest_lo.max()):
            wrong.append((g, f"a larger entry left out: {int(rest_lo.argmax())}"))
            continue
        near += 1
    return exact, near, wrong, worst


def assert_lists(ref, beam, tok, score, what, extra=0):
    exact, near, wrong, worst = classify(ref, beam, tok, score)
    msg = f"{what}: {exact} exact, {near} near, {len(wrong)} wrong of {ref['G']} lists, worst score ratio {worst:.3f}; wrong: {wrong[:4]}"
    print(msg)
    assert not wrong and near <= NEAR_TIE_CAP * ref["G"] + extra, msg
    return exact, near, worst


# ------------------------------------------------------------------------------------------------ the device's sequence
def lse_f32(x32):
    """The kernel's log-sum-exp of f32 rows [M, N] (numpy f32 in, f32 [M] out): row maximum, expf of the rounded difference, the
    fixed summation shape, logf, the addition of the maximum."""
    M, N = x32.shape
    J = (N + THREADS - 1) // THREADS
    xm = x32.max(1)
    e = np.zeros((M, J * THREADS), dtype=np.float32)
    e[:, :N] = np.exp((x32 - xm[:, None]).astype(np.float32), dtype=np.float32)
    e = e.reshape(M, J, THREADS)
    acc = np.zeros((M, 4, THREADS), dtype=np.float32)
    for j in range(J):
        acc[:, j & 3] = acc[:, j & 3] + e[:, j]
    v = (acc[:, 0] + acc[:, 1]) + (acc[:, 2] + acc[:, 3])                    # [M, 1024]: thread t = 64 wave + lane
    v = v.reshape(M, 16, 64)
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[:, :, lane ^ o]
    tot = v[:, 0, 0].copy()
    for w in range(1, 16):
        tot = tot + v[:, w, 0]
    return (xm + np.log(tot, dtype=np.float32)).astype(np.float32)


def emulate(x32, bs, nb, n_cand, lse_over_sample=False, no_beam_score=False):
    """f32 logits [M, N] (torch) and beam scores -> (beam, tok int64 [G, n_cand], score f32 [G, n_cand]) in the kernel's
    arithmetic.  The keyword arguments are the WRONG implementations of the CPU test."""
    xn = x32.numpy()
    M, N = xn.shape
    G = M // nb
    lse = lse_f32(xn)
    if lse_over_sample:
        lse = np.repeat(torch.logsumexp(x32.double().view(G, nb * N), 1).float().numpy(), nb)
    b = np.zeros(M, dtype=np.float32) if no_beam_score else bs.numpy().astype(np.float32)
    s = ((xn - lse[:, None]).astype(np.float32) + b[:, None]).astype(np.float32)
    sg = torch.from_numpy(s).view(G, nb * N)
    o = torch.sort(sg, dim=1, descending=True, stable=True).indices[:, :n_cand]
    return o // N, o % N, sg.gather(1, o)
