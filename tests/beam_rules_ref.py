"""float64 reference of the rule-aware candidate step of beam search (mvlt_beam_rules_plan + mvlt_gemm_beam_candidates_rules), on
top of beam_ref.beam_ref (lse, the summation constant, the f32 log-sum-exp of the emulation) and logit_rules_ref.sets (the two sets).

HF 4.16 beam_search hands its processors the LOG-PROBABILITIES, before the beam score is added:

    lp = x - lse_m (lse over all N columns, unprocessed)      seen(n):  lp' = lp < 0 ? lp p : lp / p  (p = the f32 penalty, once)
    s  = lp' + beam_score[m]                                  banned(n): never listed, changes nothing else
    list of sample g = the n_cand largest s over its UNBANNED entries, descending, ties by the lower flat index beam N + n;
    fewer than n_cand unbanned entries: the remaining slots are (-inf, beam 0, token 0)

Bound of one element (first order, in the style of logit_rules_ref.processed):
  lp       beam_ref's bound of x - lse: e_x + the row's largest e_x + e_lse + 2^-24 |lp|
  lp'      seen: the bound of lp times max(p, 1 / p), plus one more f32 rounding 2^-24 |lp'|
  s        plus the rounding of the final add, 2^-24 |s|
bound_s = SAFETY times the sum.  With every rule off this is beam_ref's s and bound_s, bit for bit (test_beam_rules_cpu.py).

`classify` is beam_ref.classify with two more rules: a banned entry in a list is wrong whatever its score, and the slots a sample
has no unbanned entry for must hold the fill."""
import math

import numpy as np
import torch

import beam_ref as B
import logit_rules_ref as LR
import sample_filter_ref as F
import sample_ref as S
from gemm_ref import U32

NEAR_TIE_CAP = S.NEAR_TIE_CAP
EOS = LR.EOS
C_HIST = 12                   # tokens in the histories of the bounded tests
# operand seeds per case of beam_ref.CASES (bf16, f32): the first at or after beam_ref.SEEDS for which the reference alone leaves no
# list ambiguous, with the rules off and under every set of logit_rules_ref.RULE_SETS at c = 12 and c = 0 (test_beam_rules_cpu.py)
SEEDS = {(1, 1): (101, 1101), (3, 2): (101, 1101), (2, 5): (101, 1101), (8, 8): (103, 1114), (13, 5): (126, 1107)}


def p32(penalty):
    return float(np.float32(penalty))


def case_operands(G, nb, dtype, big=False):
    """beam_ref.case_operands with the seeds above (the real-size case keeps beam_ref.BIG)."""
    if big:
        return B.case_operands(G, nb, dtype, big=True)
    A, W, bias = F.operands(G * nb, dtype, SEEDS[(G, nb)][1 if dtype == torch.float32 else 0])
    return A, W, bias, B.beam_scores(G, nb)


def histories(ref0, c=C_HIST, seed=11):
    """int64 [M, c] for a beam_ref result `ref0` (rules off): row m = beam b of sample g gets [q, a, q, s, z, q, a, z, q, s, z, q]
    with a, s = the first two tokens of the sample's unprocessed candidate list that belong to beam b (rows the list does not
    reach: the row's own two largest scores) and q, z two other tokens -- a and s are seen (penalised), follow q (banned at g = 2)
    and follow (z, q) (banned at g = 3), so every rule set changes the sample's list."""
    G, nb, N = ref0["G"], ref0["nb"], ref0["N"]
    if c == 0:
        return torch.zeros((G * nb, 0), dtype=torch.int64)
    assert c == C_HIST
    gen = torch.Generator().manual_seed(seed)
    rows = []
    for m in range(G * nb):
        g, b = divmod(m, nb)
        toks = [int(f) % N for f in ref0["flat"][g] if int(f) // N == b]
        for t in torch.topk(ref0["s"][m], 2).indices.tolist():
            if t not in toks:
                toks.append(t)
        a, s = toks[0], toks[1]
        while True:
            q, z = (int(v) for v in torch.randint(0, N, (2,), generator=gen))
            if len({q, z, a, s, EOS}) == 5:
                break
        rows.append([q, a, q, s, z, q, a, z, q, s, z, q])
    return torch.tensor(rows, dtype=torch.int64)


def beam_rules_ref(A, W, bias, bs, nb, n_cand, history, penalty=1.0, ngram=0, min_length=0, eos=None, ref0=None, base=None):
    """A [M, K], W [N, K], bias f32 [N] or None, bs f32 [M], history int64 [M, c] -> the dict of beam_ref.beam_ref for the
    processed scores, plus banned / seen [M, N] and valid [G] (listed entries per sample; flat is -1 behind them).  `ref0`: the
    beam_ref result of the same operands, when the caller has it (not changed)."""
    base = S.sample_ref(A, W, bias, 0, 0) if base is None else base          # (the caller's, when it has one: not changed)
    x, e_x = base["x"], base["e_x"]
    M, N = x.shape
    G = M // nb
    p = p32(penalty)
    lse = torch.logsumexp(x, 1) if ref0 is None else ref0["lse"]
    d = x - lse[:, None]
    e_lse = B.lse_sum(N) * U32 + S.E_LOG * (lse - x.max(1).values).abs() + U32 * lse.abs()
    e_lp = e_x + e_x.max(1).values[:, None] + e_lse[:, None] + U32 * d.abs()
    seen, banned = LR.sets(history, N, ngram, min_length, eos)
    lp = torch.where(seen, torch.where(d < 0, d * p, d / p), d)
    e_lp = torch.where(seen, e_lp * max(p, 1.0 / p) + U32 * lp.abs(), e_lp) if p != 1.0 else e_lp
    s = lp + bs.double()[:, None]
    bound_s = S.SAFETY * (e_lp + U32 * s.abs())
    sel = torch.where(banned, torch.full_like(s, -math.inf), s).view(G, nb * N)
    take = min(n_cand + 1, nb * N)
    order = torch.sort(sel, dim=1, descending=True, stable=True).indices[:, :take]
    valid = (~banned).view(G, nb * N).sum(1).clamp(max=n_cand)
    order = torch.where(torch.arange(take)[None, :] < (~banned).view(G, nb * N).sum(1)[:, None], order, torch.full_like(order, -1))
    flat = order[:, :n_cand].contiguous()
    if flat.shape[1] < n_cand:
        flat = torch.cat([flat, torch.full((G, n_cand - flat.shape[1]), -1, dtype=torch.int64)], 1)
    return dict(s=s, bound_s=bound_s, lse=lse, flat=flat, next=order, banned=banned, seen=seen, valid=valid, nb=nb, n_cand=n_cand,
                N=N, G=G)


def ambiguous(ref):
    """bool [G]: a gap among the first n_cand + 1 sorted unbanned reference scores is below the sum of the two bounds."""
    G, N, nb = ref["G"], ref["N"], ref["nb"]
    sg, bg = ref["s"].view(G, nb * N), ref["bound_s"].view(G, nb * N)
    o = ref["next"]
    ok = o >= 0
    sv, bv = sg.gather(1, o.clamp(min=0)), bg.gather(1, o.clamp(min=0))
    return (((sv[:, :-1] - sv[:, 1:]) < (bv[:, :-1] + bv[:, 1:])) & ok[:, :-1] & ok[:, 1:]).any(1)


def classify(ref, beam, tok, score):
    """beam, tok int [G, n_cand], score f32 [G, n_cand] -> (exact, near, wrong [(sample, why)], worst score ratio).  Never accepts
    a banned entry; the slots behind a sample's `valid` entries must be (-inf, 0, 0)."""
    G, N, nb, n = ref["G"], ref["N"], ref["nb"], ref["n_cand"]
    beam, tok, score = beam.cpu().long(), tok.cpu().long(), score.cpu().double()
    sg, bg, ban = ref["s"].view(G, nb * N), ref["bound_s"].view(G, nb * N), ref["banned"].view(G, nb * N)
    exact = near = 0
    wrong = []
    worst = 0.0
    for g in range(G):
        k = int(ref["valid"][g])
        if bool(((beam[g] < 0) | (beam[g] >= nb) | (tok[g] < 0) | (tok[g] >= N)).any()):
            wrong.append((g, "out of range"))
            continue
        if k < n and not (bool((score[g, k:] == -math.inf).all()) and not bool(beam[g, k:].any()) and not bool(tok[g, k:].any())):
            wrong.append((g, "the empty slots do not hold (-inf, 0, 0)"))
            continue
        flat = (beam[g] * N + tok[g])[:k]
        if bool(ban[g, flat].any()):
            wrong.append((g, f"a banned entry: {flat[ban[g, flat]].tolist()}"))
            continue
        sv, bv = sg[g, flat], bg[g, flat]
        ratio = 0.0 if k == 0 else float(((score[g, :k] - sv).abs() / bv).max()) if bool(torch.isfinite(score[g, :k]).all()) else math.inf
        worst = max(worst, ratio)
        if ratio > 1.0:
            wrong.append((g, f"score off by {ratio:.2f} bounds"))
            continue
        if torch.equal(flat, ref["flat"][g, :k]):
            exact += 1
            continue
        if flat.unique().numel() != k:
            wrong.append((g, "an entry twice"))
            continue
        if bool(((sv[:-1] + bv[:-1]) < (sv[1:] - bv[1:])).any()):
            wrong.append((g, "not sorted"))
            continue
        rest_lo = (sg[g] - bg[g]).clone()
        rest_lo[flat] = -math.inf
        rest_lo[ban[g]] = -math.inf
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
WRONG = ("on_logits", "per_occurrence", "lse_without_banned", "pre_reorder")


def _penalise32(v, p):
    return np.where(v < 0, (v * p).astype(np.float32), (v / p).astype(np.float32)).astype(np.float32)


def emulate(x32, bs, nb, n_cand, history, penalty=1.0, ngram=0, min_length=0, eos=None, wrong=None):
    """f32 logits [M, N] (torch), beam scores and histories -> (beam, tok int64 [G, n_cand], score f32 [G, n_cand]) in the kernel's
    arithmetic.  `wrong` selects one of the WRONG implementations of the CPU test:
      on_logits            the greedy placement: the rules on the raw logits, ahead of the softmax (a banned column leaves it)
      per_occurrence       the penalty once per occurrence of a token in the history
      lse_without_banned   banned columns taken out of the log-sum-exp
      pre_reorder          row m reads the history of its neighbour in the sample: the parent's sibling, before the reorder"""
    assert wrong is None or wrong in WRONG
    xn = x32.numpy().astype(np.float32)
    M, N = xn.shape
    G = M // nb
    p = np.float32(penalty)
    if wrong == "pre_reorder":
        idx = torch.arange(M).view(G, nb).roll(1, dims=1).reshape(-1)
        history = history[idx]
    seen, banned = (v.numpy() for v in LR.sets(history, N, ngram, min_length, eos))
    times = np.zeros((M, N), dtype=np.int64)
    for m in range(M):
        for t in history[m].tolist():
            if 0 <= t < N:
                times[m, t] += 1
    b = bs.numpy().astype(np.float32)
    if wrong == "on_logits":
        xp = np.where(seen, _penalise32(xn, p), xn).astype(np.float32)
        xp = np.where(banned, np.float32(-np.inf), xp).astype(np.float32)
        lp = (xp - B.lse_f32(xp)[:, None]).astype(np.float32)
    else:
        lse = B.lse_f32(np.where(banned, np.float32(-np.inf), xn).astype(np.float32)) if wrong == "lse_without_banned" else B.lse_f32(xn)
        lp = (xn - lse[:, None]).astype(np.float32)
        if wrong == "per_occurrence":
            for _ in range(int(times.max())):
                lp = np.where(times > 0, _penalise32(lp, p), lp).astype(np.float32)
                times = times - 1
        else:
            lp = np.where(seen, _penalise32(lp, p), lp).astype(np.float32)
    s = (lp + b[:, None]).astype(np.float32)
    sel = torch.from_numpy(np.where(banned, np.float32(-np.inf), s).astype(np.float32)).view(G, nb * N)
    o = torch.sort(sel, dim=1, descending=True, stable=True).indices[:, :n_cand]
    score = sel.gather(1, o)
    left = torch.from_numpy(~banned).view(G, nb * N).sum(1)
    empty = torch.arange(n_cand)[None, :] >= left[:, None]
    o = torch.where(empty, torch.zeros_like(o), o)
    return o // N, o % N, torch.where(empty, torch.full_like(score, -math.inf), score)
