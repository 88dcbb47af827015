"""References for the retrieval path: recall ranks in plain numpy, and a float64 reference of mvlt_retrieval_head with the bounds
its outputs are held to (written from the rules of include/mvlt_hip.h, stage by stage, each from the kernel's own stored input).

Ranks.  Order of a line: the stable ascending sort reversed, i.e. (score, index) lexicographic with the higher index first among
equal scores; NaN is smaller than every number.  rank = the number of entries that sort before the line's best match, the line's
length when nothing matches.  ``rank_line`` states that directly; ``rank_line_argsort`` is np.argsort(kind="stable")[::-1] with the
position of the first match (no NaN: numpy sorts NaN last).

Head.  pooled and t1 are products with an activation, rounded once to bf16:
    pooled: v = x Wp^T + bp with gemm_ref's error e_v before the output rounding; tanh has Lipschitz constant 1, so
            |pooled - tanh(v)| <= e_v + E_ACT |tanh v| + U_BF16 |tanh v|      (E_ACT = 4 * 2^-24: tanhf in f32)
    t1:     gemm_ref(pooled, Wt, bias=bt, gelu=True) and its bound, unchanged.
The f32 tail, from the stored t1 (exact in float64), u = 2^-24.  Every sum of the kernel is over H terms and a term passes through
at most DEPTH additions (4 per 4-column group, at most 4 groups per lane, 6 butterfly levels, 2 to spare for the bias and a
division): a sum's error is at most DEPTH u sum|terms| (first order), which covers ANY order of that depth:
    mean   e_m  = DEPTH u sum|t| / H + u |mean|
    d_n = t_n - mean                       e_d  = e_m + u |d_n|
    var = sum d^2 / H                      e_v  = (sum (2 |d| e_d + u d^2) + DEPTH u sum d^2) / H + u var
    r = 1 / sqrt(var + eps)                e_r  = r (e_v + u (var + eps)) / (2 (var + eps)) + 4 u r      (rounded sum, sqrt, divide)
    y_n = d_n r gamma_n + beta_n           e_y  = |gamma| (e_d r + |d| e_r) + 3 u |d r gamma| + u |y|
    l_c = sum y_n w_cn + b_c               e_l  = sum (e_y |w| + u |y w|) + DEPTH u sum |y w| + 2 u |l_c|
    p = e_1 / (e_0 + e_1) = sigmoid(l_1 - l_0), |dp/dl| = p (1 - p):
                                           e_p  = p (1 - p) (e_l0 + e_l1 + 2 u |l_1 - l_0|) + E_SOFT u p   (two expf, a sum, a divide)
bound = SAFETY x the first-order value, SAFETY = 2 as in head_ce_ref / sample_ref."""
import math

import numpy as np
import torch

from gemm_ref import U32, U_BF16, gemm_ref, logical
from sample_ref import SAFETY

E_ACT = 4.0 * U32
E_SOFT = 8.0
DEPTH = 24
RB = 16                       # rows a workgroup of csrc/retrieval.hip owns


# ------------------------------------------------------------------------------------------------ ranks
def _key(s, idx):
    s = float(s)
    return (0, 0.0, idx) if math.isnan(s) else (1, s, idx)


def rank_line(sim, match):
    """sim: 1-D scores, match: 1-D bools -> the rank of the line by the rule above (plain Python on purpose)."""
    n = len(sim)
    best = None
    for j in range(n):
        if match[j] and (best is None or _key(sim[j], j) > best):
            best = _key(sim[j], j)
    if best is None:
        return n
    return sum(1 for j in range(n) if _key(sim[j], j) > best)


def rank_line_argsort(sim, match):
    inds = np.argsort(np.asarray(sim), kind="stable")[::-1]
    for r, ind in enumerate(inds):
        if match[ind]:
            return r
    return len(sim)


def recall_ranks_ref(scores, image_group, caption_group):
    """(i2t [Ni], t2i [Nc]) int arrays for a numpy score matrix and integer group ids."""
    s = np.asarray(scores)
    ig, cg = np.asarray(image_group), np.asarray(caption_group)
    i2t = [rank_line(s[i], cg == ig[i]) for i in range(s.shape[0])]
    t2i = [rank_line(s[:, j], ig == cg[j]) for j in range(s.shape[1])]
    return np.array(i2t, dtype=np.int64), np.array(t2i, dtype=np.int64)


def recalls_ref(i2t, t2i, ks=(1, 5, 10)):
    return {"i2t_retrieval": {f"R@{k}": float((np.asarray(i2t) < k).sum()) / len(i2t) for k in ks},
            "t2i_retrieval": {f"R@{k}": float((np.asarray(t2i) < k).sum()) / len(t2i) for k in ks}}


def rank_case(Ni, Nc, seed):
    """A score matrix with everything the rule has to decide: duplicated groups, a row and a column without a match, exact ties
    between a match and non-matches on both sides of it, one NaN, a -0 / +0 pair.  Scores are quantised (bf16-like ties)."""
    g = np.random.default_rng(seed)
    s = (g.integers(0, 40, size=(Ni, Nc)) / 64.0).astype(np.float32)
    ngrp = max(1, min(Ni, Nc) // 2)
    ig = g.integers(0, ngrp, size=Ni).astype(np.int64)
    cg = g.integers(0, ngrp, size=Nc).astype(np.int64)
    if Ni > 2 and Nc > 2:
        ig[1] = 10 ** 12 + 7            # a row without a match (ids beyond 32 bits)
        cg[2] = -5                      # a column without a match
        i, j = 0, Nc // 2               # row 0: its match at j ties with non-matches on both sides
        cg[:] = np.where(cg == ig[i], ngrp + 1, cg)
        cg[j] = ig[i]
        s[i, :] = np.minimum(s[i, :], 0.25)
        s[i, j] = s[i, 0] = s[i, Nc - 1] = 0.5
        s[i, 1] = -0.0
        jj, ii = Nc - 2, Ni // 2        # the last column but one likewise, down the rows (a group of its own: rows 0 and 1 keep theirs)
        if Ni > 4:
            cg[jj] = ig[ii] = ngrp + 3
            s[:, jj] = np.minimum(s[:, jj], 0.25)
            s[ii, jj] = s[0, jj] = s[Ni - 1, jj] = 0.375
        s[Ni - 1, 1] = np.nan
    return s, ig, cg


# ------------------------------------------------------------------------------------------------ head
def head_operands(H, P, seed):
    """Packed hidden rows [R, H] (bf16) with the [CLS] rows of P pairs at irregular offsets -- every other row is poison, so a wrong
    gather shows --, the head's weights, and out_index: a permutation of the pairs over every second slot of a longer buffer."""
    g = torch.Generator().manual_seed(seed)
    lens = torch.tensor([3 + (7 * p + seed) % 11 for p in range(P)], dtype=torch.int32)
    row_start = (torch.cumsum(lens, 0) - lens).to(torch.int32)
    R = int(lens.sum()) + 5
    hidden = torch.full((R, H), 3.0e4, dtype=torch.bfloat16)
    hidden[row_start.long()] = (torch.rand(P, H, generator=g) * 2 - 1).to(torch.bfloat16)
    u = lambda *shape: torch.rand(*shape, generator=g) * 2 - 1
    s = 3.0 / math.sqrt(H)
    w = dict(w_pool=(u(H, H) * s).to(torch.bfloat16), b_pool=u(H) * 0.5, w_tr=(u(H, H) * s).to(torch.bfloat16), b_tr=u(H) * 0.5,
             gamma=1.0 + 0.2 * u(H), beta=0.1 * u(H), eps=1e-12, w_out=(u(2, H) * 2 * s).to(torch.bfloat16), b_out=u(2) * 0.5)
    out_index = (torch.randperm(P, generator=g) * 2 + 1).to(torch.int64)
    return hidden, row_start, w, out_index, 2 * P + 3


def pooled_ref(x, w_pool, b_pool):
    """x: the gathered [CLS] rows [P, H] (bf16) -> (ref, bound) float64."""
    a, b = logical(x, w_pool)
    v, _, bound_v, _, _ = gemm_ref(a, b, out_dtype=torch.bfloat16, bias=b_pool)
    e_v = bound_v - U_BF16 * v.abs()
    t = torch.tanh(v)
    return t, e_v + (E_ACT + U_BF16) * t.abs() + 1e-30


def t1_ref(pooled, w_tr, b_tr):
    """pooled: the kernel's own stored output [P, H] (bf16) -> (ref, bound) float64."""
    a, b = logical(pooled, w_tr)
    v, _, bound, _, _ = gemm_ref(a, b, out_dtype=torch.bfloat16, bias=b_tr, gelu=True)
    return v, bound


def tail_ref(t1, gamma, beta, eps, w_out, b_out):
    """t1: the kernel's own stored output [P, H] (bf16) -> dict of float64: logits, bound_logits [P, 2], prob, bound_prob [P]."""
    t = t1.double()
    H = t.shape[1]
    u = U32
    ga, be, w, bo = gamma.double(), beta.double(), w_out.double(), b_out.double()
    mean = t.mean(1, keepdim=True)
    e_m = DEPTH * u * t.abs().sum(1, keepdim=True) / H + u * mean.abs()
    d = t - mean
    e_d = e_m + u * d.abs()
    var = (d * d).mean(1, keepdim=True)
    e_v = ((2 * d.abs() * e_d + u * d * d).sum(1, keepdim=True) + DEPTH * u * (d * d).sum(1, keepdim=True)) / H + u * var
    r = 1.0 / torch.sqrt(var + eps)
    e_r = r * (e_v + u * (var + eps)) / (2 * (var + eps)) + 4 * u * r
    y = d * r * ga + be
    e_y = ga.abs() * (e_d * r + d.abs() * e_r) + 3 * u * (d * r * ga).abs() + u * y.abs()
    yw = y[:, None, :] * w[None, :, :]                                          # [P, 2, H]
    logits = yw.sum(2) + bo[None, :]
    e_l = (e_y[:, None, :] * w.abs()[None] + u * yw.abs()).sum(2) + DEPTH * u * yw.abs().sum(2) + 2 * u * logits.abs()
    z = logits[:, 1] - logits[:, 0]
    p = torch.sigmoid(z)
    e_p = p * (1 - p) * (e_l.sum(1) + 2 * u * z.abs()) + E_SOFT * u * p
    return dict(logits=logits, bound_logits=SAFETY * e_l + 1e-30, prob=p, bound_prob=SAFETY * e_p + 1e-30)


def softmax_ref(logits):
    """Class-1 probability from the kernel's own f32 logits [P, 2] -> (ref, bound) float64 (the last line of tail_ref alone)."""
    l = logits.double()
    z = l[:, 1] - l[:, 0]
    p = torch.sigmoid(z)
    return p, SAFETY * (p * (1 - p) * 2 * U32 * z.abs() + E_SOFT * U32 * p) + 1e-30


# ------------------------------------------------------------------------------------------------ f32 emulation (CPU proofs)
def _sum_f32(x, order):
    """Sum over the last dimension in f32 in one of three orders, each of depth <= DEPTH - 2."""
    H = x.shape[-1]
    if order == 0:
        return x.sum(-1, dtype=torch.float32)
    parts = x.reshape(*x.shape[:-1], H // 16, 16) if order == 1 else x.reshape(*x.shape[:-1], H // 64, 64).transpose(-1, -2)
    acc = parts[..., 0].clone()                        # order 1: 16 consecutive terms; order 2: lane-strided, H / 64 terms
    for i in range(1, parts.shape[-1]):
        acc = acc + parts[..., i]
    n = 1 << (acc.shape[-1] - 1).bit_length()
    acc = torch.nn.functional.pad(acc, (0, n - acc.shape[-1]))
    while acc.shape[-1] > 1:                           # tree over the partial sums (at most 64: depth 6)
        acc = acc[..., 0::2] + acc[..., 1::2]
    return acc[..., 0]


def _matmul_f32(a, w, order):
    a, w = a.float(), w.float()
    if order == 0:
        return a @ w.t()
    step = 32 if order == 1 else 128
    acc = torch.zeros(a.shape[0], w.shape[0])
    for k in range(0, a.shape[1], step):
        acc = acc + a[:, k:k + step] @ w[:, k:k + step].t()
    return acc


def emulate_f32(x, w, order):
    """The kernel's arithmetic in f32 torch, products and sums in summation order ``order`` -> pooled, t1 (bf16), logits, prob (f32)."""
    pooled = torch.tanh(_matmul_f32(x, w["w_pool"], order) + w["b_pool"]).to(torch.bfloat16)
    pre = _matmul_f32(pooled, w["w_tr"], order) + w["b_tr"]
    t1 = (pre * 0.5 * (1.0 + torch.erf(pre * 0.7071067811865476))).to(torch.bfloat16)
    logits, prob = emulate_tail_f32(t1, w, order)
    return pooled, t1, logits, prob


def emulate_tail_f32(t1, w, order, drop_group=None):
    """drop_group = (row, n): leave the 4-column group at n out of that row's two dot products (damage for the CPU proof)."""
    t = t1.float()
    H = t.shape[1]
    mean = _sum_f32(t, order) / H
    d = t - mean[:, None]
    var = _sum_f32(d * d, order) / H
    r = 1.0 / torch.sqrt(var + torch.tensor(w["eps"], dtype=torch.float32))
    y = d * r[:, None] * w["gamma"] + w["beta"]
    yw = y[:, None, :] * w["w_out"].float()[None]
    if drop_group is not None:
        yw[drop_group[0], :, drop_group[1]:drop_group[1] + 4] = 0
    logits = _sum_f32(yw, order) + w["b_out"]
    m = logits.max(1, keepdim=True).values
    e = torch.exp(logits - m)
    return logits, e[:, 1] / (e[:, 0] + e[:, 1])
