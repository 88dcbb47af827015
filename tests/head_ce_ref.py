"""float64 reference of mvlt_mlm_head_ce (the MLM decoder product with the cross-entropy forward in its epilogue) and the
bounds its outputs are held to.  Everything is taken from the operands the kernel reads (bf16 / f32 are exact in float64):

    v = A W^T + bias (float64)        x = v rounded to the storage dtype        lse_m = logsumexp_n x[m, n]
    nll_m = lse_m - x[m, label_m]     acc = (sum of nll over labelled valid rows, their number)

Bounds (first order, constants from the kernel's own arithmetic, csrc/headce.hip):

  e_x    the unrounded value: gemm_ref's product + bias bound, C_ACC 2^-24 sqrt(K) (|A| |W|^T) + 2^-24 (|acc| + |v|).  The stored
         logits are checked against v with gemm_ref's full bound (e_x + the output rounding), as the GEMM-route tests do.
  flip   the statistics use the ROUNDED value.  Kernel and reference round the same number up to e_x, so they agree exactly
         unless v lies within e_x of a rounding boundary; then they differ by at most e_x + one spacing of the storage grid
         (at most 2 U_OUT |x|: frexp's exponent times U_OUT).  d[m, n] = that, or 0 where no flip is possible.  lse moves by at most log sum_n p_n exp(d_n) with p the
         reference softmax (each term of the sum grows or shrinks by at most exp(d_n); Jensen gives the lower side): never more
         than the row's largest e_x plus its spacing, and far less when the flips sit in the tail of the distribution.
  sum    every term exp(x - M) reaches the row's sum through up to three factors exp(.) whose exponents add up to x - M (lane
         / wave pair / column tile maxima): __expf is off by (3 d + 4) 2^-24 relative at exponent -d (rounding of the difference,
         of d log2 e with a rounded constant, the ex2 approximation), so 3 d + 12 in all with the softmax-weighted mean of d at
         most ln V; three products; and the additions on the term's path.  The kernel adds 16 per lane, 2 exchanges, 1 wave
         pair, ceil(tiles / 64) + 6 over the tiles; the bound takes TILE + tiles additions, which covers ANY order that adds
         the 128 columns of a tile first and the ceil(V / 128) tiles afterwards:
             sum_terms(V) = 3 ln V + 12 + 3 + 128 + ceil(V / 128)        (each 2^-24, relative to the sum = absolute on lse)
  log    logf of the sum, E_LOG |lse - max| (2 ulp), and the addition of the maximum, 2^-24 |lse|.
bound_lse = flip + SAFETY (sum + log), SAFETY = 2 as in sample_ref / beam_ref on the first-order parts (flip is rigorous).
x_label: against v[m, label] with the stored logits' bound.  acc[0]: the rows' bound_lse + bound_x at the label + 2^-24 |nll| (the
subtraction), plus (ceil(R / 1024) + 11) 2^-24 sum |nll| for the fixed-order row sum (thread-strided, ten tree levels);
acc[1] is exact."""
import math

import torch

from gemm_ref import U32, U_BF16, gemm_ref, logical
from sample_ref import E_LOG, SAFETY

TILE = 128                    # HBN of csrc/headce.hip
IGNORE = -100


def sum_terms(V):
    return 3.0 * math.log(V) + 12.0 + 3.0 + TILE + math.ceil(V / TILE)


def operands(M, K, V, dtype, seed, pad=64):
    """A [M, K], W [V, K] in ``dtype`` and a f32 bias view [V] of a buffer with ``pad`` poisoned entries behind it.  W is scaled so
    that the logit of largest magnitude is +90 (exp overflows without the max subtraction); the bias has its largest entry, +6, in column
    V - 1 and its poison, 3e4, right behind it (a column mask off by one, or missing, shows in every row)."""
    g = torch.Generator().manual_seed(seed)
    A = (torch.rand(M, K, generator=g) * 2 - 1).to(dtype)
    W = torch.rand(V, K, generator=g) * 2 - 1
    x = (A.double() @ W.double().t()).reshape(-1)
    peak = float(x[x.abs().argmax()])          # signed: the largest logit becomes +90, not -90
    col = int(x.abs().argmax()) % V            # ... and sits in the last column: that row's lse lives in the partial tile
    W[[col, V - 1]] = W[[V - 1, col]]
    W = (W * (90.0 / peak)).to(dtype)
    buf = torch.full((V + pad,), 3.0e4, dtype=torch.float32)
    buf[:V] = torch.rand(V, generator=g) * 2 - 1
    buf[V - 1] = 6.0
    return A, W, buf


def edge_labels(M, V, packed, seed):
    """int64 [M]: random labels with the epilogue's edge columns in the first rows -- column 0, column V - 1, the first and the last
    column of the last, partial column tile -- and, unless ``packed``, every third row ignored (after the edge rows)."""
    g = torch.Generator().manual_seed(seed)
    lab = torch.randint(0, V, (M,), generator=g)
    edges = [0, V - 1, (V - 1) // TILE * TILE, V - 1 - ((V - 1) % 4)]
    for i, e in enumerate(edges):
        lab[(i * 6) % M] = e          # (rows 0, 6, 12, 18: never the ignored ones; M = 1 keeps the last)
    if not packed:
        idx = torch.arange(M)
        lab[(idx % 3 == 2) & (idx >= 4)] = IGNORE
    return lab


def grid_spacing(x, u_out):
    """(one step of the storage grid at x, x is a power of two or 0): frexp gives |mant| in [0.5, 1), so a p-bit significand
    (u_out = 2^-p) steps by 2^expo u_out above |x|; half of it is the distance from x to its rounding boundaries."""
    mant, expo = torch.frexp(x)
    return torch.ldexp(torch.ones_like(x), expo) * u_out, (mant.abs() == 0.5) | (x == 0)


def head_ce_ref(A, W, bias, labels, rows=None):
    """-> dict of float64 tensors over the first ``rows`` rows: v, bound_v [R, V] (stored logits), lse, bound_lse [R], x_label,
    bound_xl [R] (NaN / inf where the label is ignored), nll_sum, bound_sum, count; d [R, V] the flip allowance per element."""
    a, b = logical(A, W)
    R = A.shape[0] if rows is None else max(0, min(A.shape[0], int(rows)))
    V = W.shape[0]
    u_out = U32 if A.dtype == torch.float32 else U_BF16
    v, _, bound_v, _, _ = gemm_ref(a, b, out_dtype=A.dtype, m_eff=R, bias=bias)
    e_x = bound_v - u_out * v.abs()
    x = v.to(A.dtype).double()
    # distance of v to the nearest rounding boundary of the storage grid around x (a power of two has the finer grid below it:
    # counted as always flippable, there are few)
    spacing, pow2 = grid_spacing(x, u_out)
    flippable = pow2 | ((0.5 * spacing - (v - x).abs()) <= e_x)
    d = torch.where(flippable, e_x + 1.01 * spacing, torch.zeros_like(x))
    lse = torch.logsumexp(x, 1)
    p = torch.exp(x - lse[:, None])
    flip = torch.log((p * torch.exp(d)).sum(1))
    xmax = x.max(1).values if R else x.new_zeros(0)
    bound_lse = flip + SAFETY * (sum_terms(V) * U32 + E_LOG * (lse - xmax).abs() + U32 * lse.abs())
    lab = labels[:R].long()
    on = lab >= 0
    safe = lab.clamp(0, V - 1)[:, None]
    x_label = torch.where(on, x.gather(1, safe)[:, 0], torch.full_like(lse, math.nan))
    v_label = torch.where(on, v.gather(1, safe)[:, 0], torch.full_like(lse, math.nan))
    bound_xl = torch.where(on, bound_v.gather(1, safe)[:, 0], torch.full_like(lse, math.inf))
    nll = (lse - x_label)[on]
    n = int(on.sum())
    bound_sum = float((bound_lse[on] + bound_xl[on] + d.gather(1, safe)[:, 0][on] + U32 * nll.abs()).sum()
                      + (math.ceil(max(R, 1) / 1024) + 11) * U32 * nll.abs().sum()) + 1e-30
    return dict(v=v, bound_v=bound_v, x=x, lse=lse, bound_lse=bound_lse, x_label=v_label, bound_xl=bound_xl,
                nll_sum=float(nll.sum()), bound_sum=bound_sum, count=n, on=on, d=d)


def emulate_f32(A, W, bias, labels, rows=None, tile=96):
    """The kernel's arithmetic in f32 torch with ANOTHER summation order (column tiles of ``tile``, each summed by torch, tiles
    folded sequentially by an online max) -> (lse f32 [R], x_label f32 [R], nll_sum, count).  For the CPU test of the bound."""
    R = A.shape[0] if rows is None else int(rows)
    V = W.shape[0]
    x = ((A[:R].float() @ W.float().t()) + bias[None, :]).to(A.dtype).float()
    m = torch.full((R,), -math.inf)
    s = torch.zeros(R)
    for c0 in range(0, V, tile):
        blk = x[:, c0:c0 + tile]
        bm = blk.max(1).values
        bs = torch.exp(blk - bm[:, None]).sum(1)
        nm = torch.maximum(m, bm)
        s = s * torch.exp(m - nm) + bs * torch.exp(bm - nm)
        m = nm
    lse = m + torch.log(s)
    lab = labels[:R].long()
    on = lab >= 0
    xl = x.gather(1, lab.clamp(0, V - 1)[:, None])[:, 0]
    nll = torch.where(on, lse - xl, torch.zeros_like(lse))
    return lse, xl, float(nll.sum(dtype=torch.float32)), int(on.sum())


# the cases of tests/test_head_ce_gpu.py: (M, K, V, rows_dev) with rows_dev None = absent
SMALL = [(M, K, 777, rd) for M in (1, 63, 64, 65, 130) for K in (64, 768) for rd in (None, M, 37, 0)]
BIG = (130, 768, 30522, None)


def seed_of(M, K, V, dtype):
    return 4000 + M * 7 + K + V % 1000 + (500 if dtype == torch.float32 else 0)
