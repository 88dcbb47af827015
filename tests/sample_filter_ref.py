"""float64 reference of the filtered sampled pick (mvlt_gemm_sample_filtered / _step) on top of sample_ref.sample_ref, whose
x, e_x, y and bound_y it uses.  Per row, with x the temperature-scaled logit and top_p the f32 value the device receives:

    top-k (1 <= k < N)   tau_k = k-th largest x with multiplicity, K1 = {x_n >= tau_k}                   (ties all kept)
    top-p (0 < p < 1)    w_n = exp(x_n - max x), S = sum_K1 w, A(v) = sum_{K1, x_j > v} w_j, K = {n in K1 : A(x_n) < p S}
    token = first argmax_K (x + G),  G at index (row0 + m) N + n;   score = x_token - log sum_K exp(x)

The device decides membership on f32 x and on fixed-point masses, so next to K_ref there are the columns the bounds cannot
decide.  lo = x - SAFETY e_x, hi = x + SAFETY e_x:
    IN_k   #{j != n : hi_j >= lo_n} < k                    OUT_k   #{j : lo_j > hi_n} >= k
    IN_p   (1 + E_MASS) sum_{j != n, j not OUT_k, hi_j >= lo_n} w(hi_j)  <  p (1 - E_MASS) sum_{IN_k} w(lo_j)
    OUT_p  (1 - E_MASS) sum_{j in IN_k, lo_j > hi_n} w(lo_j)  >=  p (1 + E_MASS) sum_{j not OUT_k} w(hi_j)
    IN = IN_k & IN_p,  OUT = OUT_k | OUT_p,  U = the rest
E_MASS(N) = (3 ln N + 4) 2^-24 + N 2^-33 + 2^-51 is the relative error of a device mass sum (derived in csrc/skinny.hip: the
__expf of a rounded difference, the quantisation to rint(2^32 w), exact integer summation, the f64 product top_p S).
Pick rule: the device's token t is exact if t == argmax_{K_ref} y; else acceptable if t is not in OUT and
y_t + bound_y_t >= max_{IN} (y_n - bound_y_n); anything else is wrong.  Score rule: with U empty the score lies within
bound_lp(t) of x_t - lse(K_ref); else between x_t - lse(IN | U) and x_t - lse(IN), widened by bound_lp(t).
`emulate` is the device's own sequence on f32 logits (tests/test_sample_filter_bound_cpu.py runs it against these rules)."""
import math

import numpy as np
import torch

import sample_ref as S
from attn_ref import rng_u32
from gemm_ref import U32

K, N = 256, 4106              # the small head of the GPU tests: 16 x 256 + 10 columns (a ragged last part)
SEED = 0x9E3779B97F4A7C15
FILTERS = [(1, 1.0), (8, 1.0), (0, 0.9), (50, 0.9), (4105, 0.5)]


def e_mass(n):
    return (3.0 * math.log(n) + 4.0) * 2.0 ** -24 + n * 2.0 ** -33 + 2.0 ** -51


def p32(top_p):
    return float(np.float32(top_p))


def operands(rows, dtype, seed, n=N, k=K, std=2.5):
    """A ~ N(0, 1) [rows, k], W ~ N(0, std^2 / k) [n, k] (logit std 2.5 at T = 1: a softmax with a body and a tail; unscaled
    operands give a one-token softmax and a filter test that cannot fail), bias ~ N(0, 0.01); stored in `dtype`."""
    gen = torch.Generator().manual_seed(seed)
    A = torch.randn(rows, k, generator=gen).to(dtype)
    W = (torch.randn(n, k, generator=gen) * (std / math.sqrt(k))).to(dtype)
    bias = torch.randn(n, generator=gen) * 0.1
    return A, W, bias


def kept_ref(x, top_k, top_p, strict=True):
    """K of one row by the definitions (float64 x [N]; top_p already the f32 value) -> bool [N].  strict=False is the wrong rule
    A <= p S, kept for the tests."""
    n = x.numel()
    keep = torch.ones(n, dtype=torch.bool)
    if 1 <= top_k < n:
        keep = x >= torch.topk(x, top_k).values[-1]
    if top_p < 1.0:
        w = torch.exp(x - x.max()) * keep
        xs, order = torch.sort(x, descending=True, stable=True)
        cs = torch.cumsum(w[order], 0)
        first = torch.searchsorted(-xs, -xs, right=False)              # first position of every tie group
        above = torch.where(first > 0, cs[(first - 1).clamp(min=0)], torch.zeros_like(cs))
        ok = (above < top_p * cs[-1]) if strict else (above <= top_p * cs[-1])
        kp = torch.zeros(n, dtype=torch.bool)
        kp[order] = ok
        keep = keep & kp
    return keep


def membership(x, e_x, top_k, top_p):
    """(IN, OUT) bool [N] of one row; U = ~(IN | OUT)."""
    n = x.numel()
    lo, hi = x - S.SAFETY * e_x, x + S.SAFETY * e_x
    in_k, out_k = torch.ones(n, dtype=torch.bool), torch.zeros(n, dtype=torch.bool)
    if 1 <= top_k < n:
        hs, ls = torch.sort(hi).values, torch.sort(lo).values
        in_k = (n - torch.searchsorted(hs, lo, right=False) - 1) < top_k
        out_k = (n - torch.searchsorted(ls, hi, right=True)) >= top_k
    in_p, out_p = torch.ones(n, dtype=torch.bool), torch.zeros(n, dtype=torch.bool)
    if top_p < 1.0:
        em, c = e_mass(n), x.max()
        wh = torch.exp(hi - c) * (~out_k)                               # the most a column can weigh, if it can be in K1 at all
        wl = torch.exp(lo - c) * in_k                                   # the least, if it is in K1 for certain
        tot_hi, tot_lo = wh.sum(), wl.sum()
        hs, oh = torch.sort(hi)
        suf_h = torch.flip(torch.cumsum(torch.flip(wh[oh], [0]), 0), [0])          # sum over sorted positions >= i
        i = torch.searchsorted(hs, lo, right=False)
        above_max = torch.where(i < n, suf_h[i.clamp(max=n - 1)], torch.zeros_like(lo)) - wh          # j != n (hi_n >= lo_n always)
        in_p = (1 + em) * above_max < top_p * (1 - em) * tot_lo
        ls, ol = torch.sort(lo)
        suf_l = torch.flip(torch.cumsum(torch.flip(wl[ol], [0]), 0), [0])
        i = torch.searchsorted(ls, hi, right=True)
        above_min = torch.where(i < n, suf_l[i.clamp(max=n - 1)], torch.zeros_like(hi))
        out_p = (1 - em) * above_min >= top_p * (1 + em) * tot_hi
    return in_k & in_p, out_k | out_p


def filter_ref(A, W, bias, seed, tag, top_k, top_p, temperature=1.0, row0=0, base=None):
    """The reference of one call.  `base` = a sample_ref result of the same operands and temperature (it is not changed; its
    noise is replaced when row0 / tag differ).  Returns a dict: x, e_x, y, bound_y [M, N]; keep, IN, OUT [M, N] bool; tok [M];
    bound_lp (callable, from sample_ref)."""
    if base is None:
        base = S.sample_ref(A, W, bias, seed, tag, temperature)
    x, e_x = base["x"], base["e_x"]
    M, n = x.shape
    g = S.gumbel_ref(S.u01_ref(seed, tag, row0 + M, n)[row0:])
    y = x + g
    bound_y = S.SAFETY * (e_x + S.e_g(g) + U32 * y.abs())
    tp = p32(top_p)
    keep = torch.stack([kept_ref(x[m], top_k, tp) for m in range(M)])
    io = [membership(x[m], e_x[m], top_k, tp) for m in range(M)]
    IN, OUT = torch.stack([a for a, _ in io]), torch.stack([b for _, b in io])
    tok = torch.where(keep, y, torch.full_like(y, -math.inf)).argmax(1)
    return dict(x=x, e_x=e_x, y=y, bound_y=bound_y, keep=keep, IN=IN, OUT=OUT, tok=tok, bound_lp=base["bound_lp"])


def _lse(x, mask):
    return torch.logsumexp(torch.where(mask, x, torch.full_like(x, -math.inf)), 1)


def classify(ref, tok, score):
    """-> (exact, near, wrong [(row, token, why)], worst score ratio).  The rules of the module docstring."""
    tok, score = tok.cpu().long(), score.cpu().double()
    x, y, by, IN, OUT = ref["x"], ref["y"], ref["bound_y"], ref["IN"], ref["OUT"]
    M, n = x.shape
    exact = near = 0
    wrong = []
    inside = (tok >= 0) & (tok < n)
    t = tok.clamp(0, n - 1).view(-1, 1)
    floor = torch.where(IN, y - by, torch.full_like(y, -math.inf)).max(1).values
    for m in range(M):
        tm = int(tok[m])
        if not bool(inside[m]):
            wrong.append((m, tm, "out of range"))
        elif tm == int(ref["tok"][m]):
            exact += 1
        elif bool(OUT[m, tm]):
            wrong.append((m, tm, "filtered out"))
        elif float(y[m, tm] + by[m, tm]) >= float(floor[m]):
            near += 1
        else:
            wrong.append((m, tm, f"y short by {float(floor[m] - y[m, tm] - by[m, tm]):.3e}"))
    xt = x.gather(1, t).squeeze(1)
    b = ref["bound_lp"](t.squeeze(1))
    undecided = (~(IN | OUT)).any(1)
    lo = xt - torch.where(undecided, _lse(x, ~OUT), _lse(x, ref["keep"]))
    hi = xt - torch.where(undecided, _lse(x, IN), _lse(x, ref["keep"]))
    dev = torch.maximum(lo - score, score - hi).clamp(min=0.0)
    dev = torch.where(torch.isfinite(score), dev, torch.full_like(dev, math.inf))
    ratio = dev / b
    for m in range(M):
        if float(ratio[m]) > 1.0 and bool(inside[m]):
            wrong.append((m, int(tok[m]), f"score {float(score[m]):.6f} outside [{float(lo[m]):.6f}, {float(hi[m]):.6f}] +- {float(b[m]):.2e}"))
    return exact, near, wrong, float(ratio.max())


# ------------------------------------------------------------------------------------------------ the device's sequence
def noise_f32(seed, tag, rows, n, row0=0):
    idx = torch.arange(row0 * n, (row0 + rows) * n, dtype=torch.int64)
    k = (rng_u32(seed, tag, idx) >> 8).numpy().astype(np.uint32)
    return torch.from_numpy(S.gumbel_f32(k)).view(rows, n)


def masses(x32, xmax):
    """q = rint(2^32 expf(x - max)) as Python-exact uint64 (numpy), the kernel's filt_mass."""
    w = np.exp((x32 - xmax).astype(np.float32), dtype=np.float32)
    return np.rint(w.astype(np.float64) * 4294967296.0).astype(np.uint64)


def kept_f32(xr, top_k, top_p, strict=True, p_first=False, k_adjust=0, drop_ties=False):
    """The device's kept set of one f32 row (numpy [N]) -> bool [N].  The keyword arguments are the WRONG implementations of the
    CPU test: the rule A <= P, top-p before top-k, top-k off by one, ties at tau_k dropped."""
    n = xr.shape[0]
    xmax = xr.max()
    keep = np.ones(n, dtype=bool)

    def topk(keep):
        k = top_k + k_adjust
        if not (1 <= top_k < n):
            return keep
        vals = np.sort(xr[keep])[::-1]
        tau = vals[min(k, vals.shape[0]) - 1]
        out = keep & (xr >= tau)
        if drop_ties:                                                  # exactly k columns: the later duplicates go
            idx = np.nonzero(out)[0]
            order = idx[np.argsort(-xr[idx], kind="stable")]
            out = np.zeros(n, dtype=bool)
            out[order[:k]] = True
        return out

    def topp(keep):
        if not top_p < 1.0:
            return keep
        q = masses(xr, xmax) * keep.astype(np.uint64)
        s_int = int(q.sum(dtype=np.uint64))
        target = min(max(int(math.ceil(float(np.float32(top_p)) * float(s_int))), 1), s_int)
        order = np.argsort(-xr, kind="stable")
        xs, cs = xr[order], np.cumsum(q[order], dtype=np.uint64)
        last = np.searchsorted(-xs, -xs, side="right") - 1            # last position of every tie group: C(v) inclusive
        first = np.searchsorted(-xs, -xs, side="left")
        c_incl = cs[last].astype(object)
        a_excl = np.where(first > 0, cs[np.maximum(first - 1, 0)], np.uint64(0)).astype(object)
        if strict:
            tau = xs[np.nonzero(np.array([c >= target for c in c_incl]))[0][0]]          # largest v with C(v) >= P
        else:
            tau = xs[np.nonzero(np.array([a <= target for a in a_excl]))[0][-1]]
        return keep & (xr >= tau)

    return topk(topp(keep)) if p_first else topp(topk(keep))


def emulate(x32, seed, tag, top_k, top_p, row0=0, noise_row0=None, renorm=True, **wrong):
    """f32 logits [M, N] (torch) -> (tok, score f32, keep bool [M, N]): select on f32 x, integer masses, thresholds, the pick
    over the kept columns and the kept log-sum-exp in f32."""
    M, n = x32.shape
    g32 = noise_f32(seed, tag, M, n, row0 if noise_row0 is None else noise_row0)
    y32 = x32 + g32
    xn = x32.numpy()
    keep = torch.from_numpy(np.stack([kept_f32(xn[m], top_k, top_p, **wrong) for m in range(M)]))
    tok = torch.where(keep, y32, torch.full_like(y32, -math.inf)).argmax(1)
    xmax = x32.max(1).values
    e = torch.exp(x32 - xmax[:, None]) * (keep if renorm else torch.ones_like(keep))
    lse = xmax + torch.log(e.sum(1))
    return tok, x32.gather(1, tok.view(-1, 1)).squeeze(1) - lse, keep


# ------------------------------------------------------------------------------------------------ shared test inputs
def tied_operands(dtype, rows=8, seed=31):
    """The constructed ties of the GPU test: in every row the columns ranked 4 and 5 become copies of ONE weight row and bias,
    and so do the columns ranked 11 .. 13: bit-equal logits at the 4th place (top_k = 4 must keep 5 columns) and inside the
    nucleus.  Returns (A, W, bias, twins [rows][2], triple [rows][3]) -- per row its own duplicates, so one W serves row 0 only;
    the rows are independent products on W copies, hence rows = separate calls."""
    A, W, bias = operands(rows, dtype, seed, n=512)
    out = []
    for m in range(rows):
        Wm, bm = W.clone(), bias.clone()
        x = (A[m:m + 1].double() @ Wm.double().t() + bm.double()[None, :])[0]
        order = torch.argsort(x, descending=True)
        a, b = int(order[3]), int(order[4])
        Wm[b], bm[b] = Wm[a], bm[a]
        c = [int(order[10]), int(order[11]), int(order[12])]
        for j in c[1:]:
            Wm[j], bm[j] = Wm[c[0]], bm[c[0]]
        out.append((A[m:m + 1], Wm, bm, sorted((a, b)), sorted(c)))
    return out


def frequency_case():
    """One row of 24 logits (std 1.5), top_k = 5, 4096 tags with seed 99: (logits f64, kept mask, expected probabilities)."""
    gen = torch.Generator().manual_seed(3)
    logits = (torch.randn(24, generator=gen) * 1.5).double()
    keep = kept_ref(logits, 5, 1.0)
    p = torch.softmax(torch.where(keep, logits, torch.full_like(logits, -math.inf)), 0)
    return logits, keep, p


CHI2_CRIT_4DF = 23.51             # chi-square, 4 degrees of freedom, significance 1e-4 (the level of test_sample_bound_cpu.py)


def chi_square(tokens, keep, p, n):
    idx = [i for i in range(keep.numel()) if bool(keep[i])]
    counts = [sum(1 for t in tokens if t == i) for i in idx]
    assert sum(counts) == n, "a draw outside the kept set"
    return sum((c - n * float(p[i])) ** 2 / (n * float(p[i])) for c, i in zip(counts, idx))
