"""float64 reference of the sampled MLM-head pick (mvlt_gemm_sample / mvlt_gemm_sample_step) and per-element bounds for it.

From the operands the kernel reads (A, W, bias as stored, exact in float64; inv_t = the f32 value of 1 / temperature):

    x = (A W^T + b) inv_t                      u = rng_u32(seed, tag, m N + n)          (attn_ref.rng_u32: the host port of the hash)
    u01 = ((u >> 8) + 0.5) 2^-24               g = -log(-log(u01))                      y = x + g
    token[m] = first argmax_n y[m, n]          logprob[m] = x[m, token] - logsumexp_n x[m, n]

Bounds (first-order, every constant derived from the kernel's own arithmetic):
  x        the product bound of gemm_ref.gemm_ref with an f32 output: C_ACC 2^-24 sqrt(K) |A||W| + the f32 roundings of
           the accumulator, of the bias add and (its "output rounding" term, 2^-24 |v|) of the multiplication by inv_t
  g        e_g(u01) = 2^-22 (3 + |g|) (1 + 2^-10).  The kernel (csrc/common.h gumbel_noise) forms k + 0.5 as h + l with h = fl(k + 0.5)
           and the exact remainder l, t = -(logf(h 2^-24) + l / h), g = -logf(t).  logf is the device library's, taken at
           <= 2 ulp = 2^-22 relative (E_LOG).  |log(h 2^-24)| <= (4/3) t, so t carries at most (4/3 + 3/4 + 1/4 + 1/4) 2^-22 < 3 2^-22
           relative error (logf; l / h with a 1-ulp reciprocal and the product's rounding; the dropped (l / h)^2 / 2 <= 2^-49 against
           t >= 2^-25; the rounding of the sum) -- an ABSOLUTE error of log t -- and the outer logf adds 2^-22 |g|.
  y        e_x + e_g + 2^-24 |y|   (one f32 rounding of the sum)
  logprob  |d x_tok| + max_n |d x_n| (a log-sum-exp moves by at most the largest change of a logit) + the f32 evaluation of the
           log-sum-exp: every term exp(x_n - max) is off by at most (2 d_n + 4) 2^-24 relative, d_n = max - x_n (rounding of the
           difference, of d log2(e), and the ex2 approximation), once inside a 16-column part and once when the part sums are
           rescaled; the softmax-weighted mean of d_n is at most log N (entropy <= log N), and at most 30 f32 additions lie on
           the path of a term: (4 log N + 8 + 30) 2^-24 < LSE_SUM 2^-24 for N <= 2^16.  Then logf of the sum (2^-22 |log sum|), the
           addition of the maximum (2^-24 |lse|) and the final subtraction (2^-24 |logprob|).
`bound_y` / `bound_lp` are SAFETY = 2 times these estimates, as in attn_ref (a correct kernel sits at <= 1/2); e_g is reported
as derived (it is compared with the device's noise directly).  tests/test_sample_bound_cpu.py proves the bounds on the host:
an f32 emulation of the epilogue stays inside at a ratio <= 0.5, and five ways of getting it wrong fall outside."""
import math

import numpy as np
import torch

from attn_ref import M32, _mix32_int, rng_u32
from gemm_ref import U32, gemm_ref

E_LOG = 2.0 ** -22            # relative error taken for logf (<= 2 ulp)
LSE_SUM = 96.0                # (4 log N + 8 + 30) for N <= 2^16, see above
SAFETY = 2.0
NEAR_TIE_CAP = 0.02           # share of a test's picks that may be near-ties
TAG0 = 0x53000000             # decode.SAMPLE_TAG0


def u01_ref(seed, tag, rows, N):
    """u01 [rows, N] (float64, exact) at the documented index m N + n."""
    idx = torch.arange(rows * N, dtype=torch.int64)
    k = rng_u32(seed, tag, idx) >> 8
    return ((k.double() + 0.5) * 2.0 ** -24).view(rows, N)


def gumbel_ref(u01):
    return -torch.log(-torch.log(u01))


def e_g(g):
    return E_LOG * (3.0 + g.abs()) * (1.0 + 2.0 ** -10)


def gumbel_f32(k):
    """The kernel's own sequence of f32 operations (csrc/common.h gumbel_noise) on k = rng_u32 >> 8 (numpy uint32 / int)."""
    kf = k.astype(np.float32)
    h = kf + np.float32(0.5)
    l = (kf - h) + np.float32(0.5)
    t = -(np.log(h * np.float32(2.0 ** -24), dtype=np.float32) + l * (np.float32(1.0) / h))
    return -np.log(t, dtype=np.float32)


def inv_t_f32(temperature):
    return float(np.float32(1.0 / float(temperature)))


def sample_ref(A, W, bias, seed, tag, temperature=1.0):
    """A [M, K], W [N, K] (N = the true vocabulary: pass W[:N]), bias f32 [N] or None.  Returns a dict of float64 tensors:
    x, g, y [M, N]; tok [M]; logprob [M]; e_x, bound_y [M, N]; bound_lp(tok) -> [M] for the token actually scored."""
    M, N = A.shape[0], W.shape[0]
    v, _, e_v, _, _ = gemm_ref(A.double(), W.double().t(), out_dtype=torch.float32, bias=bias)
    it = inv_t_f32(temperature)
    x, e_x = v * it, e_v * it
    g = gumbel_ref(u01_ref(seed, tag, M, N))
    y = x + g
    tok = y.argmax(1)                                   # torch returns the first index of the maximum
    lse = torch.logsumexp(x, 1)
    eg = e_g(g)
    bound_y = SAFETY * (e_x + eg + U32 * y.abs())
    xmax = x.max(1).values
    e_lse = LSE_SUM * U32 + E_LOG * (lse - xmax).abs() + U32 * lse.abs()

    def bound_lp(t):
        xt = x.gather(1, t.view(-1, 1)).squeeze(1)
        return SAFETY * (e_x.gather(1, t.view(-1, 1)).squeeze(1) + e_x.max(1).values + e_lse + U32 * (xt - lse).abs())

    return dict(x=x, g=g, y=y, tok=tok, lse=lse, logprob=x.gather(1, tok.view(-1, 1)).squeeze(1) - lse, e_x=e_x, e_g=eg,
                bound_y=bound_y, bound_lp=bound_lp)


def classify_picks(tok, y, bound_y):
    """Every pick is the reference's token or a NEAR-TIE: the reference's y at the picked token is within the sum of the two
    elements' bounds of the reference's maximum.  Returns (exact, near, bad [(row, picked, reference, gap, allowed)])."""
    tok = tok.cpu().long()
    ref = y.argmax(1)
    exact = near = 0
    bad = []
    for m in range(y.shape[0]):
        t, r = int(tok[m]), int(ref[m])
        if t == r:
            exact += 1
            continue
        if not 0 <= t < y.shape[1]:
            bad.append((m, t, r, math.inf, 0.0))
            continue
        gap, allowed = float(y[m, r] - y[m, t]), float(bound_y[m, r] + bound_y[m, t])
        if gap <= allowed:
            near += 1
        else:
            bad.append((m, t, r, gap, allowed))
    return exact, near, bad


def assert_picks(tok, y, bound_y, what, cap=NEAR_TIE_CAP, extra=0):
    """No pick outside the near-tie margin, and at most cap * picks (+ extra) near-ties; the counts go into the message."""
    exact, near, bad = classify_picks(tok, y, bound_y)
    n = y.shape[0]
    msg = f"{what}: {exact} exact, {near} near-ties, {len(bad)} wrong of {n} picks (near-tie cap {cap:.0%} + {extra}); wrong: {bad[:4]}"
    assert not bad and near <= cap * n + extra, msg
    return exact, near


def gumbel_host_row(seed, tag, N):
    """float64 noise of one row of width N for one tag, in plain Python integers (many small draws: the chi-square test)."""
    seed &= (1 << 64) - 1
    key = _mix32_int((seed & M32) ^ ((tag * 0x9E3779B9) & M32)) ^ (seed >> 32)
    out = []
    for n in range(N):
        k = _mix32_int(((n * 0x9E3779B1) + key) & M32) >> 8
        out.append(-math.log(-math.log((k + 0.5) * 2.0 ** -24)))
    return out


def emulate_f32(x32, seed, tag, N, parts=16):
    """The device epilogue from f32 logits x32 [M, N] on (torch float32, the kernel's order of operations): noise, y, the pick,
    per-part (max, sum exp) and their rescaled combination, logf, the final subtraction.  Returns (g32, y32, tok, logprob32)."""
    M = x32.shape[0]
    idx = torch.arange(M * N, dtype=torch.int64)
    k = (rng_u32(seed, tag, idx) >> 8).numpy().astype(np.uint32)
    g32 = torch.from_numpy(gumbel_f32(k)).view(M, N)
    y32 = x32 + g32
    tok = y32.argmax(1)
    npad = (N + parts - 1) // parts * parts
    xp = torch.full((M, npad), -math.inf, dtype=torch.float32)
    xp[:, :N] = x32
    xp = xp.view(M, npad // parts, parts)
    pm = xp.max(2).values
    ps = torch.exp(xp - pm[:, :, None]).sum(2)
    xm = pm.max(1).values
    s = (ps * torch.exp(pm - xm[:, None])).sum(1)
    lse = xm + torch.log(s)
    lp = x32.gather(1, tok.view(-1, 1)).squeeze(1) - lse
    return g32, y32, tok, lp
