"""float64 reference of the per-row MLM-head pick (mvlt_gemm_pick_rows / _step) on top of sample_ref.py / gemm_ref.py, the inputs
the CPU and GPU tests share, and the teacher-forced checker of ``decode.sample_many``.  Not a test.

Row r of a call, from the operands the kernel reads (exact in float64) and the two tables:

    x = (A W^T + b)[r] inv_t[r]                inv_t: the f32 values of the table
    sampled (noise_row[r] >= 0):  y = x + g,   g = -log(-log(u01)) at index (noise_row[r] N + n) mod 2^32      (sample_ref.u01)
    greedy  (noise_row[r] <  0):  y = x,       g = 0 and e_g = 0: there is no noise term to be off
    token = first argmax_n y                   logprob = x[token] - logsumexp_n x      (the same definition for both kinds)

Bounds: those of sample_ref.sample_ref (SAFETY 2, e_g, LSE_SUM), per row with the row's inv_t and e_g = 0 on greedy rows."""
import math

import numpy as np
import torch

import sample_ref as S
from attn_ref import rng_u32
from gemm_ref import U32, gemm_ref

M32 = (1 << 32) - 1
SEED = 0x9E3779B97F4A7C15
TAG = S.TAG0 + 5
T_CYCLE = (1.0, 0.7, 1.5)          # temperatures the mixed-row tests cycle through
# (rows, K, N, dtype, operand seed) of the mixed-row tests, CPU and GPU: two groups (64 + 6 rows), a partial row tile, N no
# multiple of 16; the last is the real head
MIXED_CASES = [(70, 64, 1000, torch.bfloat16, 300), (70, 64, 1000, torch.float32, 301), (70, 768, 30522, torch.bfloat16, 302)]


def operands(R, K, N, dtype, seed):
    """CPU operands of a head product: A ~ N(0, 1) [R, K], W ~ N(0, 9 / K) [N, K] (logit std 3), bias ~ N(0, 0.01), in ``dtype``."""
    gen = torch.Generator().manual_seed(seed)
    A = torch.randn(R, K, generator=gen).to(dtype)
    W = (torch.randn(N, K, generator=gen) * (3.0 / math.sqrt(K))).to(dtype)
    bias = torch.randn(N, generator=gen) * 0.1
    return A, W, bias


def mixed_tables(R):
    """(noise_row int32 [R], inv_t f32 [R]) of the mixed-row tests: every third row greedy, (7 r + 3) % 97 on the others, the
    temperatures cycling through T_CYCLE."""
    r = torch.arange(R, dtype=torch.int64)
    noise_row = torch.where(r % 3 == 0, torch.full_like(r, -1), (7 * r + 3) % 97).to(torch.int32)
    inv_t = torch.tensor([S.inv_t_f32(T_CYCLE[i % 3]) for i in range(R)], dtype=torch.float32)
    return noise_row, inv_t


def _noise_k(noise_row, N, seed, tag):
    """k = rng_u32 >> 8 [R, N] (int64) at the documented index, whatever noise_row holds (greedy rows: an index nobody reads)."""
    idx = ((noise_row.to(torch.int64)[:, None] * N + torch.arange(N, dtype=torch.int64)[None, :]) & M32).reshape(-1)
    return (rng_u32(seed, tag, idx) >> 8).view(noise_row.numel(), N)


def pick_rows_ref(A, W, bias, noise_row, inv_t, seed, tag):
    """A [R, K], W [N, K], bias f32 [N] or None, noise_row int32 [R], inv_t f32 [R].  The dict of sample_ref.sample_ref."""
    R, N = A.shape[0], W.shape[0]
    v, _, e_v, _, _ = gemm_ref(A.double(), W.double().t(), out_dtype=torch.float32, bias=bias)
    it = inv_t.double()[:, None]
    x, e_x = v * it, e_v * it
    sampled = (noise_row >= 0)[:, None]
    u01 = (_noise_k(noise_row, N, seed, tag).double() + 0.5) * 2.0 ** -24
    zero = torch.zeros((), dtype=torch.float64)
    g = torch.where(sampled, S.gumbel_ref(u01), zero)
    eg = torch.where(sampled, S.e_g(g), zero)
    y = x + g
    tok = y.argmax(1)
    lse = torch.logsumexp(x, 1)
    bound_y = S.SAFETY * (e_x + eg + U32 * y.abs())
    e_lse = S.LSE_SUM * U32 + S.E_LOG * (lse - x.max(1).values).abs() + U32 * lse.abs()

    def bound_lp(t):
        xt = x.gather(1, t.view(-1, 1)).squeeze(1)
        return S.SAFETY * (e_x.gather(1, t.view(-1, 1)).squeeze(1) + e_x.max(1).values + e_lse + U32 * (xt - lse).abs())

    return dict(x=x, g=g, y=y, tok=tok, lse=lse, logprob=x.gather(1, tok.view(-1, 1)).squeeze(1) - lse, e_x=e_x, e_g=eg,
                bound_y=bound_y, bound_lp=bound_lp)


def lp_at(ref, tok):
    """The reference's log-probability of the tokens ``tok`` (the device's picks)."""
    return ref["x"].gather(1, tok.view(-1, 1)).squeeze(1) - ref["lse"]


def penalise32(raw32, seen, penalty):
    """HF's repetition penalty on the seen columns in f32, the kernel's two rounded operations."""
    p = torch.tensor(penalty, dtype=torch.float32)
    return torch.where(seen, torch.where(raw32 < 0, raw32 * p, raw32 / p), raw32)


def emulate_f32(raw32, noise_row, inv_t, seed, tag, parts=16, noise_idx_row=None, greedy_noise=False):
    """The device epilogue on f32 raw logits raw32 [R, N] (acc + bias, after any penalty) in the kernel's order: x = raw * inv_t[r],
    the noise of noise_row[r], y, the pick, per-part (max, sum exp) rescaled and combined, logf, the subtraction.
    ``noise_idx_row`` / ``greedy_noise``: two ways of getting it wrong (another row table for the noise; noise on greedy rows too).
    Returns (x32, y32, tok, logprob32)."""
    R, N = raw32.shape
    x32 = raw32 * inv_t[:, None]
    rows = noise_row if noise_idx_row is None else noise_idx_row
    k = _noise_k(rows, N, seed, tag).numpy().astype(np.uint32)
    g32 = torch.from_numpy(S.gumbel_f32(k.reshape(-1))).view(R, N)
    if not greedy_noise:
        g32 = torch.where((noise_row >= 0)[:, None], g32, torch.zeros((), dtype=torch.float32))
    y32 = x32 + g32
    tok = y32.argmax(1)
    npad = (N + parts - 1) // parts * parts
    xp = torch.full((R, npad), -math.inf, dtype=torch.float32)
    xp[:, :N] = x32
    xp = xp.view(R, npad // parts, parts)
    pm = xp.max(2).values
    ps = torch.exp(xp - pm[:, :, None]).sum(2)
    xm = pm.max(1).values
    lse = xm + torch.log((ps * torch.exp(pm - xm[:, None])).sum(1))
    return x32, y32, tok, x32.gather(1, tok.view(-1, 1)).squeeze(1) - lse


def teacher_forced_rows(O, sd, scfg, bcfg, image, ids, seed, noise_row, inv_t, tol=None, eos=None):
    """test_sample_gpu._teacher_forced_sampled over the rows of ``sample_many``: ids [B, S, n]; row r = b * S + s decodes image b.
    Per row and step the oracle's full-sequence recompute on the GENERATED prefix gives the logits, scaled by the row's inv_t; a
    sampled row adds the host noise of (seed, TAG0 + step, noise_row[r]), a greedy row (noise_row < 0) nothing; the device's token
    must be that argmax or a near-tie: within ``tol`` x (top - mean logit), tol = None: 2e-4 (the f32 margin of the model tests).
    Returns (exact, near, bad, logp [B, S, n] of the device's tokens under the oracle at the row's temperature)."""
    B, Sr, n = ids.shape
    R = B * Sr
    flat = ids.reshape(R, n)
    feat = O.conv_layer(image, sd, scfg).repeat_interleave(Sr, 0)
    Vv = bcfg.vocab_size
    sampled = (noise_row >= 0)[:, None]
    exact = near = 0
    bad, logp = [], torch.zeros(R, n, dtype=torch.float64)
    alive = torch.ones(R, dtype=torch.bool)
    for t in range(n):
        inp = torch.cat([flat[:, :t], torch.full((R, 1), bcfg.mask_token_id)], 1)
        o = O.mvlbert_forward(sd, bcfg, inp, feat, True)
        x = O.mlm_head(o["hidden"][:, -1], sd, "MLM_head_seq2seq", bcfg).double() * inv_t.double()[:, None]
        u01 = (_noise_k(noise_row, Vv, seed, S.TAG0 + t).double() + 0.5) * 2.0 ** -24
        y = x + torch.where(sampled, S.gumbel_ref(u01), torch.zeros((), dtype=torch.float64))
        logp[:, t] = torch.log_softmax(x, -1).gather(1, flat[:, t:t + 1].clamp(0, Vv - 1)).squeeze(1)
        spread = x.max(-1).values - x.mean(-1)
        for r in range(R):
            if not alive[r]:
                continue                        # finished rows emit PAD: nothing to pin
            m = float(y[r].max() - y[r, flat[r, t]])
            if m == 0.0:
                exact += 1
            elif m <= (tol if tol is not None else 2e-4) * float(spread[r]):
                near += 1
            else:
                bad.append((r, t, m, float(spread[r])))
        if eos is not None:
            alive &= flat[:, t] != eos
    return exact, near, bad, logp.view(B, Sr, n)
