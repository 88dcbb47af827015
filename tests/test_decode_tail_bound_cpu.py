"""The bounds tests/test_decode_tail_gpu.py applies can fail: on the host (no GPU needed) the arithmetic of ln_acc_fwd_kernel
and of one k-slice of gemm_skinny_accum_kernel, emulated in f32 torch, sits at <= 1/2 of the bound (the SAFETY = 2 convention
of tests/attn_ref.py) at every width, slice count and dtype the GPU test uses, and the faults those kernels could have -- a
slab left out of the sum, a neighbouring row's residual, a chunk left out of the mean, a shifted beta, a k-block counted in
two slices -- are rejected on at least one element."""
import pytest
import torch

from attn_ref import layernorm_ref
from gemm_ref import U32, gemm_ref

BF, F32 = torch.bfloat16, torch.float32
LN_K = 256
# (dtype, rows, C, nsplit, residual, eps): the rows of test_decode_tail_gpu.LN_ACC
LN_CASES = [
    (BF, 64, 768, 1, True, 1e-12), (BF, 64, 768, 2, True, 1e-12), (BF, 64, 768, 4, True, 1e-12), (BF, 5, 768, 3, True, 1e-12),
    (BF, 64, 768, 8, True, 1e-5), (BF, 2, 1024, 2, True, 1e-12), (BF, 5, 2048, 4, True, 1e-12), (BF, 130, 256, 3, True, 1e-5),
    (BF, 64, 772, 2, True, 1e-12), (F32, 5, 4, 2, True, 1e-12), (BF, 5, 768, 2, False, 1e-12), (F32, 64, 768, 4, True, 1e-12),
    (F32, 2, 772, 8, True, 1e-5), (F32, 130, 2048, 1, False, 1e-5),
]


def test_cases_match_the_gpu_file():
    import test_decode_tail_gpu as G
    assert [c[1:] for c in G.LN_ACC] == LN_CASES and G.LN_K == LN_K


def _rand(shape, dt, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dt)


def k_slices(K, kb, k_splits):
    nkb = K // kb
    per = (nkb + k_splits - 1) // k_splits
    return [(min(s * per, nkb) * kb, min((s + 1) * per, nkb) * kb) for s in range(k_splits)]


def emu_slab(a, w, k0, k1, kb):
    """f32 accumulator of a[:, k0:k1] @ w[:, k0:k1]^T as a skinny workgroup forms it: wave v takes the k-blocks v, v + 8, ...
    of the slice one after the other (one MFMA each), the eight wave accumulators are added in wave order."""
    waves = [torch.zeros(a.shape[0], w.shape[0], dtype=F32) for _ in range(8)]
    for i, k in enumerate(range(k0, k1, kb)):
        waves[i % 8] = waves[i % 8] + a[:, k:k + kb].float() @ w[:, k:k + kb].float().t()
    v = waves[0]
    for x in waves[1:]:
        v = v + x
    return v


def emu_slabs(a, w, nsplit, kb):
    return torch.stack([emu_slab(a, w, k0, k1, kb) for k0, k1 in k_slices(a.shape[1], kb, nsplit)])


def emu_ln(acc, bias, res, gamma, beta, eps, dt, *, skip_slab=None, res_shift=0, mean_skip_last=False, beta_shift=0):
    """ln_acc_fwd_kernel in f32 torch: slabs added in slice order, then bias, then residual; the mean as an f32 sum
    divided by C; the variance as a second pass around that mean; 1 / sqrt(var + eps); the affine map; the output rounding.
    The keyword arguments plant one fault each."""
    Cn = acc.shape[2]
    v = None
    for s in range(acc.shape[0]):
        if s == skip_slab:
            continue
        v = acc[s].clone() if v is None else v + acc[s]
    v = v + bias
    if res is not None:
        v = v + torch.roll(res, res_shift, 0).float()
    tot = (v[:, :Cn - 4] if mean_skip_last else v).sum(1, keepdim=True)
    mean = tot / Cn
    d = v - mean
    var = (d * d).sum(1, keepdim=True) / Cn
    rstd = 1.0 / torch.sqrt(var + torch.tensor(eps, dtype=F32))
    y = d * rstd * gamma + torch.roll(beta, -beta_shift)
    return y.to(dt)


def _ln_setup(dt, rows, Cn, nsplit, has_res, eps):
    seed = rows * 7 + Cn * 13 + nsplit
    a = _rand((rows, LN_K), dt, seed + 1)
    w = _rand((Cn, LN_K), dt, seed + 2, LN_K ** -0.5)
    acc = emu_slabs(a, w, nsplit, 32 if dt == BF else 16)
    bias = _rand((Cn,), F32, seed + 3) + 0.5
    res = _rand((rows, Cn), dt, seed + 4, 2.0) if has_res else None
    gamma = 1.0 + 0.25 * _rand((Cn,), F32, seed + 5)
    beta = 0.25 * _rand((Cn,), F32, seed + 6)
    x = acc.double().sum(0) + bias.double()
    mag = acc.double().abs().sum(0) + bias.double().abs()
    if res is not None:
        x, mag = x + res.double(), mag + res.double().abs()
    ref, bound = layernorm_ref(x, gamma, beta, eps, out_dtype=dt, dv=(nsplit + 2) * U32 * mag)
    return acc, bias, res, gamma, beta, ref, bound


def _worst(out, ref, bound):
    return float(((out.double() - ref).abs() / bound).max())


@pytest.mark.parametrize("dt,rows,Cn,nsplit,has_res,eps", LN_CASES)
def test_layernorm_acc_emulation_accepted(dt, rows, Cn, nsplit, has_res, eps):
    acc, bias, res, gamma, beta, ref, bound = _ln_setup(dt, rows, Cn, nsplit, has_res, eps)
    y = emu_ln(acc, bias, res, gamma, beta, eps, dt)
    assert _worst(y, ref, bound) <= 0.5, _worst(y, ref, bound)
    # the slabs in another order (what a fault-free atomic form would give) stay inside the bound itself
    assert _worst(emu_ln(acc.flip(0), bias, res, gamma, beta, eps, dt), ref, bound) <= 1.0


@pytest.mark.parametrize("dt", [BF, F32])
def test_layernorm_acc_faults_rejected(dt):
    eps = 1e-12
    acc, bias, res, gamma, beta, ref, bound = _ln_setup(dt, 64, 768, 4, True, eps)
    assert _worst(emu_ln(acc, bias, res, gamma, beta, eps, dt), ref, bound) <= 0.5
    faults = dict(skip_slab=3, res_shift=1, mean_skip_last=True, beta_shift=4)
    for name, val in faults.items():
        bad = emu_ln(acc, bias, res, gamma, beta, eps, dt, **{name: val})
        assert _worst(bad, ref, bound) > 1.0, (name, _worst(bad, ref, bound))
    # the width whose last pass holds exactly that one chunk (C = 772: lane 0 of the fourth pass)
    acc, bias, res, gamma, beta, ref, bound = _ln_setup(dt, 64, 772, 2, True, eps)
    bad = emu_ln(acc, bias, res, gamma, beta, eps, dt, mean_skip_last=True)
    assert _worst(bad, ref, bound) > 1.0, _worst(bad, ref, bound)


# (dtype, M, N, K, k_splits): shapes of test_decode_tail_gpu.ACCUM, the widest reduction and the uneven / empty slices
SLAB_CASES = [(BF, 64, 768, 3072, 4), (BF, 64, 768, 768, 5), (BF, 64, 768, 768, 7), (BF, 33, 772, 768, 2), (F32, 64, 768, 400, 3)]


@pytest.mark.parametrize("dt,M,N,K,k_splits", SLAB_CASES)
def test_slab_emulation_accepted_and_double_counted_block_rejected(dt, M, N, K, k_splits):
    kb = 32 if dt == BF else 16
    a = _rand((M, K), dt, 1)
    w = _rand((N, K), dt, 2, K ** -0.5)
    a64, b64 = a.double(), w.double().t()
    sl = k_slices(K, kb, k_splits)
    bound_sum, total = torch.zeros(M, N, dtype=torch.float64), torch.zeros(M, N, dtype=torch.float64)
    for s, (k0, k1) in enumerate(sl):
        slab = emu_slab(a, w, k0, k1, kb)
        if k1 <= k0:
            assert bool((slab == 0).all())
            continue
        ref, _, bound, _, _ = gemm_ref(a64[:, k0:k1], b64[k0:k1], out_dtype=F32)
        assert _worst(slab, ref, bound) <= 0.5, (s, _worst(slab, ref, bound))
        bound_sum += bound
        total += slab.double()
        if s + 1 < len(sl) and sl[s + 1][1] > sl[s + 1][0]:
            # the first k-block of the next slice counted here as well (kb_hi one block too far)
            bad = emu_slab(a, w, k0, k1 + kb, kb)
            assert _worst(bad, ref, bound) > 1.0, (s, _worst(bad, ref, bound))
    ref, _, _, _, _ = gemm_ref(a64, b64, out_dtype=F32)
    assert _worst(total, ref, bound_sum) <= 0.5
    # ... and in the sum: one block twice
    twice = total + (a64[:, :kb] @ b64[:kb])
    assert _worst(twice, ref, bound_sum) > 1.0
