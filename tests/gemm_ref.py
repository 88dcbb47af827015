"""float64 reference of an mvlt_gemm product and a per-element error bound for it.

The reference is taken from the SAME operands the kernel reads (bf16 and f32 values are exact in float64), with every
epilogue of MvltGemm applied in float64 in the library's order (include/mvlt_hip.h): bias, saved pre-activation, erf-GELU,
dropout, row scale, x gelu'(aux), residual, accumulate, output rounding -- and the row map / device-side row count.

The bound, per element, is

    |out - ref| <= U_OUT |ref| + L (C_ACC 2^-24 sqrt(K_eff) S + r) + tiny,      S = |A| @ |B| (float64)

with U_OUT = 2^-8 for bf16 output and 2^-24 for f32, K_eff the reduction length after m_dev, L the epilogue's
Lipschitz factor (1.13 through GELU, the dropout scale, |row scale|, |gelu'(aux)|) and r the f32 rounding of the
epilogue's own operations plus the absolute error of the A&S erfc in csrc/common.h (<= 1.5e-7; not a bug).  Unlike a
relative Frobenius norm over the whole output it rejects local damage: a dropped partial k-tile, one misplaced
4-column group, a row tile left unwritten (tests/test_gemm_bound_cpu.py proves it on the host)."""
import math

import torch

U32 = 2.0 ** -24
U_BF16 = 2.0 ** -8
C_ACC = 8.0                 # f32 accumulation: a sqrt(K) random-walk constant with room for the MFMA's internal order
GELU_LIP = 1.13             # max |d/dx x Phi(x)| = 1.1289
ERFC_ABS = 2.0e-7           # |A&S 7.1.26 - erfc| <= 1.5e-7, plus the f32 evaluation


def gelu64(x):
    return x * 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0)))


def gelu_grad64(x):
    return 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def logical(A, B, a_kmajor=False, b_kmajor=False):
    """The operands as float64 [M, K] and [K, N], whatever their storage layout."""
    a = A.double()
    b = B.double()
    return (a.t() if a_kmajor else a), (b if b_kmajor else b.t())


def gemm_ref(a, b, *, out_dtype, k_eff=None, m_eff=None, bias=None, gelu=False, keep=None, drop_p=0.0,
             rowscale=None, rowmap=None, mul_gelu_grad=None, residual=None, prev=None):
    """a: [M, K], b: [K, N] (float64, logical layout, see ``logical``).  k_eff: reduction length (a k-major A's m_dev);
    m_eff: rows computed (a row-major A's m_dev).  keep: [m_eff, N] 0/1 dropout mask (ops.dropout_mask) for drop_p.
    rowscale: (scales, rows_per_scale) indexed by the OUTPUT row; rowmap: int tensor, output row of product row m;
    mul_gelu_grad / residual: [rows_out, N] operands indexed by the output row; prev: the output's previous content for
    accumulate.  Returns (ref, pre, bound, rows, pre_bound): the float64 values of the output rows ``rows`` (the mapped
    rows of the first m_eff product rows), their per-element bound, and the pre-activation with its bound (or None)."""
    M, K = a.shape
    N = b.shape[1]
    k_eff = K if k_eff is None else max(0, min(K, int(k_eff)))
    m_eff = M if m_eff is None else max(0, min(M, int(m_eff)))
    a, b = a[:m_eff, :k_eff], b[:k_eff]
    dev = a.device
    acc = a @ b
    S = a.abs() @ b.abs()
    err = C_ACC * U32 * math.sqrt(max(k_eff, 1)) * S + U32 * acc.abs()
    rows = torch.arange(m_eff, device=dev) if rowmap is None else rowmap[:m_eff].long().to(dev)
    v = acc
    if bias is not None:
        v = v + bias.double().to(dev)[None, :]
        err = err + U32 * v.abs()
    pre = pre_err = None
    if gelu:
        pre, pre_err = v, err + U_BF16 * v.abs()            # saved in the compute dtype (f32 runs: U_BF16 is loose, fine)
        g = gelu64(v)
        err = GELU_LIP * err + ERFC_ABS * v.abs() + 4 * U32 * g.abs()
        v = g
    if drop_p > 0.0:
        scale = 1.0 / (1.0 - drop_p)
        kf = keep.double().to(dev)[:m_eff]
        v = v * kf * scale
        err = err * kf * scale + U32 * v.abs()
    if rowscale is not None:
        rs, rps = rowscale
        s = rs.double().to(dev)[rows // rps][:, None]
        v = v * s
        err = err * s.abs() + U32 * v.abs()
    if mul_gelu_grad is not None:
        h = mul_gelu_grad.double().to(dev)[rows]
        gg = gelu_grad64(h)
        err = err * (gg.abs() + ERFC_ABS) + ERFC_ABS * v.abs() + 4 * U32 * (v * gg).abs()
        v = v * gg
    if residual is not None:
        v = v + residual.double().to(dev)[rows]
        err = err + U32 * v.abs()
    if prev is not None:
        v = v + prev.double().to(dev)[rows]
        err = err + U32 * v.abs()
    u_out = U32 if out_dtype == torch.float32 else U_BF16
    bound = err + u_out * v.abs() + 1e-30
    return v, pre, bound, rows, pre_err


def colsum_ref(a, k_eff=None):
    """Column sums of the logical A over the reduction (a k-major A's bias gradient): (ref, bound) per output row."""
    K = a.shape[1]
    k_eff = K if k_eff is None else max(0, min(K, int(k_eff)))
    a = a[:, :k_eff]
    return a.sum(1), C_ACC * U32 * math.sqrt(max(k_eff, 1)) * a.abs().sum(1) + 1e-30


def check_bound(out, ref, bound, what="", heads=None):
    """Assert |out - ref| <= bound element by element; on failure name the worst element (row, column, ratio to the
    bound) and how many elements are out.  Non-finite outputs count as out with an infinite ratio.  heads = (hd, nH):
    the columns are [part][head][hd] (attention: out, dqkv), and the message names the part and head as well."""
    out = out.double().to(ref.device)
    assert out.shape == ref.shape, (what, tuple(out.shape), tuple(ref.shape))
    if out.numel() == 0:
        return
    diff = (out - ref).abs()
    ratio = torch.where(torch.isfinite(out), diff / bound, torch.full_like(diff, math.inf))
    worst = float(ratio.max())
    if not worst <= 1.0:
        flat = int(ratio.argmax())
        r, c = divmod(flat, ref.shape[1]) if ref.dim() == 2 else (flat, 0)
        bad = int((ratio > 1.0).sum())
        idx = (r, c) if ref.dim() == 2 else (r,)
        where = "" if heads is None else f" (part {c // (heads[0] * heads[1])}, head {c // heads[0] % heads[1]})"
        raise AssertionError(
            f"{what}: {bad} of {ref.numel()} elements outside the bound; worst at row {r}, column {c}{where}: "
            f"out {float(out[idx]):.9g}, ref {float(ref[idx]):.9g}, bound {float(bound[idx]):.3g}, ratio {worst:.3g}")
