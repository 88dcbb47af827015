"""float64 reference of an mvlt_layernorm_fwd / mvlt_layernorm_bwd call and per-element error bounds for it.

The reference is taken from the SAME operands the kernel reads (bf16 and f32 values are exact in float64; eps is the f32
value the struct carries).  The backward takes the saved ``mean`` / ``rstd`` it is handed as exact doubles: the stats are
judged once, in the forward, against the float64 stats of the same x (stage by stage, as test_swin_wmsa2_stage_by_stage).

Forward (csrc/norm.hip: ln_fwd_kernel), per row of width C, all in f32:
  mean   an f32 sum over C and one division:      e_mu = C_ACC 2^-24 sqrt(C) mean|x| + 2^-24 |mu|
  var    d = x - mean (one rounding each), an f32 sum of d d over C, one division.  The error of the mean enters the sum
         of squares only as e_mu^2 (sum (x - mu) = 0 kills the first-order term), which is kept because at |mu| >> spread
         it is not small against 2^-24 var:       e_var = (C_ACC sqrt(C) + 4) 2^-24 var + e_mu^2
  rstd   rsqrtf(var + eps): d rstd / d var = -rstd^3 / 2, plus the rounding of the addition (1/2 2^-24 rstd through the
         square root), of the division (1/2) and the hardware reciprocal square root (1 ulp = 2 2^-24), rounded up:
                                                  e_rstd = rstd^3 / 2 e_var + 4 2^-24 rstd
  y      attn_ref.layernorm_ref; the saved pre-activation carries the same bound, and the fused GELU the terms of
         gemm_ref (GELU_LIP on the incoming error, ERFC_ABS |v| for the A&S erfc, a few f32 roundings).

Backward (ln_bwd_kernel, ln_bwd2_kernel), with d = dy gelu'(y_pre), xh = (x - mean) rstd, g = d gamma,
s1 = mean_c g, s2 = mean_c g xh:
  dx = rstd (g - s1 - xh s2) + dres      dgamma = sum_r d xh      dbeta = sum_r d
  dz[zmap[r]] = keep(seed, tag, r C + c) dx / (1 - p) zscale[r // rps]
  e_xh = 2 2^-24 (|xh| + |mean| rstd)             covers both forms: (x - mean) rstd and fma(x, rstd, -(mean rstd))
  e_d  = ERFC_ABS |dy| + 4 2^-24 |d|              (GELU only, else 0)
  e_g  = 2^-24 |g| + |gamma| e_d
  e_s1 = C_ACC 2^-24 sqrt(C) mean|g| + mean e_g
  e_s2 = C_ACC 2^-24 sqrt(C) mean|g xh| + mean(|g| e_xh + e_g |xh|)
  e_dx = rstd (e_g + e_s1 + |xh| e_s2 + |s2| e_xh + 3 2^-24 (|g| + |s1| + |xh s2|))
         + 2 2^-24 |rstd core| + 2^-24 |dx| + U_OUT |dx|
  e_dgamma = (C_ACC sqrt(R) + 1) 2^-24 sum_r |d xh| + sum_r (|d| e_xh + e_d |xh|)
  e_dbeta  = C_ACC 2^-24 sqrt(R) sum_r |d| + sum_r e_d
  e_dz = keep |zscale| / (1 - p) (e_dx - U_OUT |dx|) + (2 2^-24 + U_OUT) |dz|     (dz is formed from the f32 dx: the
         rounding of the stored dx is not in it, its own is)
R is the number of rows summed.  accumulate adds the previous content and 2^-24 |result|.  Every reported bound is SAFETY
times the estimate.  tests/test_ln_bound_cpu.py proves on the host that an f32 emulation of the kernels stays inside the
bounds and that local damage (one lane's chunk, one row, one partial block) is rejected with its place named."""
import math

import torch

from attn_ref import C_ACC, SAFETY, U32, U_BF16, keep_ref, layernorm_ref
from gemm_ref import ERFC_ABS, GELU_LIP, check_bound, gelu64, gelu_grad64  # noqa: F401  (check_bound re-exported)

EPS = float(torch.tensor(1e-5, dtype=torch.float32))        # the f32 eps the kernels add
FAMILIES = ("plain", "offset", "edge")
FWD_WIDTHS = (32, 64, 96, 100, 128, 192, 256, 384, 512, 516, 768, 1024, 1028, 1536, 2048)
BWD2_WIDTHS = (64, 96, 128, 192, 256, 384, 512, 768, 1024)
GENERAL_BF16_WIDTHS = (32, 100, 516, 1028, 1536, 2048)
MERGE_GRIDS = ((6, 4), (14, 14))
MAX_PARTS = 512                 # partial parameter-gradient rows of one backward launch (mvlt_layernorm_bwd_workspace_rows)


def ln_class(C):
    """(lanes per row, 4-element chunks per lane) of the instantiation a width takes (the dispatch table of norm.hip)."""
    if C in (96, 192, 384):
        return C // 12, 3
    if C <= 256:
        return (16 if C <= 64 else 32 if C <= 128 else 64), 1
    return 64, (2 if C <= 512 else 3 if C <= 768 else 4 if C <= 1024 else 6 if C <= 1536 else 8)


def rows_per_block(C, waves=4):
    return waves * (64 // ln_class(C)[0])


def bwd_nparts(rows, C, waves=4):
    return min(MAX_PARTS, -(-rows // rows_per_block(C, waves)))


def fwd_row_counts(C):
    rpb = rows_per_block(C)
    return sorted({1, rpb - 1, rpb + 1, 263})


def u_out(dtype):
    return U32 if dtype == torch.float32 else U_BF16


# ------------------------------------------------------------------ operands
def ln_x(family, rows, C, dtype, seed):
    """plain: randn 2.  offset: 0.25 randn + 30 randn(rows, 1), rows whose mean is large against their spread.
    edge: plain with row 0 all zeros (a padded position: rstd = eps^-1/2), row 1 constant 3.0, row 2 a single non-zero
    element, row 3 scaled by 1e-3."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, C, generator=g)
    if family == "offset":
        x = 0.25 * x + 30.0 * torch.randn(rows, 1, generator=g)
    else:
        x = 2.0 * x
        if family == "edge":
            x[0] = 0.0
            if rows > 1:
                x[1] = 3.0
            if rows > 2:
                x[2] = 0.0
                x[2, (5 * C) // 7] = 1.5
            if rows > 3:
                x[3] *= 1e-3
        else:
            assert family == "plain", family
    return x.to(dtype)


def ln_params(C, seed):
    g = torch.Generator().manual_seed(seed)
    return 1.0 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)


def ln_rand(shape, dtype, seed, scale=1.0):
    return (scale * torch.randn(*shape, generator=torch.Generator().manual_seed(seed))).to(dtype)


def merge_index(B, H, W, Cq, device="cpu"):
    """[B H/2 W/2, 4 Cq] flat element offsets into the un-merged [B, H W, Cq] tensor: PatchMerging's
    cat(x[0::2, 0::2], x[1::2, 0::2], x[0::2, 1::2], x[1::2, 1::2]) as the oracle states it."""
    ar = torch.arange(B * H * W * Cq, device=device).view(B, H, W, Cq)
    cat = torch.cat([ar[:, 0::2, 0::2], ar[:, 1::2, 0::2], ar[:, 0::2, 1::2], ar[:, 1::2, 1::2]], -1)
    return cat.reshape(-1, 4 * Cq)


def valid_rows(rows, rows_dev):
    """Rows a launch touches for a device-side count: min(rows, max(count, 0)); None: all."""
    return rows if rows_dev is None else min(rows, max(int(rows_dev), 0))


def sum_parts(parts):
    """dy of a dy_parts launch, exactly: the parts added in f32 in part order, rounded to bf16 once."""
    acc = parts[0].float()
    for p in parts[1:]:
        acc = acc + p.float()
    return acc.to(torch.bfloat16)


# ------------------------------------------------------------------ forward
def stats_ref(x, eps=EPS):
    """float64 mean / rstd [rows] of the rows of x and their bounds."""
    x = x.double()
    C = x.shape[1]
    mu = x.mean(1)
    var = ((x - mu[:, None]) ** 2).mean(1)
    rstd = 1.0 / torch.sqrt(var + eps)
    sq = C_ACC * math.sqrt(C)
    e_mu = sq * U32 * x.abs().mean(1) + U32 * mu.abs()
    e_var = (sq + 4.0) * U32 * var + e_mu ** 2
    e_rstd = 0.5 * rstd ** 3 * e_var + 4 * U32 * rstd
    return mu, rstd, SAFETY * e_mu + 1e-30, SAFETY * e_rstd + 1e-30


def fwd_ref(x, gamma, beta, dtype, eps=EPS, gelu=False):
    """x: the logical rows [rows, C] (after a merge gather).  Returns a dict: y / y_b, mean / mean_b, rstd / rstd_b and,
    with gelu, pre / pre_b (y is then GELU of the f32 LayerNorm value)."""
    mu, rstd, mu_b, rstd_b = stats_ref(x, eps)
    y, y_b = layernorm_ref(x, gamma, beta, eps, out_dtype=dtype)
    r = dict(mean=mu, mean_b=mu_b, rstd=rstd, rstd_b=rstd_b, y=y, y_b=y_b)
    if gelu:
        _, b32 = layernorm_ref(x, gamma, beta, eps, out_dtype=torch.float32)
        g = gelu64(y)
        r.update(pre=y, pre_b=y_b, y=g,
                 y_b=GELU_LIP * b32 + SAFETY * (ERFC_ABS * y.abs() + (4 * U32 + u_out(dtype)) * g.abs()) + 1e-30)
    return r


# ------------------------------------------------------------------ backward
def bwd_ref(x, dy, mean, rstd, gamma, dtype, *, y_pre=None, dres=None, prev=None, keep=None, p=0.0, zscale=None):
    """All row operands are the LOGICAL rows [R, C] the launch sums over: x and dres after a merge gather, dy and y_pre
    gathered by dy_rowmap, only the rows below the device count.  mean, rstd [R]: what the kernel is handed.
    prev = (dgamma, dbeta) previous content for accumulate.  keep [R, C] 0/1 (keep_ref at r C + c), p, zscale [R]
    (zscale[r // rps]) describe the branch output.  Returns a dict of float64 values and bounds:
    dx, dx_b [R, C]; dg, dg_b, db, db_b [C]; dz, dz_b [R, C] in x-row order (the caller scatters by zmap)."""
    x, dy, gam = x.double(), dy.double(), gamma.double().to(x.device)
    R, C = x.shape
    mean, rstd = mean.double()[:, None], rstd.double()[:, None]
    uo = u_out(dtype)
    sqC, sqR = C_ACC * math.sqrt(C), C_ACC * math.sqrt(max(R, 1))
    if y_pre is not None:
        d = dy * gelu_grad64(y_pre.double())
        e_d = ERFC_ABS * dy.abs() + 4 * U32 * d.abs()
    else:
        d, e_d = dy, torch.zeros_like(dy)
    xh = (x - mean) * rstd
    e_xh = 2 * U32 * (xh.abs() + mean.abs() * rstd)
    g = d * gam
    e_g = U32 * g.abs() + gam.abs() * e_d
    m = lambda t: t.mean(1, keepdim=True)  # noqa: E731
    s1, s2 = m(g), m(g * xh)
    e_s1 = sqC * U32 * m(g.abs()) + m(e_g)
    e_s2 = sqC * U32 * m((g * xh).abs()) + m(g.abs() * e_xh + e_g * xh.abs())
    core = g - s1 - xh * s2
    dx = rstd * core
    if dres is not None:
        dx = dx + dres.double()
    e_f32 = rstd * (e_g + e_s1 + xh.abs() * e_s2 + s2.abs() * e_xh + 3 * U32 * (g.abs() + s1.abs() + (xh * s2).abs())) \
        + 2 * U32 * (rstd * core).abs() + U32 * dx.abs()
    e_dx = e_f32 + uo * dx.abs()
    dg, db = (d * xh).sum(0), d.sum(0)
    e_dg = (sqR + 1) * U32 * (d * xh).abs().sum(0) + (d.abs() * e_xh + e_d * xh.abs()).sum(0)
    e_db = sqR * U32 * d.abs().sum(0) + e_d.sum(0)
    if prev is not None:
        pg, pb = prev[0].double().to(x.device), prev[1].double().to(x.device)
        dg, db = dg + pg, db + pb
        e_dg, e_db = e_dg + U32 * dg.abs(), e_db + U32 * db.abs()
    out = dict(dx=dx, dx_b=SAFETY * e_dx + 1e-30, dg=dg, dg_b=SAFETY * e_dg + 1e-30, db=db, db_b=SAFETY * e_db + 1e-30)
    if keep is not None or zscale is not None:
        f = torch.ones_like(dx) if keep is None else keep.double().to(x.device) / (1.0 - p)
        if zscale is not None:
            f = f * zscale.double().to(x.device)[:, None]
        dz = dx * f
        out.update(dz=dz, dz_b=SAFETY * (f.abs() * e_f32 + (2 * U32 + uo) * dz.abs()) + 1e-30)
    else:
        out.update(dz=dx, dz_b=out["dx_b"])
    return out


def bwd_row_counts_768():
    """Rows at C = 768 (one row per wave, four per block) whose launches write nparts = 1, 15, 16, 17, 48, 49, 64, 65 and
    113 partial rows with a ragged last block: both loops of the reduce kernels on either side of i + 48 < nparts."""
    return [4 * n - 3 for n in (1, 15, 16, 17, 48, 49, 64, 65, 113)]


BWD_CAPPED = ((2069, 768), (16384 + 37, 96), (4096 + 21, 384))     # past the 512-block cap: several row groups per wave


def check_untouched(out, first, fill, what):
    """Rows first .. of `out` must still hold `fill` bit for bit (NaN: any NaN); a failure names the first row written."""
    tail = out[first:]
    if tail.numel() == 0:
        return
    tail = tail.reshape(tail.shape[0], -1)
    same = torch.isnan(tail) if fill != fill else tail == fill
    if not bool(same.all()):
        r = int((~same).any(1).nonzero()[0])
        raise AssertionError(f"{what}: row {first + r} was written ({int((~same).sum())} elements lost the fill {fill})")


def dropout_keep(seed, tag, p, R, C, device="cpu"):
    """keep [R, C] at the documented index r C + c (r: the x row)."""
    return keep_ref(seed, tag, torch.arange(R * C, dtype=torch.int64, device=device), p).view(R, C)
