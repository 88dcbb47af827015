"""The LayerNorm bounds of tests/ln_ref.py prove themselves on the host.

(a) an f32 emulation of the kernels' arithmetic (lane-local sums and the butterfly over a row's lanes, both forms of the
    normalised value -- (x - mean) rstd and fma(x, rstd, -(mean rstd)) --, the dy_parts sum, the parameter sums chunked
    by block and wave and folded by the reduce kernel's 16 streams of four partial rows) stays within the bound, at every
    width, row count and input family tests/test_ln_routes_gpu.py uses;
(b) local damage of the kind these kernels can suffer is rejected, and the message names its place;
(c) the whole-tensor norm the older tests use accepts that damage."""
import math

import pytest
import torch
import torch.nn.functional as F

import ln_ref as R
from ln_ref import check_bound

BF, F32 = torch.bfloat16, torch.float32
WORST = {}


@pytest.fixture(autouse=True, scope="module")
def _one_thread():
    """Thousands of small tensor operations: a thread pool only gets in their way (restored for the next module)."""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


def ratio(out, ref, bound):
    return float(((out.double() - ref).abs() / bound).max())


def note(key, out, ref, bound):
    r = ratio(out, ref, bound)
    WORST[key] = max(WORST.get(key, 0.0), r)
    return r


# ------------------------------------------------------------------ f32 emulation
def fma(a, b, c):
    return (a.double() * b.double() + c.double()).float()


def lanes(t, C):
    """[R, C] -> [R, NV, LPR, 4]: column 4 (lane + LPR j) + e, zeros where the width does not fill the lanes."""
    LPR, NV = R.ln_class(C)
    return F.pad(t, (0, 4 * LPR * NV - C)).view(t.shape[0], NV, LPR, 4)


def lane_sum(t, C, skip=None):
    """Row sums as the kernels form them: per lane over its chunks, then a butterfly over the row's lanes.
    skip = (row, lane, chunk): that chunk is left out (fault injection)."""
    v = lanes(t, C).clone()
    if skip is not None:
        v[skip[0], skip[2], skip[1]] = 0.0
    s = torch.zeros(v.shape[0], v.shape[2])
    for j in range(v.shape[1]):
        s = s + (((v[:, j, :, 0] + v[:, j, :, 1]) + v[:, j, :, 2]) + v[:, j, :, 3])
    while s.shape[1] > 1:
        h = s.shape[1] // 2
        s = s[:, :h] + s[:, h:]
    return s[:, 0]


def emu_fwd(x, gamma, beta, dtype, gelu=False, mean_from=None):
    """ln_fwd_kernel in f32.  mean_from = (row, other): row is normalised with the mean of `other` (fault)."""
    x = x.float()
    C = x.shape[1]
    mean = lane_sum(x, C) / C
    d = x - mean[:, None]
    rstd = torch.rsqrt(lane_sum(d * d, C) / C + torch.tensor(R.EPS))
    use = mean.clone()
    if mean_from is not None:
        use[mean_from[0]] = mean[mean_from[1]]
    o = (x - use[:, None]) * rstd[:, None] * gamma + beta
    pre = o.to(dtype) if gelu else None
    if gelu:
        o = F.gelu(o)
    return o.to(dtype), mean, rstd, pre


def param_sums(t, C, waves=4, drop_block=None):
    """Column sums of t [R, C] in the order a backward launch and the reduce kernel add them: a (block, wave, row slot)
    adds its rows pass by pass, the row slots fold by butterfly, the waves one after the other, and the reduce kernel
    walks the partial rows in 16 streams with four rows in flight.  drop_block: that partial row is left out (fault)."""
    n = t.shape[0]
    rpw = 64 // R.ln_class(C)[0]
    nparts = R.bwd_nparts(n, C, waves)
    stride = nparts * waves * rpw
    passes = -(-n // stride)
    t = F.pad(t, (0, 0, 0, passes * stride - n)).view(passes, nparts, waves, rpw, C)
    acc = torch.zeros(nparts, waves, rpw, C)
    for p in range(passes):
        acc = acc + t[p]
    while acc.shape[2] > 1:
        h = acc.shape[2] // 2
        acc = acc[:, :, :h] + acc[:, :, h:]
    part = acc[:, 0, 0]
    for w in range(1, waves):
        part = part + acc[:, w, 0]
    if drop_block is not None:
        part[drop_block] = 0.0
    out = torch.zeros(C)
    for w in range(16):
        g = [torch.zeros(C) for _ in range(4)]
        i = w
        while i + 48 < nparts:
            for k in range(4):
                g[k] = g[k] + part[i + 16 * k]
            i += 64
        while i < nparts:
            g[0] = g[0] + part[i]
            i += 16
        out = out + (g[0] + ((g[1] + g[2]) + g[3]))
    return out


def emu_bwd(x, dy, mean, rstd, gamma, dtype, *, form, y_pre=None, dres=None, keep=None, p=0.0, zscale=None, waves=4,
            skip_s1=None, no_dres_row=None, drop_block=None):
    """ln_bwd_kernel (form 'sub') / ln_bwd2_kernel (form 'fma') in f32; returns dx, dz (rounded to dtype), dgamma, dbeta."""
    x, d = x.float(), dy.float()
    C = x.shape[1]
    mean, rstd, gamma = mean.float()[:, None], rstd.float()[:, None], gamma.float()
    if y_pre is not None:
        yp = y_pre.float()
        d = d * (0.5 * (1 + torch.erf(yp * 0.70710678118654752)) + yp * 0.3989422804014327 * torch.exp(-0.5 * yp * yp))
    xh = (x - mean) * rstd if form == "sub" else fma(x, rstd, -(mean * rstd))
    g = d * gamma
    inv = torch.tensor(1.0) / C
    s1 = (lane_sum(g, C, skip_s1) * inv)[:, None]
    s2 = (lane_sum(g * xh, C) * inv)[:, None]
    rs = torch.zeros_like(x) if dres is None else dres.float().clone()
    if no_dres_row is not None:
        rs[no_dres_row] = 0.0
    if form == "sub":
        o = rstd * (g - s1 - xh * s2) + rs
    else:
        o = fma(rstd.expand_as(x), fma(d, gamma.expand_as(x), -s1.expand_as(x)) - xh * s2, rs)
    z = o
    if keep is not None:
        z = torch.where(keep.bool(), z * torch.tensor(1.0 / (1.0 - p)), torch.zeros_like(z))
    if zscale is not None:
        z = z * zscale.float()[:, None]
    return o.to(dtype), z.to(dtype), param_sums(d * xh, C, waves, drop_block), param_sums(d, C, waves)


# ------------------------------------------------------------------ operands of one case
def bwd_operands(family, rows, C, dtype, seed, gelu=False, parts=0):
    x = R.ln_x(family, rows, C, dtype, seed)
    gamma, _ = R.ln_params(C, seed + 1)
    if parts:
        dy = R.sum_parts(R.ln_rand((parts, rows, C), BF, seed + 2, 1.0 / math.sqrt(parts)))
    else:
        dy = R.ln_rand((rows, C), dtype, seed + 2)
    dres = R.ln_rand((rows, C), dtype, seed + 3)
    ypre = R.ln_rand((rows, C), dtype, seed + 4, 1.5) if gelu else None
    mu, rstd, _, _ = R.stats_ref(x)
    return x, gamma, dy, dres, ypre, mu.float(), rstd.float()


def check_bwd_emulation(key, family, rows, C, dtype, gelu=False, parts=0, waves=4):
    x, gamma, dy, dres, ypre, mean, rstd = bwd_operands(family, rows, C, dtype, 50 + C, gelu, parts)
    keep = R.dropout_keep(11, 5, 0.1, rows, C)
    zs = torch.tensor([0.5, 1.0, 0.0, 2.0, 1.25])[torch.arange(rows) // ((rows + 4) // 5)]
    ref = R.bwd_ref(x, dy, mean, rstd, gamma, dtype, y_pre=ypre, dres=dres, keep=keep, p=0.1, zscale=zs)
    worst = 0.0
    for form in ("sub", "fma"):
        dx, dz, dg, db = emu_bwd(x, dy, mean, rstd, gamma, dtype, form=form, y_pre=ypre, dres=dres, keep=keep, p=0.1,
                                 zscale=zs, waves=waves)
        tag = "bf16" if dtype == BF else "f32"
        worst = max(worst, note(f"dx {tag}", dx, ref["dx"], ref["dx_b"]), note(f"dz {tag}", dz, ref["dz"], ref["dz_b"]),
                    note("dgamma", dg, ref["dg"], ref["dg_b"]), note("dbeta", db, ref["db"], ref["db_b"]))
    assert worst <= 1.0, (key, family, rows, C, dtype, worst)


# ------------------------------------------------------------------ (a) the emulation is inside the bound
@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("C", R.FWD_WIDTHS)
def test_forward_emulation_within_bound(C, dtype):
    gamma, beta = R.ln_params(C, 3)
    tag = "bf16" if dtype == BF else "f32"
    for family in R.FAMILIES:
        for rows in R.fwd_row_counts(C):
            x = R.ln_x(family, rows, C, dtype, 7 + rows)
            for gelu in (False, True):
                y, mean, rstd, pre = emu_fwd(x, gamma, beta, dtype, gelu)
                ref = R.fwd_ref(x, gamma, beta, dtype, gelu=gelu)
                rs = [note(f"y {tag}", y, ref["y"], ref["y_b"]), note("mean", mean, ref["mean"], ref["mean_b"]),
                      note("rstd", rstd, ref["rstd"], ref["rstd_b"])]
                if gelu:
                    rs.append(note(f"y_pre {tag}", pre, ref["pre"], ref["pre_b"]))
                assert max(rs) <= 1.0, (family, rows, C, gelu, rs)


@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("C", R.FWD_WIDTHS)
def test_backward_emulation_within_bound(C, dtype):
    for family in R.FAMILIES:
        for rows in R.fwd_row_counts(C):
            check_bwd_emulation("widths", family, rows, C, dtype)
    if C in (128, 384):
        check_bwd_emulation("gelu", "plain", 263, C, dtype, gelu=True)
    if C in (96, 384) and dtype == BF:
        for parts in (2, 3, 4):
            check_bwd_emulation("parts", "offset", 263, C, dtype, parts=parts)


@pytest.mark.parametrize("rows,C", [(r, 768) for r in R.bwd_row_counts_768()] + list(R.BWD_CAPPED))
def test_parameter_sums_within_bound(rows, C):
    """The launch arithmetic of the parameter gradients: every nparts on either side of the reduce kernels' loop edges,
    and the capped launches whose waves walk several row groups; 4-wave and 8-wave blocks."""
    for family in ("plain", "offset"):
        check_bwd_emulation("rows", family, rows, C, BF)
    check_bwd_emulation("rows-8-wave", "edge", rows, C, F32, waves=8)


def test_accumulate_bound_holds_previous_content():
    rows, C = 263, 192
    x, gamma, dy, dres, _, mean, rstd = bwd_operands("plain", rows, C, BF, 91)
    prev = (R.ln_rand((C,), F32, 92, 30.0), R.ln_rand((C,), F32, 93, 30.0))
    ref = R.bwd_ref(x, dy, mean, rstd, gamma, BF, dres=dres, prev=prev)
    _, _, dg, db = emu_bwd(x, dy, mean, rstd, gamma, BF, form="fma", dres=dres)
    check_bound(dg + prev[0], ref["dg"], ref["dg_b"], "dgamma")
    check_bound(db + prev[1], ref["db"], ref["db_b"], "dbeta")
    with pytest.raises(AssertionError, match="dgamma"):
        check_bound(dg, ref["dg"], ref["dg_b"], "dgamma")          # the overwrite that accumulate + defer used to do


def test_report_worst_ratios():
    """After the emulation tests above: their worst ratio to the bound per output (printed with -s)."""
    for k in sorted(WORST):
        print(f"ln bound, emulation worst ratio: {k:12s} {WORST[k]:.3f}")
    assert all(v <= 1.0 for v in WORST.values())


# ------------------------------------------------------------------ (b) injected faults are rejected, with their place
def rejected(out, ref, bound, what, row=None, cols=None):
    with pytest.raises(AssertionError) as e:
        check_bound(out, ref, bound, what)
    msg = str(e.value)
    assert what in msg, msg
    if row is not None:
        assert f"worst at row {row}," in msg, msg
    if cols is not None:
        c = int(msg.split("column ")[1].split(":")[0].split(" ")[0])
        assert c in cols, msg
    return msg


@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
def test_fault_neighbour_mean(dtype):
    C, rows, r = 768, 23, 9
    x = R.ln_x("plain", rows, C, dtype, 1)
    gamma, beta = R.ln_params(C, 2)
    ref = R.fwd_ref(x, gamma, beta, dtype)
    y, *_ = emu_fwd(x, gamma, beta, dtype)
    check_bound(y, ref["y"], ref["y_b"], "y")
    y, *_ = emu_fwd(x, gamma, beta, dtype, mean_from=(r, r + 1))
    rejected(y, ref["y"], ref["y_b"], "y", row=r)


@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("form", ["sub", "fma"])
def test_fault_chunk_missing_from_s1(dtype, form):
    C, rows, r = 768, 23, 14
    x, gamma, dy, dres, _, mean, rstd = bwd_operands("plain", rows, C, dtype, 3)
    ref = R.bwd_ref(x, dy, mean, rstd, gamma, dtype, dres=dres)
    dx, *_ = emu_bwd(x, dy, mean, rstd, gamma, dtype, form=form, dres=dres, skip_s1=(r, 37, 2))
    rejected(dx, ref["dx"], ref["dx_b"], "dx", row=r)


@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("C,cols", [(516, range(512, 516)), (100, range(96, 100)), (1028, range(1024, 1028))])
def test_fault_tail_chunk_zero(C, cols, dtype):
    rows, r = 9, 4
    x = R.ln_x("plain", rows, C, dtype, 5)
    gamma, beta = R.ln_params(C, 6)
    ref = R.fwd_ref(x, gamma, beta, dtype)
    y, *_ = emu_fwd(x, gamma, beta, dtype)
    y[r, cols[0]:] = 0.0
    rejected(y, ref["y"], ref["y_b"], "y", row=r, cols=cols)


@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
def test_fault_dres_dropped_and_rowmap_off_by_one(dtype):
    C, rows, r = 384, 41, 17
    x, gamma, dy, dres, _, mean, rstd = bwd_operands("plain", rows, C, dtype, 8)
    perm = torch.randperm(rows, generator=torch.Generator().manual_seed(9))
    ref = R.bwd_ref(x, dy[perm], mean, rstd, gamma, dtype, dres=dres)
    dx, *_ = emu_bwd(x, dy[perm], mean, rstd, gamma, dtype, form="fma", dres=dres)
    check_bound(dx, ref["dx"], ref["dx_b"], "dx")
    dx, *_ = emu_bwd(x, dy[perm], mean, rstd, gamma, dtype, form="fma", dres=dres, no_dres_row=r)
    rejected(dx, ref["dx"], ref["dx_b"], "dx", row=r)
    off = perm.clone()
    off[r] = (perm[r] + 1) % rows
    dx, *_ = emu_bwd(x, dy[off], mean, rstd, gamma, dtype, form="fma", dres=dres)
    rejected(dx, ref["dx"], ref["dx_b"], "dx", row=r)


def test_fault_partial_block_missing_from_dgamma():
    C, rows = 768, 263
    x, gamma, dy, dres, _, mean, rstd = bwd_operands("plain", rows, C, BF, 12)
    ref = R.bwd_ref(x, dy, mean, rstd, gamma, BF, dres=dres)
    _, _, dg, db = emu_bwd(x, dy, mean, rstd, gamma, BF, form="fma", dres=dres, drop_block=40)
    check_bound(db, ref["db"], ref["db_b"], "dbeta")
    rejected(dg, ref["dg"], ref["dg_b"], "dgamma")


@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
def test_fault_merge_grid_transposed(dtype):
    B, H, W, Cq = 2, 6, 4, 16
    x = R.ln_rand((B, H * W, Cq), dtype, 13, 2.0)
    gamma, beta = R.ln_params(4 * Cq, 14)
    good = x.reshape(-1)[R.merge_index(B, H, W, Cq)]
    ref = R.fwd_ref(good, gamma, beta, dtype)
    y, *_ = emu_fwd(good, gamma, beta, dtype)
    check_bound(y, ref["y"], ref["y_b"], "y")
    y, *_ = emu_fwd(x.reshape(-1)[R.merge_index(B, W, H, Cq)], gamma, beta, dtype)
    rejected(y, ref["y"], ref["y_b"], "y")


def test_fault_dropout_mask_indexed_by_dz_row():
    C, rows = 96, 37
    x, gamma, dy, dres, _, mean, rstd = bwd_operands("plain", rows, C, BF, 15)
    zmap = torch.randperm(rows, generator=torch.Generator().manual_seed(16))
    keep = R.dropout_keep(21, 4, 0.1, rows, C)
    ref = R.bwd_ref(x, dy, mean, rstd, gamma, BF, dres=dres, keep=keep, p=0.1)
    _, dz, _, _ = emu_bwd(x, dy, mean, rstd, gamma, BF, form="fma", dres=dres, keep=keep, p=0.1)
    check_bound(dz, ref["dz"], ref["dz_b"], "dz")
    _, dz, _, _ = emu_bwd(x, dy, mean, rstd, gamma, BF, form="fma", dres=dres, keep=keep[zmap], p=0.1)
    rejected(dz, ref["dz"], ref["dz_b"], "dz")


def test_fault_rows_beyond_device_count_written():
    rows, C, nv = 19, 64, 11
    assert R.valid_rows(rows, 0) == 0 and R.valid_rows(rows, -3) == 0 and R.valid_rows(rows, rows + 5) == rows
    dx = torch.full((rows, C), 7.0, dtype=BF)
    dx[:nv] = 1.0
    R.check_untouched(dx, nv, 7.0, "dx")
    dx[nv, 8:12] = 0.5
    with pytest.raises(AssertionError, match=f"dx: row {nv} was written"):
        R.check_untouched(dx, nv, 7.0, "dx")
    mean = torch.full((rows,), float("nan"))
    mean[:nv] = 0.0
    R.check_untouched(mean, nv, float("nan"), "mean")
    mean[rows - 1] = 0.0
    with pytest.raises(AssertionError, match=f"mean: row {rows - 1} was written"):
        R.check_untouched(mean, nv, float("nan"), "mean")


# ------------------------------------------------------------------ (c) the gap: what the whole-tensor norm accepts
def test_whole_tensor_norm_accepts_a_wrong_chunk():
    rows, C, r = 523, 768, 300
    x = R.ln_x("plain", rows, C, BF, 20)
    gamma, beta = R.ln_params(C, 21)
    ref = R.fwd_ref(x, gamma, beta, BF)
    y, *_ = emu_fwd(x, gamma, beta, BF)
    y[r, 4 * 61:4 * 62] = 0.0                                     # one lane's chunk of one row
    rel = float((y.double() - ref["y"]).norm() / ref["y"].norm())
    assert rel < 6e-3, rel                                        # tests/test_kernels_gpu.py: rel(a, b) < 6e-3 for bf16
    rejected(y, ref["y"], ref["y_b"], "y", row=r, cols=range(4 * 61, 4 * 62))
