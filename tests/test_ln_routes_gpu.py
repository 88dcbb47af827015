"""Every LayerNorm route of csrc/norm.hip against the float64 reference of tests/ln_ref.py with a PER-ELEMENT bound:
y, y_pre, mean and rstd of the forward; dx, dz, dgamma and dbeta of the backward.

The launches go through the C ABI structs directly, so every output buffer can start from a sentinel (7.0; NaN for mean
and rstd) and whatever a launch must not touch is compared bit for bit.  The backward is handed the float64 stats rounded
to f32 (the forward's own stats are judged in the forward tests) and its reference is taken from exactly those values.
Case ids name the kernel a case targets: ln_bwd2<LPR,NV> (the low-footprint bf16 kernel), ln_bwd2-parts, ln_bwd (the
general kernel: f32, GELU, patch-merge, widths that do not fill the lanes, NV > 4).  Row counts come from the launch
arithmetic (ln_ref.bwd_row_counts_768, BWD_CAPPED), not from the workload.  The two process-wide A/B switches run in a
fresh child each (tests/ln_switch_worker.py) over the same bf16 backward cases.  The worst ratio to the bound per
route and output is printed by the last test (-s)."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

import ln_ref as R
from ln_ref import check_bound, check_untouched

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
NAN = float("nan")
FILL = 7.0
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_UNSUPPORTED = -1, -3
WORST = {}                      # (route, output) -> worst |out - ref| / bound
DROP = (0.1, 0x1234567, 9)      # p, seed, tag of the branch dropout
ROWSCALE = (0.5, 1.0, 0.0, 2.0, 1.25)
# what the models launch: swin.py (norm2: dres + scattered, DropPath-scaled branch; norm1: gathered dy + dres), bert.py
COMBOS = {
    "dres+branch-map-scale": dict(dres=True, branch="map+scale"),
    "rowmap+dres": dict(rowmap=True, dres=True),
    "branch-dropout+rows_dev": dict(branch="dropout", short=9),              # rows_dev = rows - 9: inside the last blocks
}


@pytest.fixture(scope="module")
def ops():
    from mvlt_amd import ops as o
    return o


@pytest.fixture(scope="module")
def L():
    from mvlt_amd import _lib
    _lib.lib()
    return _lib


def tname(dt):
    return "bf16" if dt == BF else "f32"


def bwd2_name(C):
    return "ln_bwd2<%d,%d>" % R.ln_class(C)


def checked(route, what, out, ref, bound):
    out = out.double()
    if out.numel():
        r = float(torch.where(torch.isfinite(out), (out - ref).abs() / bound, torch.full_like(ref, float("inf"))).max())
        WORST[(route, what)] = max(WORST.get((route, what), 0.0), r)
    check_bound(out, ref, bound, f"{route} {what}")


def ptr(t):
    return None if t is None else t.data_ptr()


def i32(v):
    return torch.tensor([v], dtype=torch.int32, device="cuda")


def perm32(n, seed):
    return torch.randperm(n, generator=torch.Generator().manual_seed(seed)).int().cuda()


# ------------------------------------------------------------------ launches
def launch_fwd(L, ops, x, gamma, beta, y, rows, C, *, mean=None, rstd=None, y_pre=None, out_rowmap=None, merge=None,
               gelu=False, rows_dev=None):
    p = L.MvltLayerNorm()
    p.dtype, p.rows, p.C, p.eps = ops._DT[x.dtype], rows, C, R.EPS
    p.x, p.gamma, p.beta, p.y = ptr(x), ptr(gamma), ptr(beta), ptr(y)
    p.y_pre, p.mean, p.rstd, p.out_rowmap, p.rows_dev = ptr(y_pre), ptr(mean), ptr(rstd), ptr(out_rowmap), ptr(rows_dev)
    p.gelu = int(gelu)
    if merge is not None:
        p.merge_H, p.merge_W = merge
    return L.lib().mvlt_layernorm_fwd(ctypes.byref(p), ops._stream())


def launch_bwd(L, ops, dy, x, mean, rstd, gamma, dx, dgamma, dbeta, rows, C, *, dy_rowmap=None, y_pre=None, dres=None,
               merge=None, accumulate=False, dz=None, zmap=None, zscale=None, dropout=None, rows_dev=None, parts=0):
    lib = L.lib()
    ws = ops.workspace("ln_bwd", 2 * lib.mvlt_layernorm_bwd_workspace_rows() * C * 4, x.device)
    p = L.MvltLayerNormBwd()
    p.dtype, p.rows, p.C = ops._DT[x.dtype], rows, C
    p.dy, p.dy_rowmap, p.x, p.mean, p.rstd, p.gamma = ptr(dy), ptr(dy_rowmap), ptr(x), ptr(mean), ptr(rstd), ptr(gamma)
    p.y_pre, p.gelu, p.dres, p.dx = ptr(y_pre), int(y_pre is not None), ptr(dres), ptr(dx)
    if merge is not None:
        p.merge_H, p.merge_W = merge
    p.dgamma, p.dbeta, p.accumulate, p.workspace = ptr(dgamma), ptr(dbeta), int(accumulate), ptr(ws)
    p.dz, p.dz_rowmap, p.rows_dev = ptr(dz), ptr(zmap), ptr(rows_dev)
    if zscale is not None:
        p.dz_rowscale, p.dz_rows_per_scale = ptr(zscale[0]), zscale[1]
    if dropout is not None:
        p.dz_dropout_p, p.seed, p.tag = dropout
    if parts > 1:
        p.dy_parts, p.dy_part_stride = parts, dy.stride(0)
    return lib.mvlt_layernorm_bwd(ctypes.byref(p), ops._stream())


# ------------------------------------------------------------------ forward
def fwd_case(L, ops, route, C, rows, dt, family, *, rowmap=False, gelu=False, merge=None, rows_dev=None, seed=0):
    gamma, beta = (t.cuda() for t in R.ln_params(C, 100 + C))
    logical = R.ln_x(family, rows, C, dt, seed + 1).cuda()
    if merge is not None:
        H, W = merge
        B = rows // ((H // 2) * (W // 2))
        idx = R.merge_index(B, H, W, C // 4, "cuda")
        x = torch.empty(B, H * W, C // 4, dtype=dt, device="cuda")
        x.view(-1)[idx.reshape(-1)] = logical.reshape(-1)
    else:
        x = logical
    y = torch.full((rows, C), FILL, dtype=dt, device="cuda")
    pre = torch.full((rows, C), FILL, dtype=dt, device="cuda") if gelu else None
    mean = torch.full((rows,), NAN, device="cuda")
    rstd = torch.full((rows,), NAN, device="cuda")
    perm = perm32(rows, seed + 2) if rowmap else None
    rc = launch_fwd(L, ops, x, gamma, beta, y, rows, C, mean=mean, rstd=rstd, y_pre=pre, out_rowmap=perm, merge=merge,
                    gelu=gelu, rows_dev=None if rows_dev is None else i32(rows_dev))
    assert rc == 0, (route, rc)
    n = R.valid_rows(rows, rows_dev)
    ref = R.fwd_ref(logical[:n], gamma, beta, dt, gelu=gelu)
    order = perm.long() if rowmap else torch.arange(rows, device="cuda")
    checked(route, "mean", mean[:n], ref["mean"], ref["mean_b"])
    checked(route, "rstd", rstd[:n], ref["rstd"], ref["rstd_b"])
    checked(route, f"y {tname(dt)}", y[order[:n]], ref["y"], ref["y_b"])
    check_untouched(y[order], n, FILL, f"{route} y")
    check_untouched(mean, n, NAN, f"{route} mean")
    check_untouched(rstd, n, NAN, f"{route} rstd")
    if gelu:
        checked(route, f"y_pre {tname(dt)}", pre[order[:n]], ref["pre"], ref["pre_b"])
        check_untouched(pre[order], n, FILL, f"{route} y_pre")


@pytest.mark.parametrize("dt", [F32, BF], ids=tname)
@pytest.mark.parametrize("C", R.FWD_WIDTHS)
def test_forward_widths(L, ops, C, dt):
    route = "ln_fwd<%d,%d>" % R.ln_class(C)
    for family in R.FAMILIES:
        for rows in R.fwd_row_counts(C):
            fwd_case(L, ops, route, C, rows, dt, family, seed=rows)
    fwd_case(L, ops, route, C, 263, dt, "offset", rowmap=True, seed=5)
    fwd_case(L, ops, route + "-gelu", C, 263, dt, "plain", rowmap=True, gelu=True, seed=6)


@pytest.mark.parametrize("dt", [F32, BF], ids=tname)
@pytest.mark.parametrize("C", [64, 384])
@pytest.mark.parametrize("grid", R.MERGE_GRIDS, ids=lambda g: "%dx%d" % g)
def test_forward_merge(L, ops, grid, C, dt):
    rows = 2 * (grid[0] // 2) * (grid[1] // 2)
    for family in R.FAMILIES:
        fwd_case(L, ops, "ln_fwd-merge", C, rows, dt, family, merge=grid, seed=7)


@pytest.mark.parametrize("dt", [F32, BF], ids=tname)
@pytest.mark.parametrize("C", [96, 768])
def test_forward_rows_dev(L, ops, C, dt):
    rows = 263
    for count in (0, 1, rows - 1, rows + 5, -3):
        fwd_case(L, ops, "ln_fwd-rows_dev", C, rows, dt, "plain", rowmap=True, rows_dev=count, seed=8)


def test_forward_refusals(L, ops):
    """A width beyond the table, a width that is no multiple of 4 and a merge grid with an odd side: the documented error,
    and nothing written."""
    for C, merge, rows, want in ((2052, None, 9, ERR_UNSUPPORTED), (30, None, 9, ERR_ARG), (64, (7, 4), 12, ERR_ARG)):
        x = R.ln_rand((rows, C), BF, 1).cuda()
        gamma, beta = (t.cuda() for t in R.ln_params(C, 2))
        y = torch.full((rows, C), FILL, dtype=BF, device="cuda")
        mean, rstd = torch.full((rows,), NAN, device="cuda"), torch.full((rows,), NAN, device="cuda")
        rc = launch_fwd(L, ops, x, gamma, beta, y, rows, C, mean=mean, rstd=rstd, merge=merge)
        torch.cuda.synchronize()
        assert rc == want, (C, merge, rc)
        check_untouched(y, 0, FILL, "refused y")
        check_untouched(mean, 0, NAN, "refused mean")
        check_untouched(rstd, 0, NAN, "refused rstd")


# ------------------------------------------------------------------ backward
def bwd_case(L, ops, route, C, rows, dt, family="plain", *, rowmap=False, dres=False, branch=None, count=None,
             gelu=False, merge=None, parts=0, accumulate=False, seed=0):
    """One backward launch against ln_ref.bwd_ref.  rowmap: dy (and y_pre) gathered by a permutation; branch: None,
    'map+scale' (dz scattered by a second permutation and scaled per row group) or 'dropout'; count: the device-side row
    count handed over as rows_dev (None: no pointer)."""
    gamma = R.ln_params(C, 100 + C)[0].cuda()
    logical = R.ln_x(family, rows, C, dt, seed + 1).cuda()
    idx = None
    if merge is not None:
        H, W = merge
        B = rows // ((H // 2) * (W // 2))
        idx = R.merge_index(B, H, W, C // 4, "cuda")
        x = torch.empty(B, H * W, C // 4, dtype=dt, device="cuda")
        x.view(-1)[idx.reshape(-1)] = logical.reshape(-1)
    else:
        x = logical
    if parts:
        dy = R.ln_rand((parts, rows, C), BF, seed + 2, parts ** -0.5).cuda()
        dy_eff = R.sum_parts(list(dy))
    else:
        dy = dy_eff = R.ln_rand((rows, C), dt, seed + 2).cuda()
    dr = R.ln_rand((rows, C), dt, seed + 3).cuda() if dres else None
    ypre = R.ln_rand((rows, C), dt, seed + 4, 1.5).cuda() if gelu else None
    perm = perm32(rows, seed + 5) if rowmap else None
    mu, rs, _, _ = R.stats_ref(logical)
    mean, rstd = mu.float(), rs.float()
    dx = torch.full_like(x, FILL)
    prev = None
    if accumulate:
        prev = (R.ln_rand((C,), F32, seed + 6, 30.0).cuda(), R.ln_rand((C,), F32, seed + 7, 30.0).cuda())
        dg, db = prev[0].clone(), prev[1].clone()
    else:
        dg, db = torch.full((C,), FILL, device="cuda"), torch.full((C,), FILL, device="cuda")
    dz = zmap = zscale = dropout = None
    if branch is not None:
        dz = torch.full((rows, C), FILL, dtype=dt, device="cuda")
        if branch == "map+scale":
            zmap = perm32(rows, seed + 8)
            zscale = (torch.tensor(ROWSCALE, device="cuda"), (rows + 4) // 5)
        else:
            dropout = DROP
    rc = launch_bwd(L, ops, dy, x, mean, rstd, gamma, dx, dg, db, rows, C, dy_rowmap=perm, y_pre=ypre, dres=dr, merge=merge,
                    accumulate=accumulate, dz=dz, zmap=zmap, zscale=zscale, dropout=dropout,
                    rows_dev=None if count is None else i32(count), parts=parts)
    assert rc == 0, (route, rc)
    n = R.valid_rows(rows, count)
    src = perm.long()[:n] if rowmap else slice(0, n)
    keep = zs = None
    if dropout is not None:
        keep = R.dropout_keep(DROP[1], DROP[2], DROP[0], rows, C, "cuda")[:n]
    if zscale is not None:
        zs = zscale[0][torch.arange(n, device="cuda") // zscale[1]]
    ref = R.bwd_ref(logical[:n], dy_eff[src], mean[:n], rstd[:n], gamma, dt, y_pre=None if ypre is None else ypre[src],
                    dres=None if dr is None else dr[:n], prev=prev, keep=keep, p=DROP[0] if keep is not None else 0.0, zscale=zs)
    got = dx if idx is None else dx.view(-1)[idx.reshape(-1)].view(rows, C)
    t = tname(dt)
    checked(route, f"dx {t}", got[:n], ref["dx"], ref["dx_b"])
    check_untouched(got, n, FILL, f"{route} dx")
    if dz is not None:
        order = zmap.long() if zmap is not None else torch.arange(rows, device="cuda")
        checked(route, f"dz {t}", dz[order[:n]], ref["dz"], ref["dz_b"])
        check_untouched(dz[order], n, FILL, f"{route} dz")
    checked(route, "dgamma", dg, ref["dg"], ref["dg_b"])
    checked(route, "dbeta", db, ref["db"], ref["db_b"])
    if n == 0 and not accumulate:
        assert not dg.any() and not db.any(), f"{route}: dgamma / dbeta must be exactly 0 with no valid row"


def bwd_widths(L, ops, route, C, dt):
    """One width through the three operand combinations of the models, every input family, and the row counts around
    one block."""
    rpb = R.rows_per_block(C)
    for kw in COMBOS.values():
        kw = dict(kw)
        short = kw.pop("short", None)
        for family in R.FAMILIES:
            bwd_case(L, ops, route, C, 263, dt, family, seed=11, count=None if short is None else 263 - short, **kw)
        for rows in (1, rpb - 1, rpb + 1):
            bwd_case(L, ops, route, C, rows, dt, "edge", seed=12, count=None if short is None else max(rows - short, 1), **kw)


@pytest.mark.parametrize("C", R.BWD2_WIDTHS, ids=bwd2_name)
def test_backward_bwd2(L, ops, C):
    bwd_widths(L, ops, bwd2_name(C), C, BF)


@pytest.mark.parametrize("parts", [2, 3, 4])
@pytest.mark.parametrize("C", [96, 384])
def test_backward_bwd2_parts(L, ops, C, parts):
    for family in R.FAMILIES:
        bwd_case(L, ops, "ln_bwd2-parts", C, 263, BF, family, rowmap=True, dres=True, parts=parts, seed=13)
    bwd_case(L, ops, "ln_bwd2-parts", C, R.rows_per_block(C) + 1, BF, "plain", rowmap=True, dres=True, parts=parts, seed=14)


@pytest.mark.parametrize("C,dt", [(1536, BF), (384, F32)], ids=["bf16-1536", "f32-384"])
def test_backward_parts_refused(L, ops, C, dt):
    """dy_parts outside the low-footprint kernel: MVLT_ERR_UNSUPPORTED, nothing launched, dx untouched."""
    rows = 37
    x = R.ln_x("plain", rows, C, dt, 1).cuda()
    dy = R.ln_rand((2, rows, C), dt, 2).cuda()
    mu, rs, _, _ = R.stats_ref(x)
    dx = torch.full_like(x, FILL)
    dg, db = torch.full((C,), FILL, device="cuda"), torch.full((C,), FILL, device="cuda")
    rc = launch_bwd(L, ops, dy, x, mu.float(), rs.float(), R.ln_params(C, 3)[0].cuda(), dx, dg, db, rows, C, parts=2)
    torch.cuda.synchronize()
    assert rc == ERR_UNSUPPORTED, rc
    check_untouched(dx, 0, FILL, "refused dx")
    check_untouched(dg, 0, FILL, "refused dgamma")
    check_untouched(db, 0, FILL, "refused dbeta")


@pytest.mark.parametrize("C,dt", [(C, F32) for C in R.FWD_WIDTHS] + [(C, BF) for C in R.GENERAL_BF16_WIDTHS],
                         ids=lambda v: str(v) if isinstance(v, int) else tname(v))
def test_backward_general(L, ops, C, dt):
    bwd_widths(L, ops, "ln_bwd-" + tname(dt), C, dt)


@pytest.mark.parametrize("dt", [F32, BF], ids=tname)
@pytest.mark.parametrize("C", [128, 384])
def test_backward_general_gelu(L, ops, C, dt):
    for family in R.FAMILIES:
        bwd_case(L, ops, "ln_bwd-gelu", C, 263, dt, family, rowmap=True, gelu=True, seed=15)


@pytest.mark.parametrize("dt", [F32, BF], ids=tname)
@pytest.mark.parametrize("C", [64, 384])
@pytest.mark.parametrize("grid", R.MERGE_GRIDS, ids=lambda g: "%dx%d" % g)
def test_backward_general_merge(L, ops, grid, C, dt):
    rows = 2 * (grid[0] // 2) * (grid[1] // 2)
    for family in R.FAMILIES:
        bwd_case(L, ops, "ln_bwd-merge", C, rows, dt, family, merge=grid, seed=16)


ROW_CASES = [(r, 768) for r in R.bwd_row_counts_768()] + list(R.BWD_CAPPED)


@pytest.mark.parametrize("dt", [BF, F32], ids=["ln_bwd2", "ln_bwd-f32"])
@pytest.mark.parametrize("rows,C", ROW_CASES)
def test_backward_row_counts(L, ops, rows, C, dt):
    """nparts on either side of the reduce kernels' loop edges with a ragged last block, and the launches past the
    512-block cap whose waves walk several row groups with a ragged last pass."""
    route = (bwd2_name(C) if dt == BF else "ln_bwd-f32") + "-rows"
    bwd_case(L, ops, route, C, rows, dt, "offset", rowmap=True, dres=True, seed=17)
    bwd_case(L, ops, route, C, rows, dt, "plain", branch="dropout", seed=18)


@pytest.mark.parametrize("dt", [BF, F32], ids=["ln_bwd2", "ln_bwd-f32"])
@pytest.mark.parametrize("C", [96, 768])
def test_backward_rows_dev(L, ops, C, dt):
    rows = 263
    route = (bwd2_name(C) if dt == BF else "ln_bwd-f32") + "-rows_dev"
    mid = 5 * R.rows_per_block(C) + R.rows_per_block(C) // 2 + 1
    for count in (0, 1, mid, rows + 5, -3):
        bwd_case(L, ops, route, C, rows, dt, "plain", dres=True, branch="map+scale", count=count, seed=19)
        bwd_case(L, ops, route, C, rows, dt, "edge", rowmap=True, branch="dropout", count=count, seed=20)


@pytest.mark.parametrize("dt", [BF, F32], ids=["ln_bwd2", "ln_bwd-f32"])
@pytest.mark.parametrize("rows,C", [(61, 768), (263, 192), (2069, 768)])
def test_backward_accumulate(L, ops, rows, C, dt):
    bwd_case(L, ops, "ln_param_reduce-accumulate", C, rows, dt, "plain", dres=True, accumulate=True, seed=21)


# ------------------------------------------------------------------ the batched parameter reduce
QUEUE_WIDTHS = (32, 96, 384, 768, 1536, 1024, 192, 1536, 768, 1028)
QUEUE_ROWS = (1, 37, 263, 530, 1031, 61, 9)


def test_reduce_queue_100_launches(L, ops):
    """100 deferred backward launches of mixed widths, dtypes and row counts, one flush (two reduce launches: 96 + 4
    items, blocks beyond a narrower item's width return early): every dgamma / dbeta inside its bound and bit-identical to
    the same launch reduced on its own.  The pool starts empty, so it grows while the queue fills; the slices handed
    out before must stay what the flush reads."""
    ops.LnReduceQueue._pool.pop(torch.cuda.current_device(), None)
    q = ops.LnReduceQueue()
    items = []
    for i in range(100):
        C, rows = QUEUE_WIDTHS[i % len(QUEUE_WIDTHS)], QUEUE_ROWS[i % len(QUEUE_ROWS)]
        dt = BF if i % 3 else F32
        x = R.ln_x(R.FAMILIES[i % 3], rows, C, dt, 300 + i).cuda()
        dy = R.ln_rand((rows, C), dt, 500 + i).cuda()
        gamma = R.ln_params(C, 700 + i)[0].cuda()
        mu, rs, _, _ = R.stats_ref(x)
        mean, rstd = mu.float(), rs.float()
        dg, db = torch.full((C,), FILL, device="cuda"), torch.full((C,), FILL, device="cuda")
        ops.layernorm_bwd(dy, x, mean, rstd, gamma, dg, db, defer=q)
        items.append((x, dy, gamma, mean, rstd, dg, db, dt))
    assert len(q.items) == 100 and getattr(q, "_keep", []), "the pool was expected to grow while the queue filled"
    torch.cuda.synchronize()
    for it in items:
        check_untouched(it[5], 0, FILL, "dgamma before the flush")
    q.flush()
    assert not q.items and q not in ops.LnReduceQueue._active
    for i, (x, dy, gamma, mean, rstd, dg, db, dt) in enumerate(items):
        ref = R.bwd_ref(x, dy, mean, rstd, gamma, dt)
        checked("ln_param_reduce_batch", "dgamma", dg, ref["dg"], ref["dg_b"])
        checked("ln_param_reduce_batch", "dbeta", db, ref["db"], ref["db_b"])
        dg1, db1 = torch.full_like(dg, FILL), torch.full_like(db, FILL)
        ops.layernorm_bwd(dy, x, mean, rstd, gamma, dg1, db1)
        assert torch.equal(dg, dg1) and torch.equal(db, db1), f"item {i} (C {x.shape[1]}, rows {x.shape[0]}): batched != single reduce"


def test_accumulate_with_defer_is_refused(L, ops):
    """The batched reduce overwrites: accumulate=True with defer= used to drop the flag silently.  Now an error, before
    anything is queued or launched."""
    rows, C = 37, 96
    x = R.ln_x("plain", rows, C, BF, 1).cuda()
    dy = R.ln_rand((rows, C), BF, 2).cuda()
    mu, rs, _, _ = R.stats_ref(x)
    dg, db = torch.full((C,), FILL, device="cuda"), torch.full((C,), FILL, device="cuda")
    dx = torch.full_like(x, FILL)
    q = ops.LnReduceQueue()
    with pytest.raises(ValueError, match="accumulate"):
        ops.layernorm_bwd(dy, x, mu.float(), rs.float(), R.ln_params(C, 3)[0].cuda(), dg, db, accumulate=True, defer=q, dx=dx)
    torch.cuda.synchronize()
    assert not q.items and q not in ops.LnReduceQueue._active
    check_untouched(dx, 0, FILL, "dx")
    check_untouched(dg, 0, FILL, "dgamma")


# ------------------------------------------------------------------ the A/B switches, one fresh child each
PF_ROWS = ((2069, 768), (4096 + 21, 768), (4096 + 21, 384), (8192 + 21, 384), (16384 + 37, 96))   # 1, 2 and 3 passes per wave


def bf16_backward_cases(L, ops, label, parts=True):
    """The bf16 backward cases of this file, for a child process that set one of the switches."""
    for C in R.BWD2_WIDTHS + R.GENERAL_BF16_WIDTHS:
        bwd_widths(L, ops, label, C, BF)
    for rows, C in ROW_CASES + [rc for rc in PF_ROWS if rc not in ROW_CASES]:
        bwd_case(L, ops, label + "-rows", C, rows, BF, "offset", rowmap=True, dres=True, seed=17)
        bwd_case(L, ops, label + "-rows", C, rows, BF, "plain", branch="dropout", seed=18)
    for C in (96, 768):
        for count in (0, 1, 5 * R.rows_per_block(C) + 3, 263 + 5, -3):
            bwd_case(L, ops, label + "-rows_dev", C, 263, BF, "plain", dres=True, branch="map+scale", count=count, seed=19)
    for C in (128, 384):
        bwd_case(L, ops, label + "-gelu", C, 263, BF, "plain", rowmap=True, gelu=True, seed=15)
    if parts:
        for C in (96, 384):
            for n in (2, 3, 4):
                bwd_case(L, ops, label + "-parts", C, 263, BF, "offset", rowmap=True, dres=True, parts=n, seed=13)


def report():
    for (route, what), v in sorted(WORST.items()):
        print(f"ln worst ratio  {route:34s} {what:12s} {v:.3f}")


@pytest.mark.parametrize("var,val", [("MVLT_LN_BWD2", "0"), ("MVLT_LN_BWD2_PF", "1")])
def test_switch_child(var, val):
    env = dict(os.environ)
    env.pop("MVLT_LN_BWD2", None)
    env.pop("MVLT_LN_BWD2_PF", None)
    env[var] = val
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "ln_switch_worker.py")], env=env, capture_output=True,
                       text=True, timeout=240)
    assert r.returncode == 0 and "LN-SWITCH-OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    print(r.stdout)


def test_report_worst_ratios():
    """Runs last: the worst ratio to the bound per route and output of the cases above (printed with -s)."""
    report()
    assert all(v <= 1.0 for v in WORST.values())
