"""The three entry points of csrc/seqloss.hip through the C ABI, on sentinel-filled outputs, against tests/seq_loss_ref.py:
the plan bit for bit (and against ops.label_plan on the labels it implies), mvlt_ce_bwd_weighted per element within the
reference's bound (and bit for bit against mvlt_ce_bwd_ragged at unit weights), mvlt_seq_loss_fwd within its sum bound and
reproducible, and every refusal with its outputs untouched."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import seq_loss_ref as R  # noqa: E402
from seq_loss_ref import BF, F32, check_bound, check_equal, check_untouched, check_zero  # noqa: E402

pytestmark = pytest.mark.gpu

NAN = float("nan")
FILL = 7.0
GUARD = 8
ERR_ARG = -1


@pytest.fixture(scope="module")
def ops():
    from mvlt_amd import ops as o
    return o


@pytest.fixture(scope="module")
def L():
    from mvlt_amd import _lib
    _lib.lib()
    assert _lib.ERRORS[ERR_ARG] == "MVLT_ERR_ARG"
    return _lib


def ptr(t):
    return None if t is None else t.data_ptr()


def i32(v):
    return torch.tensor([v], dtype=torch.int32, device="cuda")


def filled(shape, fill, dt=F32):
    return torch.full(shape, fill, dtype=dt, device="cuda")


# ------------------------------------------------------------------ plan
class PlanOut:
    """Sentinel-filled outputs of one plan call, each with a guard tail."""

    def __init__(self, B, T):
        n = B * T
        self.len = filled((B + GUARD,), -7, torch.int32)
        self.tf = filled((n + GUARD,), -7, torch.int64)
        self.gather = filled((n + GUARD,), -7, torch.int32)
        self.sel = filled((n + GUARD,), -7, torch.int64)
        self.rw = filled((n + GUARD,), FILL)
        self.rd = filled((1 + GUARD,), -7, torch.int32)
        self.B, self.T = B, T

    def all(self):
        return (self.len, self.tf, self.gather, self.sel, self.rw, self.rd)

    def untouched(self):
        for t in self.all():
            assert bool((t == (FILL if t.dtype == F32 else -7)).all())


def plan_call(L, ops, ids, ld, B, T, eos, w, wsb, wst, row0, step, o, over=None):
    a = dict(ids=ptr(ids), w=ptr(w), len=ptr(o.len), tf=ptr(o.tf), gather=ptr(o.gather), sel=ptr(o.sel), rw=ptr(o.rw), rd=ptr(o.rd))
    a.update(over or {})
    return L.lib().mvlt_seq_loss_plan(a["ids"], ld, B, T, eos, a["w"], wsb, wst, row0, step, a["len"], a["tf"], a["gather"],
                                      a["sel"], a["rw"], a["rd"], ops._stream())


@pytest.mark.parametrize("layout", ["b", "bt"])
@pytest.mark.parametrize("T", [1, 12, 512])
@pytest.mark.parametrize("B", [1, 3, 65])
def test_plan_equals_the_reference_and_label_plan(L, ops, B, T, layout):
    ids = R.plan_ids(B, T, seed=100 * B + T)
    ld = T + 3                                                   # a row stride of its own
    wide = torch.full((B, ld), 5, dtype=torch.int64)
    wide[:, :T] = ids
    w = R.plan_weights(B, T, layout, seed=B + T)
    row0, step = 51, 50 + T
    for eos in (R.EOS, -1):
        ref = R.plan_ref(ids, eos if eos >= 0 else None, w, row0, step)
        o = PlanOut(B, T)
        wd = w.cuda()
        rc = plan_call(L, ops, wide.cuda(), ld, B, T, eos, wd, wd.stride(0), wd.stride(1) if layout == "bt" else 0, row0, step, o)
        assert rc == 0
        n = B * T
        assert int(o.rd[0]) == ref["rows"]
        assert torch.equal(o.len[:B].cpu(), ref["len"]) and torch.equal(o.tf[:n].cpu().view(B, T), ref["tf_ids"])
        assert torch.equal(o.gather[:n].cpu(), ref["gather_row"]) and torch.equal(o.sel[:n].cpu(), ref["sel_labels"])
        check_equal(o.rw[:n].cpu(), ref["row_weight"], "row_weight")
        for t, k in ((o.len, B), (o.tf, n), (o.gather, n), (o.sel, n), (o.rd, 1)):
            assert bool((t[k:] == -7).all()), "guard tail written"
        assert bool((o.rw[n:] == FILL).all())
        # the packing is ops.label_plan's on the labels the plan implies
        lab = R.implied_labels(ids, eos if eos >= 0 else None).reshape(-1).cuda()
        text_row = (row0 + step * torch.arange(B)[:, None] + torch.arange(T)[None, :]).reshape(-1).cuda()
        g2, s2, c2 = ops.label_plan(lab, text_row)
        assert torch.equal(g2, o.gather[:n]) and torch.equal(s2, o.sel[:n]) and int(c2[0]) == int(o.rd[0])


def test_plan_keeps_a_negative_id_ahead_of_an_eos_unscored(L, ops):
    ids = torch.tensor([[5, -7, 6, R.EOS, 9], [8, 9, 0, 0, 0]], dtype=torch.int64)
    w = torch.tensor([2.0, 3.0])
    ref = R.plan_ref(ids, R.EOS, w, 10, 20)
    o = PlanOut(2, 5)
    assert plan_call(L, ops, ids.cuda(), 5, 2, 5, R.EOS, w.cuda(), 1, 0, 10, 20, o) == 0
    assert int(o.rd[0]) == ref["rows"] == 6 and o.len[:2].tolist() == [4, 2]
    assert torch.equal(o.sel[:10].cpu(), ref["sel_labels"]) and o.sel[:6].tolist() == [5, -100, 6, R.EOS, 8, 9]
    assert torch.equal(o.gather[:10].cpu(), ref["gather_row"]) and torch.equal(o.tf[:10].cpu().view(2, 5), ref["tf_ids"])
    check_equal(o.rw[:10].cpu(), ref["row_weight"], "row_weight")
    assert o.rw[:6].tolist() == [2.0, 0.0, 2.0, 2.0, 3.0, 3.0] and o.tf[:5].tolist() == [5, 0, 6, R.EOS, 0]


def test_plan_is_stateless_and_takes_a_broadcast_weight(L, ops):
    B, T = 3, 12
    ids = R.plan_ids(B, T, seed=1).cuda()
    w = torch.tensor([2.5], device="cuda")
    o = PlanOut(B, T)
    assert plan_call(L, ops, ids, T, B, T, R.EOS, w, 0, 0, 0, T, o) == 0
    first = [t.clone() for t in o.all()]
    assert plan_call(L, ops, ids, T, B, T, R.EOS, w, 0, 0, 0, T, o) == 0          # onto its own results
    for a, b in zip(first, o.all()):
        assert torch.equal(a, b)
    n = int(o.rd[0])
    assert bool((o.rw[:n] == 2.5).all()) and bool((o.rw[n:B * T] == 0).all())


def test_plan_refusals_leave_the_outputs_alone(L, ops):
    B, T = 3, 12
    ids = R.plan_ids(B, T, seed=2).cuda()
    w = torch.ones(B, device="cuda")
    o = PlanOut(B, T)
    ok = dict(ld=T, B=B, T=T, wsb=1, wst=0, row0=0, step=T)

    def call(**kw):
        over = {k: kw.pop(k) for k in list(kw) if k in ("ids", "w", "len", "tf", "gather", "sel", "rw", "rd")}
        a = dict(ok, **kw)
        return plan_call(L, ops, ids, a["ld"], a["B"], a["T"], R.EOS, w, a["wsb"], a["wst"], a["row0"], a["step"], o, over=over)

    for name in ("ids", "w", "len", "tf", "gather", "sel", "rw", "rd"):
        assert call(**{name: None}) == ERR_ARG, name
    for kw in (dict(B=0), dict(B=4097), dict(T=0), dict(T=513), dict(ld=T - 1), dict(wsb=-1), dict(wst=-1), dict(row0=-1),
               dict(step=-1), dict(row0=2 ** 31 - 5), dict(ids=ids.data_ptr() + 4), dict(tf=o.tf.data_ptr() + 4),
               dict(rw=o.rw.data_ptr() + 2)):
        assert call(**kw) == ERR_ARG, kw
    torch.cuda.synchronize()
    o.untouched()
    assert call() == 0


# ------------------------------------------------------------------ weighted backward
def bwd_call(L, ops, x, V, labels, lse, w, count, gs_dev, out, rows_dev, rows=None, ld=None, gscale=R.GSCALE, over=None):
    a = dict(x=ptr(x), labels=ptr(labels), lse=ptr(lse), w=ptr(w), count=ptr(count), out=ptr(out), gsd=ptr(gs_dev), rd=ptr(rows_dev))
    a.update(over or {})
    return L.lib().mvlt_ce_bwd_weighted(ops._DT[x.dtype], a["x"], x.stride(0) if ld is None else ld,
                                        x.shape[0] if rows is None else rows, V, a["labels"], a["lse"], a["w"], a["count"], gscale,
                                        a["gsd"], a["out"], a["rd"], ops._stream())


def bwd_operands(shape, dt, rd):
    rows, V, ld = shape
    n_valid = rows if rd is None else rd
    x, labels, w, lse, count = R.weighted_case(rows, V, ld, dt, seed=rows * V + ld, n_valid=n_valid)
    dev = [t.cuda() for t in (x, labels, w, lse)]
    return (x, labels, w, lse, count, n_valid), dev, torch.tensor([count], device="cuda"), torch.tensor([R.GSCALE_DEV], device="cuda")


@pytest.mark.parametrize("dt", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("rd_kind", ["none", "zero", "rows-2"])
@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_ce_bwd_weighted_against_the_reference(L, ops, shape, rd_kind, dt):
    rows, V, ld = shape
    rd = {"none": None, "zero": 0, "rows-2": rows - 2}[rd_kind]
    (x, labels, w, lse, count, n_valid), (xd, labd, wd, lsed), cnt, gsd = bwd_operands(shape, dt, rd)
    rows_dev = None if rd is None else i32(rd)
    out = filled((rows + GUARD, ld), FILL, dt)
    assert bwd_call(L, ops, xd, V, labd, lsed, wd, cnt, gsd, out, rows_dev) == 0
    got = out.cpu()
    dl, bound = R.weighted_dl_ref(x, V, labels, lse, w, count, R.GSCALE, R.GSCALE_DEV, dt, n_valid=n_valid)
    check_bound(got[:n_valid, :V], dl, bound, f"dlogits {shape} {dt} rows_dev={rd}")
    if n_valid:
        print(f"{shape} {dt} rows_dev={rd}: worst ratio {float(((got[:n_valid, :V].double() - dl).abs() / bound).max()):.3f}")
    check_untouched(got, n_valid, FILL, "rows at or beyond rows_dev (and the guard rows)")
    check_zero(got[:n_valid, V:], "pad columns")
    if n_valid > R.IGNORED_ROW:
        check_zero(got[R.IGNORED_ROW], "ignored row")
    if n_valid > R.ZERO_ROW:
        check_zero(got[R.ZERO_ROW], "zero-weight row holding an inf logit")
    # in place gives the same bits
    xin = xd.clone()
    assert bwd_call(L, ops, xin, V, labd, lsed, wd, cnt, gsd, xin, rows_dev) == 0
    check_equal(xin[:n_valid].cpu(), got[:n_valid], "in place against out of place")
    if n_valid < rows:
        same = xin[n_valid:].cpu().view(torch.int16 if dt == BF else torch.int32) == x[n_valid:].view(torch.int16 if dt == BF else torch.int32)
        assert bool(same.all()), "in place: a row at or beyond rows_dev was written"


@pytest.mark.parametrize("dt", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_unit_weights_give_the_bits_of_ce_bwd_ragged(L, ops, shape, dt):
    rows, V, ld = shape
    (x, labels, w, lse, count, _), (xd, labd, wd, lsed), cnt, gsd = bwd_operands(shape, dt, None)
    # finite logits everywhere: the existing kernel evaluates every labelled row
    xd = torch.where(torch.isinf(xd), torch.zeros_like(xd), xd)
    ones = torch.ones(rows, device="cuda")
    rows_dev = i32(rows - 1)
    new = filled((rows, ld), FILL, dt)
    old = filled((rows, ld), FILL, dt)
    assert bwd_call(L, ops, xd, V, labd, lsed, ones, cnt, gsd, new, rows_dev) == 0
    rc = L.lib().mvlt_ce_bwd_ragged(ops._DT[dt], ptr(xd), ld, rows, V, ptr(labd), ptr(lsed), ptr(cnt), R.GSCALE, ptr(gsd), ptr(old),
                                    ptr(rows_dev), ops._stream())
    assert rc == 0
    check_equal(new.cpu(), old.cpu(), f"weights == 1 against mvlt_ce_bwd_ragged {shape} {dt}")


def test_ce_bwd_weighted_many_rows_stride_the_grid(L, ops):
    """More rows than the 2048 row slots of the grid: the strided rows are written too (bf16, a short row)."""
    rows, V, ld = 2048 + 37, 67, 128
    g = R.gen(9)
    x = (3.0 * torch.randn(rows, ld, generator=g)).to(BF)
    labels = torch.randint(0, V, (rows,), generator=g)
    w = torch.randn(rows, generator=g)
    lse = torch.logsumexp(x[:, :V].double(), 1).float()
    out = filled((rows + GUARD, ld), FILL, BF)
    cnt, gsd = torch.tensor([float(rows)], device="cuda"), torch.tensor([R.GSCALE_DEV], device="cuda")
    assert bwd_call(L, ops, x.cuda(), V, labels.cuda(), lse.cuda(), w.cuda(), cnt, gsd, out, None) == 0
    dl, bound = R.weighted_dl_ref(x, V, labels, lse, w, float(rows), R.GSCALE, R.GSCALE_DEV, BF)
    got = out.cpu()
    check_bound(got[:rows, :V], dl, bound, "2085 rows")
    check_zero(got[:rows, V:], "pad columns")
    check_untouched(got, rows, FILL, "guard rows")


def test_ce_bwd_weighted_refusals_leave_the_output_alone(L, ops):
    shape = R.SHAPES[0]
    rows, V, ld = shape
    _, (xd, labd, wd, lsed), cnt, gsd = bwd_operands(shape, BF, None)
    out = filled((rows + GUARD, ld), FILL, BF)
    for name in ("x", "labels", "lse", "w", "count", "out"):
        assert bwd_call(L, ops, xd, V, labd, lsed, wd, cnt, gsd, out, None, over={name: None}) == ERR_ARG, name
    assert bwd_call(L, ops, xd, V, labd, lsed, wd, cnt, gsd, out, None, rows=0) == ERR_ARG
    assert bwd_call(L, ops, xd, 0, labd, lsed, wd, cnt, gsd, out, None) == ERR_ARG
    assert bwd_call(L, ops, xd, V, labd, lsed, wd, cnt, gsd, out, None, ld=V - 1) == ERR_ARG
    # misaligned vector operands: ld is a multiple of 16 bytes, the bases are not
    assert bwd_call(L, ops, xd, V, labd, lsed, wd, cnt, gsd, out, None, over={'x': xd.data_ptr() + 2}) == ERR_ARG
    assert bwd_call(L, ops, xd, V, labd, lsed, wd, cnt, gsd, out, None, over={'out': out.data_ptr() + 8}) == ERR_ARG
    assert bwd_call(L, ops, xd, V, labd, lsed, wd, cnt, gsd, out, None, over={'lse': lsed.data_ptr() + 2}) == ERR_ARG
    assert bwd_call(L, ops, xd, V, labd, lsed, wd, cnt, gsd, out, None, over={'labels': labd.data_ptr() + 4}) == ERR_ARG
    rd = i32(rows)
    for name, t in (("w", wd), ("count", cnt), ("gsd", gsd), ("rd", rd)):
        assert bwd_call(L, ops, xd, V, labd, lsed, wd, cnt, gsd, out, rd, over={name: t.data_ptr() + 2}) == ERR_ARG, name
    # an element-wise ld asks for element alignment only
    assert bwd_call(L, ops, xd, V, labd, lsed, wd, cnt, gsd, out, None, ld=ld - 1, rows=rows - 1, over={'out': out.data_ptr() + 1}) == ERR_ARG
    torch.cuda.synchronize()
    assert bool((out == FILL).all())
    f16 = torch.zeros(rows, ld, dtype=torch.float16, device="cuda")
    assert L.lib().mvlt_ce_bwd_weighted(99, ptr(f16), ld, rows, V, ptr(labd), ptr(lsed), ptr(wd), ptr(cnt), 1.0, None, ptr(f16), None,
                                        ops._stream()) not in (0, ERR_ARG)


# ------------------------------------------------------------------ weighted sum
def fwd_call(L, ops, lse, xl, w, rows, rows_dev, acc, over=None):
    a = dict(lse=ptr(lse), xl=ptr(xl), w=ptr(w), acc=ptr(acc), rd=ptr(rows_dev))
    a.update(over or {})
    return L.lib().mvlt_seq_loss_fwd(a["lse"], a["xl"], a["w"], rows, a["rd"], a["acc"], ops._stream())


@pytest.mark.parametrize("n,rd", [(1, None), (37, 23), (1024, None), (1025, 1025), (4801, 4800), (40, 0)])
def test_seq_loss_fwd_sum_bound_and_bits(L, ops, n, rd):
    g = R.gen(n)
    lse = (8.0 + torch.randn(n, generator=g)).float()
    xl = (lse - 6.0 * torch.rand(n, generator=g)).float()
    w = torch.randn(n, generator=g).float()
    w[::5] = 0.0
    lse[0] = math.inf                                      # a row of weight 0 is never read
    if n > 5:
        xl[5] = NAN
    n_valid = n if rd is None else rd
    if n_valid < n:
        lse[n_valid:], xl[n_valid:], w[n_valid:] = NAN, NAN, NAN
    ref, bound, _ = R.seq_sum_ref(lse, xl, w, n_valid)
    dev = [t.cuda() for t in (lse, xl, w)]
    rows_dev = None if rd is None else i32(rd)
    runs = []
    for _ in range(2):
        acc = filled((2 + GUARD,), FILL)
        assert fwd_call(L, ops, *dev, n, rows_dev, acc) == 0
        runs.append(acc.cpu())
    a = runs[0]
    print(f"n={n} rows_dev={rd}: sum {float(a[0])!r} ref {ref!r} bound {bound:.3g}")
    assert abs(float(a[0]) - ref) <= bound, (float(a[0]), ref, bound)
    assert float(a[1]) == float(n_valid) and bool((a[2:] == FILL).all())
    check_equal(runs[0], runs[1], "two runs")
    if n_valid == 0:
        assert float(a[0]) == 0.0 and float(a[1]) == 0.0


def test_seq_loss_fwd_refusals_leave_the_output_alone(L, ops):
    n = 16
    lse, xl, w = (torch.ones(n, device="cuda") for _ in range(3))
    acc = filled((2 + GUARD,), FILL)
    for name in ("lse", "xl", "w", "acc"):
        assert fwd_call(L, ops, lse, xl, w, n, None, acc, over={name: None}) == ERR_ARG, name
    assert fwd_call(L, ops, lse, xl, w, 0, None, acc) == ERR_ARG
    assert fwd_call(L, ops, lse, xl, w, 4096 * 512 + 1, None, acc) == ERR_ARG
    assert fwd_call(L, ops, lse, xl, w, n, None, acc, over={'lse': lse.data_ptr() + 2}) == ERR_ARG
    assert fwd_call(L, ops, lse, xl, w, n, None, acc, over={'acc': acc.data_ptr() + 1}) == ERR_ARG
    rd = i32(n)
    for name, t in (("xl", xl), ("w", w), ("rd", rd)):
        assert fwd_call(L, ops, lse, xl, w, n, rd, acc, over={name: t.data_ptr() + 2}) == ERR_ARG, name
    torch.cuda.synchronize()
    assert bool((acc == FILL).all())
