"""mvlt_mlm_head_ce through ops.mlm_head_ce (and, where outputs must be pre-filled, through the C entry point with the structs
ops builds): lse, the logit at the label, the loss sum and count and the stored logits against the float64 reference and bounds
of tests/head_ce_ref.py, in bf16 and f32; ragged row counts, bit-reproducibility, the no-logits form, refusals."""
import ctypes as C
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import head_ce_ref as R  # noqa: E402
from gemm_ref import check_bound  # noqa: E402

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
ERR_ARG = -1
SENT = -12345.0


@pytest.fixture(scope="module")
def M():
    import mvlt_amd
    return mvlt_amd


_cache = {}


def _case(Mr, K, V, rd, dtype):
    """Operands (host), labels and the reference, computed once per (shape, dtype, row count) and left unchanged."""
    key = (Mr, K, V, rd, dtype)
    if key not in _cache:
        A, W, buf = R.operands(Mr, K, V, dtype, R.seed_of(Mr, K, V, dtype))
        lab = R.edge_labels(Mr, V, rd is not None, 11 + Mr)
        _cache[key] = (A, W, buf, lab, R.head_ce_ref(A, W, buf[:V], lab, rd))
    return _cache[key]


def _run_raw(M, A, W, bias, lab, rd, want_logits, change=None, p_change=None):
    """The C entry point on pre-filled outputs -> (rc, lse, x_label, acc, logits or None)."""
    from mvlt_amd import _lib as L
    ops = M.ops
    rows, V = A.shape[0], W.shape[0]
    p, _, _ = ops._head_gemm(A, W, bias)
    ld = (V + 63) // 64 * 64
    logits = torch.full((rows, ld), SENT, dtype=A.dtype, device="cuda") if want_logits else None
    if want_logits:
        p.C, p.ldc = logits.data_ptr(), ld
    if rd is not None:
        rdt = torch.tensor([rd], dtype=torch.int32, device="cuda")
        p.m_dev = rdt.data_ptr()
    lse = torch.full((rows,), SENT, device="cuda")
    xl = torch.full((rows,), SENT, device="cuda")
    acc = torch.full((2,), SENT, device="cuda")
    ws = torch.empty(L.lib().mvlt_mlm_head_ce_workspace_bytes(rows, V), dtype=torch.uint8, device="cuda")
    h = L.MvltHeadCE()
    h.labels, h.lse, h.x_label, h.acc = lab.data_ptr(), lse.data_ptr(), xl.data_ptr(), acc.data_ptr()
    h.workspace, h.workspace_bytes = ws.data_ptr(), ws.numel()
    for k, v in (change or {}).items():
        setattr(h, k, v)
    for k, v in (p_change or {}).items():
        setattr(p, k, v)
    rc = L.lib().mvlt_mlm_head_ce(C.byref(p), C.byref(h), None)
    torch.cuda.synchronize()
    return rc, lse, xl, acc, logits


def _check(ref, lse, xl, acc, logits, rows_total, what):
    n = ref["lse"].numel()
    ratio = ((lse[:n].double().cpu() - ref["lse"]).abs() / ref["bound_lse"])
    print(f"{what}: lse worst ratio {float(ratio.max()) if n else 0.0:.3g}; acc {acc.tolist()} ref ({ref['nll_sum']:.6f}, {ref['count']})"
          f" bound {ref['bound_sum']:.3g}")
    assert n == 0 or float(ratio.max()) <= 1.0, what
    on = ref["on"]
    d = (xl[:n].double().cpu() - ref["x_label"]).abs()
    assert bool((d[on] <= ref["bound_xl"][on]).all()), what
    assert float(acc[1]) == ref["count"], what
    assert abs(float(acc[0]) - ref["nll_sum"]) <= ref["bound_sum"], what
    if logits is not None:
        V = ref["v"].shape[1]
        check_bound(logits[:n, :V].cpu(), ref["v"], ref["bound_v"], what + " logits")


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("Mr,K,V,rd", R.SMALL)
def test_head_ce_against_host_reference(M, Mr, K, V, rd, dtype):
    A, W, buf, lab, ref = _case(Mr, K, V, rd, dtype)
    Ad, Wd, bd, ld_ = A.cuda(), W.cuda(), buf.cuda()[:V], lab.cuda()
    what = f"{Mr}x{K}x{V} rows_dev {rd}"
    rc, lse, xl, acc, logits = _run_raw(M, Ad, Wd, bd, ld_, rd, True)
    assert rc == 0
    _check(ref, lse, xl, acc, logits, Mr, what)
    n = ref["lse"].numel()
    # rows at or beyond *rows_dev are not written; neither is x_label of an ignored row, nor a logits column at or beyond V
    assert bool((lse[n:] == SENT).all()) and bool((xl[n:] == SENT).all()) and bool((logits[n:] == SENT).all()), what
    assert bool((xl[:n][~ref["on"].cuda()] == SENT).all()), what
    assert bool((logits[:, V:] == SENT).all()), what
    if rd == 0:
        assert acc.tolist() == [0.0, 0.0]
    # the public call: the same bits, twice, and without the logits
    rdt = None if rd is None else torch.tensor([rd], dtype=torch.int32, device="cuda")
    o1 = M.ops.mlm_head_ce(Ad, Wd, bd, ld_, V, rows_dev=rdt, want_logits=True)
    o2 = M.ops.mlm_head_ce(Ad, Wd, bd, ld_, V, rows_dev=rdt, want_logits=True)
    o3 = M.ops.mlm_head_ce(Ad, Wd, bd, ld_, V, rows_dev=rdt, want_logits=False)
    assert o3[3] is None and o1[3].shape == (Mr, (V + 63) // 64 * 64) and o1[3].dtype == dtype
    on = torch.zeros(Mr, dtype=torch.bool, device="cuda")
    on[:n] = ref["on"].cuda()
    for o in (o1, o2, o3):
        assert torch.equal(o[0], acc), what
        assert torch.equal(o[1][:n], lse[:n]) and torch.equal(o[2][on], xl[on]), what
    assert torch.equal(o1[3][:n, :V], logits[:n, :V]) and torch.equal(o2[3][:n, :V], logits[:n, :V]), what


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
def test_head_ce_full_vocabulary_and_memory(M, dtype):
    Mr, K, V, rd = R.BIG
    A, W, buf, lab, ref = _case(Mr, K, V, rd, dtype)
    Ad, Wd, bd, ld_ = A.cuda(), W.cuda(), buf.cuda()[:V], lab.cuda()
    M.ops.mlm_head_ce(Ad[:1], Wd, bd, ld_[:1], V, want_logits=False)          # (the workspace exists before the measurement)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    acc, lse, xl, none = M.ops.mlm_head_ce(Ad, Wd, bd, ld_, V, want_logits=False)
    torch.cuda.synchronize()
    delta = torch.cuda.max_memory_allocated() - base
    print(f"peak allocated delta without logits: {delta} bytes (a bf16 logits buffer: {Mr * V * 2})")
    assert none is None and delta < Mr * V * 2
    _check(ref, lse, xl, acc, None, Mr, f"{Mr}x{K}x{V} no logits")
    acc2, lse2, xl2, logits = M.ops.mlm_head_ce(Ad, Wd, bd, ld_, V, want_logits=True)
    on = ref["on"].cuda()
    assert torch.equal(acc2, acc) and torch.equal(lse2, lse) and torch.equal(xl2[on], xl[on])
    check_bound(logits[:, :V].cpu(), ref["v"], ref["bound_v"], "full vocabulary logits")


def test_head_ce_feeds_ce_bwd_like_the_three_launch_route(M):
    """acc / lse / logits go into ops.ce_bwd unchanged: dlogits agree with those of gemm + ce_fwd + ce_bwd on the same operands.
    Both sets of logits are held to the reference's per-element bound (whichever kernel mvlt_gemm routes the plain product to),
    the loss sums to the reference's bound, and dlogits = (exp(x - lse) - onehot) / count to what those bounds let it move."""
    Mr, K, V, rd = 65, 64, 777, None
    A, W, buf, lab, ref = _case(Mr, K, V, rd, F32)
    Ad, Wd, bd, ld_ = A.cuda(), W.cuda(), buf.cuda()[:V].contiguous(), lab.cuda()
    acc, lse, _, logits = M.ops.mlm_head_ce(Ad, Wd, bd, ld_, V)
    old = M.ops.gemm(Ad, Wd, bias=bd, ldc=logits.shape[1])
    check_bound(old[:, :V].cpu(), ref["v"], ref["bound_v"], "plain product")
    check_bound(logits[:, :V].cpu(), ref["v"], ref["bound_v"], "fused product")
    acc0, lse0 = M.ops.ce_fwd(old, V, ld_)
    assert float(acc0[1]) == float(acc[1]) == ref["count"]
    assert abs(float(acc0[0]) - ref["nll_sum"]) <= ref["bound_sum"] and abs(float(acc[0]) - ref["nll_sum"]) <= ref["bound_sum"]
    d0 = M.ops.ce_bwd(old.clone(), V, ld_, lse0, acc0)[:, :V].double().cpu()
    d1 = M.ops.ce_bwd(logits.clone(), V, ld_, lse, acc)[:, :V].double().cpu()
    # |d exp(x - lse)| <= exp(x - lse) (|dx| + |dlse|), each side within its bound of the reference: twice the sum, plus f32 rounding
    p = torch.exp(ref["x"] - ref["lse"][:, None])
    tol = (2.0 * p * (ref["bound_v"] + ref["bound_lse"][:, None]) + 1e-6) / max(ref["count"], 1)
    on = ref["on"]
    assert bool(((d1 - d0).abs()[on] <= tol[on]).all())
    assert bool((d1[~on] == 0).all()) and bool((d0[~on] == 0).all())


def test_label_outside_the_vocabulary_poisons_the_loss(M):
    Mr, K, V, rd = 65, 64, 777, None
    A, W, buf, lab, _ = _case(Mr, K, V, rd, BF16)
    bad = lab.clone()
    bad[3] = V
    acc, lse, _, _ = M.ops.mlm_head_ce(A.cuda(), W.cuda(), buf.cuda()[:V], bad.cuda(), V, want_logits=False)
    assert math.isnan(float(acc[0])) and bool(torch.isfinite(lse).all())


def test_head_ce_refusals_launch_nothing(M):
    Mr, K, V, rd = 65, 64, 777, None
    A, W, buf, lab, _ = _case(Mr, K, V, rd, BF16)
    Ad, Wd, bfull, ld_ = A.cuda(), W.cuda(), buf.cuda(), lab.cuda()
    bd = bfull[:V]
    wide = torch.zeros((Mr, K + 8), dtype=BF16, device="cuda")
    cases = [
        ("labels NULL", dict(labels=None), {}),
        ("lse NULL", dict(lse=None), {}),
        ("acc NULL", dict(acc=None), {}),
        ("workspace NULL", dict(workspace=None), {}),
        ("workspace too small", dict(workspace_bytes=64), {}),
        ("ldc < V", {}, dict(ldc=V - 1)),
        ("ldc not a multiple of 4", {}, dict(ldc=V + 2)),
        ("bias NULL", {}, dict(bias=None)),
        ("A off by one element", {}, dict(A=wide.data_ptr() + 2, lda=K + 8)),
        ("lda not a multiple of 16 bytes", {}, dict(A=wide.data_ptr(), lda=K + 3)),
        ("C off by one element", {}, dict(C=-1)),
        ("k-major W", {}, dict(b_kmajor=1)),
        ("another epilogue bit", {}, dict(epilogue=3)),
    ]
    for what, change, p_change in cases:
        if p_change.get("C") == -1:
            spare = torch.full((Mr + 1, 832), SENT, dtype=BF16, device="cuda")
            p_change = dict(C=spare.data_ptr() + 2)
        rc, lse, xl, acc, logits = _run_raw(M, Ad, Wd, bd, ld_, None, True, change, p_change)
        assert rc == ERR_ARG, (what, rc)
        for t in (lse, xl, acc, logits):
            assert bool((t == SENT).all()), what
        if "C" in p_change:
            assert bool((spare == SENT).all()), what
