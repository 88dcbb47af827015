"""tests/swin_attn_half_ref.py discriminates: a plain torch emulation of the attention half of a Swin block (f32 arithmetic,
rounded to the compute dtype where the kernels store) sits inside every bound at shifts 0 and 3, in bf16 and f32, on every
backward mode, and each of a named list of wiring faults is rejected with the tensor and the place named.

What the bounds can and cannot see.  The forward tensors, proj.weight / proj.bias, the residual part of dx0 and the rows of
dropped samples are judged one stage deep and are sharp in both dtypes.  dbias_table, qkv.weight / qkv.bias, norm1.weight /
norm1.bias and the branch part of dx0 stand two to four stages behind the last known operand, and every stage carries its
input's bound through |W| as a worst case (a sum of n roundings counts n times, not sqrt(n) times).  In f32 that chain
stays orders of magnitude below the values and every fault below is rejected.  In bf16 the roundings of dyw, dO, dS and dqkv
(2^-8 each) through sums of 192, 32, 49 and 576 terms give a dxn1w bound larger than dxn1w itself, so three faults that
show only there -- the last dxn part not summed, one dbias workspace row not reduced, norm1.weight from the un-gathered
dy -- are rejected at f32 precision only; BF16_BLIND lists them, the test prints their bf16 ratios (0.004 .. 1.5 of the
bound), and a bf16 GPU run on backward modes 1 / 2 cannot reject them per element either: there the GPU test holds the two
host paths to bit-equality on every route, which sees such a fault in one path but not one that both share.

For every fault the two criteria the suite had for this composition are evaluated as well, on the seven attention-side
gradients of the block: the whole-gradient criterion of test_swin_backward_routes_in_the_model
(sqrt(sum |g - ref|^2 / sum |ref|^2) < 3e-2) and the per-parameter one of test_swin_backward_is_the_same_on_both_host_paths
(|g - ref| / |ref| < 2e-4; that test compares the two host paths in f32, so a fault both paths share passes it whatever
this number is).  test_old_criteria_report prints the table; several faults pass the first criterion, and the faults that
touch only dx0 are invisible to both at the level of this block."""
import math

import pytest
import torch

import attn_ref as A
import ln_ref as R
import swin_attn_half_ref as H
from swin_attn_half_ref import BF, F32

GEOM = dict(res=14, C=192, nH=6, B=3)              # 12 windows, two qkv-dgrad parts, a dropped sample first and a kept one last
DROP_P = 0.25
CLEAN = [(BF, 0, 2), (BF, 3, 2), (BF, 3, 1), (BF, 0, 0), (BF, 3, 0), (F32, 0, 0), (F32, 3, 0)]      # (dtype, shift, backward mode)
FORWARD = ("xn1w", "mean1", "rstd1", "qkv", "ao", "lse", "x1")
# fault -> (tensors that must leave their bound, True: and no other tensor does | False: and no forward tensor does | None)
FAULTS = {
    "w2n and n2w exchanged": (("xn1w", "x1", "dx0"), None),
    "s1 missing in the backward": (("proj.bias", "proj.weight", "dx0"), False),
    "s1 applied to dres": (("dx0",), True),
    "dbproj from the unscaled dx2": (("proj.bias",), True),
    "dres omitted from dx0": (("dx0",), True),
    "last dxn part not summed": (("dx0", "norm1.weight", "norm1.bias"), True),
    "one workgroup's dbias workspace row not reduced": (("dbias_table",), True),
    "one head's column of dbias_table dropped": (("dbias_table",), True),
    "shift mask ignored in the backward": (("dx0", "qkv.weight", "dbias_table"), False),
    "qkv.weight from xn in token order": (("qkv.weight",), True),
    "norm1.weight from the un-gathered dy": (("norm1.weight",), True),
    "mean and rstd exchanged": (("mean1", "rstd1"), None),
}
LOST_WINDOW = 6                                     # a window of sample 1 (kept)
# bf16 only: tensors whose chained bound exceeds what the fault moves (module docstring); rejected in f32
BF16_BLIND = {"w2n and n2w exchanged": ("dx0",), "last dxn part not summed": ("dx0", "norm1.weight", "norm1.bias"),
              "one workgroup's dbias workspace row not reduced": ("dbias_table",),
              "norm1.weight from the un-gathered dy": ("norm1.weight",)}


def case_of(dt, shift, bwd):
    return dict(GEOM, dtype=dt, shift=shift, bwd=bwd)


def make_inputs(case, seed=5, s1_none=False):
    """The operands of one block call: activations, the DropPath scales (first sample dropped) and the parameters, drawn as
    tests/test_swin_attn_half_gpu.py draws them: one-dimensional parameters away from 0 / 1, the bias table with std 0.5,
    qkv weights scaled so that scale q.k has std ~2.5 (attn_ref.LOGIT_STD)."""
    res, C, nH, B, dt = (case[k] for k in ("res", "C", "nH", "B", "dtype"))
    g = torch.Generator().manual_seed(seed)
    rows = B * res * res
    wqkv = torch.randn(3 * C, C, generator=g) * C ** -0.5
    wqkv[:2 * C] *= math.sqrt(A.LOGIT_STD)
    keep = torch.tensor([0.0] + [1.0] * (B - 1))
    return dict(x=torch.randn(rows, C, generator=g).to(dt), dx2=torch.randn(rows, C, generator=g).to(dt),
                s1=None if s1_none else keep / (1.0 - DROP_P),
                gamma1=1.0 + 0.1 * torch.randn(C, generator=g), beta1=0.1 * torch.randn(C, generator=g),
                wqkv=wqkv.to(dt), bqkv=0.1 * torch.randn(3 * C, generator=g),
                wproj=(torch.randn(C, C, generator=g) * C ** -0.5).to(dt), bproj=0.1 * torch.randn(C, generator=g),
                table=0.5 * torch.randn(169, nH, generator=g))


def emulate(inp, case, fault=None):
    """The half in f32, stored tensors rounded to the compute dtype; `fault` names one entry of FAULTS."""
    res, C, nH, B, dt, shift, bwd = (case[k] for k in ("res", "C", "nH", "B", "dtype", "shift", "bwd"))
    Lt, nW, hd = res * res, (res // 7) ** 2, C // nH
    rows, nseq, scale = B * Lt, B * nW, (C // nH) ** -0.5
    w2n, n2w = H.window_maps(B, res, shift)
    if fault == "w2n and n2w exchanged":
        w2n, n2w = n2w, w2n
    x, dx2 = inp["x"].float(), inp["dx2"].float()
    gam, bet = inp["gamma1"], inp["beta1"]
    wq, wp = inp["wqkv"].float(), inp["wproj"].float()
    s1 = torch.ones(B) if inp["s1"] is None else inp["s1"]
    s_tok = s1[torch.arange(rows) // Lt][:, None]                # the maps permute rows inside a sample: the same scale in either order
    heads = lambda t: t.float().view(nseq, 49, nH, hd).permute(0, 2, 1, 3)              # noqa: E731
    unheads = lambda t: t.permute(0, 2, 1, 3).reshape(rows, C)                          # noqa: E731
    # ---- forward
    mean = x.mean(1)
    d = x - mean[:, None]
    rstd = torch.rsqrt((d * d).mean(1) + R.EPS)
    xn = (d * rstd[:, None] * gam + bet).to(dt)
    xn1w = xn[w2n]
    qkv = (xn1w.float() @ wq.t() + inp["bqkv"]).to(dt)
    Q, K, V = heads(qkv[:, :C]), heads(qkv[:, C:2 * C]), heads(qkv[:, 2 * C:])
    s = scale * (Q @ K.transpose(-1, -2)) + A.swin_bias(inp["table"], nW, res, shift, nseq).float()
    m = s.amax(-1, keepdim=True)
    e = torch.exp(s - m)
    ssum = e.sum(-1, keepdim=True)
    lse = (m + torch.log(ssum))[..., 0]
    ao = unheads((e / ssum).to(dt).float() @ V).to(dt)
    x1 = torch.empty(rows, C, dtype=dt)
    x1[w2n] = ((ao.float() @ wp.t() + inp["bproj"]) * s_tok + x[w2n]).to(dt)
    # ---- backward
    dyw = (dx2[w2n] * (1.0 if fault == "s1 missing in the backward" else s_tok)).to(dt)
    dO = heads((dyw.float() @ wp).to(dt))
    sb = s
    if fault == "shift mask ignored in the backward":
        sb = scale * (Q @ K.transpose(-1, -2)) + A.swin_bias(inp["table"], nW, res, 0, nseq).float()
    P = torch.exp(sb - lse[..., None])
    delta = (dO * heads(ao)).sum(-1, keepdim=True)
    dS = (P * (dO @ V.transpose(-1, -2) - delta)).to(dt).float()
    dqkv32 = torch.cat([unheads(scale * (dS @ K)), unheads(scale * (dS.transpose(-1, -2) @ Q)),
                        unheads(P.to(dt).float().transpose(-1, -2) @ dO)], 1)
    dqkv = dqkv32.to(dt)
    # the bias-table gradient: one partial row per window (the workspace of a workgroup), then the reduce
    from oracle import mvlt_oracle as O
    ws = dS.permute(0, 2, 3, 1).reshape(nseq, 49 * 49, nH).clone()
    if fault == "one workgroup's dbias workspace row not reduced":
        ws[LOST_WINDOW] = 0.0
    dtab = torch.zeros(169, nH).index_add_(0, O.relative_position_index(7).view(-1), ws.sum(0))
    if fault == "one head's column of dbias_table dropped":
        dtab[:, nH - 1] = 0.0
    if bwd == 2:          # nH / 3 partial products, each stored in bf16, added in f32 by norm1's backward and rounded once
        parts = []
        for gi in range(nH // 3):
            cols = torch.cat([torch.arange(p * C + 3 * gi * hd, p * C + 3 * (gi + 1) * hd) for p in range(3)])
            parts.append((dqkv32[:, cols] @ wq[cols]).to(dt))
        if fault == "last dxn part not summed":
            parts = parts[:-1]
        dxn = R.sum_parts(parts).float() if dt == BF else sum(parts)
    else:
        dxn = (dqkv.float() @ wq).to(dt).float()
    if fault == "mean and rstd exchanged":
        mean, rstd = rstd, mean
    dy = dxn[n2w]
    xh = (x - mean[:, None]) * rstd[:, None]
    g = dy * gam
    core = g - g.mean(1, keepdim=True) - xh * (g * xh).mean(1, keepdim=True)
    dres = {"s1 applied to dres": dx2 * s_tok, "dres omitted from dx0": 0.0}.get(fault, dx2)
    dx0 = (rstd[:, None] * core + dres).to(dt)
    out = dict(inp)
    out.update(xn1w=xn1w, mean1=mean, rstd1=rstd, qkv=qkv, ao=ao, lse=lse, x1=x1, x2=x1.clone(), dx0=dx0, dbias_table=dtab)
    out["norm1.weight"] = ((dxn if fault == "norm1.weight from the un-gathered dy" else dy) * xh).sum(0)
    out["norm1.bias"] = dy.sum(0)
    out["proj.weight"] = dyw.float().t() @ ao.float()
    out["proj.bias"] = dx2.sum(0) if fault == "dbproj from the unscaled dx2" else dyw.float().sum(0)
    out["qkv.weight"] = dqkv.float().t() @ (xn if fault == "qkv.weight from xn in token order" else xn1w).float()
    out["qkv.bias"] = dqkv.float().sum(0)
    for k, shape in zip(H.MLP_GRADS, ((4 * C, C), (4 * C,), (C, 4 * C), (C,), (C,), (C,))):
        out[k] = torch.zeros(shape)
    if inp["s1"] is None:
        del out["s1"]
    return out


def test_window_maps_are_the_library_maps():
    from mvlt_amd.indexing import batched_window_maps
    for B, res, shift in ((3, 14, 0), (3, 14, 3), (2, 7, 0), (2, 28, 3)):
        w2n, n2w = H.window_maps(B, res, shift)
        lw, ln = batched_window_maps(B, res, res, 7, shift, "cpu")
        assert torch.equal(w2n.int(), lw) and torch.equal(n2w.int(), ln), (B, res, shift)
    w2n, n2w = H.window_maps(3, 14, 3)
    assert not torch.equal(w2n, n2w), "the exchanged-maps fault needs maps that differ"


@pytest.mark.parametrize("dt,shift,bwd", CLEAN, ids=lambda v: str(v).replace("torch.", ""))
@pytest.mark.parametrize("s1_none", [False, True], ids=["s1-mixed", "s1-none"])
def test_emulation_sits_inside_every_bound(dt, shift, bwd, s1_none):
    case = case_of(dt, shift, bwd)
    run = emulate(make_inputs(case, s1_none=s1_none), case)
    ref = H.reference(run, case)
    for k, v in H.worst_ratios(ref).items():
        print(f"emulation {str(dt)[6:]:8s} shift {shift} bwd {bwd} {'s1=None' if s1_none else 's1 mixed'} {k:13s} worst ratio to the bound {v:.3f}")
    bad = H.failures(ref)
    assert not bad, bad
    H.check_dropped_rows(run, case)
    assert set(ref) == set(H.SAVED) | set(H.COMPARED)


def test_premises_are_asserted():
    case = case_of(BF, 3, 2)
    run = emulate(make_inputs(case), case)
    broken = dict(run, x2=run["x1"].clone())
    broken["x2"][17, 5] += 1.0
    with pytest.raises(AssertionError, match="x2 == x1.*row 17, column 5"):
        H.reference(broken, case)
    broken = dict(run)
    broken["fc1.bias"] = run["fc1.bias"].clone()
    broken["fc1.bias"][3] = 1e-30
    with pytest.raises(AssertionError, match="fc1.bias is exactly zero.*row 3"):
        H.reference(broken, case)


def old_criteria(run, ref, clean):
    """(whole-gradient relative error against the float64 values, worst per-parameter relative error against the clean run of
    the same arithmetic -- that criterion compares two runs --, relative error of dx0) over the attention-side gradients."""
    num = {k: float((run[k].double() - ref[k][0]).pow(2).sum()) for k in H.ATTN_GRADS}
    den = {k: float(ref[k][0].pow(2).sum()) for k in H.ATTN_GRADS}
    whole = math.sqrt(sum(num.values()) / sum(den.values()))
    per = max(float((run[k].double() - clean[k].double()).norm() / clean[k].double().norm()) for k in H.ATTN_GRADS)
    dx0 = float((run["dx0"].double() - ref["dx0"][0]).norm() / ref["dx0"][0].norm())
    return whole, per, dx0


@pytest.fixture(scope="module")
def fault_runs():
    """{(fault, shift, dtype): (run, ref)} on backward mode 2 (its part sums emulated in either dtype), plus the clean runs
    under fault None."""
    out = {}
    for dt in (BF, F32):
        for shift in (0, 3):
            case = case_of(dt, shift, 2)
            inp = make_inputs(case)
            for fault in [None] + list(FAULTS):
                if fault == "shift mask ignored in the backward" and shift == 0:
                    continue                              # no mask at shift 0: not a fault there
                run = emulate(inp, case, fault)
                out[fault, shift, dt] = (run, H.reference(run, case))
    return out


@pytest.mark.parametrize("dt", [BF, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("shift", [0, 3])
@pytest.mark.parametrize("fault", list(FAULTS))
def test_fault_is_rejected_by_name(fault_runs, fault, shift, dt):
    if (fault, shift, dt) not in fault_runs:
        assert fault == "shift mask ignored in the backward" and shift == 0
        return
    must, scope = FAULTS[fault]
    blind = BF16_BLIND.get(fault, ()) if dt == BF else ()
    run, ref = fault_runs[fault, shift, dt]
    bad = H.failures(ref, fault)
    ratios = H.worst_ratios(ref)
    for k in must:
        print(f"{fault}, shift {shift}, {str(dt)[6:]}: {k} at {ratios[k]:.3g} of its bound")
        if k in blind:
            continue
        assert k in bad, (fault, shift, k, "was accepted", sorted(bad))
        assert f"{fault} {k}: " in bad[k] and "worst at row" in bad[k], bad[k]
        print(bad[k])
    if scope is True:
        assert set(bad) <= set(must) and set(bad) >= set(must) - set(blind), (fault, shift, sorted(bad))
    elif scope is False:
        assert not set(bad) & set(FORWARD), (fault, shift, sorted(bad))
    case = case_of(dt, shift, 2)
    Lt = case["res"] ** 2
    if fault == "one head's column of dbias_table dropped":
        assert f"column {case['nH'] - 1}:" in bad["dbias_table"], bad["dbias_table"]
    if fault == "last dxn part not summed":
        assert "qkv.weight" not in bad and "qkv.bias" not in bad           # dqkv itself is whole
    if fault in ("s1 applied to dres", "dres omitted from dx0", "s1 missing in the backward"):
        # the dropped sample: no residual gradient, or a branch gradient it must not receive
        with pytest.raises(AssertionError, match=r"dx0 rows of dropped sample 0 \(rows from 0\)"):
            H.check_dropped_rows(run, case)
    elif fault not in ("w2n and n2w exchanged", "mean and rstd exchanged"):
        H.check_dropped_rows(run, case)


def test_old_criteria_report(fault_runs):
    """Which faults the whole-gradient criterion (3e-2) and the per-parameter criterion (2e-4) accept."""
    accepted_whole, accepted_both = [], []
    for (fault, shift, dt), (run, ref) in fault_runs.items():
        if dt != BF:
            continue
        whole, per, dx0 = old_criteria(run, ref, fault_runs[None, shift, dt][0])
        a, b = whole < 3e-2, per < 2e-4
        print(f"shift {shift} {str(fault):50s} whole gradient {whole:9.2e} {'ACCEPTED' if a else 'rejected'}   "
              f"worst parameter {per:9.2e} {'ACCEPTED' if b else 'rejected'}   dx0 {dx0:9.2e}")
        if fault is None:
            assert a, "the clean bf16 emulation meets the whole-gradient criterion"
            continue
        if a:
            accepted_whole.append((fault, shift))
        if a and b:
            accepted_both.append((fault, shift))
    print("accepted by the whole-gradient criterion:", sorted({f for f, _ in accepted_whole}))
    print("accepted by both:", sorted({f for f, _ in accepted_both}))
    # by construction: a fault that touches dx0 alone leaves every gradient of this block as it was
    for fault in ("s1 applied to dres", "dres omitted from dx0"):
        for shift in (0, 3):
            assert (fault, shift) in accepted_whole, (fault, shift)
    assert len({f for f, _ in accepted_whole}) >= 4, "several faults pass the whole-gradient criterion"
