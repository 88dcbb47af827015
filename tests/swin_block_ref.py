"""float64 reference of a whole Swin block,

    x1 = x  + s1 proj(W-MSA(qkv(norm1 x)))          s1, s2: DropPath scales per sample (0 or 1 / (1 - p)) or None
    x2 = x1 + s2 fc2(GELU(fc1(norm2 x1)))

and of its backward, with a per-element bound for every tensor the block functions save or hand back (swin.py _block_fwd /
_block_bwd and csrc/host.cpp swin_block_fwd / swin_block_bwd), both halves live at once: x1 != x, dx1 != dx2, dyw is no
scaled copy of dx2 -- the wiring between the halves that tests/test_swin_attn_half_gpu.py (s2 = 0) and
tests/test_swin_droppath_compact_gpu.py (s1 = 0) leave degenerate.

Built only from tests/swin_attn_half_ref.py, tests/gemm_ref.py, tests/ln_ref.py, tests/attn_ref.py and tests/misc_ref.py with
their constants unchanged: this module introduces no tolerance of its own.  The window maps are those of
swin_attn_half_ref.window_maps (stated from the definition).  The stage formulas of the Mlp half, which
tests/test_swin_droppath_compact_gpu.py wrote out for s1 = 0, are stated here once (mlp_forward / the Mlp part of reference).

Rows.  Logical (dense) order: row = sample * Lt + token.  A block that ran its Mlp half on the kept samples only hands over
perm / inv / count (mvlt_droppath_plan): its stored xn2 / h / act are in the plan's compact order (compact row i is logical
row perm[i]; rows at or beyond count of h / act are never written and never read here).  Everything else, and every backward
stage a run hands over, is in logical order: the rows of dropped samples are exact zeros there, and dense_saved() moves the
stored xn2 / h / act of a compact run to that order (h / act scattered through perm, zeros elsewhere), an exact move.

Forward, each stage from the saved operand the kernel itself read, so the bounds do not compound:
  xn1w, mean1, rstd1   ln_ref.fwd_ref(x[w2n])                      qkv    gemm_ref(saved xn1w, Wqkv, bias)
  ao, lse              attn_ref.AttnRef(saved qkv, swin_bias)      x1     gemm_ref(saved ao, Wproj, bias, s1, w2n, residual x)
  xn2, mean2, rstd2    ln_ref.fwd_ref(saved x1)   (xn2 read back through inv)
  h, act               gemm_ref(saved xn2, W1, bias, gelu) over the first `count` rows
  x2                   gemm_ref(saved act, W2, bias, s2, perm, residual saved x1); rows of samples the plan drops: x1 itself
Backward, judged twice (the rule of tests/bert_layer_ref.py).
  CHAINED from dx2: float64 values of dy2, dh, dxn2, dx1, dyw, dqkv, dxn1w, the bound of each stage = the stage's own bound
  (as if its input were exact) + the bound e of its input carried through the stage's own linear map, first order:
    dy2   = dx2 s2          one f32 product and one store rounding, (U32 + U_OUT) |dy2|; exact (the same tensor) without s2.
                            Handed over by the producer block instead (`dy2_pre`): formed there from the f32 dx0 whose rounded
                            copy is dx2, so U_OUT s2 |dx2| + (2 U32 + U_OUT) |dy2| (ln_ref's rule for a branch output)
    dh    = (dy2 W2) gelu'(h)         + (e_dy2 |W2|) (|gelu'(h)| + ERFC_ABS)
    dxn2  = dh W1                     + e_dh |W1|
    dx1, dyw   ln_ref.bwd_ref(saved x1, dxn2, dres = dx2, zscale = s1): dx1 = J dxn2 + dx2, dyw[n2w[r]] = s1 dx1[r] formed from
               the f32 dx1;  + ln_carry(e_dxn2), times s1 for dyw
    dO    = dyw Wproj                 + e_dyw |Wproj|          (all three backward modes: swin_attn_half_ref)
    dqkv, dbias_table   AttnRef(saved qkv, dO, dout_err = e_dO)
    dxn1w = dqkv Wqkv                 + e_dqkv |Wqkv|  (+ U_OUT |dqkv| |Wqkv| for the bf16 parts of backward mode 2)
    dx0   ln_ref.bwd_ref(x, dxn1w[n2w], dres = dx1)           + ln_carry(e_dxn1w[n2w]) + e_dx1
    weight gradients gemm_ref(dY^T, X, out f32) + e_dY^T |X|, bias gradients colsum_ref + sum_r e_dY, over the live rows:
    fc2 (dy2, act)  fc1 (dh, xn2)  proj (dyw, ao)  qkv (dqkv, xn1w);  norm2 / norm1 parameters: bwd_ref's own + sum_r e |xh| / e
  CUT.  Behind two products, a LayerNorm backward, the attention backward and another product the chained bound of dx0's
  branch part stands near the signal in bf16, so a wiring fault between the halves can hide in it.  A run may therefore hand
  over the STORED intermediates STAGES of a replay of its backward -- the launch list of swin.py _block_bwd issued one by one
  by the test on the run's own saved tensors.  reference() then judges each handed-over tensor against its stage's value and
  bound as above and starts the next stage from the stored tensor with a zero input bound, exactly as the forward is judged:
  every bound is one stage deep, and what the block returns is held one stage deep to intermediates that are themselves held
  one stage deep to float64.  The same formulas, no new constant.
A second output of the native backward (dy2n = dx0 s2_next, the branch gradient of the block that consumes dx0) is judged
as swin_attn_half_ref does: dx0_ref s2_next within s2_next dx0_bound + U_OUT |.|, read back through the consumer's inv.
Bit-exact facts (check_dropped_rows): s1[b] == 0: the x1 rows of sample b equal x; s2[b] == 0: its x2 rows equal x1; both 0:
its dx0 rows equal dx2.

tests/test_swin_block_cpu.py proves on the host that an f32 and a bf16 emulation of the block sit inside every bound, chained
and cut, and that a list of wiring faults between the halves is rejected by the cut reference in both dtypes with the tensor
and the place named; tests/test_swin_block_gpu.py runs every route of both host paths against it."""
import torch

import attn_ref as A
import gemm_ref as G
import ln_ref as R
import misc_ref as Mi
import swin_attn_half_ref as H
from gemm_ref import U32, check_bound  # noqa: F401
from swin_attn_half_ref import ATTN_GRADS, BF, F32, MLP_GRADS, WS, failures, window_maps, worst_ratios  # noqa: F401

PARAMS = ("gamma1", "beta1", "wqkv", "bqkv", "wproj", "bproj", "table", "gamma2", "beta2", "w1", "b1", "w2", "b2")
SAVED = ("xn1w", "mean1", "rstd1", "qkv", "ao", "lse", "x1", "xn2", "mean2", "rstd2", "h", "act")
FORWARD = SAVED + ("x2",)
GRADS = ATTN_GRADS + MLP_GRADS                                   # all thirteen
BACKWARD = ("dx0",) + GRADS
STAGES = ("dy2", "dh", "dxn2", "dx1", "dyw", "dqkv", "dxn1w")    # what a run may hand over to cut the chain (logical order)
PLAN = ("perm", "inv", "count")


def ln_carry(e, xh, rstd, gam):
    """A perturbation bounded by e of the dy of a LayerNorm backward moves its dx by at most this (first order)."""
    ge = gam * e
    return rstd * (ge + ge.mean(1, keepdim=True) + xh * (ge * xh).mean(1, keepdim=True))


def plan_of(r, rows, dev):
    """(perm, inv int64 [rows], count) of the run: its row plan, or the identity for a dense run."""
    if "perm" in r:
        return r["perm"].long().to(dev), r["inv"].long().to(dev), int(r["count"])
    ident = torch.arange(rows, device=dev)
    return ident, ident, rows


def scale_rows(s, rows, Lt, dev):
    """[rows, 1] float64: the scale of each logical row's sample (ones without scales)."""
    if s is None:
        return torch.ones(rows, 1, dtype=torch.float64, device=dev)
    return s.double().to(dev)[torch.arange(rows, device=dev) // Lt][:, None]


def dense_saved(r, rows):
    """(xn2, h, act) of a run in logical order: a compact run's rows scattered through perm, the rows it never wrote zero."""
    if "perm" not in r:
        return r["xn2"], r["h"], r["act"]
    perm, inv, count = plan_of(r, rows, r["xn2"].device)
    out = [r["xn2"][inv]]
    for k in ("h", "act"):
        t = torch.zeros_like(r[k])
        t[perm[:count]] = r[k][:count]
        out.append(t)
    return tuple(out)


def mlp_forward(r, case, ref):
    """The Mlp half's forward stages into `ref` (module docstring), for either row order."""
    res, B, dt = case["res"], case["B"], case["dtype"]
    Lt, rows = res * res, B * res * res
    dev = r["x1"].device
    uo = R.u_out(dt)
    perm, inv, count = plan_of(r, rows, dev)
    x1, s2 = r["x1"], r.get("s2")
    f = R.fwd_ref(x1, r["gamma2"], r["beta2"], dt)
    ref["xn2"] = (f["y"], f["y_b"], r["xn2"][inv])
    ref["mean2"] = (f["mean"], f["mean_b"], r["mean2"])
    ref["rstd2"] = (f["rstd"], f["rstd_b"], r["rstd2"])
    a, b = G.logical(r["xn2"], r["w1"])
    v, pre, bound, _, pre_b = G.gemm_ref(a, b, out_dtype=dt, m_eff=count, bias=r["b1"], gelu=True)
    ref["act"] = (v, bound, r["act"][:count])
    ref["h"] = (pre, pre_b + 1e-30, r["h"][:count])
    a, b = G.logical(r["act"][:count], r["w2"])
    live = perm[:count]
    v, _, bound, _, _ = G.gemm_ref(a, b, out_dtype=dt, bias=r["b2"], rowscale=None if s2 is None else (s2, Lt), rowmap=live,
                                   residual=x1)
    x2_ref, x2_b = x1.double().clone(), uo * x1.double().abs() + 1e-30       # rows the plan drops: x1 (asserted bit for bit too)
    x2_ref[live], x2_b[live] = v, bound
    ref["x2"] = (x2_ref, x2_b, r["x2"])


def reference(r, case):
    """r: the tensors of one run, all on one device: inputs x, dx2, s1 / s2 (absent: None); PARAMS as the kernels read them
    (weights in the compute dtype, one-dimensional parameters and the bias table f32); SAVED; perm / inv / count of a compact
    run; outputs x2, dx0 and the thirteen GRADS; optionally any of STAGES (logical order; dxn1w of backward mode 2 as
    ln_ref.sum_parts of its parts), `dy2_pre` (True: the dy2 the block used came from its producer), dy2n with s2_next and
    inv_next.  case: dict(res, C, nH, B, dtype, shift, bwd).
    -> {name: (float64 value, bound, what the run produced)}."""
    res, C, nH, B, dt, shift, bwd = (case[k] for k in ("res", "C", "nH", "B", "dtype", "shift", "bwd"))
    Lt, nW, hd = res * res, (res // WS) ** 2, C // nH
    rows, nseq, scale = B * Lt, B * nW, (C // nH) ** -0.5
    dev = r["x"].device
    uo = R.u_out(dt)
    w2n, n2w = (t.to(dev) for t in window_maps(B, res, shift))
    x, x1, s1, s2 = r["x"], r["x1"], r.get("s1"), r.get("s2")
    perm, inv, count = plan_of(r, rows, dev)
    live = perm[:count]
    ref = {}
    # ---- forward: the attention half, stage by stage (swin_attn_half_ref), then the Mlp half
    f = R.fwd_ref(x[w2n], r["gamma1"], r["beta1"], dt)
    ref["xn1w"] = (f["y"], f["y_b"], r["xn1w"])
    ref["mean1"] = (f["mean"][n2w], f["mean_b"][n2w], r["mean1"])
    ref["rstd1"] = (f["rstd"][n2w], f["rstd_b"][n2w], r["rstd1"])
    a, b = G.logical(r["xn1w"], r["wqkv"])
    v, _, bound, _, _ = G.gemm_ref(a, b, out_dtype=dt, bias=r["bqkv"])
    ref["qkv"] = (v, bound, r["qkv"])
    a, b = G.logical(r["ao"], r["wproj"])
    v, _, bound, out_rows, _ = G.gemm_ref(a, b, out_dtype=dt, bias=r["bproj"], rowmap=w2n,
                                          rowscale=None if s1 is None else (s1, Lt), residual=x)
    ref["x1"] = (v, bound, x1[out_rows])
    mlp_forward(r, case, ref)

    # ---- backward
    def stage(name, v, e):
        """Judge the run's own stored `name`, if it hands it over, and start the next stage from it: the chain is cut there."""
        if name not in r:
            return v, e
        ref[name] = (v, e, r[name])
        return r[name].double(), torch.full_like(e, 1e-30)

    def scatter(vc, ec):
        v = torch.zeros(rows, vc.shape[1], dtype=torch.float64, device=dev)
        e = torch.full_like(v, 1e-30)
        v[live], e[live] = vc, ec
        return v, e

    wp, wq, w1, w2 = (r[k].double() for k in ("wproj", "wqkv", "w1", "w2"))       # as stored: y = a W^T, da = dy W
    dx2 = r["dx2"].double()
    srow2, srow1 = scale_rows(s2, rows, Lt, dev), scale_rows(s1, rows, Lt, dev)
    dy2 = dx2 * srow2
    if s2 is None:
        e_dy2 = torch.full_like(dy2, 1e-30)
    elif r.get("dy2_pre"):
        e_dy2 = uo * srow2 * dx2.abs() + (2 * U32 + uo) * dy2.abs() + 1e-30
    else:
        e_dy2 = (U32 + uo) * dy2.abs() + 1e-30
    dy2, e_dy2 = stage("dy2", dy2, e_dy2)
    dy2c, e_dy2c = dy2[live], e_dy2[live]
    hc, actc, xn2c = r["h"][:count], r["act"][:count].double(), r["xn2"][:count].double()
    dh, _, dh_b, _, _ = G.gemm_ref(dy2c, w2, out_dtype=dt, mul_gelu_grad=hc)
    dh_b = dh_b + (e_dy2c @ w2.abs()) * (G.gelu_grad64(hc.double()).abs() + G.ERFC_ABS)
    dh, e_dh = stage("dh", *scatter(dh, dh_b))
    dhc, e_dhc = dh[live], e_dh[live]
    dxn2, _, dxn2_b, _, _ = G.gemm_ref(dhc, w1, out_dtype=dt)
    dxn2, e_dxn2 = stage("dxn2", *scatter(dxn2, dxn2_b + e_dhc @ w1.abs()))
    # norm2's backward: dx1 and the branch output dyw (window order, s1 applied) from the same launch
    mean2, rstd2 = r["mean2"], r["rstd2"]
    bw = R.bwd_ref(x1, dxn2, mean2, rstd2, r["gamma2"], dt, dres=r["dx2"], zscale=None if s1 is None else srow1[:, 0])
    gam = r["gamma2"].double().abs()[None, :]
    rs = rstd2.double()[:, None]
    xh = ((x1.double() - mean2.double()[:, None]) * rs).abs()
    carry = ln_carry(e_dxn2, xh, rs, gam)
    ref["norm2.weight"] = (bw["dg"], bw["dg_b"] + (e_dxn2 * xh).sum(0), r["norm2.weight"])
    ref["norm2.bias"] = (bw["db"], bw["db_b"] + e_dxn2.sum(0), r["norm2.bias"])
    dx1, e_dx1 = stage("dx1", bw["dx"], bw["dx_b"] + carry)
    dyw, e_dyw = stage("dyw", bw["dz"][w2n], (bw["dz_b"] + carry * srow1)[w2n])
    # the attention half's backward (swin_attn_half_ref, its dyw and dres now those of a live Mlp half)
    dO, _, dO_b, _, _ = G.gemm_ref(dyw, wp, out_dtype=dt)
    dO_b = dO_b + e_dyw @ wp.abs()
    bias = A.swin_bias(r["table"], nW, res, shift, nseq)
    at = A.AttnRef(r["qkv"], dO, nseq=nseq, L=WS * WS, nH=nH, hd=hd, scale=scale, bias=bias, dtype=dt, dout_err=dO_b)
    ref["ao"] = (at.out, at.out_b, r["ao"])
    ref["lse"] = (H.lse_rows(at.lse), H.lse_rows(at.lse_b), H.lse_rows(r["lse"]))
    ref["dbias_table"] = at.dbias_table() + (r["dbias_table"],)
    dqkv, e_dqkv = stage("dqkv", at.dqkv, at.dqkv_b)
    dxn, _, dxn_b, _, _ = G.gemm_ref(dqkv, wq, out_dtype=dt)
    dxn_b = dxn_b + e_dqkv @ wq.abs()
    if bwd == 2:
        dxn_b = dxn_b + uo * (dqkv.abs() @ wq.abs())
    dxn, e_dxn = stage("dxn1w", dxn, dxn_b)
    e_in = e_dxn[n2w]
    mean1, rstd1 = r["mean1"], r["rstd1"]
    bw = R.bwd_ref(x, dxn[n2w], mean1, rstd1, r["gamma1"], dt, dres=dx1)
    gam = r["gamma1"].double().abs()[None, :]
    rs = rstd1.double()[:, None]
    xh = ((x.double() - mean1.double()[:, None]) * rs).abs()
    dx0_b = bw["dx_b"] + ln_carry(e_in, xh, rs, gam) + e_dx1
    ref["dx0"] = (bw["dx"], dx0_b, r["dx0"])
    ref["norm1.weight"] = (bw["dg"], bw["dg_b"] + (e_in * xh).sum(0), r["norm1.weight"])
    ref["norm1.bias"] = (bw["db"], bw["db_b"] + e_in.sum(0), r["norm1.bias"])
    # weight and bias gradients: dY^T X over the live rows
    for name, dY, e_dY, X in (("fc2", dy2c, e_dy2c, actc), ("fc1", dhc, e_dhc, xn2c), ("proj", dyw, e_dyw, r["ao"].double()),
                              ("qkv", dqkv, e_dqkv, r["xn1w"].double())):
        v, _, bound, _, _ = G.gemm_ref(dY.t(), X, out_dtype=F32)
        ref[name + ".weight"] = (v, bound + e_dY.t() @ X.abs(), r[name + ".weight"])
        v, bound = G.colsum_ref(dY.t())
        ref[name + ".bias"] = (v, bound + e_dY.sum(0), r[name + ".bias"])
    if "dy2n" in r:
        s2n = scale_rows(r["s2_next"], rows, Lt, dev)
        dz = bw["dx"] * s2n
        got = r["dy2n"][r["inv_next"].long()] if "inv_next" in r else r["dy2n"]         # dy2n[inv[row]] = dx0[row] s2_next
        ref["dy2n"] = (dz, s2n * dx0_b + uo * dz.abs() + 1e-30, got)
    assert set(ref) - set(STAGES) - {"dy2n"} == set(FORWARD) | set(BACKWARD)
    return ref


def signal_to_bound(ref):
    """{name: median |value| / median bound over the elements whose value is not zero (rows of dropped samples are)}: how far
    the values of a tensor stand above their own bound (below ~1 the bound cannot see a fault of the size of the tensor itself)."""
    out = {}
    for k, (v, b, _) in ref.items():
        m = v != 0
        out[k] = float(v[m].abs().median() / b[m].median()) if bool(m.any()) else float("inf")
    return out


def dropped(s):
    return [] if s is None else [b for b, v in enumerate(s.tolist()) if v == 0.0]


def check_dropped_rows(r, case, label=""):
    """s1[b] == 0: the x1 rows of sample b equal x; s2[b] == 0: its x2 rows equal x1; both: its dx0 rows equal dx2."""
    Lt = case["res"] ** 2
    d1, d2 = dropped(r.get("s1")), dropped(r.get("s2"))
    for b in range(case["B"]):
        sl = slice(b * Lt, (b + 1) * Lt)
        where = f"of dropped sample {b} (rows from {b * Lt})"
        if b in d1:
            Mi.check_equal(r["x1"][sl], r["x"][sl], f"{label} x1 rows {where}".strip())
        if b in d2:
            Mi.check_equal(r["x2"][sl], r["x1"][sl], f"{label} x2 rows {where}".strip())
        if b in d1 and b in d2:
            Mi.check_equal(r["dx0"][sl], r["dx2"][sl], f"{label} dx0 rows {where}".strip())
