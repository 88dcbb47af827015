"""float64 reference of the attention half of a Swin block, x1 = x + s1 proj(W-MSA(qkv(norm1(x)))), and of its backward,
with a per-element bound for every tensor the block functions hand back (swin.py _block_fwd / _block_bwd and csrc/host.cpp
swin_block_fwd / swin_block_bwd called with s2 = 0, so that the block IS this half).

Built only from tests/ln_ref.py, tests/gemm_ref.py, tests/attn_ref.py and tests/misc_ref.py with their constants unchanged:
this module introduces no tolerance of its own.  The window maps are stated here from the definition (roll by -shift, then
window partition), not taken from mvlt_amd.indexing.

The s2 = 0 premises are asserted, not assumed: x2 == x1 bit for bit, and the six Mlp-side gradients (fc1 / fc2 weight and
bias, norm2 weight and bias) are exactly zero -- the evidence that dy2 = 0, hence dx1 == dx2 bit for bit (norm2's backward
adds the residual gradient to an exact zero).  The reference takes dx1 = dx2.

Forward, each stage from the operand the kernel itself read, so the bounds do not compound:
  xn1w, mean1, rstd1   ln_ref.fwd_ref of x[w2n] (the statistics are stored per token row)
  qkv                  gemm_ref from the saved xn1w
  ao, lse              attn_ref.AttnRef from the saved qkv with swin_bias
  x1                   gemm_ref from the saved ao: bias, row scale (s1, Lt), row map w2n, residual x
Backward.  dqkv and dxn1w are not returned, so their float64 values are chained, and the bound of each stage carries the bound
of its input through the stage's own linear map, first order, with no constant of its own (the rule of
tests/test_swin_droppath_compact_gpu.py):
  dyw   = dx2[w2n] s1, stored in the compute dtype by norm2's backward: one f32 product and one store rounding,
          (U32 + U_OUT) |dyw|; exact without s1 (a gather)
  dO    = dyw Wproj.  Backward mode 0: a product of its own.  Modes 1 / 2 form it inside the attention backward per head,
          an f32 sum over the C inputs rounded to bf16 once: the same arithmetic, so gemm_ref's bound serves all three
          (C_ACC U32 sqrt(C) |dyw| |Wproj| + U_OUT |dO|; test_attention_route / test_swin_wmsa2_stage_by_stage write the
          rounding as U_BF16 |dyw| |Wproj|, which is never smaller).  e_dyw |Wproj| is added.
  dqkv, dbias_table    AttnRef(dout_err = the bound of dO)
  dxn1w = dqkv Wqkv: gemm_ref's bound + dqkv_b |Wqkv|.  Mode 2 writes nH / 3 partial products, each rounded to bf16, which
          norm1's backward adds in f32 and rounds once (ln_ref.sum_parts): the rounding of the sum is gemm_ref's output
          rounding; the roundings of the parts add U_OUT sum_p |part_p| <= U_OUT |dqkv| |Wqkv| (the parts split the columns
          of dqkv between them)
  dx0, norm1.weight, norm1.bias   ln_ref.bwd_ref with dy = dxn1w gathered through n2w and dres = dx2; the bound e of dxn1w
          enters through the LayerNorm Jacobian, rstd (|gamma| e + mean(|gamma| e) + |xh| mean(|gamma| e |xh|)), and through
          sum_r e |xh| / sum_r e for the two parameter gradients
  proj.weight = dyw^T ao, proj.bias = colsum(dyw)     operands known; e_dyw carried through |ao| / the sum
  qkv.weight = dqkv^T xn1w, qkv.bias = colsum(dqkv)   dqkv_b carried through |xn1w| / the sum
Bit-exact facts of the samples DropPath drops (s1[b] == 0): their x1 rows equal x, their dx0 rows equal dx2.
A second output of the native backward (dx0 s2_next, the next consumer's branch gradient) must equal dx0_ref s2_next within
s2_next dx0_bound + U_BF16 |.|, in the consumer's `inv` order when it runs on the kept rows only.

tests/test_swin_attn_half_cpu.py proves on the host that an f32 emulation of the half sits inside every bound and that a list
of wiring faults is rejected with the tensor and the place named; tests/test_swin_attn_half_gpu.py runs every route of both
host paths against it."""
import math

import torch

import attn_ref as A
import gemm_ref as G
import ln_ref as R
import misc_ref as Mi
from gemm_ref import U32, U_BF16, check_bound

BF, F32 = torch.bfloat16, torch.float32
WS = 7                                      # window side; L = 49 tokens per window
ATTN_GRADS = ("norm1.weight", "norm1.bias", "qkv.weight", "qkv.bias", "proj.weight", "proj.bias", "dbias_table")
MLP_GRADS = ("fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias", "norm2.weight", "norm2.bias")
SAVED = ("xn1w", "mean1", "rstd1", "qkv", "ao", "lse")
COMPARED = ("x1", "dx0") + ATTN_GRADS        # what any two runs of the same inputs share, whatever their routes


def window_maps(B, res, shift):
    """(w2n, n2w) int64 [B res res]: w2n[window row] = the token row that sits there after roll(-shift, -shift) and the
    window partition; n2w its inverse."""
    idx = torch.arange(B * res * res).view(B, res, res)
    if shift:
        idx = torch.roll(idx, shifts=(-shift, -shift), dims=(1, 2))
    n = res // WS
    w2n = idx.view(B, n, WS, n, WS).permute(0, 1, 3, 2, 4).reshape(-1)
    n2w = torch.empty_like(w2n)
    n2w[w2n] = torch.arange(B * res * res)
    return w2n, n2w


def lse_rows(t):
    """[nseq, nH, L] -> [nseq L, nH]: row = sequence * 49 + query, column = head (the layout attn_ref.check_lse names)."""
    nseq, nH, L = t.shape
    return t.permute(0, 2, 1).reshape(nseq * L, nH)


def dropped_samples(r):
    s1 = r.get("s1")
    return [] if s1 is None else [b for b, v in enumerate(s1.tolist()) if v == 0.0]


def reference(r, case):
    """r: the tensors of one run (inputs x, dx2, s1 or None, the parameters gamma1, beta1, wqkv, bqkv, wproj, bproj, table;
    saved xn1w, mean1, rstd1, qkv, ao, lse, x1; outputs x2, dx0, the seven attention-side and six Mlp-side gradients;
    optionally dy2n, s2_next and inv_next), all on one device.  case: dict(res, C, nH, B, dtype, shift, bwd) with bwd the
    backward mode the run took (swin._bwd_mode).  -> {name: (float64 value, bound, what the run produced)}."""
    res, C, nH, B, dt, shift, bwd = (case[k] for k in ("res", "C", "nH", "B", "dtype", "shift", "bwd"))
    Lt, nW, hd = res * res, (res // WS) ** 2, C // nH
    rows, nseq, scale = B * Lt, B * nW, (C // nH) ** -0.5
    dev = r["x"].device
    uo = R.u_out(dt)
    w2n, n2w = (t.to(dev) for t in window_maps(B, res, shift))
    x, s1 = r["x"], r.get("s1")
    # ---- the s2 = 0 premises
    Mi.check_equal(r["x2"], r["x1"], "s2 = 0: x2 == x1 bit for bit")
    for k in MLP_GRADS:
        Mi.check_zero(r[k], f"s2 = 0: {k} is exactly zero")
    ref = {}
    # ---- forward, stage by stage
    f = R.fwd_ref(x[w2n], r["gamma1"], r["beta1"], dt)
    ref["xn1w"] = (f["y"], f["y_b"], r["xn1w"])
    ref["mean1"] = (f["mean"][n2w], f["mean_b"][n2w], r["mean1"])
    ref["rstd1"] = (f["rstd"][n2w], f["rstd_b"][n2w], r["rstd1"])
    a, b = G.logical(r["xn1w"], r["wqkv"])
    v, _, bound, _, _ = G.gemm_ref(a, b, out_dtype=dt, bias=r["bqkv"])
    ref["qkv"] = (v, bound, r["qkv"])
    # ---- dyw and dO (module docstring), then one AttnRef for the forward and the backward of the attention itself
    dx2 = r["dx2"].double()
    if s1 is None:
        dyw = dx2[w2n]
        e_dyw = torch.zeros_like(dyw)
    else:
        dyw = dx2[w2n] * s1.double()[w2n // Lt][:, None]
        e_dyw = (U32 + uo) * dyw.abs()
    wp, wq = r["wproj"].double(), r["wqkv"].double()          # [C, C] and [3C, C] as stored: y = a W^T, da = dy W
    dO, _, dO_b, _, _ = G.gemm_ref(dyw, wp, out_dtype=dt)
    dO_b = dO_b + e_dyw @ wp.abs()
    bias = A.swin_bias(r["table"], nW, res, shift, nseq)
    at = A.AttnRef(r["qkv"], dO, nseq=nseq, L=WS * WS, nH=nH, hd=hd, scale=scale, bias=bias, dtype=dt, dout_err=dO_b)
    ref["ao"] = (at.out, at.out_b, r["ao"])
    ref["lse"] = (lse_rows(at.lse), lse_rows(at.lse_b), lse_rows(r["lse"]))
    a, b = G.logical(r["ao"], r["wproj"])
    v, _, bound, out_rows, _ = G.gemm_ref(a, b, out_dtype=dt, bias=r["bproj"], rowmap=w2n,
                                          rowscale=None if s1 is None else (s1, Lt), residual=x)
    ref["x1"] = (v, bound, r["x1"][out_rows])
    # ---- backward
    dqkv, dqkv_b = at.dqkv, at.dqkv_b
    ref["dbias_table"] = at.dbias_table() + (r["dbias_table"],)
    dxn, _, dxn_b, _, _ = G.gemm_ref(dqkv, wq, out_dtype=dt)
    dxn_b = dxn_b + dqkv_b @ wq.abs()
    if bwd == 2:
        dxn_b = dxn_b + uo * (dqkv.abs() @ wq.abs())
    e_in = dxn_b[n2w]
    mean, rstd = r["mean1"], r["rstd1"]
    bw = R.bwd_ref(x, dxn[n2w], mean, rstd, r["gamma1"], dt, dres=r["dx2"])
    gam = r["gamma1"].double().abs()[None, :]
    rs = rstd.double()[:, None]
    xh = ((x.double() - mean.double()[:, None]) * rs).abs()
    ge = gam * e_in
    dx0_b = bw["dx_b"] + rs * (ge + ge.mean(1, keepdim=True) + xh * (ge * xh).mean(1, keepdim=True))
    ref["dx0"] = (bw["dx"], dx0_b, r["dx0"])
    ref["norm1.weight"] = (bw["dg"], bw["dg_b"] + (e_in * xh).sum(0), r["norm1.weight"])
    ref["norm1.bias"] = (bw["db"], bw["db_b"] + e_in.sum(0), r["norm1.bias"])
    aov, xnv = r["ao"].double(), r["xn1w"].double()
    v, _, bound, _, _ = G.gemm_ref(dyw.t(), aov, out_dtype=F32)
    ref["proj.weight"] = (v, bound + e_dyw.t() @ aov.abs(), r["proj.weight"])
    v, bound = G.colsum_ref(dyw.t())
    ref["proj.bias"] = (v, bound + e_dyw.sum(0), r["proj.bias"])
    v, _, bound, _, _ = G.gemm_ref(dqkv.t(), xnv, out_dtype=F32)
    ref["qkv.weight"] = (v, bound + dqkv_b.t() @ xnv.abs(), r["qkv.weight"])
    v, bound = G.colsum_ref(dqkv.t())
    ref["qkv.bias"] = (v, bound + dqkv_b.sum(0), r["qkv.bias"])
    if "dy2n" in r:
        s2n = r["s2_next"].double()[torch.arange(rows, device=dev) // Lt][:, None]
        dz = bw["dx"] * s2n
        got = r["dy2n"][r["inv_next"].long()] if "inv_next" in r else r["dy2n"]         # dy2n[inv[row]] = dx0[row] s2_next
        ref["dy2n"] = (dz, s2n * dx0_b + U_BF16 * dz.abs() + 1e-30, got)
    return ref


def worst_ratios(ref):
    """{name: the largest |got - value| / bound of the tensor} (inf where an output is not finite)."""
    out = {}
    for k, (v, b, got) in ref.items():
        g = got.double().to(v.device)
        ratio = torch.where(torch.isfinite(g), (g - v).abs() / b, torch.full_like(v, math.inf))
        out[k] = float(ratio.max()) if ratio.numel() else 0.0
    return out


def failures(ref, label=""):
    """{name: check_bound's message} of every tensor that leaves its bound: the message names the worst row and column."""
    bad = {}
    for k, (v, b, got) in ref.items():
        try:
            check_bound(got, v, b, f"{label} {k}".strip())
        except AssertionError as e:
            bad[k] = str(e)
    return bad


def check_dropped_rows(r, case, label=""):
    """s1[b] == 0: the x1 rows of sample b equal x and its dx0 rows equal dx2, bit for bit."""
    Lt = case["res"] ** 2
    for b in dropped_samples(r):
        sl = slice(b * Lt, (b + 1) * Lt)
        Mi.check_equal(r["x1"][sl], r["x"][sl], f"{label} x1 rows of dropped sample {b} (rows from {b * Lt})".strip())
        Mi.check_equal(r["dx0"][sl], r["dx2"][sl], f"{label} dx0 rows of dropped sample {b} (rows from {b * Lt})".strip())
