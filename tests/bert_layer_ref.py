"""float64 reference of one BertLayer of the MVLBert encoder, forward and backward, with a per-element bound for every tensor
the layer functions save or hand back (bert.py _layer_fwd / _layer_bwd and csrc/host.cpp bert_layer_fwd / bert_layer_bwd).

Built only from tests/gemm_ref.py, tests/ln_ref.py, tests/attn_ref.py and tests/misc_ref.py with their constants unchanged:
this module introduces no tolerance of its own.  The layer, from the definition (post-LayerNorm BERT, eps = 1e-12 as f32):

    qkv = x [Wq; Wk; Wv]^T + [bq; bk; bv]        one [3H, H] product; the span order is query, key, value -- the reference
                                                 is handed the three weights and biases of the module SEPARATELY and joins
                                                 them in this order itself, it does not take the order from the arena
    ctx = softmax(scale q.k + mask) (x keep_a / (1 - p_a)) v     mask: attn_ref.bert_bias (bidirectional key mask from the ids
                                                 and image_mask | seq2seq); keep_a: tag 8 i + 0 at ((seq nH + h) L + q) L + k
    y1  = dropout(ctx Wo^T + bo) + x             tag 8 i + 1 at row C + column
    x1  = LayerNorm(y1) g1 + b1
    h   = x1 Wi^T + bi,   act = GELU(h)
    y2  = dropout(act Wo2^T + bo2) + x1          tag 8 i + 2
    x2  = LayerNorm(y2) g2 + b2

Rows.  Dense: row = sample * L + position.  Packed: sample s holds the rows row_start[s] .. + seq_len[s], the sequences follow
each other without a gap, and `rows_dev` (their total) may be smaller than the allocation: only the rows below it are
computed and compared, and nothing at or beyond it may enter a gradient (the GPU test fills those rows of x and dx with NaN
and asks every gradient to be finite).

Forward, each stage from the operand the kernel itself read (the SAVED tensor), so the bounds do not compound:
  qkv                  gemm_ref(x, Wqkv, bias)
  ctx, lse             attn_ref.AttnRef from the saved qkv (bias, keep, pack)
  y1                   gemm_ref(saved ctx, Wo, bias, keep, drop_p, residual = x)
  x1, mean1, rstd1     ln_ref.fwd_ref(saved y1, eps)
  h, act               gemm_ref(saved x1, Wi, bias, gelu): pre / pre_err and the value
  y2                   gemm_ref(saved act, Wo2, bias, keep, drop_p, residual = saved x1)
  x2, mean2, rstd2     ln_ref.fwd_ref(saved y2, eps)
Backward.  Only dx_in and the twelve parameter gradients come back, so dy2, dz2, dh, dx1, dy1, dz1, dctx and dqkv are chained in
float64, and the bound of each stage is the stage's own bound (as if its input were exact) plus the bound e of its input
carried through the stage's own linear map, first order, no constant of its own (the rules of tests/swin_attn_half_ref.py):
  dy2, dz2   ln_ref.bwd_ref(saved y2, dx, saved stats, keep tag 8 i + 2): inputs known, nothing carried.  p_h = 0: there is
             no branch output, dz2 IS dy2 (the same stored tensor), and the reference takes the same object
  dh  = (dz2 Wo2) gelu'(h)          + (e_dz2 |Wo2|) |gelu'(h)|
  dx1 = dh Wi + dy2                 + e_dh |Wi| + e_dy2
  dy1, dz1   bwd_ref(saved y1, dx1, ...): e_dx1 enters through the LayerNorm Jacobian,
             rstd (|g| e + mean(|g| e) + |xh| mean(|g| e |xh|)), times keep / (1 - p) for dz1
  dctx = dz1 Wo                     + e_dz1 |Wo|
  dqkv       AttnRef(dout = dctx, dout_err = e_dctx)
  dx_in = dqkv Wqkv + dy1           + e_dqkv |Wqkv| + e_dy1
  W grads    gemm_ref(dY^T, X, out f32) over the rows below rows_dev, X the saved act / x1 / ctx / x, dY the chained dz2 / dh /
             dz1 / dqkv: + e_dY^T |X|;  bias grads gemm_ref.colsum_ref: + sum_r e_dY
  ln2.weight / ln2.bias   bwd_ref's own (inputs known);  ln1.weight / ln1.bias: + sum_r e_dx1 |xh| / sum_r e_dx1
The key third of qkv.bias is zero in exact arithmetic: every logit of a query moves by the same q.b_k when the key bias
moves, and softmax does not see a shift of a whole row, so sum_q dS[q, k] scale q = dK sums to zero over the keys.  Its chained
float64 value is rounding noise and its bound exceeds its value everywhere: there only the bound is asserted
(tests/test_bert_layer_cpu.py asserts bound > |value| on that third).

Cutting the chain.  Carried through |W| as a worst case, a bound grows by about sqrt(K) per product against a signal that
cancels, and gemm_ref's own term C_ACC 2^-24 sqrt(K) S is of the same kind.  Behind four products, two LayerNorm backwards
and the attention backward the chained bound of dqkv, hence of dx_in, qkv.weight and qkv.bias, EXCEEDS the signal -- in bf16
by three orders of magnitude and in f32 still by one (tests/test_bert_layer_cpu.py prints signal / bound per tensor; at
H = 128 in f32: fc2.weight 1e4, fc1.weight 900, o.weight 30, qkv.weight 0.09, dx_in 0.04).  A fault that shows only there
("dx_in residual from dz1") passes the chained reference in f32 too.  The identity the issue of this reference proposed,
dz1 from dctx = dz1 Wo, cannot be used: dctx is not returned either, and the returned o.weight = dz1^T ctx has lost the row
index.  No returned tensor determines an intermediate row by row, so the chain cannot be cut from the layer's outputs alone.
It is cut from the side instead: a run may hand over the STORED intermediates STAGES (dy2, dz2, dh, dx1, dy1, dz1, dctx,
dqkv) of a stage-by-stage replay of the backward -- the same eight launches issued one by one, from the definition, on the
run's own saved tensors (tests/test_bert_layer_gpu.py replay_backward; the kernels are deterministic).  reference() then
judges each handed-over tensor against its stage's value and bound as above and starts the next stage from the stored tensor
with a zero input bound, exactly as the forward is judged: every bound is one stage deep, and what the layer returns is held
one stage deep to intermediates that are themselves held one stage deep to float64.  Nothing else changes: the same formulas,
no new constant.  The chained judgement stays and is asserted beside the cut one.

tests/test_bert_layer_cpu.py proves on the host that an f32 and a bf16 emulation of the layer sit inside every bound, chained
and cut, and that a list of wiring faults is rejected by the cut reference in both dtypes with the tensor and the place named,
and records which of them the chained reference accepts; tests/test_bert_layer_gpu.py runs both host paths against it."""
import torch

import attn_ref as A
import gemm_ref as G
import ln_ref as R
import misc_ref as Mi  # noqa: F401  (check_equal: the tests' bit-equality checks go through this module)
from gemm_ref import check_bound  # noqa: F401
from swin_attn_half_ref import failures, worst_ratios  # noqa: F401  (shared judges, re-exported)

BF, F32 = torch.bfloat16, torch.float32
FORWARD = ("qkv", "ctx", "lse", "y1", "mean1", "rstd1", "x1", "h", "act", "y2", "mean2", "rstd2", "x2")
GRADS = ("qkv.weight", "qkv.bias", "o.weight", "o.bias", "ln1.weight", "ln1.bias", "fc1.weight", "fc1.bias", "fc2.weight",
         "fc2.bias", "ln2.weight", "ln2.bias")
BACKWARD = ("dx_in",) + GRADS
PARAMS = ("wq", "wk", "wv", "bq", "bk", "bv", "wo", "bo", "g1", "b1", "wi", "bi", "wo2", "bo2", "g2", "b2")
STAGES = ("dy2", "dz2", "dh", "dx1", "dy1", "dz1", "dctx", "dqkv")        # what a run may hand over to cut the chain
QKV_GRADS = ("query.weight", "key.weight", "value.weight", "query.bias", "key.bias", "value.bias")


def layout(case):
    """(row_index int64 [B L]: the activation row of dense row (sample, position) or -1, seq_len int32 [B] or None, the number
    of rows computed).  Packed sequences follow each other without a gap."""
    B, L = case["B"], case["n_img"] + 2 + case["T"]
    lens = case.get("lens")
    if lens is None:
        return None, None, B * L
    row_index = torch.full((B * L,), -1, dtype=torch.int64)
    r = 0
    for s, ln in enumerate(lens):
        row_index[s * L: s * L + ln] = r + torch.arange(ln)
        r += ln
    return row_index, torch.tensor(lens, dtype=torch.int32), r


def eps32(case):
    return float(torch.tensor(case["eps"], dtype=torch.float32))


def lse_rows(t, valid):
    """[B, nH, L] -> [B L, nH] with the queries a sequence does not have set to 0 (attn_ref.check_lse)."""
    B, nH, L = t.shape
    t = t.double().permute(0, 2, 1).reshape(B * L, nH)
    return torch.where(valid, t, torch.zeros_like(t))


def ln_carry(e, xh, rstd, gam):
    """A perturbation bounded by e of the dy of a LayerNorm backward moves its dx by at most this (first order)."""
    ge = gam * e
    return rstd * (ge + ge.mean(1, keepdim=True) + xh * (ge * xh).mean(1, keepdim=True))


def reference(r, case):
    """r: the tensors of one run, all on one device: inputs x, dx [rows, H]; the parameters PARAMS as the kernels read them
    (weights in the compute dtype, one-dimensional parameters f32); the saved qkv, ctx, lse, y1, mean1, rstd1, x1, h, act, y2,
    mean2, rstd2; the outputs x2, dx_in and the gradients: QKV_GRADS of the three modules and GRADS[2:].
    case: dict(H, nH, I, B, T, n_img, dtype, s2s, p_h, p_a, seed, layer, eps; ids [B, T] / image_mask [B, n_img] or None
    (bidirectional mode); lens: rows of each packed sample or None).  -> {name: (float64 value, bound, what the run produced)}
    over the rows that are computed."""
    H, nH, B, dt = case["H"], case["nH"], case["B"], case["dtype"]
    L, hd = case["n_img"] + 2 + case["T"], case["H"] // case["nH"]
    p_h, p_a, seed, i = case["p_h"], case["p_a"], case["seed"], case["layer"]
    dev = r["x"].device
    eps = eps32(case)
    row_index, seq_len, rv = layout(case)
    pack = None if row_index is None else (row_index.to(dev), seq_len.to(dev))
    s = lambda k: r[k][:rv]                                                   # noqa: E731
    wqkv = torch.cat([r["wq"], r["wk"], r["wv"]], 0)                          # [3H, H]: query, key, value
    bqkv = torch.cat([r["bq"], r["bk"], r["bv"]], 0)
    keep_a = A.attn_keep(seed, 8 * i + 0, p_a, B, nH, L, device=dev) if p_a > 0 else None
    keep1 = R.dropout_keep(seed, 8 * i + 1, p_h, rv, H, device=dev) if p_h > 0 else None
    keep2 = R.dropout_keep(seed, 8 * i + 2, p_h, rv, H, device=dev) if p_h > 0 else None
    ids, im = case.get("ids"), case.get("image_mask")
    bias = A.bert_bias(case["s2s"], B, L, case["n_img"], ids, im).to(dev)
    ref = {}
    # ---- forward, stage by stage
    a, b = G.logical(s("x"), wqkv)
    v, _, bound, _, _ = G.gemm_ref(a, b, out_dtype=dt, bias=bqkv)
    ref["qkv"] = (v, bound, s("qkv"))
    a, b = G.logical(s("ctx"), r["wo"])
    v, _, bound, _, _ = G.gemm_ref(a, b, out_dtype=dt, bias=r["bo"], keep=keep1, drop_p=p_h, residual=s("x"))
    ref["y1"] = (v, bound, s("y1"))
    f = R.fwd_ref(s("y1"), r["g1"], r["b1"], dt, eps=eps)
    ref["x1"], ref["mean1"], ref["rstd1"] = (f["y"], f["y_b"], s("x1")), (f["mean"], f["mean_b"], s("mean1")), \
        (f["rstd"], f["rstd_b"], s("rstd1"))
    a, b = G.logical(s("x1"), r["wi"])
    v, pre, bound, _, pre_b = G.gemm_ref(a, b, out_dtype=dt, bias=r["bi"], gelu=True)
    ref["h"], ref["act"] = (pre, pre_b + 1e-30, s("h")), (v, bound, s("act"))
    a, b = G.logical(s("act"), r["wo2"])
    v, _, bound, _, _ = G.gemm_ref(a, b, out_dtype=dt, bias=r["bo2"], keep=keep2, drop_p=p_h, residual=s("x1"))
    ref["y2"] = (v, bound, s("y2"))
    f = R.fwd_ref(s("y2"), r["g2"], r["b2"], dt, eps=eps)
    ref["x2"], ref["mean2"], ref["rstd2"] = (f["y"], f["y_b"], s("x2")), (f["mean"], f["mean_b"], s("mean2")), \
        (f["rstd"], f["rstd_b"], s("rstd2"))
    # ---- backward chain down to dctx (module docstring)
    wo, wi, wo2, wq = r["wo"].double(), r["wi"].double(), r["wo2"].double(), wqkv.double()       # as stored: y = a W^T, da = dy W
    def stage(name, v, e):
        """Judge the run's own stored `name`, if it hands it over, and start the next stage from it: the chain is cut there."""
        if name not in r:
            return v, e
        ref[name] = (v, e, s(name))
        return s(name).double(), torch.zeros_like(e)

    bw = R.bwd_ref(s("y2"), s("dx"), s("mean2"), s("rstd2"), r["g2"], dt, keep=keep2, p=p_h)
    if p_h == 0:
        assert bw["dz"] is bw["dx"], "p_h = 0: dz is dy"
    dy2, e_dy2 = stage("dy2", bw["dx"], bw["dx_b"])
    dz2, e_dz2 = (dy2, e_dy2) if p_h == 0 else stage("dz2", bw["dz"], bw["dz_b"])
    ref["ln2.weight"], ref["ln2.bias"] = (bw["dg"], bw["dg_b"], r["ln2.weight"]), (bw["db"], bw["db_b"], r["ln2.bias"])
    hv = s("h")
    dh, _, dh_b, _, _ = G.gemm_ref(dz2, wo2, out_dtype=dt, mul_gelu_grad=hv)
    dh, e_dh = stage("dh", dh, dh_b + (e_dz2 @ wo2.abs()) * G.gelu_grad64(hv.double()).abs())
    dx1, _, dx1_b, _, _ = G.gemm_ref(dh, wi, out_dtype=dt, residual=dy2)
    dx1, e_dx1 = stage("dx1", dx1, dx1_b + e_dh @ wi.abs() + e_dy2)
    bw = R.bwd_ref(s("y1"), dx1, s("mean1"), s("rstd1"), r["g1"], dt, keep=keep1, p=p_h)
    gam = r["g1"].double().abs()[None, :]
    rs = s("rstd1").double()[:, None]
    xh = ((s("y1").double() - s("mean1").double()[:, None]) * rs).abs()
    carry = ln_carry(e_dx1, xh, rs, gam)
    dy1, e_dy1 = stage("dy1", bw["dx"], bw["dx_b"] + carry)
    if p_h == 0:
        assert bw["dz"] is bw["dx"], "p_h = 0: dz is dy"
        dz1, e_dz1 = dy1, e_dy1
    else:
        dz1, e_dz1 = stage("dz1", bw["dz"], bw["dz_b"] + carry * keep1.double() / (1.0 - p_h))
    ref["ln1.weight"] = (bw["dg"], bw["dg_b"] + (e_dx1 * xh).sum(0), r["ln1.weight"])
    ref["ln1.bias"] = (bw["db"], bw["db_b"] + e_dx1.sum(0), r["ln1.bias"])
    dctx, _, dctx_b, _, _ = G.gemm_ref(dz1, wo, out_dtype=dt)
    dctx, e_dctx = stage("dctx", dctx, dctx_b + e_dz1 @ wo.abs())
    # ---- one AttnRef for the forward and the backward of the attention itself
    at = A.AttnRef(s("qkv"), dctx, nseq=B, L=L, nH=nH, hd=hd, scale=hd ** -0.5, bias=bias, dtype=dt, keep=keep_a, p=p_a,
                   pack=pack, dout_err=e_dctx)
    ref["ctx"] = (at.out, at.out_b, s("ctx"))
    valid = torch.isfinite(at.lse).permute(0, 2, 1).reshape(B * L, nH)
    ref["lse"] = (lse_rows(at.lse, valid), lse_rows(at.lse_b, valid) + 1e-30, lse_rows(r["lse"], valid))
    dqkv, e_dqkv = stage("dqkv", at.dqkv, at.dqkv_b)
    v, _, bound, _, _ = G.gemm_ref(dqkv, wq, out_dtype=dt, residual=dy1)
    ref["dx_in"] = (v, bound + e_dqkv @ wq.abs() + e_dy1, s("dx_in"))
    # ---- weight and bias gradients: the rows below rows_dev
    got_w = torch.cat([r["query.weight"], r["key.weight"], r["value.weight"]], 0)
    got_b = torch.cat([r["query.bias"], r["key.bias"], r["value.bias"]], 0)
    for name, dY, e_dY, X, gw, gb in (("fc2", dz2, e_dz2, s("act"), r["fc2.weight"], r["fc2.bias"]),
                                      ("fc1", dh, e_dh, s("x1"), r["fc1.weight"], r["fc1.bias"]),
                                      ("o", dz1, e_dz1, s("ctx"), r["o.weight"], r["o.bias"]),
                                      ("qkv", dqkv, e_dqkv, s("x"), got_w, got_b)):
        Xd = X.double()
        v, _, bound, _, _ = G.gemm_ref(dY.t(), Xd, out_dtype=F32)
        ref[name + ".weight"] = (v, bound + e_dY.t() @ Xd.abs(), gw)
        v, bound = G.colsum_ref(dY.t())
        ref[name + ".bias"] = (v, bound + e_dY.sum(0), gb)
    assert set(ref) - set(STAGES) == set(FORWARD) | set(BACKWARD)
    return ref


def signal_to_bound(ref):
    """{name: median |value| / median bound}: how far the values of a tensor stand above their own bound (below ~1 the bound
    cannot see a fault of the size of the tensor itself)."""
    return {k: float(v.abs().median() / b.median()) for k, (v, b, _) in ref.items()}


def check_finite(r, names, label=""):
    for k in names:
        assert bool(torch.isfinite(r[k]).all()), f"{label} {k}: not finite (a row at or beyond the row count was read)".strip()

