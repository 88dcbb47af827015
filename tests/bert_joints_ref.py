"""float64 statement of the joints of the BERT side: the code BETWEEN the kernels in bert.py MVLBert._forward / _backward and in
model.py (the embedding ends, the pooler and its dgrad into the [CLS] rows, the labelled-row gather / scatter, _MlmLossFn on both
loss routes, _LinearCEFn, _LinearFn, _TransformLinearFn, _FeatureProjFn, the row arithmetic of the heads), with a per-element
bound for every tensor a joint hands over.

Built only from tests/gemm_ref.py, tests/ln_ref.py, tests/misc_ref.py and tests/head_ce_ref.py with their constants unchanged:
this module introduces no tolerance of its own.  Every joint is judged ONE STAGE DEEP from the operand that was really handed
over (cut); where a run does not hand an intermediate over, its float64 value is chained and its bound carried to first order
through |W| / the LayerNorm Jacobian (bert_layer_ref.ln_carry), exactly as tests/bert_layer_ref.py does it: `stage(name, ...)`
judges the stored tensor `name` if the run has it and starts the next stage from it with a zero input bound.

Host statements (plain index arithmetic, compared bit for bit):
  pack_plan_host     sample b keeps [CLS] img [SEP] and its caption up to the last position with a non-zero id or a label; the
                     samples follow each other without a gap; text_row[b T + t] is the packed row of caption position t, the
                     sample's [CLS] row for a dropped one
  label_plan_host    stable partition of the caption positions by (label >= 0) THROUGH text_row: gather_row, sel_labels, count
  embed_rows         misc_ref.embed_statement, the rows of the packed layout taken sample by sample
  cls_rows           b Lq dense, row_start[b] packed
  caption_text_row   'unilm' first = n_img + 2, 'normal' first = n_img + 1 ([SEP] for t = 0)

Joints with bounds (each -> {name: (float64 value, bound, what the run produced)}):
  pooler      pre = gemm_ref(cls, Wp, bp) is not stored: pooled = tanh(pre) carries pre's bound through the largest slope of
              tanh within it (at most 1) beside unary_ref("tanh")'s own.  dpre = unary_ref("tanh_bwd", pooled, dpooled) is not
              stored either; pooler.dense.weight / .bias are gemm_ref / colsum_ref of the float64 dpre with its bound carried
              through |cls|; the [CLS] rows of the dx handed to the last layer are dhidden + dpre Wp: dense, one accumulate
              (gemm_ref prev =, one output rounding); packed, the product is rounded, then added and rounded again
              (index_add_): gemm_ref's bound of the product plus U_OUT |sum|.  Every other row IS dhidden, bit for bit.
  mlm_head    x -> (pre, t1) gemm_ref gelu -> (t2, mean, rstd) ln_ref.fwd_ref -> logits gemm_ref into ld = ceil64(V) ->
              ce_fwd_ref (lse, nll sum), or head_ce_ref on the fused route -> loss = acc[0] / acc[1] (one f32 division).
              Backward: dl = ce_bwd_ref(stored logits, stored lse, the count the kernel was handed, dloss) -- the product
              overwrites the logits in place, so dl IS a stored tensor -- dt2 = dl Wd, decoder.weight / .bias, LayerNorm
              backward dt1 / weight / bias, dpre = gelu_bwd(pre, dt1), dx = dpre Wt, transform.dense.weight / .bias.
              Only the rows below the device-side count exist; dx at or beyond it is exactly zero (checked by the caller).
  linear_ce   _LinearCEFn (ITM): logits into ld = 4, ce_fwd_ref, dl, dx, weight / bias.
  linear      _LinearFn: dropout keep mask ln_ref.dropout_keep(seed, 4001, p, rows, H) forward (bit for bit) and replayed
              backward (bit for bit), logits, dxd, weight / bias.
  transform_linear   _TransformLinearFn: the transform of mlm_head followed by a small Linear.
  feature_proj       _FeatureProjFn: Linear and its three gradients.
  embed_backward     misc_ref.embed_bwd_ref from the dx layer 0 returned: dimg is a copy (bit for bit), word (float atomics:
                     embed_bwd_ref's bound for repeated ids) / position / token_type tables.

tests/test_bert_joints_cpu.py proves on the host that an f32 and a bf16 emulation of these joints sit inside every bound and
that a list of named wiring faults is rejected with the tensor named; tests/test_bert_joints_gpu.py runs the models against it."""
import torch

import gemm_ref as G
import head_ce_ref as HC
import ln_ref as R
import misc_ref as Mi
from gemm_ref import U32, check_bound  # noqa: F401
from swin_attn_half_ref import failures, worst_ratios  # noqa: F401  (shared judges, re-exported)

BF, F32 = torch.bfloat16, torch.float32
IGNORE = -100
DROP_TAG = 4001                                     # _LinearFn's dropout site
CLS_ID, SEP_ID, MASK_ID = 101, 102, 103


def ceil_to(n, k):
    return (n + k - 1) // k * k


# ------------------------------------------------------------------ host statements
def pack_plan_host(ids, labels, n_img):
    """ids [B, T], labels [B, T] or None -> (row_start [B], seq_len [B], total, text_row int64 [B T])."""
    B, T = ids.shape
    live = ids != 0
    if labels is not None:
        live = live | (labels.reshape(B, T) >= 0)
    cap = [(int(live[b].nonzero().max()) + 1) if bool(live[b].any()) else 0 for b in range(B)]
    seq_len = [c + n_img + 2 for c in cap]
    row_start = [sum(seq_len[:b]) for b in range(B)]
    text_row = torch.empty(B * T, dtype=torch.int64)
    for b in range(B):
        for t in range(T):
            text_row[b * T + t] = row_start[b] + n_img + 2 + t if t < cap[b] else row_start[b]
    return row_start, seq_len, sum(seq_len), text_row


def dense_text_row(B, T, n_img, first=None):
    """Row of caption position (b, t) in the dense [B Lq] layout, reading from position `first` (default n_img + 2)."""
    Lq = n_img + 2 + T
    first = n_img + 2 if first is None else first
    return ((torch.arange(B) * Lq + first)[:, None] + torch.arange(T)[None, :]).reshape(-1)


def caption_text_row(B, T, n_img, strategy):
    assert strategy in ("unilm", "normal")
    return dense_text_row(B, T, n_img, n_img + (2 if strategy == "unilm" else 1))


def label_plan_host(labels, text_row=None):
    """labels int64 [N] -> (gather_row int32 [N], sel_labels int64 [N], count): labelled positions first, both halves in order."""
    labels = labels.reshape(-1)
    on = labels >= 0
    order = torch.cat([on.nonzero().flatten(), (~on).nonzero().flatten()])
    rows = order if text_row is None else text_row[order]
    return rows.to(torch.int32), labels[order], int(on.sum())


def cls_rows(B, Lq, row_start=None):
    return torch.arange(B) * Lq if row_start is None else torch.as_tensor(row_start, dtype=torch.int64)


def embed_rows(ids, image, word, pos, typ, dtype, n_img, seq_len=None):
    """The rows layer 0 receives: [B Lq, H] dense, or the kept rows of every sample one after the other."""
    B, T = ids.shape
    x = Mi.embed_statement(ids.cpu(), image.cpu(), word.cpu(), pos.cpu(), typ.cpu(), CLS_ID, SEP_ID, dtype, B=B, n_img=n_img, T=T)
    if seq_len is None:
        return x.reshape(B * (n_img + 2 + T), -1)
    return torch.cat([x[b, :seq_len[b]] for b in range(B)], 0)


def to_dense(rows2d, B, Lq, seq_len=None):
    """[rows, H] -> ([B, Lq, H] with zeros where a position is not materialised, valid [B, Lq])."""
    H = rows2d.shape[1]
    if seq_len is None:
        return rows2d[:B * Lq].reshape(B, Lq, H), torch.ones(B, Lq, dtype=torch.bool)
    out = torch.zeros(B, Lq, H, dtype=rows2d.dtype, device=rows2d.device)
    valid = torch.zeros(B, Lq, dtype=torch.bool)
    r = 0
    for b, n in enumerate(seq_len):
        out[b, :n] = rows2d[r:r + n]
        valid[b, :n] = True
        r += n
    return out, valid


def make_batch(T, n_img=49, vocab=3000):
    """The batch of the joints tests, B = 4: caption lengths (T, 13 or 9, 0, T // 2 + 1); sample 1 has no label, sample 2 no
    caption; sample 0 is labelled at its last kept position; word 777 stands at four unlabelled positions (the float-atomic
    word-table row), and every labelled position holds [MASK].  -> (ids [B, T], labels [B, T], itm [B], lens)."""
    lens = (T, 13 if T > 13 else 9, 0, T // 2 + 1)
    g = torch.Generator().manual_seed(700 + T)
    ids = torch.randint(1000, vocab, (4, T), generator=g)
    labels = torch.full((4, T), IGNORE, dtype=torch.int64)
    for b, n in enumerate(lens):
        ids[b, n:] = 0
    ids[0, 1] = ids[0, 4] = ids[1, 2] = ids[3, 0] = 777
    marked = {0: [0, 3, 5, 6, 7, 10, 11, 14, 17, 20, 21, T - 1], 3: [1, 2, 5, 7, 8, 9, lens[3] - 1]}
    for b, ts in marked.items():
        for t in sorted(set(ts)):
            labels[b, t] = ids[b, t]
            ids[b, t] = MASK_ID
    labels[0, T - 1] = vocab - 1                                  # the last valid column, in the 64-column group that straddles V
    labels[3, 1] = vocab - 8
    return ids, labels, torch.tensor([1, 0, 1, 1]), lens


def check_label_requirements(ids, labels, lens, row_tile=64):
    """What the issue of these tests asks of the labels, from the labels themselves."""
    B, T = ids.shape
    per = (labels >= 0).sum(1).tolist()
    assert 0 in per, "one sample has no label"
    assert 0 in lens and not bool((ids[lens.index(0)] != 0).any()), "one sample has zero caption length"
    assert any(n > 0 and int(labels[b, n - 1]) >= 0 for b, n in enumerate(lens)), "one label at the last kept position of its sample"
    kept = torch.cat([ids[b, :n] for b, n in enumerate(lens)])
    assert int(torch.bincount(kept).max()) >= 3, "one id repeats at least three times"
    total = sum(per)
    assert total % 16 != 0 and 0 < total < row_tile, total
    for b, n in enumerate(lens):
        assert not bool((ids[b, n:] != 0).any()) and not bool((labels[b, n:] >= 0).any())
    return total


# ------------------------------------------------------------------ judging helpers
def _stage(ref, r, name, v, e, rows=None):
    """Judge the run's own stored `name`, if it hands it over, and start the next stage from it: the chain is cut there."""
    if name not in r:
        return v, e
    got = r[name] if rows is None else r[name][:rows]
    ref[name] = (v, e, got)
    return got.double(), torch.zeros_like(e)


def check_same(out, ref, what):
    """Equal values element by element (0.0 equals -0.0); names the first that differs."""
    assert out.shape == ref.shape, (what, tuple(out.shape), tuple(ref.shape))
    a, b = out.reshape(out.shape[0], -1), ref.to(out.device).reshape(out.shape[0], -1)
    same = (a == b) | (torch.isnan(a) & torch.isnan(b))
    if not bool(same.all()):
        bad = (~same).nonzero()[0]
        i, j = int(bad[0]), int(bad[1])
        raise AssertionError(f"{what}: {int((~same).sum())} of {a.numel()} elements differ; first at row {i}, column {j}: "
                             f"out {float(a[i, j])!r}, expected {float(b[i, j])!r}")


def loss_of(nll, nll_b, count, got):
    """loss = acc[0] / acc[1]: one f32 division.  -> (value, bound, got) as 1-element tensors."""
    c = max(float(count), 0.0)
    v = torch.as_tensor(float(nll) / c if c else float("nan"), dtype=torch.float64).reshape(1)
    b = torch.as_tensor(float(nll_b) / c if c else 0.0, dtype=torch.float64).reshape(1) + U32 * v.abs() + 1e-30
    return v.to(got.device), b.to(got.device), got.reshape(1)


# ------------------------------------------------------------------ pooler
def pooler(r, dt):
    """r: cls [B, H] (the rows handed to the pooler), wp [H, H], bp, pooled [B, H]; optionally dpooled [B, H], pooler.weight,
    pooler.bias (f32 gradients), dh_cls (the [CLS] rows of dhidden), dx_cls (those of the dx handed to the last layer), and
    packed (the accumulate goes through index_add_: two roundings)."""
    ref = {}
    a, b = G.logical(r["cls"], r["wp"])
    pre, _, pre_b, _, _ = G.gemm_ref(a, b, out_dtype=dt, bias=r["bp"])
    v, b_t = Mi.unary_ref("tanh", pre, None, dt)
    slope = 1.0 - torch.tanh((pre.abs() - pre_b).clamp(min=0.0)) ** 2          # the largest tanh' within pre +- pre_b
    ref["pooled"] = (v, b_t + slope * pre_b, r["pooled"])
    if r.get("dpooled") is None:
        return ref
    dpre, e_dpre = Mi.unary_ref("tanh_bwd", r["pooled"], r["dpooled"], dt)
    dpre, e_dpre = _stage(ref, r, "dpre", dpre, e_dpre)
    cls = r["cls"].double()
    v, _, bound, _, _ = G.gemm_ref(dpre.t(), cls, out_dtype=F32)
    ref["pooler.weight"] = (v, bound + e_dpre.t() @ cls.abs(), r["pooler.weight"])
    v, bound = G.colsum_ref(dpre.t())
    ref["pooler.bias"] = (v, bound + e_dpre.sum(0), r["pooler.bias"])
    wp = r["wp"].double()
    if r.get("packed"):
        v, _, bound, _, _ = G.gemm_ref(dpre, wp, out_dtype=dt)
        v = v + r["dh_cls"].double()
        bound = bound + R.u_out(dt) * v.abs()
    else:
        v, _, bound, _, _ = G.gemm_ref(dpre, wp, out_dtype=dt, prev=r["dh_cls"])
    ref["dx_cls"] = (v, bound + e_dpre @ wp.abs(), r["dx_cls"])
    return ref


# ------------------------------------------------------------------ transform (dense + GELU + LayerNorm), shared
def _transform_fwd(ref, r, n, dt, eps):
    a, b = G.logical(r["x"][:n], r["wt"])
    v, pre, bound, _, pre_b = G.gemm_ref(a, b, out_dtype=dt, bias=r["bt"], gelu=True)
    ref["pre"], ref["t1"] = (pre, pre_b + 1e-30, r["pre"][:n]), (v, bound, r["t1"][:n])
    f = R.fwd_ref(r["t1"][:n], r["gamma"], r["beta"], dt, eps=eps)
    ref["t2"], ref["mean"], ref["rstd"] = (f["y"], f["y_b"], r["t2"][:n]), (f["mean"], f["mean_b"], r["mean"][:n]), \
        (f["rstd"], f["rstd_b"], r["rstd"][:n])


def _transform_bwd(ref, r, n, dt, dt2, e_dt2):
    """From dt2 (value, bound) [n, H]: dt1, LayerNorm gradients, dpre, dx, transform.dense gradients."""
    t1 = r["t1"][:n]
    bw = R.bwd_ref(t1, dt2, r["mean"][:n], r["rstd"][:n], r["gamma"], dt)
    gam = r["gamma"].double().abs()[None, :]
    rs = r["rstd"][:n].double()[:, None]
    xh = ((t1.double() - r["mean"][:n].double()[:, None]) * rs).abs()
    ge = gam * e_dt2
    carry = rs * (ge + ge.mean(1, keepdim=True) + xh * (ge * xh).mean(1, keepdim=True))          # bert_layer_ref.ln_carry
    ref["ln.weight"] = (bw["dg"], bw["dg_b"] + (e_dt2 * xh).sum(0), r["ln.weight"])
    ref["ln.bias"] = (bw["db"], bw["db_b"] + e_dt2.sum(0), r["ln.bias"])
    dt1, e_dt1 = _stage(ref, r, "dt1", bw["dx"], bw["dx_b"] + carry, n)
    pre = r["pre"][:n]
    v, bound = Mi.unary_ref("gelu_bwd", pre, dt1, dt)
    dpre, e_dpre = _stage(ref, r, "dpre", v, bound + e_dt1 * G.gelu_grad64(pre.double()).abs(), n)
    wt = r["wt"].double()
    v, _, bound, _, _ = G.gemm_ref(dpre, wt, out_dtype=dt)
    ref["dx"] = (v, bound + e_dpre @ wt.abs(), r["dx"][:n])
    xd = r["x"][:n].double()
    v, _, bound, _, _ = G.gemm_ref(dpre.t(), xd, out_dtype=F32)
    ref["transform.weight"] = (v, bound + e_dpre.t() @ xd.abs(), r["transform.weight"])
    v, bound = G.colsum_ref(dpre.t())
    ref["transform.bias"] = (v, bound + e_dpre.sum(0), r["transform.bias"])


# ------------------------------------------------------------------ MLM head + cross entropy
def mlm_head(r, dt, *, V, n, fused, eps, backward=True):
    """r: x [N, H], labels int64 [N] (as the head received them), wt, bt, gamma, beta, wd [V, H], bd [V]; the saved pre, t1, t2,
    mean, rstd; logits [N, ld] (the stored forward logits), lse [N], acc f32 [2] (the pair the backward is handed: acc[1] is the
    count the loss is divided by), nll (acc[0] as the loss kernel wrote it), loss; backward: dloss (a number), dl [N, ld] (the
    logits buffer after the in-place CE backward), dx [N, H], the six parameter gradients decoder.weight / decoder.bias /
    ln.weight / ln.bias / transform.weight / transform.bias; optionally the stored stages dt2, dt1, dpre (a replay).
    n: the rows that exist (the device-side count, or N)."""
    ref = {}
    _transform_fwd(ref, r, n, dt, eps)
    lab = r["labels"][:n]
    on = lab >= 0
    count = int(on.sum())
    logits = r["logits"]
    if fused:
        h = HC.head_ce_ref(r["t2"], r["wd"], r["bd"], r["labels"], rows=n)
        ref["logits"] = (h["v"], h["bound_v"], logits[:n, :V])
        ref["lse"] = (h["lse"][on], h["bound_lse"][on], r["lse"][:n][on])
        nll, nll_b = h["nll_sum"], h["bound_sum"]
        assert h["count"] == count
    else:
        a, b = G.logical(r["t2"][:n], r["wd"])
        v, _, bound, _, _ = G.gemm_ref(a, b, out_dtype=dt, bias=r["bd"])
        ref["logits"] = (v, bound, logits[:n, :V])
        c = Mi.ce_fwd_ref(logits, V, r["labels"], n_valid=n)
        ref["lse"] = (c["lse"][on], c["lse_b"][on], r["lse"][:n][on])
        nll, nll_b = float(c["loss"]), float(c["loss_b"])
        assert c["count"] == count
    one = lambda x: torch.as_tensor(x, dtype=torch.float64, device=logits.device).reshape(1)          # noqa: E731
    ref["nll"] = (one(nll), one(nll_b), r["nll"].reshape(1))
    ref["loss"] = loss_of(float(r["nll"]), 0.0, float(r["acc"][1]), r["loss"])          # cut: from the stored sum and count
    if not backward:
        return ref
    dl, e_dl = Mi.ce_bwd_ref(logits, V, r["labels"], r["lse"], float(r["acc"][1]), 1.0, r["dloss"], dt, n_valid=n)
    if "dl" in r:
        ref["dl"] = (dl, e_dl, r["dl"][:n, :V])
        dl, e_dl = r["dl"][:n, :V].double(), torch.zeros_like(e_dl)
    wd = r["wd"].double()
    v, _, bound, _, _ = G.gemm_ref(dl, wd, out_dtype=dt)
    dt2, e_dt2 = _stage(ref, r, "dt2", v, bound + e_dl @ wd.abs(), n)
    t2 = r["t2"][:n].double()
    v, _, bound, _, _ = G.gemm_ref(dl.t(), t2, out_dtype=F32)
    ref["decoder.weight"] = (v, bound + e_dl.t() @ t2.abs(), r["decoder.weight"])
    v, bound = G.colsum_ref(dl.t())
    ref["decoder.bias"] = (v, bound + e_dl.sum(0), r["decoder.bias"])
    _transform_bwd(ref, r, n, dt, dt2, e_dt2)
    return ref


# ------------------------------------------------------------------ small classifier + cross entropy (ITM)
def linear_ce(r, dt, backward=True):
    """r: x [B, H], w [V, H], b [V], labels [B], logits [B, ld] (stored forward logits), lse, acc, loss; backward: dloss, dl
    (the buffer after the in-place CE backward), dx, weight, bias."""
    ref = {}
    V = r["w"].shape[0]
    a, b = G.logical(r["x"], r["w"])
    v, _, bound, _, _ = G.gemm_ref(a, b, out_dtype=dt, bias=r["b"])
    ref["logits"] = (v, bound, r["logits"][:, :V])
    c = Mi.ce_fwd_ref(r["logits"], V, r["labels"])
    on = c["on"]
    ref["lse"] = (c["lse"][on], c["lse_b"][on], r["lse"][on])
    ref["loss"] = loss_of(float(c["loss"]), float(c["loss_b"]), c["count"], r["loss"])
    assert float(r["acc"][1]) == c["count"]
    if not backward:
        return ref
    dl, dl_b = Mi.ce_bwd_ref(r["logits"], V, r["labels"], r["lse"], float(r["acc"][1]), 1.0, r["dloss"], dt)
    ref["dl"] = (dl, dl_b, r["dl"][:, :V])
    dl = r["dl"][:, :V].double()
    v, _, bound, _, _ = G.gemm_ref(dl, r["w"].double(), out_dtype=dt)
    ref["dx"] = (v, bound, r["dx"])
    v, _, bound, _, _ = G.gemm_ref(dl.t(), r["x"].double(), out_dtype=F32)
    ref["weight"] = (v, bound, r["weight"])
    v, bound = G.colsum_ref(dl.t())
    ref["bias"] = (v, bound, r["bias"])
    return ref


# ------------------------------------------------------------------ (dropout ->) Linear with f32 logits (VQA)
def linear(r, dt, *, p, seed):
    """r: x [B, H], xd (the saved dropped-out input), w [V, H], b, logits f32 [B, V] (what the Function returned); backward:
    dlogits f32 [B, V], dx, weight, bias.  Bit-for-bit checks are made here; -> the bounded tensors."""
    ref = {}
    B, Hd = r["x"].shape
    keep = None
    if p > 0:
        keep = R.dropout_keep(seed, DROP_TAG, p, B, Hd, device=r["x"].device)
        v = r["x"].double() * keep.double() / (1.0 - p)
        ref["xd"] = (v, (2 * U32 + R.u_out(dt)) * v.abs() + 1e-30, r["xd"])
        Mi.check_zero(r["xd"][keep == 0], "the dropped elements of xd")
    else:
        Mi.check_equal(r["xd"], r["x"], "p = 0: xd is x")
    a, b = G.logical(r["xd"], r["w"])
    v, _, bound, _, _ = G.gemm_ref(a, b, out_dtype=dt, bias=r["b"])
    ref["logits"] = (v, bound, r["logits"])
    if "dlogits" not in r:
        return ref
    dl = r["dlogits"].to(dt).double()                       # the cast of the f32 gradient to the compute dtype: IEEE, exact statement
    w = r["w"].double()
    dxd, _, dxd_b, _, _ = G.gemm_ref(dl, w, out_dtype=dt)
    if p > 0:
        f = keep.double() / (1.0 - p)
        v = dxd * f
        ref["dx"] = (v, dxd_b * f + (2 * U32 + R.u_out(dt)) * v.abs() + 1e-30, r["dx"])
        Mi.check_zero(r["dx"][keep == 0], "dx where the forward dropped: the backward replays the forward's mask")
    else:
        ref["dx"] = (dxd, dxd_b, r["dx"])
    v, _, bound, _, _ = G.gemm_ref(dl.t(), r["xd"].double(), out_dtype=F32)
    ref["weight"] = (v, bound, r["weight"])
    v, bound = G.colsum_ref(dl.t())
    ref["bias"] = (v, bound, r["bias"])
    return ref


# ------------------------------------------------------------------ transform + small Linear (retrieval)
def transform_linear(r, dt, *, eps):
    """r: x [B, H], wt, bt, gamma, beta, w [V, H], b, the saved pre, t1, t2, mean, rstd, logits f32 [B, V]; backward: dlogits,
    dx, weight, bias, ln.weight, ln.bias, transform.weight, transform.bias; optionally the stored stages dt2, dt1, dpre."""
    ref = {}
    n = r["x"].shape[0]
    _transform_fwd(ref, r, n, dt, eps)
    a, b = G.logical(r["t2"], r["w"])
    v, _, bound, _, _ = G.gemm_ref(a, b, out_dtype=dt, bias=r["b"])
    ref["logits"] = (v, bound, r["logits"])
    if "dlogits" not in r:
        return ref
    dl = r["dlogits"].to(dt).double()
    w = r["w"].double()
    v, _, bound, _, _ = G.gemm_ref(dl, w, out_dtype=dt)
    dt2, e_dt2 = _stage(ref, r, "dt2", v, bound, n)
    v, _, bound, _, _ = G.gemm_ref(dl.t(), r["t2"].double(), out_dtype=F32)
    ref["weight"] = (v, bound, r["weight"])
    v, bound = G.colsum_ref(dl.t())
    ref["bias"] = (v, bound, r["bias"])
    _transform_bwd(ref, r, n, dt, dt2, e_dt2)
    return ref


# ------------------------------------------------------------------ feature projection
def feature_proj(r, dt):
    """r: x [rows, C], w [H, C], b, y [rows, H]; backward: dy, dx, weight, bias."""
    ref = {}
    a, b = G.logical(r["x"], r["w"])
    v, _, bound, _, _ = G.gemm_ref(a, b, out_dtype=dt, bias=r["b"])
    ref["y"] = (v, bound, r["y"])
    if "dy" not in r:
        return ref
    dy = r["dy"].double()
    v, _, bound, _, _ = G.gemm_ref(dy, r["w"].double(), out_dtype=dt)
    ref["dx"] = (v, bound, r["dx"])
    v, _, bound, _, _ = G.gemm_ref(dy.t(), r["x"].double(), out_dtype=F32)
    ref["weight"] = (v, bound, r["weight"])
    v, bound = G.colsum_ref(dy.t())
    ref["bias"] = (v, bound, r["bias"])
    return ref


def pair_flatten(v):
    """Conv_layer on a 5-D pair batch [B, n, ...]: the tower sees the images in (n, B) order."""
    B, n = v.shape[:2]
    return v.transpose(0, 1).reshape(n * B, *v.shape[2:])


def pair_unflatten(f, B, n):
    """[n B, L, H] in (n, B) order -> [B, n L, H]: the views of one sample side by side."""
    return f.view(n, B, f.shape[1], f.shape[2]).transpose(0, 1).reshape(B, n * f.shape[1], f.shape[2])


# ------------------------------------------------------------------ embedding backward
def embed_backward(r, ids, n_img, seq_len=None):
    """r: dx0 [rows, H] (what layer 0 returned), dimg [B, n_img, H], word / position / token_type (f32 table gradients).
    -> (the bounded tables, {name: message} of the bit-for-bit statements that fail: dimg is a copy, the rows no position
    reaches are exactly 0)."""
    B, T = ids.shape
    Lq = n_img + 2 + T
    dout, valid = to_dense(r["dx0"].cpu(), B, Lq, seq_len)
    wid = Mi.embed_word_ids(ids.cpu(), B, n_img, T, CLS_ID, SEP_ID)
    e = Mi.embed_bwd_ref(dout, wid, valid, torch.zeros(r["word"].shape, dtype=torch.float32), n_img=n_img,
                         pos_rows=r["position"].shape[0], type_rows=r["token_type"].shape[0])
    exact = {}
    for name, fn in (("dimg", lambda: Mi.check_equal(r["dimg"].cpu().reshape(B, n_img, -1), dout[:, 1:1 + n_img].contiguous(),
                                                     "dimg is the image rows of dx0")),
                     ("word rows unused", lambda: Mi.check_zero(r["word"].cpu()[e["hits"] == 0], "word rows no kept position holds")),
                     ("position rows unused", lambda: Mi.check_zero(r["position"].cpu()[~e["pos_used"]], "position rows beyond the sequence")),
                     ("token_type rows unused", lambda: Mi.check_zero(r["token_type"].cpu()[~e["type_used"]], "token_type rows nobody uses"))):
        try:
            fn()
        except AssertionError as err:
            exact[name] = str(err)
    return {"word": (e["dword"], e["dword_b"], r["word"].cpu()), "position": (e["dpos"], e["dpos_b"], r["position"].cpu()),
            "token_type": (e["dtype"], e["dtype_b"], r["token_type"].cpu())}, exact


def signal_to_bound(ref):
    return {k: float(v.abs().median() / b.median()) for k, (v, b, _) in ref.items() if v.numel()}


# ------------------------------------------------------------------ one pretraining step, joint by joint
def head_rows_host(rec):
    """The row arithmetic of MVLBertForPretraining.forward / MVLBertForImageCaption._head_rows on the host.  rec: ids, labels,
    n_img, layout ("auto": the plan from the ids and labels; "packed": seq_len / row_start from the caller's text_lengths, rows
    of positions beyond a length are row_start + n_img + 2 + t all the same, clamped into the allocation; "dense"), lab_first,
    cap (mlm_max_labels_per_sample or None), first.  -> (src int64: the row of hidden every row of x reads, the labels that
    travel with it, the rows that exist, gather_row int32 or None)."""
    ids, labels, n_img = rec["ids"], rec["labels"], rec["n_img"]
    B, T = ids.shape
    flat = labels.reshape(-1)
    if rec["layout"] == "auto":
        text_row = pack_plan_host(ids, labels, n_img)[3]
    elif rec["layout"] == "packed":
        rs = torch.as_tensor(rec["row_start"], dtype=torch.int64)
        text_row = ((rs + n_img + 2)[:, None] + torch.arange(T)[None, :]).reshape(-1).clamp(max=sum(rec["seq_len"]) - 1)
    else:
        text_row = dense_text_row(B, T, n_img, rec.get("first"))
    if rec["lab_first"]:
        grow, sel, n = label_plan_host(flat, text_row)
        return grow.long(), sel, n, grow
    cap = rec.get("cap")
    if cap is not None and cap * B < B * T:
        order = torch.argsort((flat < 0).to(torch.int8), stable=True)[:cap * B]
        return text_row[order], flat[order], cap * B, None
    return text_row, flat, flat.numel(), None


def judge_pretrain(rec, label=""):
    """rec: the normalised record of one MVLBertForPretraining step (tests/test_bert_joints_cpu.py `emulate` and
    tests/test_bert_joints_gpu.py `record_of` build it; the keys are read below).  -> (failures {name: message}, worst ratios
    {name: ratio}): every bounded tensor under "<joint> <tensor>", every bit-for-bit statement under its own name."""
    bad, ratios = {}, {}
    dt, B, T, n_img, V = rec["dt"], rec["B"], rec["T"], rec["n_img"], rec["V"]
    Lq = n_img + 2 + T
    dev = rec["hidden"].device
    seq_len, row_start = rec.get("seq_len"), rec.get("row_start")
    rows = B * Lq if seq_len is None else sum(seq_len)

    def exact(name, fn):
        try:
            fn()
        except AssertionError as e:
            bad[name] = f"{label} {name}: {e}".strip()

    def bounded(joint, ref):
        for k, v in worst_ratios(ref).items():
            ratios[f"{joint} {k}"] = v
        for k, m in failures(ref, f"{label} {joint}".strip()).items():
            bad[f"{joint} {k}"] = m

    hidden = rec["hidden"]
    # ---- embeddings to layer 0
    if "x0" in rec:
        want = embed_rows(rec["ids"], rec["image"], rec["word"], rec["pos"], rec["typ"], dt, n_img, seq_len)
        exact("x0", lambda: Mi.check_equal(rec["x0"][:rows].cpu(), want, "the rows layer 0 receives are the embedding sum"))
    # ---- encoder to pooler
    crow = cls_rows(B, Lq, row_start).to(dev)
    if "cls" in rec:
        exact("cls", lambda: Mi.check_equal(rec["cls"], hidden[crow], "cls is the first row of every sample"))
        dpooled = rec.get("dpooled")
        pr = dict(cls=rec["cls"], wp=rec["wp"], bp=rec["bp"], pooled=rec["pooled"], dpooled=dpooled, packed=seq_len is not None)
        if dpooled is not None:
            pr.update({"pooler.weight": rec["g_wp"], "pooler.bias": rec["g_bp"], "dh_cls": rec["dhidden"][crow],
                       "dx_cls": rec["dx_last"][crow]})
        bounded("pooler", pooler(pr, dt))
        if "dx_last" in rec:
            other = torch.ones(rows, dtype=torch.bool, device=dev)
            if dpooled is not None:
                other[crow] = False
            exact("dx_last", lambda: Mi.check_equal(rec["dx_last"][:rows][other], rec["dhidden"][:rows][other],
                                                    "the dx handed to the last layer is dhidden off the [CLS] rows"))
    # ---- MLM head
    m = rec.get("mlm")
    if m is not None:
        src, sel, n, grow = head_rows_host(rec)
        flat = rec["labels"].reshape(-1)
        if rec["lab_first"]:
            exact("gather_row", lambda: Mi.check_equal(m["gather_row"].cpu(), grow, "gather_row: labelled positions first, through text_row"))
            exact("sel_labels", lambda: Mi.check_equal(m["labels"].cpu(), sel, "sel_labels travel with gather_row"))
            exact("rd", lambda: Mi.check_equal(torch.as_tensor(m["rd"]).reshape(1).cpu().long(), torch.tensor([n]), "the device-side count"))
        else:
            exact("labels", lambda: Mi.check_equal(m["labels"].cpu(), sel, "the labels of the all-rows head"))
        src = src.to(dev)
        exact("mlm x", lambda: Mi.check_equal(m["x"], hidden[src], "x is hidden[gather_row]"))
        count = int((sel >= 0).sum())                           # (a capacity below the real count drops labels: the loss is NaN then)
        factor = rec.get("sync") or 1.0
        exact("count", lambda: Mi.check_equal(m["acc"][1:2].cpu().double(), torch.tensor([factor * count], dtype=torch.float64),
                                              "the count the loss is divided by"))
        bounded("mlm", mlm_head(dict(m, dloss=rec["dloss"]), dt, V=V, n=n, fused=rec["fused"], eps=rec["eps"], backward="dx" in m))
        if "dx" in m:
            exact("mlm dx beyond rd", lambda: Mi.check_zero(m["dx"][n:], "dx rows at or beyond the device-side count"))
            exact("mlm dloss", lambda: Mi.check_equal(torch.as_tensor(m["dloss_seen"]).reshape(1).cpu().float(),
                                                      torch.tensor([rec["dloss"]]), "dloss reaches the MLM loss"))
            want = torch.zeros_like(rec["dhidden"])
            want.index_add_(0, src[:n], m["dx"][:n])
            live = torch.zeros(want.shape[0], dtype=torch.bool, device=dev)
            live[src[:n][(sel[:n] >= 0).to(dev)]] = True
            exact("dhidden", lambda: check_same(rec["dhidden"][:rows], want[:rows], "dhidden[gather_row[i]] = dx[i]"))
            exact("dhidden rows nobody gathered", lambda: Mi.check_zero(rec["dhidden"][~live], "dhidden off the labelled rows"))
    # ---- ITM head
    it = rec.get("itm")
    if it is not None:
        exact("itm x", lambda: Mi.check_equal(it["x"], rec["pooled"], "the ITM head reads pooled"))
        bounded("itm", linear_ce(dict(it, dloss=rec["dloss"]), dt, backward="dx" in it))
        if "dx" in it:
            exact("dpooled", lambda: Mi.check_equal(rec["dpooled"], it["dx"], "dpooled is the ITM head's dx"))
            exact("itm dloss", lambda: Mi.check_equal(torch.as_tensor(it["dloss_seen"]).reshape(1).cpu().float(),
                                                      torch.tensor([rec["dloss"]]), "dloss reaches the ITM loss"))
    if m is not None and it is not None:
        want = (m["loss"].float() + it["loss"].float()).reshape(1)
        if rec.get("nan"):                                      # over capacity / a label beyond the stated length: NaN, as stated
            want = torch.full_like(want, float("nan"))
        exact("total", lambda: Mi.check_equal(rec["total"].reshape(1).float(), want, "the total is mlm + itm"))
    # ---- embedding backward
    if "dx0" in rec:
        er, ex = embed_backward(dict(dx0=rec["dx0"][:rows], dimg=rec["dimg"], word=rec["g_word"], position=rec["g_pos"],
                                     token_type=rec["g_typ"]), rec["ids"], n_img, seq_len)
        bad.update({f"embed {k}": f"{label} embed {k}: {v}".strip() for k, v in ex.items()})
        bounded("embed", er)
    return bad, ratios
