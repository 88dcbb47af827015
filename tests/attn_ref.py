"""float64 reference of an MvltAttn call (forward and backward) and a per-element error bound for it.

The reference is taken from the SAME operands the kernel reads (bf16 and f32 values of qkv / dout are exact in float64);
the masks come from the oracle's own statements (relative_position_index, shift_attn_mask, bidir_bool_mask with its
image_mask, seq2seq_bool_mask, additive_mask), never from the kernel's index logic, and the dropout keep mask from a host
port of the counter hash (``keep_ref``).  The backward is the exact float64 gradient of that forward.

The bound follows the kernel's own arithmetic, per (sequence, head, query, key):
  logits   s = scale (q.k) + b in f32:        ds = C_ACC 2^-24 sqrt(hd) scale |q|.|k| + 2 2^-24 |s|
  softmax  __expf / __logf of s - max:        de = C_EXP 2^-24 + 2 2^-24 |s - max|   (the argument's own rounding)
           P = e / sum:                       dP/P = ds + sum_j P_j ds_j + de + sum_j P_j de_j + C_ACC 2^-24 sqrt(L) + 3 2^-24
  PV       P (x keep / (1-p)) rounded to the compute dtype, f32 sum over L, output rounding
  lse      sum_j P_j ds_j + sum_j P_j de_j + C_ACC 2^-24 sqrt(L) + C_LOG 2^-24 (|lse| + 1)
  backward P recomputed from the saved lse (its bound enters here, and only here), dP = dO.V^T in f32,
           delta = rowsum(P o dP) or rowsum(dO o O) from the rounded forward output (both bounded: max of the two),
           dS = P (dP - delta) rounded to the compute dtype, f32 sums over L (dQ, dK, dV) and, for the bias table,
           over every (window, q, k) that shares a relative index; output rounding (dqkv in the compute dtype, the
           bias-table gradient in f32).
U_OUT / U_OP are the unit roundoffs, 2^-8 for bf16 (8 significant bits) and 2^-24 for f32.  The reported bound is
SAFETY = 2 times this worst-case first-order estimate, so a correct kernel sits at <= 1/2 of it.
tests/test_attn_bound_cpu.py proves on the host that the bound accepts the kernels' roundings at a ratio <= 0.5 and
rejects a single wrong (sequence, head)."""
import math

import torch

from gemm_ref import C_ACC, U32, U_BF16, check_bound  # noqa: F401  (check_bound re-exported for the attention tests)

C_EXP = 4.0                 # __expf: ex2 approximation (<= 2 ulp) plus the rounding of x * log2(e)
C_LOG = 4.0                 # __logf: log2 approximation (<= 2 ulp) times ln 2, plus the add of the row max
MASK_OUT = -1.0e30          # keys a packed sequence does not have: exp() is exactly 0 in float64, as NEG_BIG is in f32
SAFETY = 2.0                # reported bound / first-order estimate: second-order terms and a margin a correct kernel never uses
LOGIT_STD = 2.5             # attn_operands: std of scale * q.k, so P is peaked and one wrong key or row stands out


# ------------------------------------------------------------------ dropout hash (csrc/common.h mix32 / rng_u32 / rng_keep)
M32 = 0xFFFFFFFF


def _mul32(a, c):
    """(a * c) mod 2^32 for int64 tensors holding uint32 values: split c in 16-bit halves so nothing overflows."""
    lo, hi = c & 0xFFFF, c >> 16
    return ((a * lo) + (((a * hi) & 0xFFFF) << 16)) & M32


def mix32(h):
    h = h ^ (h >> 16)
    h = _mul32(h, 0x7FEB352D)
    h = h ^ (h >> 15)
    h = _mul32(h, 0x846CA68B)
    return h ^ (h >> 16)


def _mix32_int(h):
    h ^= h >> 16
    h = (h * 0x7FEB352D) & M32
    h ^= h >> 15
    h = (h * 0x846CA68B) & M32
    return h ^ (h >> 16)


def rng_u32(seed, tag, idx):
    """rng_u32(seed, tag, idx) of csrc/common.h; idx: int64 tensor of uint32 values -> int64 tensor of uint32 values."""
    seed, tag = int(seed) & ((1 << 64) - 1), int(tag) & M32
    key = _mix32_int((seed & M32) ^ ((tag * 0x9E3779B9) & M32)) ^ (seed >> 32)
    return mix32((_mul32(idx & M32, 0x9E3779B1) + key) & M32)


def keep_ref(seed, tag, idx, p):
    """rng_keep: kept iff rng_u32 >= thresh, thresh = (uint32)(p * 2^32) as MvltAttn / mvlt_dropout_mask form it."""
    thresh = int(float(torch.tensor(p, dtype=torch.float32)) * 4294967296.0)
    return rng_u32(seed, tag, idx) >= thresh


def attn_keep(seed, tag, p, nseq, nH, L, device="cpu"):
    """The attention dropout mask [nseq, nH, L, L] (float64 0/1) at the documented index ((seq nH + h) L + q) L + k."""
    idx = torch.arange(nseq * nH * L * L, dtype=torch.int64, device=device)
    return keep_ref(seed, tag, idx, p).double().view(nseq, nH, L, L)


# ------------------------------------------------------------------ masks, from the oracle's statements
def swin_bias(table, nW, res, shift, nseq):
    """Additive logit term [nseq, nH, 49, 49]: relative-position bias + the shift mask of window seq % nW."""
    from oracle import mvlt_oracle as O
    idx = O.relative_position_index(7).to(table.device)
    nH = table.shape[1]
    b = table.double()[idx.view(-1)].view(49, 49, nH).permute(2, 0, 1)[None].expand(nseq, nH, 49, 49)
    if shift:
        m = O.shift_attn_mask(res, res, 7, shift).double().to(table.device)
        b = b + m[torch.arange(nseq, device=table.device) % nW][:, None]
    return b


def bert_bias(mode_s2s, nseq, L, n_img, ids=None, image_mask=None):
    """Additive logit term [nseq, 1, L, L] (-10000 masks) of the MVLBert modes."""
    from oracle import mvlt_oracle as O
    if mode_s2s:
        return O.additive_mask(O.seq2seq_bool_mask(L, n_img + 1)[None].expand(nseq, L, L)).double()
    m = O.additive_mask(O.bidir_bool_mask(ids.cpu(), nseq, n_img, None if image_mask is None else image_mask.cpu()))
    return m.double().expand(nseq, 1, L, L)


# ------------------------------------------------------------------ operands
def attn_operands(nseq, L, nH, hd, dtype, seed, rows=None, row_index=None, device="cpu"):
    """qkv [rows, 3 nH hd] and dout [rows, nH hd] in `dtype` from one seeded generator; q and k are drawn so that
    scale * q.k has std LOGIT_STD (scale = hd^-0.5).  row_index (packed layouts): the activation row of each dense
    (seq, token) row that exists; other rows of the returned tensors are NaN."""
    g = torch.Generator().manual_seed(seed)
    C = nH * hd
    n = nseq * L
    sig = math.sqrt(LOGIT_STD)                       # (hd^-0.5) (q.k) has std sig^2
    qkv = torch.randn(n, 3 * C, generator=g)
    qkv[:, :2 * C] *= sig
    dout = torch.randn(n, C, generator=g)
    qkv, dout = qkv.to(dtype), dout.to(dtype)
    if row_index is not None:
        R = rows
        q2 = torch.full((R, 3 * C), float("nan"), dtype=dtype)
        d2 = torch.full((R, C), float("nan"), dtype=dtype)
        dense = row_index >= 0
        q2[row_index[dense]] = qkv[dense]
        d2[row_index[dense]] = dout[dense]
        qkv, dout = q2, d2
    return qkv.to(device), dout.to(device)


def pack_layout(lens, L, gap=3):
    """row_start / seq_len (int32) of sequences of `lens` rows with `gap` unused rows before each, the total row count,
    and row_index: the activation row of dense row (s, t), or -1."""
    starts, r = [], 0
    for ln in lens:
        r += gap
        starts.append(r)
        r += ln
    row_index = torch.full((len(lens) * L,), -1, dtype=torch.int64)
    for s, (st, ln) in enumerate(zip(starts, lens)):
        row_index[s * L: s * L + ln] = st + torch.arange(ln)
    return (torch.tensor(starts, dtype=torch.int32), torch.tensor(lens, dtype=torch.int32), r + gap, row_index)


# ------------------------------------------------------------------ reference + bound
def _heads(x, nseq, L, nH, hd, row_index):
    """[rows, nH hd] activation rows -> float64 [nseq, nH, L, hd] (rows a packed sequence does not have: 0)."""
    x = x.double()
    if row_index is not None:
        dense = torch.zeros(nseq * L, x.shape[1], dtype=torch.float64, device=x.device)
        ok = row_index >= 0
        dense[ok] = x[row_index[ok].to(x.device)]
        x = dense
    return x.view(nseq, L, nH, hd).permute(0, 2, 1, 3)


def _rows(t, row_index):
    """[nseq, nH, L, hd] -> [nseq L, nH hd] (dense) or the packed activation rows it has."""
    nseq, nH, L, hd = t.shape
    t = t.permute(0, 2, 1, 3).reshape(nseq * L, nH * hd)
    return t if row_index is None else t[(row_index >= 0).to(t.device)]


class AttnRef:
    """float64 forward / backward of one MvltAttn call and their per-element bounds.

    qkv, dout: the kernel's operands; bias: additive logit term broadcastable to [nseq, nH, L, L] (swin_bias / bert_bias);
    keep: [nseq, nH, L, L] 0/1 or None, p its dropout probability; dtype: the compute dtype; pack: (row_index, seq_len)
    for packed rows; dout_err: [rows, nH hd] bound on the error of a dO the kernel forms itself (Swin dout_weight).  Attributes (activation-row layout as the kernel writes it, only rows a sequence has):
      out, out_b  [rows, nH hd]       lse, lse_b  [nseq, nH, L] (q >= seq_len: NaN, not checked)
      dqkv, dqkv_b [rows, 3 nH hd]    dS, dS_b   [nseq, nH, L, L] (for the bias-table gradient)"""

    def __init__(self, qkv, dout, *, nseq, L, nH, hd, scale, bias, dtype, keep=None, p=0.0, pack=None, dout_err=None,
                 device=None):
        dev = device or qkv.device
        qkv, dout = qkv.to(dev), (None if dout is None else dout.to(dev))
        row_index, seq_len = (None, None) if pack is None else (pack[0].to(dev), pack[1].to(dev))
        self.row_index = row_index
        C = nH * hd
        u_op = U_BF16 if dtype == torch.bfloat16 else U32
        u_out = u_op
        Q = _heads(qkv[:, :C], nseq, L, nH, hd, row_index)
        K = _heads(qkv[:, C:2 * C], nseq, L, nH, hd, row_index)
        V = _heads(qkv[:, 2 * C:], nseq, L, nH, hd, row_index)
        s = scale * (Q @ K.transpose(-1, -2)) + bias.to(dev).double()
        qvalid = torch.ones(nseq, 1, L, 1, dtype=torch.bool, device=dev)
        if seq_len is not None:
            ar = torch.arange(L, device=dev)
            kvalid = ar[None, :] < seq_len.long()[:, None]
            s = torch.where(kvalid[:, None, None, :], s, torch.full_like(s, MASK_OUT))
            qvalid = kvalid[:, None, :, None]
        ds = C_ACC * U32 * math.sqrt(hd) * scale * (Q.abs() @ K.abs().transpose(-1, -2)) + 2 * U32 * s.abs()
        m = s.amax(-1, keepdim=True)
        e = torch.exp(s - m)
        ssum = e.sum(-1, keepdim=True)
        P = e / ssum
        lse = m + torch.log(ssum)
        de = C_EXP * U32 + 2 * U32 * (s - m).abs()
        pds = (P * ds).sum(-1, keepdim=True)
        pde = (P * de).sum(-1, keepdim=True)
        sum_rel = pde + C_ACC * U32 * math.sqrt(L)
        dP = P * (ds + pds + de + sum_rel + 3 * U32)
        D = torch.ones_like(P) if keep is None else keep.to(dev).double() / (1.0 - p)
        Pd = P * D
        out = Pd @ V
        aV = V.abs()
        out_b = (D * dP + (u_op + U32) * Pd) @ aV + C_ACC * U32 * math.sqrt(L) * (Pd @ aV) + u_out * out.abs()
        lse_b = pds + sum_rel + C_LOG * U32 * (lse.abs() + 1.0)
        self.out, self.out_b = _rows(out, row_index), SAFETY * _rows(out_b, row_index) + 1e-30
        nanq = ~qvalid[..., 0]
        self.lse = lse[..., 0].masked_fill(nanq, float("nan"))
        self.lse_b = SAFETY * lse_b[..., 0] + 1e-30
        self.P, self.s = P, s
        if dout is None:
            return
        dO = _heads(dout, nseq, L, nH, hd, row_index) * qvalid          # rows a sequence does not have send nothing
        eO = torch.zeros_like(dO) if dout_err is None else _heads(dout_err.to(dev), nseq, L, nH, hd, row_index) * qvalid
        dPd = dO @ V.transpose(-1, -2)
        dPk = dPd * D
        delta = (dO * out).sum(-1, keepdim=True)                          # == rowsum(P o dP)
        dS = P * (dPk - delta)
        dQ = scale * (dS @ K)
        dK = scale * (dS.transpose(-1, -2) @ Q)
        dV = Pd.transpose(-1, -2) @ dO
        # backward: P recomputed as exp(s - lse_saved)
        relPb = ds + lse_b + C_EXP * U32 + 2 * U32 * (s - lse).abs() + U32
        dPb = P * relPb
        ddp = D * (C_ACC * U32 * math.sqrt(hd) * (dO.abs() @ aV.transpose(-1, -2)) + eO @ aV.transpose(-1, -2)) + U32 * dPk.abs()
        del_pp = (dPb * dPk.abs() + P * ddp).sum(-1, keepdim=True) + C_ACC * U32 * math.sqrt(L) * (P * dPk).abs().sum(-1, keepdim=True)
        del_oo = ((dO.abs() + eO) * out_b + eO * out.abs()).sum(-1, keepdim=True) + \
            C_ACC * U32 * math.sqrt(hd) * (dO * out).abs().sum(-1, keepdim=True)
        ddelta = torch.maximum(del_pp, del_oo)
        self.dS_b = dPb * (dPk - delta).abs() + P * (ddp + ddelta) + (u_op + 2 * U32) * dS.abs()
        self.dS = dS
        aK, aQ, adO = K.abs(), Q.abs(), dO.abs()
        sq = C_ACC * U32 * math.sqrt(L)
        dQ_b = scale * (self.dS_b @ aK + sq * (dS.abs() @ aK)) + (u_out + U32) * dQ.abs()
        dK_b = scale * (self.dS_b.transpose(-1, -2) @ aQ + sq * (dS.abs().transpose(-1, -2) @ aQ)) + (u_out + U32) * dK.abs()
        dV_b = (D * dPb + u_op * Pd).transpose(-1, -2) @ adO + sq * (Pd.transpose(-1, -2) @ adO) + u_out * dV.abs()
        if dout_err is not None:
            dV_b = dV_b + Pd.transpose(-1, -2) @ eO
        self.dqkv = torch.cat([_rows(dQ, row_index), _rows(dK, row_index), _rows(dV, row_index)], 1)
        self.dqkv_b = SAFETY * torch.cat([_rows(dQ_b, row_index), _rows(dK_b, row_index), _rows(dV_b, row_index)], 1) + 1e-30

    def dbias_table(self):
        """Swin: the relative-position bias-table gradient [169, nH] (f32 output) and its bound: the dS of every
        (window, q, k) that shares a relative index, summed."""
        from oracle import mvlt_oracle as O
        idx = O.relative_position_index(7).view(-1).to(self.dS.device)
        nH = self.dS.shape[1]
        dS = self.dS.permute(0, 2, 3, 1).reshape(-1, 49 * 49, nH).sum(0)
        aS = self.dS.abs().permute(0, 2, 3, 1).reshape(-1, 49 * 49, nH).sum(0)
        bS = self.dS_b.permute(0, 2, 3, 1).reshape(-1, 49 * 49, nH).sum(0)
        ref = torch.zeros(169, nH, dtype=torch.float64, device=dS.device).index_add_(0, idx, dS)
        a = torch.zeros_like(ref).index_add_(0, idx, aS)
        b = torch.zeros_like(ref).index_add_(0, idx, bS)
        cnt = torch.bincount(idx, minlength=169).double()[:, None] * self.dS.shape[0]
        return ref, SAFETY * (b + C_ACC * U32 * cnt.sqrt() * a + U32 * ref.abs()) + 1e-30


def check_lse(lse, ref):
    """lse [nseq, nH, L] against AttnRef.lse / lse_b: only the queries a sequence has; a failure names
    (sequence, head, query)."""
    ok = torch.isfinite(ref.lse)
    got = lse.double().to(ref.lse.device)
    nseq, nH, L = ref.lse.shape
    # row = seq * L + q, column = head
    r = lambda t: t.permute(0, 2, 1).reshape(nseq * L, nH)  # noqa: E731
    okr = r(ok)
    want, bound, out = r(ref.lse), r(ref.lse_b), r(got)
    want = torch.where(okr, want, torch.zeros_like(want))
    out = torch.where(okr, out, torch.zeros_like(out))
    check_bound(out, want, bound, f"lse (row = sequence * {L} + query, column = head)")


def cached_ref(qkv_new, k_cache, v_cache, past, scale):
    """mvlt_attn_cached in float64: new row r of (b, h) attends to the keys cache[0, past) + the new rows 0..r (causal
    over the new rows).  Built as the last n_new query rows of one sequence of past + n_new tokens, so the bound is the
    forward bound of AttnRef (P kept in f32 by these kernels: the compute-dtype term of P is then loose, never short).
    Returns (out, bound) [B n_new, nH hd]."""
    B, nH, _, hd = k_cache.shape
    n_new = qkv_new.shape[0] // B
    L = past + n_new
    C = nH * hd
    dev = qkv_new.device
    full = torch.zeros(B, L, 3, nH, hd, dtype=torch.float64, device=dev)
    new = qkv_new.double().view(B, n_new, 3, nH, hd)
    full[:, past:] = new
    full[:, :past, 1] = k_cache[:, :, :past].double().permute(0, 2, 1, 3)
    full[:, :past, 2] = v_cache[:, :, :past].double().permute(0, 2, 1, 3)
    ar = torch.arange(L, device=dev)
    bias = torch.where(ar[None, :] <= ar[:, None], 0.0, MASK_OUT).double()[None, None]
    ref = AttnRef(full.view(B * L, 3 * C), None, nseq=B, L=L, nH=nH, hd=hd, scale=scale, bias=bias, dtype=qkv_new.dtype)
    rows = (torch.arange(B, device=dev)[:, None] * L + past + torch.arange(n_new, device=dev)[None, :]).view(-1)
    return ref.out[rows], ref.out_b[rows]


def layernorm_ref(x, gamma, beta, eps, out_dtype=torch.bfloat16, dv=None):
    """LayerNorm in float64 and its bound for an f32 evaluation rounded to out_dtype: the mean and the variance are f32
    sums over C (C_ACC 2^-24 sqrt(C) each), the normalised value and the affine map a few f32 roundings (4 2^-24), the
    output rounding U_OUT (2^-8 for bf16, 2^-24 for f32).
    dv: optional per-element bound on the error of the row the kernel normalises against x (a row the kernel forms itself
    in f32, mvlt_layernorm_acc_fwd: the additions of the slabs, the bias and the residual).  To first order a perturbation
    d of the row moves y by gamma rstd (d - mean(d) - xh mean(xh d)), so dv enters as
    |gamma| rstd (dv + mean(dv) + |xh| mean(|xh| dv)).  Returns (y, bound) of the rows of x."""
    x = x.double()
    C = x.shape[1]
    g, b = gamma.double().to(x.device), beta.double().to(x.device)
    mu = x.mean(1, keepdim=True)
    var = ((x - mu) ** 2).mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    xh = (x - mu) * rstd
    y = xh * g + b
    sq = C_ACC * U32 * math.sqrt(C)
    d_mu = sq * x.abs().mean(1, keepdim=True)
    u_out = U32 if out_dtype == torch.float32 else U_BF16
    est = g.abs() * (d_mu * rstd + (sq + 4 * U32) * xh.abs()) + 4 * U32 * b.abs() + u_out * y.abs()
    if dv is not None:
        dv = dv.double().to(x.device)
        est = est + g.abs() * rstd * (dv + dv.mean(1, keepdim=True) + xh.abs() * (xh.abs() * dv).mean(1, keepdim=True))
    return y, SAFETY * est + 1e-30
