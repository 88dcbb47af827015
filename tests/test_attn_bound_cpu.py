"""The per-element attention bound of tests/attn_ref.py can fail: on the host it accepts an emulation of the kernels'
roundings (f32 logits, P and dS rounded to bf16, bf16 outputs, lse and delta in f32) at a ratio <= 0.5, and rejects
faults a relative Frobenius norm over the whole output lets through, each on a single (sequence, head)."""
import pytest
import torch

from attn_ref import (MASK_OUT, AttnRef, _heads, _rows, attn_keep, attn_operands, bert_bias, check_bound, check_lse,
                      M32, _mix32_int, keep_ref, pack_layout, rng_u32, swin_bias)

BF = torch.bfloat16


def emulate(qkv, dout, *, nseq, L, nH, hd, scale, bias, keep=None, p=0.0, pack=None, delta_from_out=True, fault=None):
    """The kernels' arithmetic in f32 with their bf16 roundings; `fault` = {name: (seq, head, arg)} bends one step."""
    fault = fault or {}
    row_index = None if pack is None else pack[0]
    C = nH * hd
    f = lambda t: _heads(t, nseq, L, nH, hd, row_index).float()  # noqa: E731
    Q, K, V = f(qkv[:, :C]), f(qkv[:, C:2 * C]), f(qkv[:, 2 * C:])
    b = bias.expand(nseq, nH, L, L).float().clone()
    if pack is not None:
        kvalid = torch.arange(L)[None, :] < pack[1].long()[:, None]
        b = torch.where(kvalid[:, None, None, :], b, torch.full_like(b, MASK_OUT))
    if "bias" in fault:
        s_, h_, fn = fault["bias"]
        b[s_, h_] = fn(b[s_, h_])
    s = (Q @ K.transpose(-1, -2)) * scale + b
    m = s.amax(-1, keepdim=True)
    e = torch.exp(s - m)
    ssum = e.sum(-1, keepdim=True)
    P = e / ssum
    lse = (m + torch.log(ssum))[..., 0]
    if "lse" in fault:
        s_, h_, q_ = fault["lse"]
        k_ = int(P[s_, h_, q_].argmax())
        lse[s_, h_, q_] = torch.log(ssum[s_, h_, q_, 0] - e[s_, h_, q_, k_]) + m[s_, h_, q_, 0]
    D = torch.ones_like(P) if keep is None else keep.float() / (1.0 - p)
    if "keep" in fault:
        s_, h_, fn = fault["keep"]
        D[s_, h_] = fn(D[s_, h_])
    out = ((P * D).to(BF).float() @ V).to(BF)
    Pb = torch.exp(s - lse[..., None])
    dO = f(dout)
    dP = (dO @ V.transpose(-1, -2)) * D
    delta = (dO * out.float()).sum(-1, keepdim=True) if delta_from_out else (Pb * dP).sum(-1, keepdim=True)
    if "delta" in fault:
        s_, h_, t_ = fault["delta"]
        delta[s_, h_, 16 * t_:16 * t_ + 16] = delta[s_, h_, 16 * t_ + 1:16 * t_ + 17].clone()
    dS = Pb * (dP - delta)
    dSb = (dS * scale).to(BF).float()
    dQ = dSb @ K
    dK = dSb.transpose(-1, -2) @ Q
    dV = (Pb * D).to(BF).float().transpose(-1, -2) @ dO
    rows = lambda t: _rows(t.double(), row_index)  # noqa: E731
    out_r = rows(out.float())
    if "out_row" in fault:
        r_, h_ = fault["out_row"]
        out_r[r_, h_ * hd:(h_ + 1) * hd] = out_r[r_, (h_ + 1) * hd:(h_ + 2) * hd]
    dqkv = torch.cat([rows(dQ), rows(dK), rows(dV)], 1).to(BF)
    return out_r.to(BF), lse, dqkv, dS


def _check_all(ref, got, hd, nH, what):
    out, lse, dqkv, _ = got
    check_bound(out, ref.out, ref.out_b, f"{what} out", heads=(hd, nH))
    check_lse(lse, ref)
    check_bound(dqkv, ref.dqkv, ref.dqkv_b, f"{what} dqkv", heads=(hd, nH))


def _worst(got, ref):
    out, lse, dqkv, _ = got
    r1 = float(((out.double() - ref.out).abs() / ref.out_b).max())
    ok = torch.isfinite(ref.lse)
    r2 = float(((lse.double() - ref.lse).abs() / ref.lse_b)[ok].max())
    r3 = float(((dqkv.double() - ref.dqkv).abs() / ref.dqkv_b).max())
    return max(r1, r2, r3)


# ------------------------------------------------------------------ the three layouts
@pytest.fixture(scope="module")
def swin():
    """A shifted block at res 14 (4 windows: 0..2 interior or one border, 3 the corner), 2 images, 3 heads."""
    res, shift, nH, hd = 14, 3, 3, 32
    nW = (res // 7) ** 2
    nseq = 2 * nW
    qkv, dout = attn_operands(nseq, 49, nH, hd, BF, 201)
    table = (0.5 * torch.randn(169, nH, generator=torch.Generator().manual_seed(202))).float()
    bias = swin_bias(table, nW, res, shift, nseq)
    kw = dict(nseq=nseq, L=49, nH=nH, hd=hd, scale=hd ** -0.5)
    ref = AttnRef(qkv, dout, bias=bias, dtype=BF, **kw)
    return dict(qkv=qkv, dout=dout, bias=bias, kw=kw, ref=ref, nW=nW, table=table)


@pytest.fixture(scope="module")
def bert():
    """MVLBert L = 131 (49 image tokens, T = 80) with padded captions, an image_mask and attention dropout 0.1."""
    n_img, T, nH, hd, p = 49, 80, 2, 64, 0.1
    L = n_img + 2 + T
    lens = [80, 37, 1, 0]
    nseq = len(lens)
    ids = torch.zeros(nseq, T, dtype=torch.long)
    for b, ln in enumerate(lens):
        ids[b, :ln] = 5 + torch.arange(ln)
    im = torch.ones(nseq, n_img, dtype=torch.uint8)
    im[1, 0] = im[1, -1] = 0
    qkv, dout = attn_operands(nseq, L, nH, hd, BF, 203)
    bias = bert_bias(False, nseq, L, n_img, ids, im)
    keep = attn_keep(99, 5, p, nseq, nH, L)
    kw = dict(nseq=nseq, L=L, nH=nH, hd=hd, scale=hd ** -0.5, keep=keep, p=p)
    ref = AttnRef(qkv, dout, bias=bias, dtype=BF, **kw)
    return dict(qkv=qkv, dout=dout, bias=bias, kw=kw, ref=ref, lens=lens, n_img=n_img, L=L, nH=nH, hd=hd)


@pytest.fixture(scope="module")
def packed():
    """Packed seq2seq rows with gaps (NaN) between three sequences of 131, 60 and 100 rows."""
    L, nH, hd, n_img = 131, 2, 64, 49
    row_start, seq_len, R, row_index = pack_layout([131, 60, 100], L)
    nseq = 3
    qkv, dout = attn_operands(nseq, L, nH, hd, BF, 204, rows=R, row_index=row_index)
    bias = bert_bias(True, nseq, L, n_img)
    kw = dict(nseq=nseq, L=L, nH=nH, hd=hd, scale=hd ** -0.5)
    ref = AttnRef(qkv, dout, bias=bias, dtype=BF, pack=(row_index, seq_len), **kw)
    return dict(qkv=qkv, dout=dout, bias=bias, kw=kw, ref=ref, pack=(row_index, seq_len))


@pytest.mark.parametrize("case", ["swin", "bert", "packed"])
@pytest.mark.parametrize("delta_from_out", [True, False])
def test_bound_accepts_emulated_kernels(case, delta_from_out, request):
    c = request.getfixturevalue(case)
    got = emulate(c["qkv"], c["dout"], bias=c["bias"], pack=c.get("pack"), delta_from_out=delta_from_out, **c["kw"])
    _check_all(c["ref"], got, c["kw"]["hd"], c["kw"]["nH"], case)
    assert _worst(got, c["ref"]) <= 0.5


def test_operands_spread_the_logits(bert):
    P = bert["ref"].P
    assert float(P.amax(-1).median()) > 0.2            # peaked rows: a wrong key or row is not averaged away
    s = bert["ref"].s[0, 0, :, :51] - bert["bias"][0, 0, :, :51]
    assert 2.0 < float(s.std()) < 3.0


def test_swin_bias_gradient_accepts_and_rejects_a_missing_window(swin):
    ref = swin["ref"]
    want, bound = ref.dbias_table()
    _, _, _, dS = emulate(swin["qkv"], swin["dout"], bias=swin["bias"], **swin["kw"])
    from oracle import mvlt_oracle as O
    idx = O.relative_position_index(7).view(-1)
    def table(dS):
        return torch.zeros(169, dS.shape[1], dtype=torch.float64).index_add_(0, idx, dS.double().permute(0, 2, 3, 1).reshape(-1, 2401, dS.shape[1]).sum(0))
    got = table(dS).float()
    check_bound(got, want, bound, "dbias_table", heads=(1, dS.shape[1]))
    assert float(((got.double() - want).abs() / bound).max()) <= 0.5
    dS2 = dS.clone()
    dS2[5, 1] = 0                                     # window 5 of head 1 never flushed
    with pytest.raises(AssertionError, match=r"outside the bound.*head 1\)"):
        check_bound(table(dS2).float(), want, bound, "dbias_table", heads=(1, dS.shape[1]))


# ------------------------------------------------------------------ faults, each on one (sequence, head)
def _rejects(c, match, **fault):
    got = emulate(c["qkv"], c["dout"], bias=c["bias"], pack=c.get("pack"), fault=fault, **c["kw"])
    with pytest.raises(AssertionError, match=match):
        _check_all(c["ref"], got, c["kw"]["hd"], c["kw"]["nH"], "fault")


def test_rejects_key_mask_off_by_one(bert):
    first_pad = bert["n_img"] + 2 + bert["lens"][1]     # the mask ends one key late: the first padded key of sequence 1 is read
    def fn(b):
        b = b.clone()
        b[:, first_pad] = 0.0
        return b
    _rejects(bert, r"head 1\)", bias=(1, 1, fn))


def test_rejects_last_partial_key_tile_dropped(bert):
    def fn(b):
        b = b.clone()
        b[:, 128:131] = MASK_OUT
        return b
    _rejects(bert, r"outside the bound.*head 0\)", bias=(0, 0, fn))


def test_rejects_row_from_neighbouring_head(bert):
    _rejects(bert, r"row 200, column \d+ \(part 0, head 0\)", out_row=(200, 0))


def test_rejects_shift_mask_in_interior_window(swin):
    from oracle import mvlt_oracle as O
    corner = O.shift_attn_mask(14, 14, 7, 3)[3].float()
    _rejects(swin, r"head 2\)", bias=(4, 2, lambda b: b + corner))       # sequence 4 = window 0 of image 1


def test_rejects_transposed_relative_index(swin):
    _rejects(swin, r"head 1\)", bias=(2, 1, lambda b: b.t().contiguous()))


def test_rejects_dropout_index_q_k_swapped(bert):
    _rejects(bert, r"head 1\)", keep=(0, 1, lambda d: d.t().contiguous()))


def test_rejects_lse_missing_a_key(bert):
    with pytest.raises(AssertionError, match=r"lse .*row 400, column 1"):
        got = emulate(bert["qkv"], bert["dout"], bias=bert["bias"], fault={"lse": (3, 1, 400 - 3 * 131)}, **bert["kw"])
        check_lse(got[1], bert["ref"])


def test_rejects_delta_shifted_by_a_row(packed):
    _rejects(packed, r"dqkv.*head 0\)", delta=(1, 0, 2))


def test_rejects_image_mask_ignored(bert):
    def fn(b):
        b = b.clone()
        b[:, 1 + bert["n_img"] - 1] = 0.0                # the last image key of sequence 1 is masked: read it anyway
        return b
    _rejects(bert, r"head 0\)", bias=(1, 0, fn))


# ------------------------------------------------------------------ the dropout hash
def test_keep_ref_is_deterministic_and_keeps_one_minus_p():
    idx = torch.arange(1 << 20, dtype=torch.int64)
    a, b = keep_ref(1234, 7, idx, 0.1), keep_ref(1234, 7, idx, 0.1)
    assert torch.equal(a, b)
    assert not torch.equal(a, keep_ref(1235, 7, idx, 0.1)) and not torch.equal(a, keep_ref(1234, 8, idx, 0.1))
    n = idx.numel()
    frac = float(a.double().mean())
    sigma = (0.9 * 0.1 / n) ** 0.5
    assert abs(frac - 0.9) < 5 * sigma, frac
    # the 16-bit split multiply of the tensor port against plain Python integers, up to the top of the uint32 range
    hi = torch.cat([torch.arange((1 << 32) - 1024, 1 << 32), torch.tensor([0, 1, 0x7FFFFFFF, 0x80000000, 0xDEADBEEF])])
    for seed, tag in ((1234, 7), ((1 << 40) + 12345, 0xFFFFFFFF)):
        got = rng_u32(seed, tag, hi)
        key = _mix32_int((seed & M32) ^ ((tag * 0x9E3779B9) & M32)) ^ (seed >> 32)
        want = torch.tensor([_mix32_int(((i * 0x9E3779B1) + key) & M32) for i in hi.tolist()])
        assert torch.equal(got, want)
        thresh = int(float(torch.tensor(0.1, dtype=torch.float32)) * 4294967296.0)
        assert torch.equal(keep_ref(seed, tag, hi, 0.1), want >= thresh)
