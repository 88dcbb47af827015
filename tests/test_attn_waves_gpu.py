"""The bf16 MVLBert attention kernels that give every tile a wave of its own (csrc/attn.hip): bert_attn_fwd_kernel, one
query tile per wave, behind BERT_FWD_KT5 / KT9 / KT13, and bert_attn_bwd2_kernel, one key tile per wave (10 / 12 waves),
behind BERT_BWD2_NW5 / NW6.  Checked like tests/test_attn_routes_gpu.py: the float64 reference and per-element bounds of
tests/attn_ref.py, outputs pre-filled with NaN, gap rows of packed batches and lse entries at q >= seq_len must keep
their fill.  The shapes sit where the wave <-> tile ownership can go wrong:
  * sequences of 131 / 96 / 80 / 64 / 51 rows in one packed launch at 12 heads: 9 / 6 / 5 / 4 / 4 tiles, so waves without
    a tile in every sequence but the first (they must still reach every barrier), lengths that are exact multiples of the
    16-row tile and of the 32-query block of the backward, and one that is neither;
  * more (sequence, head) pairs than one dispatch round holds (576 workgroups);
  * the 12-key-tile backward and the 13-tile forward.
All cases: bf16, head dim 64, 49 image tokens (obj_end 50)."""
import pytest
import torch

from attn_ref import AttnRef, attn_keep, attn_operands, bert_bias, check_bound, check_lse, pack_layout

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
NAN = float("nan")
N_IMG, HD = 49, 64

#        id                  T    caption lengths        packed  nH  s2s    forward route     backward route
CASES = {
    "edges-bidir":   dict(T=80, lens=[80, 45, 29, 13, 0], pack=True, nH=12, s2s=False, fwd="BERT_FWD_KT9", bwd="BERT_BWD2_NW5"),
    "edges-s2s":     dict(T=80, lens=[80, 45, 29, 13, 0], pack=True, nH=12, s2s=True, fwd="BERT_FWD_KT9", bwd="BERT_BWD2_NW5"),
    # 48 x 12 = 576 workgroups: a second dispatch round of the same launch (at most two workgroups per CU are resident)
    "two-rounds":    dict(T=23, lens=[(7 * b) % 24 for b in range(48)], pack=False, nH=12, s2s=False,
                          fwd="BERT_FWD_KT5", bwd="BERT_BWD2_NW5"),
    # L_s = 192 / 176 / 161: 12 / 11 / 11 key tiles
    "bwd-12-tiles":  dict(T=141, lens=[141, 125, 110], pack=True, nH=4, s2s=True, fwd="BERT_FWD_KT13", bwd="BERT_BWD2_NW6"),
    # L_s = 208 / 161: 13 / 11 query tiles; the backward of this shape is the two-launch split route
    "fwd-13-tiles":  dict(T=157, lens=[157, 110], pack=True, nH=4, s2s=False, fwd="BERT_FWD_KT13", bwd="BERT_BWD_SPLIT_KT13"),
}
DROP = (0.1, 99, 5)                 # p, seed, tag


def _setup(c):
    from mvlt_amd._lib import ATTN_BIDIR, ATTN_SEQ2SEQ
    T, lens, nH = c["T"], c["lens"], c["nH"]
    nseq, L = len(lens), N_IMG + 2 + T
    ids = torch.zeros(nseq, T, dtype=torch.long)
    for b, ln in enumerate(lens):
        ids[b, :ln] = 5 + torch.arange(ln)
    rows = row_index = pack = None
    if c["pack"]:
        row_start, seq_len, rows, row_index = pack_layout([N_IMG + 2 + ln for ln in lens], L)
        pack = (row_start.cuda(), seq_len.cuda(), rows)
    qkv, dout = attn_operands(nseq, L, nH, HD, BF, 900 + L + nH, rows=rows, row_index=row_index)
    qkv, dout = qkv.cuda(), dout.cuda()
    kw = dict(text_ids=ids.cuda(), obj_end=N_IMG + 1, dropout=DROP)
    if pack is not None:
        kw["pack"] = pack
    args = (ATTN_SEQ2SEQ if c["s2s"] else ATTN_BIDIR, nseq, L, nH, HD, 0.125)
    return qkv, dout, args, kw, ids, row_index, (None if pack is None else seq_len)


def _run(ops, qkv, dout, args, kw):
    nseq, L, nH = args[1], args[2], args[3]
    out = torch.full((qkv.shape[0], nH * HD), NAN, dtype=BF, device="cuda")
    lse = torch.full((nseq, nH, L), NAN, dtype=torch.float32, device="cuda")
    ops.attn_fwd(qkv, *args, out=out, lse=lse, **kw)
    dqkv = torch.full_like(qkv, NAN)
    ops.attn_bwd(dout, qkv, out, lse, *args, dqkv=dqkv, **kw)
    torch.cuda.synchronize()
    return out, lse, dqkv


@pytest.fixture(scope="module")
def ops():
    from mvlt_amd import ops as o
    return o


@pytest.mark.parametrize("name", list(CASES))
def test_one_tile_per_wave(ops, name):
    c = CASES[name]
    qkv, dout, args, kw, ids, row_index, seq_len = _setup(c)
    nseq, L, nH = args[1], args[2], args[3]
    assert ops.attn_route(qkv, *args, **kw) == c["fwd"]
    assert ops.attn_route(qkv, *args, bwd=True, **kw) == c["bwd"]
    keep = attn_keep(DROP[1], DROP[2], DROP[0], nseq, nH, L, "cuda")
    bias = bert_bias(c["s2s"], nseq, L, N_IMG, ids).cuda()
    ref = AttnRef(qkv, dout, nseq=nseq, L=L, nH=nH, hd=HD, scale=0.125, bias=bias, dtype=BF, keep=keep, p=DROP[0],
                  pack=None if row_index is None else (row_index, seq_len))
    out, lse, dqkv = _run(ops, qkv, dout, args, kw)
    gap = None
    if row_index is not None:
        gap = torch.ones(qkv.shape[0], dtype=torch.bool).index_fill_(0, row_index[row_index >= 0], False).cuda()
        assert bool(gap.any())
    check_bound(out if gap is None else out[~gap], ref.out, ref.out_b, "out", heads=(HD, nH))
    check_lse(lse, ref)
    assert torch.isnan(lse.cpu()[~torch.isfinite(ref.lse.cpu())]).all(), "lse written at q >= seq_len"
    check_bound(dqkv if gap is None else dqkv[~gap], ref.dqkv, ref.dqkv_b, "dqkv", heads=(HD, nH))
    if gap is not None:
        assert torch.isnan(out[gap]).all(), "a gap row of out was written"
        assert torch.isnan(dqkv[gap]).all(), "a gap row of dqkv was written"


@pytest.mark.parametrize("name", ["edges-bidir", "edges-s2s"])
def test_one_tile_per_wave_is_bit_reproducible(ops, name):
    """No atomics and no hand-off between workgroups: two calls on the same operands agree bit for bit (the NaN fill of
    gap rows included, hence the integer views)."""
    qkv, dout, args, kw, *_ = _setup(CASES[name])
    a = _run(ops, qkv, dout, args, kw)
    b = _run(ops, qkv, dout, args, kw)
    for x, y, what in zip(a, b, ("out", "lse", "dqkv")):
        iv = torch.int32 if x.dtype == torch.float32 else torch.int16
        assert torch.equal(x.view(iv), y.view(iv)), what
