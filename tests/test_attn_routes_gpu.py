"""Every MvltAttn dispatch route (csrc/attn.hip: attn_route) against the float64 reference of tests/attn_ref.py with a
PER-ELEMENT bound: out and lse of the forward, dqkv and the Swin bias-table gradient of the backward.

Each row of ROUTES names the kernel it targets and the attn_route condition that sends it there, and asserts
ops.attn_route first (forward and backward): a threshold that moves a shape off its route fails here and the row gets
re-pointed instead of quietly testing another kernel.  Outputs start filled with NaN; packed rows leave gaps of NaN
rows in qkv / dout that must not be read, and the gap rows of out / dqkv and the lse entries at q >= seq_len must keep
their fill.  A backward whose forward route is unsupported (f32 beyond 192 rows) reads the reference's out / lse.
The KV-cache kernels (mvlt_attn_cached) and the fused Swin half (mvlt_swin_wmsa2_fwd / _bwd, stage by stage) follow.
Everything here calls ops.* directly.  How a Swin block wires these kernels together -- swin.py _block_fwd / _block_bwd and
csrc/host.cpp swin_block_fwd / swin_block_bwd, every forward and backward mode on both host paths -- is judged per element in
tests/test_swin_attn_half_gpu.py (reference: tests/swin_attn_half_ref.py, proven in tests/test_swin_attn_half_cpu.py)."""
import math

import pytest
import torch

from attn_ref import C_ACC, U32, U_BF16, AttnRef, attn_keep, attn_operands, bert_bias, check_bound, check_lse, keep_ref, pack_layout, swin_bias

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
NAN = float("nan")


@pytest.fixture(scope="module")
def ops():
    from mvlt_amd import ops as o
    return o


def S(id, dt, res, nH, shift, B, fwd, bwd, drop=0.0, proj=False):
    return pytest.param(dict(kind="swin", dt=dt, res=res, nH=nH, shift=shift, B=B, fwd=fwd, bwd=bwd, drop=drop, proj=proj),
                        id=id)


def B_(id, dt, T, fwd, bwd, nseq=3, nH=4, s2s=False, drop=0.0, lens=None, image_mask=False, delta_ws=True, pack=False):
    return pytest.param(dict(kind="bert", dt=dt, T=T, fwd=fwd, bwd=bwd, nseq=nseq, nH=nH, s2s=s2s, drop=drop, lens=lens,
                             image_mask=image_mask, delta_ws=delta_ws, pack=pack), id=id)


ROUTES = [
    # ---- Swin (hd 32, L 49): attn_fwd_kernel<T, 32, 4, SWIN>; the backward takes swin_attn_bwd2_kernel (scores once) for
    #      bf16 without dropout and shift 0 / 3 (KS = heads with dout_weight, else 0), attn_bwd_kernel otherwise
    S("swin-r14-s3-bf16", BF, 14, 12, 3, 2, "SWIN_FWD", "SWIN_BWD_KS0"),            # border windows, SWIN_PAIRS path
    S("swin-r14-s3-f32", F32, 14, 12, 3, 2, "SWIN_FWD", "SWIN_BWD"),                # f32: generic backward
    S("swin-r7-s0-24h", BF, 7, 24, 0, 4, "SWIN_FWD", "SWIN_BWD_KS0"),               # stage 3: one window, 24 heads
    S("swin-r7-s0-24h-f32", F32, 7, 24, 0, 4, "SWIN_FWD", "SWIN_BWD"),
    # B = 32 at res 56, 3 heads: 2048 windows; forward grid capped at 2048 / 3 = 682, backward at the CU count
    S("swin-r56-B32", BF, 56, 3, 3, 32, "SWIN_FWD", "SWIN_BWD_KS0"),
    S("swin-r28-B32", BF, 28, 6, 0, 32, "SWIN_FWD", "SWIN_BWD_KS0"),               # stage 1: 6272 windows x 6 heads, capped
    S("swin-r14-B32", BF, 14, 12, 3, 32, "SWIN_FWD", "SWIN_BWD_KS0"),              # stage 2: 128 windows x 12 heads
    S("swin-r14-s5", BF, 14, 12, 5, 2, "SWIN_FWD", "SWIN_BWD"),                     # shift 5: SwinLane::init, generic bwd
    S("swin-r14-s3-drop", BF, 14, 12, 3, 2, "SWIN_FWD", "SWIN_BWD", drop=0.1),      # attention dropout: generic bwd
    # dout_weight (output-projection dgrad inside the launch): KS = 3 / 6 / 12 at the B = 32 stage shapes, and below the cap
    S("swin-ks3-stage0", BF, 56, 3, 3, 32, "SWIN_FWD", "SWIN_BWD_KS3", proj=True),
    S("swin-ks6-stage1", BF, 28, 6, 0, 32, "SWIN_FWD", "SWIN_BWD_KS6", proj=True),
    S("swin-ks12-stage2", BF, 14, 12, 3, 32, "SWIN_FWD", "SWIN_BWD_KS12", proj=True),
    S("swin-ks12-small", BF, 14, 12, 3, 2, "SWIN_FWD", "SWIN_BWD_KS12", proj=True),
    S("swin-ks3-small-s0", BF, 56, 3, 0, 1, "SWIN_FWD", "SWIN_BWD_KS3", proj=True),
    # ---- MVLBert (hd 64, L = 51 + T): forward KT = 5 / 9 / 13 key tiles (L <= 80 / 144 / 208); backward bf16 one launch
    #      (bert_attn_bwd2, NT <= 10: 5 waves, <= 12: 6 waves), else the two-launch split with delta_ws, else generic
    B_("bert-L74-bf16", BF, 23, "BERT_FWD_KT5", "BERT_BWD2_NW5"),
    B_("bert-L74-f32", F32, 23, "BERT_FWD_KT5", "BERT_BWD_SPLIT_KT5"),
    B_("bert-L74-f32-generic", F32, 23, "BERT_FWD_KT5", "BERT_BWD_KT5", delta_ws=False),
    # the step: L = 131, dropout 0.1, every caption length 0 .. 80
    B_("bert-L131-step", BF, 80, "BERT_FWD_KT9", "BERT_BWD2_NW5", nseq=81, nH=2, drop=0.1, lens=list(range(81))),
    B_("bert-L131-f32-split", F32, 80, "BERT_FWD_KT9", "BERT_BWD_SPLIT_KT9", drop=0.1),
    B_("bert-L131-f32-generic", F32, 80, "BERT_FWD_KT9", "BERT_BWD_KT9", drop=0.1, delta_ws=False),
    B_("bert-L131-s2s", BF, 80, "BERT_FWD_KT9", "BERT_BWD2_NW5", s2s=True, drop=0.1),
    B_("bert-L131-image-mask", BF, 80, "BERT_FWD_KT9", "BERT_BWD2_NW5", image_mask=True),
    B_("bert-L160", BF, 109, "BERT_FWD_KT13", "BERT_BWD2_NW5", s2s=True, drop=0.1),     # 10 key tiles: 5 waves
    B_("bert-L161", BF, 110, "BERT_FWD_KT13", "BERT_BWD2_NW6", drop=0.1),               # 11: 6 waves
    B_("bert-L179", BF, 128, "BERT_FWD_KT13", "BERT_BWD2_NW6"),
    B_("bert-L192", BF, 141, "BERT_FWD_KT13", "BERT_BWD2_NW6", s2s=True),
    B_("bert-L193", BF, 142, "BERT_FWD_KT13", "BERT_BWD_SPLIT_KT13", drop=0.1),         # 13 key tiles: split KT13
    B_("bert-L208", BF, 157, "BERT_FWD_KT13", "BERT_BWD_SPLIT_KT13", s2s=True),
    B_("bert-L179-f32-split", F32, 128, "BERT_FWD_KT13", "BERT_BWD_SPLIT_KT13"),         # 12 key tiles
    B_("bert-L193-f32-split", F32, 142, "UNSUPPORTED", "BERT_BWD_SPLIT_KT13"),           # f32 forward at 13 tiles: > 160 KB LDS
    # packed rows with NaN gaps
    B_("bert-packed-s2s", BF, 80, "BERT_FWD_KT9", "BERT_BWD2_NW5", s2s=True, drop=0.1, lens=[80, 79, 0, 13], pack=True),
    B_("bert-packed-bidir-f32", F32, 80, "BERT_FWD_KT9", "BERT_BWD_SPLIT_KT9", lens=[80, 29, 1], pack=True),
    B_("bert-packed-L193", BF, 142, "BERT_FWD_KT13", "BERT_BWD_SPLIT_KT13", lens=[142, 100, 60], pack=True),
]


def _swin_case(ops, c):
    from mvlt_amd._lib import ATTN_SWIN
    dt, res, nH, shift, B = c["dt"], c["res"], c["nH"], c["shift"], c["B"]
    nW = (res // 7) ** 2
    nseq, hd, Cn = B * nW, 32, nH * 32
    qkv, dout = attn_operands(nseq, 49, nH, hd, dt, 300 + res + nH)
    table = (0.5 * torch.randn(169, nH, generator=torch.Generator().manual_seed(301))).float().cuda()
    qkv, dout = qkv.cuda(), dout.cuda()
    kw = dict(bias_table=table, nW=nW, win_res=res, shift=shift)
    keep = None
    if c["drop"]:
        kw["dropout"] = (c["drop"], 77, 3)
        keep = attn_keep(77, 3, c["drop"], nseq, nH, 49, "cuda")
    bias = swin_bias(table, nW, res, shift, nseq)
    args = (ATTN_SWIN, nseq, 49, nH, hd, hd ** -0.5)
    bkw, dO, dO_err = {}, dout, None
    if c["proj"]:
        g = torch.Generator().manual_seed(302)
        w = (torch.randn(Cn, Cn, generator=g) * Cn ** -0.5).to(dt).cuda()
        bkw["dout_weight"] = w
        dO = dout.double() @ w.double()                 # the kernel forms dO = dy W per head, rounded to bf16
        # f32 sum over the C inputs (C_ACC 2^-24 sqrt(C)), then dO rounded to bf16 (U_BF16)
        dO_err = (U_BF16 + C_ACC * U32 * math.sqrt(Cn)) * (dout.double().abs() @ w.double().abs())
    ref = AttnRef(qkv, dO, nseq=nseq, L=49, nH=nH, hd=hd, scale=hd ** -0.5, bias=bias, dtype=dt, keep=keep, p=c["drop"],
                  dout_err=dO_err)
    return qkv, dout, args, kw, bkw, ref, None


def _bert_case(ops, c):
    from mvlt_amd._lib import ATTN_BIDIR, ATTN_SEQ2SEQ
    dt, T, nseq, nH = c["dt"], c["T"], c["nseq"], c["nH"]
    n_img, hd = 49, 64
    L = n_img + 2 + T
    lens = c["lens"] or [T, max(1, T // 3), 1][:nseq]
    nseq = len(lens)
    ids = torch.zeros(nseq, T, dtype=torch.long)
    for b, ln in enumerate(lens):
        ids[b, :ln] = 5 + torch.arange(ln)
    im = None
    if c["image_mask"]:
        im = torch.ones(nseq, n_img, dtype=torch.uint8)
        im[:, 0] = 0
        im[1 % nseq, -1] = 0                               # the first and the last image token
    pack = row_index = seq_len = None
    rows = None
    if c["pack"]:
        row_start, seq_len, rows, row_index = pack_layout([n_img + 2 + ln for ln in lens], L)
    qkv, dout = attn_operands(nseq, L, nH, hd, dt, 400 + L, rows=rows, row_index=row_index)
    qkv, dout = qkv.cuda(), dout.cuda()
    mode = ATTN_SEQ2SEQ if c["s2s"] else ATTN_BIDIR
    kw = dict(text_ids=ids.cuda(), obj_end=n_img + 1)
    if im is not None:
        kw["image_mask"] = im.cuda()
    keep = None
    if c["drop"]:
        kw["dropout"] = (c["drop"], 99, 5)
        keep = attn_keep(99, 5, c["drop"], nseq, nH, L, "cuda")
    if c["pack"]:
        pack = (row_start.cuda(), seq_len.cuda(), rows)
        kw["pack"] = pack
    bias = bert_bias(c["s2s"], nseq, L, n_img, ids, im).cuda()
    ref = AttnRef(qkv, dout, nseq=nseq, L=L, nH=nH, hd=hd, scale=0.125, bias=bias, dtype=dt, keep=keep, p=c["drop"],
                  pack=None if pack is None else (row_index, seq_len))
    args = (mode, nseq, L, nH, hd, 0.125)
    bkw = {} if c["delta_ws"] else {"delta_ws": False}
    return qkv, dout, args, kw, bkw, ref, row_index


@pytest.mark.parametrize("c", ROUTES)
def test_attention_route(ops, c):
    qkv, dout, args, kw, bkw, ref, row_index = (_swin_case if c["kind"] == "swin" else _bert_case)(ops, c)
    nseq, L, nH, hd = args[1], args[2], args[3], args[4]
    assert ops.attn_route(qkv, *args, **kw) == c["fwd"]
    assert ops.attn_route(qkv, *args, bwd=True, dout_weight=bkw.get("dout_weight"), delta_ws=bkw.get("delta_ws", True),
                          **kw) == c["bwd"]
    rows = qkv.shape[0]
    out = torch.full((rows, nH * hd), NAN, dtype=qkv.dtype, device=qkv.device)
    lse = torch.full((nseq, nH, L), NAN, dtype=torch.float32, device=qkv.device)
    gap = None if row_index is None else torch.ones(rows, dtype=torch.bool).index_fill_(0, row_index[row_index >= 0], False).cuda()
    if c["fwd"] != "UNSUPPORTED":
        ops.attn_fwd(qkv, *args, out=out, lse=lse, **kw)
        torch.cuda.synchronize()
        kept = out if gap is None else out[~gap]
        check_bound(kept, ref.out, ref.out_b, "out", heads=(hd, nH))
        check_lse(lse, ref)
        assert torch.isnan(lse.cpu()[~torch.isfinite(ref.lse.cpu())]).all(), "lse written at q >= seq_len"
        if gap is not None:
            assert torch.isnan(out[gap]).all(), "a gap row of out was written"
    else:
        kept_rows = torch.arange(rows, device=qkv.device) if gap is None else (~gap).nonzero()[:, 0]
        out[kept_rows] = ref.out.to(qkv.dtype)
        lse.copy_(torch.nan_to_num(ref.lse, nan=0.0).float())
    dqkv = torch.full_like(qkv, NAN)
    dtab = torch.zeros_like(kw["bias_table"]) if "bias_table" in kw else None
    ops.attn_bwd(dout, qkv, out, lse, *args, dbias_table=dtab, dqkv=dqkv, **bkw, **kw)
    torch.cuda.synchronize()
    kept = dqkv if gap is None else dqkv[~gap]
    check_bound(kept, ref.dqkv, ref.dqkv_b, "dqkv", heads=(hd, nH))
    if gap is not None:
        assert torch.isnan(dqkv[gap]).all(), "a gap row of dqkv was written"
    if dtab is not None:
        want, bound = ref.dbias_table()
        check_bound(dtab, want, bound, "dbias_table (row = relative index, column = head)", heads=(1, nH))


# ------------------------------------------------------------------ refusals: unsupported, nothing written
@pytest.mark.parametrize("case", ["bert-L209", "f32-NT11-no-delta", "f32-NT13-no-delta", "swin-hd64"])
def test_attention_refusals_touch_nothing(ops, case):
    from mvlt_amd._lib import ATTN_BIDIR, ATTN_SWIN
    dt = F32 if case.startswith("f32") else BF
    if case == "swin-hd64":
        nH, hd, L, nseq = 2, 64, 49, 4
        kw = dict(bias_table=torch.randn(169, nH, device="cuda"), nW=4, win_res=14, shift=0)
        args = (ATTN_SWIN, nseq, L, nH, hd, hd ** -0.5)
    else:
        T = {"bert-L209": 158, "f32-NT11-no-delta": 110, "f32-NT13-no-delta": 142}[case]
        nH, hd, L, nseq = 2, 64, 51 + T, 2
        ids = torch.ones(nseq, T, dtype=torch.long, device="cuda")
        kw = dict(text_ids=ids, obj_end=50)
        args = (ATTN_BIDIR, nseq, L, nH, hd, 0.125)
    qkv, dout = attn_operands(nseq, L, nH, hd, dt, 500)
    qkv, dout = qkv.cuda(), dout.cuda()
    bkw = {} if case == "bert-L209" or case == "swin-hd64" else {"delta_ws": False}
    assert ops.attn_route(qkv, *args, bwd=True, delta_ws=bkw.get("delta_ws", True), **kw) == "UNSUPPORTED"
    out = torch.full((nseq * L, nH * hd), NAN, dtype=dt, device="cuda")
    lse = torch.full((nseq, nH, L), NAN, device="cuda")
    if case in ("bert-L209", "swin-hd64"):
        assert ops.attn_route(qkv, *args, **kw) == "UNSUPPORTED"
        with pytest.raises(RuntimeError, match="UNSUPPORTED"):
            ops.attn_fwd(qkv, *args, out=out, lse=lse, **kw)
    else:
        out.normal_()
        lse.normal_()
    out0, lse0 = out.clone(), lse.clone()
    dqkv = torch.full_like(qkv, NAN)
    dtab = torch.full((169, nH), NAN, device="cuda") if case == "swin-hd64" else None
    with pytest.raises(RuntimeError, match="UNSUPPORTED"):
        ops.attn_bwd(dout, qkv, out, lse, *args, dqkv=dqkv, dbias_table=dtab, **bkw, **kw)
    torch.cuda.synchronize()
    assert torch.isnan(dqkv).all()
    assert dtab is None or torch.isnan(dtab).all()
    assert torch.equal(out.nan_to_num(7.0), out0.nan_to_num(7.0)) and torch.equal(lse.nan_to_num(7.0), lse0.nan_to_num(7.0))


# ------------------------------------------------------------------ the dropout hash, bit for bit
def test_dropout_mask_equals_host_hash(ops):
    n = 1 << 22
    for seed, tag, p in ((99, 5, 0.1), ((1 << 40) + 12345, 0xFFFFFFFF, 0.37)):
        got = ops.dropout_mask(n, p, seed, tag, torch.device("cuda"))
        want = keep_ref(seed, tag, torch.arange(n, dtype=torch.int64, device="cuda"), p)
        assert torch.equal(got.bool(), want), (seed, tag, p, int((got.bool() != want).sum()))
    # indices near 2^32 - 1 (the top of the uint32 index an attention call may reach)
    n = (1 << 32) - 1
    got = ops.dropout_mask(n, 0.1, 7, 9, torch.device("cuda"))
    tail = torch.arange(n - 4096, n, dtype=torch.int64, device="cuda")
    assert torch.equal(got[-4096:].bool(), keep_ref(7, 9, tail, 0.1))
    del got


# ------------------------------------------------------------------ mvlt_attn_cached (csrc/misc.hip)
# fast path: hd == 64, n_new <= 4, 16-byte aligned; attn_cached_kernel<bf16, 4> when cap > 64 and bf16, else <T, 1>;
# anything else: attn_cached_serial_kernel.  The cache holds NaN beyond `past` before the call; slots [past, past + n_new)
# receive the new K / V bit for bit, every other slot keeps its content.
CACHED = [
    pytest.param(BF, 64, 64, 2, 200, False, id="bf16x4-past64"),        # past ends on a 64-key block
    pytest.param(BF, 64, 65, 3, 200, False, id="bf16x4-past65"),        # one past it
    pytest.param(BF, 64, 127, 4, 202, True, id="bf16x4-past-dev"),      # past_dev, new rows cross into the third block
    pytest.param(BF, 64, 30, 2, 64, False, id="bf16x1-cap64"),          # cap <= 64: <bf16, 1>
    pytest.param(F32, 64, 128, 3, 200, False, id="f32x1-past128"),      # f32: <float, 1>
    pytest.param(F32, 64, 63, 1, 200, True, id="f32x1-past63-dev"),
    pytest.param(BF, 64, 63, 5, 100, False, id="serial-5new"),          # n_new > 4: serial
    pytest.param(F32, 32, 64, 2, 80, False, id="serial-hd32"),          # hd 32: serial
    pytest.param(BF, 32, 65, 1, 80, True, id="serial-hd32-dev"),
]


@pytest.mark.parametrize("dt,hd,past,n_new,cap,dev_past", CACHED)
def test_cached_attention(ops, dt, hd, past, n_new, cap, dev_past):
    from attn_ref import cached_ref
    B, nH = 2, 3
    g = torch.Generator().manual_seed(600 + past + n_new)
    sig = 2.5 ** 0.5
    kc = torch.full((B, nH, cap, hd), NAN, dtype=dt)
    vc = torch.full((B, nH, cap, hd), NAN, dtype=dt)
    kc[:, :, :past] = (torch.randn(B, nH, past, hd, generator=g) * sig).to(dt)
    vc[:, :, :past] = torch.randn(B, nH, past, hd, generator=g).to(dt)
    qkv = torch.randn(B * n_new, 3 * nH * hd, generator=g)
    qkv[:, :2 * nH * hd] *= sig
    qkv, kc, vc = qkv.to(dt).cuda(), kc.cuda(), vc.cuda()
    k0, v0 = kc.clone(), vc.clone()
    ref, bound = cached_ref(qkv, k0, v0, past, hd ** -0.5)
    out = torch.full((B * n_new, nH * hd), NAN, dtype=dt, device="cuda")
    ops.attn_cached(qkv, kc, vc, torch.tensor([past], dtype=torch.int32, device="cuda") if dev_past else past, hd ** -0.5,
                    out=out)
    torch.cuda.synchronize()
    check_bound(out, ref, bound, "cached out", heads=(hd, nH))
    new = qkv.view(B, n_new, 3, nH, hd)
    assert torch.equal(kc[:, :, past:past + n_new], new[:, :, 1].permute(0, 2, 1, 3))
    assert torch.equal(vc[:, :, past:past + n_new], new[:, :, 2].permute(0, 2, 1, 3))
    assert torch.equal(kc[:, :, :past], k0[:, :, :past]) and torch.equal(vc[:, :, :past], v0[:, :, :past])
    assert torch.isnan(kc[:, :, past + n_new:]).all() and torch.isnan(vc[:, :, past + n_new:]).all()


# ------------------------------------------------------------------ fused Swin half, stage by stage
# Each saved output of mvlt_swin_wmsa2_fwd is checked from the kernel's OWN saved input to that stage, so the bounds do
# not compound: xn (LayerNorm of x, window order), qkv (gemm_ref from xn), attention output and lse (AttnRef from qkv),
# y (gemm_ref from the attention output: bias, row scale, window -> token row map, residual).  The backward
# (mvlt_swin_wmsa2_bwd) is checked by AttnRef with dO = dy Wproj (and its bf16 rounding in the bound); the SUM of its
# qkv-dgrad parts by gemm_ref from the kernel's dqkv, plus the bf16 rounding of that dqkv (the parts are formed before it)
# and the bf16 rounding of each part.
WMSA2 = [
    pytest.param(56, 96, 3, 32, True, id="stage0-B32"),
    pytest.param(28, 192, 0, 32, False, id="stage1-B32"),
    pytest.param(14, 384, 3, 32, True, id="stage2-B32"),
    pytest.param(14, 384, 3, 48, False, id="stage2-B48-persistent"),
    pytest.param(14, 384, 0, 3, True, id="stage2-B3"),
]


@pytest.mark.parametrize("res,C_,shift,B,dp", WMSA2)
def test_swin_wmsa2_stage_by_stage(ops, res, C_, shift, B, dp):
    from attn_ref import layernorm_ref
    from gemm_ref import gemm_ref
    from mvlt_amd.indexing import batched_window_maps
    dt = BF
    nH, hd = C_ // 32, 32
    nW = (res // 7) ** 2
    nseq = B * nW
    assert ops.swin_wmsa2_supported(dt, B, res, C_, nH)
    g = torch.Generator().manual_seed(700 + res + B)
    x = torch.randn(B * res * res, C_, generator=g).to(dt).cuda()
    g1 = (1.0 + 0.1 * torch.randn(C_, generator=g)).cuda()
    b1 = (0.1 * torch.randn(C_, generator=g)).cuda()
    # qkv weights scaled so that scale * q.k has std ~2.5, as attn_operands draws it
    wqkv = (torch.randn(3 * C_, C_, generator=g) * C_ ** -0.5)
    wqkv[:2 * C_] *= 2.5 ** 0.5
    wqkv = wqkv.to(dt).cuda()
    bqkv = (0.1 * torch.randn(3 * C_, generator=g)).cuda()
    wproj = (torch.randn(C_, C_, generator=g) * C_ ** -0.5).to(dt).cuda()
    bproj = (0.1 * torch.randn(C_, generator=g)).cuda()
    table = (0.5 * torch.randn(169, nH, generator=g)).cuda()
    rs = (0.25 + torch.arange(B, dtype=torch.float32) % 3).cuda() if dp else None
    scale = hd ** -0.5
    w2n, _ = batched_window_maps(B, res, res, 7, shift, x.device)
    args = (x, w2n, B, res, nH, shift, g1, b1, 1e-5, wqkv, bqkv, wproj, bproj, table, scale)
    y, (xn, qkv, ao, lse, mean, rstd) = ops.swin_wmsa2_fwd(*args, rowscale=rs, save=True)
    torch.cuda.synchronize()
    # xn: LayerNorm of the token row each window row maps to
    xn_ref, xn_b = layernorm_ref(x[w2n.long()], g1, b1, 1e-5)
    check_bound(xn, xn_ref, xn_b, "xn")
    # qkv from the kernel's xn
    q_ref, _, q_b, _, _ = gemm_ref(xn.double(), wqkv.double().t(), out_dtype=dt, bias=bqkv)
    check_bound(qkv, q_ref, q_b, "qkv")
    # attention output and lse from the kernel's qkv
    bias = swin_bias(table, nW, res, shift, nseq)
    aref = AttnRef(qkv, None, nseq=nseq, L=49, nH=nH, hd=hd, scale=scale, bias=bias, dtype=dt)
    check_bound(ao, aref.out, aref.out_b, "attention output", heads=(hd, nH))
    check_lse(lse, aref)
    # y from the kernel's attention output, in token order
    y_ref, _, y_b, rows, _ = gemm_ref(ao.double(), wproj.double().t(), out_dtype=dt, bias=bproj, rowmap=w2n,
                                      rowscale=None if rs is None else (rs, res * res), residual=x)
    check_bound(y[rows], y_ref, y_b, "y")
    # backward of the attention half from the forward's saved qkv / lse
    dy = torch.randn(B * res * res, C_, generator=g).to(dt).cuda()
    dtab = torch.zeros_like(table)
    dqkv, parts = ops.swin_wmsa2_bwd(dy, qkv, lse, B, res, nH, shift, wproj, wqkv, table, scale, dtab)
    torch.cuda.synchronize()
    dO = dy.double() @ wproj.double()
    # f32 sum over the C inputs (C_ACC 2^-24 sqrt(C)), then dO rounded to bf16 (U_BF16)
    dO_err = (U_BF16 + C_ACC * U32 * math.sqrt(C_)) * (dy.double().abs() @ wproj.double().abs())
    bref = AttnRef(qkv, dO, nseq=nseq, L=49, nH=nH, hd=hd, scale=scale, bias=bias, dtype=dt, dout_err=dO_err)
    check_bound(dqkv, bref.dqkv, bref.dqkv_b, "dqkv", heads=(hd, nH))
    want, bound = bref.dbias_table()
    check_bound(dtab, want, bound, "dbias_table (row = relative index, column = head)", heads=(1, nH))
    dxn_ref, _, dxn_b, _, _ = gemm_ref(dqkv.double(), wqkv.double(), out_dtype=F32)
    dxn_b = dxn_b + U_BF16 * (dqkv.double().abs() @ wqkv.double().abs()) + U_BF16 * parts.double().abs().sum(0)
    check_bound(parts.double().sum(0), dxn_ref, dxn_b, "sum of the qkv-dgrad parts")
