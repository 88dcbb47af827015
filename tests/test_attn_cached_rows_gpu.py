"""``mvlt_attn_cached_rows`` / ``mvlt_embed_fwd_rows`` (csrc/misc.hip): the cached decode step for a batch whose rows sit at
different positions.  A row's output is bit for bit the launch without a table on that row alone at its own position, inside
the float64 bound of the cached-attention test; the row's cache receives the new K / V at its own slots and nothing else moves;
an all-zero table is the launch without one; a shift outside the legal range is clamped into the row's cache."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from attn_ref import cached_ref  # noqa: E402
from gemm_ref import check_bound  # noqa: E402

pytestmark = pytest.mark.gpu

F32, BF = torch.float32, torch.bfloat16
NAN = float("nan")
B, NH, HD, N_NEW, CAP, PAST = 3, 4, 64, 2, 96, 70
SHIFTS = [0, -5, -17]          # key counts 72 / 67 / 55: either side of the 64-key block (bf16) and of 32-key blocks (f32)


@pytest.fixture(scope="module")
def ops():
    import mvlt_amd
    return mvlt_amd.ops


def _past_arg(dev_past, past=PAST):
    return torch.tensor([past], dtype=torch.int32, device="cuda") if dev_past else past


def _operands(dt, seed, fill=NAN):
    """qkv of the new rows and caches with data below PAST and ``fill`` behind it.  The caches are the middle rows of a larger
    allocation whose first and last row are guards."""
    g = torch.Generator().manual_seed(seed)
    sig = 2.5 ** 0.5
    kg = torch.full((B + 2, NH, CAP, HD), fill, dtype=dt)
    vg = torch.full((B + 2, NH, CAP, HD), fill, dtype=dt)
    kg[:, :, :PAST] = (torch.randn(B + 2, NH, PAST, HD, generator=g) * sig).to(dt)
    vg[:, :, :PAST] = torch.randn(B + 2, NH, PAST, HD, generator=g).to(dt)
    if fill == fill:          # finite fill: random data everywhere
        kg[:, :, PAST:] = (torch.randn(B + 2, NH, CAP - PAST, HD, generator=g) * sig).to(dt)
        vg[:, :, PAST:] = torch.randn(B + 2, NH, CAP - PAST, HD, generator=g).to(dt)
    qkv = torch.randn(B * N_NEW, 3 * NH * HD, generator=g)
    qkv[:, :2 * NH * HD] *= sig
    return qkv.to(dt).cuda(), kg.cuda(), vg.cuda()


def _same(a, b):
    """Bit equality, NaN slots included."""
    return torch.equal(a.view(torch.int16 if a.dtype == BF else torch.int32), b.view(torch.int16 if b.dtype == BF else torch.int32))


@pytest.mark.parametrize("dev_past", [False, True], ids=["past-host", "past-dev"])
@pytest.mark.parametrize("dt", [F32, BF], ids=["f32", "bf16"])
def test_rows_equal_the_single_row_launch_at_their_own_position(ops, dt, dev_past):
    qkv, kg, vg = _operands(dt, 700)
    k0, v0 = kg.clone(), vg.clone()
    kc, vc = kg[1:B + 1], vg[1:B + 1]
    shift = torch.tensor(SHIFTS, dtype=torch.int32, device="cuda")
    out = torch.full((B * N_NEW, NH * HD), NAN, dtype=dt, device="cuda")
    ops.attn_cached(qkv, kc, vc, _past_arg(dev_past), HD ** -0.5, out=out, row_shift=shift)
    torch.cuda.synchronize()
    new = qkv.view(B, N_NEW, 3, NH, HD)
    for b, s in enumerate(SHIFTS):
        pb = PAST + s
        kb, vb = k0[1 + b:2 + b].clone(), v0[1 + b:2 + b].clone()
        rows = slice(b * N_NEW, (b + 1) * N_NEW)
        want = ops.attn_cached(qkv[rows].contiguous(), kb, vb, _past_arg(dev_past, pb), HD ** -0.5)
        assert _same(out[rows], want), (b, float((out[rows].float() - want.float()).abs().max()))
        ref, bound = cached_ref(qkv[rows], k0[1 + b:2 + b], v0[1 + b:2 + b], pb, HD ** -0.5)
        check_bound(out[rows], ref, bound, f"rows out, row {b}", heads=(HD, NH))
        # the row's cache: the new K / V at its own two slots, every other slot as before (the single-row launch wrote the same)
        assert torch.equal(kc[b, :, pb:pb + N_NEW], new[b, :, 1].permute(1, 0, 2))
        assert torch.equal(vc[b, :, pb:pb + N_NEW], new[b, :, 2].permute(1, 0, 2))
        assert _same(kc[b:b + 1], kb) and _same(vc[b:b + 1], vb)
        keep = torch.ones(CAP, dtype=torch.bool, device="cuda")
        keep[pb:pb + N_NEW] = False
        assert _same(kc[b][:, keep], k0[1 + b][:, keep]) and _same(vc[b][:, keep], v0[1 + b][:, keep])
    for guard in (0, B + 1):
        assert _same(kg[guard], k0[guard]) and _same(vg[guard], v0[guard])


@pytest.mark.parametrize("dt", [F32, BF], ids=["f32", "bf16"])
def test_zero_shifts_equal_the_launch_without_a_table(ops, dt):
    qkv, kg, vg = _operands(dt, 701)
    ka, va, kb, vb = kg[1:B + 1].clone(), vg[1:B + 1].clone(), kg[1:B + 1].clone(), vg[1:B + 1].clone()
    zero = torch.zeros(B, dtype=torch.int32, device="cuda")
    got = ops.attn_cached(qkv, ka, va, PAST, HD ** -0.5, row_shift=zero)
    want = ops.attn_cached(qkv, kb, vb, PAST, HD ** -0.5)
    torch.cuda.synchronize()
    assert _same(got, want) and _same(ka, kb) and _same(va, vb)


@pytest.mark.parametrize("dt", [F32, BF], ids=["f32", "bf16"])
def test_a_shift_outside_the_range_is_clamped_into_the_rows_cache(ops, dt):
    """Shifts far beyond either end: the row lands at position 0 or at cache_cap - n_new (a defined result: that of the
    single-row launch there), writes its two slots and nothing else; the neighbouring rows and the guards keep every bit."""
    qkv, kg, vg = _operands(dt, 702, fill=0.5)
    k0, v0 = kg.clone(), vg.clone()
    kc, vc = kg[1:B + 1], vg[1:B + 1]
    shifts = [2 ** 31 - 1, -2 ** 31, -17]
    landed = [CAP - N_NEW, 0, PAST - 17]
    out = ops.attn_cached(qkv, kc, vc, PAST, HD ** -0.5, row_shift=torch.tensor(shifts, dtype=torch.int32, device="cuda"))
    torch.cuda.synchronize()
    for b, pb in enumerate(landed):
        kb, vb = k0[1 + b:2 + b].clone(), v0[1 + b:2 + b].clone()
        rows = slice(b * N_NEW, (b + 1) * N_NEW)
        want = ops.attn_cached(qkv[rows].contiguous(), kb, vb, pb, HD ** -0.5)
        assert _same(out[rows], want), b
        assert _same(kc[b:b + 1], kb) and _same(vc[b:b + 1], vb)
        keep = torch.ones(CAP, dtype=torch.bool, device="cuda")
        keep[pb:pb + N_NEW] = False
        assert _same(kc[b][:, keep], k0[1 + b][:, keep]) and _same(vc[b][:, keep], v0[1 + b][:, keep])
    for guard in (0, B + 1):
        assert _same(kg[guard], k0[guard]) and _same(vg[guard], v0[guard])


def test_refusals(ops):
    import ctypes as C
    from mvlt_amd import _lib as L
    qkv, kg, vg = _operands(F32, 703)
    kc, vc = kg[1:B + 1], vg[1:B + 1]
    shift = torch.zeros(B, dtype=torch.int32, device="cuda")
    with pytest.raises(RuntimeError, match="MVLT_ERR_ARG"):          # past + n_new beyond the cache, known on the host
        ops.attn_cached(qkv, kc, vc, CAP - 1, HD ** -0.5, row_shift=shift)
    p = L.MvltAttnCached()
    p.dtype, p.B, p.nH, p.hd, p.n_new, p.cache_cap, p.past = L.F32, B, NH, HD, N_NEW, CAP, PAST
    out = torch.empty((B * N_NEW, NH * HD), device="cuda")
    p.qkv_new, p.k_cache, p.v_cache, p.out, p.scale = qkv.data_ptr(), kc.data_ptr(), vc.data_ptr(), out.data_ptr(), 0.125
    lib = L.lib()
    err = {v: k for k, v in L.ERRORS.items()}
    assert lib.mvlt_attn_cached_rows(C.byref(p), None, None) == err["MVLT_ERR_ARG"]          # no table
    p.hd = 32
    assert lib.mvlt_attn_cached_rows(C.byref(p), shift.data_ptr(), None) == err["MVLT_ERR_UNSUPPORTED"]          # no serial form
    p.hd, p.n_new = 64, 5
    assert lib.mvlt_attn_cached_rows(C.byref(p), shift.data_ptr(), None) == err["MVLT_ERR_UNSUPPORTED"]
    torch.cuda.synchronize()
    assert _same(kg, _operands(F32, 703)[1])          # nothing was launched


# ------------------------------------------------------------------ mvlt_embed_fwd_rows
def _tables(seed, V=500, H=256, P=128):
    g = torch.Generator().manual_seed(seed)
    word, pos, typ = torch.randn(V, H, generator=g), torch.randn(P, H, generator=g), torch.randn(2, H, generator=g)
    ids = torch.randint(1, V, (B, 2), generator=g)
    return ids.cuda(), word.cuda(), pos.cuda(), typ.cuda()


@pytest.mark.parametrize("dev_past", [False, True], ids=["pos-host", "pos-dev"])
@pytest.mark.parametrize("dt", [F32, BF], ids=["f32", "bf16"])
def test_embed_rows_equal_the_single_row_launch_at_their_own_position(ops, dt, dev_past):
    ids, word, pos, typ = _tables(710)
    shift = torch.tensor(SHIFTS, dtype=torch.int32, device="cuda")
    kw = dict(dtype=dt, type_override=0)
    got = ops.embed_fwd(ids, None, word, pos, typ, 101, 102, pos_offset=_past_arg(dev_past), row_shift=shift, **kw)
    assert got.shape == (B, 2, 256) and got.dtype == dt
    for b, s in enumerate(SHIFTS):
        want = ops.embed_fwd(ids[b:b + 1].contiguous(), None, word, pos, typ, 101, 102, pos_offset=_past_arg(dev_past, PAST + s), **kw)
        assert _same(got[b:b + 1], want), b
        ref = (word[ids[b]] + typ[0] + pos[PAST + s:PAST + s + 2]).to(dt)          # f32 sums in the kernel's order
        assert _same(got[b], ref), b
    zero = torch.zeros(B, dtype=torch.int32, device="cuda")
    a = ops.embed_fwd(ids, None, word, pos, typ, 101, 102, pos_offset=_past_arg(dev_past), row_shift=zero, **kw)
    assert _same(a, ops.embed_fwd(ids, None, word, pos, typ, 101, 102, pos_offset=_past_arg(dev_past), **kw))


def test_embed_shift_outside_the_table_is_clamped(ops):
    ids, word, pos, typ = _tables(711)
    shift = torch.tensor([2 ** 31 - 1, -2 ** 31, 0], dtype=torch.int32, device="cuda")
    got = ops.embed_fwd(ids, None, word, pos, typ, 101, 102, dtype=F32, pos_offset=PAST, type_override=0, row_shift=shift)
    torch.cuda.synchronize()
    assert _same(got[0], word[ids[0]] + typ[0] + pos[127:128])          # both tokens at the last row of the table
    assert _same(got[1], word[ids[1]] + typ[0] + pos[0:1])              # both at the first
    assert _same(got[2], word[ids[2]] + typ[0] + pos[PAST:PAST + 2])
