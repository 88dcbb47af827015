"""The tail of a cached decode step, kernel by kernel, against float64 references with PER-ELEMENT bounds: the K-split skinny
product (mvlt_gemm_skinny_accum, csrc/skinny.hip gemm_skinny_accum_kernel), the LayerNorm that consumes its slabs
(mvlt_layernorm_acc_fwd, csrc/norm.hip ln_acc_fwd_kernel) and the embedding sum in its cached-step form (mvlt_embed_fwd,
csrc/misc.hip embed_fwd_kernel with n_img = -1).  The whole-model decode tests compare token ids on tiny weights: a defect
in one of these shows there only when it flips an argmax.

Stage by stage (the rule of test_swin_wmsa2_stage_by_stage): the LayerNorm is fed the product kernel's own slabs and its
reference starts from those, so no bound compounds.  Everything a kernel must leave alone holds NaN before the call: operand
padding (lda / ldb beyond K), a guard row behind the slabs and behind y, the gaps of a packed embedding output.
tests/test_decode_tail_bound_cpu.py proves on the host that these bounds accept the kernels' arithmetic at <= 1/2 and reject
the faults the kernels could have.  Every check prints its worst ratio to the bound (pytest -s)."""
import ctypes as C

import pytest
import torch

from attn_ref import layernorm_ref
from gemm_ref import U32, check_bound, gemm_ref

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
NAN = float("nan")
ERR_ARG, ERR_UNSUPPORTED = -1, -3


@pytest.fixture(scope="module")
def ops():
    from mvlt_amd import ops as o
    return o


@pytest.fixture(scope="module")
def L():
    from mvlt_amd import _lib
    return _lib


def _rand(shape, dt, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dt).cuda()


def _padded(vals, pad):
    """[rows, cols] view holding `vals` inside a [rows, cols + pad] buffer whose padding is NaN."""
    rows, cols = vals.shape
    buf = torch.full((rows, cols + pad), NAN, dtype=vals.dtype, device="cuda")
    buf[:, :cols] = vals
    return buf[:, :cols]


def _ratio(out, ref, bound):
    out = out.double()
    r = torch.where(torch.isfinite(out), (out - ref).abs() / bound, torch.full_like(ref, float("inf")))
    return float(r.max()) if r.numel() else 0.0


def _note(request, what, value):
    print(f"BOUND-RATIO {request.node.name} {what} {value:.4f}")


def k_slices(K, kb, k_splits):
    """The slice rule of mvlt_gemm_skinny_accum (include/mvlt_hip.h): [k0, k1) of every slice, in elements."""
    nkb = K // kb
    per = (nkb + k_splits - 1) // k_splits
    return [(min(s * per, nkb) * kb, min((s + 1) * per, nkb) * kb) for s in range(k_splits)]


def _slabs(M, N, k_splits):
    """NaN slabs [k_splits, M, N] with one guard row behind them -> (slabs, guard)."""
    buf = torch.full((k_splits * M + 1, N), NAN, device="cuda")
    return buf[:k_splits * M].view(k_splits, M, N), buf[k_splits * M]


def _accum(L, ops, A, W, acc, k_splits, *, M=None, a_kmajor=0, b_kmajor=0, epilogue=0):
    """mvlt_gemm_skinny_accum on a hand-filled struct; returns the call's answer."""
    p = L.MvltGemm()
    p.dtype, p.M, p.N, p.K = (L.BF16 if A.dtype == BF else L.F32), (A.shape[0] if M is None else M), W.shape[0], A.shape[1]
    p.A, p.lda, p.B, p.ldb = A.data_ptr(), A.stride(0), W.data_ptr(), W.stride(0)
    p.a_kmajor, p.b_kmajor, p.epilogue = a_kmajor, b_kmajor, epilogue
    rc = L.lib().mvlt_gemm_skinny_accum(C.byref(p), C.c_void_p(acc.data_ptr()), k_splits, ops._stream())
    torch.cuda.synchronize()
    return rc


# ===================================================================================================== mvlt_gemm_skinny_accum
ACCUM = [
    # id, dtype, M, N, K, k_splits                      what the row reaches in gemm_skinny_accum_kernel
    ("attn-out-b1", BF, 2, 768, 768, 2),               # decode shapes (decode._SPLITS): one row tile, 2 of 16 rows stored
    ("attn-out-b32", BF, 64, 768, 768, 2),
    ("ffn-out-b1", BF, 2, 768, 3072, 4),               # 24 blocks per slice: one round of 8 waves x 3
    ("ffn-out-b32", BF, 64, 768, 3072, 4),
    ("partial-row-tile", BF, 17, 768, 768, 2),         # 16 i + r15 < M inside the second row tile
    ("n-tail", BF, 33, 772, 768, 2),                   # the last 16-column tile holds 4 columns: clamped weight rows
    ("scalar-tail", BF, 5, 30, 768, 2),                # N % 4 != 0: the scalar tail stores (columns 28, 29)
    ("single-slice", BF, 64, 768, 768, 1),             # 24 blocks, no split
    ("uneven-slices", BF, 64, 768, 768, 5),            # per = 5: slices of 5, 5, 5, 5, 4 blocks (waves 5 .. 7 idle)
    ("one-empty-slice", BF, 64, 768, 768, 7),          # per = 4: six slices of 4, the seventh empty -> exact zeros
    ("many-empty-slices", BF, 64, 768, 768, 64),       # per = 1: 24 slices of one block, forty empty
    ("f32-ffn-out-b32", F32, 64, 768, 3072, 4),        # 48 f32 blocks per slice: two full rounds
    ("f32", F32, 64, 768, 400, 3),                     # f32 k-block = 16: 25 blocks in slices of 9, 9, 7 (a reloaded block)
]


@pytest.mark.parametrize("dt,M,N,K,k_splits", [pytest.param(*c[1:], id=c[0]) for c in ACCUM])
def test_skinny_accum_slabs(ops, L, request, dt, M, N, K, k_splits):
    """Every slab against gemm_ref of the operands restricted to its k-slice (f32 out, no epilogue), the sum of the slabs
    against gemm_ref over the full K within the sum of the slab bounds; an empty slice holds exact zeros; the guard row
    behind the slabs stays NaN; a second run gives the same bits."""
    kb = 32 if dt == BF else 16
    seed = M * 7 + N * 13 + K + k_splits
    A = _padded(_rand((M, K), dt, seed + 1), 8)
    W = _padded(_rand((N, K), dt, seed + 2, K ** -0.5), 8)
    a64, b64 = A.double(), W.double().t()
    acc, guard = _slabs(M, N, k_splits)
    assert _accum(L, ops, A, W, acc, k_splits) == 0
    assert bool(torch.isnan(guard).all()), "guard row behind the slabs written"
    sl = k_slices(K, kb, k_splits)
    assert sl[0][0] == 0 and max(k1 for _, k1 in sl) == K
    bound_sum = torch.zeros(M, N, dtype=torch.float64, device="cuda")
    worst = 0.0
    for s, (k0, k1) in enumerate(sl):
        if k1 <= k0:
            assert bool((acc[s] == 0).all()), f"slab {s}: an empty k-slice must be written as zeros"
            continue
        ref, _, bound, _, _ = gemm_ref(a64[:, k0:k1], b64[k0:k1], out_dtype=F32)
        worst = max(worst, _ratio(acc[s], ref, bound))
        check_bound(acc[s], ref, bound, f"slab {s} (k {k0}..{k1})")
        bound_sum += bound
    _note(request, "slab", worst)
    ref, _, _, _, _ = gemm_ref(a64, b64, out_dtype=F32)
    total = acc.double().sum(0)
    _note(request, "sum", _ratio(total, ref, bound_sum))
    check_bound(total, ref, bound_sum, "sum of the slabs")
    acc2, _ = _slabs(M, N, k_splits)
    assert _accum(L, ops, A, W, acc2, k_splits) == 0
    assert torch.equal(acc, acc2), "two runs differ"


@pytest.mark.parametrize("dt,M,N,K,k_splits", [(BF, 33, 772, 768, 5), (F32, 17, 30, 400, 3)])
def test_skinny_accum_exact(ops, L, dt, M, N, K, k_splits):
    """Small integer operands (|a|, |w| <= 4): every product and partial sum is an integer below 2^24, so nothing rounds --
    each slab IS its slice's product and the slabs add up to the full product, bit for bit, whatever the order."""
    g = torch.Generator().manual_seed(K + k_splits)
    A = _padded(torch.randint(-4, 5, (M, K), generator=g).to(dt).cuda(), 8)
    W = _padded(torch.randint(-4, 5, (N, K), generator=g).to(dt).cuda(), 8)
    a64, b64 = A.double(), W.double().t()
    acc, guard = _slabs(M, N, k_splits)
    assert _accum(L, ops, A, W, acc, k_splits) == 0
    for s, (k0, k1) in enumerate(k_slices(K, 32 if dt == BF else 16, k_splits)):
        want = (a64[:, k0:k1] @ b64[k0:k1]).float()
        assert torch.equal(acc[s], want), f"slab {s} (k {k0}..{k1})"
    total = acc[0].clone()
    for s in range(1, k_splits):
        total += acc[s]
    assert torch.equal(total, (a64 @ b64).float())
    assert bool(torch.isnan(guard).all())


def test_skinny_accum_refusals(ops, L):
    """What the header promises to refuse, with the answer it promises; a refused call writes nothing."""
    M, N, K = 64, 64, 768
    A, W = _rand((M, K), BF, 1), _rand((N, K), BF, 2)
    A65 = _rand((65, K), BF, 3)
    Aodd = _rand((M, K + 16), BF, 4)                  # K = 784: not a multiple of the bf16 k-block
    Wodd = _rand((N, K + 16), BF, 5)
    acc = torch.full((2, 65, N), NAN, device="cuda")
    cases = [
        ("k_splits 0", ERR_ARG, dict(A=A, W=W, k_splits=0)),
        ("k_splits 65", ERR_ARG, dict(A=A, W=W, k_splits=65)),
        ("M 65", ERR_UNSUPPORTED, dict(A=A65, W=W, k_splits=2)),
        ("k-major A", ERR_UNSUPPORTED, dict(A=A, W=W, k_splits=2, a_kmajor=1)),
        ("k-major B", ERR_UNSUPPORTED, dict(A=A, W=W, k_splits=2, b_kmajor=1)),
        ("epilogue", ERR_UNSUPPORTED, dict(A=A, W=W, k_splits=2, epilogue=L.EPI_BIAS)),
        ("K % 32", ERR_UNSUPPORTED, dict(A=Aodd, W=Wodd, k_splits=2)),
    ]
    for name, want, kw in cases:
        a, w, ks = kw.pop("A"), kw.pop("W"), kw.pop("k_splits")
        assert _accum(L, ops, a, w, acc, ks, **kw) == want, name
        assert bool(torch.isnan(acc).all()), f"{name}: a refused call wrote into the slabs"


# ===================================================================================================== mvlt_layernorm_acc_fwd
LN_K = 256          # reduction of the product that makes the slabs: 8 bf16 / 16 f32 k-blocks (nsplit = 8: one / two per slice)
LN_ACC = [
    # id, dtype, rows, C, nsplit, residual, eps         what the row reaches in ln_acc_fwd_kernel
    ("ns1", BF, 64, 768, 1, True, 1e-12),              # NS = 1 / 2 / 4: the slice count at compile time
    ("ns2", BF, 64, 768, 2, True, 1e-12),
    ("ns4", BF, 64, 768, 4, True, 1e-12),
    ("ns3-loop", BF, 5, 768, 3, True, 1e-12),          # NS = 0: the loop; rows % 4 != 0 (a block with one live wave)
    ("ns8-loop", BF, 64, 768, 8, True, 1e-5),
    ("c1024", BF, 2, 1024, 2, True, 1e-12),            # four full 256-column passes; B = 1 decode rows
    ("c2048", BF, 5, 2048, 4, True, 1e-12),            # the maximum: all eight passes
    ("c256-rows130", BF, 130, 256, 3, True, 1e-5),     # one pass; 33 blocks, the last with two live waves
    ("c772", BF, 64, 772, 2, True, 1e-12),             # the fourth pass covers 4 columns (lane 0 alone)
    ("c4", F32, 5, 4, 2, True, 1e-12),                 # one lane of one pass
    ("no-residual", BF, 5, 768, 2, False, 1e-12),      # residual == NULL
    ("f32-ns4", F32, 64, 768, 4, True, 1e-12),
    ("f32-c772-ns8", F32, 2, 772, 8, True, 1e-5),
    ("f32-c2048-no-residual", F32, 130, 2048, 1, False, 1e-5),
]


def _kernel_slabs(L, ops, dt, rows, Cn, nsplit, seed):
    """[nsplit, rows, Cn] f32 slabs made by mvlt_gemm_skinny_accum itself (<= 64 rows per call), copied into one tensor."""
    A = _rand((rows, LN_K), dt, seed + 1)
    W = _rand((Cn, LN_K), dt, seed + 2, LN_K ** -0.5)
    acc = torch.empty((nsplit, rows, Cn), device="cuda")
    for r0 in range(0, rows, 64):
        r1 = min(rows, r0 + 64)
        part = torch.full((nsplit, r1 - r0, Cn), NAN, device="cuda")
        assert _accum(L, ops, A[r0:r1], W, part, nsplit) == 0
        acc[:, r0:r1] = part
    assert bool(torch.isfinite(acc).all())
    return acc


def _ln_acc(L, ops, dt, acc, nsplit, bias, res, gamma, beta, eps, rows, Cn, y):
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)          # noqa: E731
    rc = L.lib().mvlt_layernorm_acc_fwd(L.BF16 if dt == BF else L.F32, p(acc), nsplit, p(bias), p(res), p(gamma), p(beta),
                                        float(eps), rows, Cn, p(y), ops._stream())
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("dt,rows,Cn,nsplit,has_res,eps", [pytest.param(*c[1:], id=c[0]) for c in LN_ACC])
def test_layernorm_acc(ops, L, request, dt, rows, Cn, nsplit, has_res, eps):
    """y against LN(sum_s acc[s] + bias + residual) gamma + beta in float64 (attn_ref.layernorm_ref), the f32 additions that
    form the row entering the bound as dv = (nsplit + 2) 2^-24 (sum_s |acc[s]| + |bias| + |residual|); the guard row
    behind y stays NaN, the slabs are bit-identical after the call (read only), a second run gives the same bits."""
    seed = rows * 7 + Cn * 13 + nsplit
    acc = _kernel_slabs(L, ops, dt, rows, Cn, nsplit, seed)
    bias = _rand((Cn,), F32, seed + 3) + 0.5          # a row mean away from zero
    res = _rand((rows, Cn), dt, seed + 4, 2.0) if has_res else None
    gamma = 1.0 + 0.25 * _rand((Cn,), F32, seed + 5)
    beta = 0.25 * _rand((Cn,), F32, seed + 6)
    ybuf = torch.full((rows + 1, Cn), NAN, dtype=dt, device="cuda")
    keep = acc.clone()
    assert _ln_acc(L, ops, dt, acc, nsplit, bias, res, gamma, beta, eps, rows, Cn, ybuf) == 0
    y = ybuf[:rows]
    assert bool(torch.isnan(ybuf[rows].float()).all()), "guard row behind y written"
    assert torch.equal(acc, keep), "the slabs are read only"
    x = acc.double().sum(0) + bias.double()
    mag = acc.double().abs().sum(0) + bias.double().abs()
    if res is not None:
        x, mag = x + res.double(), mag + res.double().abs()
    ref, bound = layernorm_ref(x, gamma, beta, eps, out_dtype=dt, dv=(nsplit + 2) * U32 * mag)
    _note(request, "y", _ratio(y, ref, bound))
    check_bound(y, ref, bound, "y")
    y2 = torch.full((rows + 1, Cn), NAN, dtype=dt, device="cuda")
    assert _ln_acc(L, ops, dt, acc, nsplit, bias, res, gamma, beta, eps, rows, Cn, y2) == 0
    assert torch.equal(y2[:rows], y), "two runs differ"


def test_layernorm_acc_refusals(ops, L):
    rows = 4
    acc = torch.zeros((2, rows, 2052), device="cuda")
    bias, gamma, beta = (torch.ones(2052, device="cuda") for _ in range(3))
    y = torch.full((rows, 2052), NAN, dtype=BF, device="cuda")
    for name, nsplit, r, Cn in (("nsplit 0", 0, rows, 768), ("nsplit 65", 65, rows, 768), ("C 770", 2, rows, 770),
                                ("C 2052", 2, rows, 2052), ("rows 0", 2, 0, 768)):
        assert _ln_acc(L, ops, BF, acc, nsplit, bias, None, gamma, beta, 1e-12, r, Cn, y) == ERR_ARG, name
        assert bool(torch.isnan(y.float()).all()), f"{name}: a refused call wrote into y"


# ===================================================================================================== mvlt_embed_fwd
EMB_H, EMB_V, EMB_POS = 72, 50, 40          # H / 4 = 18 chunks per row: a 256-thread block spans rows


def _tables():
    g = torch.Generator().manual_seed(90)
    word = torch.randn(EMB_V, EMB_H, generator=g).cuda()
    typ = torch.randn(3, EMB_H, generator=g).cuda()
    # a distinct value per ROW (row r holds r + c / 128, exact in f32): a position off by one cannot cancel
    pos = (torch.arange(EMB_POS, dtype=F32)[:, None] + torch.arange(EMB_H, dtype=F32)[None, :] / 128.0).cuda()
    return word, pos, typ


@pytest.mark.parametrize("dt", [BF, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("B", [1, 32])
@pytest.mark.parametrize("mode", ["host", "device", "both"])
def test_embed_cached_step_bits(ops, L, dt, B, mode):
    """The cached decode step's form (n_img = -1, type_override = 0, two new tokens): out = (word[id] + type[0]) +
    pos[pos_offset + *pos_offset_dev + t], three f32 values added in that order and rounded once -- the same three f32
    operations in torch give the same bits."""
    word, pos, typ = _tables()
    T = 2
    ids = torch.randint(0, EMB_V, (B, T), generator=torch.Generator().manual_seed(B)).cuda()
    ids[B - 1, 1] = EMB_V - 1                          # the last row of the word table
    host_off, dev_off = (7 if mode != "device" else 0), (11 if mode != "host" else 0)
    dev = torch.tensor([dev_off], dtype=torch.int32, device="cuda") if mode != "host" else None
    buf = torch.full((B * T + 1, EMB_H), NAN, dtype=dt, device="cuda")
    p = ops._embed_struct(dt, B, -1, T, EMB_H, ids, word, pos, typ, 101, 102, dev if dev is not None else 0, 0)
    p.pos_offset = host_off
    p.out = C.c_void_p(buf.data_ptr())
    L.check(L.lib().mvlt_embed_fwd(C.byref(p), ops._stream()), "mvlt_embed_fwd")
    torch.cuda.synchronize()
    rows = pos[host_off + dev_off: host_off + dev_off + T]
    want = ((word[ids] + typ[0]) + rows[None]).to(dt).view(B * T, EMB_H)
    assert torch.equal(buf[:B * T], want)
    assert bool(torch.isnan(buf[B * T].float()).all()), "guard row written"


@pytest.mark.parametrize("dt", [BF, F32], ids=["bf16", "f32"])
def test_embed_full_form_bits(ops, dt):
    """[CLS] / image / [SEP] / text, type 1 up to and including the separator and 0 after it, packed rows with NaN gaps."""
    word, pos, typ = _tables()
    B, n_img, T, cls_id, sep_id = 3, 5, 6, 3, EMB_V - 1
    g = torch.Generator().manual_seed(91)
    feat = torch.randn(B, n_img, EMB_H, generator=g).to(dt).cuda()
    ids = torch.randint(0, EMB_V, (B, T), generator=g).cuda()
    lens = [n_img + 2 + t for t in (6, 1, 3)]
    gap, starts, r = 2, [], 0
    for ln in lens:
        r += gap
        starts.append(r)
        r += ln
    total = r + gap
    pack = (torch.tensor(starts, dtype=torch.int32).cuda(), torch.tensor(lens, dtype=torch.int32).cuda(), total)
    out = torch.full((total, EMB_H), NAN, dtype=dt, device="cuda")
    ops.embed_fwd(ids, feat, word, pos, typ, cls_id, sep_id, pack=pack, out=out)
    torch.cuda.synchronize()
    Lq = n_img + 2 + T
    src = torch.cat([word[cls_id].expand(B, 1, EMB_H), feat.float(), word[sep_id].expand(B, 1, EMB_H), word[ids]], 1)
    tt = (torch.arange(Lq, device="cuda") <= n_img + 1).long()
    dense = ((src + typ[tt][None]) + pos[:Lq][None]).to(dt)
    written = torch.zeros(total, dtype=torch.bool, device="cuda")
    for b, (st, ln) in enumerate(zip(starts, lens)):
        assert torch.equal(out[st:st + ln], dense[b, :ln]), f"sample {b}"
        written[st:st + ln] = True
    assert bool(torch.isnan(out[~written].float()).all()), "rows between the packed sequences written"
