"""Every mvlt_gemm dispatch route (csrc/gemm.hip: choose_plan, gemm_dispatch) against the float64 reference of
tests/gemm_ref.py with a PER-ELEMENT bound, not a relative norm over the whole output.

Each row of ROUTES names the kernel it targets and the gemm_dispatch condition that sends it there, and asserts the
planner's (bm, bn, split) first: a planner change that moves a shape off its route fails here and the row gets
re-pointed instead of quietly testing another kernel (the plan does not say LDS-DMA vs register-staged, or wide vs
narrow epilogue: the comment does; rows with route= also assert mvlt_gemm_route's answer for the same struct, so a row
pointed at the wrong kernel fails there and does not pass on another kernel's arithmetic).  Every run also checks what
the kernel must leave alone, pre-filled with NaN: the padding columns N..ldc, a guard row behind the output, and the
rows at or beyond a row-major A's device-side row count (m_dev) -- every route here promises that.  Operand padding
(lda / ldb beyond the extent) and the operand rows beyond m_dev hold NaN too: the kernel must not use them."""
import ctypes as C

import pytest
import torch

from gemm_ref import check_bound, colsum_ref, gemm_ref, logical

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
RD = 301                     # labelled rows of a B = 32, T = 80 step (the MLM head's m_dev): inside the fifth 64-row tile


def R(id, dt, M, N, K, ak=False, bk=False, pad=(0, 0, 0), epi=(), split=0, mdev=None, plan=None, route=None):
    """pad: extra elements per row of A / B / C storage (lda, ldb, ldc beyond the extent); epi: subset of bias, gelu
    (+ saved pre-activation), gelu_nopre (GELU alone: what the cached decode step issues for FFN-in), dropout, rowscale,
    rowmap, aux (x gelu'), residual, f32 (output), accum, colsum;
    mdev: None or the device-side row count (a row-major A's rows, a k-major A's reduction);
    route: None or the name (_lib.GEMM_ROUTES) mvlt_gemm_route must answer for the filled struct, with plan[2] k-slices."""
    return pytest.param(dict(dt=dt, M=M, N=N, K=K, ak=ak, bk=bk, pad=pad, epi=set(epi), split=split, mdev=mdev,
                             plan=plan, route=route), id=id)


SK = dict(plan=(64, 16, 1), route="SKINNY")          # what mvlt_gemm_plan / mvlt_gemm_route answer for a skinny product


ROUTES = [
    # ---- LDS-DMA loop, gemm_glds_kernel (bf16, row-major A, K % 64 == 0, lda / ldb % 8 == 0, bm in {64, 160});
    #      d.wide (N % 8 == 0 and ldc % 8 == 0, bn != 96, no split / f32 / accumulate) picks the 16-byte epilogue
    # 64x128, row-major B: N >= 2304 and K <= 1024 turn 128x128 into 64x128; 32 x 24 tiles >= 512 keep BN = 128
    R("glds64x128-wide", BF, 2000, 3072, 768, epi=("bias", "gelu"), plan=(64, 128, 1)),
    R("glds64x128-narrow", BF, 2000, 3072, 768, pad=(0, 0, 4), epi=("bias", "dropout", "residual"), mdev=1500,
      plan=(64, 128, 1)),                                                     # ldc % 8 == 4: tile_epilogue (8 bytes)
    # 64x96: N % 96 == 0, N % 64 != 0 (the forward 64x64 rule needs N % 64 == 0); bn == 96 is never wide
    R("glds64x96", BF, 3000, 480, 320, epi=("bias", "gelu", "rowscale", "residual"), plan=(64, 96, 1)),
    R("glds64x96-epi4", BF, 3000, 480, 320, pad=(0, 0, 2), epi=("bias", "rowmap"), mdev=2049,
      plan=(64, 96, 1)),                                                      # ldc % 4 != 0: epilogue4 per quad
    # 64x64, row-major B: forward rule (N % 64 == 0, M <= 8192, K <= 768, N <= 2304); K < 768: two LDS stages
    R("glds64x64-wide", BF, 1500, 768, 512, epi=("bias", "dropout"), mdev=1472, plan=(64, 64, 1)),   # m_dev on a tile boundary
    R("glds64x64-narrow", BF, 1500, 768, 512, pad=(8, 0, 4), epi=("bias", "residual"), plan=(64, 64, 1)),
    # three LDS stages: 64x64, row-major B, wide, K span >= 768, <= 400 tiles (24 x 12 here)
    R("glds64x64-3stage", BF, 1500, 768, 768, epi=("bias", "gelu"), mdev=1000, plan=(64, 64, 1)),
    R("glds64x64-3stage-k1536", BF, 1500, 768, 1536, epi=("bias", "residual"), plan=(64, 64, 1)),    # 64x128 -> 64x64 (< 512 tiles)
    R("glds64x64-k768-narrow", BF, 1500, 768, 768, pad=(0, 0, 4), epi=("bias", "gelu"), plan=(64, 64, 1)),  # 3 stages need wide: 2
    # k-major B (dgrad), N % 8 == 0, bn in {64, 128}: gemm_glds_kernel<64, BN, true>
    R("glds64x128-bk-wide", BF, 2000, 1000, 512, bk=True, epi=("aux",), plan=(64, 128, 1)),  # N % 64 != 0 keeps BN = 128
    R("glds64x128-bk-narrow", BF, 2000, 1000, 512, bk=True, pad=(0, 8, 4), epi=("residual",), mdev=777, plan=(64, 128, 1)),
    R("glds64x64-bk-wide", BF, 1500, 768, 512, bk=True, epi=("residual",), plan=(64, 64, 1)),     # 64x128 -> 64x64 (< 512 tiles)
    R("glds64x64-bk-narrow", BF, 1500, 768, 512, bk=True, pad=(0, 0, 4), epi=("aux",), mdev=64, plan=(64, 64, 1)),
    # 160x128 (forward only, wide only): 340 < 20 x 24 tiles <= 512 ...
    R("glds160x128", BF, 3150, 3072, 768, epi=("bias", "gelu"), plan=(160, 128, 1)),
    # ... and up to 680 launched tiles with m_dev (27 x 24 = 648; without m_dev the same shape is not 160-row)
    R("glds160x128-mdev", BF, 4192, 3072, 768, epi=("bias", "dropout", "residual"), mdev=3001, plan=(160, 128, 1)),
    # ---- register-staged gemm_kernel (launch_layout): bm == 128, K % 64 != 0, lda % 8 != 0, k-major A or f32
    # 128x128: >= 384 tiles of 128x128, N < 2304, K > 768 (no 64-row rules), 19 x 16 <= 340 tiles of 160 rows
    R("reg128x128-wide", BF, 3000, 2048, 1024, epi=("bias", "gelu"), plan=(128, 128, 1)),
    R("reg128x128-ktail", BF, 3000, 2048, 1000, pad=(0, 0, 4), epi=("residual",), mdev=2500, plan=(128, 128, 1)),
    # 128x96: N % 96 == 0, N % 128 != 0, 32 x 13 >= 384 tiles; bn 96: tile_epilogue
    R("reg128x96", BF, 4000, 1248, 384, epi=("bias", "residual"), plan=(128, 96, 1)),
    # 64-row tiles on the register-staged kernels, all four layouts
    R("reg64x96-ktail", BF, 3000, 480, 200, epi=("bias",), plan=(64, 96, 1)),                     # K % 64 != 0: not LDS-DMA
    R("reg64x128-lda", BF, 2000, 1000, 512, bk=True, pad=(4, 0, 0), epi=("aux",), plan=(64, 128, 1)),  # lda % 8 != 0: no a_vec
    R("reg64x128-ak-bk", BF, 600, 520, 700, ak=True, bk=True, epi=("f32", "colsum"), plan=(64, 128, 1)),
    R("reg64x128-ak", BF, 600, 520, 700, ak=True, epi=("bias",), plan=(64, 128, 1)),
    # k-major A whose extent is not a multiple of 8 behind a padded lda (lda % 8 == 0: the fast, unpredicated loads)
    R("reg64x128-ak-ragged", BF, 601, 520, 700, ak=True, bk=True, pad=(7, 0, 0), epi=("f32", "colsum"), plan=(64, 128, 1)),
    # k-major B whose extent is not a multiple of 8 behind a padded ldb (K % 64 != 0: register-staged; lda % 8 == 0: fast loads)
    R("reg64x128-bk-ragged", BF, 600, 250, 712, bk=True, pad=(0, 6, 2), epi=("bias",), plan=(64, 128, 1)),
    # f32: register-staged only
    R("f32-reg128x128", F32, 3000, 2048, 1024, epi=("bias", "gelu"), plan=(128, 128, 1)),
    R("f32-reg64x96-bk", F32, 1000, 288, 200, bk=True, epi=("aux",), mdev=999, plan=(64, 96, 1)),
    R("f32-reg64x64-ak-ragged", F32, 333, 384, 200, ak=True, pad=(3, 0, 0), epi=("accum",), plan=(64, 64, 1)),
    R("f32-reg64x64-akbk", F32, 77, 30, 50, ak=True, bk=True, plan=(64, 64, 1)),
    # ---- split-K: slabs in the workspace, splitk_reduce_kernel applies the epilogue
    # row-major A and B on the LDS-DMA loop (K span 1024 % 64 == 0), vector reduce; bias + residual in the reduce
    R("split-glds-rr", BF, 500, 768, 4096, split=4, epi=("bias", "residual"), plan=(64, 64, 4)),
    # row-major A, k-major B on LDS-DMA; bias + GELU + saved pre-activation in the reduce; m_dev on a tile boundary
    R("split-glds-rk", BF, 500, 768, 4096, bk=True, split=3, epi=("bias", "gelu"), mdev=128, plan=(64, 64, 3)),
    # k-major A (weight gradient), f32 out, column sums through the colsum slabs
    R("split-akbk-colsum", BF, 384, 192, 5000, ak=True, bk=True, split=5, epi=("f32", "colsum"), plan=(64, 96, 5)),
    R("split-akbk-accum", BF, 384, 192, 5000, ak=True, bk=True, split=5, epi=("f32", "accum", "colsum"), plan=(64, 96, 5)),
    R("split-ak-rowB", BF, 384, 192, 5000, ak=True, split=5, epi=("f32",), plan=(64, 96, 5)),
    # k-major A with m_dev limiting the reduction: slice 4 ends inside it, slice 5 is empty
    R("split-akbk-mdev", BF, 384, 192, 5000, ak=True, bk=True, split=5, epi=("f32", "colsum"), mdev=3333, plan=(64, 96, 5)),
    R("split-akbk-mdev0", BF, 384, 192, 5000, ak=True, bk=True, split=5, epi=("f32", "colsum", "bias"), mdev=0, plan=(64, 96, 5)),
    # auto split: < 200 tiles, >= 16 k-tiles -> min(ceil(768 / tiles), nkt / 8); the last slice partial
    R("split-auto-akbk", BF, 768, 192, 6000, ak=True, bk=True, epi=("f32", "colsum"), plan=(64, 96, 11)),
    R("split-auto-rr", BF, 256, 256, 8192, epi=("bias",), plan=(64, 64, 16)),
    # N % 4 != 0: the scalar slab writes and the scalar reduce branch
    R("split-scalar-akbk", BF, 200, 150, 3000, ak=True, bk=True, split=4, epi=("f32", "colsum"), plan=(64, 128, 4)),
    R("split-scalar-rr", BF, 300, 150, 3000, split=3, pad=(0, 0, 2), epi=("bias", "residual"), mdev=257, plan=(64, 128, 3)),
    # empty trailing splits dropped: 10 k-tiles over 8 requested slices = 5 slices of 2
    R("split-dropped", BF, 300, 256, 640, split=8, epi=("bias",), plan=(64, 64, 8)),
    R("f32-split-rk", F32, 300, 256, 1000, bk=True, split=3, epi=("bias",), mdev=RD, plan=(64, 64, 3)),
    # m_dev >= M and m_dev == 0 on a row-major A
    R("glds64x64-mdev-big", BF, 1500, 768, 512, epi=("bias",), mdev=4000, plan=(64, 64, 1)),
    R("glds64x64-mdev0", BF, 1500, 768, 512, epi=("bias",), mdev=0, plan=(64, 64, 1)),
    # ---- the MLM head of a B = 32, T = 80 step (model.py: _logits, _backward_from_dlogits) at its exact arguments
    # decoder forward: N = 30522 (N % 4 != 0: epilogue4), ldc = 30528, m_dev; gemm_glds_kernel<64, 128, false, false>
    R("mlm-decoder-fwd", BF, 2560, 30522, 768, pad=(0, 0, 6), epi=("bias",), mdev=RD, plan=(64, 128, 1)),
    # decoder dgrad: dl = dlogits[:, :30522] (K % 64 != 0, lda = 30528), k-major W, split 8: register-staged 64x64
    R("mlm-decoder-dgrad", BF, 2560, 768, 30522, bk=True, pad=(6, 0, 0), split=8, mdev=RD, plan=(64, 64, 8)),
    # decoder weight gradient: both k-major, f32 out, a_colsum, m_dev = reduction; ragged last row tile (30522 % 128)
    R("mlm-decoder-wgrad", BF, 30522, 768, 2560, ak=True, bk=True, pad=(6, 0, 0), epi=("f32", "colsum"), mdev=RD,
      plan=(128, 128, 1)),
    # ---- arms of the tile epilogues (csrc/gemm_dev.h) the rows above do not reach: the row map (the Swin projection scatter)
    #      through tile_epilogue_wide and tile_epilogue, and the in-place accumulate of a bf16 output through tile_epilogue.
    #      Three row tiles of 64 with a partial last row block (150 = 2 x 64 + 16 + 6: the clamped rows are read); forward
    #      rule -> 64 x 64 tiles, 2 k-tiles: no k-slices.  (wide = N % 8 == 0 and ldc % 8 == 0, as in the first block above)
    R("glds64x64-wide-rowmap", BF, 150, 256, 128, epi=("bias", "rowscale", "residual", "rowmap"), plan=(64, 64, 1), route="GLDS"),
    R("glds64x64-narrow-rowmap", BF, 150, 192, 128, pad=(0, 0, 4), epi=("bias", "rowscale", "rowmap"), plan=(64, 64, 1),
      route="GLDS"),                                                          # ldc % 8 == 4: 8 bytes per lane
    R("reg64x64-accum", BF, 150, 192, 96, epi=("bias", "accum"), plan=(64, 64, 1), route="REG"),   # K % 64 != 0: register-staged
    # ---- gemm_skinny_kernel<T, false> (csrc/skinny.hip; gemm_host.h is_skinny + skinny_loads_ok: M <= 64, both operands
    #      k-contiguous, K % k-block == 0 (32 in bf16, 16 in f32), no split, lda / ldb % 8 (f32: 4) == 0, 16-byte aligned).
    #      A workgroup = 16 columns x all rows; 8 waves x 3 k-blocks in flight; fast_epi = only bias / GELU / residual bits,
    #      epi_vec and a whole 16-column tile, per lane a row < M: pre-fetched operands; everything else through epilogue4.
    # the products of a cached decode step (decode._layers_cached) at B = 1 and B = 32 (2 new tokens per sample)
    R("skinny-qkv-b1", BF, 2, 2304, 768, epi=("bias",), **SK),                       # one row tile, 2 of 16 rows live
    R("skinny-qkv-b32", BF, 64, 2304, 768, epi=("bias",), **SK),
    R("skinny-ffn-in-b1", BF, 2, 3072, 768, epi=("bias", "gelu_nopre"), **SK),         # the only GELU fast_epi takes
    R("skinny-attn-out-b32", BF, 64, 768, 768, epi=("bias", "residual"), **SK),
    R("skinny-ffn-out-b32", BF, 64, 768, 3072, epi=("bias", "residual"), **SK),        # 96 k-blocks: four full rounds of 8 x 3
    R("skinny-f32-ffn-out-b32", F32, 64, 768, 3072, epi=("bias", "residual"), **SK),   # the exact-f32 decode: 192 k-blocks
    # k-loop edges
    R("skinny-k32", BF, 16, 64, 32, epi=("bias", "gelu_nopre", "residual"), **SK),     # one k-block: seven waves add zeros
    R("skinny-k800", BF, 17, 64, 800, **SK),       # 25 blocks: round 2 = block 24 live + two reloaded (wave 0); no epilogue
    R("skinny-f32-k16", F32, 1, 64, 16, epi=("bias", "residual"), **SK),               # f32 k-block = 16; M = 1
    R("skinny-f32-k400", F32, 49, 96, 400, epi=("bias", "gelu"), **SK),                # 25 f32 blocks; GELU + pre: epilogue4
    # row-tile edges: M = 1 (f32 above), 16 (k32), 17 (k800), 49; m_dev inside a 16-row tile, 0, beyond M
    R("skinny-m1", BF, 1, 768, 768, epi=("bias", "gelu_nopre"), **SK),
    R("skinny-m49-rowmap", BF, 49, 768, 768, epi=("bias", "rowscale", "rowmap"), **SK),   # epilogue4, last tile 1 row
    R("skinny-mdev37", BF, 64, 768, 768, epi=("bias", "residual"), mdev=37, **SK),     # fast_epi per lane: rows 32..36 of tile 2
    R("skinny-mdev0", BF, 64, 768, 768, epi=("bias",), mdev=0, **SK),                  # nothing written
    R("skinny-mdev-big", BF, 33, 768, 768, epi=("bias", "dropout"), mdev=100, **SK),
    # column edges: fast_epi off for the whole launch or for the last tile only
    R("skinny-n30", BF, 33, 30, 64, epi=("bias", "residual"), **SK),                   # N % 4 != 0: scalar stores, 2 tiles
    R("skinny-n2-classifier", BF, 5, 2, 768, epi=("bias",), **SK),
    R("skinny-ldc-pad2", BF, 64, 768, 768, pad=(0, 0, 2), epi=("bias", "gelu"), **SK),   # ldc % 4 != 0: epi_vec false
    R("skinny-n776", BF, 33, 776, 768, epi=("bias", "gelu_nopre", "residual"), **SK),  # 48 fast tiles + one of 8 columns
    # the remaining epilogue bits at M <= 64 (epilogue4): GELU + saved pre-activation with vector stores (and a last tile
    # of 8 columns), x gelu'(aux), accumulate, f32 output
    R("skinny-gelu-pre", BF, 32, 3000, 256, epi=("bias", "gelu"), **SK),
    R("skinny-aux-accum", BF, 49, 96, 64, epi=("aux", "accum"), **SK),
    R("skinny-f32out-accum", BF, 33, 100, 96, epi=("bias", "f32", "accum"), **SK),
    # strided A: the pooler's hidden[:, 0] of a [B, L, H] tensor with L = 3 (lda = 3 K), NaN in the gap
    R("skinny-pooler-strided", BF, 32, 768, 768, pad=(2 * 768, 0, 0), epi=("bias",), **SK),
    R("skinny-f32-strided", F32, 5, 2, 768, pad=(2 * 768, 0, 0), epi=("bias", "residual"), **SK),
    # ---- M <= 64 that is NOT skinny: the tile kernels at a single, mostly empty row tile
    R("short-ktail-reg", BF, 33, 768, 200, epi=("bias",), plan=(64, 64, 1), route="REG"),          # K % 32 != 0
    # lda % 8 != 0: is_skinny holds (the plan says 64 x 16) but skinny_loads_ok does not: register-staged 64 x 64
    R("short-lda-reg", BF, 33, 768, 768, pad=(4, 0, 0), epi=("bias", "residual"), plan=(64, 16, 1), route="REG"),
    R("short-bk-glds", BF, 33, 768, 768, bk=True, epi=("aux",), plan=(64, 64, 1), route="GLDS"),   # k-major B
    R("short-split2-glds", BF, 33, 768, 768, split=2, epi=("bias",), plan=(64, 64, 2), route="GLDS"),   # split_k = 2
]


@pytest.fixture(scope="module")
def ops():
    from mvlt_amd import ops as o
    return o


def _rand(shape, dt, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dt).cuda()


def _plan(L, ops, dt, M, N, K, A, B, out, *, ak, bk, split, epi_bits, m_dev, colsum, res, pre, aux, bias, rowscale=None,
          rowmap=None, drop_p=0.0, want_route=False):
    """mvlt_gemm_plan on the struct ops.gemm fills (the fields the planner reads) and, when asked, mvlt_gemm_route on the
    same struct (the dispatch itself in its no-launch mode): ((bm, bn, split), (route name, k-slices) or None)."""
    q = L.MvltGemm()
    q.dtype, q.M, q.N, q.K = (L.BF16 if dt == BF else L.F32), M, N, K
    q.A, q.lda = A.data_ptr(), A.stride(0)
    q.B, q.ldb = B.data_ptr(), B.stride(0)
    q.C, q.ldc = out.data_ptr(), out.stride(0)
    q.a_kmajor, q.b_kmajor, q.split_k, q.epilogue = int(ak), int(bk), split, epi_bits
    q.m_dev = m_dev.data_ptr() if m_dev is not None else None
    q.a_colsum = colsum.data_ptr() if colsum is not None else None
    if res is not None:
        q.residual, q.ldr = res.data_ptr(), res.stride(0)
    q.pre = pre.data_ptr() if pre is not None else None
    q.aux = aux.data_ptr() if aux is not None else None
    q.bias = bias.data_ptr() if bias is not None else None
    if rowscale is not None:
        q.rowscale, q.rows_per_scale = rowscale[0].data_ptr(), rowscale[1]
    q.rowmap = rowmap.data_ptr() if rowmap is not None else None
    q.dropout_p = drop_p
    bm, bn, sp = C.c_int(), C.c_int(), C.c_int()
    assert L.lib().mvlt_gemm_plan(C.byref(q), C.byref(bm), C.byref(bn), C.byref(sp)) == 0
    route = None
    if want_route:
        need = L.lib().mvlt_gemm_workspace_bytes(C.byref(q))
        if need:
            ws = ops.workspace("gemm", need, A.device)
            q.workspace, q.workspace_bytes = ws.data_ptr(), ws.numel()
        route = L.gemm_route_name(L.lib().mvlt_gemm_route(C.byref(q)))
    return (bm.value, bn.value, sp.value), route


def _note(request, what, out, ref, bound):
    """Print the worst ratio to the bound (pytest -s shows it; a correct kernel sits at <= 0.5 of the f32 terms, while
    the rounding of a bf16 output alone reaches U_OUT |ref| by construction)."""
    if ref.numel():
        o = out.double()
        ratio = torch.where(torch.isfinite(o), (o - ref).abs() / bound, torch.full_like(ref, float("inf")))
        print(f"BOUND-RATIO {request.node.name} {what} {float(ratio.max()):.4f}")


def _padded(rows, cols, pad, dt, seed, scale=1.0):
    """[rows, cols] view of a [rows, cols + pad] buffer whose padding holds NaN."""
    buf = torch.full((rows, cols + pad), float("nan"), dtype=dt, device="cuda")
    buf[:, :cols] = _rand((rows, cols), dt, seed, scale)
    return buf[:, :cols]


@pytest.mark.parametrize("r", ROUTES)
def test_gemm_route(ops, r, request):
    from mvlt_amd import _lib as L
    dt, M, N, K, ak, bk, epi, mdev = r["dt"], r["M"], r["N"], r["K"], r["ak"], r["bk"], r["epi"], r["mdev"]
    pa, pb, pc = r["pad"]
    seed = M * 7 + N * 13 + K
    A = _padded(K, M, pa, dt, seed + 1) if ak else _padded(M, K, pa, dt, seed + 1)
    B = _padded(K, N, pb, dt, seed + 2, K ** -0.5) if bk else _padded(N, K, pb, dt, seed + 2, K ** -0.5)
    a64, b64 = logical(A, B, ak, bk)
    m_dev = None if mdev is None else torch.tensor([mdev], dtype=torch.int32, device="cuda")
    k_eff = min(max(mdev, 0), K) if (mdev is not None and ak) else None
    m_eff = min(max(mdev, 0), M) if (mdev is not None and not ak) else M
    # operand rows beyond the device-side count are stale in the model (dense upper-bound buffers): NaN here
    if mdev is not None and ak:
        A[k_eff:] = float("nan")
        if bk:
            B[k_eff:] = float("nan")
        else:
            B[:, k_eff:] = float("nan")
    elif mdev is not None:
        A[m_eff:] = float("nan")

    odt = F32 if "f32" in epi else dt
    rows_out = M
    out_buf = torch.full((rows_out + 1, N + pc), float("nan"), dtype=odt, device="cuda")   # guard row + padding columns
    out = out_buf[:rows_out, :N]
    kw, ref_kw = {}, {}
    if "bias" in epi:
        kw["bias"] = ref_kw["bias"] = _rand((N,), F32, seed + 3)
    pre = None
    if "gelu_nopre" in epi:
        assert "gelu" not in epi
        kw["gelu"] = ref_kw["gelu"] = True
    if "gelu" in epi:
        kw["gelu"] = ref_kw["gelu"] = True
        pre_buf = torch.full((rows_out + 1, N + pc), float("nan"), dtype=dt, device="cuda")
        pre = kw["save_pre"] = pre_buf[:rows_out, :N]
    keep = None
    if "dropout" in epi:
        kw["dropout"] = (0.1, 4321, 9)
        keep = ops.dropout_mask(M * N, 0.1, 4321, 9, out.device).view(M, N)
        ref_kw.update(keep=keep, drop_p=0.1)
    rowmap = None
    if "rowmap" in epi:
        rowmap = torch.randperm(M, generator=torch.Generator().manual_seed(seed + 4)).int().cuda()
        kw["rowmap"] = ref_kw["rowmap"] = rowmap
    if "rowscale" in epi:
        rps = 97 if M > 194 else max(1, (M + 2) // 3)          # at least two scale groups, one of them zero
        rs = (0.25 + (torch.arange((M + rps - 1) // rps) % 5).float()).cuda()
        assert rs.numel() > 1
        rs[1] = 0.0
        kw["rowscale"] = ref_kw["rowscale"] = (rs, rps)
    aux = res = None
    if "aux" in epi:
        aux_buf = torch.full((rows_out, N + pc), float("nan"), dtype=dt, device="cuda")
        aux_buf[:, :N] = _rand((rows_out, N), dt, seed + 5)
        aux = kw["mul_gelu_grad"] = ref_kw["mul_gelu_grad"] = aux_buf[:, :N]
    if "residual" in epi:
        res = kw["residual"] = ref_kw["residual"] = _padded(rows_out, N, 8, dt, seed + 6)
    if "f32" in epi:
        kw["out_f32"] = True
    if "accum" in epi:
        out[:] = _rand((rows_out, N), odt, seed + 7)
        kw["accumulate"] = True
    prev = out.clone()
    cs = cs_prev = None
    if "colsum" in epi:
        assert ak
        cs_buf = torch.full((M + 1,), float("nan"), device="cuda")
        cs = kw["a_colsum"] = cs_buf[:M]
        if "accum" in epi:
            cs[:] = _rand((M,), F32, seed + 8)
        cs_prev = cs.clone()
    if m_dev is not None:
        kw["m_dev"] = m_dev

    epi_bits = ((L.EPI_BIAS if "bias" in kw else 0) | (L.EPI_GELU if "gelu" in kw else 0) |
                (L.EPI_SAVE_PRE if pre is not None else 0) | (L.EPI_DROPOUT if keep is not None else 0) |
                (L.EPI_ROWSCALE if "rowscale" in kw else 0) | (L.EPI_RESIDUAL if res is not None else 0) |
                (L.EPI_ROWMAP if rowmap is not None else 0) | (L.EPI_MUL_GELU_GRAD if aux is not None else 0) |
                (L.EPI_OUT_F32 if "f32" in epi else 0) | (L.EPI_ACCUM if "accum" in epi else 0))
    plan, route = _plan(L, ops, dt, M, N, K, A, B, out, ak=ak, bk=bk, split=r["split"], epi_bits=epi_bits, m_dev=m_dev,
                        colsum=cs, res=res, pre=pre, aux=aux, bias=kw.get("bias"), rowscale=kw.get("rowscale"), rowmap=rowmap,
                        drop_p=0.1 if keep is not None else 0.0, want_route=r["route"] is not None)
    assert plan == r["plan"], f"planner moved this shape off its route: {plan} != {r['plan']}"
    if r["route"] is not None:
        assert route == (r["route"], plan[2]), f"dispatch moved this shape off its kernel: {route} != {(r['route'], plan[2])}"

    got = ops.gemm(A, B, a_kmajor=ak, b_kmajor=bk, out=out, split_k=r["split"], **kw)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr()

    ref, pre_ref, bound, rows, pre_bound = gemm_ref(
        a64, b64, out_dtype=odt, k_eff=k_eff, m_eff=m_eff, prev=prev if "accum" in epi else None, **ref_kw)
    _note(request, "out", out[rows], ref, bound)
    check_bound(out[rows], ref, bound, "output")
    if pre is not None:
        _note(request, "pre", pre[rows], pre_ref, pre_bound)
        check_bound(pre[rows], pre_ref, pre_bound, "saved pre-activation")
    # nothing written where the kernel has no business: padding columns, the guard row, rows at / beyond m_dev
    written = torch.zeros(rows_out + 1, dtype=torch.bool, device="cuda")
    written[rows] = True
    for name, buf in (("output", out_buf), ("pre-activation", pre_buf if pre is not None else None)):
        if buf is None:
            continue
        assert bool(torch.isnan(buf[:, N:].float()).all()), f"{name}: padding columns N..ldc written"
        if "accum" not in epi or name != "output":
            stale = buf[~written].float()
            assert bool(torch.isnan(stale).all()), f"{name}: rows outside the computed set written"
        else:
            assert bool(torch.isnan(buf[rows_out].float()).all()), "guard row written"
            assert torch.equal(buf[:rows_out][~written[:rows_out]], prev[~written[:rows_out]]), "stale rows changed"
    if cs is not None:
        cs_ref, cs_bound = colsum_ref(a64, k_eff)
        if "accum" in epi:
            cs_ref = cs_ref + cs_prev.double()
            cs_bound = cs_bound + 2.0 ** -24 * cs_ref.abs()
        check_bound(cs, cs_ref, cs_bound, "a_colsum")
        assert bool(torch.isnan(cs_buf[M])), "a_colsum guard written"
