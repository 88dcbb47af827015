"""The three GEMM families with the most intricate synchronisation -- row streaming (csrc/rowstream.hip), the 8-wave
ping-pong engine (csrc/gemm8.hip) and the grouped weight gradients (mvlt_gemm_group in csrc/gemm.hip) -- against the
float64 reference of tests/gemm_ref.py with its PER-ELEMENT bound, at shapes that reach the parts that can go wrong:
ring slots that are re-filled, tile lists of two and three tiles per workgroup, every group form, k-slices with a
short / empty last slice and a reduction length on the device.

Every row asserts its ROUTE first (mvlt_gemm_route / mvlt_gemm_group_route: the dispatch itself in its no-launch mode, on
the very struct that is launched next), runs the product once and checks every element, the saved pre-activation and the
bias gradients.  Output padding, a guard row behind every output and the rows beyond a device-side row count are
pre-filled with NaN and must keep it; operand rows beyond a device-side count hold NaN.

tests/test_gemm_bound_cpu.py shows on the host that this bound rejects the faults these kernels could produce.

Not covered here (read once per process, so a test cannot switch them): MVLT_WGRAD_GLDS (the two-stage 64 x 128 LDS-DMA
group form, GROUP_GLDS_64x128_S2, and the register-staged forms by switch), MVLT_WGRAD_BM, MVLT_WGRAD_PER_CU,
MVLT_G8_WGRAD_GRID.  Row streaming: the chunked shape of bit 7 cannot have ns <= D + 1 at an eligible M (64 row groups:
M >= 16384 gives 8 stages against D = 5), and no chunked shape can have two stages per workgroup."""
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch

from gemm_ref import check_bound, colsum_ref, gemm_ref, logical

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")
WORST = {}                      # test id -> worst |out - ref| / bound (printed per row: profiles/gemm_engine_bounds.md)


@pytest.fixture(scope="module")
def L():
    from mvlt_amd import _lib
    _lib.lib()
    return _lib


@pytest.fixture(scope="module")
def ops():
    from mvlt_amd import ops as o
    return o


def _randn(shape, dt, seed, scale=1.0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.randn(shape, generator=g, device="cuda") * scale).to(dt)


def _padded(rows, cols, pad, dt, seed, scale=1.0, guard=0):
    """[rows, cols] view of a [rows + guard, cols + pad] buffer whose padding (and guard rows) hold NaN."""
    buf = torch.full((rows + guard, cols + pad), NAN, dtype=dt, device="cuda")
    buf[:rows, :cols] = _randn((rows, cols), dt, seed, scale)
    return buf[:rows, :cols]


def _ratio(out, ref, bound):
    out = out.double()
    r = torch.where(torch.isfinite(out), (out - ref).abs() / bound, torch.full_like(ref, float("inf")))
    return float(r.max()) if r.numel() else 0.0


def _note(request, what, value):
    key = request.node.name
    WORST[key] = max(WORST.get(key, 0.0), value)
    print(f"BOUND-RATIO {key} {what} {value:.4f}")


def _route(L, r):
    return L.gemm_route_name(r)


# ===================================================================================================== single products
class Product:
    """One mvlt_gemm call on a hand-filled MvltGemm: the same struct answers the route query and is launched."""

    def __init__(self, L, ops, dt, M, N, K, *, bk=False, pad=(0, 0, 0), epi=(), rps=784, mdev=None, bias_off=0, seed=1):
        self.L, self.ops, self.M, self.N, self.K, self.bk, self.epi = L, ops, M, N, K, bk, set(epi)
        pa, pb, pc = pad
        self.A = _padded(M, K, pa, dt, seed + 1)
        self.B = _padded(K, N, pb, dt, seed + 2, K ** -0.5) if bk else _padded(N, K, pb, dt, seed + 2, K ** -0.5)
        self.a64, self.b64 = logical(self.A, self.B, False, bk)
        self.m_eff = M if mdev is None else min(max(mdev, 0), M)
        self.m_dev = None if mdev is None else torch.tensor([mdev], dtype=torch.int32, device="cuda")
        if mdev is not None:
            self.A[self.m_eff:] = NAN
        self.out_buf = torch.full((M + 1, N + pc), NAN, dtype=dt, device="cuda")
        self.out = self.out_buf[:M, :N]
        self.ref_kw = {}
        p = self.p = L.MvltGemm()
        p.dtype, p.M, p.N, p.K = (L.BF16 if dt == BF else L.F32), M, N, K
        p.A, p.lda, p.B, p.ldb, p.b_kmajor = self.A.data_ptr(), self.A.stride(0), self.B.data_ptr(), self.B.stride(0), int(bk)
        p.C, p.ldc = self.out.data_ptr(), self.out.stride(0)
        bits = 0
        self.pre_buf = self.pre = None
        self.keep = []
        if "bias" in self.epi:
            store = _randn((N + 4 + bias_off,), F32, seed + 3)
            bias = store[bias_off:bias_off + N] if bias_off else store[:N]          # bias_off = 1: 4-byte aligned only
            self.keep.append(store)
            self.ref_kw["bias"] = bias
            p.bias = bias.data_ptr()
            bits |= L.EPI_BIAS
        if "gelu" in self.epi:
            self.ref_kw["gelu"] = True
            bits |= L.EPI_GELU
        if "pre" in self.epi:
            self.pre_buf = torch.full((M + 1, N + pc), NAN, dtype=dt, device="cuda")
            self.pre = self.pre_buf[:M, :N]
            p.pre = self.pre.data_ptr()
            bits |= L.EPI_SAVE_PRE
        if "rowscale" in self.epi:
            rs = (0.25 + (torch.arange((M + rps - 1) // rps) % 5).float()).cuda()
            rs[1 % rs.numel()] = 0.0
            self.ref_kw["rowscale"] = (rs, rps)
            p.rowscale, p.rows_per_scale = rs.data_ptr(), rps
            bits |= L.EPI_ROWSCALE
        if "aux" in self.epi:
            aux = _padded(M, N, pc, dt, seed + 5)
            self.ref_kw["mul_gelu_grad"] = aux
            p.aux = aux.data_ptr()
            bits |= L.EPI_MUL_GELU_GRAD
        if "residual" in self.epi:
            res = _padded(M, N, 8, dt, seed + 6)
            self.ref_kw["residual"] = res
            p.residual, p.ldr = res.data_ptr(), res.stride(0)
            bits |= L.EPI_RESIDUAL
        p.epilogue = bits
        if self.m_dev is not None:
            p.m_dev = self.m_dev.data_ptr()
        assert L.lib().mvlt_gemm_workspace_bytes(C.byref(p)) == 0          # (no split-K row in this file)

    def route(self):
        return _route(self.L, self.L.lib().mvlt_gemm_route(C.byref(self.p)))

    def run_and_check(self, request, block=32768):
        L, M, N = self.L, self.M, self.N
        L.check(L.lib().mvlt_gemm(C.byref(self.p), self.ops._stream()), "mvlt_gemm")
        torch.cuda.synchronize()
        dt = self.out.dtype
        for r0 in range(0, self.m_eff, block):          # float64 reference on the device, in row blocks
            r1 = min(r0 + block, self.m_eff)
            rows = torch.arange(r0, r1, dtype=torch.int32, device="cuda")
            ref, pre_ref, bound, _, pre_bound = gemm_ref(self.a64[r0:r1], self.b64, out_dtype=dt, rowmap=rows, **self.ref_kw)
            check_bound(self.out[r0:r1], ref, bound, f"output rows {r0}..{r1}")
            _note(request, "out", _ratio(self.out[r0:r1], ref, bound))
            if self.pre is not None:
                check_bound(self.pre[r0:r1], pre_ref, pre_bound, f"saved pre-activation rows {r0}..{r1}")
                _note(request, "pre", _ratio(self.pre[r0:r1], pre_ref, pre_bound))
        for name, buf in (("output", self.out_buf), ("pre-activation", self.pre_buf)):
            if buf is None:
                continue
            assert bool(torch.isnan(buf[:, N:].float()).all()), f"{name}: padding columns N..ldc written"
            assert bool(torch.isnan(buf[self.m_eff:].float()).all()), f"{name}: guard row / rows beyond m_dev written"


# ------------------------------------------------------------------------------------------------------ row streaming
# bit -> (K, N, k-major B, epilogue needs a row operand, RING, D, row groups); csrc/rowstream.hip RsCfg / mvlt_rowstream_try
RS = {0: (96, 384, False, False, 21, 20, 256), 1: (384, 96, False, True, 5, 4, 256), 2: (192, 768, False, False, 11, 10, 64),
      3: (96, 384, True, True, 5, 4, 256), 4: (384, 96, True, False, 6, 5, 256), 5: (96, 96, True, False, 21, 20, 256),
      6: (288, 96, True, False, 7, 6, 256), 7: (192, 768, True, True, 6, 5, 64), 8: (192, 192, True, False, 11, 10, 256)}
# the epilogues the Swin block issues on each shape (first = the one run at the large M)
RS_EPI = {0: [("bias", "gelu", "pre"), ("bias", "gelu")],                                  # Mlp fc1 forward
          1: [("bias", "rowscale", "residual"), ("residual",)],                            # Mlp fc2 / proj forward
          2: [("bias", "gelu", "pre"), ("bias", "gelu")],
          3: [("aux",), ("residual",)],                                                    # fc2 dgrad x gelu'(pre), dgrad + residual
          4: [(), ("bias", "rowscale")], 5: [(), ("rowscale",)], 6: [()],                  # fc1 / proj / qkv dgrads
          7: [("aux",), ("residual",)], 8: [()]}


def _stages(M, rg_count):
    """stages (32 rows) of every row group: the kernel's own partition (16-row fragments, rowstream_kernel)"""
    F = (M + 15) // 16
    ns, half = [], 0
    for rg in range(rg_count):
        f0, f1 = F * rg // rg_count, F * (rg + 1) // rg_count
        rows = min(f1 * 16, M) - f0 * 16
        ns.append((rows + 31) // 32)
        half += (f1 - f0) % 2
    return ns, half


def _rs_m(bit, kind):
    """large: every workgroup runs the steady-state loop and re-fills slots (ns >= RING + 2; two full revolutions,
    ns >= 2 RING + 1, where RING <= 7), neighbours differ in their stage count, ranges end on half stages; floor: just
    above the 16384-row floor (two stages per workgroup where the shape is not chunked); first: ns in {D, D + 1} -- the
    first re-fill is the last issue (ns = D + 1) or never happens (ns = D)."""
    K, N, bk, x2, RING, D, RG = RS[bit]
    if kind == "floor":
        return 16391
    if kind == "large":
        ns_min = 2 * RING + 1 if RING <= 7 else RING + 2
        # 2 ns_min or 2 ns_min + 1 fragments per row group: ns_min or ns_min + 1 stages, the odd ranges end on a half stage
        return (2 * ns_min * RG + (100 if RG == 256 else 20)) * 16 - 5
    return (2 * D * RG + RG // 2) * 16 - 7                              # fragments alternate 2 D and 2 D + 1


RS_ROWS = []
for _bit in range(9):
    for _i, _e in enumerate(RS_EPI[_bit]):
        RS_ROWS.append(pytest.param(_bit, "floor", _e, 16 if _i else 784, id=f"bit{_bit}-floor-{'+'.join(_e) or 'plain'}"))
    RS_ROWS.append(pytest.param(_bit, "large", RS_EPI[_bit][0], 784, id=f"bit{_bit}-large"))
    if _bit != 7:
        RS_ROWS.append(pytest.param(_bit, "first", RS_EPI[_bit][-1], 16, id=f"bit{_bit}-first-refill"))


@pytest.mark.parametrize("bit,kind,epi,rps", RS_ROWS)
def test_rowstream_route(L, ops, monkeypatch, request, bit, kind, epi, rps):
    K, N, bk, x2, RING, D, RG = RS[bit]
    M = _rs_m(bit, kind)
    ns, half = _stages(M, RG)
    assert M % 16 and M >= 16384
    if kind == "large":
        assert min(ns) >= (2 * RING + 1 if RING <= 7 else RING + 2) and len(set(ns)) > 1 and half > 0, (min(ns), max(ns), half)
    elif kind == "first":
        assert set(ns) == {D, D + 1}, sorted(set(ns))
    elif RG == 256:
        assert min(ns) == 2 and min(ns) < D - 1, sorted(set(ns))
    monkeypatch.setenv("MVLT_ROWSTREAM", hex(1 << bit))
    pr = Product(L, ops, BF, M, N, K, bk=bk, epi=epi, rps=rps, seed=100 + bit)
    assert pr.route() == (f"ROWSTREAM_{bit}", 1)
    pr.run_and_check(request)


# the conditions of mvlt_rowstream_try, one broken at a time on bit 1's shape (K = 384, N = 96: 64 x 96 tiles, LDS-DMA loop)
RS_REFUSED = [
    pytest.param(dict(pad=(8, 0, 0)), id="lda-not-K"),
    pytest.param(dict(pad=(0, 0, 8)), id="ldc-not-N"),
    pytest.param(dict(mdev=16000), id="m_dev"),
    pytest.param(dict(bias_off=1), id="bias-unaligned"),
    pytest.param(dict(rps=24), id="rps-not-16n"),
    pytest.param(dict(M=16383), id="below-floor"),
]


@pytest.mark.parametrize("kw", RS_REFUSED)
def test_rowstream_refusal_falls_through(L, ops, monkeypatch, request, kw):
    monkeypatch.setenv("MVLT_ROWSTREAM", "0x1ff")
    monkeypatch.delenv("MVLT_G8", raising=False)
    kw = dict(kw)
    M = kw.pop("M", 16391)
    pr = Product(L, ops, BF, M, 96, 384, epi=("bias", "rowscale", "residual"), seed=120, **kw)
    assert pr.route() == ("GLDS", 1)
    pr.run_and_check(request)


@pytest.mark.parametrize("bit,M,want", [(1, 49152, "ROWSTREAM_1"), (1, 49151, "REG"), (2, 49152, "G8_22_WIDE"), (2, 49151, "G8_22_WIDE")])
def test_rowstream_default_mask_and_floor(L, ops, monkeypatch, request, bit, M, want):
    """Without the switch: bits 0, 1, 3, 4, 5, 6 from 49152 rows.  Bit 1 one row below the floor: 384 row tiles of 128, the
    register-staged 128 x 96 kernel.  Bit 2 is off at any M: 192 x 3 = 576 tiles of 256 x 256 >= 400, which the automatic mode
    gives to the 8-wave engine (three tiles per workgroup for 64 of them, K = 192)."""
    monkeypatch.delenv("MVLT_ROWSTREAM", raising=False)
    monkeypatch.delenv("MVLT_G8", raising=False)
    K, N, bk = RS[bit][:3]
    pr = Product(L, ops, BF, M, N, K, bk=bk, epi=RS_EPI[bit][0], seed=130 + bit)
    assert pr.route() == (want, 1)
    pr.run_and_check(request)


# ------------------------------------------------------------------------------------- 8-wave engine, forward and dgrad
def G(id, tile, M, N, K, bk=False, epi=(), narrow=False, mdev=None):
    return pytest.param(dict(tile=tile, M=M, N=N, K=K, bk=bk, epi=epi, narrow=narrow, mdev=mdev), id=id)


# 128 x 256 tiles: 17 x 17 = 289 tiles on 256 workgroups (33 walk two, 223 one); 23 x 23 = 529 (17 walk three)
# 256 x 256 tiles: 18 x 17 = 306.  Ragged in M and N.  K = 64: one K-tile, the ring crosses a tile boundary every
# tile; K = 192: an odd K-tile count (the 2- and 4-deep rings end a tile in a different slot than they started it).
M12, N12, M22, N22 = 16 * 128 + 37, 16 * 256 + 40, 17 * 256 + 37, 16 * 256 + 40
G8_ROWS = [
    G("12-fwd-none-k64", 12, M12, N12, 64),
    G("12-fwd-bias-k192-narrow", 12, M12, N12, 192, epi=("bias",), narrow=True),
    G("12-fwd-gelu-k192", 12, M12, N12, 192, epi=("bias", "gelu")),
    G("12-fwd-pre-k64-narrow-mdev-in-tile", 12, M12, N12, 64, epi=("bias", "gelu", "pre"), narrow=True, mdev=1000),
    G("12-fwd-pre-k192-513tiles", 12, 22 * 128 + 37, 22 * 256 + 40, 192, epi=("bias", "gelu", "pre")),
    G("12-dgrad-none-k192-narrow", 12, M12, N12, 192, bk=True, narrow=True),
    G("12-dgrad-aux-k64", 12, M12, N12, 64, bk=True, epi=("aux",)),
    G("12-dgrad-res-k192-mdev-boundary", 12, M12, N12, 192, bk=True, epi=("residual",), mdev=1536),
    G("12-dgrad-res-k64-513tiles-narrow", 12, 22 * 128 + 37, 22 * 256 + 40, 64, bk=True, epi=("residual",), narrow=True),
    G("22-fwd-none-k192-narrow", 22, M22, N22, 192, narrow=True),
    G("22-fwd-bias-k64", 22, M22, N22, 64, epi=("bias",)),
    G("22-fwd-gelu-k64-narrow", 22, M22, N22, 64, epi=("bias", "gelu"), narrow=True),
    G("22-fwd-pre-k192-mdev-boundary", 22, M22, N22, 192, epi=("bias", "gelu", "pre"), mdev=2048),
    G("22-fwd-bias-k64-mdev0", 22, M22, N22, 64, epi=("bias",), mdev=0),
    G("22-dgrad-none-k64", 22, M22, N22, 64, bk=True),
    G("22-dgrad-aux-k192-narrow-mdev-in-tile", 22, M22, N22, 192, bk=True, epi=("aux",), narrow=True, mdev=3000),
    G("22-dgrad-res-k192", 22, M22, N22, 192, bk=True, epi=("residual",)),
    G("22-dgrad-aux-k64-513tiles", 22, 23 * 256 + 37, 22 * 256 + 40, 64, bk=True, epi=("aux",)),
]


@pytest.mark.parametrize("r", G8_ROWS)
def test_gemm8_route(L, ops, monkeypatch, request, r):
    monkeypatch.setenv("MVLT_G8", "1")
    monkeypatch.setenv("MVLT_G8_TILE", str(r["tile"]))
    monkeypatch.delenv("MVLT_G8_WIDE", raising=False)
    bm = 256 if r["tile"] == 22 else 128
    tiles = -(-r["M"] // bm) * -(-r["N"] // 256)
    assert tiles > 256 and tiles % 256 != 0, tiles
    pr = Product(L, ops, BF, r["M"], r["N"], r["K"], bk=r["bk"], epi=r["epi"], pad=(0, 0, 4 if r["narrow"] else 0),
                 mdev=r["mdev"], seed=200 + r["K"])
    assert pr.route() == (f"G8_{r['tile']}_{'NARROW' if r['narrow'] else 'WIDE'}", 1)
    pr.run_and_check(request)


@pytest.mark.parametrize("M,N,want", [(20 * 256 - 10, 20 * 256, "G8_22_WIDE"), (19 * 256 - 10, 21 * 256, "GLDS")])
def test_gemm8_automatic_threshold(L, ops, monkeypatch, request, M, N, want):
    """MVLT_G8 unset: 400 tiles of 256 x 256 are taken, 399 with K < 1536 are not."""
    for v in ("MVLT_G8", "MVLT_G8_TILE", "MVLT_G8_WIDE", "MVLT_TILE"):
        monkeypatch.delenv(v, raising=False)
    assert -(-M // 256) * -(-N // 256) == (400 if want.startswith("G8") else 399)
    pr = Product(L, ops, BF, M, N, 128, epi=("bias",), seed=260)
    assert pr.route() == (want, 1)
    pr.run_and_check(request)


# ============================================================================================ grouped weight gradients
class Group:
    """dW_i = dY_i^T X_i (+ bias gradients) as one mvlt_gemm_group call on hand-filled structs."""

    def __init__(self, L, ops, dt, shapes, R, *, lda_pad=0, ldc_pad=0, mdev=None, no_colsum=(), ws=True, seed=300):
        self.L, self.ops, self.n, self.R = L, ops, len(shapes), R
        self.k_eff = R if mdev is None else min(max(mdev, 0), R)
        self.m_dev = None if mdev is None else torch.tensor([mdev], dtype=torch.int32, device="cuda")
        self.arr = (L.MvltGemm * self.n)()
        self.items = []
        for i, (no, ni) in enumerate(shapes):
            dy = _padded(R, no, lda_pad, dt, seed + 2 * i)
            x = _padded(R, ni, 0, dt, seed + 2 * i + 1, R ** -0.5)
            a64, b64 = logical(dy, x, True, True)
            if mdev is not None:          # stale rows of dense upper-bound buffers
                dy[self.k_eff:] = NAN
                x[self.k_eff:] = NAN
            dw_buf = torch.full((no + 1, ni + ldc_pad), NAN, dtype=F32, device="cuda")
            dw = dw_buf[:no, :ni]
            cs_buf = None if i in no_colsum else torch.full((no + 1,), NAN, device="cuda")
            p = self.arr[i]
            p.dtype, p.M, p.N, p.K = (L.BF16 if dt == BF else L.F32), no, ni, R
            p.A, p.lda, p.a_kmajor = dy.data_ptr(), dy.stride(0), 1
            p.B, p.ldb, p.b_kmajor = x.data_ptr(), x.stride(0), 1
            p.C, p.ldc = dw.data_ptr(), dw.stride(0)
            p.epilogue, p.split_k = L.EPI_OUT_F32, 1
            if self.m_dev is not None:
                p.m_dev = self.m_dev.data_ptr()
            if cs_buf is not None:
                p.a_colsum = cs_buf.data_ptr()
            self.items.append((dy, x, a64, b64, dw_buf, cs_buf))
        self.ws = None
        need = L.lib().mvlt_gemm_group_workspace_bytes(self.arr, self.n)
        self.ws_need = need
        if need and ws:
            self.ws = torch.empty(need, dtype=torch.uint8, device="cuda")
            self.arr[0].workspace, self.arr[0].workspace_bytes = self.ws.data_ptr(), need

    def route(self):
        return _route(self.L, self.L.lib().mvlt_gemm_group_route(self.arr, self.n))

    def launch(self):
        self.L.check(self.L.lib().mvlt_gemm_group(self.arr, self.n, self.ops._stream()), "mvlt_gemm_group")
        torch.cuda.synchronize()

    def run_and_check(self, request):
        self.launch()
        for i, (dy, x, a64, b64, dw_buf, cs_buf) in enumerate(self.items):
            no, ni = a64.shape[0], b64.shape[1]
            ref, _, bound, _, _ = gemm_ref(a64, b64, out_dtype=F32, k_eff=self.k_eff)
            check_bound(dw_buf[:no, :ni], ref, bound, f"dW of product {i}")
            _note(request, f"dW{i}", _ratio(dw_buf[:no, :ni], ref, bound))
            assert bool(torch.isnan(dw_buf[no]).all()) and bool(torch.isnan(dw_buf[:, ni:]).all()), f"dW {i}: guard row / padding written"
            if cs_buf is not None:
                cs, cs_bound = colsum_ref(a64, self.k_eff)
                check_bound(cs_buf[:no], cs, cs_bound, f"bias gradient of product {i}")
                _note(request, f"db{i}", _ratio(cs_buf[:no], cs, cs_bound))
                assert bool(torch.isnan(cs_buf[no])), f"bias gradient {i}: guard written"


def W(id, want, dt, shapes, R, env=(), **kw):
    return pytest.param(dict(want=want, dt=dt, shapes=shapes, R=R, env=dict(env), kw=kw), id=id)


G8ON, G8OFF = (("MVLT_G8", "1"),), (("MVLT_G8", "0"),)
# 2 x (1544 x 1536): 13 x 12 tiles of 128 x 128 each = 312 >= 256 -> 128-row tiles; 2 x (776 x 1024): 56 tiles of 128 rows
# each (< 256) but 13 x 8 x 2 = 208 tiles of 64 rows (>= 200: no k-slices, not the engine's)
# 2 x (776 x 960): 13 x 10 x 2 = 260 tiles of 64 x 96
BIG, MID, W96 = [(1544, 1536), (1544, 1536)], [(776, 1024), (776, 1024)], [(776, 960), (776, 960)]
SMALL = [(256, 384), (384, 256), (128, 128)]          # 6 + 6 + 1 = 13 tiles of 128 x 128: k-slices
GROUP_ROWS = [
    W("glds128x128", ("GROUP_GLDS_128x128", 1), BF, BIG, 328, ldc_pad=4),
    W("glds64x128-s3", ("GROUP_GLDS_64x128_S3", 1), BF, MID, 456, ldc_pad=4, no_colsum=(1,)),
    # an operand whose row stride is not a multiple of 8 elements: no 16-byte loads, the register-staged kernels
    W("reg128x128", ("GROUP_REG_128x128", 1), BF, BIG, 328, lda_pad=4, ldc_pad=2),
    W("reg64x128", ("GROUP_REG_64x128", 1), BF, MID, 456, lda_pad=4, mdev=300),
    W("reg64x96", ("GROUP_REG_64x96", 1), BF, W96, 456, ldc_pad=4, no_colsum=(0,)),
    W("f32-reg64x96", ("GROUP_REG_64x96", 1), F32, [(200, 192), (96, 288)], 300, ldc_pad=1),
    W("f32-reg64x128", ("GROUP_REG_64x128", 1), F32, [(200, 128), (72, 256)], 300, mdev=123),
    W("f32-reg128x128", ("GROUP_REG_128x128", 1), F32, BIG, 136),
    # atomic k-slices (the engine switched off): 13 x 2 tiles of 64 x 128; 18 K-tiles -> 2 slices (576 + 524 rows)
    W("atomic-split2", ("GROUP_ATOMIC", 2), BF, SMALL, 1100, env=G8OFF),
    # 81 K-tiles -> 10 slices of 9 K-tiles: the tenth is EMPTY; the ninth ends at row 5150 (partial K-tile)
    W("atomic-split10-empty-last", ("GROUP_ATOMIC", 10), BF, SMALL, 5150, env=G8OFF, no_colsum=(2,)),
    W("atomic-split4-partial-last", ("GROUP_ATOMIC", 4), BF, SMALL, 2100, env=G8OFF),
    W("atomic-mdev0", ("GROUP_ATOMIC", 4), BF, SMALL, 2100, env=G8OFF, mdev=0),
    W("atomic-mdev-first-slice", ("GROUP_ATOMIC", 4), BF, SMALL, 2100, env=G8OFF, mdev=333),
    W("atomic-mdev-third-slice", ("GROUP_ATOMIC", 4), BF, SMALL, 2100, env=G8OFF, mdev=1500),
    # the engine's group form, every tile mode, unsliced and with forced slices (20 K-tiles in 3 slices: 7 + 7 + 6, the
    # last K-tile partial: 1250 = 19 x 64 + 34)
    W("g8-22-split1", ("GROUP_G8_22", 1), BF, SMALL, 1250, env=G8ON + (("MVLT_G8_TILE", "22"), ("MVLT_G8_SPLIT", "1"))),
    W("g8-12-split1", ("GROUP_G8_12", 1), BF, SMALL, 1250, env=G8ON + (("MVLT_G8_TILE", "12"), ("MVLT_G8_SPLIT", "1"))),
    W("g8-11-split1", ("GROUP_G8_11", 1), BF, SMALL, 1250, env=G8ON + (("MVLT_G8_TILE", "11"), ("MVLT_G8_SPLIT", "1")), no_colsum=(1,)),
    W("g8-22-split3", ("GROUP_G8_22", 3), BF, SMALL, 1250, env=G8ON + (("MVLT_G8_TILE", "22"), ("MVLT_G8_SPLIT", "3"))),
    W("g8-12-split3", ("GROUP_G8_12", 3), BF, SMALL, 1250, env=G8ON + (("MVLT_G8_TILE", "12"), ("MVLT_G8_SPLIT", "3")), no_colsum=(0,)),
    W("g8-11-split3", ("GROUP_G8_11", 3), BF, SMALL, 1250, env=G8ON + (("MVLT_G8_TILE", "11"), ("MVLT_G8_SPLIT", "3"))),
    # 9 K-tiles per slice, 4 slices for 33 K-tiles: 9 + 9 + 9 + 6
    W("g8-11-split4", ("GROUP_G8_11", 4), BF, SMALL, 2100, env=G8ON + (("MVLT_G8_TILE", "11"), ("MVLT_G8_SPLIT", "4"))),
    # no workspace: the unsliced plan of the same shape
    W("g8-11-no-workspace", ("GROUP_G8_11", 1), BF, SMALL, 1250, env=G8ON + (("MVLT_G8_TILE", "11"), ("MVLT_G8_SPLIT", "3")), ws=False),
    # 3 x 16 tiles x 3 slices = 144 units on 128 workgroups: 16 workgroups walk two units of different tiles and products
    W("g8-11-units-over-cap", ("GROUP_G8_11", 3), BF, [(512, 512)] * 3, 1250,
      env=G8ON + (("MVLT_G8_TILE", "11"), ("MVLT_G8_SPLIT", "3")), no_colsum=(1,)),
    # the reduction length on the device in the sliced engine form: 0, inside the first slice, inside the last
    W("g8-11-split3-mdev0", ("GROUP_G8_11", 3), BF, SMALL, 1250, env=G8ON + (("MVLT_G8_TILE", "11"), ("MVLT_G8_SPLIT", "3")), mdev=0),
    W("g8-11-split3-mdev-first-slice", ("GROUP_G8_11", 3), BF, SMALL, 1250, env=G8ON + (("MVLT_G8_TILE", "11"), ("MVLT_G8_SPLIT", "3")), mdev=100),
    W("g8-12-split3-mdev-last-slice", ("GROUP_G8_12", 3), BF, SMALL, 1250, env=G8ON + (("MVLT_G8_TILE", "12"), ("MVLT_G8_SPLIT", "3")), mdev=1001),
    W("g8-22-split3-mdev-first-slice", ("GROUP_G8_22", 3), BF, SMALL, 1250, env=G8ON + (("MVLT_G8_TILE", "22"), ("MVLT_G8_SPLIT", "3")), mdev=63),
]


@pytest.mark.parametrize("r", GROUP_ROWS)
def test_gemm_group_route(L, ops, monkeypatch, request, r):
    for v in ("MVLT_G8", "MVLT_G8_TILE", "MVLT_G8_SPLIT"):
        monkeypatch.delenv(v, raising=False)
    for k, v in r["env"].items():
        monkeypatch.setenv(k, v)
    g = Group(L, ops, r["dt"], r["shapes"], r["R"], **r["kw"])
    if r["want"][0].startswith("GROUP_G8") and r["want"][1] > 1:
        assert g.ws_need > 0
    assert g.route() == r["want"]
    g.run_and_check(request)


def test_gemm_group_default_plan_is_the_engine(L, ops, monkeypatch, request):
    """No switch at all, the workspace the library asks for: a group with fewer than 200 tiles and thousands of reduction
    rows goes to the engine, cut into slices (whichever shape and count its cost model picks)."""
    for v in ("MVLT_G8", "MVLT_G8_TILE", "MVLT_G8_SPLIT"):
        monkeypatch.delenv(v, raising=False)
    g = Group(L, ops, BF, SMALL, 4000 - 24, no_colsum=(1,))
    name, slices = g.route()
    print(f"default plan: {name} x {slices}")
    assert name.startswith("GROUP_G8_") and slices > 1 and g.ws_need > 0
    g.run_and_check(request)


def test_gemm_group_deterministic_child(L):
    """MVLT_DETERMINISTIC=1 is read once per process: a fresh child runs the sliced group twice (bit-identical) and checks
    it against the bound (tests/gemm_group_det_worker.py)."""
    env = dict(os.environ, MVLT_DETERMINISTIC="1")
    for v in ("MVLT_G8", "MVLT_G8_TILE", "MVLT_G8_SPLIT"):
        env.pop(v, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "gemm_group_det_worker.py")], env=env, capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0 and "DETERMINISTIC-GROUP-OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    print(r.stdout)
