"""The per-element GEMM bound of tests/gemm_ref.py can fail: on the host, in float64, it accepts a correctly rounded
result and rejects the local faults a relative Frobenius norm lets through (no GPU needed)."""
import pytest
import torch

from gemm_ref import check_bound, colsum_ref, gemm_ref, gelu64


def _operands(M, N, K, seed):
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(M, K, generator=g).bfloat16().double()
    b = (torch.randn(K, N, generator=g) * K ** -0.5).bfloat16().double()
    return a, b


@pytest.fixture(scope="module")
def mlm():
    """The MLM decoder dgrad's reduction: K = 30522 = 476 whole 64-deep k-tiles + a partial one of 58."""
    M, N, K = 192, 136, 30522
    a, b = _operands(M, N, K, 11)
    ref, _, bound, _, _ = gemm_ref(a, b, out_dtype=torch.bfloat16)
    return a, b, ref, bound


def test_bound_accepts_rounded_result(mlm):
    a, b, ref, bound = mlm
    check_bound(ref.bfloat16(), ref, bound, "bf16-rounded reference")
    # an f32 accumulation in another order, rounded to bf16, is inside it too
    check_bound((a.float() @ b.float()).bfloat16(), ref, bound, "f32 product")


def test_bound_rejects_dropped_partial_k_tile(mlm):
    a, b, ref, bound = mlm
    K = a.shape[1]
    tail = K - K % 64
    assert K - tail == 58
    bad = (a[:, :tail] @ b[:tail]).bfloat16()
    with pytest.raises(AssertionError, match="outside the bound"):
        check_bound(bad, ref, bound, "partial k-tile dropped")


def test_bound_rejects_shifted_column_group(mlm):
    _, _, ref, bound = mlm
    bad = ref.clone()
    bad[:, 68:72] = ref[:, 72:76]              # one 4-column group takes its neighbour's values
    with pytest.raises(AssertionError, match="column 6[89]|column 7[01]"):
        check_bound(bad.bfloat16(), ref, bound, "4-column group shifted")


def test_bound_rejects_zero_row_tile():
    # a big output where one 64-row tile out of 64 is 1.6 % of the rows
    a, b = _operands(4096, 64, 256, 12)
    ref, _, bound, _, _ = gemm_ref(a, b, out_dtype=torch.bfloat16)
    check_bound(ref.bfloat16(), ref, bound, "bf16-rounded reference")
    bad = ref.clone()
    bad[4032:] = 0.0                           # the last row tile never written (a zeroed output)
    with pytest.raises(AssertionError, match="row 40[3-9][0-9]"):
        check_bound(bad.bfloat16(), ref, bound, "row tile zero")


def test_bound_with_epilogue_and_f32_output():
    """GELU (with the A&S erfc's absolute error), bias, residual in f32 output: an f32 evaluation is accepted, an f32
    evaluation that misses a single k-slice of 32 is not; column sums likewise."""
    M, N, K = 96, 40, 3000
    a, b = _operands(M, N, K, 13)
    bias = torch.randn(N, generator=torch.Generator().manual_seed(14))
    res = torch.randn(M, N, generator=torch.Generator().manual_seed(15))
    ref, pre, bound, _, pre_bound = gemm_ref(a, b, out_dtype=torch.float32, bias=bias, gelu=True, residual=res)
    got_pre = a.float() @ b.float() + bias
    got = torch.nn.functional.gelu(got_pre) + res
    check_bound(got, ref, bound, "f32 GELU + residual")
    check_bound(got_pre.bfloat16(), pre, pre_bound, "pre-activation")
    bad_pre = a[:, 32:].float() @ b[32:].float() + bias
    with pytest.raises(AssertionError):
        check_bound(gelu64(bad_pre.double()).float() + res, ref, bound, "k-slice dropped")
    cs, cs_bound = colsum_ref(a)
    check_bound(a.float().sum(1), cs, cs_bound, "colsum")
    with pytest.raises(AssertionError):
        check_bound(a[:, :-1].float().sum(1), cs, cs_bound, "colsum short")


def test_bound_reports_non_finite():
    ref = torch.ones(4, 4, dtype=torch.float64)
    out = ref.clone()
    out[2, 3] = float("nan")
    with pytest.raises(AssertionError, match="row 2, column 3"):
        check_bound(out, ref, torch.full_like(ref, 1e-3), "nan")


# ---------------------------------------------------------------------------------------------------------------------
# The row-streaming kernel (csrc/rowstream.hip), the 8-wave engine (csrc/gemm8.hip) and the grouped weight gradients
# (mvlt_gemm_group): their rounding emulated on the host -- bf16 operands, f32 accumulation one 32-deep MFMA k-block
# after the other, k-slices added in f32 in slice order, output rounding -- is accepted by the bound, and the faults
# their synchronisation could produce, damaged in as few elements as the fault would touch, are rejected.
# tests/test_gemm_engines_gpu.py applies the same bound to the kernels themselves.
def _emu_acc(a, b, k0=0, k1=None):
    """f32 accumulator of a[:, k0:k1] @ b[k0:k1] in the kernels' k order: one 32-deep block after the other."""
    k1 = a.shape[1] if k1 is None else k1
    acc = torch.zeros(a.shape[0], b.shape[1], dtype=torch.float32)
    for k in range(k0, k1, 32):
        e = min(k + 32, k1)
        acc = acc + a[:, k:e].float() @ b[k:e].float()
    return acc


def _emu_colsum(a, k0=0, k1=None):
    """the bias gradient as the engine forms it: ones^T . A on the matrix pipe, f32, 32-deep blocks"""
    k1 = a.shape[1] if k1 is None else k1
    acc = torch.zeros(a.shape[0], dtype=torch.float32)
    for k in range(k0, k1, 32):
        acc = acc + a[:, k:min(k + 32, k1)].float().sum(1)
    return acc


def _slices(K, split):
    """k-ranges of the engine's k-slices (gemm8.hip locate(): ceil(nk / S) 64-deep K-tiles per slice; the last is short)"""
    nk = (K + 63) // 64
    per = (nk + split - 1) // split
    return [(min(s * per * 64, K), min((s + 1) * per * 64, K)) for s in range(split)]


def _worst(out, ref, bound):
    return float(((out.double() - ref).abs() / bound).max())


RS_RING = {1: 5, 0: 21}          # RsCfg<384, 96, x2>::RING and RsCfg<96, 384>::RING (the issue's table)


@pytest.fixture(scope="module")
def rowstream():
    """Bit 1 of the row-streaming kernel (K = 384, N = 96, bias + residual; RING = 5): 22 stages of 32 rows and a 16-row
    fragment at the range end.  Returns the operands, the emulated output and the reference."""
    M, N, K = 22 * 32 + 16 - 3, 96, 384
    a, b = _operands(M, N, K, 21)
    g = torch.Generator().manual_seed(22)
    bias = torch.randn(N, generator=g)
    res = torch.randn(M, N, generator=g).bfloat16()
    ref, _, bound, _, _ = gemm_ref(a, b, out_dtype=torch.bfloat16, bias=bias, residual=res)

    def emulate(x, r, dt=torch.bfloat16):
        return ((_emu_acc(x, b) + bias) + r.float()).to(dt)
    return a, res, emulate, ref, bound


def test_rowstream_emulation_accepted(rowstream):
    a, res, emulate, ref, bound = rowstream
    out = emulate(a, res)
    check_bound(out, ref, bound, "row-streaming emulation")
    # Round-to-nearest bf16 alone reaches U_OUT |ref| = 2^-8 |ref| (8 significant bits), so the ratio of a bf16 output comes
    # close to 1 by construction; the room of the bound's MODEL is what the value before the output rounding leaves of
    # the f32 bound: accumulation over K = 384 and the epilogue's f32 roundings.
    f32_bound = bound - 2.0 ** -8 * ref.abs() + 2.0 ** -24 * ref.abs()
    assert _worst(emulate(a, res, torch.float32), ref, f32_bound) <= 0.25, _worst(emulate(a, res, torch.float32), ref, f32_bound)


def test_rowstream_stale_ring_slot_rejected(rowstream):
    """(a) one 32-row stage computed from the slot's previous content, the rows RING x 32 earlier (re-filled too late or
    read too early): activation rows and the residual block both live in the slot."""
    a, res, emulate, ref, bound = rowstream
    out = emulate(a, res)
    s, back = 9, RS_RING[1] * 32
    bad = out.clone()
    bad[s * 32:(s + 1) * 32] = emulate(a[s * 32 - back:(s + 1) * 32 - back], res[s * 32 - back:(s + 1) * 32 - back])
    with pytest.raises(AssertionError, match=r"row (28[89]|29[0-9]|30[0-9]|31[0-9])\b"):
        check_bound(bad, ref, bound, "stale ring slot")
    # only the activation rows stale (the residual block's DMA had landed): still out
    bad[s * 32:(s + 1) * 32] = emulate(a[s * 32 - back:(s + 1) * 32 - back], res[s * 32:(s + 1) * 32])
    with pytest.raises(AssertionError, match="outside the bound"):
        check_bound(bad, ref, bound, "stale activation rows")


def test_rowstream_range_end_fragment_rejected(rowstream):
    """(b) the 16-row fragment at a workgroup's range end: left unwritten (the output buffer's previous content, here
    zero and NaN), or written twice as long -- the first fragment of the next range holds this range's next rows of the
    SLOT, i.e. what the stage's second half computed from the clamped / neighbouring rows."""
    a, res, emulate, ref, bound = rowstream
    out = emulate(a, res)
    end = 11 * 32 + 16                              # a range that ends on a half stage
    for fill in (0.0, float("nan")):
        bad = out.clone()
        bad[end - 16:end] = fill
        with pytest.raises(AssertionError, match=r"row 3(5[2-9]|6[0-7])\b"):
            check_bound(bad, ref, bound, "fragment unwritten")
    bad = out.clone()
    bad[end:end + 16] = out[end - 16:end]           # the write ran one fragment too far with the rows it had
    with pytest.raises(AssertionError, match=r"row 3(6[89]|7[0-9]|8[0-3])\b"):
        check_bound(bad, ref, bound, "fragment written twice as long")


@pytest.fixture(scope="module")
def wgrad():
    """A weight gradient dW = dY^T X with its bias gradient, 256 x 256 outputs (2 x 2 tiles of 128 x 128), K = 2000
    reduction rows in 4 k-slices of 8 K-tiles (the last one short: 464 rows)."""
    M, N, K, split = 256, 256, 2000, 4
    a, b = _operands(M, N, K, 23)
    ref, _, bound, _, _ = gemm_ref(a, b, out_dtype=torch.float32)
    cs, cs_bound = colsum_ref(a)
    sl = _slices(K, split)
    assert sl[-1] == (1536, 2000)
    parts = [_emu_acc(a, b, k0, k1) for k0, k1 in sl]
    cparts = [_emu_colsum(a, k0, k1) for k0, k1 in sl]
    return ref, bound, cs, cs_bound, parts, cparts


def _slab_sum(parts):
    v = torch.zeros_like(parts[0])
    for p in parts:
        v = v + p                                   # f32, slice order (the last arriver's loop)
    return v


def test_sliced_wgrad_emulation_accepted(wgrad):
    """k-slices added in f32: `split` extra additions per element, each <= 2^-24 of a partial sum <= S.  The bound's
    accumulation term C_ACC 2^-24 sqrt(K) S covers split <= C_ACC sqrt(K) with room (here 4 against 357; the planners
    keep >= 6 K-tiles per slice, so split <= K / 384 < 8 sqrt(K) for every K): no extra term is needed, and the ratio
    below shows it."""
    ref, bound, cs, cs_bound, parts, cparts = wgrad
    out, cout = _slab_sum(parts), _slab_sum(cparts)
    check_bound(out, ref, bound, "k-sliced weight gradient")
    check_bound(cout, cs, cs_bound, "k-sliced bias gradient")
    assert _worst(out, ref, bound) <= 0.25 and _worst(cout, cs, cs_bound) <= 0.25, (
        _worst(out, ref, bound), _worst(cout, cs, cs_bound))
    # any order of the slices (the atomic form) is inside it as well
    check_bound(_slab_sum(parts[::-1]), ref, bound, "k-slices in reverse order")


def test_sliced_wgrad_missing_slice_rejected(wgrad):
    """(c) one k-slice of one 128 x 128 tile missing from the sum -- the short last one, a quarter of an eighth of the
    output's energy -- in the weight and in the bias gradient."""
    ref, bound, cs, cs_bound, parts, cparts = wgrad
    bad = _slab_sum(parts)
    bad[128:, :128] = _slab_sum(parts[:-1])[128:, :128]
    with pytest.raises(AssertionError, match=r"row (12[89]|1[3-9][0-9]|2[0-5][0-9]), column ([0-9]|[1-9][0-9]|1[01][0-9]|12[0-7])\b"):
        check_bound(bad, ref, bound, "k-slice missing")
    cbad = _slab_sum(cparts)
    cbad[128:] = _slab_sum(cparts[:-1])[128:]
    with pytest.raises(AssertionError, match=r"row (12[89]|1[3-9][0-9]|2[0-5][0-9])\b"):
        check_bound(cbad, cs, cs_bound, "k-slice missing from the bias gradient")
    # a slice counted twice (a ticket drawn before the slab was visible, the stale slab of the previous call)
    bad[128:, :128] = (_slab_sum(parts) + parts[1])[128:, :128]
    with pytest.raises(AssertionError, match="outside the bound"):
        check_bound(bad, ref, bound, "k-slice twice")


@pytest.fixture(scope="module")
def engine():
    """A forward product on the 8-wave engine's 128 x 256 tiles: 3 x 3 tiles (ragged in M and N), K = 192 (3 K-tiles)."""
    M, N, K = 300, 640, 192
    a, b = _operands(M, N, K, 24)
    g = torch.Generator().manual_seed(25)
    bias = torch.randn(N, generator=g)
    ref, _, bound, _, _ = gemm_ref(a, b, out_dtype=torch.bfloat16, bias=bias)
    return a, b, bias, ref, bound


def test_engine_emulation_accepted(engine):
    a, b, bias, ref, bound = engine
    out = (_emu_acc(a, b) + bias).bfloat16()
    check_bound(out, ref, bound, "8-wave engine emulation")
    f32_bound = bound - 2.0 ** -8 * ref.abs() + 2.0 ** -24 * ref.abs()          # (see test_rowstream_emulation_accepted)
    assert _worst(_emu_acc(a, b) + bias, ref, f32_bound) <= 0.25, _worst(_emu_acc(a, b) + bias, ref, f32_bound)


def test_engine_next_tiles_operands_rejected(engine):
    """(d) one tile of a persistent list computed from the operands of the list's next tile (the loads of tile i + 1 are
    in flight under the epilogue of tile i): tile (1, 0) holds A's rows of tile (1, 1)'s row band x B's columns of it."""
    a, b, bias, ref, bound = engine
    out = (_emu_acc(a, b) + bias).bfloat16()
    bad = out.clone()
    bad[128:256, 0:256] = (_emu_acc(a[128:256], b[:, 256:512]) + bias[0:256]).bfloat16()
    with pytest.raises(AssertionError, match=r"row (12[89]|1[3-9][0-9]|2[0-4][0-9]|25[0-5]), column ([0-9]|[1-9][0-9]|1[0-9][0-9]|2[0-4][0-9]|25[0-5])\b"):
        check_bound(bad, ref, bound, "tile from the next tile's operands")


def test_engine_stale_half_tile_rejected(engine):
    """(e) one 64-deep half-tile (128 operand rows x 64 k) of one K-tile taken from the previous K-tile: the ring slot was
    read before its re-fill landed.  Once for an A half (128 output rows of one tile), once for a B half (128 of the
    tile's 256 columns)."""
    a, b, bias, ref, bound = engine
    out = (_emu_acc(a, b) + bias).bfloat16()
    a_bad = a[0:128].clone()
    a_bad[:, 128:192] = a[0:128, 64:128]
    bad = out.clone()
    bad[0:128, 256:512] = (_emu_acc(a_bad, b[:, 256:512]) + bias[256:512]).bfloat16()
    with pytest.raises(AssertionError, match=r"row ([0-9]|[1-9][0-9]|1[01][0-9]|12[0-7]), column (25[6-9]|2[6-9][0-9]|[34][0-9][0-9]|50[0-9]|51[01])\b"):
        check_bound(bad, ref, bound, "stale A half-tile")
    b_bad = b[:, 384:512].clone()
    b_bad[64:128] = b[0:64, 384:512]
    bad = out.clone()
    bad[0:128, 384:512] = (_emu_acc(a[0:128], b_bad) + bias[384:512]).bfloat16()
    with pytest.raises(AssertionError, match=r"column (38[4-9]|39[0-9]|4[0-9][0-9]|50[0-9]|51[01])\b"):
        check_bound(bad, ref, bound, "stale B half-tile")
