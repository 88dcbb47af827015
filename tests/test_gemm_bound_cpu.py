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
