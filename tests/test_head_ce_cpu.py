"""The bound of tests/head_ce_ref.py is a property of the inputs, not of the kernel: an f32 emulation of mvlt_mlm_head_ce that
sums in another order (96-column tiles folded one after the other) stays inside it on the operands the GPU tests use, and damage
an epilogue can do -- a column past V let in, a missing max subtraction, a dropped tile -- leaves it."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import head_ce_ref as R  # noqa: E402

F32, BF16 = torch.float32, torch.bfloat16
CASES = [(130, 64, 777, None), (65, 768, 777, 37), (1, 64, 777, None)]


def _case(M, K, V, rd, dtype):
    A, W, buf = R.operands(M, K, V, dtype, R.seed_of(M, K, V, dtype))
    lab = R.edge_labels(M, V, rd is not None, 11 + M)
    return A, W, buf, lab


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("M,K,V,rd", CASES)
def test_emulation_in_another_order_is_inside_the_bound(M, K, V, rd, dtype):
    A, W, buf, lab = _case(M, K, V, rd, dtype)
    ref = R.head_ce_ref(A, W, buf[:V], lab, rd)
    lse, xl, s, n = R.emulate_f32(A, W, buf[:V], lab, ref["lse"].numel())
    ratio = ((lse.double() - ref["lse"]).abs() / ref["bound_lse"]).max()
    print(f"lse worst ratio {float(ratio):.3g}, bound max {float(ref['bound_lse'].max()):.3g}")
    assert float(ratio) <= 1.0
    on = ref["on"]
    assert bool(((xl.double() - ref["x_label"]).abs()[on] <= ref["bound_xl"][on]).all())
    assert n == ref["count"] and abs(s - ref["nll_sum"]) <= ref["bound_sum"]
    # a row whose largest logits sit on a rounding boundary may move by a storage step (0.5 at 90 in bf16); the typical row may not
    assert float(ref["bound_lse"].median()) < 1e-2          # (f32: the product bound e_x itself, ~5e-3 at K = 768)


def test_operands_reach_the_edges():
    M, K, V = 130, 64, 777
    A, W, buf, lab = _case(M, K, V, None, BF16)
    x = A.double() @ W.double().t()
    assert 80.0 < float(x.abs().max()) <= 91.0          # exp(90) overflows f32 without the max subtraction
    assert int(buf[:V].argmax()) == V - 1 and float(buf[V]) > 1e4
    for e in (0, V - 1, (V - 1) // R.TILE * R.TILE):
        assert bool((lab == e).any()), e
    assert bool((lab == R.IGNORE).any())


def test_bound_rejects_epilogue_damage():
    M, K, V = 65, 64, 777
    A, W, buf, lab = _case(M, K, V, None, F32)
    ref = R.head_ce_ref(A, W, buf[:V], lab)
    x = ref["x"]

    def off(lse):
        return float(((lse - ref["lse"]).abs() / ref["bound_lse"]).max())
    # the poisoned bias column right behind V let into the sum
    extra = (A.double() @ W.double()[:1].t())[:, 0] + float(buf[V])
    assert off(torch.logsumexp(torch.cat([x, extra[:, None]], 1), 1)) > 1.0
    # the last, partial column tile dropped
    assert off(torch.logsumexp(x[:, :(V - 1) // R.TILE * R.TILE], 1)) > 1.0
    # no max subtraction in f32: overflow
    naive = torch.log(torch.exp(x.float()).sum(1)).double()
    assert not bool(torch.isfinite(naive).all()) or off(naive) > 1.0
    # the label's logit read one column off
    wrong = x.gather(1, (lab.clamp(0) + 1).clamp(max=V - 1)[:, None])[:, 0]
    on = ref["on"] & (lab < V - 1)
    assert bool(((wrong - ref["x_label"]).abs()[on] > ref["bound_xl"][on]).any())


def test_sum_terms_counts_the_built_shape():
    # 16 per lane + 2 exchanges + 1 wave pair + ceil(tiles / 64) + 6 over the tiles never exceeds TILE + tiles
    for V in (1, 777, 30522, 1 << 20):
        tiles = math.ceil(V / R.TILE)
        assert 16 + 2 + 1 + math.ceil(tiles / 64) + 6 <= R.TILE + tiles


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
def test_grid_spacing_is_the_storage_step(dtype):
    """The spacing the flip term rests on, against the neighbour in the storage format itself."""
    from gemm_ref import U32, U_BF16
    g = torch.Generator().manual_seed(5)
    x = ((torch.rand(4096, generator=g) * 2 - 1) * 90).to(dtype)
    x = torch.cat([x, torch.tensor([1.0, -2.0, 64.0, 0.75, 89.5]).to(dtype)])
    if dtype == BF16:
        up = (x.view(torch.int16) + 1).view(BF16)          # next value away from zero
    else:
        up = torch.nextafter(x, torch.sign(x) * math.inf)
    step, _ = R.grid_spacing(x.double(), U_BF16 if dtype == BF16 else U32)
    assert torch.equal(step, (up.double() - x.double()).abs())


@pytest.mark.parametrize("M,K,V,rd", CASES[:2])
def test_every_rounding_flip_of_the_emulation_is_allowed_for(M, K, V, rd):
    """Where an f32 evaluation rounds a logit to another bf16 value than the float64 reference does, the element carries a flip
    allowance that covers the difference -- and some do flip on these operands, so the term is exercised."""
    A, W, buf, lab = _case(M, K, V, rd, BF16)
    ref = R.head_ce_ref(A, W, buf[:V], lab, rd)
    n = ref["lse"].numel()
    x32 = ((A[:n].float() @ W.float().t()) + buf[None, :V]).to(BF16).double()
    diff = (x32 - ref["x"]).abs()
    assert int((diff > 0).sum()) > 0
    assert bool((diff <= ref["d"]).all()), int((diff > ref["d"]).sum())
    print(f"flagged {float((ref['d'] > 0).double().mean()):.4f} of the elements, {int((diff > 0).sum())} flipped")
