"""Host proof of tests/beam_ref.py: an f32 emulation of the kernel's arithmetic (numpy, the kernel's summation shape) stays inside
bound_s at a ratio <= 0.5 and returns reference lists; three wrong implementations fall outside or are classified wrong; and
the inputs of tests/test_beam_gpu.py leave at most NEAR_TIE_CAP of their lists ambiguous in the reference alone."""
import functools

import pytest
import torch

import beam_ref as R
from gemm_ref import gemm_ref

BF16, F32 = torch.bfloat16, torch.float32


def x_f32(A, W, bias):
    """f32 logits the way an f32-accumulating product forms them (f32 matmul of the stored operands, one rounded bias add)."""
    return (A.float() @ W.float().t() + bias.float()[None, :]).float()


@functools.lru_cache(maxsize=None)
def small(G, nb, dtype):
    A, W, bias, bs = R.case_operands(G, nb, dtype)
    return A, W, bias, bs, R.beam_ref(A, W, bias, bs, nb, 2 * nb)


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("G,nb", R.CASES)
def test_f32_emulation_stays_inside_the_bound(G, nb, dtype):
    A, W, bias, bs, ref = small(G, nb, dtype)
    beam, tok, score = R.emulate(x_f32(A, W, bias), bs, nb, 2 * nb)
    exact, near, wrong, worst = R.classify(ref, beam, tok, score)
    assert not wrong and worst <= 0.5, (exact, near, wrong, worst)
    amb = int(R.ambiguous(ref).sum())
    assert near <= amb, (near, amb)          # a list can only differ from the reference where the reference is ambiguous


@pytest.mark.parametrize("variant", ["bf16_logits", "lse_over_sample", "no_beam_score"])
def test_wrong_implementations_are_caught(variant):
    G, nb = 8, 8
    A, W, bias, bs, ref = small(G, nb, BF16)
    x = x_f32(A, W, bias)
    if variant == "bf16_logits":
        out = R.emulate(x.bfloat16().float(), bs, nb, 2 * nb)
    else:
        out = R.emulate(x, bs, nb, 2 * nb, **{variant: True})
    exact, near, wrong, worst = R.classify(ref, *out)
    assert len(wrong) == G and worst > 1.0, (variant, exact, near, wrong, worst)


def test_gpu_inputs_are_not_ambiguous():
    lists = amb = 0
    for dtype in (BF16, F32):
        for G, nb in R.CASES:
            ref = small(G, nb, dtype)[4]
            a = R.ambiguous(ref)
            lists, amb = lists + G, amb + int(a.sum())
            assert int(a.sum()) <= R.NEAR_TIE_CAP * G, (G, nb, dtype, a.nonzero().flatten().tolist())
    A, W, bias, bs = R.case_operands(0, 0, BF16, big=True)
    ref = R.beam_ref(A, W, bias, bs, R.BIG["num_beams"], 2 * R.BIG["num_beams"])
    a = R.ambiguous(ref)
    assert int(a.sum()) <= R.NEAR_TIE_CAP * ref["G"], a.nonzero().flatten().tolist()
    assert amb + int(a.sum()) <= R.NEAR_TIE_CAP * (lists + ref["G"])


def test_lse_constant_counts_the_summation_shape():
    assert R.lse_sum(30522) == pytest.approx(3 * 10.3262 + 4 + 8 + 23, abs=1e-3)
    assert R.lse_sum(4106) == pytest.approx(3 * 8.3202 + 4 + 2 + 23, abs=1e-3)
