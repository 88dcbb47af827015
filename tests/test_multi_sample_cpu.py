"""Host proof of the per-row pick's reference (tests/multi_sample_ref.py) and of the host-only pieces of multi-sample decoding
(no GPU): an f32 emulation of the epilogue stays inside the bounds at a ratio <= 0.5 on the very inputs of
tests/test_pick_rows_gpu.py, with no more near-ties than the cap; ways of getting the epilogue wrong fall outside; the row tables
of ``decode.sample_many``; the advantage arithmetic of ``scst``; the header and the binding."""
import os
import re
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import multi_sample_ref as R  # noqa: E402
import sample_ref as S  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, BF16 = torch.float32, torch.bfloat16
MIXED_CASES = R.MIXED_CASES          # the inputs of the mixed-row GPU tests


def _ratio(out, ref, bound):
    out = out.double()
    r = torch.where(torch.isfinite(out), (out - ref).abs() / bound, torch.full_like(ref, float("inf")))
    return float(r.max())


def _case(rows, K, N, dtype, seed):
    A, W, bias = R.operands(rows, K, N, dtype, seed)
    noise_row, inv_t = R.mixed_tables(rows)
    ref = R.pick_rows_ref(A, W, bias, noise_row, inv_t, R.SEED, R.TAG)
    raw32 = A.float() @ W.float().t() + bias[None, :]                 # an f32 product in another summation order
    return raw32, noise_row, inv_t, ref


@pytest.mark.parametrize("case", MIXED_CASES, ids=lambda c: f"R{c[0]}-K{c[1]}-N{c[2]}-{str(c[3])[6:]}")
def test_f32_emulation_stays_inside_the_bounds_on_the_gpu_tests_inputs(case):
    """ratio <= 0.5 for y and the log-probability, and at most NEAR_TIE_CAP (2 %: 1 of 70 picks) near-ties for the fixed seeds
    the GPU tests use."""
    raw32, noise_row, inv_t, ref = _case(*case)
    _, y32, tok, lp = R.emulate_f32(raw32, noise_row, inv_t, R.SEED, R.TAG)
    r_y, r_lp = _ratio(y32, ref["y"], ref["bound_y"]), _ratio(lp, ref["logprob"], ref["bound_lp"](tok))
    exact, near = S.assert_picks(tok, ref["y"], ref["bound_y"], f"f32 emulation {case[:3]}")
    print(f"{case[:4]}: y ratio {r_y:.3f}, logprob ratio {r_lp:.3f}; {exact} exact / {near} near-ties of {case[0]} picks")
    assert r_y <= 0.5 and r_lp <= 0.5, (r_y, r_lp)
    assert near <= 1
    greedy = noise_row < 0
    assert bool((ref["g"][greedy] == 0).all()) and bool((ref["e_g"][greedy] == 0).all()) and bool((ref["g"][~greedy] != 0).any())
    assert torch.equal(ref["tok"][greedy], ref["x"][greedy].argmax(1))          # a greedy row is the argmax of its logits


def test_wrong_epilogues_fall_outside():
    rows = 70
    raw32, noise_row, inv_t, ref = _case(*MIXED_CASES[1])

    def rejected(y32, tok):
        _, near, bad = S.classify_picks(tok, ref["y"], ref["bound_y"])
        return _ratio(y32, ref["y"], ref["bound_y"]) > 1.0 and (bool(bad) or near > S.NEAR_TIE_CAP * rows)

    # 1. the noise indexed by the row of the launch instead of noise_row[r]
    _, y_w, tok_w, _ = R.emulate_f32(raw32, noise_row, inv_t, R.SEED, R.TAG, noise_idx_row=torch.arange(rows, dtype=torch.int32))
    assert rejected(y_w, tok_w)
    # 2. noise on the greedy rows as well
    _, y_w, tok_w, _ = R.emulate_f32(raw32, noise_row, inv_t, R.SEED, R.TAG, greedy_noise=True)
    assert rejected(y_w, tok_w)
    g = noise_row < 0
    assert _ratio(y_w[~g], ref["y"][~g], ref["bound_y"][~g]) <= 0.5          # (the sampled rows are untouched by this damage)
    # 3. one inv_t for all rows
    x_w, y_w, tok_w, lp_w = R.emulate_f32(raw32, noise_row, torch.full_like(inv_t, float(inv_t[1])), R.SEED, R.TAG)
    assert _ratio(y_w, ref["y"], ref["bound_y"]) > 1.0
    assert _ratio(lp_w, R.lp_at(ref, tok_w), ref["bound_lp"](tok_w)) > 1.0
    same_t = inv_t == inv_t[1]
    assert _ratio(y_w[same_t], ref["y"][same_t], ref["bound_y"][same_t]) <= 0.5


def test_penalty_after_the_temperature_is_another_rounding_only():
    """The penalty acts on the raw logit AHEAD of inv_t.  In real arithmetic (raw * p) * inv_t and (raw * inv_t) * p are one number
    (inv_t > 0 keeps the sign the penalty branches on), so no error bound can tell the two orders apart: both sit inside the
    reference's bounds.  What separates them is the rounding -- the f32 values differ in many elements -- which is why the GPU
    test of the _rules form asks for bit-for-bit equality with the chunked siblings and not for a bound."""
    raw32, noise_row, inv_t, _ = _case(*MIXED_CASES[1])
    seen = torch.zeros_like(raw32, dtype=torch.bool)
    seen[:, ::7] = True
    pen = 1.3
    before = R.penalise32(raw32, seen, pen) * inv_t[:, None]
    after = R.penalise32(raw32 * inv_t[:, None], seen, pen)
    hot = seen & (inv_t != 1.0)[:, None]
    differ = int((before != after)[hot].sum())
    assert differ > 0.05 * int(hot.sum()), differ
    assert torch.equal(before[~hot], after[~hot])
    assert float(((before - after).abs() / before.abs().clamp_min(1e-30)).max()) < 2.0 ** -22


@pytest.mark.parametrize("B,K,greedy,noise,slot0", [
    (3, 3, True, [-1, 0, 1, 2, -1, 3, 4, 5, -1, 6, 7, 8], [0, 1, 2, 3] * 3),
    (3, 3, False, [0, 1, 2, 3, 4, 5, 6, 7, 8], [0, 1, 2] * 3),
    (2, 1, True, [-1, 0, -1, 1], [0, 1] * 2),
])
def test_row_tables_of_sample_many(B, K, greedy, noise, slot0):
    from mvlt_amd import decode
    T = 0.7
    noise_row, inv_t, slot = decode.multi_sample_tables(B, K, greedy, T, 5)
    assert noise_row.dtype == torch.int32 and inv_t.dtype == torch.float32 and slot.dtype == torch.int32
    assert noise_row.tolist() == noise
    it = S.inv_t_f32(T)
    assert inv_t.tolist() == [1.0 if n < 0 else it for n in noise]
    assert tuple(slot.shape) == (len(noise), 5) and slot.is_contiguous()
    assert slot[:, 0].tolist() == slot0 and bool((slot == slot[:, :1]).all())
    # the draws do not depend on include_greedy: the sampled rows carry the same noise rows either way
    other, _, _ = decode.multi_sample_tables(B, K, not greedy, T, 5)
    assert noise_row[noise_row >= 0].tolist() == other[other >= 0].tolist() == list(range(B * K))


def test_advantages_on_cpu_tensors():
    from mvlt_amd import scst
    gen = torch.Generator().manual_seed(4)
    r = torch.rand(5, 4, generator=gen, dtype=torch.float64) * 3
    rg = torch.rand(5, generator=gen, dtype=torch.float64) * 3
    a = scst.advantages(r, rg, 'greedy')
    assert a.dtype == torch.float32 and tuple(a.shape) == (5, 4) and not a.requires_grad
    assert torch.equal(a, (r - rg[:, None]).to(torch.float32))
    m = scst.advantages(r, None, 'mean')
    want = torch.stack([r[:, k] - (r.sum(1) - r[:, k]) / 3 for k in range(4)], 1)
    assert m.dtype == torch.float32 and torch.equal(m, want.to(torch.float32))
    # the leave-one-out rows sum to 0 within f64 rounding (checked on the f64 values the cast starts from)
    assert float(want.sum(1).abs().max()) <= 16 * 2.0 ** -52 * float(r.abs().max())
    assert float(m.double().sum(1).abs().max()) <= 4 * 2.0 ** -24 * float(r.abs().max()) * 4
    two = scst.advantages(torch.tensor([[1.0, 3.0]], dtype=torch.float64), None, 'mean')
    assert two.tolist() == [[-2.0, 2.0]]
    with pytest.raises(ValueError):
        scst.advantages(r[:, :1], None, 'mean')                # K = 1 has no other sample
    with pytest.raises(ValueError):
        scst.advantages(r, rg, 'median')
    with pytest.raises(ValueError):
        scst.advantages(r, None, 'greedy')


def test_header_and_binding():
    import inspect
    import mvlt_amd
    from mvlt_amd import _lib, decode, scst
    hdr = open(os.path.join(ROOT, "include", "mvlt_hip.h")).read()
    assert int(re.search(r"#define\s+MVLT_ABI_VERSION\s+(\d+)", hdr).group(1)) == 17 == _lib.ABI_VERSION == _lib.lib().mvlt_version()
    assert re.search(r"MVLT_STRUCT_COUNT = 21\b", hdr) and len(_lib.STRUCTS) == 21
    for name in ("mvlt_gemm_pick_rows", "mvlt_gemm_pick_rows_rules", "mvlt_gemm_pick_rows_step", "mvlt_gemm_pick_rows_step_rules"):
        assert re.search(r"\bint " + name + r"\(const MvltGemm\* p, float\* part_val, int32_t\* part_idx, const int32_t\* noise_row,\s+"
                         r"const float\* inv_t,", hdr), name
        assert name in _lib.SYMBOLS and hasattr(_lib.lib(), name), name
    assert len(_lib.SYMBOLS["mvlt_gemm_pick_rows"][1]) == 10 and len(_lib.SYMBOLS["mvlt_gemm_pick_rows_step"][1]) == 7
    assert mvlt_amd.sample_many is decode.sample_many
    sig = inspect.signature(decode.sample_many)
    assert "top_k" not in sig.parameters and "top_p" not in sig.parameters and "learning_strategy" not in sig.parameters
    assert sig.parameters["include_greedy"].default is True
    sig = inspect.signature(scst.self_critical_loss)
    assert (sig.parameters["num_samples"].default, sig.parameters["baseline"].default, sig.parameters["one_pass"].default) == (1, 'greedy', None)
    assert inspect.signature(mvlt_amd.MVLBertForImageCaption.generate).parameters["num_return_sequences"].default == 1
