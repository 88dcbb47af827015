"""Host side of global-norm gradient clipping / non-finite step skip: the fp64 reference of tests/grad_clip_ref.py against
torch.nn.utils.clip_grad_norm_, the argument refusals of FusedAdamW / PretrainStep, and the C-ABI additions (three entry points, no
new struct, no ABI bump)."""
import math
import os
import re

import numpy as np
import pytest
import torch

import grad_clip_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _sets():
    g = torch.Generator().manual_seed(4101)
    shapes = [(7, 13), (64,), (3, 5, 2), (129,)]
    # (scale of the gradients, max_norm): two clipped sets, and one whose norm is BELOW max_norm (nothing is clipped)
    return [([torch.randn(s, generator=g) * sc for s in shapes], mx) for sc, mx in ((1.0, 1.0), (30.0, 0.25), (1e-3, 1.0))]


@pytest.mark.parametrize("case", range(3))
def test_reference_norm_and_clipped_gradients_equal_torch_clip_grad_norm(case):
    """torch clips fp64 tensors with an fp64 coefficient; the reference (like the kernel) rounds the norm to f32 and forms the
    coefficient in f32: three f32 roundings (norm, norm + 1e-6, the quotient) = 3 * 2^-24 relative on every clipped element.  The
    norm itself differs only by fp64 summation order."""
    grads, mx = _sets()[case]
    ps = [torch.nn.Parameter(torch.zeros_like(g, dtype=torch.float64)) for g in grads]
    for p, g in zip(ps, grads):
        p.grad = g.double().clone()
    tn = float(torch.nn.utils.clip_grad_norm_(ps, mx))
    norm = R.grad_norm(grads)
    assert abs(norm - tn) <= 1e-13 * tn
    coef = R.clip_coef(norm, mx)
    assert coef.dtype == np.float32
    if case == 2:
        assert norm < mx and coef == np.float32(1.0)
        for p, g in zip(ps, grads):
            assert torch.equal(p.grad, g.double())
    else:
        assert norm > mx and coef < 1.0
    for p, g in zip(ps, grads):
        want, got = p.grad, g.double() * float(coef)
        assert float((got - want).abs().max()) <= 3 * 2.0 ** -24 * float(want.abs().max())


def test_reference_coefficient_and_skip_follow_the_kernel_contract():
    assert R.clip_coef(5.0, 0.0) == 1.0 and R.clip_coef(5.0, -1.0) == 1.0 and R.clip_coef(5.0, None) == 1.0
    assert math.isnan(float(R.clip_coef(float("nan"), 1.0)))
    assert float(R.clip_coef(float("inf"), 1.0)) == 0.0          # torch: max_norm / (inf + 1e-6) = 0
    assert R.clip_coef(2.0, 1.0) == np.float32(1.0) / (np.float32(2.0) + np.float32(1e-6))
    big = [torch.tensor([3e19, 1e-30, 1.0])]
    x = float(torch.tensor(3e19))                                # (3e19 rounded to f32)
    assert math.isfinite(R.grad_norm(big)) and abs(R.grad_norm(big) - x) < 1e-12 * x      # 3e19 ** 2 overflows f32, not fp64
    for bad in (float("nan"), float("inf"), -float("inf")):
        ssq = R.sumsq([torch.tensor([1.0, bad, 2.0])])
        assert R.skip(ssq, True) and not R.skip(ssq, False)
    assert not R.skip(R.sumsq(big), True)


def _ref_run(clip, scales=(1.0, 4.0, 0.25), n=4099, steps=3):
    g = torch.Generator().manual_seed(4102)
    ref = R.RefAdamW(torch.randn(n, generator=g), lr=1e-3, max_grad_norm=clip)
    for k in range(steps):
        ref.step(torch.randn(n, generator=g) * scales[k])
    return ref


def test_reference_adamw_equals_torch_adamw_and_sees_the_clip():
    """The reference update is torch.optim.AdamW's, and a clip is VISIBLE in it when the norms differ between steps (Adam's first
    step alone is scale-invariant): with gradient scales 1, 4, 1/4 and a max_norm below every norm, three clipped steps are more
    than ten times the GPU tests' 1e-6 bound away from three unclipped ones -- the reference side of
    test_grad_clip_gpu.py::test_optimizer_clipped_steps_match_reference."""
    from conftest import rel_err
    g = torch.Generator().manual_seed(4102)
    p = torch.randn(4099, generator=g).double().requires_grad_(True)
    opt = torch.optim.AdamW([p], lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=1e-4)
    for k in range(3):
        p.grad = (torch.randn(4099, generator=g) * (1.0, 4.0, 0.25)[k]).double()
        opt.step()
    plain = _ref_run(None)
    assert rel_err(plain.p, p.detach()) < 1e-14
    clipped = _ref_run(0.5)
    assert plain.last_norm > 10 * 0.5                       # every step's norm is far above max_norm (sqrt(4099) * scale)
    assert rel_err(clipped.p, plain.p) > 10 * 1e-6


def test_reference_skipped_step_never_happened():
    ref = _ref_run(None)
    ref.skip_nonfinite = True
    before = (ref.p.clone(), ref.m.clone(), ref.v.clone(), ref.steps.clone())
    g = torch.ones(4099)
    g[17] = float("nan")
    ref.step(g)
    assert ref.skipped == 1 and all(torch.equal(a, b) for a, b in zip(before, (ref.p, ref.m, ref.v, ref.steps)))


# ------------------------------------------------------------------ argument refusals
@pytest.mark.parametrize("bad", [0, 0.0, -1.0, float("inf"), float("nan"), "1.0", True])
def test_max_grad_norm_must_be_a_finite_positive_number(bad):
    from mvlt_amd.optim import FusedAdamW
    with pytest.raises(ValueError):
        FusedAdamW(torch.nn.Linear(3, 3), max_grad_norm=bad)
    opt = FusedAdamW(torch.nn.Linear(3, 3))
    with pytest.raises(ValueError):
        opt.max_grad_norm = bad


@pytest.mark.parametrize("kw", [dict(max_grad_norm=1.0), dict(skip_nonfinite=True)])
def test_guard_refuses_partial_sweeps_in_both_orders(kw, monkeypatch):
    from mvlt_amd.optim import FusedAdamW
    from mvlt_amd.train import PretrainStep
    lin = torch.nn.Linear(3, 3)
    with pytest.raises(ValueError):
        FusedAdamW(lin, defer_tail=True, **kw)
    with pytest.raises(ValueError):
        FusedAdamW(lin, **kw).overlap_with_backward()             # options first, overlap second
    # overlap first, options second (the arena hooks need a GPU: stubbed, the refusal is host logic)
    monkeypatch.setattr(FusedAdamW, "_state", lambda self: None)
    monkeypatch.setattr(FusedAdamW, "_hook", lambda self, ar: None)
    opt = FusedAdamW(lin).overlap_with_backward()
    with pytest.raises(ValueError):
        for k, v in kw.items():
            setattr(opt, k, v)
    assert not opt._guarded
    opt = FusedAdamW(lin, defer_tail=True)
    with pytest.raises(ValueError):
        for k, v in kw.items():
            setattr(opt, k, v)
    for other in (dict(overlap_optimizer=True), dict(defer_optimizer_tail=True)):
        with pytest.raises(ValueError):
            PretrainStep(lin, lr=1e-3, **other, **kw)
    with pytest.raises(ValueError):
        PretrainStep(lin, lr=1e-3, max_grad_norm=-1.0)
    step = PretrainStep(lin, lr=1e-3, max_grad_norm=2, skip_nonfinite=True)      # passed through
    assert step.opt.max_grad_norm == 2.0 and step.opt.skip_nonfinite is True
    assert FusedAdamW(lin).max_grad_norm is None and FusedAdamW(lin).skip_nonfinite is False


# ------------------------------------------------------------------ C-ABI
NEW = ("mvlt_grad_sumsq", "mvlt_grad_norm_finish", "mvlt_adamw_guarded")


def test_new_entry_points_are_bound_and_exported_without_an_abi_bump():
    from mvlt_amd import _lib
    L = _lib.lib()
    for name in NEW + ("mvlt_grad_sumsq_parts",):
        assert name in _lib.SYMBOLS and getattr(L, name) is not None
    with open(os.path.join(ROOT, "include", "mvlt_hip.h")) as f:
        hdr = f.read()
    for name in NEW + ("mvlt_grad_sumsq_parts",):
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
    assert int(re.search(r"#define\s+MVLT_ABI_VERSION\s+(\d+)", hdr).group(1)) == 17 == _lib.ABI_VERSION == L.mvlt_version()
    assert re.search(r"MVLT_STRUCT_COUNT = 21\b", hdr) and len(_lib.STRUCTS) == 21
    assert L.mvlt_grad_sumsq_parts() >= 1


def test_new_entry_points_refuse_bad_arguments_before_any_launch():
    """NULL pointers, n < 1 and a misaligned gradient pointer return MVLT_ERR_ARG (checked before the launch: no GPU needed)."""
    import ctypes as C
    from mvlt_amd import _lib
    L = _lib.lib()
    ERR_ARG = next(k for k, v in _lib.ERRORS.items() if v == "MVLT_ERR_ARG")
    buf = (C.c_double * 64)()
    a = C.addressof(buf)
    assert a % 16 == 0 or (a + 8) % 16 == 0
    a += a % 16
    vp = C.c_void_p
    assert L.mvlt_grad_sumsq(vp(0), 4, vp(a), 0, vp(0)) == ERR_ARG
    assert L.mvlt_grad_sumsq(vp(a), 4, vp(0), 0, vp(0)) == ERR_ARG
    assert L.mvlt_grad_sumsq(vp(a), 0, vp(a), 0, vp(0)) == ERR_ARG
    assert L.mvlt_grad_sumsq(vp(a + 4), 4, vp(a), 0, vp(0)) == ERR_ARG
    assert L.mvlt_grad_norm_finish(vp(0), 1, 1.0, 1.0, 0, vp(a), vp(a), vp(0)) == ERR_ARG
    assert L.mvlt_grad_norm_finish(vp(a), 0, 1.0, 1.0, 0, vp(a), vp(a), vp(0)) == ERR_ARG
    assert L.mvlt_grad_norm_finish(vp(a), 1, 1.0, 1.0, 0, vp(0), vp(a), vp(0)) == ERR_ARG
    assert L.mvlt_grad_norm_finish(vp(a), 1, 1.0, 1.0, 0, vp(a), vp(0), vp(0)) == ERR_ARG
    args = (4, 1e-3, 0.9, 0.999, 1e-6, 1e-4, 1, 1.0)
    assert L.mvlt_adamw_guarded(vp(a), vp(a), vp(a), vp(a), vp(0), *args, vp(0), vp(a), vp(0)) == ERR_ARG
    assert L.mvlt_adamw_guarded(vp(a), vp(a), vp(a), vp(a), vp(0), *args, vp(a), vp(0), vp(0)) == ERR_ARG
    assert L.mvlt_adamw_guarded(vp(a), vp(a + 4), vp(a), vp(a), vp(0), *args, vp(a), vp(a), vp(0)) == ERR_ARG
