"""Global-norm gradient clipping and the non-finite step skip on the device: mvlt_grad_sumsq / mvlt_grad_norm_finish /
mvlt_adamw_guarded per element, and FusedAdamW(max_grad_norm=, skip_nonfinite=) on the tiny pre-training model against the fp64
reference of tests/grad_clip_ref.py.

Two runs of the model are not bit-identical (the relative-position-bias and word-embedding gradients are accumulated with float
atomics), so wherever two OPTIMIZER runs are compared with torch.equal the second run still does its own forward and backward pass
but then overwrites the gradient arena with the bytes the first run recorded: equal gradients in, equal parameters out."""
import contextlib
import json
import math
import os
import random

import numpy as np
import pytest
import torch

import grad_clip_ref as R
from conftest import hash_sd, rel_err, synth_batch

pytestmark = pytest.mark.gpu
F32, BF16 = torch.float32, torch.bfloat16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53
HYPER = (4e-5, 0.9, 0.999, 1e-6, 1e-4)          # lr, betas, eps, weight decay of test_adamw_matches_torch


@pytest.fixture(scope="module")
def M():
    import mvlt_amd
    return mvlt_amd


@pytest.fixture(scope="module")
def ops(M):
    return M.ops


# ------------------------------------------------------------------ 1. sum of squares
def _exact_sumsq(*xs):
    """Correctly rounded sum of the (exact) fp64 squares of f32 values."""
    return math.fsum(v for x in xs for v in (x.double() ** 2).tolist())


def _chain(ops, n):
    """Longest chain of fp64 additions behind one partial after one launch over n elements: a lane's vectors into its four sums
    (the grid is fixed: grad_sumsq_parts() workgroups of 256 lanes), 2 to fold the four, 1 tail element, the 6 levels of the wave
    butterfly, 3 to fold the four waves, 1 into partial[b]."""
    lanes = ops.grad_sumsq_parts() * 256
    return -(-(n // 4) // lanes) + 2 + 1 + 6 + 3 + 1


def _total(partial):
    s = 0.0
    for v in partial.tolist():          # index order, as mvlt_grad_norm_finish adds them
        s += v
    return s


def _vec(n, seed):
    return torch.randn(n, generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("n", [1, 3, 4, 5, 255, 1024, 4099, 1000003])
def test_sumsq_matches_fp64_within_the_addition_chain(ops, n):
    """The squares are exact in fp64 and every term is >= 0, so the relative error of the sum is at most (number of additions on
    the longest path) * 2^-53: the chain inside a partial plus the nparts additions over the partials (+1: the rounding of the
    exact reference)."""
    x = _vec(n, 500 + n % 97)
    xd = x.cuda()
    part = ops.grad_sumsq(xd)
    again = ops.grad_sumsq(xd)
    torch.cuda.synchronize()
    assert part.dtype == torch.float64 and part.numel() == ops.grad_sumsq_parts()
    assert torch.equal(part, again)                                     # bit-reproducible
    want, got = _exact_sumsq(x), _total(part)
    c = _chain(ops, n) + ops.grad_sumsq_parts() + 1
    print(f"n={n} rel err {abs(got - want) / want:.3e} bound {c * U:.3e}")
    assert abs(got - want) <= c * U * want


def test_sumsq_accumulates_ranges_in_launch_order(ops):
    xs = [_vec(n, 600 + n) for n in (4099, 5, 1024)]
    part = torch.full((ops.grad_sumsq_parts(),), float("nan"), dtype=torch.float64, device="cuda")    # the first launch STORES
    runs = []
    for _ in range(2):
        for k, x in enumerate(xs):
            ops.grad_sumsq(x.cuda(), part, accumulate=k > 0)
        runs.append(part.clone())
    assert torch.equal(runs[0], runs[1])
    want, got = _exact_sumsq(*xs), _total(runs[0])
    c = sum(_chain(ops, x.numel()) for x in xs) + ops.grad_sumsq_parts() + 1
    assert abs(got - want) <= c * U * want


def test_sumsq_widens_before_squaring(ops):
    """3e19 squared overflows f32 and 1e-30 squared underflows it; widened first, both squares are exact."""
    x = _vec(4099, 611)
    x[7], x[100] = 3e19, 1e-30
    want, got = _exact_sumsq(x), _total(ops.grad_sumsq(x.cuda()))
    assert math.isfinite(got) and abs(got - want) <= (_chain(ops, 4099) + ops.grad_sumsq_parts() + 1) * U * want
    tiny = torch.full((8,), 1e-30)
    assert _total(ops.grad_sumsq(tiny.cuda())) == _exact_sumsq(tiny) > 0.0
    out, flags = ops.grad_norm_finish(ops.grad_sumsq(x.cuda()), 1.0, 1.0, True)
    assert flags.tolist() == [0, 0] and abs(out[0].item() - math.sqrt(want)) <= 2.0 ** -22 * math.sqrt(want)


# ------------------------------------------------------------------ 2. finish
@pytest.mark.parametrize("gs,mx", [(1.0, 1.0), (0.5, 7.5), (-0.25, 3.0), (1.0, 1e4), (1.0, 0.0), (0.5, -2.0)])
def test_finish_norm_and_coefficient(ops, gs, mx):
    x = _vec(4099, 620)
    part = ops.grad_sumsq(x.cuda())
    flags = torch.tensor([7, 3], dtype=torch.int32, device="cuda")
    out, flags = ops.grad_norm_finish(part, gs, mx, True, flags=flags)
    want = abs(gs) * math.sqrt(_exact_sumsq(x))
    norm, coef = np.float32(out[0].item()), np.float32(out[1].item())
    assert abs(float(norm) - want) <= 2.0 ** -22 * want
    assert coef == R.clip_coef(norm, mx)                       # the f32 formula on the kernel's own f32 norm, bit for bit
    if mx <= 0 or want < mx:
        assert coef == np.float32(1.0)
    else:
        assert coef < np.float32(1.0)
    assert flags.tolist() == [0, 3]                            # finite: the flag is cleared, the count stays


# ------------------------------------------------------------------ 3. non-finite inputs
@pytest.mark.parametrize("pos", ["first", "middle", "tail"])
@pytest.mark.parametrize("bad", [float("nan"), float("inf"), -float("inf")])
def test_nonfinite_gradient_raises_the_skip_flag(ops, bad, pos):
    """n % 4 == 3: the last element is read by the scalar tail.  Without skip_nonfinite nothing is special-cased and the value
    propagates as it does through torch.nn.utils.clip_grad_norm_: a NaN norm gives a NaN coefficient; an Inf norm gives
    max_norm / (inf + 1e-6) = 0, and 0 * inf is the NaN the sweep would consume."""
    n = 4099
    assert n % 4 == 3
    x = _vec(n, 630)
    i = {"first": 0, "middle": n // 2, "tail": n - 1}[pos]
    x[i] = bad
    part = ops.grad_sumsq(x.cuda())
    flags = torch.tensor([0, 5], dtype=torch.int32, device="cuda")
    out, flags = ops.grad_norm_finish(part, 1.0, 1.0, True, flags=flags)
    assert flags.tolist() == [1, 6]
    out, flags = ops.grad_norm_finish(part, 1.0, 1.0, True, flags=flags)
    assert flags.tolist() == [1, 7]
    out, flags = ops.grad_norm_finish(part, 1.0, 1.0, False, flags=flags)
    assert flags.tolist() == [0, 7]
    norm, coef = out[0].item(), out[1].item()
    assert not math.isfinite(norm)
    if math.isnan(bad):
        assert math.isnan(coef)
    else:
        assert coef == 0.0 == float(R.clip_coef(norm, 1.0))
    assert not math.isfinite(coef * bad)


# ------------------------------------------------------------------ 4. guarded AdamW
def _adamw_state(n=10007):
    p0 = _vec(n, 90)
    p = torch.zeros(n + 1, device="cuda")[:n].copy_(p0)          # 16B-aligned base
    return [p, torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda"), torch.zeros(n, dtype=torch.bfloat16, device="cuda")]


@pytest.mark.parametrize("gs,c", [(1.0, 1.0), (0.5, 1.0), (1.0, 0.37), (0.5, 0.0123)])
def test_guarded_adamw_is_adamw_with_the_scaled_gradient(ops, gs, c):
    n = 10007
    a, b = _adamw_state(n), _adamw_state(n)
    coef = torch.tensor([c], dtype=torch.float32, device="cuda")
    skip = torch.zeros(1, dtype=torch.int32, device="cuda")
    scale = float(np.float32(gs) * np.float32(c))
    for step in range(1, 4):
        g = _vec(n, 90 + step).cuda()
        ops.adamw(a[0], g, a[1], a[2], a[3], *HYPER, step, scale)
        ops.adamw_guarded(b[0], g, b[1], b[2], b[3], *HYPER, step, gs, coef, skip)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert torch.equal(b[3], b[0].to(torch.bfloat16))


def test_guarded_adamw_writes_nothing_when_the_flag_is_raised(ops):
    n = 10007
    b = _adamw_state(n)
    coef = torch.ones(1, dtype=torch.float32, device="cuda")
    skip = torch.zeros(1, dtype=torch.int32, device="cuda")
    for step in range(1, 3):
        ops.adamw_guarded(b[0], _vec(n, 90 + step).cuda(), b[1], b[2], b[3], *HYPER, step, 1.0, coef, skip)
    before = [t.clone() for t in b]
    skip.fill_(1)
    g = _vec(n, 99).cuda()
    g[5] = float("nan")
    ops.adamw_guarded(b[0], g, b[1], b[2], b[3], *HYPER, 3, 1.0, coef, skip)
    ops.adamw_guarded(b[0][:3], g[:3], b[1][:3], b[2][:3], b[3][:3], *HYPER, 3, 1.0, coef, skip)       # (tail-only launch)
    torch.cuda.synchronize()
    for x, y in zip(before, b):
        assert torch.equal(x, y)


# ------------------------------------------------------------------ the optimizer on the tiny pre-training model
LR, MAX_NORM, SCALES = 1e-3, 0.01, (1.0, 4.0, 0.25)


def _model(M, cd=F32):
    with open(os.path.join(ROOT, "tests", "golden", "specs_hash.json")) as f:
        spec = json.load(f)["hash_tiny_pretrain"]
    cfg = M.MVLBertPretrainConfig(hidden_size=256, num_hidden_layers=2, num_attention_heads=4, intermediate_size=1024, vocab_size=3000)
    cfg.swin.update(embed_dim=32, depths=[2, 2, 2, 2], num_heads=[1, 2, 4, 8], drop_path_rate=0.2)
    cfg.ITM_task = True
    model = M.MVLBertForPretraining(cfg)
    model.load_state_dict(hash_sd(spec), strict=False)
    return M.set_compute_dtype(model.cuda().eval(), cd)


def _batch(seed):
    return tuple(t.cuda() for t in synth_batch(4, 24, seed=seed, vocab=3000))


@contextlib.contextmanager
def _coin(value):
    """The seq2seq / bidirectional coin flip of the pre-training model: < 0.5 trains the seq2seq MLM head, else the other."""
    real = random.random
    random.random = lambda: value
    try:
        yield
    finally:
        random.random = real


def _arena(model):
    from mvlt_amd.arena import Arena
    from mvlt_amd.runtime import compute_dtype_of
    return Arena.of(model, compute_dtype_of(model))


def _backward(model, batch, flip):
    with _coin(flip):
        model(*batch).backward()
    return _arena(model)


def _live(ar):
    """bool mask over the arena: the (unpadded) elements of the parameters that received a gradient in the last backward pass."""
    m = torch.zeros(ar.total, dtype=torch.bool)
    for p in ar.params:
        if ar.has_grad[id(p)]:
            m[ar.offset[id(p)]:ar.offset[id(p)] + p.numel()] = True
    return m


def _steps(ar):
    return {n: ar.steps[id(p)] for n, p in zip(ar.names, ar.params)}


def _snapshot(ar):
    return [t.clone() for t in (ar.flat, ar.exp_avg, ar.exp_avg_sq)] + ([ar.shadow.clone()] if ar.shadow is not None else [])


def _run(M, kw, seeds, flips, cd=F32, scales=None, replay=None):
    """len(seeds) optimizer steps; returns what a comparison needs.  ``scales``: the gradient arena is multiplied by scales[i] after
    backward pass i (norms that differ between steps); ``replay``: it is overwritten with replay[i] (see the module docstring)."""
    from mvlt_amd.optim import FusedAdamW
    model = _model(M, cd)
    opt = FusedAdamW(model, lr=LR, **kw)
    out = dict(model=model, opt=opt, grads=[], live=[], pnorm=[], norms=[])
    for i, (seed, flip) in enumerate(zip(seeds, flips)):
        ar = _backward(model, _batch(seed), flip)
        if i == 0:
            out["p0"] = ar.flat.clone()
        if replay is not None:
            ar.grad.copy_(replay[i])
        elif scales is not None:
            ar.grad.mul_(scales[i])
        out["grads"].append(ar.grad.clone())
        out["live"].append(_live(ar))
        # fp64 norm of the PUBLISHED p.grad tensors (unpadded views): dirt in the arena's padding would show against it
        out["pnorm"].append(R.grad_norm([p.grad for p in model.parameters() if p.grad is not None], opt.grad_scale))
        opt.step()
        if opt.last_grad_norm is not None:
            out["norms"].append(opt.last_grad_norm.clone())
    torch.cuda.synchronize()
    out["ar"] = _arena(model)
    return out


@pytest.fixture(scope="module")
def plain_run(M):
    return _run(M, {}, (71, 72, 73), (0.9, 0.9, 0.9), scales=SCALES)


@pytest.fixture(scope="module")
def clipped_run(M):
    return _run(M, dict(max_grad_norm=MAX_NORM), (71, 72, 73), (0.9, 0.9, 0.9), scales=SCALES)


def _reference(run, max_grad_norm):
    ref = R.RefAdamW(run["p0"], lr=LR, max_grad_norm=max_grad_norm)
    for g, live in zip(run["grads"], run["live"]):
        ref.step(g, live)
    return ref


@pytest.mark.parametrize("kw", [dict(max_grad_norm=1e30), dict(max_grad_norm=1e30, skip_nonfinite=True), dict(skip_nonfinite=True)])
def test_optimizer_with_an_unreachable_clip_equals_the_plain_optimizer(M, plain_run, kw):
    """coef = 1, skip = 0: the guarded sweep is the plain one, bit for bit, over three steps (also the check that the plain run --
    options off -- still launches what it launched before: its own result is pinned by test_optimizer_plain_steps_match_reference)."""
    got = _run(M, kw, (71, 72, 73), (0.9, 0.9, 0.9), replay=plain_run["grads"])
    a, b = plain_run["ar"], got["ar"]
    assert torch.equal(a.flat, b.flat) and torch.equal(a.exp_avg, b.exp_avg) and torch.equal(a.exp_avg_sq, b.exp_avg_sq)
    assert _steps(a) == _steps(b) and got["opt"].steps_skipped == 0
    assert plain_run["opt"].last_grad_norm is None and len(got["norms"]) == 3


def test_optimizer_plain_steps_match_reference(plain_run):
    ref = _reference(plain_run, None)
    assert rel_err(plain_run["ar"].flat.cpu(), ref.p) < 1e-6


def test_optimizer_clipped_steps_match_reference(clipped_run):
    """Three clipped steps against the fp64 reference fed the gradients read back from the arena, at the 1e-6 of
    test_adamw_matches_torch -- and the test can SEE the clip: the same parameters miss the unclipped reference by more than ten
    times that bound (gradient scales 1, 4, 1/4: Adam's first step alone would be scale-invariant; the reference side of this is
    test_grad_clip_cpu.py::test_reference_adamw_equals_torch_adamw_and_sees_the_clip)."""
    assert all(n > 10 * MAX_NORM for n in clipped_run["pnorm"]), clipped_run["pnorm"]
    assert max(clipped_run["pnorm"]) > 3 * min(clipped_run["pnorm"])
    got = clipped_run["ar"].flat.cpu()
    e_clip, e_plain = rel_err(got, _reference(clipped_run, MAX_NORM).p), rel_err(got, _reference(clipped_run, None).p)
    print(f"norms {clipped_run['pnorm']} vs clipped reference {e_clip:.3e}, vs unclipped reference {e_plain:.3e}")
    assert e_clip < 1e-6
    assert e_plain > 10 * 1e-6


def test_last_grad_norm_is_the_norm_of_the_published_gradients(clipped_run):
    """opt.last_grad_norm (taken over the sweep's runs, ALIGN padding included) against the fp64 norm of the unpadded p.grad views."""
    assert len(clipped_run["norms"]) == 3
    for got, want in zip(clipped_run["norms"], clipped_run["pnorm"]):
        assert got.is_cuda and got.dtype == torch.float32 and got.dim() == 0
        assert abs(got.item() - want) <= 2.0 ** -22 * want, (got.item(), want)
    ar = clipped_run["ar"]
    pad = torch.ones(ar.total, dtype=torch.bool)
    for p in ar.params:
        pad[ar.offset[id(p)]:ar.offset[id(p)] + p.numel()] = False
    assert float(ar.grad.cpu()[pad].abs().sum()) == 0.0            # nothing writes the padding


def _poison(model):
    p = next(p for n, p in model.named_parameters() if p.grad is not None and n.endswith("intermediate.dense.weight"))
    p.grad.view(-1)[p.numel() // 2] = float("nan")                  # plain data: nothing faults


@pytest.mark.parametrize("cd", [F32, BF16])
def test_skipped_step_never_happened(M, cd):
    from mvlt_amd.optim import FusedAdamW
    kw = dict(max_grad_norm=MAX_NORM, skip_nonfinite=True)
    twin = _run(M, kw, (71, 72), (0.9, 0.9), cd=cd)                 # never makes the poisoned call
    model = _model(M, cd)
    opt = FusedAdamW(model, lr=LR, **kw)
    ar = _backward(model, _batch(71), 0.9)
    ar.grad.copy_(twin["grads"][0])
    opt.step()
    assert opt.steps_skipped == 0
    before, steps_before = _snapshot(ar), _steps(ar)
    assert (ar.shadow is not None) == (cd == BF16) and max(steps_before.values()) == 1
    _backward(model, _batch(73), 0.9)
    _poison(model)
    opt.step()
    assert opt.steps_skipped == 1                                   # (reconciles the step counts)
    assert math.isnan(opt.last_grad_norm.item())
    for x, y in zip(before, _snapshot(ar)):
        assert torch.equal(x, y)
    assert _steps(ar) == steps_before
    ar = _backward(model, _batch(72), 0.9)
    ar.grad.copy_(twin["grads"][1])
    opt.step()
    torch.cuda.synchronize()
    for x, y in zip(_snapshot(twin["ar"]), _snapshot(ar)):
        assert torch.equal(x, y)
    assert _steps(ar) == _steps(twin["ar"]) and opt.steps_skipped == 1 and twin["opt"].steps_skipped == 0
    sd, tsd = opt.state_dict()["state"], twin["opt"].state_dict()["state"]
    assert {k: v["step"] for k, v in sd.items()} == {k: v["step"] for k, v in tsd.items()}


def test_skipped_step_keeps_the_count_of_an_idle_head(M):
    """Alternating MLM heads: the seq2seq head is idle during the skipped (bidirectional) step and must keep ITS count, the
    bidirectional head must lose the bump of the step that was refused."""
    from mvlt_amd.optim import FusedAdamW
    kw = dict(skip_nonfinite=True)
    twin = _run(M, kw, (71, 72, 74), (0.1, 0.9, 0.1))
    model = _model(M)
    opt = FusedAdamW(model, lr=LR, **kw)
    ar = _backward(model, _batch(71), 0.1)
    ar.grad.copy_(twin["grads"][0])
    opt.step()
    _backward(model, _batch(73), 0.9)
    _poison(model)
    opt.step()
    opt.flush()                                                     # (flush() settles the counts as well)
    st, final = _steps(ar), _steps(twin["ar"])
    # the parameters of each head that its steps update (the twin took two seq2seq steps and one bidirectional step)
    seq = [k for k in st if k.startswith("MLM_head_seq2seq") and final[k] == 2]
    bid = [k for k in st if k.startswith("MLM_head_bidir") and final[k] == 1]
    assert len(seq) >= 4 and len(bid) >= 4
    assert all(st[k] == 1 for k in seq), [(k, st[k]) for k in seq]
    assert all(st[k] == 0 for k in bid), [(k, st[k]) for k in bid]
    for i, (seed, flip) in enumerate(((72, 0.9), (74, 0.1)), start=1):
        ar = _backward(model, _batch(seed), flip)
        ar.grad.copy_(twin["grads"][i])
        opt.step()
    torch.cuda.synchronize()
    for x, y in zip(_snapshot(twin["ar"]), _snapshot(ar)):
        assert torch.equal(x, y)
    st = _steps(ar)
    assert st == _steps(twin["ar"]) and opt.steps_skipped == 1
    assert all(st[k] == 2 for k in seq) and all(st[k] == 1 for k in bid)


def test_clipped_step_after_two_backward_passes_uses_the_summed_gradient(M):
    """Gradient accumulation (two backward passes, one step): the norm is taken at step() time, over the merged gradients."""
    from mvlt_amd.optim import FusedAdamW
    model = _model(M)
    opt = FusedAdamW(model, lr=LR, max_grad_norm=MAX_NORM)
    ar = _backward(model, _batch(72), 0.9)
    g2 = ar.grad.clone()
    opt.zero_grad()                                                 # (done with these: the next pass starts afresh)
    ar = _backward(model, _batch(71), 0.9)
    g1, p0 = ar.grad.clone(), ar.flat.clone()
    ar = _backward(model, _batch(72), 0.9)                          # accumulates into the live gradients of the pass before
    live, merged = _live(ar), ar.grad.clone()
    # the merged arena IS the sum (the second pass's gradients are recomputed here: float-atomic accumulations differ at 1e-6)
    assert rel_err(merged.cpu()[live], (g1.double() + g2.double()).cpu()[live]) < 1e-6
    opt.step()
    torch.cuda.synchronize()
    ref = R.RefAdamW(p0, lr=LR, max_grad_norm=MAX_NORM)
    ref.step(merged, live)
    assert ref.last_norm > 10 * MAX_NORM
    assert abs(opt.last_grad_norm.item() - ref.last_norm) <= 2.0 ** -22 * ref.last_norm
    assert rel_err(ar.flat.cpu(), ref.p) < 1e-6
    one = R.RefAdamW(p0, lr=LR, max_grad_norm=MAX_NORM)
    one.step(g1, live)
    assert rel_err(ar.flat.cpu(), one.p) > 10 * 1e-6                # (the second pass's gradients are in the update)


def test_guard_refuses_overlap_on_a_real_arena(M):
    from mvlt_amd.optim import FusedAdamW
    model = _model(M)
    opt = FusedAdamW(model, lr=LR).overlap_with_backward()
    with pytest.raises(ValueError):
        opt.max_grad_norm = 1.0
    with pytest.raises(ValueError):
        opt.skip_nonfinite = True
