"""Parameter groups resolved inside the AdamW sweep (mvlt_adamw_groups) and LR schedules: the kernel per element against
misc_ref.adamw_ref called per same-group segment, its bit identities with mvlt_adamw / the guarded form, the grid switch in a fresh
child, and FusedAdamW(param_groups=...) / LRSchedule / PretrainStep on the tiny pre-training model against the fp64 reference of
tests/param_groups_ref.py on every route (plain, clipped, deferred tail, overlapped with the backward pass, checkpoint resume).

Two runs of the model are not bit-identical (float-atomic gradient accumulations), so wherever two OPTIMIZER runs are compared with
torch.equal the second run does its own forward and backward pass and then overwrites the gradient arena with the bytes the first
run recorded (the scheme of test_grad_clip_gpu.py)."""
import contextlib
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

import misc_ref as MR
import param_groups_ref as PG
from conftest import hash_sd, rel_err, synth_batch
from misc_ref import check_bound, check_equal, check_untouched

pytestmark = pytest.mark.gpu
F32, BF16 = torch.float32, torch.bfloat16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL = 7.0
GUARD = 64                      # elements in front of and behind every buffer (keeps the 16-byte alignment)
BLOCK = 64
SCALES = (1.0, 0.1, 0.0, 2.5)
TRIP = MR.ADAMW_SWEEP           # elements of one trip of the capped grid


@pytest.fixture(scope="module")
def M():
    import mvlt_amd
    return mvlt_amd


@pytest.fixture(scope="module")
def ops(M):
    return M.ops


# ------------------------------------------------------------------ 1. the kernel, per element
def _tables(ngroups, wd):
    """lr_scale[g] walks SCALES, weight_decay[g] walks (wd, 0, 2 wd): every group differs from its neighbours in both."""
    return (torch.tensor([SCALES[g % 4] for g in range(ngroups)], dtype=F32),
            torch.tensor([(wd, 0.0, 2.0 * wd)[g % 3] for g in range(ngroups)], dtype=F32))


def _map(n, case):
    """uint8 [n / 64] and the number of groups of the tables."""
    nb = n // BLOCK
    if case == "one":
        return torch.zeros(nb, dtype=torch.uint8), 1
    if case == "two":                           # the second half of the blocks is group 1
        m = torch.zeros(nb, dtype=torch.uint8)
        m[nb // 2:] = 1
        return m, 2
    if case == "every-block":                   # 0 1 2 3 0 ...: four groups inside one wave's 256 elements
        return (torch.arange(nb) % 4).to(torch.uint8), 4
    if case == "trip":                          # a new group at every trip boundary of the capped grid
        return (torch.arange(nb) // (TRIP // BLOCK) + 1).to(torch.uint8), 4
    if case == "trip255":                       # the same with 256 groups and id 255 in the middle trip
        return torch.tensor([1, 255, 3, 0], dtype=torch.uint8)[torch.arange(nb) // (TRIP // BLOCK)], 256
    if case == "id255":                         # 256 groups, ids 255 / 7 / 128 / 0 in use
        return torch.tensor([255, 7, 128, 0], dtype=torch.uint8)[torch.arange(nb) % 4], 256
    raise ValueError(case)


def _segments(bmap):
    """Maximal same-group segments [(lo, hi, group)] in elements."""
    out, lo = [], 0
    ids = bmap.tolist()
    for b in range(1, len(ids) + 1):
        if b == len(ids) or ids[b] != ids[lo]:
            out.append((lo * BLOCK, b * BLOCK, ids[lo]))
            lo = b
    return out


def _guarded(t):
    buf = torch.full((t.numel() + 2 * GUARD,), FILL, dtype=t.dtype, device="cuda")
    view = buf[GUARD:GUARD + t.numel()]
    view.copy_(t)
    return buf, view


def _state(n, late, seed, shadow=True):
    p = torch.randn(n, generator=MR.gen(seed))
    if late:
        m = 0.1 * torch.randn(n, generator=MR.gen(seed + 1))
        v = torch.rand(n, generator=MR.gen(seed + 2)) * 0.01 + 1e-8
    else:
        m, v = torch.zeros(n), torch.zeros(n)
    bufs = [_guarded(t) for t in (p, m, v)]
    bufs.append(_guarded(torch.zeros(n, dtype=BF16)) if shadow else (None, None))
    return bufs


def _check_guards(bufs, what):
    for name, (buf, view) in zip(("p", "m", "v", "shadow"), bufs):
        if buf is not None:
            fill = torch.full((GUARD,), FILL, dtype=buf.dtype, device="cuda")
            check_equal(buf[:GUARD], fill, f"{what} {name} front guard")
            check_untouched(buf, GUARD + view.numel(), FILL, f"{what} {name} guard")


def grouped_steps(ops, n, case, hyper, family, steps, *, late=False, shadow=True, coef=None, seed=90, check=True):
    lr, wd = MR.ADAMW_HYPER[hyper]
    bmap_c, ng = _map(n, case)
    assert bmap_c.numel() * BLOCK == n and int(bmap_c.max()) < ng
    lrs_c, wds_c = _tables(ng, wd)
    bmap, lrs, wds = bmap_c.cuda(), lrs_c.cuda(), wds_c.cuda()
    bufs = _state(n, late, seed, shadow)
    (p, m, v, sh) = (b[1] for b in bufs)
    cf = None if coef is None else torch.tensor([coef], device="cuda")
    skip = None if coef is None else torch.zeros(4, dtype=torch.int32, device="cuda")
    for step in steps:
        g_c, gscale = MR.adamw_grad(family, n, seed + 10 + step)
        g = g_c.cuda()
        refs = []
        if check:
            for lo, hi, grp in _segments(bmap_c):
                lr_g = float(np.float32(lr) * np.float32(lrs_c[grp].item()))          # the f32 product the kernel forms
                refs.append((lo, hi, grp, MR.adamw_ref(p[lo:hi], g[lo:hi], m[lo:hi], v[lo:hi], lr_g, wds_c[grp].item(), step, gscale, coef)))
        ops.adamw_groups(p, g, m, v, sh, bmap, lrs, wds, lr, *MR.ADAMW_BETAS, MR.ADAMW_EPS, step, gscale, cf, skip)
        what = f"adamw_groups n={n} {case} {hyper} {family} step={step}" + ("" if coef is None else f" coef={coef}")
        for lo, hi, grp, ref in refs:
            for k, o in zip("pmv", (p, m, v)):
                check_bound(o[lo:hi].double(), ref[k], ref[k + "_b"], f"{what} {k} of segment [{lo}, {hi}) group {grp}")
        if shadow:
            assert torch.equal(sh, p.to(BF16)), what + " shadow"
        _check_guards(bufs, what)
    return p, m, v, sh


KERNEL_CASES = [(64, "one"), (128, "two"), (320, "every-block"), (320, "id255"), (TRIP + 64, "trip"), (2 * TRIP + 192, "trip"),
                (2 * TRIP + 192, "trip255")]


@pytest.mark.parametrize("n,case", KERNEL_CASES, ids=lambda x: str(x))
def test_kernel_sizes_and_maps(ops, n, case):
    """Steps 1, 2 from zero moments and step 1000 from settled ones.  n = 320 puts four groups inside one wave's 256 elements;
    524288 + 64 and 2 * 524288 + 192 take the capped grid to its second and third trips with a new group at each trip boundary."""
    assert (TRIP + 64) % BLOCK == 0 and (2 * TRIP + 192) // TRIP == 2
    grouped_steps(ops, n, case, "big-lr-wd", "randn", (1, 2))
    grouped_steps(ops, n, case, "project", "randn", (1000,), late=True, seed=190)


@pytest.mark.parametrize("hyper", list(MR.ADAMW_HYPER))
@pytest.mark.parametrize("family", ["randn", "zeros-third", "huge"])
def test_kernel_gradient_families(ops, family, hyper):
    for case in ("every-block", "id255"):
        grouped_steps(ops, 320 + 64 * 37, case, hyper, family, (1, 2))
        grouped_steps(ops, 320 + 64 * 37, case, hyper, family, (1000,), late=True, seed=190)


def test_kernel_guarded_coefficient_and_null_shadow(ops):
    grouped_steps(ops, 320, "every-block", "big-lr-wd", "randn", (1, 2), coef=0.37)
    grouped_steps(ops, TRIP + 64, "trip", "project", "randn", (1000,), late=True, coef=0.37, shadow=False, seed=190)
    grouped_steps(ops, 128, "two", "big-lr", "randn", (1, 2), shadow=False)


def test_kernel_lr_scale_zero_only_leaves_the_moments_moving(ops):
    """lr_scale 0 (group 2 of SCALES): lr_g = 0, so the parameter is untouched bit for bit while m and v still follow the gradient."""
    n = 320
    bmap_c, ng = _map(n, "every-block")
    lrs, wds = (t.cuda() for t in _tables(ng, 1e-2))
    bufs = _state(n, False, 31)
    p, m, v, sh = (b[1] for b in bufs)
    p0 = p.clone()
    g = torch.randn(n, generator=MR.gen(32)).cuda()
    ops.adamw_groups(p, g, m, v, sh, bmap_c.cuda(), lrs, wds, 1e-2, *MR.ADAMW_BETAS, MR.ADAMW_EPS, 1, 1.0)
    frozen = (bmap_c == 2).repeat_interleave(BLOCK).cuda()
    assert bool(frozen.any()) and torch.equal(p[frozen], p0[frozen]) and bool((p[~frozen] != p0[~frozen]).all())
    assert bool((m[frozen] != 0).all()) and bool((v[frozen] > 0).all())


# ------------------------------------------------------------------ 2. bit identities
def _run_plain(ops, n, hyper, steps, gscale, seed=90, guard=None):
    lr, wd = MR.ADAMW_HYPER[hyper]
    p, m, v, sh = (b[1] for b in _state(n, False, seed))
    for step in steps:
        g = MR.adamw_grad("randn", n, seed + 10 + step)[0].cuda()
        if guard is None:
            ops.adamw(p, g, m, v, sh, lr, *MR.ADAMW_BETAS, MR.ADAMW_EPS, wd, step, gscale)
        else:
            ops.adamw_guarded(p, g, m, v, sh, lr, *MR.ADAMW_BETAS, MR.ADAMW_EPS, wd, step, gscale, *guard)
    return p, m, v, sh


def _run_grouped(ops, n, case, hyper, steps, gscale, tables=None, seed=90, guard=None):
    lr, wd = MR.ADAMW_HYPER[hyper]
    bmap_c, ng = _map(n, case)
    lrs, wds = tables if tables is not None else _tables(ng, wd)
    p, m, v, sh = (b[1] for b in _state(n, False, seed))
    coef, skip = guard if guard is not None else (None, None)
    for step in steps:
        g = MR.adamw_grad("randn", n, seed + 10 + step)[0].cuda()
        ops.adamw_groups(p, g, m, v, sh, bmap_c.cuda(), lrs.cuda(), wds.cuda(), lr, *MR.ADAMW_BETAS, MR.ADAMW_EPS, step, gscale, coef, skip)
    return p, m, v, sh


@pytest.mark.parametrize("hyper", list(MR.ADAMW_HYPER))
@pytest.mark.parametrize("n,case", [(320, "every-block"), (2 * TRIP + 192, "id255")], ids=lambda x: str(x))
def test_groups_of_one_and_the_optimizer_decay_are_mvlt_adamw_bit_for_bit(ops, n, case, hyper):
    """Every group (1.0, wd): the element arithmetic is adamw_sweep's own, so all four buffers equal ops.adamw's."""
    wd = MR.ADAMW_HYPER[hyper][1]
    ng = _map(n, case)[1]
    tables = (torch.ones(ng, dtype=F32), torch.full((ng,), wd, dtype=F32))
    for gscale in (1.0, 1.0 / 1024):
        a = _run_plain(ops, n, hyper, (1, 2, 3), gscale)
        b = _run_grouped(ops, n, case, hyper, (1, 2, 3), gscale, tables)
        for name, x, y in zip(("p", "m", "v", "shadow"), a, b):
            check_equal(y, x, f"grouped (1, wd) vs mvlt_adamw n={n} {hyper} gscale={gscale}: {name}")


def test_guarded_grouped_sweep_follows_the_guarded_contract(ops):
    n, case, hyper = TRIP + 64, "trip", "big-lr-wd"
    one = torch.ones(1, device="cuda")
    half = torch.full((1,), 0.5, device="cuda")
    go = torch.zeros(1, dtype=torch.int32, device="cuda")
    plain = _run_grouped(ops, n, case, hyper, (1, 2), 0.75)
    for name, x, y in zip("pmvs", plain, _run_grouped(ops, n, case, hyper, (1, 2), 0.75, guard=(one, go))):
        check_equal(y, x, f"guarded coef=1 skip=0 vs unguarded grouped: {name}")
    scaled = _run_grouped(ops, n, case, hyper, (1, 2), float(np.float32(0.75) * np.float32(0.5)))
    for name, x, y in zip("pmvs", scaled, _run_grouped(ops, n, case, hyper, (1, 2), 0.75, guard=(half, go))):
        check_equal(y, x, f"guarded coef=0.5 vs unguarded at grad_scale * 0.5: {name}")
    # skip = 1: nothing is written, not even from a NaN gradient
    lr, wd = MR.ADAMW_HYPER[hyper]
    bmap_c, ng = _map(n, case)
    lrs, wds = (t.cuda() for t in _tables(ng, wd))
    bufs = _state(n, True, 190)
    p, m, v, sh = (b[1] for b in bufs)
    sh.copy_(p)
    before = [t.clone() for t in (p, m, v, sh)]
    g = torch.randn(n, generator=MR.gen(5)).cuda()
    g[5] = float("nan")
    stop = torch.ones(1, dtype=torch.int32, device="cuda")
    ops.adamw_groups(p, g, m, v, sh, bmap_c.cuda(), lrs, wds, lr, *MR.ADAMW_BETAS, MR.ADAMW_EPS, 3, 1.0, one, stop)
    torch.cuda.synchronize()
    for x, y in zip(before, (p, m, v, sh)):
        assert torch.equal(x, y)
    _check_guards(bufs, "skipped grouped sweep")


# ------------------------------------------------------------------ 3. the grid
def grid_run(ops):
    return [t.cpu() for t in grouped_steps(ops, TRIP + 64, "trip", "big-lr-wd", "randn", (1, 2, 3), check=False)]


def test_grid_does_not_matter(ops, tmp_path):
    """MVLT_ADAMW_BLOCKS=3 (read once per process: a fresh child, tests/param_groups_worker.py) takes n = 524288 + 64 through 171
    trips of a three-workgroup grid instead of two of the default one; the sweep is elementwise and the LDS tables are staged per
    workgroup, so p, m, v and the shadow equal the default grid's bit for bit."""
    path = str(tmp_path / "groups_blocks3.pt")
    env = dict(os.environ)
    env["MVLT_ADAMW_BLOCKS"] = "3"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "param_groups_worker.py"), path], env=env,
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0 and "ADAMW-GROUPS-GRID-OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    theirs = torch.load(path)
    for name, a, b in zip(("p", "m", "v", "shadow"), grid_run(ops), theirs):
        check_equal(a, b, f"adamw_groups default grid vs MVLT_ADAMW_BLOCKS=3: {name}")


# ------------------------------------------------------------------ 4. the optimizer on the tiny pre-training model
LR, WD = 1e-3, 0.1
SEEDS, FLIPS = (71, 72, 73), (0.9, 0.1, 0.9)          # the live set and the run plan change between steps
MAX_NORM = 0.01


def _cfg(M):
    cfg = M.MVLBertPretrainConfig(hidden_size=256, num_hidden_layers=2, num_attention_heads=4, intermediate_size=1024, vocab_size=3000)
    cfg.swin.update(embed_dim=32, depths=[2, 2, 2, 2], num_heads=[1, 2, 4, 8], drop_path_rate=0.2)
    cfg.ITM_task = True
    return cfg


def _model(M, cd=F32):
    with open(os.path.join(ROOT, "tests", "golden", "specs_hash.json")) as f:
        spec = json.load(f)["hash_tiny_pretrain"]
    model = M.MVLBertForPretraining(_cfg(M))
    model.load_state_dict(hash_sd(spec), strict=False)
    return M.set_compute_dtype(model.cuda().eval(), cd)


def _batch(seed):
    return tuple(t.cuda() for t in synth_batch(4, 24, seed=seed, vocab=3000))


@contextlib.contextmanager
def _coin(value):
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
    m = torch.zeros(ar.total, dtype=torch.bool)
    for p in ar.params:
        if ar.has_grad[id(p)]:
            m[ar.offset[id(p)]:ar.offset[id(p)] + p.numel()] = True
    return m


def _steps(ar):
    return {n: ar.steps[id(p)] for n, p in zip(ar.names, ar.params)}


def _groups(model):
    from mvlt_amd.optim import no_decay_rules, param_groups_by_name
    return param_groups_by_name(model, [(r"^conv\.", dict(lr_scale=0.1))] + no_decay_rules())


def _run(M, kw, cd=F32, replay=None, grouped=True, overlap=False, schedule=None, seeds=SEEDS, flips=FLIPS, model=None, opt=None, first=0):
    """len(seeds) optimizer steps of FusedAdamW(lr=LR, weight_decay=WD, param_groups=the no-decay + backbone groups, **kw)."""
    from mvlt_amd.optim import FusedAdamW, LRSchedule
    model = _model(M, cd) if model is None else model
    if opt is None:
        opt = FusedAdamW(model, lr=LR, weight_decay=WD, param_groups=_groups(model) if grouped else None, **kw)
        if overlap:
            opt.overlap_with_backward()
            opt._overlap["chunk"] = (64 << 10) // 4          # many slices even on the tiny model
    sch = LRSchedule(opt, **schedule) if isinstance(schedule, dict) else schedule
    out = dict(model=model, opt=opt, sch=sch, grads=[], live=[], lrs=[])
    for i, (seed, flip) in enumerate(zip(seeds, flips)):
        ar_before = _arena(model)
        if i == 0:
            out["p0"] = ar_before.flat.clone()
        ar = _backward(model, _batch(seed), flip)
        assert ar is ar_before
        if replay is not None:
            ar.grad.copy_(replay[first + i])
        out["grads"].append(ar.grad.clone())
        out["live"].append(_live(ar))
        out["lrs"].append(opt.lr)
        opt.step()
        if sch is not None:
            sch.step()
    opt.flush()
    torch.cuda.synchronize()
    out["ar"] = _arena(model)
    return out


def _reference(run, grouped=True, max_grad_norm=None):
    ar, opt = run["ar"], run["opt"]
    scale_v, wd_v = PG.element_hyper(ar, opt) if grouped else (torch.ones(ar.total, dtype=torch.float64), WD)
    ref = PG.RefGroupedAdamW(run["p0"], LR * scale_v, wd_v, max_grad_norm=max_grad_norm)
    for g, live, lr in zip(run["grads"], run["live"], run["lrs"]):
        ref.step(g, live, lr=lr * scale_v)          # (run["lrs"]: opt.lr when the step was launched -- a schedule moves it)
    return ref


def _ref_steps(ar, ref):
    return {n: int(ref.steps[ar.offset[id(p)]]) for n, p in zip(ar.names, ar.params)}


@pytest.fixture(scope="module")
def grouped_run(M):
    return _run(M, {})


def _equal_state(a, b):
    assert torch.equal(a.flat, b.flat) and torch.equal(a.exp_avg, b.exp_avg) and torch.equal(a.exp_avg_sq, b.exp_avg_sq)
    assert (a.shadow is None) == (b.shadow is None) and (a.shadow is None or torch.equal(a.shadow, b.shadow))
    assert _steps(a) == _steps(b)


def test_the_test_model_has_the_four_groups_and_changing_runs(grouped_run):
    opt, ar = grouped_run["opt"], grouped_run["ar"]
    assert sorted((g["lr_scale"], g["weight_decay"]) for g in opt.param_groups) == [(0.1, 0.0), (0.1, WD), (1.0, 0.0), (1.0, WD)]
    t = opt._tables
    assert t is not None and t["map"].is_cuda and t["map"].numel() * BLOCK == ar.total and sorted(set(t["map"].tolist())) == [0, 1, 2, 3]
    assert not torch.equal(grouped_run["live"][0], grouped_run["live"][1])          # the coin flips change the live set
    assert len(set(_steps(ar).values())) >= 3                                        # heads at 1 and 2 steps, idle parameters at 0


@pytest.mark.parametrize("cd", [F32, BF16], ids=["f32", "bf16"])
def test_grouped_steps_match_the_reference_and_see_the_groups(M, grouped_run, cd):
    run = grouped_run if cd == F32 else _run(M, {}, cd=cd)
    ar = run["ar"]
    got = ar.flat.cpu()
    ref, plain = _reference(run), _reference(run, grouped=False)
    e_grouped, e_plain = rel_err(got, ref.p), rel_err(got, plain.p)
    print(f"{cd}: vs grouped reference {e_grouped:.3e}, vs ungrouped reference {e_plain:.3e}")
    assert e_grouped < 1e-6
    assert e_plain > 10 * 1e-6
    # the moments: the kernel carries the betas as f32, and 1 - f32(0.999) is 1.29e-5 away (relative) from the reference's
    # fp64 0.001, 1 - f32(0.9) 2.4e-7 from 0.1 -- the plain sweep's own offsets, far below what a wrong group would leave in p
    assert rel_err(ar.exp_avg.cpu(), ref.m) < 1e-6 and rel_err(ar.exp_avg_sq.cpu(), ref.v) < 1e-4
    assert _steps(ar) == _ref_steps(ar, ref)
    assert (ar.shadow is not None) == (cd == BF16)
    if cd == BF16:
        assert torch.equal(ar.shadow, ar.flat.to(BF16))


def test_clipped_grouped_steps_match_the_reference(M):
    run = _run(M, dict(max_grad_norm=MAX_NORM))
    ref = _reference(run, max_grad_norm=MAX_NORM)
    assert ref.last_norm > 10 * MAX_NORM
    got = run["ar"].flat.cpu()
    assert rel_err(got, ref.p) < 1e-6
    assert rel_err(got, _reference(run, grouped=False, max_grad_norm=MAX_NORM).p) > 10 * 1e-6
    assert abs(run["opt"].last_grad_norm.item() - ref.last_norm) <= 2.0 ** -22 * ref.last_norm
    assert _steps(run["ar"]) == _ref_steps(run["ar"], ref)


def test_skipped_grouped_step_never_happened(M, grouped_run):
    """skip_nonfinite beside param_groups: a finite step equals the plain grouped one bit for bit (coef = 1, skip = 0), a poisoned
    one writes nothing and gives its step counts back."""
    from mvlt_amd.optim import FusedAdamW
    model = _model(M)
    opt = FusedAdamW(model, lr=LR, weight_decay=WD, param_groups=_groups(model), skip_nonfinite=True)
    twin = _run(M, {}, seeds=SEEDS[:1], flips=FLIPS[:1], replay=grouped_run["grads"])
    ar = _backward(model, _batch(SEEDS[0]), FLIPS[0])
    ar.grad.copy_(grouped_run["grads"][0])
    opt.step()
    assert opt.steps_skipped == 0
    _equal_state(twin["ar"], ar)
    before, steps_before = [t.clone() for t in (ar.flat, ar.exp_avg, ar.exp_avg_sq)], _steps(ar)
    _backward(model, _batch(SEEDS[1]), FLIPS[1])
    p = next(p for n, p in model.named_parameters() if p.grad is not None and n.endswith("intermediate.dense.weight"))
    p.grad.view(-1)[p.numel() // 2] = float("nan")                  # plain data: nothing faults
    opt.step()
    assert opt.steps_skipped == 1
    for x, y in zip(before, (ar.flat, ar.exp_avg, ar.exp_avg_sq)):
        assert torch.equal(x, y)
    assert _steps(ar) == steps_before


def test_deferred_tail_equals_the_plain_grouped_run(M, grouped_run):
    from mvlt_amd.optim import FusedAdamW, _OptTail
    seen = []
    real = _OptTail._run

    def spy(self, ch):
        seen.append(ch["lo"])
        return real(self, ch)
    _OptTail._run = spy
    try:
        got = _run(M, dict(defer_tail=True), replay=grouped_run["grads"])
    finally:
        _OptTail._run = real
    assert seen, "nothing was deferred"
    _equal_state(grouped_run["ar"], got["ar"])


def test_overlapped_grouped_steps_match_the_reference(M):
    calls = []
    from mvlt_amd import ops
    real = ops.adamw_groups

    def spy(*a, **k):
        calls.append(ops._stream().value == ops.opt_stream(a[0].device).cuda_stream)
        return real(*a, **k)
    ops.adamw_groups = spy
    try:
        run = _run(M, {}, overlap=True)
    finally:
        ops.adamw_groups = real
    assert any(calls), "no sweep ran on the optimizer stream during the backward pass"
    ref = _reference(run)
    assert rel_err(run["ar"].flat.cpu(), ref.p) < 1e-6
    assert rel_err(run["ar"].flat.cpu(), _reference(run, grouped=False).p) > 10 * 1e-6
    assert _steps(run["ar"]) == _ref_steps(run["ar"], ref)


def test_without_param_groups_nothing_changes(M, grouped_run):
    """param_groups=None never reaches the new entry point, and the run equals the plain launches (ops.adamw per run of the plan,
    as before this feature) bit for bit on replayed gradients."""
    from mvlt_amd import ops
    from mvlt_amd.optim import FusedAdamW
    count = [0]
    real = ops.adamw_groups

    def spy(*a, **k):
        count[0] += 1
        return real(*a, **k)
    ops.adamw_groups = spy
    try:
        got = _run(M, {}, grouped=False, replay=grouped_run["grads"])
    finally:
        ops.adamw_groups = real
    assert count[0] == 0 and got["opt"]._tables is None
    assert got["opt"].param_groups == [dict(lr=LR, lr_scale=1.0, weight_decay=WD, names=[n for n, _ in got["model"].named_parameters()])]
    # today's plain run, spelled out: one ops.adamw per planned run
    model = _model(M)
    opt = FusedAdamW(model, lr=LR, weight_decay=WD)
    for i, (seed, flip) in enumerate(zip(SEEDS, FLIPS)):
        ar = _backward(model, _batch(seed), flip)
        ar.grad.copy_(grouped_run["grads"][i])
        st = opt._state()
        assert st is ar
        for lo, hi, ids in opt._plan_runs(ar, [p for p in ar.params if ar.has_grad[id(p)]]):
            ops.adamw(ar.flat[lo:hi], ar.grad[lo:hi], ar.exp_avg[lo:hi], ar.exp_avg_sq[lo:hi], None, LR, 0.9, 0.999, 1e-6, WD,
                      ar.steps[ids[0]] + 1, 1.0)
        ar.bump_steps()
        ar.note_params_written_by_kernel()
        ar.note_grads_consumed()
    torch.cuda.synchronize()
    _equal_state(ar, got["ar"])
    assert rel_err(got["ar"].flat.cpu(), _reference(got, grouped=False).p) < 1e-6


# ------------------------------------------------------------------ 5. the schedule through PretrainStep
@pytest.mark.parametrize("defer", [False, True], ids=["plain", "deferred-tail"])
def test_every_launch_runs_at_the_lr_of_its_step(M, defer):
    from mvlt_amd.optim import FusedAdamW, LRSchedule
    from mvlt_amd.train import PretrainStep
    model = _model(M)
    step = PretrainStep(model, lr=LR, defer_optimizer_tail=defer, param_groups=_groups(model),
                        lr_schedule=dict(warmup_steps=2, total_steps=6, kind="cosine", min_ratio=0.1))
    assert isinstance(step.schedule, LRSchedule) and step.opt.defer_tail == defer
    want = [LR * step.schedule.factor(t) for t in range(4)]
    assert want[0] == 0.0 and want[1] == LR / 2 and want[2] == LR and want[3] < LR
    seen, call = [], [0]
    real = FusedAdamW._launch

    def spy(self, ar, lo, hi, st, hyper, guard=None):
        seen.append((call[0], st, hyper[0]))
        return real(self, ar, lo, hi, st, hyper, guard)
    FusedAdamW._launch = spy
    try:
        with _coin(0.9):                                    # one live set: every launch of step k carries step count k
            for k in range(4):
                call[0] = k
                step(_batch(71 + k))
                assert step.opt.lr == LR * step.schedule.factor(k + 1)
            call[0] = 4
            step.flush()
    finally:
        FusedAdamW._launch = real
    torch.cuda.synchronize()
    assert {st for _, st, _ in seen} == {1, 2, 3, 4}
    for when, st, lr in seen:
        assert lr == want[st - 1], (when, st, lr, want)
    late = [(when, st) for when, st, _ in seen if when != st - 1]
    if defer:
        assert late and all(when == st for when, st in late)          # the tail of step k ran during call k + 1, at step k's lr
    else:
        assert not late


# ------------------------------------------------------------------ 6. checkpoint
def test_resume_from_a_checkpoint_equals_the_uninterrupted_run(M, tmp_path):
    from mvlt_amd.optim import FusedAdamW, LRSchedule
    sched = dict(warmup_steps=1, total_steps=5, kind="linear", min_ratio=0.1)
    whole = _run(M, {}, schedule=sched)
    assert len(set(whole["lrs"])) == 3
    assert rel_err(whole["ar"].flat.cpu(), _reference(whole).p) < 1e-6
    head = _run(M, {}, schedule=sched, seeds=SEEDS[:2], flips=FLIPS[:2], replay=whole["grads"])
    path = str(tmp_path / "ckpt")
    head["model"].save_pretrained(path)
    torch.save(dict(opt=head["opt"].state_dict(), sch=head["sch"].state_dict()), os.path.join(path, "opt.pt"))
    model = M.MVLBertForPretraining.from_pretrained(path, config=_cfg(M))
    model = M.set_compute_dtype(model.cuda().eval(), F32)
    opt = FusedAdamW(model, lr=123.0, weight_decay=7.0)                # everything comes from the checkpoint
    sch = LRSchedule(opt, **sched)
    sd = torch.load(os.path.join(path, "opt.pt"))
    opt.load_state_dict(sd["opt"])
    sch.load_state_dict(sd["sch"])
    assert [dict(g, lr=None) for g in opt.param_groups] == [dict(g, lr=None) for g in whole["opt"].param_groups]
    assert opt.lr == whole["lrs"][2] and opt.weight_decay == WD
    tail = _run(M, {}, schedule=sch, seeds=SEEDS[2:], flips=FLIPS[2:], replay=whole["grads"], model=model, opt=opt, first=2)
    _equal_state(whole["ar"], tail["ar"])
