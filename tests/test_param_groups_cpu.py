"""Host side of parameter groups and LR schedules: the fp64 reference of tests/param_groups_ref.py against torch.optim.AdamW with
torch param groups, no_decay_rules() / param_groups_by_name on the tiny pre-training model's names, the byte map over a CPU arena,
LRSchedule against its closed forms, the refusals, the state_dict round trip and the C-ABI additions (two entry points, no struct, no
ABI bump)."""
import math
import os
import re

import pytest
import torch

import grad_clip_ref as R
import param_groups_ref as PG
from conftest import rel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = torch.float32


# ------------------------------------------------------------------ the reference
def _ref_setup():
    g = torch.Generator().manual_seed(5201)
    shapes = [(37, 11), (64,), (5, 3, 2), (129,)]
    ps = [torch.randn(s, generator=g).double() for s in shapes]
    grads = [[torch.randn(s, generator=g).double() for s in shapes] for _ in range(5)]
    # parameter -> (lr_scale, weight_decay): the default group, one at lr_scale 0.1, one without decay, the default again
    hyper = [(1.0, 0.1), (0.1, 0.1), (1.0, 0.0), (1.0, 0.1)]
    return ps, grads, hyper


def _flat(ts):
    return torch.cat([t.reshape(-1) for t in ts])


def test_reference_equals_torch_adamw_with_param_groups_and_sees_the_groups():
    ps, grads, hyper = _ref_setup()
    LR = 1e-3
    tp = [torch.nn.Parameter(p.clone()) for p in ps]
    opt = torch.optim.AdamW([dict(params=[p], lr=LR * s, weight_decay=wd) for p, (s, wd) in zip(tp, hyper)],
                            lr=LR, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.1)
    lr_v = _flat([torch.full_like(p, LR * s) for p, (s, _) in zip(ps, hyper)])
    wd_v = _flat([torch.full_like(p, wd) for p, (_, wd) in zip(ps, hyper)])
    ref = PG.RefGroupedAdamW(_flat(ps), lr_v, wd_v)
    plain = R.RefAdamW(_flat(ps), lr=LR, weight_decay=0.1)
    for gs in grads:
        for p, g in zip(tp, gs):
            p.grad = g.clone()
        opt.step()
        ref.step(_flat(gs))
        plain.step(_flat(gs))
    want = _flat([p.detach() for p in tp])
    assert rel_err(ref.p, want) < 1e-14
    # scalar hyper-parameters give grad_clip_ref's reference back, and the groups are VISIBLE at the GPU tests' 1e-6 bound
    same = PG.RefGroupedAdamW(_flat(ps), LR, 0.1)
    for gs in grads:
        same.step(_flat(gs))
    assert torch.equal(same.p, plain.p)
    assert rel_err(plain.p, ref.p) > 10 * 1e-6


def test_reference_live_mask_step_counts_clip_and_skip():
    ps, grads, _ = _ref_setup()
    n = _flat(ps).numel()
    live = torch.zeros(n, dtype=torch.bool)
    live[: n // 2] = True
    a = PG.RefGroupedAdamW(_flat(ps), 1e-3, 0.1, max_grad_norm=0.5, skip_nonfinite=True)
    b = R.RefAdamW(_flat(ps), lr=1e-3, weight_decay=0.1, max_grad_norm=0.5, skip_nonfinite=True)
    for k, gs in enumerate(grads[:3]):
        g = _flat(gs)
        if k == 1:
            g = g.clone()
            g[3] = float("nan")
        a.step(g, live if k == 0 else None)
        b.step(g, live if k == 0 else None)
    assert torch.equal(a.p, b.p) and torch.equal(a.steps, b.steps) and a.skipped == b.skipped == 1
    assert a.steps[0] == 2 and a.steps[-1] == 1


# ------------------------------------------------------------------ rules on the tiny pre-training model
@pytest.fixture(scope="module")
def tiny():
    import mvlt_amd as M
    cfg = M.MVLBertPretrainConfig(hidden_size=256, num_hidden_layers=2, num_attention_heads=4, intermediate_size=1024, vocab_size=3000)
    cfg.swin.update(embed_dim=32, depths=[2, 2, 2, 2], num_heads=[1, 2, 4, 8], drop_path_rate=0.2)
    cfg.ITM_task = True
    return M.MVLBertForPretraining(cfg)


def _decay_of(model, groups, default=0.1):
    from mvlt_amd.optim import FusedAdamW
    opt = FusedAdamW(model, lr=1e-3, weight_decay=default, param_groups=groups)
    return {n: g for g in opt.param_groups for n in g["names"]}, opt


def test_no_decay_rules_on_the_tiny_model(tiny):
    from mvlt_amd.optim import no_decay_rules, param_groups_by_name
    of, opt = _decay_of(tiny, param_groups_by_name(tiny, no_decay_rules()))
    named = dict(tiny.named_parameters())
    assert set(of) == set(named)
    seen = dict(bias=0, norm=0, table=0, matrix=0, embedding=0)
    for name, p in named.items():
        wd = of[name]["weight_decay"]
        assert of[name]["lr_scale"] == 1.0 and of[name]["lr"] == 1e-3
        if name.endswith(".bias"):
            assert wd == 0.0, name
            seen["bias"] += 1
        elif "relative_position_bias_table" in name:
            assert wd == 0.0, name
            seen["table"] += 1
        elif re.search(r"(LayerNorm|norm\d?)\.weight$", name):
            assert p.dim() == 1 and wd == 0.0, name
            seen["norm"] += 1
        elif p.dim() >= 2:
            assert wd == 0.1, name
            seen["embedding" if "embeddings" in name else "matrix"] += 1
        else:
            assert wd == 0.0, name              # (any other vector)
    assert all(v > 0 for v in seen.values()), seen
    assert len(opt.param_groups) == 2


def test_rules_compose_into_exactly_four_groups(tiny):
    from mvlt_amd.optim import no_decay_rules, param_groups_by_name
    groups = param_groups_by_name(tiny, [(r"^conv\.", dict(lr_scale=0.1))] + no_decay_rules())
    of, opt = _decay_of(tiny, groups)
    view = opt.param_groups
    assert len(view) == 4
    assert sorted((g["lr_scale"], g["weight_decay"]) for g in view) == [(0.1, 0.0), (0.1, 0.1), (1.0, 0.0), (1.0, 0.1)]
    assert sum(len(g["names"]) for g in view) == len(dict(tiny.named_parameters()))
    for name, p in tiny.named_parameters():
        assert of[name]["lr_scale"] == (0.1 if name.startswith("conv.") else 1.0), name
        assert of[name]["lr"] == 1e-3 * of[name]["lr_scale"]
    assert any(n.startswith("conv.") for n in of) and any(not n.startswith("conv.") for n in of)
    # the first rule that sets a value wins
    first = param_groups_by_name(tiny, [(r"^conv\.", dict(lr_scale=0.1)), (r".", dict(lr_scale=0.5))])
    assert sorted(g["lr_scale"] for g in first) == [0.1, 0.5]
    assert all(n.startswith("conv.") == (g["lr_scale"] == 0.1) for g in first for n in g["names"])


def test_byte_map_covers_every_block_of_every_parameter(tiny):
    from mvlt_amd.arena import ALIGN, Arena
    from mvlt_amd.optim import FusedAdamW, no_decay_rules, param_groups_by_name
    ar = Arena(tiny, F32, allow_cpu=True)
    groups = param_groups_by_name(tiny, [(r"^conv\.", dict(lr_scale=0.1))] + no_decay_rules())
    opt = FusedAdamW(tiny, lr=1e-3, weight_decay=0.1, param_groups=groups)
    t = opt._build_group_tables(ar)
    bmap = t["map"]
    assert bmap.dtype == torch.uint8 and bmap.numel() * ALIGN == ar.total and int(bmap.max()) == 3
    assert t["lr_scale"].dtype == t["weight_decay"].dtype == F32 and t["lr_scale"].numel() == t["weight_decay"].numel() == 4
    view = opt.param_groups
    gid = {n: k for k, g in enumerate(view) for n in g["names"]}
    covered = torch.zeros(bmap.numel(), dtype=torch.bool)
    for name, p in zip(ar.names, ar.params):
        o = ar.offset[id(p)]
        assert o % ALIGN == 0
        blocks = slice(o // ALIGN, (o + p.numel() + ALIGN - 1) // ALIGN)          # padding included
        assert bool((bmap[blocks] == gid[name]).all()), name
        assert not bool(covered[blocks].any())
        covered[blocks] = True
        assert float(t["lr_scale"][gid[name]]) == pytest.approx(view[gid[name]]["lr_scale"], rel=1e-7)
        assert float(t["weight_decay"][gid[name]]) == pytest.approx(view[gid[name]]["weight_decay"], rel=1e-7)
    assert bool(covered.all())
    # the fused QKV weights (and biases) of every BERT layer are still adjacent, and the weights share a group
    off = {n: ar.offset[id(p)] for n, p in zip(ar.names, ar.params)}
    num = {n: p.numel() for n, p in zip(ar.names, ar.params)}
    layers = sorted({n[:-len("query.weight")] for n in off if n.endswith("attention.self.query.weight")})
    assert layers
    for pre in layers:
        for kind in ("weight", "bias"):
            q, k, v = (pre + x + "." + kind for x in ("query", "key", "value"))
            assert off[k] == off[q] + num[q] and off[v] == off[k] + num[k]
            assert gid[q] == gid[k] == gid[v]
    # the run plan does not know about groups: the same runs with and without them
    plain = FusedAdamW(tiny, lr=1e-3, weight_decay=0.1)
    some = [p for i, p in enumerate(ar.params) if i % 7 != 3]
    for params in (list(ar.params), some):
        assert opt._plan_runs(ar, params) == plain._plan_runs(ar, params)
    assert len(opt._plan_runs(ar, list(ar.params))) == 1


# ------------------------------------------------------------------ LRSchedule
class _Opt:
    def __init__(self, lr):
        self.lr = lr


def _closed_form(kind, t, w, n, r):
    if t < w:
        return t / w
    if t >= n:
        return r
    if kind == "constant":
        return 1.0
    if kind == "linear":
        return max(r, (n - t) / (n - w))
    return r + (1 - r) * 0.5 * (1 + math.cos(math.pi * ((t - w) / (n - w))))


@pytest.mark.parametrize("min_ratio", [0.0, 0.1])
@pytest.mark.parametrize("kind", ["linear", "cosine", "constant"])
def test_lr_schedule_follows_the_closed_forms(kind, min_ratio):
    from mvlt_amd.optim import LRSchedule
    base, w, n = 3e-4, 10, 50
    opt = _Opt(base)
    sch = LRSchedule(opt, w, n, kind=kind, min_ratio=min_ratio)
    seen = [opt.lr]                                    # the lr of step 0 is set by the constructor
    for _ in range(n + 5):
        sch.step()
        seen.append(opt.lr)
    for t, lr in enumerate(seen):
        want = base * _closed_form(kind, t, w, n, min_ratio)
        assert abs(lr - want) <= 1e-12 * abs(want), (t, lr, want)
    assert seen[0] == 0.0 and seen[w] == base
    assert all(a < b for a, b in zip(seen[:w], seen[1:w + 1]))
    past = seen[n:]
    if kind == "constant":
        assert all(x == base for x in seen[w:n])
    assert all(a >= b for a, b in zip(seen[w:], seen[w + 1:]))
    assert len(past) == 6 and all(abs(x - base * min_ratio) <= 1e-12 * base for x in past)          # past total_steps: min_ratio
    # state_dict round trip: a fresh schedule over a fresh optimizer continues where this one was
    sch2 = LRSchedule(_Opt(base), w, n, kind=kind, min_ratio=min_ratio)
    for _ in range(17):
        sch2.step()
    sd = sch2.state_dict()
    assert sd == dict(t=17, base_lr=base)
    opt3 = _Opt(123.0)                                 # (e.g. an optimizer whose lr a checkpoint has already restored)
    sch3 = LRSchedule(opt3, w, n, kind=kind, min_ratio=min_ratio)
    sch3.load_state_dict(sd)
    assert opt3.lr == seen[17] and sch3.base_lr == base
    sch3.step()
    assert opt3.lr == seen[18]


def test_lr_schedule_refuses_bad_arguments():
    from mvlt_amd.optim import LRSchedule
    for kw in (dict(warmup_steps=10, total_steps=10), dict(warmup_steps=-1, total_steps=10), dict(warmup_steps=1, total_steps=10, kind="step"),
               dict(warmup_steps=1, total_steps=10, min_ratio=1.5), dict(warmup_steps=1.5, total_steps=10)):
        with pytest.raises(ValueError):
            LRSchedule(_Opt(1e-3), **kw)
    opt = _Opt(1e-3)
    LRSchedule(opt, 0, 10)                             # no warm-up: the first step runs at the base lr
    assert opt.lr == 1e-3


# ------------------------------------------------------------------ refusals
def _lin():
    return torch.nn.Sequential(torch.nn.Linear(3, 3), torch.nn.LayerNorm(3))


def test_param_groups_refusals_name_the_offender():
    from mvlt_amd.optim import FusedAdamW, param_groups_by_name
    m = _lin()
    w = m[0].weight
    with pytest.raises(ValueError, match="0.weight"):
        FusedAdamW(m, param_groups=[dict(params=[w], lr_scale=0.5), dict(names=["0.weight"], weight_decay=0.0)])
    with pytest.raises(ValueError, match="0.weight"):
        FusedAdamW(m, param_groups=[dict(params=[w], names=["0.weight"])])
    with pytest.raises(KeyError, match="nope.weight"):
        FusedAdamW(m, param_groups=[dict(names=["nope.weight"])])
    with pytest.raises(ValueError, match=r"\(2, 5\)"):
        FusedAdamW(m, param_groups=[dict(params=[torch.nn.Parameter(torch.zeros(2, 5))])])
    with pytest.raises(ValueError, match="256"):
        FusedAdamW(m, param_groups=[dict(names=[], lr_scale=1.0 + k) for k in range(256)])          # + the unlisted parameters = 257
    for key in ("lr_scale", "weight_decay"):
        for bad in (-0.1, float("inf"), float("nan"), "1", True):
            with pytest.raises(ValueError, match=key):
                FusedAdamW(m, param_groups=[dict(params=[w], **{key: bad})])
            with pytest.raises(ValueError, match=key):
                param_groups_by_name(m, [(r"weight", {key: bad})])
    with pytest.raises(ValueError, match="betas"):
        FusedAdamW(m, param_groups=[dict(params=[w], betas=(0.9, 0.99))])
    # accepted: 255 groups beside the unlisted parameters; zero is a legal scale and a legal decay
    opt = FusedAdamW(m, param_groups=[dict(names=[], lr_scale=1.0 + k) for k in range(255)])
    assert len(opt.param_groups) == 256
    opt = FusedAdamW(m, lr=1e-3, param_groups=[dict(params=[w], lr_scale=0.0, weight_decay=0)])
    assert opt.param_groups[1] == dict(lr=0.0, lr_scale=0.0, weight_decay=0.0, names=["0.weight"])
    # without param_groups: one entry, everything in it
    assert FusedAdamW(m, lr=1e-3, weight_decay=0.2).param_groups == [
        dict(lr=1e-3, lr_scale=1.0, weight_decay=0.2, names=["0.weight", "0.bias", "1.weight", "1.bias"])]


def test_pretrain_step_passes_groups_and_schedule_through():
    from mvlt_amd.optim import LRSchedule
    from mvlt_amd.train import PretrainStep
    m = _lin()
    step = PretrainStep(m, lr=1e-3)
    assert step.schedule is None and step.opt._groups is None
    step = PretrainStep(m, lr=1e-3, param_groups=[dict(names=["0.bias"], weight_decay=0.0)],
                        lr_schedule=dict(warmup_steps=2, total_steps=10, kind="cosine"))
    assert isinstance(step.schedule, LRSchedule) and step.schedule.opt is step.opt and step.opt.lr == 0.0
    assert [g["names"] for g in step.opt.param_groups] == [["0.weight", "1.weight", "1.bias"], ["0.bias"]]
    step = PretrainStep(m, lr=1e-3, lr_schedule=lambda opt: LRSchedule(opt, 0, 4, kind="linear", min_ratio=0.5))
    assert step.opt.lr == 1e-3 and step.schedule.min_ratio == 0.5
    with pytest.raises(ValueError):
        PretrainStep(m, lr=1e-3, param_groups=[dict(names=["0.bias"], lr_scale=-1.0)])


# ------------------------------------------------------------------ state_dict
def test_state_dict_round_trip_keeps_the_groups(monkeypatch):
    """(The moments need an arena on a GPU: _state / flush are stubbed, the groups are host state.)"""
    from mvlt_amd.optim import FusedAdamW

    class _Ar:
        names, params, offset, steps = [], [], {}, {}
        exp_avg = exp_avg_sq = torch.zeros(1)
    monkeypatch.setattr(FusedAdamW, "_state", lambda self: _Ar)
    monkeypatch.setattr(FusedAdamW, "flush", lambda self: None)
    m = _lin()
    groups = [dict(names=["0.bias", "1.bias"], weight_decay=0.0), dict(params=[m[0].weight], lr_scale=0.25)]
    opt = FusedAdamW(m, lr=1e-3, weight_decay=0.1, param_groups=groups)
    sd = opt.state_dict()
    assert sd["hyper"]["param_groups"] == [dict(names=["0.bias", "1.bias"], lr_scale=1.0, weight_decay=0.0),
                                           dict(names=["0.weight"], lr_scale=0.25, weight_decay=None)]
    fresh = FusedAdamW(m, lr=5.0, weight_decay=0.7)
    assert fresh._groups is None
    fresh.load_state_dict(sd)
    assert fresh.param_groups == opt.param_groups and fresh.lr == 1e-3
    # a checkpoint without the key loads as before: hyper-parameters restored, the groups of the optimizer untouched
    old = dict(hyper=dict(lr=2e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.3), state={})
    for o in (fresh, FusedAdamW(m)):
        before = o._groups
        o.load_state_dict(old)
        assert o._groups == before and o.lr == 2e-3 and o.weight_decay == 0.3
    assert fresh.param_groups[0]["weight_decay"] == 0.3 and fresh.param_groups[1]["weight_decay"] == 0.0
    plain = FusedAdamW(m).state_dict()
    assert "param_groups" not in plain["hyper"]
    bad = dict(hyper=dict(param_groups=[dict(names=["gone.weight"])]), state={})
    with pytest.raises(KeyError, match="gone.weight"):
        FusedAdamW(m).load_state_dict(bad)


# ------------------------------------------------------------------ C-ABI
NEW = ("mvlt_adamw_groups", "mvlt_adamw_groups_block")


def test_new_entry_points_are_bound_and_exported_without_an_abi_bump():
    from mvlt_amd import _lib, arena
    L = _lib.lib()
    with open(os.path.join(ROOT, "include", "mvlt_hip.h")) as f:
        hdr = f.read()
    for name in NEW:
        assert name in _lib.SYMBOLS and getattr(L, name) is not None
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
    assert len(_lib.SYMBOLS["mvlt_adamw_groups"][1]) == 19
    assert int(re.search(r"#define\s+MVLT_ABI_VERSION\s+(\d+)", hdr).group(1)) == 17 == _lib.ABI_VERSION == L.mvlt_version()
    assert re.search(r"MVLT_STRUCT_COUNT = 21\b", hdr) and len(_lib.STRUCTS) == 21
    assert L.mvlt_adamw_groups_block() == arena.ALIGN == 64


def test_adamw_groups_refuses_bad_arguments_before_any_launch():
    """Every MVLT_ERR_ARG case of the contract comment, on host pointers and without a GPU: the checks precede the launch (a valid
    call would launch -- none is made here)."""
    import ctypes as C
    from mvlt_amd import _lib
    L = _lib.lib()
    ERR_ARG = next(k for k, v in _lib.ERRORS.items() if v == "MVLT_ERR_ARG")
    buf = (C.c_double * 64)()
    a = C.addressof(buf)
    a += a % 16
    assert a % 16 == 0
    vp = C.c_void_p
    good = dict(param=a, grad=a, exp_avg=a, exp_avg_sq=a, shadow=0, n=64, block_group=a, lr_scale=a, weight_decay=a, ngroups=1,
                coef=0, skip=0)

    def call(**kw):
        k = dict(good, **kw)
        return L.mvlt_adamw_groups(vp(k["param"]), vp(k["grad"]), vp(k["exp_avg"]), vp(k["exp_avg_sq"]), vp(k["shadow"]), k["n"],
                                   vp(k["block_group"]), vp(k["lr_scale"]), vp(k["weight_decay"]), k["ngroups"],
                                   1e-3, 0.9, 0.999, 1e-6, 1, 1.0, vp(k["coef"]), vp(k["skip"]), vp(0))
    for name in ("param", "grad", "exp_avg", "exp_avg_sq", "block_group", "lr_scale", "weight_decay"):
        assert call(**{name: 0}) == ERR_ARG, name
    for n in (0, 4, 63, 65, 96, -64):
        assert call(n=n) == ERR_ARG, n
    for g in (0, -1, 257, 1000):
        assert call(ngroups=g) == ERR_ARG, g
    for name in ("param", "grad", "exp_avg", "exp_avg_sq"):
        assert call(**{name: a + 4}) == ERR_ARG and call(**{name: a + 8}) == ERR_ARG, name
    assert call(coef=a) == ERR_ARG and call(skip=a) == ERR_ARG
