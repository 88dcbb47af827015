"""A whole Swin block, x2 = x1 + s2 Mlp(norm2 x1) with x1 = x + s1 proj(W-MSA(qkv(norm1 x))), and its backward, with BOTH
DropPath scales live, on every route and both host paths: swin.py _block_fwd / _block_bwd with ops.NATIVE true (csrc/host.cpp
swin_block_fwd / swin_block_bwd, the Mlp half on the kept rows only or dense) and false (the Python launches).

tests/test_swin_attn_half_gpu.py (s2 = 0) and tests/test_swin_droppath_compact_gpu.py (s1 = 0) each switch one half off, which
makes x1 == x or dx1 == dx2 and hides every fault that confuses them.  Here the block functions are called directly with
hand-made s1 != s2, both mixed (KEEP), and every run is judged per element against the float64 reference of
tests/swin_block_ref.py (its docstring states the stages and the bounds; tests/test_swin_block_cpu.py shows which wiring faults
they reject): the twelve saved tensors and x2 stage by stage from the operand the kernel read; dx0, the thirteen parameter
gradients and the hand-off dx0 s2_next twice --
  chained   from dx2 through float64 values of the seven intermediates nobody returns, each bound carrying its input's bound;
  cut       every backward stage from the STORED intermediate of a replay: the test issues the launch list of swin.py
            _block_bwd one by one through mvlt_amd.ops on the run's own saved tensors.  The replayed dy2, dh, dxn2, dx1, dyw,
            dqkv and dxn1w are judged one stage deep themselves, and what the block returns is judged one stage deep from them.
            A compact run's two Mlp dgrads are replayed as that run issued them (the plan's row order, the device row count)
            and their outputs moved to logical order, an exact move: replayed densely, the res 7 / C 768 products take another
            GEMM route than the block's own (a device row count refuses some), whose f32 sums round differently -- measured
            2 .. 6 of the 768 columns of dxn2 hold one element that differs by one bf16 step, which a bound one stage deep
            behind dxn2 does not absorb (dx0 at 77 to 102 times its bound, qkv.weight at 313).
Routes are switched with monkeypatch on ops.NATIVE and the swin switches, which are read at call time (_DROP_COMPACT too:
test_drop_compact_is_read_at_call_time); every case first asserts the route it got (swin._wmsa_mode, swin._bwd_mode, compact
or dense by the length of what the forward saved) and prints it beside its worst ratios.  NaN blocks of the intermediate sizes
are handed back to the caching allocator before each call and every output must be finite.
Between runs of the same inputs: native and Python on the same dense route are bit-equal in everything saved and returned;
any two runs (compact against dense, one route against another) differ by at most their two bounds plus the distance of
their float64 values.
The consumer side of the hand-off (test_consumer_takes_the_producers_branch_gradient): block 1's backward with s2_next = block
0's s2 forms `pre` in block 0's `inv` order; block 0's backward then runs with dy2_pre = pre and with None, compact and dense,
and all four meet the reference; `pre` itself is judged against block 1's dx0 s2_next.  A dy2_pre of a wrong shape or dtype is
refused on the host before any launch (test_bad_hand_off_is_refused_on_the_host).
No hand-off timeout is shortened, no CU is held, no failure path of a kernel is provoked; the largest launch is the 128
workgroups of the second design.

Measured on an MI355X, worst ratio to the bound over every route, host path, keep pattern and the hand-off runs
(test_worst_ratios_summary prints them; each case prints its own).  bf16 forward: xn1w / xn2 0.50, mean 0.003, rstd 0.03, qkv
0.99, ao 0.43, lse 0.02, x1 0.99, h / act 0.99, x2 0.99.  bf16 cut backward: dy2 0.74, dh 0.99, dxn2 0.98, dx1 / dyw / dx0
0.50, dqkv 0.39, dxn1w 0.96, dx0 s2_next 0.33, dbias_table 0.06, the eight weight and bias gradients 0.002 .. 0.036, the four
LayerNorm gradients at most 0.006.  bf16 chained backward: fc2.weight 0.39, fc1.weight 0.28, fc2.bias 0.19, fc1.bias 0.16,
proj.weight 0.15, proj.bias 0.09, dx0 0.025, everything behind the attention backward at most 0.006.  f32: at most 0.06
everywhere except the replayed dh 0.65 (ERFC_ABS against the A&S erfc inside gelu'(h), tests/test_bert_layer_gpu.py), dy2
0.42 and dx0 s2_next 0.17.  The pattern is that of the two half files: a GEMM output judged one stage deep stands at 0.96 ..
0.99 because gemm_ref's bound has no safety factor and its leading term is the rounding of the output itself; LayerNorm
outputs stand at 0.50 (SAFETY = 2 over the same rounding); sums over rows and chained tensors stand far below.
The file takes 5.2 s alone (59 tests; the first case pays 1.9 s of start-up, no other exceeds 0.2 s)."""
import math

import pytest
import torch

import attn_ref as A
import ln_ref as R
import misc_ref as Mi
import swin_block_ref as S
from swin_block_ref import BF, F32

pytestmark = pytest.mark.gpu

DROP_P = 0.25
# name -> (res, C, B, dtype, shifts, [(asked (forward, backward), native, compact asked, (forward, backward) the block must take)])
GEOMS = {
    "r14-C384-B16": (14, 384, 16, BF, (0, 3), [((2, 2), True, True, (2, 2)), ((2, 2), True, False, (2, 2)),
                                               ((1, 1), True, False, (1, 1)), ((0, 0), False, False, (0, 0)),
                                               ((2, 2), False, False, (2, 2))]),
    "r7-C768-B4": (7, 768, 4, BF, (0,), [((2, 2), True, True, (0, 0)), ((2, 2), True, False, (0, 0)), ((2, 2), False, False, (0, 0))]),
    "r14-C96-B16": (14, 96, 16, BF, (0,), [((2, 2), True, False, (2, 2)), ((2, 2), False, False, (2, 2))]),
    "r14-C192-B16": (14, 192, 16, BF, (3,), [((2, 2), True, False, (2, 2)), ((2, 2), False, False, (2, 2))]),
    "r14-C96-B2-f32": (14, 96, 2, F32, (0,), [((1, 0), True, False, (1, 0)), ((1, 0), False, False, (1, 0))]),
    "r14-C384-B2-f32": (14, 384, 2, F32, (3,), [((1, 0), True, False, (1, 0)), ((1, 0), False, False, (1, 0))]),
}


def keep(B, which):
    """0 / 1 per sample.  "a": first and last dropped and every b % 5 == 3; "b": the first dropped and every b % 3 == 1 -- together
    a sample dropped by both (0, and 13 at B = 16), by one only, and kept by both; B = 2: one each."""
    if B == 2:
        return [0.0, 1.0] if which == "a" else [1.0, 0.0]
    if which == "a":
        return [0.0 if b in (0, B - 1) or b % 5 == 3 else 1.0 for b in range(B)]
    return [0.0 if b == 0 or b % 3 == 1 else 1.0 for b in range(B)]


# pattern -> (s1, s2) as keep lists, None (no scales) or a constant
KEEP = {"mixed": ("a", "b"), "s2-all-kept": ("a", 1.0), "s2-all-dropped": ("a", 0.0), "s1-none": (None, "b"), "both-none": (None, None)}
EXTRA_PATTERNS = {"r14-C384-B16": 3, "r7-C768-B4": 0}       # geometry -> the shift whose native runs take every pattern
CASES = []
for _g, _v in GEOMS.items():
    for _shift in _v[4]:
        for _ask, _native, _compact, _ in _v[5]:
            CASES.append((_g, _shift, _ask, _native, _compact, "mixed"))
            if _native and _ask == (2, 2) and EXTRA_PATTERNS.get(_g) == _shift:
                CASES += [(_g, _shift, _ask, _native, _compact, p) for p in KEEP if p != "mixed"]
GROUPS = sorted({(c[0], c[1], c[5]) for c in CASES})


def case_id(c):
    return "%s-s%d-fwd%d-bwd%d-%s-%s-%s" % (c[0], c[1], c[2][0], c[2][1], "native" if c[3] else "python", "compact" if c[4] else "dense", c[5])


COMPARED = ("x1", "x2", "dx0") + S.GRADS          # what any two runs of the same inputs share, whatever their routes
_towers, _runs, _worst = {}, {}, {}


def tower(res, C, dt):
    """One stage of two blocks at resolution `res` (block 0 at shift 0, block 1 at shift 3 when res > 7), as the towers of
    tests/test_swin_attn_half_gpu.py: one-dimensional parameters away from 0 / 1, bias tables with std 0.5, LOGIT_STD logits --
    and Mlp weights of std fan_in^-0.5 like the projections', so that |dx1 - dx2| is of the order of |dx2|
    (tests/test_swin_block_cpu.py test_inputs_make_the_halves_differ)."""
    if (res, C, dt) not in _towers:
        import mvlt_amd as M
        from mvlt_amd.arena import Arena
        from mvlt_amd.swin import SwinTransformer
        torch.manual_seed(41)
        m = SwinTransformer(img_size=4 * res, embed_dim=C, depths=[2], num_heads=[C // 32], num_classes=0, drop_path_rate=0.3)
        g = torch.Generator().manual_seed(42)
        for n, p in m.named_parameters():
            if p.dim() == 1:
                p.data.copy_((1.0 if n.endswith(("norm1.weight", "norm2.weight", "norm.weight")) else 0.0)
                             + 0.1 * torch.randn(p.shape, generator=g))
        for blk in m.layers[0].blocks:
            at = blk.attn
            w = torch.randn(3 * C, C, generator=g) * C ** -0.5
            w[:2 * C] *= math.sqrt(A.LOGIT_STD)
            at.qkv.weight.data.copy_(w)
            at.proj.weight.data.copy_(torch.randn(C, C, generator=g) * C ** -0.5)
            at.relative_position_bias_table.data.copy_(0.5 * torch.randn(169, C // 32, generator=g))
            blk.mlp.fc1.weight.data.copy_(torch.randn(4 * C, C, generator=g) * C ** -0.5)
            blk.mlp.fc2.weight.data.copy_(torch.randn(C, 4 * C, generator=g) * (4 * C) ** -0.5)
        m = M.set_compute_dtype(m.cuda().train(), dt)
        ar = Arena.of(m, dt)
        ar.refresh_shadow(tail=False)
        _towers[res, C, dt] = (m, ar)
    return _towers[res, C, dt]


def poison(shapes, dt, device):
    ts = [torch.full(s, float("nan"), dtype=dt, device=device) for s in shapes]
    torch.cuda.synchronize()
    del ts


def set_route(mp, ask, native, compact):
    from mvlt_amd import ops, swin
    mp.setattr(ops, "NATIVE", native)
    mp.setattr(swin, "_FUSED_WMSA", "0" if ask[0] == 0 else "1")
    mp.setattr(swin, "_WMSA2", ask[0] == 2)
    mp.setattr(swin, "_SWIN_BWD_ONE", 96 if ask[1] == 2 else 1 << 30)
    mp.setattr(swin, "_SWIN_BWD_PROJ", ask[1] >= 1)
    mp.setattr(swin, "_DROP_COMPACT", compact)


def scales(B, pattern, dev):
    def one(k):
        if k is None:
            return None
        v = [k] * B if isinstance(k, float) else keep(B, k)
        return (torch.tensor(v) / (1.0 - DROP_P)).to(dev)
    return tuple(one(k) for k in KEEP[pattern])


def params_of(ar, blk):
    at, mlp = blk.attn, blk.mlp
    return dict(gamma1=blk.norm1.weight.data, beta1=blk.norm1.bias.data, wqkv=ar.compute(at.qkv.weight), bqkv=at.qkv.bias.data,
                wproj=ar.compute(at.proj.weight), bproj=at.proj.bias.data, table=at.relative_position_bias_table.data,
                gamma2=blk.norm2.weight.data, beta2=blk.norm2.bias.data, w1=ar.compute(mlp.fc1.weight), b1=mlp.fc1.bias.data,
                w2=ar.compute(mlp.fc2.weight), b2=mlp.fc2.bias.data)


def grads_of(ar, blk):
    at, mlp = blk.attn, blk.mlp
    ps = (("norm1.weight", blk.norm1.weight), ("norm1.bias", blk.norm1.bias), ("qkv.weight", at.qkv.weight), ("qkv.bias", at.qkv.bias),
          ("proj.weight", at.proj.weight), ("proj.bias", at.proj.bias), ("dbias_table", at.relative_position_bias_table),
          ("fc1.weight", mlp.fc1.weight), ("fc1.bias", mlp.fc1.bias), ("fc2.weight", mlp.fc2.weight), ("fc2.bias", mlp.fc2.bias),
          ("norm2.weight", blk.norm2.weight), ("norm2.bias", blk.norm2.bias))
    return {name: ar.grad_view(p).view(p.shape) for name, p in ps}


def saved_of(sv, native):
    """{name: tensor} of what a forward saved: the two host paths keep it in different tuples (csrc/host.cpp swin_block_fwd,
    swin.py _block_fwd); a compact forward appends its plan."""
    if native:
        assert len(sv) == 6 and len(sv[1]) in (11, 14)
        x, stat1, xn1w, qkv, ao, lse, x1, stat2, xn2, h, act = sv[1][:11]
        out = dict(x=x, mean1=stat1[0], rstd1=stat1[1], xn1w=xn1w, qkv=qkv, ao=ao, lse=lse, x1=x1, mean2=stat2[0], rstd2=stat2[1],
                   xn2=xn2, h=h, act=act)
        if len(sv[1]) == 14:
            out.update(perm=sv[1][11], inv=sv[1][12], count=sv[1][13])
        return out
    assert len(sv) == 18
    return dict(zip(("x", "mean1", "rstd1", "xn1w", "qkv", "ao", "lse", "x1", "mean2", "rstd2", "xn2", "h", "act"), sv[1:14]))


def forward(m, ar, blk, x, B, res, s1, s2, dt):
    rows, C = x.shape
    poison([(rows, 3 * C), (rows, C), (rows, C), (rows, 4 * C), (rows, 4 * C)], dt, x.device)
    return m._block_fwd(ar, blk, x, B, res, res, s1, s2, True)


def backward(m, ar, blk, sv, dx2, B, res, native, nparts, dy2_pre=None, s2_next=None):
    """One _block_bwd with everything that completes it (deferred reduces, the side stream) -> (dx0, dy2n, the gradients)."""
    from mvlt_amd import ops
    rows, C = dx2.shape
    dev = dx2.device
    ar.begin_backward()
    ar.grad_view(blk.attn.relative_position_bias_table).zero_()
    lnq = None
    if not native:
        lnq = m.__dict__["_lnq"] = ops.LnReduceQueue()
    poison([(rows, 3 * C), (rows, C), (nparts * rows, C), (rows, 4 * C), (rows, C), (rows, C)], dx2.dtype, dev)
    dx0, dy2n = m._block_bwd(ar, sv, dx2, B, dy2_pre, s2_next)
    if native:
        ops.host().lnq_flush(ops.stream_int())
    else:
        lnq.flush()
    ops.join_side(dev)
    torch.cuda.synchronize()
    if native:
        ops.host().side_release()
    assert ops.wmsa2_sync_errors() == 0, "a hand-off wait of mvlt_swin_wmsa2_fwd ran out"
    return dx0, dy2n, {k: v.detach().clone() for k, v in grads_of(ar, blk).items()}


def replay(run, case, blk, dy2=None):
    """The launch list of swin.py _block_bwd, issued one by one from the definition on the run's own saved tensors -> the seven
    stored intermediates in logical order (dxn1w of backward mode 2 as the sum of its parts, ln_ref.sum_parts).  dy2: the
    producer's branch gradient in the run's own stored row order, when the block used one."""
    from mvlt_amd import _lib as L, ops
    res, C, nH, B, dt, shift, bwd = (case[k] for k in ("res", "C", "nH", "B", "dtype", "shift", "bwd"))
    Lt, nW = res * res, (res // 7) ** 2
    rows = B * Lt
    dev = run["x"].device
    _, n2w = (t.int().to(dev) for t in S.window_maps(B, res, shift))
    s1, s2 = run.get("s1"), run.get("s2")
    if "perm" in run:
        # the two Mlp dgrads as the compact block issues them: the plan's row order, the device row count, zeros behind it
        perm, inv, count = run["perm"], run["inv"].long(), int(run["count"])
        dy2c = dy2 if dy2 is not None else ops.rows_transform(run["dx2"], rowmap=perm, rowscale=(s2, Lt))
        dhc = ops.gemm(dy2c, run["w2"], b_kmajor=True, mul_gelu_grad=run["h"], m_dev=run["count"])
        dxn2 = ops.gemm(dhc, run["w1"], b_kmajor=True, m_dev=run["count"], tail=True)[inv]
        dy2 = dy2c[inv]
        dh = torch.zeros_like(dhc)
        dh[perm.long()[:count]] = dhc[:count]
    else:
        if dy2 is None:
            dy2 = ops.rows_transform(run["dx2"], rowscale=(s2, Lt)) if s2 is not None else run["dx2"]
        dh = ops.gemm(dy2, run["w2"], b_kmajor=True, mul_gelu_grad=run["h"])
        dxn2 = ops.gemm(dh, run["w1"], b_kmajor=True)
    scratch = torch.empty(2, C, dtype=torch.float32, device=dev)
    dx1, dyw = ops.layernorm_bwd(dxn2, run["x1"], run["mean2"].contiguous(), run["rstd2"].contiguous(), run["gamma2"], scratch[0], scratch[1],
                                 dres=run["dx2"], branch=dict(rowmap=n2w, rowscale=(s1, Lt) if s1 is not None else None))
    dtab = torch.zeros(169, nH, dtype=torch.float32, device=dev)
    scale = blk.attn.scale
    if bwd == 2:
        dqkv, parts = ops.swin_wmsa2_bwd(dyw, run["qkv"], run["lse"], B, res, nH, shift, run["wproj"], run["wqkv"], run["table"], scale, dtab)
        dxn1w = R.sum_parts(list(parts))
    else:
        if bwd == 1:
            dao, wp = dyw, run["wproj"]
        else:
            dao, wp = ops.gemm(dyw, run["wproj"], b_kmajor=True), None
        dqkv = ops.attn_bwd(dao, run["qkv"], run["ao"], run["lse"], L.ATTN_SWIN, B * nW, 49, nH, C // nH, scale, dbias_table=dtab,
                            bias_table=run["table"], nW=nW, win_res=res, shift=shift, dout_weight=wp)
        dxn1w = ops.gemm(dqkv, run["wqkv"], b_kmajor=True)
    ops.join_side(dev)
    torch.cuda.synchronize()
    return dict(dy2=dy2, dh=dh, dxn2=dxn2, dx1=dx1, dyw=dyw, dqkv=dqkv, dxn1w=dxn1w)


def inputs(res, C, B, shift, dt, dev):
    g = torch.Generator().manual_seed(2000 + 7 * res + C + B + shift)
    rows = B * res * res
    return torch.randn(rows, C, generator=g).to(dt).to(dev), torch.randn(rows, C, generator=g).to(dt).to(dev)


def check_finite(run, case_name):
    count = int(run["count"]) if "count" in run else None
    for k, v in run.items():
        if torch.is_tensor(v) and v.is_floating_point():
            t = v[:count] if (count is not None and k in ("h", "act")) else v            # rows behind the count are never written
            assert bool(torch.isfinite(t).all()), (case_name, k, "not finite")


def run_case(c):
    """-> (case dict, run dict of device tensors, the replayed stages); the routes are asserted before anything is launched."""
    from mvlt_amd import ops, swin
    geom, shift, ask, native, compact, pattern = c
    res, C, B, dt, _, routes = GEOMS[geom]
    want = next(w for a, n, k, w in routes if (a, n, k) == (ask, native, compact))
    nH, Lt = C // 32, res * res
    dev = torch.device("cuda")
    m, ar = tower(res, C, dt)
    blk = m.layers[0].blocks[1 if shift else 0]
    assert blk.shift_size == shift and blk.window_size == 7 and blk.num_heads == nH
    with pytest.MonkeyPatch.context() as mp:
        set_route(mp, ask, native, compact)
        fwd_mode, bwd_mode = swin._wmsa_mode(dt, B, res, C, nH), swin._bwd_mode(dt, B, res, C, nH, shift)
        assert (fwd_mode, bwd_mode) == want, (case_id(c), "modes", fwd_mode, bwd_mode)
        assert bool(m._drop_compact(C, dt)) == compact, (case_id(c), "compact or dense")
        x, dx2 = inputs(res, C, B, shift, dt, dev)
        s1, s2 = scales(B, pattern, dev)
        s2_next = (torch.tensor([0.0 if b % 4 == 2 else 1.0 for b in range(B)]) / (1.0 - DROP_P)).to(dev) if native else None
        x2, sv = forward(m, ar, blk, x, B, res, s1, s2, dt)
        saved = saved_of(sv, native)
        assert ("perm" in saved) == (compact and s2 is not None), (case_id(c), "compact vs dense by what the forward saved")
        assert saved["x"].data_ptr() == x.data_ptr()
        nparts = max(1, ops.swin_wmsa2_bwd_parts(dt, B, res, C, nH)) if bwd_mode == 2 else 1
        dx0, dy2n, grads = backward(m, ar, blk, sv, dx2, B, res, native, nparts, None, s2_next)
        plan_next = m._dp_plan_of(s2_next, B, Lt, C, dt) if s2_next is not None else None
    run = dict(saved, dx2=dx2, x2=x2, dx0=dx0, **params_of(ar, blk), **grads)
    if s1 is not None:
        run["s1"] = s1
    if s2 is not None:
        run["s2"] = s2
    if s2_next is not None:
        assert dy2n is not None, "the native backward hands dx0 * s2_next back"
        run.update(dy2n=dy2n, s2_next=s2_next)
        assert (plan_next is not None) == compact
        if plan_next is not None:
            run["inv_next"] = plan_next[1]
    run = {k: v.detach().clone() for k, v in run.items()}
    check_finite(run, case_id(c))
    case = dict(res=res, C=C, nH=nH, B=B, dtype=dt, shift=shift, fwd=want[0], bwd=want[1], compact="perm" in run)
    return case, run, replay(run, case, blk)


def note_worst(label, dt, ref):
    for k, v in S.worst_ratios(ref).items():
        key = ("bf16" if dt == BF else "f32", label, k)
        _worst[key] = max(_worst.get(key, 0.0), v)


def judged(c):
    """(case, run, failures, the cut reference of what runs are compared in, its names) of a case, run and judged once per session."""
    if c not in _runs:
        case, run, stages = run_case(c)
        chained = S.reference(run, case)
        cut = S.reference(dict(run, **stages), case)
        print(f"{case_id(c)}: forward mode {case['fwd']}, backward mode {case['bwd']}, {'compact' if case['compact'] else 'dense'}")
        for name, ref in (("chained", chained), ("cut", cut)):
            note_worst(name, case["dtype"], ref)
            print(f"  {name:7s} " + "  ".join(f"{k} {v:.3f}" for k, v in S.worst_ratios(ref).items()))
        bad = S.failures(cut, case_id(c) + " cut")
        bad.update({"chained " + k: v for k, v in S.failures(chained, case_id(c) + " chained").items()})
        assert set(cut) - set(chained) == set(S.STAGES)
        _runs[c] = (case, run, bad, {k: cut[k] for k in COMPARED}, set(cut))
    return _runs[c]


def test_drop_compact_is_read_at_call_time():
    from mvlt_amd import ops, swin
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(ops, "NATIVE", True)
        mp.setattr(swin, "_DROP_COMPACT", True)
        assert swin.SwinTransformer._drop_compact(384, BF) and not swin.SwinTransformer._drop_compact(192, BF)
        assert not swin.SwinTransformer._drop_compact(384, F32)
        mp.setattr(swin, "_DROP_COMPACT", False)
        assert not swin.SwinTransformer._drop_compact(384, BF)
        mp.setattr(swin, "_DROP_COMPACT", True)
        mp.setattr(ops, "NATIVE", False)
        assert not swin.SwinTransformer._drop_compact(384, BF)


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_block_route(c):
    case, run, bad, _, names = judged(c)
    assert not bad, "\n".join(bad.values())
    S.check_dropped_rows(run, case, case_id(c))
    if c[5] == "mixed" and case["B"] > 2:
        d1, d2 = set(S.dropped(run["s1"])), set(S.dropped(run["s2"]))
        assert d1 & d2 and d1 - d2 and d2 - d1 and set(range(case["B"])) - d1 - d2, "both, one only, neither"
        assert {0, case["B"] - 1} <= d1, "first and last sample dropped"
    if c[3]:
        assert "dy2n" in names, "the native path's second output is judged on every native run"


@pytest.mark.parametrize("group", GROUPS, ids=lambda g: "%s-s%d-%s" % g)
def test_runs_of_one_geometry_agree(group):
    """Every run of one (geometry, shift, pattern) shares its inputs.  The two host paths on one dense route launch the same
    kernels on the same operands: whatever they save or return is bit-equal (the bias table of backward modes 0 / 1 is formed
    with float atomics and excepted).  Any other two runs -- compact against dense, one route against another -- each sit
    inside their bound around the float64 value of their OWN saved operands, so they differ by at most the two bounds plus
    the distance of those two values."""
    geom, shift, pattern = group
    cs = [c for c in CASES if (c[0], c[1], c[5]) == group]
    rs = [judged(c) for c in cs]
    for k in ("x", "dx2", "wqkv", "wproj", "w1", "w2", "table", "gamma1", "gamma2"):
        for _, run, _, _, _ in rs[1:]:
            assert torch.equal(run[k], rs[0][1][k]), ("the runs of a group share their inputs", k)
    pairs = 0
    for i in range(len(cs)):
        for j in range(i + 1, len(cs)):
            what = f"{case_id(cs[i])} against {case_id(cs[j])}"
            (ci, ri, _, ui, _), (cj, rj, _, uj, _) = rs[i], rs[j]
            for k in COMPARED:
                (vi, bi, gi), (vj, bj, gj) = ui[k], uj[k]
                over = (gi.double() - gj.double()).abs() > bi + bj + (vi - vj).abs()
                assert not bool(over.any()), (what, k, int(over.sum()), "elements further apart than the two bounds allow")
            if (ci["fwd"], ci["bwd"], ci["compact"]) == (cj["fwd"], cj["bwd"], cj["compact"]) and cs[i][3] != cs[j][3]:
                pairs += 1
                assert not ci["compact"]
                for k in S.SAVED + ("x2", "dx0") + tuple(g for g in S.GRADS if g != "dbias_table" or ci["bwd"] == 2):
                    Mi.check_equal(ri[k], rj[k], f"{what}: {k}")
    if pattern == "mixed":
        assert pairs >= 1, "every geometry runs one dense route on both host paths"


HANDOFF = [("r14-C384-B16", True), ("r14-C384-B16", False), ("r7-C768-B4", True), ("r7-C768-B4", False)]


@pytest.mark.parametrize("geom,compact", HANDOFF, ids=lambda v: v if isinstance(v, str) else ("compact" if v else "dense"))
def test_consumer_takes_the_producers_branch_gradient(geom, compact):
    """Blocks 0 and 1 of a stage, native: x -> block 0 -> block 1, then block 1's backward with s2_next = block 0's s2 forms
    `pre` = dx0 s2 in block 0's `inv` order (dense order when block 0 ran dense), and block 0's backward runs on dx2 = block 1's
    dx0 twice: with dy2_pre = pre and with None.  Both meet the reference, chained and cut (the replay starts from the dy2 the
    block really used); `pre` is judged one stage deep against block 1's dx0 s2_next."""
    from mvlt_amd import ops, swin
    res, C, B, dt, _, _ = GEOMS[geom]
    nH, Lt = C // 32, res * res
    dev = torch.device("cuda")
    m, ar = tower(res, C, dt)
    b0, b1 = m.layers[0].blocks
    want = next(w for a, n, k, w in GEOMS[geom][5] if (a, n, k) == ((2, 2), True, compact))
    with pytest.MonkeyPatch.context() as mp:
        set_route(mp, (2, 2), True, compact)
        modes = [(swin._wmsa_mode(dt, B, res, C, nH), swin._bwd_mode(dt, B, res, C, nH, b.shift_size)) for b in (b0, b1)]
        assert modes[0] == want and modes[1] == want, modes
        x, dx3 = inputs(res, C, B, 5, dt, dev)
        s1a, s2a = scales(B, "mixed", dev)
        s2b, s1b = scales(B, "mixed", dev)                      # block 1: the two patterns the other way round
        x2, sv0 = forward(m, ar, b0, x, B, res, s1a, s2a, dt)
        x3, sv1 = forward(m, ar, b1, x2, B, res, s1b, s2b, dt)
        assert (len(sv0[1]) == 14) == compact and (len(sv1[1]) == 14) == compact
        nparts = max(1, ops.swin_wmsa2_bwd_parts(dt, B, res, C, nH)) if want[1] == 2 else 1
        dx2, pre, g1 = backward(m, ar, b1, sv1, dx3, B, res, True, nparts, None, s2a)
        assert pre is not None
        plan0 = m._dp_plan_of(s2a, B, Lt, C, dt)
        assert (plan0 is not None) == compact
        if compact:
            assert torch.equal(plan0[1], sv0[1][12]), "the producer scatters through the consumer's own inv"
        outs = {}
        for label, given in (("with dy2_pre", pre), ("without", None)):
            outs[label] = backward(m, ar, b0, sv0, dx2, B, res, True, nparts, given, None)
    # ---- block 1, the producer: the whole block and its second output
    case1 = dict(res=res, C=C, nH=nH, B=B, dtype=dt, shift=b1.shift_size, fwd=want[0], bwd=want[1])
    run1 = dict(saved_of(sv1, True), dx2=dx3, x2=x3, dx0=dx2, dy2n=pre, s2_next=s2a, s1=s1b, s2=s2b, **params_of(ar, b1), **g1)
    if compact:
        run1["inv_next"] = plan0[1]
    cut1 = S.reference(dict(run1, **replay(run1, case1, b1)), case1)
    note_worst("cut", dt, cut1)
    print(f"{geom} {'compact' if compact else 'dense'} producer: " + "  ".join(f"{k} {v:.3f}" for k, v in S.worst_ratios(cut1).items()))
    bad = S.failures(cut1, "producer cut")
    assert not bad, "\n".join(bad.values())
    # ---- block 0, the consumer, both ways
    case0 = dict(res=res, C=C, nH=nH, B=B, dtype=dt, shift=b0.shift_size, fwd=want[0], bwd=want[1])
    for label, (dx0, none, g0) in outs.items():
        assert none is None
        run0 = dict(saved_of(sv0, True), dx2=dx2, x2=x2, dx0=dx0, s1=s1a, s2=s2a, **params_of(ar, b0), **g0)
        check_finite(run0, f"consumer {label}")
        if label == "with dy2_pre":
            run0["dy2_pre"] = True
        stages = replay(run0, case0, b0, dy2=pre if label == "with dy2_pre" else None)
        for name, ref in (("chained", S.reference(run0, case0)), ("cut", S.reference(dict(run0, **stages), case0))):
            note_worst(name, dt, ref)
            print(f"{geom} {'compact' if compact else 'dense'} consumer {label} {name}: "
                  + "  ".join(f"{k} {v:.3f}" for k, v in S.worst_ratios(ref).items()))
            bad = S.failures(ref, f"consumer {label} {name}")
            assert not bad, "\n".join(bad.values())
        S.check_dropped_rows(run0, case0, f"consumer {label}")


def test_bad_hand_off_is_refused_on_the_host():
    """s2 given with a dy2_pre of a wrong shape or dtype: TORCH_CHECK on the host, before any launch."""
    from mvlt_amd import ops
    res, C, B, dt = 7, 768, 4, BF
    dev = torch.device("cuda")
    m, ar = tower(res, C, dt)
    blk = m.layers[0].blocks[0]
    with pytest.MonkeyPatch.context() as mp:
        set_route(mp, (2, 2), True, True)
        x, dx2 = inputs(res, C, B, 0, dt, dev)
        s1, s2 = scales(B, "mixed", dev)
        _, sv = forward(m, ar, blk, x, B, res, s1, s2, dt)
        torch.cuda.synchronize()
        ar.begin_backward()
        for wrong in (torch.zeros(B * res * res - 1, C, dtype=dt, device=dev), torch.zeros(B * res * res, C, dtype=torch.float32, device=dev),
                      torch.zeros(B * res * res, 2 * C, dtype=dt, device=dev)[:, :C]):
            with pytest.raises(RuntimeError, match="dy2_pre"):
                m._block_bwd(ar, sv, dx2, B, wrong, None)
        torch.cuda.synchronize()
        ops.host().side_release()


def test_worst_ratios_summary():
    """Prints the worst ratio to the bound per tensor over everything this file ran (the figures of the module docstring)."""
    assert _worst, "runs after the route tests"
    for dtn in ("bf16", "f32"):
        for label in ("chained", "cut"):
            items = sorted((k[2], v) for k, v in _worst.items() if k[0] == dtn and k[1] == label)
            print(f"{dtn} {label}: " + ", ".join(f"{k} {v:.3f}" for k, v in items))
