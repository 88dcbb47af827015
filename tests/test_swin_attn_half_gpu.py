"""The attention half of a Swin block, x1 = x + s1 proj(W-MSA(qkv(norm1(x)))) and its backward, on every route and both host
paths: forward as four launches, mvlt_swin_wmsa_fwd or mvlt_swin_wmsa2_fwd (swin._wmsa_mode 0 / 1 / 2), backward as three
launches, with the projection dgrad inside the attention backward, or mvlt_swin_wmsa2_bwd plus the deferred bias-table reduce
(swin._bwd_mode 0 / 1 / 2), through swin.py _block_fwd / _block_bwd and through csrc/host.cpp swin_block_fwd / swin_block_bwd.

The block functions are called directly with s2 = 0, the mirror image of tests/test_swin_droppath_compact_gpu.py: the block IS
the attention half.  Every run is judged per element against the float64 reference of tests/swin_attn_half_ref.py (its
docstring states the stages, the bounds and the s2 = 0 premises it asserts; tests/test_swin_attn_half_cpu.py shows which
wiring faults those bounds reject and which they cannot see in bf16).  Routes are switched with monkeypatch on ops.NATIVE and
the swin switches, which are read at call time; every case first asserts the route it got (swin._wmsa_mode, swin._bwd_mode
and, for backward modes 0 / 1, ops.attn_route), so a threshold that moves a case off its route fails loudly.  NaN blocks of
the intermediate sizes are handed back to the caching allocator before each call and every output must be finite.

Between runs, which are free because the inputs are identical: the native and the Python path on the same route must agree bit
for bit in everything they save and return (test_runs_of_one_geometry_agree says why, and why runs on different routes are
held to their two bounds plus the distance of their two float64 values, not to the bare sum of the bounds).  On the native
path one run per geometry also asks for the second output dx0 s2_next.
No hand-off timeout is shortened, no CU is held, no failure path is provoked; the largest launch is 128 workgroups of the
second design.

Measured on an MI355X, worst ratio to the bound over every route and host path (each case prints its own): bf16 xn1w 0.50,
mean1 0.004, rstd1 0.03, qkv 0.99, ao 0.47, lse 0.02, x1 0.99, proj.weight 0.39, proj.bias 0.20, dbias_table 0.03,
qkv.weight 0.015, qkv.bias 0.010, dx0 0.003, norm1.weight / norm1.bias below 0.001, dx0 s2_next 0.22; f32 at most 0.07
everywhere.  qkv and x1 stand at 0.99 because gemm_ref's bound carries no safety factor and its leading term is the bf16
rounding of the output itself, which a correct kernel does reach; the chained tensors stand far below 1/2 because their bounds
are worst cases over long sums (tests/test_swin_attn_half_cpu.py).  The 64 runs and 14 cross-checks take 3 s together."""
import math

import pytest
import torch

import attn_ref as A
import misc_ref as Mi
import swin_attn_half_ref as H
from swin_attn_half_ref import BF, F32

pytestmark = pytest.mark.gpu

DROP_P = 0.25
ROUTES = [(2, 2), (1, 1), (0, 0)]
# name -> (res, C, B, dtype, shifts, s1 mixed?, [((asked forward, asked backward), (forward, backward) the block must take)])
GEOMS = {
    # 64 windows: wmsa2, wb2<384>, the deferred dbias reduce, KS12, the stage-2 products
    "r14-C384-B16": (14, 384, 16, BF, (0, 3), True, [(r, r) for r in ROUTES]),
    "r14-C96-B16": (14, 96, 16, BF, (0, 3), True, [(r, r) for r in ROUTES]),                  # the 96-wide instantiations, KS3
    "r14-C192-B16": (14, 192, 16, BF, (3,), True, [(r, r) for r in ROUTES]),                  # 192-wide, KS6
    "r14-C384-B16-s1none": (14, 384, 16, BF, (3,), False, [((2, 2), (2, 2)), ((0, 0), (0, 0))]),   # no rowscale pointer (eval, p = 0)
    "r7-C384-B3": (7, 384, 3, BF, (0,), True, [((2, 2), (1, 1))]),       # odd window count: the second design refused both ways
    "r7-C768-B4": (7, 768, 4, BF, (0,), True, [((2, 2), (0, 0)), ((1, 1), (0, 0))]),          # stage 3: no fused forward, no KS route
    "r14-C128-B2": (14, 128, 2, BF, (3,), True, [((1, 0), (1, 0)), ((0, 0), (0, 0))]),        # Swin-B widths of the first design
    "r14-C512-B2": (14, 512, 2, BF, (3,), True, [((1, 0), (1, 0)), ((0, 0), (0, 0))]),        # ... and its largest LDS tile
    "r14-C384-B2-f32": (14, 384, 2, F32, (0, 3), True, [((1, 0), (1, 0)), ((0, 0), (0, 0))]),  # first design in f32, generic backward
    "r14-C96-B2-f32": (14, 96, 2, F32, (0, 3), True, [((1, 0), (1, 0)), ((0, 0), (0, 0))]),
}
CASES = [(g, shift, ask, native) for g, v in GEOMS.items() for shift in v[4] for ask, _ in v[6] for native in (True, False)]
GROUPS = [(g, shift) for g, v in GEOMS.items() for shift in v[4]]


def case_id(c):
    return "%s-s%d-fwd%d-bwd%d-%s" % (c[0], c[1], c[2][0], c[2][1], "native" if c[3] else "python")


def keep_pattern(B, flip):
    """First and last sample dropped (B >= 3); B = 2 drops one of the two, the other one when `flip`."""
    if B == 2:
        return [1.0, 0.0] if flip else [0.0, 1.0]
    return [0.0 if b in (0, B - 1) or b % 5 == 3 else 1.0 for b in range(B)]


_towers, _runs = {}, {}


def tower(res, C, dt):
    """One stage of two blocks at resolution `res` (block 0 at shift 0, block 1 at shift 3 when res > 7).  One-dimensional
    parameters away from 0 / 1, the bias tables with std 0.5, qkv weights so that scale q.k has std ~2.5 (attn_ref.LOGIT_STD:
    peaked softmax rows, so that one wrong key or row stands out)."""
    if (res, C, dt) not in _towers:
        import mvlt_amd as M
        from mvlt_amd.arena import Arena
        from mvlt_amd.swin import SwinTransformer
        torch.manual_seed(21)
        m = SwinTransformer(img_size=4 * res, embed_dim=C, depths=[2], num_heads=[C // 32], num_classes=0, drop_path_rate=0.3)
        g = torch.Generator().manual_seed(22)
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
        m = M.set_compute_dtype(m.cuda().train(), dt)
        ar = Arena.of(m, dt)
        ar.refresh_shadow(tail=False)
        _towers[res, C, dt] = (m, ar)
    return _towers[res, C, dt]


def poison(shapes, dt, device):
    ts = [torch.full(s, float("nan"), dtype=dt, device=device) for s in shapes]
    torch.cuda.synchronize()
    del ts


def set_route(mp, ask, native):
    from mvlt_amd import ops, swin
    mp.setattr(ops, "NATIVE", native)
    mp.setattr(swin, "_FUSED_WMSA", "0" if ask[0] == 0 else "1")
    mp.setattr(swin, "_WMSA2", ask[0] == 2)
    mp.setattr(swin, "_SWIN_BWD_ONE", 96 if ask[1] == 2 else 1 << 30)
    mp.setattr(swin, "_SWIN_BWD_PROJ", ask[1] >= 1)


def run_case(c):
    """-> (case dict, run dict of device tensors) of one case; the routes are asserted before anything is launched."""
    from mvlt_amd import _lib as L, ops, swin
    geom, shift, ask, native = c
    res, C, B, dt, _, mixed, pairs = GEOMS[geom]
    want = dict(pairs)[ask]
    nH, Lt, nW = C // 32, res * res, (res // 7) ** 2
    rows = B * Lt
    dev = torch.device("cuda")
    m, ar = tower(res, C, dt)
    blk = m.layers[0].blocks[1 if shift else 0]
    at = blk.attn
    assert blk.shift_size == shift and blk.window_size == 7 and blk.num_heads == nH
    with pytest.MonkeyPatch.context() as mp:
        set_route(mp, ask, native)
        # ---- the routes this case is about
        assert swin._wmsa_mode(dt, B, res, C, nH) == want[0], (case_id(c), "forward mode", swin._wmsa_mode(dt, B, res, C, nH))
        assert swin._bwd_mode(dt, B, res, C, nH, shift) == want[1], (case_id(c), "backward mode", swin._bwd_mode(dt, B, res, C, nH, shift))
        if want[1] in (0, 1):
            probe = torch.empty((rows, 3 * C), dtype=dt, device=dev)
            route = ops.attn_route(probe, L.ATTN_SWIN, B * nW, 49, nH, 32, at.scale, bwd=True,
                                   dout_weight=ar.compute(at.proj.weight) if want[1] == 1 else None,
                                   bias_table=at.relative_position_bias_table.data, nW=nW, win_res=res, shift=shift)
            assert route == ("SWIN_BWD_KS%d" % nH if want[1] == 1 else "SWIN_BWD_KS0" if dt == BF else "SWIN_BWD"), (case_id(c), route)
        # ---- inputs: the same for every route and host path of a (geometry, shift)
        g = torch.Generator().manual_seed(1000 + 7 * res + C + B + shift)
        x = torch.randn(rows, C, generator=g).to(dt).to(dev)
        dx2 = torch.randn(rows, C, generator=g).to(dt).to(dev)
        s1 = (torch.tensor(keep_pattern(B, flip=(shift == 3) != (C == 512))) / (1.0 - DROP_P)).to(dev) if mixed else None
        s2 = torch.zeros(B, device=dev)
        # the second output, dx0 s2_next: native path, the first route of the geometry
        s2_next = None
        if native and ask == pairs[0][0]:
            s2_next = (torch.tensor([0.0 if b % 3 == 1 else 1.0 for b in range(B)]) / (1.0 - DROP_P)).to(dev)
        poison([(rows, 3 * C), (rows, C), (rows, C), (rows, 4 * C), (rows, 4 * C)], dt, dev)
        x2, sv = m._block_fwd(ar, blk, x, B, res, res, s1, s2, True)
        ar.begin_backward()
        ar.grad_view(at.relative_position_bias_table).zero_()
        lnq = None
        if not native:
            lnq = m.__dict__["_lnq"] = ops.LnReduceQueue()
        nparts = max(1, ops.swin_wmsa2_bwd_parts(dt, B, res, C, nH)) if want[1] == 2 else 1
        poison([(rows, 3 * C), (rows, C), (nparts * rows, C), (rows, 4 * C), (rows, C)], dt, dev)
        dx0, dy2n = m._block_bwd(ar, sv, dx2, B, None, s2_next)
        if native:
            ops.host().lnq_flush(ops.stream_int())
        else:
            lnq.flush()
        ops.join_side(dev)
        torch.cuda.synchronize()
        if native:
            ops.host().side_release()
        assert ops.wmsa2_sync_errors() == 0, "a hand-off wait of mvlt_swin_wmsa2_fwd ran out"
        plan_next = m._dp_plan_of(s2_next, B, Lt, C, dt) if s2_next is not None else None
    # ---- saved tensors: the two host paths keep them in different tuples (csrc/host.cpp swin_block_fwd, swin.py _block_fwd)
    if native:
        assert len(sv) == 6
        sx, stat1, xn1w, qkv, ao, lse, x1 = sv[1][:7]
        mean1, rstd1 = stat1[0], stat1[1]
    else:
        assert len(sv) == 18
        sx, mean1, rstd1, xn1w, qkv, ao, lse, x1 = sv[1:9]
    assert sx.data_ptr() == x.data_ptr()
    out = dict(x=x, dx2=dx2, x2=x2, dx0=dx0, xn1w=xn1w, mean1=mean1, rstd1=rstd1, qkv=qkv, ao=ao, lse=lse, x1=x1,
               gamma1=blk.norm1.weight.data, beta1=blk.norm1.bias.data, wqkv=ar.compute(at.qkv.weight), bqkv=at.qkv.bias.data,
               wproj=ar.compute(at.proj.weight), bproj=at.proj.bias.data, table=at.relative_position_bias_table.data)
    if s1 is not None:
        out["s1"] = s1
    if s2_next is not None:
        assert dy2n is not None, "the native backward hands dx0 * s2_next back"
        out.update(dy2n=dy2n, s2_next=s2_next)
        if plan_next is not None:
            out["inv_next"] = plan_next[1]
    mlp = blk.mlp
    for name, p in (("norm1.weight", blk.norm1.weight), ("norm1.bias", blk.norm1.bias), ("qkv.weight", at.qkv.weight),
                    ("qkv.bias", at.qkv.bias), ("proj.weight", at.proj.weight), ("proj.bias", at.proj.bias),
                    ("dbias_table", at.relative_position_bias_table), ("fc1.weight", mlp.fc1.weight), ("fc1.bias", mlp.fc1.bias),
                    ("fc2.weight", mlp.fc2.weight), ("fc2.bias", mlp.fc2.bias), ("norm2.weight", blk.norm2.weight),
                    ("norm2.bias", blk.norm2.bias)):
        out[name] = ar.grad_view(p).view(p.shape)
    out = {k: v.detach().clone() for k, v in out.items()}
    for k, v in out.items():
        if v.is_floating_point():
            assert bool(torch.isfinite(v).all()), (case_id(c), k, "not finite")
    return dict(res=res, C=C, nH=nH, B=B, dtype=dt, shift=shift, fwd=want[0], bwd=want[1]), out


def judged(c):
    """(case, run, reference) of a case, run and judged once per session: the cross-checks read what the route tests left."""
    if c not in _runs:
        case, run = run_case(c)
        ref = H.reference(run, case)
        for k, v in H.worst_ratios(ref).items():
            print(f"{case_id(c):48s} {k:13s} worst ratio to the bound {v:.3f}")
        _runs[c] = (case, run, {k: ref[k] for k in H.COMPARED + H.SAVED + (("dy2n",) if "dy2n" in ref else ())})
    return _runs[c]


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_attention_half_route(c):
    case, run, ref = judged(c)
    bad = H.failures(ref, case_id(c))
    assert not bad, "\n".join(bad.values())
    H.check_dropped_rows(run, case, case_id(c))
    if "s1" in run:
        assert H.dropped_samples(run), "the mixed scales drop a sample"
    if c[3] and c[2] == GEOMS[c[0]][6][0][0]:
        assert "dy2n" in ref, "the native path's second output is judged on the first route of every geometry"
        assert ("inv_next" in run) == (case["C"] >= 384 and case["dtype"] == BF), "the consumer's row order"


@pytest.mark.parametrize("group", GROUPS, ids=lambda g: "%s-s%d" % g)
def test_runs_of_one_geometry_agree(group):
    """Every run of one (geometry, shift) shares its inputs.
    The two host paths on one route launch the same kernels on the same operands: whatever they save or return is bit-equal --
    saved tensors, x1, dx0 and every gradient that no f32 atomic forms (the bias table of backward
    modes 0 / 1 is accumulated with atomics in arbitrary order; mode 2 reduces per-workgroup rows in a fixed order).  This is
    the check that sees a wiring fault of ONE host path at any depth, bf16 included, where the float64 chain is too wide.
    Two runs on different routes each sit inside their bound around the float64 value of their OWN saved operands (the
    forward is judged stage by stage), so they differ by at most the two bounds plus the distance of those two values."""
    geom, shift = group
    cs = [c for c in CASES if c[0] == geom and c[1] == shift]
    rs = [judged(c) for c in cs]
    for k in ("x", "dx2", "wqkv", "wproj", "table", "gamma1"):
        for _, run, _ in rs[1:]:
            assert torch.equal(run[k], rs[0][1][k]), ("the runs of a group share their inputs", k)
    pairs = 0
    for i in range(len(cs)):
        for j in range(i + 1, len(cs)):
            what = f"{case_id(cs[i])} against {case_id(cs[j])}"
            for k in H.COMPARED:
                (vi, bi, gi), (vj, bj, gj) = rs[i][2][k], rs[j][2][k]
                over = (gi.double() - gj.double()).abs() > bi + bj + (vi - vj).abs()
                assert not bool(over.any()), (what, k, int(over.sum()), "elements further apart than the two bounds allow")
            (ci, ri), (cj, rj) = rs[i][:2], rs[j][:2]
            if (ci["fwd"], ci["bwd"]) == (cj["fwd"], cj["bwd"]) and cs[i][3] != cs[j][3]:
                pairs += 1
                for k in H.SAVED + ("x1", "dx0") + tuple(g for g in H.ATTN_GRADS if g != "dbias_table" or ci["bwd"] == 2):
                    Mi.check_equal(ri[k], rj[k], f"{what}: {k}")
    assert pairs >= 1, "every group runs at least one route on both host paths"
