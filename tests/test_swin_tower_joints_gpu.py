"""The joints of SwinTransformer._forward / _backward, per element: what happens BETWEEN the block calls -- patch embedding,
PatchMerging, the final norm with its fused GELU, the DropPath index arithmetic (_dp_plan_all / _dp_plan_of, rows 2i / 2i + 1 of
the scales) and the hand-off of dx0 s2 from a block to the one before it -- which the suite judged by whole-tensor norms only.

Tower: SwinTransformer(img_size=56, embed_dim=192, depths=[2, 2], num_heads=[6, 12], drop_path_rate=0.3), B = 4, training
mode, runtime.manual_seed(SEED) chosen so that every block with p > 0 has a kept and a dropped sample in both of its scale
rows (asserted from last_droppath).  Stage 1 is C 384 at res 7: the Mlp half runs on the kept rows there (native, bf16) and
dense at stage 0.  Runs: bf16 native (compact), bf16 native with swin._DROP_COMPACT off, bf16 Python, f32 native; fuse_gelu
true and false.

_block_fwd / _block_bwd / _forward are wrapped by a recorder that taps their arguments and results and changes nothing.  Every
joint is judged one stage deep from tensors that were really handed over, with the bounds of tests/gemm_ref.py /
tests/ln_ref.py unchanged and no tolerance of its own:
  patch embedding   cols bit for bit against F.unfold; x0 = gemm_ref(cols, W, bias); the patch LayerNorm and its stats from x0
                    (its output IS the x recorded into block 0); backward from the dx0 block 0 returned: norm.weight / norm.bias
                    by ln_ref.bwd_ref, proj.weight / proj.bias through gemm_ref / colsum_ref with bwd_ref's dx bound carried
  patch merging     the merge LayerNorm of ln_ref.merge_index rows of the x2 the last block of stage 0 returned, its stats, the
                    reduction product (IS the x recorded into stage 1); backward from the dx0 the first block of stage 1
                    returned: reduction.weight by gemm_ref; dxm chained with its bound carried through the LayerNorm Jacobian
                    into the dx2 recorded into the last block of stage 0, and into the merge norm's weight / bias
  final norm        y, y_pre and the stats from the x2 of the last block; backward to the dx2 recorded into the last block,
                    norm.weight / norm.bias, with and without GELU
  the chain         every native block with s2 that is not the last of its stage received as dy2_pre the very object its
                    producer returned, equal to the producer's stored dx0 times this block's s2 in this block's inv order
                    within U_OUT s2 |dx0| + (2 U32 + U_OUT) |.| (formed from the f32 dx0: ln_ref's rule for a branch output);
                    the last block of a stage, and every block on the Python path, receives None; _dp_plan_of answers the host
                    statement of the plan for the block's row of last_droppath (None where the block runs dense); the recorded
                    s1 / s2 are rows 2i / 2i + 1 of last_droppath (None at p = 0)
  every block       the whole-block reference of tests/swin_block_ref.py from the recorded arguments (chained judgement), so the
                    tower's own calls are held per element too
  host paths        native (dense) and Python of the same seed: bit-equal in the whole forward and in the backward up to the first
                    hand-off (the final norm and the last block, float-atomic bias tables excepted); behind it the native
                    path's dy2 skips one rounding, so each run is held to the bounds around the float64 values of its own
                    recorded operands.  Native compact against native dense: bit-equal up to the first compact product.

Measured on an MI355X, worst ratio to the bound over the eight runs (test_worst_ratios_summary prints them).  bf16: patch x0
0.99, patch / merge / final LayerNorm outputs 0.50, their stats at most 0.017, merge reduction 0.96, final dx 0.50, merge dx 0.52
(dxm's bound carried), the hand-off dy2_pre of block 2 0.80, merge norm.weight / norm.bias 0.18 / 0.13, patch proj.weight /
proj.bias 0.05 / 0.03, merge reduction.weight 0.02, every other parameter gradient of a joint at most 0.006; the blocks as in
tests/test_swin_block_gpu.py's chained judgement (qkv / x1 / x2 / h / act 0.99, fc2.weight 0.45, dx0 0.017).  f32: at most 0.07
everywhere except the hand-off 0.23 and dx0 s2_next 0.10.  In this tower exactly one hand-off is live (block 2 takes block 3's):
block 0 has p = 0 and blocks 1 and 3 are the last of their stages.  The file takes 4.1 s alone (47 tests, eight tower runs; the
first pays 1.4 s of start-up)."""
import pytest
import torch
import torch.nn.functional as F

import gemm_ref as G
import ln_ref as R
import misc_ref as Mi
import swin_block_ref as S
from swin_block_ref import BF, F32
from test_swin_droppath_compact_gpu import host_plan

pytestmark = pytest.mark.gpu

SEED = 277
B, IMG, P = 4, 56, 4
# run -> (dtype, native, swin._DROP_COMPACT)
RUNS = {"bf16-native": (BF, True, True), "bf16-native-dense": (BF, True, False), "bf16-python": (BF, False, True),
        "f32-native": (F32, True, True)}
VARIANTS = [(r, fg) for r in RUNS for fg in (False, True)]
_towers, _done, _worst = {}, {}, {}


def tower(dt):
    if dt not in _towers:
        import math

        import attn_ref as A
        import mvlt_amd as M
        from mvlt_amd.swin import SwinTransformer
        torch.manual_seed(51)
        m = SwinTransformer(img_size=IMG, embed_dim=192, depths=[2, 2], num_heads=[6, 12], num_classes=0, drop_path_rate=0.3)
        g = torch.Generator().manual_seed(52)
        for n, p in m.named_parameters():
            if p.dim() == 1:
                p.data.copy_((1.0 if n.endswith(("norm1.weight", "norm2.weight", "norm.weight")) else 0.0)
                             + 0.1 * torch.randn(p.shape, generator=g))
        for layer in m.layers:
            for blk in layer.blocks:
                C, at = blk.dim, blk.attn
                w = torch.randn(3 * C, C, generator=g) * C ** -0.5
                w[:2 * C] *= math.sqrt(A.LOGIT_STD)
                at.qkv.weight.data.copy_(w)
                at.proj.weight.data.copy_(torch.randn(C, C, generator=g) * C ** -0.5)
                at.relative_position_bias_table.data.copy_(0.5 * torch.randn(169, blk.num_heads, generator=g))
                blk.mlp.fc1.weight.data.copy_(torch.randn(4 * C, C, generator=g) * C ** -0.5)
                blk.mlp.fc2.weight.data.copy_(torch.randn(C, 4 * C, generator=g) * (4 * C) ** -0.5)
            if layer.downsample is not None:
                w = layer.downsample.reduction.weight
                w.data.copy_(torch.randn(w.shape, generator=g) * w.shape[1] ** -0.5)
        w = m.patch_embed.proj.weight
        w.data.copy_(torch.randn(w.shape, generator=g) * (w.numel() // w.shape[0]) ** -0.5)
        _towers[dt] = M.set_compute_dtype(m.cuda().train(), dt)
    return _towers[dt]


def run_tower(name, fuse_gelu):
    """One forward and backward of the tower with the recorder on -> everything the joints are judged from."""
    from mvlt_amd import ops, runtime, swin
    if (name, fuse_gelu) in _done:
        return _done[name, fuse_gelu]
    dt, native, compact = RUNS[name]
    m = tower(dt)
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(60)
    img = torch.randn(B, 3, IMG, IMG, generator=g).to(dev)
    rec = dict(fwd=[], bwd=[], forward=[])
    f0, b0, F0 = m._block_fwd, m._block_bwd, m._forward

    def tap_fwd(ar, blk, x, Bn, H, W, s1, s2, save):
        out = f0(ar, blk, x, Bn, H, W, s1, s2, save)
        rec["fwd"].append(dict(blk=blk, x=x, s1=s1, s2=s2, H=H, x2=out[0], sv=out[1]))
        return out

    def tap_bwd(ar, sv, dx2, Bn, dy2_pre=None, s2_next=None):
        out = b0(ar, sv, dx2, Bn, dy2_pre, s2_next)
        rec["bwd"].append(dict(sv=sv, dx2=dx2, dy2_pre=dy2_pre, s2_next=s2_next, dx0=out[0], pre=out[1]))
        return out

    def tap_forward(image, fg, save):
        out = F0(image, fg, save)
        rec["forward"].append(out[1])
        return out

    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(ops, "NATIVE", native)
        mp.setattr(swin, "_DROP_COMPACT", compact)
        mp.setattr(m, "_block_fwd", tap_fwd)
        mp.setattr(m, "_block_bwd", tap_bwd)
        mp.setattr(m, "_forward", tap_forward)
        runtime.manual_seed(SEED)
        m.zero_grad(set_to_none=True)                  # torch semantics: gradients left in p.grad by an earlier run would be added to
        y = m(img, fuse_gelu=fuse_gelu)
        dp = m.last_droppath
        dout = torch.randn(y.shape, generator=g).to(dt).to(dev)
        y.backward(dout)
        torch.cuda.synchronize()
        if native:
            ops.host().side_release()
        assert ops.wmsa2_sync_errors() == 0
        saved = rec["forward"][0]
        ar = saved["arena"]
        grads = {n: ar.grad_view(p).view(p.shape).detach().clone() for n, p in m.named_parameters()}
        blocks = [b for _, b in m._blocks()]
        plans, modes = [], []
        for i, f in enumerate(rec["fwd"]):
            Lt = f["H"] ** 2
            pl = m._dp_plan_of(f["s2"], B, Lt, f["blk"].dim, dt)
            plans.append(None if pl is None else [t.clone() for t in pl])
            modes.append((swin._wmsa_mode(dt, B, f["H"], f["blk"].dim, f["blk"].num_heads),
                          swin._bwd_mode(dt, B, f["H"], f["blk"].dim, f["blk"].num_heads, f["blk"].shift_size)))
        torch.cuda.synchronize()
    assert len(rec["fwd"]) == len(rec["bwd"]) == len(blocks) == 4
    rec["bwd"].reverse()                                                 # block order
    for f, b, blk in zip(rec["fwd"], rec["bwd"], blocks):
        assert f["blk"] is blk and b["sv"] is f["sv"], "the backward walks the blocks in reverse, each with what its forward saved"
    out = dict(m=m, ar=ar, img=img, y=y.detach(), dout=dout, dp=dp.clone(), saved=saved, fwd=rec["fwd"], bwd=rec["bwd"], grads=grads,
               plans=plans, modes=modes, dt=dt, native=native, compact=compact and native and dt == BF, fuse_gelu=fuse_gelu, name=name)
    _done[name, fuse_gelu] = out
    return out


def judge(run, label, value, bound, got):
    g = got.double()
    ratio = float(torch.where(torch.isfinite(g), (g - value).abs() / bound, torch.full_like(value, float("inf"))).max())
    key = ("bf16" if run["dt"] == BF else "f32", label)
    _worst[key] = max(_worst.get(key, 0.0), ratio)
    print(f"{run['name']:18s} gelu {int(run['fuse_gelu'])} {label:28s} worst ratio to the bound {ratio:.3f}")
    G.check_bound(got, value, bound, f"{run['name']} {label}")


@pytest.mark.parametrize("name,fuse_gelu", VARIANTS, ids=lambda v: v if isinstance(v, str) else "gelu%d" % int(v))
def test_droppath_rows_and_plans(name, fuse_gelu):
    run = run_tower(name, fuse_gelu)
    dp, dt = run["dp"], run["dt"]
    assert dp.shape == (8, B)
    keep = (dp != 0).cpu()
    for i, f in enumerate(run["fwd"]):
        p = f["blk"].drop_path_prob
        if p == 0:
            assert f["s1"] is None and f["s2"] is None and i == 0
            assert run["plans"][i] is None
            continue
        for row, s in ((2 * i, f["s1"]), (2 * i + 1, f["s2"])):
            assert s is not None and s._base is run["m"].last_droppath and s.storage_offset() == row * B and s.numel() == B, \
                (i, row, "the scales of block i are rows 2i / 2i + 1")
            assert torch.equal(s, dp[row])
            assert bool(keep[row].any()) and not bool(keep[row].all()), (i, row, "a kept and a dropped sample: choose another SEED")
        Lt, C = f["H"] ** 2, f["blk"].dim
        plan = run["plans"][i]
        native_sv = len(f["sv"]) == 6
        assert native_sv == run["native"]
        if run["compact"] and C >= 384:
            perm, inv, count = host_plan(keep[2 * i + 1].tolist(), Lt)
            assert plan is not None and torch.equal(plan[0].cpu(), perm) and torch.equal(plan[1].cpu(), inv) and int(plan[2]) == count
            assert len(f["sv"][1]) == 14, "the block ran compact"
            for t, want in zip(f["sv"][1][11:14], (perm, inv, torch.tensor([count], dtype=torch.int32))):
                assert torch.equal(t.cpu(), want), "the block ran on the plan of its own row"
        else:
            assert plan is None
            assert not native_sv or len(f["sv"][1]) == 11, "the block ran dense"


@pytest.mark.parametrize("name,fuse_gelu", VARIANTS, ids=lambda v: v if isinstance(v, str) else "gelu%d" % int(v))
def test_hand_off_chain(name, fuse_gelu):
    run = run_tower(name, fuse_gelu)
    dt = run["dt"]
    uo = R.u_out(dt)
    last_of_stage = {1, 3}
    for i, (f, b) in enumerate(zip(run["fwd"], run["bwd"])):
        assert b["dx2"].shape == f["x"].shape
        if i + 1 < 4 and i not in last_of_stage:
            assert b["dx2"] is run["bwd"][i + 1]["dx0"], "a block's dx2 is the object the block after it returned"
        if not run["native"] or f["s2"] is None or i in last_of_stage:
            assert b["dy2_pre"] is None, (i, "no hand-off: Python path, no scales, or the last block of a stage")
            if not run["native"]:
                assert b["pre"] is None
            continue
        prod = run["bwd"][i + 1]
        assert prod["s2_next"] is f["s2"], (i, "the producer scales with the consumer's s2")
        assert b["dy2_pre"] is prod["pre"] and prod["pre"] is not None, (i, "the consumer takes the object its producer returned")
        Lt = f["H"] ** 2
        rows = B * Lt
        srow = S.scale_rows(f["s2"], rows, Lt, f["x"].device)
        dz = prod["dx0"].double() * srow
        bound = uo * srow * prod["dx0"].double().abs() + (2 * G.U32 + uo) * dz.abs() + 1e-30
        plan = run["plans"][i]
        got = prod["pre"] if plan is None else prod["pre"][plan[1].long()]
        judge(run, f"block {i} dy2_pre", dz, bound, got)
    # block 0 has p = 0: its producer is asked for no second output
    assert run["bwd"][1]["s2_next"] is None and run["bwd"][1]["pre"] is None


@pytest.mark.parametrize("name,fuse_gelu", VARIANTS, ids=lambda v: v if isinstance(v, str) else "gelu%d" % int(v))
def test_patch_embedding(name, fuse_gelu):
    run = run_tower(name, fuse_gelu)
    m, ar, dt, gr = run["m"], run["ar"], run["dt"], run["grads"]
    pe = m.patch_embed
    cols, x0, mean, rstd = run["saved"]["pe"]
    Gd = IMG // P
    stmt = F.unfold(run["img"], kernel_size=P, stride=P).transpose(1, 2).reshape(B * Gd * Gd, 3 * P * P).to(dt)
    Mi.check_equal(cols, stmt, f"{name} im2col")
    w = ar.compute(pe.proj.weight).view(pe.proj.weight.shape[0], -1)
    a, b = G.logical(cols, w)
    v, _, bound, _, _ = G.gemm_ref(a, b, out_dtype=dt, bias=pe.proj.bias.data)
    judge(run, "patch x0", v, bound, x0)
    f = R.fwd_ref(x0, pe.norm.weight.data, pe.norm.bias.data, dt, eps=Mi.f32(pe.norm.eps))
    x_in = run["fwd"][0]["x"]
    judge(run, "patch norm y", f["y"], f["y_b"], x_in.view(-1, x0.shape[1]))
    judge(run, "patch norm mean", f["mean"][:, None], f["mean_b"][:, None], mean[:, None])
    judge(run, "patch norm rstd", f["rstd"][:, None], f["rstd_b"][:, None], rstd[:, None])
    # backward from the dx0 block 0 really returned
    dx = run["bwd"][0]["dx0"]
    bw = R.bwd_ref(x0, dx, mean, rstd, pe.norm.weight.data, dt)
    judge(run, "patch norm.weight", bw["dg"][:, None], bw["dg_b"][:, None], gr["patch_embed.norm.weight"][:, None])
    judge(run, "patch norm.bias", bw["db"][:, None], bw["db_b"][:, None], gr["patch_embed.norm.bias"][:, None])
    d0, e0, cd = bw["dx"], bw["dx_b"], cols.double()
    v, _, bound, _, _ = G.gemm_ref(d0.t(), cd, out_dtype=F32)
    judge(run, "patch proj.weight", v, bound + e0.t() @ cd.abs(), gr["patch_embed.proj.weight"].view(v.shape))
    v, bound = G.colsum_ref(d0.t())
    judge(run, "patch proj.bias", v[:, None], (bound + e0.sum(0))[:, None], gr["patch_embed.proj.bias"][:, None])


@pytest.mark.parametrize("name,fuse_gelu", VARIANTS, ids=lambda v: v if isinstance(v, str) else "gelu%d" % int(v))
def test_patch_merging(name, fuse_gelu):
    run = run_tower(name, fuse_gelu)
    m, ar, dt, gr = run["m"], run["ar"], run["dt"], run["grads"]
    layer = m.layers[0]
    ds = layer.downsample
    H, W = layer.input_resolution
    C = layer.dim
    xin, xm, mean, rstd = run["saved"]["merges"][0]
    assert xin is run["fwd"][1]["x2"], "the merge reads what the last block of the stage returned"
    idx = R.merge_index(B, H, W, C, xin.device)
    logical = xin.reshape(-1)[idx.reshape(-1)].view(-1, 4 * C)
    f = R.fwd_ref(logical, ds.norm.weight.data, ds.norm.bias.data, dt, eps=Mi.f32(ds.norm.eps))
    judge(run, "merge norm y", f["y"], f["y_b"], xm)
    judge(run, "merge norm mean", f["mean"][:, None], f["mean_b"][:, None], mean[:, None])
    judge(run, "merge norm rstd", f["rstd"][:, None], f["rstd_b"][:, None], rstd[:, None])
    wr = ar.compute(ds.reduction.weight)
    a, b = G.logical(xm, wr)
    v, _, bound, _, _ = G.gemm_ref(a, b, out_dtype=dt)
    judge(run, "merge reduction", v, bound, run["fwd"][2]["x"])
    # backward from the dx0 the first block of stage 1 really returned
    dx = run["bwd"][2]["dx0"]
    v, _, bound, _, _ = G.gemm_ref(dx.double().t(), xm.double(), out_dtype=F32)
    judge(run, "merge reduction.weight", v, bound, gr["layers.0.downsample.reduction.weight"])
    dxm, _, dxm_b, _, _ = G.gemm_ref(dx.double(), wr.double(), out_dtype=dt)
    bw = R.bwd_ref(logical, dxm, mean, rstd, ds.norm.weight.data, dt)
    gam = ds.norm.weight.data.double().abs()[None, :]
    rs = rstd.double()[:, None]
    xh = ((logical.double() - mean.double()[:, None]) * rs).abs()
    got = run["bwd"][1]["dx2"].reshape(-1)[idx.reshape(-1)].view(-1, 4 * C)
    judge(run, "merge dx", bw["dx"], bw["dx_b"] + S.ln_carry(dxm_b, xh, rs, gam), got)
    judge(run, "merge norm.weight", bw["dg"][:, None], (bw["dg_b"] + (dxm_b * xh).sum(0))[:, None], gr["layers.0.downsample.norm.weight"][:, None])
    judge(run, "merge norm.bias", bw["db"][:, None], (bw["db_b"] + dxm_b.sum(0))[:, None], gr["layers.0.downsample.norm.bias"][:, None])


@pytest.mark.parametrize("name,fuse_gelu", VARIANTS, ids=lambda v: v if isinstance(v, str) else "gelu%d" % int(v))
def test_final_norm(name, fuse_gelu):
    run = run_tower(name, fuse_gelu)
    m, dt, gr = run["m"], run["dt"], run["grads"]
    x, mean, rstd, ypre = run["saved"]["final"]
    assert x is run["fwd"][3]["x2"], "the final norm reads what the last block returned"
    assert (ypre is not None) == fuse_gelu
    f = R.fwd_ref(x, m.norm.weight.data, m.norm.bias.data, dt, eps=Mi.f32(m.norm.eps), gelu=fuse_gelu)
    Cn = x.shape[1]
    judge(run, "final y", f["y"], f["y_b"], run["y"].reshape(-1, Cn))
    if fuse_gelu:
        judge(run, "final y_pre", f["pre"], f["pre_b"], ypre.reshape(-1, Cn))
    judge(run, "final mean", f["mean"][:, None], f["mean_b"][:, None], mean[:, None])
    judge(run, "final rstd", f["rstd"][:, None], f["rstd_b"][:, None], rstd[:, None])
    bw = R.bwd_ref(x, run["dout"].reshape(-1, Cn), mean, rstd, m.norm.weight.data, dt, y_pre=ypre.reshape(-1, Cn) if fuse_gelu else None)
    judge(run, "final dx", bw["dx"], bw["dx_b"], run["bwd"][3]["dx2"])
    judge(run, "final norm.weight", bw["dg"][:, None], bw["dg_b"][:, None], gr["norm.weight"][:, None])
    judge(run, "final norm.bias", bw["db"][:, None], bw["db_b"][:, None], gr["norm.bias"][:, None])


def block_run(run, i):
    """(case, run dict) of block i for swin_block_ref.reference, from what the recorder tapped."""
    from test_swin_block_gpu import params_of, saved_of
    f, b = run["fwd"][i], run["bwd"][i]
    blk = f["blk"]
    r = dict(saved_of(f["sv"], run["native"]), dx2=b["dx2"], x2=f["x2"], dx0=b["dx0"], **params_of(run["ar"], blk))
    for k in ("s1", "s2"):
        if f[k] is not None:
            r[k] = f[k]
    if b["dy2_pre"] is not None:
        r["dy2_pre"] = True
    if b["pre"] is not None:
        r.update(dy2n=b["pre"], s2_next=b["s2_next"])
        if run["plans"][i - 1] is not None:
            r["inv_next"] = run["plans"][i - 1][1]
    pre = f"layers.{i // 2}.blocks.{i % 2}."
    names = {"norm1.weight": "norm1.weight", "norm1.bias": "norm1.bias", "qkv.weight": "attn.qkv.weight", "qkv.bias": "attn.qkv.bias",
             "proj.weight": "attn.proj.weight", "proj.bias": "attn.proj.bias", "dbias_table": "attn.relative_position_bias_table",
             "fc1.weight": "mlp.fc1.weight", "fc1.bias": "mlp.fc1.bias", "fc2.weight": "mlp.fc2.weight", "fc2.bias": "mlp.fc2.bias",
             "norm2.weight": "norm2.weight", "norm2.bias": "norm2.bias"}
    for k, n in names.items():
        r[k] = run["grads"][pre + n]
    case = dict(res=f["H"], C=blk.dim, nH=blk.num_heads, B=B, dtype=run["dt"], shift=blk.shift_size, bwd=run["modes"][i][1])
    return case, r


@pytest.mark.parametrize("name,fuse_gelu", [v for v in VARIANTS if not v[1]], ids=lambda v: v if isinstance(v, str) else "gelu%d" % int(v))
def test_every_block_of_the_tower(name, fuse_gelu):
    run = run_tower(name, fuse_gelu)
    for i in range(4):
        case, r = block_run(run, i)
        ref = S.reference(r, case)
        for k, v in S.worst_ratios(ref).items():
            key = ("bf16" if run["dt"] == BF else "f32", "block " + k)
            _worst[key] = max(_worst.get(key, 0.0), v)
        print(f"{name} block {i} modes {run['modes'][i]}: " + "  ".join(f"{k} {v:.3f}" for k, v in S.worst_ratios(ref).items()))
        bad = S.failures(ref, f"{name} block {i}")
        assert not bad, "\n".join(bad.values())
        S.check_dropped_rows(r, case, f"{name} block {i}")


@pytest.mark.parametrize("fuse_gelu", [False, True], ids=["gelu0", "gelu1"])
def test_host_paths_agree(fuse_gelu):
    """bf16, the same seed.  Native (dense) against Python launch the same kernels on the same operands up to the first hand-off:
    the whole forward (everything every block saved, y), the final norm's backward and the whole backward of the last block are
    bit-equal, the bias table that float atomics form excepted (backward modes 0 / 1: held to the block reference by
    test_every_block_of_the_tower).  From the first hand-off on they are two arithmetics: the native consumer takes dx0 s2 formed
    from the producer's f32 dx0, the Python path scales the stored (rounded) dx0 in a launch of its own, one rounding more
    (test_hand_off_chain bounds the difference), so every gradient behind it differs in the last bits and each run is held to
    the bounds around the float64 values of its own recorded operands (the other tests of this file, run by run).
    Native compact against native dense: stage 1 runs its Mlp products in another row order and with a device row count, which
    may take another GEMM route, so only what precedes the first compact product is bit-equal -- the whole of stage 0, the
    merge and the attention half of the first block of stage 1; behind it the same holds."""
    from test_swin_block_gpu import saved_of
    nd, py, nc = (run_tower(n, fuse_gelu) for n in ("bf16-native-dense", "bf16-python", "bf16-native"))
    assert torch.equal(nd["dp"], py["dp"]) and torch.equal(nd["dp"], nc["dp"]), "the same seed draws the same scales"
    assert nd["modes"] == py["modes"] == nc["modes"]
    Mi.check_equal(nd["y"], py["y"], "native dense against Python: y")
    for i in range(4):
        a, b = saved_of(nd["fwd"][i]["sv"], True), saved_of(py["fwd"][i]["sv"], False)
        for k in S.SAVED:
            Mi.check_equal(a[k].contiguous(), b[k].contiguous(), f"native dense against Python: block {i} saved {k}")
        Mi.check_equal(nd["fwd"][i]["x2"], py["fwd"][i]["x2"], f"native dense against Python: block {i} x2")
    last = "layers.1.blocks.1."
    exact = ["norm.weight", "norm.bias"] + [k for k in nd["grads"] if k.startswith(last)]
    if nd["modes"][3][1] != 2:
        exact.remove(last + "attn.relative_position_bias_table")
    assert len(exact) >= 14
    for k in exact:
        Mi.check_equal(nd["grads"][k], py["grads"][k], f"native dense against Python: {k}")
    Mi.check_equal(nd["bwd"][3]["dx2"], py["bwd"][3]["dx2"], "native dense against Python: dx2 of the last block")
    Mi.check_equal(nd["bwd"][3]["dx0"], py["bwd"][3]["dx0"], "native dense against Python: dx0 of the last block")
    assert nd["bwd"][2]["dy2_pre"] is not None and py["bwd"][2]["dy2_pre"] is None, "the first hand-off: block 2, native only"
    Mi.check_equal(nc["fwd"][2]["x"], nd["fwd"][2]["x"], "native compact against dense: the input of stage 1")
    Mi.check_equal(nc["fwd"][2]["sv"][1][6], nd["fwd"][2]["sv"][1][6], "native compact against dense: x1 of the first block of stage 1")
    assert nc["compact"] and len(nc["fwd"][2]["sv"][1]) == 14 and len(nd["fwd"][2]["sv"][1]) == 11


def test_worst_ratios_summary():
    assert _worst, "runs after the joint tests"
    for dtn in ("bf16", "f32"):
        print(f"{dtn}: " + ", ".join(f"{k[1]} {v:.3f}" for k, v in sorted(_worst.items()) if k[0] == dtn))
