"""The Mlp branch of a Swin stage-2 / 3 block on the rows of the samples DropPath keeps (csrc/host.cpp swin_block_fwd / _bwd,
MVLT_SWIN_DROP_COMPACT, default on), the row plan behind it (mvlt_droppath_plan) and the epilogue bit it rests on
(MVLT_EPI_TAIL).

The block functions are called directly with hand-made scales.  s1 = 0 drops the attention branch of every sample, so the
block IS x2 = x + s2 * Mlp(LN(x)) and its backward: x1 == x bit for bit, and dx0 = dx1 because the attention half receives
zeros.  Every case is judged twice:
  * against float64, stage by stage, from the operands each kernel itself read (tests/gemm_ref.py, tests/ln_ref.py, their
    constants unchanged).  Forward: norm2 from x1; fc1 from the stored xn2; fc2 from the stored act.  Backward: the
    intermediates (dy2, dh, dxn2) are not returned, so their float64 values are chained and the bound of each stage carries
    the bound of its input through the stage's own linear map (|W| for a dgrad, |operand| for a weight gradient, the
    LayerNorm Jacobian rstd (|gamma| e + mean(|gamma| e) + |xh| mean(|gamma| e |xh|)) for norm2) -- first order, no constant
    of its own.  The forward's saved h / act / xn2 / mean / rstd are taken as handed over, as tests/ln_ref.py does.
  * against the dense route of the same build (MVLT_SWIN_DROP_COMPACT=0 is read once per process: one fresh child runs
    every case and hands its tensors back).  Both routes meet the float64 bound on the same inputs, so they differ by at
    most twice the bound; the dense results are also checked against the bound itself.
Unwritten rows must not leak: NaN-filled blocks of the sizes of h / act / dh / dy2 / dxn2 are handed back to the caching
allocator before each call; every output must be finite and the x2 rows of dropped samples bit-equal to x1."""
import math
import os
import subprocess
import sys
import tempfile

import pytest
import torch

import gemm_ref as G
import ln_ref as R
from gemm_ref import check_bound

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (stage of the test tower, res, C, heads, B): stage 3 has 49 rows per sample -- the count is never a multiple of 16 or 64
GEOMS = {"stage2": (0, 14, 384, 12, 3), "stage3": (1, 7, 768, 24, 4)}
PATTERNS = {"none": lambda B: [1] * B, "all": lambda B: [0] * B, "first": lambda B: [0] + [1] * (B - 1),
            "last": lambda B: [1] * (B - 1) + [0], "alternating": lambda B: [b % 2 for b in range(B)]}
CASES = [(g, p, None) for g in GEOMS for p in PATTERNS] + [(g, p, 1) for g in GEOMS for p in ("none", "all")]
DROP_P = 0.25
GRADS = ("fc2.weight", "fc2.bias", "fc1.weight", "fc1.bias", "norm2.weight", "norm2.bias")


def case_id(c):
    return "%s-%s%s" % (c[0], c[1], "" if c[2] is None else "-B1")


def tower():
    """A two-stage tower whose stages have the geometry of Swin stages 2 and 3 (res 14 / C 384 and res 7 / C 768)."""
    import mvlt_amd as M
    from mvlt_amd.arena import Arena
    from mvlt_amd.swin import SwinTransformer
    torch.manual_seed(11)
    m = SwinTransformer(img_size=56, embed_dim=384, depths=[1, 1], num_heads=[12, 24], num_classes=0, drop_path_rate=0.3)
    g = torch.Generator().manual_seed(12)
    for n, p in m.named_parameters():           # biases and LayerNorm parameters that are not 0 / 1
        if p.dim() == 1:
            p.data.copy_((1.0 if n.endswith("norm1.weight") or n.endswith("norm2.weight") or n.endswith("norm.weight") else 0.0)
                         + 0.1 * torch.randn(p.shape, generator=g))
    m = M.set_compute_dtype(m.cuda().train(), BF)
    ar = Arena.of(m, BF)
    ar.refresh_shadow(tail=False)
    return m, ar


def poison(shapes, device):
    ts = [torch.full(s, float("nan"), dtype=BF, device=device) for s in shapes]
    torch.cuda.synchronize()
    del ts


def run_case(m, ar, case):
    """-> dict of CPU tensors: inputs, saved forward tensors, x2, dx and the parameter gradients of one case."""
    from mvlt_amd import ops
    geom, pattern, b1 = case
    li, res, C, nH, B = GEOMS[geom]
    B = B if b1 is None else b1
    Lt, rows = res * res, B * res * res
    blk = m.layers[li].blocks[0]
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(100 + 7 * li + len(pattern) + B)
    x = torch.randn(rows, C, generator=g).to(BF).to(dev)
    dx2 = torch.randn(rows, C, generator=g).to(BF).to(dev)
    keep = torch.tensor(PATTERNS[pattern](B), dtype=torch.float32)
    s1 = torch.zeros(B, device=dev)
    s2 = (keep / (1.0 - DROP_P)).to(dev)
    poison([(rows, 4 * C)] * 2, dev)
    x2, sv = m._block_fwd(ar, blk, x, B, res, res, s1, s2, True)
    saved = sv[1]
    ar.begin_backward()
    ar.grad_view(blk.attn.relative_position_bias_table).zero_()
    poison([(rows, 4 * C), (rows, C), (rows, C)], dev)
    dx, _ = m._block_bwd(ar, sv, dx2, B)
    ops.host().lnq_flush(ops.stream_int())
    ops.join_side(dev)
    torch.cuda.synchronize()
    ops.host().side_release()
    out = dict(x=x, dx2=dx2, s2=s2, x2=x2, dx=dx, x1=saved[6], stat2=saved[7], xn2=saved[8], h=saved[9], act=saved[10])
    if len(saved) >= 14:
        out.update(perm=saved[11], inv=saved[12], count=saved[13])
    mlp = blk.mlp
    for name, p in (("fc2.weight", mlp.fc2.weight), ("fc2.bias", mlp.fc2.bias), ("fc1.weight", mlp.fc1.weight),
                    ("fc1.bias", mlp.fc1.bias), ("norm2.weight", blk.norm2.weight), ("norm2.bias", blk.norm2.bias)):
        out[name] = ar.grad_view(p)
    out["w1"], out["w2"] = ar.compute(mlp.fc1.weight), ar.compute(mlp.fc2.weight)
    out["b1"], out["b2"], out["gamma"], out["beta"] = mlp.fc1.bias.data, mlp.fc2.bias.data, blk.norm2.weight.data, blk.norm2.bias.data
    return {k: v.detach().cpu().clone() for k, v in out.items()}


def run_all():
    m, ar = tower()
    return {case_id(c): run_case(m, ar, c) for c in CASES}


@pytest.fixture(scope="module")
def compact():
    from mvlt_amd import swin
    assert swin._DROP_COMPACT, "the compact route is the default"
    return run_all()


@pytest.fixture(scope="module")
def dense():
    """Every case again with MVLT_SWIN_DROP_COMPACT=0, in a fresh child (the switch is read once per process)."""
    env = dict(os.environ)
    env["MVLT_SWIN_DROP_COMPACT"] = "0"
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "dense.pt")
        r = subprocess.run([sys.executable, os.path.abspath(__file__), path], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "DENSE-OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
        return torch.load(path)


def host_plan(keep, Lt):
    """perm / inv / count as the issue states them: kept samples first in sample order, dropped ones behind, a full permutation."""
    B = len(keep)
    order = [b for b in range(B) if keep[b]] + [b for b in range(B) if not keep[b]]
    perm = torch.tensor([b * Lt + t for b in order for t in range(Lt)], dtype=torch.int32)
    inv = torch.empty_like(perm)
    inv[perm.long()] = torch.arange(B * Lt, dtype=torch.int32)
    return perm, inv, sum(1 for k in keep if k) * Lt


def reference(r, case):
    """float64 values and bounds of every compared tensor of one case, from the tensors `r` of a run (module docstring).
    Works for both routes: the order of the stored xn2 / h / act rows is `perm` (the identity for the dense route)."""
    geom, pattern, b1 = case
    _, res, C, _, B = GEOMS[geom]
    B = B if b1 is None else b1
    Lt, rows = res * res, B * res * res
    ident = torch.arange(rows, dtype=torch.int32)
    perm = r.get("perm", ident).long()
    inv = r.get("inv", ident).long()
    count = int(r["count"]) if "count" in r else rows
    s2, x1 = r["s2"].double(), r["x1"]
    srow = s2[torch.arange(rows) // Lt]                       # logical row -> scale
    ref = {}
    # ---- forward, stage by stage
    f = R.fwd_ref(x1, r["gamma"], r["beta"], BF)
    ref["xn2"] = (f["y"], f["y_b"], r["xn2"][inv])           # logical order
    ref["mean"] = (f["mean"], f["mean_b"], r["stat2"][0])
    ref["rstd"] = (f["rstd"], f["rstd_b"], r["stat2"][1])
    a, b = G.logical(r["xn2"], r["w1"])
    v, pre, bound, _, pre_b = G.gemm_ref(a, b, out_dtype=BF, m_eff=count, bias=r["b1"], gelu=True)
    ref["act"] = (v, bound, r["act"][:count])
    ref["h"] = (pre, pre_b, r["h"][:count])
    a, b = G.logical(r["act"][:count], r["w2"])
    v, _, bound, _, _ = G.gemm_ref(a, b, out_dtype=BF, bias=r["b2"], rowscale=(r["s2"], Lt), rowmap=perm[:count].int(), residual=x1)
    live = perm[:count]
    x2_ref, x2_b = x1.double().clone(), G.U_BF16 * x1.double().abs() + 1e-30
    x2_ref[live], x2_b[live] = v, bound
    ref["x2"] = (x2_ref, x2_b, r["x2"])
    # ---- backward: dy2 -> dh -> dxn2 chained in float64, bounds carried through each stage's linear map
    dx2 = r["dx2"].double()
    dy2 = (dx2 * srow[:, None])[perm][:count]                # the stored order, rows that exist
    e_dy2 = (G.U32 + G.U_BF16) * dy2.abs()
    hsv, actv, xn2v = r["h"][:count], r["act"][:count].double(), r["xn2"][:count].double()
    w1, w2 = r["w1"].double(), r["w2"].double()             # [4C, C], [C, 4C]
    dh, _, dh_b, _, _ = G.gemm_ref(dy2, w2, out_dtype=BF, mul_gelu_grad=hsv)
    dh_b = dh_b + (e_dy2 @ w2.abs()) * (G.gelu_grad64(hsv.double()).abs() + G.ERFC_ABS)
    dxn2c, _, dxn2c_b, _, _ = G.gemm_ref(dh, w1, out_dtype=BF)
    dxn2c_b = dxn2c_b + dh_b @ w1.abs()
    dxn2 = torch.zeros(rows, C, dtype=torch.float64)
    e_in = torch.zeros(rows, C, dtype=torch.float64)
    dxn2[live], e_in[live] = dxn2c, dxn2c_b                  # logical order; rows of dropped samples are exact zeros
    mean, rstd = r["stat2"][0], r["stat2"][1]
    bw = R.bwd_ref(x1, dxn2, mean, rstd, r["gamma"], BF, dres=r["dx2"])
    gam = r["gamma"].double().abs()[None, :]
    rs = rstd.double()[:, None]
    xh = ((x1.double() - mean.double()[:, None]) * rs).abs()
    ge = gam * e_in
    ref["dx"] = (bw["dx"], bw["dx_b"] + rs * (ge + ge.mean(1, keepdim=True) + xh * (ge * xh).mean(1, keepdim=True)), r["dx"])
    ref["norm2.weight"] = (bw["dg"], bw["dg_b"] + (e_in * xh).sum(0), r["norm2.weight"])
    ref["norm2.bias"] = (bw["db"], bw["db_b"] + e_in.sum(0), r["norm2.bias"])
    v, _, bound, _, _ = G.gemm_ref(dy2.t(), actv, out_dtype=torch.float32)
    ref["fc2.weight"] = (v, bound + e_dy2.t() @ actv.abs(), r["fc2.weight"])
    v, bound = G.colsum_ref(dy2.t())
    ref["fc2.bias"] = (v, bound + e_dy2.sum(0), r["fc2.bias"])
    v, _, bound, _, _ = G.gemm_ref(dh.t(), xn2v, out_dtype=torch.float32)
    ref["fc1.weight"] = (v, bound + dh_b.t() @ xn2v.abs(), r["fc1.weight"])
    v, bound = G.colsum_ref(dh.t())
    ref["fc1.bias"] = (v, bound + dh_b.sum(0), r["fc1.bias"])
    return ref


def check_run(r, case, label):
    for k in ("x2", "dx", "xn2") + GRADS:
        assert bool(torch.isfinite(r[k].float()).all()), (label, case_id(case), k, "not finite")
    assert torch.equal(r["x1"], r["x"]), (label, "s1 = 0 must leave x1 == x")
    ref = reference(r, case)
    worst = {}
    for k, (v, b, out) in ref.items():
        ratio = float(((out.double() - v).abs() / b).max()) if out.numel() else 0.0
        worst[k] = ratio
        print(f"{label:8s} {case_id(case):22s} {k:13s} worst ratio to the bound {ratio:.3f}")
    for k, (v, b, out) in ref.items():
        check_bound(out, v, b, f"{label} {case_id(case)} {k}")
    return ref


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_block_against_fp64_and_dense_route(compact, dense, case):
    c, d = compact[case_id(case)], dense[case_id(case)]
    geom, pattern, b1 = case
    _, res, C, _, B = GEOMS[geom]
    B = B if b1 is None else b1
    Lt = res * res
    keep = PATTERNS[pattern](B)
    assert "perm" in c and "perm" not in d, "the parent runs the compact route, the child the dense one"
    for k in ("x", "dx2", "s2", "w1", "w2"):
        assert torch.equal(c[k], d[k]), ("the two processes must run the same inputs", k)
    # plan kernel against the host statement of it
    perm, inv, count = host_plan(keep, Lt)
    assert torch.equal(c["perm"], perm) and torch.equal(c["inv"], inv) and int(c["count"]) == count
    # float64, both routes on the same inputs
    rc = check_run(c, case, "compact")
    rd = check_run(d, case, "dense")
    # the two routes: each inside its bound around the same float64 value
    for k in ("x2", "dx") + GRADS:
        assert (c[k].double() - d[k].double()).abs().le(rc[k][1] + rd[k][1]).all(), (case_id(case), k, "compact vs dense")
    # rows of dropped samples: x2 == x1 bit for bit, and no gradient but the residual's
    for b in range(B):
        if not keep[b]:
            sl = slice(b * Lt, (b + 1) * Lt)
            assert torch.equal(c["x2"][sl], c["x1"][sl]), (case_id(case), "x2 of dropped sample", b)
            assert torch.equal(c["dx"][sl], c["dx2"][sl]), (case_id(case), "dx of dropped sample", b)
    if count == 0:
        for k in ("fc2.weight", "fc2.bias", "fc1.weight", "fc1.bias", "norm2.weight", "norm2.bias"):
            assert not c[k].any(), (k, "every sample dropped: the gradient is zero")


@pytest.mark.parametrize("B,keep", [(1, [1]), (1, [0]), (5, [1, 0, 0, 1, 1]), (32, [b % 3 != 1 for b in range(32)])])
def test_plan_kernel_many_blocks(B, keep):
    """One launch for several blocks with different token counts, a block that takes no plan (lt = 0) and one whose rows
    do not fit ld: their outputs stay untouched."""
    from mvlt_amd import ops
    dev = torch.device("cuda")
    lts = [196, 0, 49, 400]
    ld = B * 196
    scales = torch.zeros(2 * len(lts), B)
    for i in range(len(lts)):
        scales[2 * i] = 1.0                                             # the attention branch's row: never read
        scales[2 * i + 1] = torch.tensor([1.25 * float(k) for k in (keep if i != 2 else keep[::-1])])
    from mvlt_amd import _lib as L
    lt = torch.tensor(lts, dtype=torch.int32, device=dev)
    sd = scales.to(dev)
    perm = torch.full((len(lts), ld), -7, dtype=torch.int32, device=dev)
    inv = torch.full((len(lts), ld), -7, dtype=torch.int32, device=dev)
    count = torch.full((len(lts),), -7, dtype=torch.int32, device=dev)
    L.check(L.lib().mvlt_droppath_plan(sd.data_ptr(), 1, 2, lt.data_ptr(), len(lts), B, ld, perm.data_ptr(), inv.data_ptr(),
                                       count.data_ptr(), ops.stream_int()), "mvlt_droppath_plan")
    torch.cuda.synchronize()
    perm, inv, count = perm.cpu(), inv.cpu(), count.cpu()
    for i, Lt in enumerate(lts):
        if Lt == 0 or B * Lt > ld:
            assert (perm[i] == -7).all() and (inv[i] == -7).all() and int(count[i]) == -7
            continue
        p, v, c = host_plan(keep if i != 2 else keep[::-1], Lt)
        n = B * Lt
        assert torch.equal(perm[i, :n], p) and torch.equal(inv[i, :n], v) and int(count[i]) == c
        assert (perm[i, n:] == -7).all() and (inv[i, n:] == -7).all()


@pytest.mark.parametrize("full", [False, True], ids=["plain", "rowmap+residual+rowscale"])
@pytest.mark.parametrize("bk", [False, True], ids=["B[n,k]", "B[k,n]"])
@pytest.mark.parametrize("m_dev", [0, 49, 64, 100, 192])
def test_epi_tail_kernel(m_dev, bk, full):
    """MVLT_EPI_TAIL on one product, M = 192, N = 128, K = 128: the rows of A at or beyond the count are NaN, every row of C is
    written; rows below the count are the plain product, rows beyond it the epilogue of a zero accumulator."""
    from mvlt_amd import _lib as L, ops
    M, N, K = 192, 128, 128
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(5 + m_dev)
    A = torch.randn(M, K, generator=g).to(BF)
    A[m_dev:] = float("nan")
    Bm = (0.1 * torch.randn((K, N) if bk else (N, K), generator=g)).to(BF)
    bias = torch.randn(N, generator=g)
    md = torch.tensor([m_dev], dtype=torch.int32, device=dev)
    kw, rkw = dict(bias=bias.to(dev)), dict(bias=bias)
    rowmap = torch.arange(M, dtype=torch.int32)
    if full:
        rowmap = torch.randperm(M, generator=g).int()
        res = torch.randn(M, N, generator=g).to(BF)
        rs = torch.tensor([1.5, 0.0, 2.0, 0.0])                       # 48 rows per scale
        kw.update(rowmap=rowmap.to(dev), residual=res.to(dev), rowscale=(rs.to(dev), 48))
        rkw.update(rowmap=rowmap, residual=res, rowscale=(rs, 48))
    out = torch.full((M, N), 7.0, dtype=BF, device=dev)
    ops.gemm(A.to(dev), Bm.to(dev), b_kmajor=bk, out=out, m_dev=md, tail=True, **kw)
    torch.cuda.synchronize()
    out = out.cpu()
    assert bool(torch.isfinite(out.float()).all())
    a, b = G.logical(A, Bm, b_kmajor=bk)
    v, _, bound, rows, _ = G.gemm_ref(a, b, out_dtype=BF, m_eff=m_dev, **rkw)
    check_bound(out[rows], v, bound, f"tail m_dev={m_dev} live rows")
    # rows beyond the count: a zero accumulator through the same epilogue
    dead = rowmap[m_dev:].long()
    z = bias.double()[None, :].expand(M - m_dev, N)
    if not full:
        assert torch.equal(out[dead], z.float().to(BF)), "rows beyond the count: the bias, rounded once"
    else:
        sc = rs.double()[dead // 48][:, None]
        zs = z * sc
        z = zs + res.double()[dead]
        check_bound(out[dead], z, G.U_BF16 * z.abs() + 2 * G.U32 * (zs.abs() + z.abs()) + 1e-30, f"tail m_dev={m_dev} rows beyond the count")
        gone = (sc == 0).expand_as(z)
        assert torch.equal(out[dead][gone], res[dead][gone]), "scale 0: the residual row, bit for bit"
    # k-slices refuse the bit
    with pytest.raises(Exception):
        ops.gemm(A.to(dev), Bm.to(dev), b_kmajor=bk, out=out.to(dev), m_dev=md, tail=True, split_k=2, **kw)


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from mvlt_amd import swin as _swin
    assert not _swin._DROP_COMPACT
    torch.save(run_all(), sys.argv[1])
    print("DENSE-OK")
