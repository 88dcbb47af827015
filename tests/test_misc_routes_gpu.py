"""The training-step kernels of csrc/misc.hip against the float64 references of tests/misc_ref.py with PER-ELEMENT bounds:
cross entropy (lse, loss_sum, count, dlogits), AdamW (param, exp_avg, exp_avg_sq, bf16 shadow), the VL embeddings (forward
bit for bit; dimage, dword, dpos, dtype_emb), column sums, the row movers, cast and the unary kernels.

The launches go through the C ABI wherever the Python wrapper would allocate an output, so every output buffer starts
from a sentinel (7.0 or NaN) and carries a guard tail: whatever the contract says is not written is compared bit for
bit.  Pad columns and the rows behind a device-side row count hold NaN on the way in.  Every pointer handed to the library
is 16-byte aligned (column-sliced views keep the base of the wider tensor).  Shapes come from the launch arithmetic: the
1024-column trips and the 4-column groups of the CE kernels, one capped sweep of the AdamW grid (512 x 256 x 4 elements),
8192 x 256 items of the grid-stride kernels, the 32 columns of a position workgroup and its 64 position lanes, the 128
row slices of the column sums.  The worst ratio to the bound per quantity is printed by the last test (-s).

Measured on an MI355X, worst |out - ref| / bound over all cases (a bound is SAFETY = 2 times the estimate, so 0.5 is the
estimate itself; bf16 outputs sit at 0.5 by construction, the output rounding being half an ulp exactly):
  lse 0.313   loss_sum 0.176   dl bf16 0.498 / f32 0.433      m 0.483   v 0.446   p 0.199
  dword 0.500 (a row hit once is one rounding)   dpos 0.072   dtype 0.043
  colsum bf16 0.578 / f32 0.855 (gemm_ref.colsum_ref's form carries no SAFETY; the worst case is M = 1 under accumulate,
  where the whole error is the one rounding of prev + x against a bound of U |result| + 8 U |x|)
  gelu bf16 0.488 / f32 0.422   gelu_bwd 0.498 / 0.423   tanh 0.474 / 0.246   tanh_bwd 0.498 / 0.248
The device keeps f32 denormals in exp_avg_sq (it does not flush them) and casts denormals exactly, both ways.
The file takes 7 s on its own (5 s inside the whole suite)."""
import ctypes
import math
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

import misc_ref as R
from misc_ref import BF, F32, check_bound, check_equal, check_untouched, check_zero

pytestmark = pytest.mark.gpu

NAN = float("nan")
FILL = 7.0
GUARD = 8                       # elements (or rows) of guard tail behind an output
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORST = {}                      # quantity -> worst |out - ref| / bound
NOTES = {}                      # what the device was seen to do where the contract leaves a choice
DTS = [F32, BF]


@pytest.fixture(scope="module")
def ops():
    from mvlt_amd import ops as o
    return o


@pytest.fixture(scope="module")
def L():
    from mvlt_amd import _lib
    _lib.lib()
    return _lib


def tname(dt):
    return "bf16" if dt == BF else "f32"


def checked(key, out, ref, bound, what):
    out = out.double()
    if out.dim() == 0:
        out, ref, bound = out.reshape(1), ref.reshape(1), bound.reshape(1)
    assert bool(torch.isfinite(ref).all()) and bool(torch.isfinite(bound).all()), f"{what}: non-finite reference or bound"
    if out.numel():
        r = float(torch.where(torch.isfinite(out), (out - ref).abs() / bound, torch.full_like(ref, math.inf)).max())
        WORST[key] = max(WORST.get(key, 0.0), r)
    check_bound(out, ref, bound, what)


def ptr(t):
    return None if t is None else t.data_ptr()


def i32(v):
    return torch.tensor([v], dtype=torch.int32, device="cuda")


def filled(shape, fill, dt=F32):
    return torch.full(shape, fill, dtype=dt, device="cuda")


def guarded(n, fill, dt=F32):
    """(buffer of n + GUARD elements holding fill, its first n elements): same base pointer."""
    buf = filled((n + GUARD,), fill, dt)
    return buf, buf[:n]


# ------------------------------------------------------------------ cross entropy
def ce_fwd(L, ops, x, V, labels, lse, acc, rows_dev):
    """loss_sum -> acc[0], count -> acc[4] (16 bytes apart)."""
    return L.lib().mvlt_ce_fwd_ragged(ops._DT[x.dtype], ptr(x), x.stride(0), x.shape[0], V, ptr(labels), ptr(lse), ptr(acc),
                                      ptr(acc[4:]), ptr(rows_dev), ops._stream())


def ce_bwd(L, ops, x, V, labels, lse, count, gscale, gscale_dev, out, rows_dev):
    return L.lib().mvlt_ce_bwd_ragged(ops._DT[x.dtype], ptr(x), x.stride(0), x.shape[0], V, ptr(labels), ptr(lse), ptr(count),
                                      gscale, ptr(gscale_dev), ptr(out), ptr(rows_dev), ops._stream())


def ce_case(L, ops, family, V, ld, dt, rowcfg, *, ignore="third", seed=0):
    rows, rows_dev = R.CE_ROWS[rowcfg]
    n_valid = rows if rows_dev is None else rows_dev
    labels_c = R.ce_labels(rows, V, 11 + seed, ignore)
    x = R.ce_logits(family, rows, V, ld, dt, 12 + seed, labels_c, n_valid).cuda()
    labels = labels_c.cuda()
    rd = None if rows_dev is None else i32(rows_dev)
    what = f"ce {family} V={V} ld={ld} {tname(dt)} {rowcfg}"
    # forward
    lse = filled((rows,), FILL)
    acc = torch.zeros(8, device="cuda")
    assert ce_fwd(L, ops, x, V, labels, lse, acc, rd) == 0
    ref = R.ce_fwd_ref(x, V, labels, n_valid)
    on = ref["on"]
    assert float(acc[4]) == ref["count"] == int((labels_c[:n_valid] >= 0).sum()), what
    assert not bool(torch.isnan(acc).any()) and bool((acc[[1, 2, 3, 5, 6, 7]] == 0).all()), what
    check_zero(lse[:n_valid][~on], what + " lse of ignored rows")
    check_untouched(lse, n_valid, FILL, what + " lse")
    if ref["count"]:
        checked("lse", lse[:n_valid][on], ref["lse"][on], ref["lse_b"][on], what + " lse")
        checked("loss_sum", acc[0], ref["loss"], ref["loss_b"], what + " loss_sum")
    else:
        assert float(acc[0]) == 0.0, what
    # backward: handed the float64 lse rounded to f32 and the exact count (the forward above judged the kernel's own)
    lse_in = filled((rows,), NAN)
    lse_in[:n_valid] = ref["lse"].float()
    cnt = torch.tensor([float(ref["count"])], device="cuda")
    gdev = torch.tensor([R.CE_GSCALE_DEV], device="cuda")
    out = filled((rows, ld), NAN, dt)
    assert ce_bwd(L, ops, x, V, labels, lse_in, cnt, R.CE_GSCALE, gdev, out, rd) == 0
    dl, dl_b = R.ce_bwd_ref(x, V, labels, lse_in, ref["count"], R.CE_GSCALE, R.CE_GSCALE_DEV, dt, n_valid)
    checked("dl " + tname(dt), out[:n_valid, :V], dl, dl_b, what + " dl")
    check_zero(out[:n_valid, V:], what + " dl pad columns")
    check_zero(out[:n_valid, :V][~on], what + " dl of ignored rows")
    check_untouched(out, n_valid, NAN, what + " dl")
    x2 = x.clone()                                                   # in place (out = None in ops.ce_bwd)
    assert ce_bwd(L, ops, x2, V, labels, lse_in, cnt, R.CE_GSCALE, gdev, x2, rd) == 0
    check_equal(x2[:n_valid], out[:n_valid], what + " in-place dl")
    check_untouched(x2, n_valid, NAN, what + " in-place dl")
    return ref


@pytest.mark.parametrize("dt", DTS, ids=tname)
@pytest.mark.parametrize("family", R.CE_FAMILIES)
@pytest.mark.parametrize("V,ld", R.CE_SHAPES)
def test_ce_third_ignored(L, ops, V, ld, family, dt):
    ce_case(L, ops, family, V, ld, dt, "third-ignored")


@pytest.mark.parametrize("dt", DTS, ids=tname)
@pytest.mark.parametrize("rowcfg", ["one-row", "ragged"])
@pytest.mark.parametrize("i", range(len(R.CE_SHAPES)))
def test_ce_one_row_and_ragged(L, ops, i, rowcfg, dt):
    V, ld = R.CE_SHAPES[i]
    ce_case(L, ops, R.CE_FAMILIES[(i + (rowcfg == "ragged")) % len(R.CE_FAMILIES)], V, ld, dt, rowcfg, seed=3)


@pytest.mark.parametrize("dt", DTS, ids=tname)
@pytest.mark.parametrize("V,ld", [(1025, 1028), (1027, 1027), (2, 4)])
def test_ce_every_label_ignored(L, ops, V, ld, dt):
    """loss_sum == 0, count == 0, dl all zeros, nothing NaN."""
    ref = ce_case(L, ops, "plain", V, ld, dt, "third-ignored", ignore="all")
    assert ref["count"] == 0


@pytest.mark.parametrize("dt", DTS, ids=tname)
def test_ce_bwd_count_zero_is_clamped(L, ops, dt):
    """sc = gscale / max(count, 1): a backward handed count = 0 with labelled rows scales by gscale alone."""
    V, ld, rows = 1025, 1028, 5
    labels = R.ce_labels(rows, V, 21, "none")
    x = R.ce_logits("plain", rows, V, ld, dt, 22, labels).cuda()
    labels = labels.cuda()
    lse = R.ce_fwd_ref(x, V, labels)["lse"].float()
    out = filled((rows, ld), NAN, dt)
    assert ce_bwd(L, ops, x, V, labels, lse, torch.zeros(4, device="cuda"), 0.5, None, out, None) == 0
    dl, dl_b = R.ce_bwd_ref(x, V, labels, lse, 0.0, 0.5, None, dt)
    checked("dl " + tname(dt), out[:, :V], dl, dl_b, "ce count=0 dl")
    check_zero(out[:, V:], "ce count=0 dl pad columns")


# ------------------------------------------------------------------ AdamW
def adamw_state(n, late, seed):
    p = torch.randn(n, generator=R.gen(seed))
    if late:
        m = 0.1 * torch.randn(n, generator=R.gen(seed + 1))
        v = torch.rand(n, generator=R.gen(seed + 2)) * 0.01 + 1e-8
    else:
        m, v = torch.zeros(n), torch.zeros(n)
    bufs = []
    for t in (p, m, v):
        buf, view = guarded(n, FILL)
        view.copy_(t)
        bufs.append((buf, view))
    return bufs


def adamw_steps(ops, n, hyper, family, steps, *, late=False, shadow=True, coef=None, seed=90):
    lr, wd = R.ADAMW_HYPER[hyper]
    (pb, p), (mb, m), (vb, v) = adamw_state(n, late, seed)
    shb, sh = guarded(n, FILL, BF) if shadow else (None, None)
    cf = None if coef is None else torch.tensor([coef], device="cuda")
    skip = torch.zeros(4, dtype=torch.int32, device="cuda")
    for step in steps:
        g_c, gscale = R.adamw_grad(family, n, seed + 10 + step)
        g = g_c.cuda()
        ref = R.adamw_ref(p, g, m, v, lr, wd, step, gscale, coef)          # from the operands as they stand now
        p_in = p.clone()
        if coef is None:
            ops.adamw(p, g, m, v, sh, lr, *R.ADAMW_BETAS, R.ADAMW_EPS, wd, step, gscale)
        else:
            ops.adamw_guarded(p, g, m, v, sh, lr, *R.ADAMW_BETAS, R.ADAMW_EPS, wd, step, gscale, cf, skip)
        what = f"adamw n={n} {hyper} {family} step={step}" + ("" if coef is None else f" coef={coef}")
        for k, o in zip("pmv", (p, m, v)):
            checked(k, o, ref[k], ref[k + "_b"], f"{what} {k}")
        if shadow:
            assert torch.equal(sh, p.to(BF)), what + " shadow"
        for name, buf in (("p", pb), ("m", mb), ("v", vb), ("shadow", shb)):
            if buf is not None:
                check_untouched(buf, n, FILL, f"{what} {name} guard")
        if family == "zeros-third" and not late and step == 1:
            # g = m = v = 0: the decayed parameter and nothing else
            z = slice(0, None, 3)
            c = 1.0 - R.f32(lr) * R.f32(wd)
            assert bool(((p[z].double() - p_in[z].double() * c).abs() <= ref["p_b"][z]).all()), what
            check_zero(m[z], what + " m at zero gradients")
            check_zero(v[z], what + " v at zero gradients")
        if family == "tiny" and not late and step == 1:
            sub = (ref["v"] > 0) & (ref["v"] < 2.0 ** -126)
            if bool(sub.any()):
                NOTES["exp_avg_sq denormals"] = "kept" if bool((v[sub] != 0).any()) else "flushed to zero"
    return p, m, v, sh


@pytest.mark.parametrize("n", R.ADAMW_N)
def test_adamw_sizes(ops, n):
    """Steps 1, 2, 3 from zero moments with the project's hyperparameters; the last three sizes take the sweep of the capped
    grid to its second and third trips (and 2 * 524288 + 1203 ends in a scalar tail of three)."""
    assert (n > R.ADAMW_SWEEP) == (n in R.ADAMW_N[-2:]) and R.ADAMW_N[-1] > 2 * R.ADAMW_SWEEP
    adamw_steps(ops, n, "project", "randn", (1, 2, 3))


@pytest.mark.parametrize("hyper", list(R.ADAMW_HYPER))
@pytest.mark.parametrize("family", R.ADAMW_GRADS)
def test_adamw_families(ops, family, hyper):
    adamw_steps(ops, 10007, hyper, family, (1, 2, 3))
    for step in (1000, 100000):
        adamw_steps(ops, 10007, hyper, family, (step,), late=True, seed=190)


@pytest.mark.parametrize("n", [5, 10007, 2 * 524288 + 1203])
def test_adamw_guarded_coef_and_null_shadow(ops, n):
    """The guarded sweep with coef != 1 (the gradient scale is the f32 product gscale coef), and a null shadow."""
    adamw_steps(ops, n, "big-lr-wd", "gscale", (1, 2), coef=0.37)
    adamw_steps(ops, n, "project", "randn", (1000,), late=True, coef=0.37, shadow=False)
    adamw_steps(ops, n, "big-lr", "randn", (1, 2), shadow=False)


def adamw_grid_run(ops):
    p, m, v, sh = adamw_steps(ops, 10007, "big-lr-wd", "randn", (1, 2, 3))
    return [t.cpu() for t in (p, m, v, sh)]


def test_adamw_grid_does_not_matter(ops, tmp_path):
    """MVLT_ADAMW_BLOCKS=3 (read once per process: a fresh child, tests/misc_adamw_worker.py) takes n = 10007 through four
    trips of a three-workgroup grid; the sweep is elementwise, so p, m, v and the shadow equal the default grid's bit for bit."""
    path = str(tmp_path / "adamw_blocks3.pt")
    env = dict(os.environ)
    env["MVLT_ADAMW_BLOCKS"] = "3"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "misc_adamw_worker.py"), path], env=env,
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0 and "ADAMW-GRID-OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    theirs = torch.load(path)
    for name, a, b in zip(("p", "m", "v", "shadow"), adamw_grid_run(ops), theirs):
        check_equal(a, b, f"adamw default grid vs MVLT_ADAMW_BLOCKS=3: {name}")


# ------------------------------------------------------------------ embeddings
CLS_ID, SEP_ID, VOCAB = 1, 2, 300


def embed_struct(L, ops, dt, B, n_img, T, H, ids, word, pos, typ, pos_offset, type_override, pack):
    p = ops._embed_struct(dt, B, n_img, T, H, ids, word, pos, typ, CLS_ID, SEP_ID, pos_offset, type_override)
    if pack is not None:
        p.row_start, p.seq_len = ptr(pack[0]), ptr(pack[1])
    return p


def embed_case(L, ops, dt, B, n_img, T, H, *, pos_offset=0, type_override=-1, lens=None, want_dimage=True, want_dpos=True,
               want_dtype=True, pos_dev=False, seed=0):
    """Forward and backward of one layout.  lens: text lengths of the packed layout (None: dense)."""
    lib = L.lib()
    Lq = T if n_img < 0 else n_img + 2 + T
    pos_rows = pos_offset + Lq + 5
    ids_c = R.embed_ids(B, T, VOCAB, CLS_ID, SEP_ID, 70 + seed) if T else None
    word_c, pos_c, typ_c = (torch.randn(n, H, generator=R.gen(60 + n + seed)) for n in (VOCAB, pos_rows, 3))
    img_c = torch.randn(B, n_img, H, generator=R.gen(66 + seed)).to(dt) if n_img > 0 else None
    ids, word, pos, typ, img = (None if t is None else t.cuda() for t in (ids_c, word_c, pos_c, typ_c, img_c))
    valid = torch.ones(B, Lq, dtype=torch.bool)
    pack = None
    if lens is not None:
        seq = torch.tensor([(0 if n_img < 0 else n_img + 2) + n for n in lens], dtype=torch.int32)
        valid = torch.arange(Lq)[None, :] < seq[:, None]
        pack = ((torch.cumsum(seq, 0) - seq).int().cuda(), seq.cuda())
    rows = valid.reshape(-1).nonzero().flatten()                  # dense row of every materialised row, in packed order
    n_rows = rows.numel()
    what = f"embed {tname(dt)} B={B} n_img={n_img} T={T} H={H} off={pos_offset} type={type_override}" + \
        ("" if lens is None else f" packed{tuple(lens)}")
    # forward: bit for bit the plain statement
    stmt = R.embed_statement(ids_c, img_c, word_c, pos_c, typ_c, CLS_ID, SEP_ID, dt, B=B, n_img=n_img, T=T,
                             pos_offset=pos_offset, type_override=type_override).view(B * Lq, H)[rows]
    for dev in ((False, True) if pos_dev else (False,)):
        out = filled((n_rows + GUARD, H), FILL, dt)
        p = embed_struct(L, ops, dt, B, n_img, T, H, ids, word, pos, typ, i32(pos_offset) if dev else pos_offset, type_override,
                         pack)
        p.image_feature, p.out = ptr(img), ptr(out)
        assert lib.mvlt_embed_fwd(ctypes.byref(p), ops._stream()) == 0, what
        check_equal(out[:n_rows].cpu(), stmt, what + (" forward (pos_offset_dev)" if dev else " forward"))
        check_untouched(out, n_rows, FILL, what + " forward")
    # backward
    dout_c = torch.randn(B, Lq, H, generator=R.gen(67 + seed)).to(dt)
    dout = dout_c.view(B * Lq, H)[rows].contiguous().cuda()
    prior_c = torch.randn(VOCAB, H, generator=R.gen(68 + seed))
    runs = []
    for _ in range(2):
        dword = prior_c.cuda()
        dpos = filled((pos_rows + GUARD, H), FILL) if want_dpos else None
        dty = filled((3 + GUARD, H), -3.0) if want_dtype else None
        dimg = filled((B * n_img + GUARD, H), NAN, dt) if (want_dimage and n_img > 0) else None
        p = embed_struct(L, ops, dt, B, n_img, T, H, ids, word, pos, typ, pos_offset, type_override, pack)
        p.dout, p.dimage, p.dword, p.dpos, p.dtype_emb = ptr(dout), ptr(dimg), ptr(dword), ptr(dpos), ptr(dty)
        p.pos_rows, p.type_rows = (pos_rows if want_dpos else 0), (3 if want_dtype else 0)
        assert lib.mvlt_embed_bwd(ctypes.byref(p), ops._stream()) == 0, what
        runs.append((dword, dpos, dty, dimg))
    dword, dpos, dty, dimg = runs[0]
    for name, a, b in zip(("dpos", "dtype", "dimage"), runs[0][1:], runs[1][1:]):
        if a is not None:
            check_equal(a, b, what + f" {name}: second run")
    wid = R.embed_word_ids(ids_c, B, n_img, T, CLS_ID, SEP_ID)
    ref = R.embed_bwd_ref(dout_c, wid, valid, prior_c, n_img=n_img, pos_rows=pos_rows, type_rows=3, pos_offset=pos_offset,
                          type_override=type_override)
    if dimg is not None:
        check_equal(dimg[:B * n_img].cpu(), dout_c[:, 1:1 + n_img].reshape(B * n_img, H), what + " dimage")
        check_untouched(dimg, B * n_img, NAN, what + " dimage")
    hits = ref["hits"]
    checked("dword", dword.cpu(), ref["dword"], ref["dword_b"], what + " dword")
    check_equal(dword.cpu()[hits == 0], prior_c[hits == 0], what + " untouched dword rows")
    once = hits == 1
    if n_img >= 0:
        once[CLS_ID] = once[SEP_ID] = False              # prior + an ordered batch sum: one rounding only at B = 1
    sel = valid & (wid >= 0)
    one = torch.zeros_like(prior_c).index_add_(0, wid[sel], dout_c.float()[sel])
    check_equal(dword.cpu()[once], (prior_c + one)[once], what + " dword rows hit once")
    if want_dpos:
        checked("dpos", dpos[:pos_rows].cpu(), ref["dpos"], ref["dpos_b"], what + " dpos")
        check_zero(dpos[:pos_rows].cpu()[~ref["pos_used"]], what + " dpos rows outside the window")
        check_untouched(dpos, pos_rows, FILL, what + " dpos")
    if want_dtype:
        checked("dtype", dty[:3].cpu(), ref["dtype"], ref["dtype_b"], what + " dtype_emb")
        check_zero(dty[:3].cpu()[~ref["type_used"]], what + " unused dtype_emb rows")
        check_untouched(dty, 3, -3.0, what + " dtype_emb")
    return dword.cpu(), ref


@pytest.mark.parametrize("dt", DTS, ids=tname)
@pytest.mark.parametrize("H", [4, 36, 256, 768])
@pytest.mark.parametrize("B,n_img,T", [(5, 9, 24), (1, 49, 24), (5, 49, 80)])
def test_embed_dense(L, ops, B, n_img, T, H, dt):
    """L = 35 (below the 64 position lanes), 75 = 64 + 11, 131 (a third trip of the lane loop); H = 4 and 36 end inside the
    32 columns of a position workgroup, 768 takes 24 of them."""
    embed_case(L, ops, dt, B, n_img, T, H)


@pytest.mark.parametrize("dt", DTS, ids=tname)
@pytest.mark.parametrize("H", [36, 256])
def test_embed_variants(L, ops, H, dt):
    embed_case(L, ops, dt, 5, 9, 0, H)                                              # T = 0: [CLS] image [SEP] alone
    embed_case(L, ops, dt, 5, 49, 24, H, pos_offset=7, type_override=2)
    embed_case(L, ops, dt, 5, 49, 24, H, lens=(24, 0, 3, 24, 11))                   # packed, lengths 0 and full among them
    embed_case(L, ops, dt, 1, 9, 24, H, lens=(0,))
    embed_case(L, ops, dt, 5, 9, 24, H, want_dimage=False)
    embed_case(L, ops, dt, 5, 9, 24, H, want_dpos=False)
    embed_case(L, ops, dt, 5, 9, 24, H, want_dtype=False, pos_offset=7)
    embed_case(L, ops, dt, 5, 9, 24, H, want_dpos=False, want_dtype=False, want_dimage=False)


@pytest.mark.parametrize("dt", DTS, ids=tname)
@pytest.mark.parametrize("B,T,H", [(5, 30, 36), (1, 75, 4), (5, 131, 256)])
def test_embed_text_only(L, ops, B, T, H, dt):
    """The cached-step layout (image_feature null, n_img = -1, L = T): the forward with a host and a device position
    offset; the backward is the regression test of the word gradient of text position 0, which embed_bwd_tokens_kernel
    dropped (its [CLS] / [SEP] test read posi == 0 at n_img = -1 and the position kernel adds those rows back only behind
    an image prefix).  Every sample's first word is hit there."""
    dword, ref = embed_case(L, ops, dt, B, -1, T, H, pos_offset=7, pos_dev=True)
    ids = R.embed_ids(B, T, VOCAB, CLS_ID, SEP_ID, 70)
    assert bool((ref["hits"][ids[:, 0]] >= 1).all())
    embed_case(L, ops, dt, B, -1, T, H, type_override=2, seed=1)
    embed_case(L, ops, dt, B, -1, T, H, lens=tuple([T, 0, 3, T, 1][:B]), seed=2)


@pytest.mark.parametrize("dt", DTS, ids=tname)
def test_embed_second_trip(L, ops, dt):
    """B L H / 4 = 48 x 231 x 192 > 8192 x 256: the grid-stride loops of embed_fwd_kernel and embed_bwd_tokens_kernel take a
    second trip.  Forward against the statement, dimage by equality, dpos on a column sample."""
    B, n_img, T, H = 48, 49, 180, 768
    Lq = n_img + 2 + T
    assert B * Lq * (H // 4) > 8192 * 256
    ids_c = R.embed_ids(B, T, VOCAB, CLS_ID, SEP_ID, 80)
    word_c, pos_c, typ_c = (torch.randn(n, H, generator=R.gen(81 + n)) for n in (VOCAB, Lq, 3))
    img_c = torch.randn(B, n_img, H, generator=R.gen(82)).to(dt)
    ids, word, pos, typ, img = (t.cuda() for t in (ids_c, word_c, pos_c, typ_c, img_c))
    out = filled((B * Lq + GUARD, H), FILL, dt)
    p = embed_struct(L, ops, dt, B, n_img, T, H, ids, word, pos, typ, 0, -1, None)
    p.image_feature, p.out = ptr(img), ptr(out)
    assert L.lib().mvlt_embed_fwd(ctypes.byref(p), ops._stream()) == 0
    stmt = R.embed_statement(ids_c, img_c, word_c, pos_c, typ_c, CLS_ID, SEP_ID, dt, B=B, n_img=n_img, T=T)
    check_equal(out[:B * Lq].cpu(), stmt.view(B * Lq, H), "embed second trip: forward")
    check_untouched(out, B * Lq, FILL, "embed second trip: forward")
    dout = torch.randn(B, Lq, H, generator=R.gen(83)).to(dt).cuda()
    dpos, dimg = filled((Lq + GUARD, H), FILL), filled((B * n_img + GUARD, H), NAN, dt)
    p = embed_struct(L, ops, dt, B, n_img, T, H, ids, word, pos, typ, 0, -1, None)
    p.dout, p.dimage, p.dpos, p.pos_rows = ptr(dout), ptr(dimg), ptr(dpos), Lq
    assert L.lib().mvlt_embed_bwd(ctypes.byref(p), ops._stream()) == 0
    check_equal(dimg[:B * n_img], dout[:, 1:1 + n_img].reshape(B * n_img, H), "embed second trip: dimage")
    check_untouched(dimg, B * n_img, NAN, "embed second trip: dimage")
    cols = torch.arange(0, H, 37, device="cuda")
    ref, bound = R.batch_sum_ref(dout[:, :, cols])
    checked("dpos", dpos[:Lq][:, cols], ref, bound, "embed second trip: dpos")
    check_untouched(dpos, Lq, FILL, "embed second trip: dpos")


# ------------------------------------------------------------------ column sums
@pytest.mark.parametrize("dt", DTS, ids=tname)
@pytest.mark.parametrize("M", R.COLSUM_M)
def test_colsum(ops, M, dt):
    """M = 8197 exceeds the cap of 128 row slices, M < 64 is one slice; ld % 4 != 0 and the group that straddles N take the
    scalar loads; columns >= N of the wider tensor are NaN."""
    for N in R.COLSUM_N:
        for kind in R.COLSUM_LD:
            ld = R.colsum_ld(N, kind)
            for family in ("randn", "offset"):
                wide = R.colsum_x(family, M, N, ld, dt, M + N).cuda()
                x = wide[:, :N]
                assert x.data_ptr() % 16 == 0 and (M == 1 or x.stride(0) == ld)
                prev = torch.randn(N, generator=R.gen(3)).cuda()
                for acc in (False, True):
                    buf, out = guarded(N, NAN)
                    if acc:
                        out.copy_(prev)
                    ops.colsum(x, out, accumulate=acc)
                    ref, bound = R.colsum_ref(x, prev if acc else None)
                    what = f"colsum {tname(dt)} M={M} N={N} {kind} {family}" + (" accumulate" if acc else "")
                    checked("colsum " + tname(dt), out, ref, bound, what)
                    check_untouched(buf, N, NAN, what)


# ------------------------------------------------------------------ movers
@pytest.mark.parametrize("dt", DTS, ids=tname)
@pytest.mark.parametrize("rows,C", [(120, 64), (7, 4), (8200, 1028)])
def test_rows_transform_is_the_plain_statement(ops, rows, C, dt):
    """out[i] = x[rowmap[i]] * rowscale[rowmap[i] // rps] in f32, rounded once; 8200 x 1028 / 4 exceeds one capped sweep
    (8192 x 256 vectors)."""
    assert (rows * (C // 4) > 8192 * 256) == (rows == 8200)
    x_c = torch.randn(rows, C, generator=R.gen(70)).to(dt)
    x = x_c.cuda()
    perm_c = torch.randperm(rows, generator=R.gen(3))
    perm = perm_c.int().cuda()
    rps = max(rows // 3, 1)
    rs_c = torch.tensor([0.0, 2.0, 1.5, -0.3])
    rs = rs_c.cuda()
    scale = rs_c[perm_c // rps][:, None]
    for name, kw, stmt in (("rowmap", dict(rowmap=perm), x_c[perm_c]),
                           ("rowmap+rowscale", dict(rowmap=perm, rowscale=(rs, rps)), (x_c.float()[perm_c] * scale).to(dt)),
                           ("rowscale", dict(rowscale=(rs, rps)),
                            (x_c.float() * rs_c[torch.arange(rows) // rps][:, None]).to(dt))):
        out = filled((rows + GUARD, C), FILL, dt)
        ops.rows_transform(x, out=out, **kw)
        check_equal(out[:rows].cpu(), stmt, f"rows_transform {name} {tname(dt)} {rows}x{C}")
        check_untouched(out, rows, FILL, f"rows_transform {name}")


@pytest.mark.parametrize("dt", DTS, ids=tname)
@pytest.mark.parametrize("rows,C,count", [(40, 36, 17), (40, 36, 0), (40, 36, 99), (8200, 1028, 8200)])
def test_rows_scatter_is_the_plain_statement(ops, rows, C, count, dt):
    x = torch.randn(rows, C, generator=R.gen(71)).to(dt).cuda()
    perm = torch.randperm(rows + 5, generator=R.gen(4))[:rows].cuda()
    out = filled((rows + 5 + GUARD, C), FILL, dt)
    ops.rows_scatter(x, perm.int(), i32(count), out)
    n = min(rows, count)
    exp = filled((rows + 5 + GUARD, C), FILL, dt)
    exp[perm[:n]] = x[:n]
    check_equal(out, exp, f"rows_scatter {tname(dt)} rows={rows} count={count}")


@pytest.mark.parametrize("dt", DTS, ids=tname)
@pytest.mark.parametrize("B,Cin,S,P", [(2, 3, 32, 4), (1, 3, 12, 2), (2, 3, 224, 4), (3, 1, 24, 8)])
def test_im2col_is_unfold(L, ops, B, Cin, S, P, dt):
    """The values themselves, not a product with them: F.unfold's (c, dy, dx) columns per patch, patches row-major."""
    img = torch.randn(B, Cin, S, S, generator=R.gen(60)).cuda()
    G, K = S // P, Cin * P * P
    cols = filled((B * G * G + GUARD, K), NAN, dt)
    assert L.lib().mvlt_im2col_patch(ops._DT[dt], ptr(img), ptr(cols), B, Cin, S, P, ops._stream()) == 0
    stmt = F.unfold(img.cpu(), kernel_size=P, stride=P).transpose(1, 2).reshape(B * G * G, K).to(dt)
    check_equal(cols[:B * G * G].cpu(), stmt, f"im2col {tname(dt)} B={B} Cin={Cin} S={S} P={P}")
    check_untouched(cols, B * G * G, NAN, "im2col")


@pytest.mark.parametrize("n", R.CAST_N)
def test_cast_sizes(ops, n):
    """n = 1, 2, 3 and 5 are the scalar tail alone or behind one vector; the last n exceeds 4 x 8192 x 256 (a second trip)."""
    assert (n > 4 * 8192 * 256) == (n == R.CAST_N[-1])
    z = torch.randn(n, generator=R.gen(71)).cuda()
    for src, dst in ((F32, BF), (BF, F32), (F32, F32), (BF, BF)):
        a = z.to(src)
        buf, out = guarded(n, FILL, dst)
        ops.cast(a, dst, out=out)
        assert torch.equal(out, a.to(dst)), f"cast {tname(src)} -> {tname(dst)} n={n}"
        check_untouched(buf, n, FILL, f"cast {tname(src)} -> {tname(dst)} n={n}")


def test_cast_special_values(ops):
    """Ties, +-inf, NaN, the largest finite f32 and f32 denormals, each with its sign.  Finite normals, infinities and
    NaN-ness equal torch's round-to-nearest-even.  For denormal inputs (and results) the contract leaves the device a
    choice that this test measures and reports: exact RNE or a zero of the input's sign.
    Measured on an MI355X: exact RNE for every f32 denormal (2^-149 .. 2^-126 - 2^-149, both signs), and the widening of
    bf16 denormals is exact as well: the device flushes neither."""
    v, den = R.cast_specials()
    exp = v.to(BF)
    out = ops.cast(v.cuda(), BF).cpu()
    assert torch.equal(torch.isnan(out), torch.isnan(exp))
    norm = ~den & ~torch.isnan(v)
    check_equal(out[norm], exp[norm], "cast f32 -> bf16 specials")
    rne = (out[den] == exp[den]) & (torch.signbit(out[den]) == torch.signbit(exp[den]))
    zero = (out[den] == 0) & (torch.signbit(out[den]) == torch.signbit(v[den]))
    assert bool((rne | zero).all()), (v[den][~(rne | zero)], out[den][~(rne | zero)])
    NOTES["cast f32 -> bf16 denormals"] = "exact RNE" if bool(rne.all()) else \
        ("signed zero" if bool(zero.all()) else f"RNE for {int(rne.sum())} of {int(den.sum())}, signed zero for the rest")
    # widening is exact, bf16 denormals included
    b = exp[~torch.isnan(exp)]
    wide = ops.cast(b.cuda(), F32).cpu()
    bden = (b.float().abs() < 2.0 ** -126) & (b != 0)
    check_equal(wide[~bden], b.float()[~bden], "cast bf16 -> f32 specials")
    same = (wide[bden] == b.float()[bden]) | ((wide[bden] == 0) & (torch.signbit(wide[bden]) == torch.signbit(b[bden])))
    assert bool(same.all())
    NOTES["cast bf16 -> f32 denormals"] = "exact" if bool((wide[bden] == b.float()[bden]).all()) else "some flushed to signed zero"


# ------------------------------------------------------------------ unary kernels
def unary_launch(L, ops, name, dt, a, b, n):
    buf, out = guarded(n, NAN, dt)
    fn = getattr(L.lib(), "mvlt_" + name)
    args = (ops._DT[dt], ptr(a)) + ((ptr(b),) if b is not None else ()) + (ptr(out), n, ops._stream())
    assert fn(*args) == 0
    check_untouched(buf, n, NAN, f"{name} n={n}")
    return out


@pytest.mark.parametrize("dt", DTS, ids=tname)
@pytest.mark.parametrize("n", R.UNARY_N)
def test_unary_kernels(L, ops, n, dt):
    """gelu / gelu_bwd / tanh / tanh_bwd per element; n = 8192 x 256 + 257 takes unary_kernel's loop to a second trip; the
    first elements are +-0, +-8 and +-40."""
    x = R.unary_x(n, dt, 5).cuda()
    dy = torch.randn(n, generator=R.gen(6)).to(dt).cuda()
    y = unary_launch(L, ops, "gelu_fwd", dt, x, None, n)
    checked("gelu " + tname(dt), y, *R.unary_ref("gelu", x, None, dt), f"gelu {tname(dt)} n={n}")
    d = unary_launch(L, ops, "gelu_bwd", dt, x, dy, n)
    checked("gelu_bwd " + tname(dt), d, *R.unary_ref("gelu_bwd", x, dy, dt), f"gelu_bwd {tname(dt)} n={n}")
    t = unary_launch(L, ops, "tanh_fwd", dt, x, None, n)
    checked("tanh " + tname(dt), t, *R.unary_ref("tanh", x, None, dt), f"tanh {tname(dt)} n={n}")
    d = unary_launch(L, ops, "tanh_bwd", dt, t, dy, n)
    checked("tanh_bwd " + tname(dt), d, *R.unary_ref("tanh_bwd", t, dy, dt), f"tanh_bwd {tname(dt)} n={n}")


# ------------------------------------------------------------------ report
def report():
    for key, v in sorted(WORST.items()):
        print(f"misc worst ratio  {key:14s} {v:.3f}")
    for key, v in sorted(NOTES.items()):
        print(f"misc device note  {key}: {v}")


def test_report_worst_ratios():
    """Runs last: the worst ratio to the bound per quantity over the cases above, and what the device does with denormals
    (printed with -s)."""
    report()
    assert all(v <= 1.0 for v in WORST.values())
