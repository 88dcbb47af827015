"""The bounds of tests/misc_ref.py prove themselves on the host.

(a) an f32 emulation of each kernel's arithmetic stays within the bound at the shapes and families
    tests/test_misc_routes_gpu.py uses (the largest sizes cut down in rows, not in width): cross entropy with the per-lane
    partial sums at stride 1024 (vector and scalar groups), the wave butterflies and the fold of the four waves,
    __expf as exp2(f32(t log2 e)), the loss atomics in two orders; AdamW in the kernel's order of operations, with and
    without the contractions a compiler may make; the ordered batch sums and the 64 position lanes of the embedding
    backward, its word atomics in two orders; the slices, sub-slices and the final fold of the column sums;
(b) listed faults are rejected, and the message names their place;
(c) the whole-tensor criteria of the older tests (rel < 1e-6 on p, rel < 1e-2 on a bf16 dlogits) accept such faults;
(d) no reference value or bound is NaN or infinite where no poison was planted."""
import math

import pytest
import torch

import misc_ref as R
from misc_ref import BF, F32, check_bound, check_equal, check_zero

WORST = {}
LOG2E = torch.tensor(1.4426950408889634, dtype=F32)


@pytest.fixture(autouse=True, scope="module")
def _one_thread():
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


def tname(dt):
    return "bf16" if dt == BF else "f32"


def inside(key, out, ref, bound, what):
    assert bool(torch.isfinite(ref).all()) and bool(torch.isfinite(bound).all()), f"{what}: non-finite reference or bound"
    out, ref, bound = (t.reshape(-1) if t.dim() == 0 else t for t in (out.double(), ref, bound))
    check_bound(out, ref, bound, what)
    if out.numel():
        WORST[key] = max(WORST.get(key, 0.0), float(((out - ref).abs() / bound).max()))


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def fma(a, b, c):
    return (a.double() * b.double() + c.double()).float()


# ------------------------------------------------------------------ cross entropy
def expf(t):
    return torch.exp2(t * LOG2E)


def ce_fwd_emul(x, V, ld, labels, n_valid, order="fwd", drop_group=None, first_trip_max=False):
    """-> (lse [n_valid], loss_sum, count) as ce_fwd_kernel forms them.  drop_group = (row, group): that 4-column group is
    left out of the row sum; first_trip_max: the maximum is taken over the first 1024 columns only."""
    xv = x[:n_valid, :V].float()
    lab = labels[:n_valid]
    rows = xv.shape[0]
    mx = (xv[:, :1024] if first_trip_max else xv).max(1).values
    J = -(-V // 1024)
    e = torch.zeros(rows, J * 1024)
    e[:, :V] = expf(xv - mx[:, None])
    if drop_group is not None:
        e[drop_group[0], 4 * drop_group[1]:4 * drop_group[1] + 4] = 0.0
    e = e.view(rows, J, 256, 4)
    c0 = (torch.arange(J)[:, None] * 1024 + torch.arange(256)[None, :] * 4)
    vec = (c0 + 3 < V) & (ld % 4 == 0)
    s = torch.zeros(rows, 256)
    for j in range(J):
        q = e[:, j]
        sv = s + (((q[..., 0] + q[..., 1]) + q[..., 2]) + q[..., 3])
        ss = (((s + q[..., 0]) + q[..., 1]) + q[..., 2]) + q[..., 3]
        s = torch.where(vec[j][None, :], sv, ss)
    w = s.view(rows, 4, 64)
    lane = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        w = w + w[..., lane ^ o]
    tot = ((w[:, 0, 0] + w[:, 1, 0]) + w[:, 2, 0]) + w[:, 3, 0]
    lse = mx + torch.log(tot)
    on = lab >= 0
    term = lse - xv.gather(1, lab.clamp(min=0)[:, None])[:, 0]
    loss = torch.zeros((), dtype=F32)
    idx = on.nonzero().flatten().tolist()
    for r in (idx if order == "fwd" else idx[::-1]):
        loss = loss + term[r]
    return torch.where(on, lse, torch.zeros_like(lse)), loss, float(len(idx))


def ce_bwd_emul(x, V, ld, labels, lse, count, gscale, gdev, dtype, n_valid, *, hot_shift=0, raw_count=False, pad_leak=False):
    """-> dl [n_valid, ld] in dtype as ce_bwd_kernel forms it.  Faults: hot_shift (the label's -1 that many columns off),
    raw_count (sc divides by count, not max(count, 1)), pad_leak (column V carries sc exp(.) of the last logit)."""
    xv = x[:n_valid, :V].float()
    lab = labels[:n_valid]
    g = torch.tensor(gscale, dtype=F32) * torch.tensor(gdev, dtype=F32)
    cnt = torch.tensor(float(count), dtype=F32)
    sc = g / (cnt if raw_count else torch.clamp(cnt, min=1.0))
    hot = (torch.arange(V)[None, :] == (lab[:, None] + hot_shift)).float()
    d = sc * (expf(xv - lse[:n_valid, None]) - hot)
    d = torch.where((lab >= 0)[:, None], d, torch.zeros_like(d))
    out = torch.zeros(xv.shape[0], ld)
    out[:, :V] = d
    if pad_leak and ld > V:
        out[:, V] = d[:, V - 1]
    return out.to(dtype)


def ce_case(family, V, ld, dt, rows, rows_dev, seed=0, ignore="third"):
    n_valid = rows if rows_dev is None else rows_dev
    labels = R.ce_labels(rows, V, 11 + seed, ignore)
    x = R.ce_logits(family, rows, V, ld, dt, 12 + seed, labels, n_valid)
    return x, labels, n_valid


def ce_rows(V, name):
    rows, rows_dev = R.CE_ROWS[name]
    if V > 4000:                      # cut down in rows, not in width
        rows, rows_dev = (min(rows, 7), None if rows_dev is None else 4)
    return rows, rows_dev


CE_CPU_CASES = [(V, ld, "third-ignored") for V, ld in R.CE_SHAPES] + [(1025, 1028, "one-row"), (1027, 1027, "one-row"),
                                                                      (2, 4, "one-row"), (1025, 1028, "ragged"),
                                                                      (3000, 3008, "ragged"), (3, 3, "ragged")]


@pytest.mark.parametrize("dt", [F32, BF], ids=tname)
@pytest.mark.parametrize("family", R.CE_FAMILIES)
@pytest.mark.parametrize("V,ld,rowcfg", CE_CPU_CASES)
def test_ce_emulation_inside(V, ld, rowcfg, family, dt):
    rows, rows_dev = ce_rows(V, rowcfg)
    x, labels, n_valid = ce_case(family, V, ld, dt, rows, rows_dev)
    ref = R.ce_fwd_ref(x, V, labels, n_valid)
    assert ref["count"] == int((labels[:n_valid] >= 0).sum())
    for order in ("fwd", "rev"):
        lse, loss, count = ce_fwd_emul(x, V, ld, labels, n_valid, order)
        assert count == ref["count"]
        on = ref["on"]
        check_zero(lse[~on], "lse of ignored rows")
        inside(("ce", "lse"), lse[on], ref["lse"][on], ref["lse_b"][on], f"lse {family} V={V}")
        inside(("ce", "loss_sum"), loss, ref["loss"], ref["loss_b"], f"loss_sum {family} V={V} {order}")
    lse32 = ref["lse"].float()
    dl, dl_b = R.ce_bwd_ref(x, V, labels, lse32, ref["count"], R.CE_GSCALE, R.CE_GSCALE_DEV, dt, n_valid)
    out = ce_bwd_emul(x, V, ld, labels, lse32, ref["count"], R.CE_GSCALE, R.CE_GSCALE_DEV, dt, n_valid)
    inside(("ce", "dl " + tname(dt)), out[:, :V], dl, dl_b, f"dl {family} V={V}")
    check_zero(out[:, V:], "dl pad columns")
    check_zero(out[:, :V][~ref["on"]], "dl of ignored rows")


def test_ce_all_ignored():
    V, ld, rows = 1025, 1028, 5
    labels = R.ce_labels(rows, V, 3, "all")
    x = R.ce_logits("plain", rows, V, ld, F32, 4, labels)
    ref = R.ce_fwd_ref(x, V, labels)
    assert ref["count"] == 0 and float(ref["loss"]) == 0.0 and math.isfinite(float(ref["loss_b"]))
    lse, loss, count = ce_fwd_emul(x, V, ld, labels, rows)
    assert count == 0 and float(loss) == 0.0
    dl, dl_b = R.ce_bwd_ref(x, V, labels, lse, 0.0, 1.0, None, F32)
    check_zero(dl, "reference dl with every label ignored")
    assert bool(torch.isfinite(dl_b).all())
    check_zero(ce_bwd_emul(x, V, ld, labels, lse, 0.0, 1.0, 1.0, F32, rows), "dl with every label ignored")


def test_ce_fault_group_left_out():
    V, ld = 1027, 1027
    x, labels, n = ce_case("plain", V, ld, F32, 8, None)
    ref = R.ce_fwd_ref(x, V, labels, n)
    lse, _, _ = ce_fwd_emul(x, V, ld, labels, n, drop_group=(4, 200))
    with pytest.raises(AssertionError, match=r"worst at row 4, column 0"):
        check_bound(lse[:, None], ref["lse"][:, None], ref["lse_b"][:, None], "lse")
    # the straddling group of the scalar tail too (columns 1024..1026)
    lse, _, _ = ce_fwd_emul(x, V, ld, labels, n, drop_group=(1, 256))
    with pytest.raises(AssertionError, match=r"worst at row 1, column 0"):
        check_bound(lse[:, None], ref["lse"][:, None], ref["lse_b"][:, None], "lse")


def test_ce_fault_max_over_first_trip():
    """logsumexp does not depend on the shift, so a maximum taken over the first 1024 columns only shows where the row's
    spread exceeds the f32 exponent range: the true maximum 80 of row 2 sits behind column 1024, everything else stays below -20 (30 in the other rows:
    exp(50) is finite and their lse is still right)."""
    V, ld, rows = 3000, 3008, 4
    labels = R.ce_labels(rows, V, 5, "none")
    x = R.ce_logits("wide", rows, V, ld, F32, 6, labels)
    x[:, :V] = x[:, :V].clamp(max=-20.0)
    x[2, 1500] = 80.0
    x[[0, 1, 3], 1500] = 30.0
    ref = R.ce_fwd_ref(x, V, labels)
    good, _, _ = ce_fwd_emul(x, V, ld, labels, rows)
    check_bound(good[:, None], ref["lse"][:, None], ref["lse_b"][:, None], "lse")
    lse, _, _ = ce_fwd_emul(x, V, ld, labels, rows, first_trip_max=True)
    with pytest.raises(AssertionError, match=r"worst at row 2, column 0"):
        check_bound(lse[:, None], ref["lse"][:, None], ref["lse_b"][:, None], "lse")


def ce_bwd_setup(dt, V=1025, ld=1028, rows=8, ignore="third"):
    x, labels, n = ce_case("plain", V, ld, dt, rows, None, ignore=ignore)
    ref = R.ce_fwd_ref(x, V, labels, n)
    return x, labels, n, ref["lse"].float(), ref["count"]


@pytest.mark.parametrize("dt", [F32, BF], ids=tname)
def test_ce_fault_label_one_column_off(dt):
    V, ld = 1025, 1028
    x, labels, n, lse, count = ce_bwd_setup(dt)
    labels[3] = 517
    dl, dl_b = R.ce_bwd_ref(x, V, labels, lse, count, 0.5, 3.0, dt)
    check_bound(ce_bwd_emul(x, V, ld, labels, lse, count, 0.5, 3.0, dt, n)[:, :V], dl, dl_b, "dl")
    off = labels.clone()
    off[3] = 518                                          # row 3's -1 lands on column 518
    out = ce_bwd_emul(x, V, ld, off, lse, count, 0.5, 3.0, dt, n)
    with pytest.raises(AssertionError, match=r"2 of \d+ elements outside the bound; worst at row 3, column 51[78]"):
        check_bound(out[:, :V], dl, dl_b, "dl")


def test_ce_fault_count_not_clamped():
    """The backward is handed count = 0 with labelled rows (a count that another launch owns and has not filled): the
    contract is gscale / max(count, 1)."""
    V, ld = 1025, 1028
    x, labels, n, lse, _ = ce_bwd_setup(F32)
    dl, dl_b = R.ce_bwd_ref(x, V, labels, lse, 0.0, 0.5, 3.0, F32)
    assert bool(torch.isfinite(dl).all())
    check_bound(ce_bwd_emul(x, V, ld, labels, lse, 0.0, 0.5, 3.0, F32, n)[:, :V], dl, dl_b, "dl")
    out = ce_bwd_emul(x, V, ld, labels, lse, 0.0, 0.5, 3.0, F32, n, raw_count=True)
    with pytest.raises(AssertionError, match=r"worst at row 0, column 0.*ratio inf"):
        check_bound(out[:, :V], dl, dl_b, "dl")


def test_ce_fault_pad_column_written():
    V, ld = 1025, 1028
    x, labels, n, lse, count = ce_bwd_setup(BF)
    out = ce_bwd_emul(x, V, ld, labels, lse, count, 0.5, 3.0, BF, n, pad_leak=True)
    with pytest.raises(AssertionError, match=r"dl pad columns: \d+ of \d+ elements are not 0; first at row 0, column 0"):
        check_zero(out[:, V:], "dl pad columns")


def test_old_ce_criterion_accepts_a_wrong_lse():
    """One 4-column group left out of every row sum shifts lse by about 4 / V: the bf16 dlogits that follow from it pass
    rel < 1e-2 (and the mean loss moves by 1e-3 of itself, under the old 1e-4 only by luck of the shape), the lse bound
    rejects every row."""
    V, ld, dt = 1025, 1028, BF
    x, labels, n = ce_case("plain", V, ld, dt, 8, None)
    ref = R.ce_fwd_ref(x, V, labels, n)
    xv = x[:, :V].double()
    on = ref["on"]                                  # ignored rows hold lse 0 in the reference: judge the labelled ones
    lse_true = torch.logsumexp(xv, 1)
    lse_bad = torch.log(torch.exp(lse_true) - torch.exp(xv[:, 400:404]).sum(1)).float()
    good, _ = R.ce_bwd_ref(x, V, labels, lse_true.float(), ref["count"], 1.0, None, dt)
    bad = ce_bwd_emul(x, V, ld, labels, lse_bad, ref["count"], 1.0, 1.0, dt, n)
    assert rel(bad[:, :V][on], good[on]) < 1e-2                       # the old criterion: accepted
    with pytest.raises(AssertionError, match=r"lse: \d+ of \d+ elements outside the bound"):
        check_bound(lse_bad[on][:, None], ref["lse"][on][:, None], ref["lse_b"][on][:, None], "lse")


# ------------------------------------------------------------------ AdamW
def adamw_emul(p, g, m, v, lr, wd, step, gscale=1.0, coef=None, *, fused=False, fault=None, betas=R.ADAMW_BETAS,
               eps=R.ADAMW_EPS):
    """adamw_sweep in f32, operation by operation (fused: with the multiply-adds contracted).  Faults: "v-beta1",
    "bias-step-1", "wd-after", "tail" (the last n & 3 elements untouched), ("vector", i) (elements 4 i .. 4 i + 3 untouched)."""
    t = lambda a: torch.tensor(a, dtype=F32)  # noqa: E731
    lr, wd, eps, b1, b2 = t(lr), t(wd), t(eps), t(betas[0]), t(betas[1])
    s = step - 1 if fault == "bias-step-1" else step
    bc1 = t(1.0 - float(b1) ** s)
    bc2s = t(math.sqrt(1.0 - float(b2) ** s))
    gs = t(gscale) if coef is None else t(gscale) * t(coef)
    one = t(1.0)
    gr = g * gs
    c = one - lr * wd
    p1 = p if fault == "wd-after" else p * c
    bv = b1 if fault == "v-beta1" else b2
    if fused:
        m1 = fma(b1.expand_as(m), m, (one - b1) * gr)
        v1 = fma(bv.expand_as(v), v, (one - bv) * gr * gr)
    else:
        m1 = b1 * m + (one - b1) * gr
        v1 = bv * v + (one - bv) * gr * gr
    q = (lr / bc1) * m1 / (torch.sqrt(v1) / bc2s + eps)
    p2 = p1 - q
    if fault == "wd-after":
        p2 = p2 * c
    if fault == "tail":
        k = p.numel() - (p.numel() & 3)
        p2[k:], m1[k:], v1[k:] = p[k:], m[k:], v[k:]
    if isinstance(fault, tuple):
        sl = slice(4 * fault[1], 4 * fault[1] + 4)
        p2[sl], m1[sl], v1[sl] = p[sl], m[sl], v[sl]
    return p2, m1, v1


def adamw_inside(key, out, ref, what):
    for k, o in zip("pmv", out):
        inside(("adamw", k), o, ref[k], ref[k + "_b"], f"{what} {k}")


@pytest.mark.parametrize("hyper", list(R.ADAMW_HYPER))
@pytest.mark.parametrize("family", R.ADAMW_GRADS)
def test_adamw_emulation_inside(family, hyper):
    lr, wd = R.ADAMW_HYPER[hyper]
    for n in (1, 5, 1023, 10007):
        for fused in (False, True):
            p = torch.randn(n, generator=R.gen(90))
            m, v = torch.zeros(n), torch.zeros(n)
            for step in (1, 2, 3):
                g, gscale = R.adamw_grad(family, n, 90 + step)
                ref = R.adamw_ref(p, g, m, v, lr, wd, step, gscale)
                out = adamw_emul(p, g, m, v, lr, wd, step, gscale, fused=fused)
                adamw_inside("seq", out, ref, f"adamw {family} {hyper} n={n} step={step}")
                if family == "zeros-third":
                    z = slice(0, None, 3)
                    assert not bool(torch.isnan(out[0]).any())
                    if step == 1:       # m = v = 0 and g = 0: the decayed parameter, nothing else
                        c = 1.0 - R.f32(lr) * R.f32(wd)
                        assert bool(((out[0][z].double() - p[z].double() * c).abs() <= ref["p_b"][z]).all())
                p, m, v = out
            for step in (1000, 100000):
                p = torch.randn(n, generator=R.gen(91))
                m = 0.1 * torch.randn(n, generator=R.gen(92))
                v = torch.rand(n, generator=R.gen(93)) * 0.01 + 1e-8
                g, gscale = R.adamw_grad(family, n, 94)
                ref = R.adamw_ref(p, g, m, v, lr, wd, step, gscale, coef=0.37)
                out = adamw_emul(p, g, m, v, lr, wd, step, gscale, coef=0.37, fused=fused)
                adamw_inside("late", out, ref, f"adamw {family} {hyper} n={n} step={step}")


def adamw_fault_case(n, hyper, step, seed=95):
    lr, wd = R.ADAMW_HYPER[hyper]
    p = torch.randn(n, generator=R.gen(seed))
    m = 0.1 * torch.randn(n, generator=R.gen(seed + 1))
    v = torch.rand(n, generator=R.gen(seed + 2)) * 0.01 + 1e-4
    g = torch.randn(n, generator=R.gen(seed + 3))
    return (p, g, m, v, lr, wd, step), R.adamw_ref(p, g, m, v, lr, wd, step)


@pytest.mark.parametrize("fault,hyper,key", [("v-beta1", "project", "v"), ("bias-step-1", "project", "p"),
                                             ("wd-after", "big-lr-wd", "p")])
def test_adamw_fault_formula(fault, hyper, key):
    args, ref = adamw_fault_case(1023, hyper, 2)
    good = dict(zip("pmv", adamw_emul(*args)))
    check_bound(good[key], ref[key], ref[key + "_b"], key)
    out = dict(zip("pmv", adamw_emul(*args, fault=fault)))
    with pytest.raises(AssertionError, match=rf"{key}: \d+ of 1023 elements outside the bound; worst at row \d+, column 0"):
        check_bound(out[key], ref[key], ref[key + "_b"], key)


def test_adamw_fault_tail_untouched_and_old_criterion():
    """The last n & 3 elements left as they were: rel(p) is 4e-5 sqrt(3 / 10007) = 7e-7 < 1e-6, so the old check of
    test_adamw_matches_torch accepts it (as it accepts a 2 % error in EVERY update: 0.02 x 4e-5); the bound names them."""
    n = 10007
    args, ref = adamw_fault_case(n, "project", 2)
    out = adamw_emul(*args, fault="tail")
    assert rel(out[0], ref["p"]) < 1e-6
    lr, wd = R.ADAMW_HYPER["project"]
    p, g, m, v = args[:4]
    good = adamw_emul(*args)
    two_percent = p * (1.0 - lr * wd) + 1.02 * (good[0] - p * (1.0 - lr * wd))
    assert rel(two_percent, ref["p"]) < 1e-6
    with pytest.raises(AssertionError, match=r"p: \d+ of 10007 elements outside the bound"):
        check_bound(two_percent, ref["p"], ref["p_b"], "p")
    for k, o in zip("pmv", out):
        with pytest.raises(AssertionError, match=rf"{k}: 3 of 10007 elements outside the bound; worst at row 1000[456], column 0"):
            check_bound(o, ref[k], ref[k + "_b"], k)


def test_adamw_fault_vector_of_second_trip_untouched():
    n = R.ADAMW_SWEEP + 4
    args, ref = adamw_fault_case(n, "project", 2)
    i = R.ADAMW_SWEEP // 4                      # the first vector of the second trip
    out = adamw_emul(*args, fault=("vector", i))
    assert rel(out[0], ref["p"]) < 1e-6        # the old criterion: accepted
    for k, o in zip("pmv", out):
        with pytest.raises(AssertionError, match=rf"{k}: 4 of {n} elements outside the bound; worst at row 52428[89]|52429[01], column 0"):
            check_bound(o, ref[k], ref[k + "_b"], k)


# ------------------------------------------------------------------ embeddings
def seq_sum(terms):
    """f32 sum in list order, from 0."""
    s = torch.zeros_like(terms[0])
    for t in terms:
        s = s + t
    return s


def embed_bwd_emul(dout, wid, valid, prior, *, n_img, cls_id, sep_id, pos_rows, type_rows, pos_offset=0, type_override=-1,
                   order="fwd", fault=None):
    """embed_bwd_tokens_kernel + embed_bwd_pos_kernel in f32.  Faults: ("dpos-sample", posi) (the last sample missing from
    that row), "text-only-pos0" (the parent's bug: the word gradient of position 0 dropped when n_img < 0), "type-swap"."""
    B, L, H = dout.shape
    g = dout.float() * valid[:, :, None].float()
    dword = prior.clone().float()
    special = (lambda posi: n_img >= 0 and posi in (0, n_img + 1))
    hits = [(b, posi) for b in range(B) for posi in range(L) if valid[b, posi] and wid[b, posi] >= 0 and not special(posi)]
    if fault == "text-only-pos0" and n_img < 0:
        hits = [h for h in hits if h[1] != 0]
    for b, posi in (hits if order == "fwd" else hits[::-1]):
        dword[wid[b, posi]] += g[b, posi]
    sx = []
    for posi in range(L):
        nb = B - 1 if fault == ("dpos-sample", posi) else B
        sx.append(seq_sum([g[b, posi] for b in range(nb)]))
    dpos = torch.zeros(pos_rows, H)
    for posi in range(L):
        dpos[pos_offset + posi] = sx[posi]
        if special(posi):
            dword[cls_id if posi == 0 else sep_id] += sx[posi]
    dty = torch.zeros(type_rows, H)
    first = [type_override >= 0 or posi > n_img + 1 for posi in range(L)]
    for which in (0, 1):
        lanes = [seq_sum([sx[posi] for posi in range(pl, L, 64) if first[posi] == (which == 0)] or [torch.zeros(H)])
                 for pl in range(64)]
        s = seq_sum(lanes)
        if which == 0:
            dty[type_override if type_override >= 0 else 0] = s
        elif type_override < 0:
            dty[1] = s
    if fault == "type-swap":
        dty[[0, 1]] = dty[[1, 0]]
    return dword, dpos, dty


def embed_case(B, n_img, T, H, dt, *, vocab=40, seed=0, lens=None):
    cls_id, sep_id = 1, 2
    L = T if n_img < 0 else n_img + 2 + T
    ids = R.embed_ids(B, T, vocab, cls_id, sep_id, 70 + seed) if T else None
    wid = R.embed_word_ids(ids, B, n_img, T, cls_id, sep_id)
    valid = torch.ones(B, L, dtype=torch.bool)
    if lens is not None:
        valid = torch.arange(L)[None, :] < torch.tensor(lens)[:, None]
    dout = torch.randn(B, L, H, generator=R.gen(71 + seed)).to(dt)
    prior = torch.randn(vocab, H, generator=R.gen(72 + seed))
    return dout, wid, valid, prior, cls_id, sep_id


EMBED_CPU_CASES = [
    # B, n_img, T, H, pos_offset, type_override, packed lengths
    (5, 9, 24, 36, 0, -1, None), (1, 9, 24, 4, 0, -1, None), (5, 49, 24, 36, 7, 2, None), (5, 60, 80, 4, 0, -1, None),
    (5, 9, 0, 36, 0, -1, None), (5, 9, 24, 36, 0, -1, (35, 11, 0, 20, 35)), (5, -1, 30, 36, 7, -1, None),
    (1, -1, 75, 4, 0, -1, None), (5, 9, 24, 256, 0, -1, None), (1, 49, 24, 768, 0, -1, None),
]


@pytest.mark.parametrize("dt", [F32, BF], ids=tname)
@pytest.mark.parametrize("B,n_img,T,H,pos_offset,type_override,lens", EMBED_CPU_CASES)
def test_embed_bwd_emulation_inside(B, n_img, T, H, pos_offset, type_override, lens, dt):
    dout, wid, valid, prior, cls_id, sep_id = embed_case(B, n_img, T, H, dt, lens=lens)
    L = dout.shape[1]
    kw = dict(n_img=n_img, pos_rows=pos_offset + L + 5, type_rows=3, pos_offset=pos_offset, type_override=type_override)
    ref = R.embed_bwd_ref(dout, wid, valid, prior, **kw)
    for order in ("fwd", "rev"):
        dword, dpos, dty = embed_bwd_emul(dout, wid, valid, prior, cls_id=cls_id, sep_id=sep_id, order=order, **kw)
        inside(("embed", "dword"), dword, ref["dword"], ref["dword_b"], "dword")
        inside(("embed", "dpos"), dpos, ref["dpos"], ref["dpos_b"], "dpos")
        inside(("embed", "dtype"), dty, ref["dtype"], ref["dtype_b"], "dtype")
        check_equal(dword[ref["hits"] == 0], prior[ref["hits"] == 0], "untouched dword rows")
        check_zero(dpos[~ref["pos_used"]], "dpos rows outside the window")
        check_zero(dty[~ref["type_used"]], "unused dtype rows")
        once = ref["hits"] == 1
        if n_img >= 0:
            once[cls_id] = once[sep_id] = False
        idx = wid[valid & (wid >= 0)]
        gsum = torch.zeros_like(prior).index_add_(0, idx, dout.float()[valid & (wid >= 0)])
        check_equal(dword[once], (prior + gsum)[once], "dword rows hit once")


def test_embed_fault_sample_missing_from_dpos():
    dout, wid, valid, prior, cls_id, sep_id = embed_case(5, 9, 24, 36, F32)
    kw = dict(n_img=9, pos_rows=40, type_rows=3)
    ref = R.embed_bwd_ref(dout, wid, valid, prior, **kw)
    _, dpos, _ = embed_bwd_emul(dout, wid, valid, prior, cls_id=cls_id, sep_id=sep_id, fault=("dpos-sample", 17), **kw)
    with pytest.raises(AssertionError, match=r"dpos: 36 of \d+ elements outside the bound; worst at row 17, column"):
        check_bound(dpos, ref["dpos"], ref["dpos_b"], "dpos")


def test_embed_fault_text_only_position_0_dropped():
    """The bug this suite found in embed_bwd_tokens_kernel: with n_img = -1 the [CLS] / [SEP] test read posi == 0."""
    dout, wid, valid, prior, cls_id, sep_id = embed_case(5, -1, 30, 36, F32)
    wid[:, 0] = torch.tensor([7, 7, 9, 11, 13])                  # the words of position 0
    wid[:, 1:][(wid[:, 1:] == 9) | (wid[:, 1:] == 11)] = 5       # words 9 and 11 occur at position 0 only
    kw = dict(n_img=-1, pos_rows=40, type_rows=3)
    ref = R.embed_bwd_ref(dout, wid, valid, prior, **kw)
    good, _, _ = embed_bwd_emul(dout, wid, valid, prior, cls_id=cls_id, sep_id=sep_id, **kw)
    check_bound(good, ref["dword"], ref["dword_b"], "dword")
    dword, _, _ = embed_bwd_emul(dout, wid, valid, prior, cls_id=cls_id, sep_id=sep_id, fault="text-only-pos0", **kw)
    with pytest.raises(AssertionError, match=r"dword: \d+ of \d+ elements outside the bound; worst at row (7|9|11|13), column"):
        check_bound(dword, ref["dword"], ref["dword_b"], "dword")
    assert bool(((dword - good)[[7, 9, 11, 13]] != 0).all()) and torch.equal(dword[9], prior[9])


def test_embed_fault_type_rows_swapped():
    dout, wid, valid, prior, cls_id, sep_id = embed_case(5, 9, 24, 36, BF)
    kw = dict(n_img=9, pos_rows=40, type_rows=3)
    ref = R.embed_bwd_ref(dout, wid, valid, prior, **kw)
    _, _, dty = embed_bwd_emul(dout, wid, valid, prior, cls_id=cls_id, sep_id=sep_id, fault="type-swap", **kw)
    with pytest.raises(AssertionError, match=r"dtype: 72 of 108 elements outside the bound; worst at row [01], column"):
        check_bound(dty, ref["dtype"], ref["dtype_b"], "dtype")


def test_embed_statement_is_the_oracle_sum():
    """embed_statement against the unordered float64 sum: within two f32 roundings and the output rounding."""
    B, n_img, T, H = 3, 9, 24, 36
    ids = R.embed_ids(B, T, 40, 1, 2, 5)
    word, pos, typ = (torch.randn(n, H, generator=R.gen(6 + n)) for n in (40, 60, 3))
    img = torch.randn(B, n_img, H, generator=R.gen(9)).to(BF)
    out = R.embed_statement(ids, img, word, pos, typ, 1, 2, BF, B=B, n_img=n_img, T=T, pos_offset=7)
    wid = R.embed_word_ids(ids, B, n_img, T, 1, 2)
    src = word.double()[wid.clamp(min=0)]
    src[:, 1:1 + n_img] = img.double()
    ref = src + typ.double()[R.embed_types(n_img + 2 + T, n_img, -1)][None] + pos.double()[7:7 + n_img + 2 + T][None]
    mag = src.abs() + typ.abs().max() + pos.abs().max()
    assert bool(((out.double() - ref).abs() <= 2 * R.U32 * mag + R.U_BF16 * ref.abs()).all())


# ------------------------------------------------------------------ column sums
def colsum_emul(x, M, N, ld, *, prev=None, drop_slice=None, drop_straddle_last=False):
    """colsum_partial_kernel + colsum_final_kernel in f32 (the vector and the scalar loads add the same values in the same
    order).  Faults: drop_slice (that partial row left at 0), drop_straddle_last (column N - 1 of a straddling group never
    added)."""
    xv = x[:, :N].float()
    slices = max(1, min(R.COLSUM_SLICES, M // 64))
    rows_per = -(-M // slices)
    part = torch.zeros(slices, N)
    for s in range(slices):
        r0, r1 = s * rows_per, min(M, (s + 1) * rows_per)
        sub = [seq_sum([xv[r] for r in range(r0 + k, r1, 4)] or [torch.zeros(N)]) for k in range(4)]
        part[s] = ((sub[0] + sub[1]) + sub[2]) + sub[3]
    if drop_slice is not None:
        part[drop_slice] = 0.0
    if drop_straddle_last:
        assert N % 4 != 0
        part[:, N - 1] = 0.0
    w = [seq_sum([part[i] for i in range(k, slices, 4)] or [torch.zeros(N)]) for k in range(4)]
    s = ((w[0] + w[1]) + w[2]) + w[3]
    return s if prev is None else prev + s


@pytest.mark.parametrize("dt", [F32, BF], ids=tname)
@pytest.mark.parametrize("M", [m for m in R.COLSUM_M if m <= 3000] + [8197])
def test_colsum_emulation_inside(M, dt):
    for N in (R.COLSUM_N if M <= 129 else (5, 388)):
        for kind in R.COLSUM_LD:
            ld = R.colsum_ld(N, kind)
            assert ld >= N and (ld == N) == (kind == "ld==N") and ((ld % 4 == 0) or kind != "ld>N,ld%4==0")
            for family in ("randn", "offset"):
                wide = R.colsum_x(family, M, N, ld, dt, M + N)
                prev = torch.randn(N, generator=R.gen(3))
                for pv in (None, prev):
                    ref, bound = R.colsum_ref(wide[:, :N], pv)
                    inside(("colsum", tname(dt)), colsum_emul(wide, M, N, ld, prev=pv), ref, bound,
                           f"colsum M={M} N={N} {kind} {family}")


def test_colsum_faults():
    M, N = 3000, 257
    wide = R.colsum_x("offset", M, N, R.colsum_ld(N, "ld>N,ld%4!=0"), BF, 1)
    ref, bound = R.colsum_ref(wide[:, :N])
    out = colsum_emul(wide, M, N, wide.shape[1], drop_slice=17)
    with pytest.raises(AssertionError, match=rf"colsum: {N} of {N} elements outside the bound"):
        check_bound(out, ref, bound, "colsum")
    # zero-mean data: one slice of 46 is 1 / 46 of a sum that is itself a random walk -- still far outside
    wide = R.colsum_x("randn", M, N, N, F32, 2)
    ref, bound = R.colsum_ref(wide)
    out = colsum_emul(wide, M, N, N, drop_slice=3)
    with pytest.raises(AssertionError, match=r"colsum: 2\d\d of 257 elements outside the bound"):
        check_bound(out, ref, bound, "colsum")
    out = colsum_emul(wide, M, N, N, drop_straddle_last=True)
    with pytest.raises(AssertionError, match=r"colsum: 1 of 257 elements outside the bound; worst at row 256, column 0"):
        check_bound(out, ref, bound, "colsum")


# ------------------------------------------------------------------ elementwise and the helpers
def test_unary_references_are_finite_and_reject_a_wrong_branch():
    x = R.unary_x(257, F32, 1)
    dy = torch.randn(257, generator=R.gen(2))
    for op, a, b in (("gelu", x, None), ("tanh", x, None), ("gelu_bwd", x, dy), ("tanh_bwd", torch.tanh(x), dy)):
        ref, bound = R.unary_ref(op, a, b, F32)
        assert bool(torch.isfinite(ref).all()) and bool(torch.isfinite(bound).all()), op
        check_bound(ref.float(), ref, bound, op)
    ref, bound = R.unary_ref("gelu", x, None, F32)
    tanh_gelu = torch.nn.functional.gelu(x, approximate="tanh")           # the other GELU: off by up to 5e-4
    with pytest.raises(AssertionError, match=r"gelu: \d+ of 257 elements outside the bound"):
        check_bound(tanh_gelu, ref, bound, "gelu")


def test_cast_specials_cover_the_rules():
    v, den = R.cast_specials()
    b = v.to(BF)
    assert int(den.sum()) == 14 and bool(torch.isnan(b[-2:]).all()) and bool(torch.isinf(b[v.abs() > 3.39e38]).all())
    assert float(b[0]) == 1.0 and float(b[1]) == 1.0 + 2.0 ** -6          # ties to even: down, then up


def test_check_helpers_name_the_place():
    a = torch.zeros(4, 6)
    b = a.clone()
    b[2, 5] = -0.0
    with pytest.raises(AssertionError, match=r"x: 1 of 24 elements differ; first at row 2, column 5"):
        check_equal(b, a, "x")
    b[2, 5] = 1e-45
    with pytest.raises(AssertionError, match=r"x: 1 of 24 elements are not 0; first at row 2, column 5"):
        check_zero(b, "x")
    n = torch.full((3,), math.nan)
    check_equal(n, n.clone(), "nan")


def test_report_worst_ratios():
    """Runs last: the worst ratio of the emulations to the bounds (printed with -s); a correct kernel leaves room."""
    for key, v in sorted(WORST.items()):
        print(f"misc emulation worst ratio  {key[0]:8s} {key[1]:10s} {v:.3f}")
    assert WORST and all(v <= 1.0 for v in WORST.values())
