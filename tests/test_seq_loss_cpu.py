"""The sequence loss on the host: the float64 reference of tests/seq_loss_ref.py against naive loops, torch autograd and
F.cross_entropy; its bounds against wrong results; the C ABI of the three entry points; the refusals that fire before a launch."""
import math
import os
import re
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import seq_loss_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF, F32 = torch.bfloat16, torch.float32
EOS = R.EOS


def _naive_len(row, eos):
    """The issue's sentence, word for word."""
    T = len(row)
    if eos is not None:
        for t in range(T):
            if row[t] == eos:
                return t + 1
    for t in range(T):
        if row[t] <= 0:
            return t
    return T


EDGE_ROWS = [
    ([EOS, 5, 6, 7, 8, 9], EOS, 1),                  # eos at position 0
    ([5, 6, EOS, 7, 0, 0], EOS, 3),                  # in the middle
    ([5, 6, 7, 8, 9, EOS], EOS, 6),                  # at T - 1
    ([5, 6, 7, 8, 9, 10], EOS, 6),                   # neither eos nor PAD
    ([5, 0, 7, EOS, 9, 10], EOS, 4),                 # a PAD ahead of an eos: the eos ends the row
    ([0, 0, 0, 0, 0, 0], EOS, 0),                    # all PAD
    ([5, 6, EOS, 7, 0, 0], None, 4),                 # eos=None: only PAD ends a row
    ([5, 6, 7, 0, 0, 0], EOS, 3),                    # PAD-terminated
]


def test_lengths_of_the_edge_rows():
    for row, eos, want in EDGE_ROWS:
        assert R.seq_len(row, eos) == want == _naive_len(row, eos), (row, eos)
    assert R.seq_len([5, EOS], -1) == 2              # a negative eos means none


@pytest.mark.parametrize("layout", ["b", "bt"])
@pytest.mark.parametrize("eos", [EOS, None])
def test_plan_reference_equals_a_naive_per_sample_loop(layout, eos):
    ids = torch.tensor([r for r, _, _ in EDGE_ROWS], dtype=torch.int64)
    B, T = ids.shape
    w = R.plan_weights(B, T, layout, 5)
    row0, step = 51, 57
    plan = R.plan_ref(ids, eos, w, row0, step)
    lens = [_naive_len(r, eos) for r in ids.tolist()]
    assert plan["len"].tolist() == lens and plan["rows"] == sum(lens)
    # scored positions sample by sample, then everything else in (b, t) order
    scored = [(b, t) for b in range(B) for t in range(lens[b])]
    rest = [(b, t) for b in range(B) for t in range(lens[b], T)]
    order = scored + rest
    assert plan["gather_row"].tolist() == [row0 + b * step + t for b, t in order]
    assert plan["sel_labels"].tolist() == [int(ids[b, t]) for b, t in scored] + [-100] * len(rest)
    wt = w if layout == "bt" else w[:, None].expand(B, T)
    assert plan["row_weight"].tolist() == [float(wt[b, t]) for b, t in scored] + [0.0] * len(rest)
    tf = ids.clone()
    for b in range(B):
        tf[b, lens[b]:] = 0
    assert torch.equal(plan["tf_ids"], tf)
    # the same packing as a stable partition of the implied labels (what ops.label_plan computes)
    lab = R.implied_labels(ids, eos).reshape(-1)
    on = (lab >= 0).nonzero().flatten().tolist()
    assert plan["sel_labels"][:len(on)].tolist() == lab[on].tolist() and len(on) == plan["rows"]


def test_a_negative_id_ahead_of_an_eos_keeps_its_slot_unscored():
    ids = torch.tensor([[5, -7, 6, EOS, 9]], dtype=torch.int64)
    plan = R.plan_ref(ids, EOS, torch.tensor([2.0]), 10, 20)
    assert plan["len"].tolist() == [4] and plan["rows"] == 4
    assert plan["sel_labels"].tolist() == [5, -100, 6, EOS, -100]
    assert plan["row_weight"].tolist() == [2.0, 0.0, 2.0, 2.0, 0.0]
    assert plan["tf_ids"].tolist() == [[5, 0, 6, EOS, 0]]


def _packed_problem(seed, V=23):
    """A plan and f64 logits on its packed rows."""
    ids = R.plan_ids(9, 7, seed) % V
    ids[ids == 0] = 1
    ids = torch.where(R.plan_ids(9, 7, seed) <= 0, torch.zeros_like(ids), ids)
    w = R.plan_weights(9, 7, "bt", seed + 1)
    plan = R.plan_ref(ids, None, w, 0, 7)
    x = torch.randn(9 * 7, V, dtype=torch.float64, generator=R.gen(seed + 2), requires_grad=True)
    return ids, w, plan, x


def test_reference_loss_and_gradient_equal_torch_autograd():
    ids, w, plan, x = _packed_problem(11)
    n = plan["rows"]
    lab, rw = plan["sel_labels"], plan["row_weight"]
    # torch: log_softmax -> gather -> weights -> mask, on the packed rows
    logp = torch.log_softmax(x, 1).gather(1, lab.clamp(min=0)[:, None])[:, 0]
    mask = (torch.arange(x.shape[0]) < n).double()
    loss = -(rw.double() * logp * mask).sum() / n
    loss.backward()
    lse = torch.logsumexp(x.detach(), 1)
    xl = x.detach().gather(1, lab.clamp(min=0)[:, None])[:, 0]
    s = (rw[:n].double() * (lse[:n] - xl[:n])).sum()
    assert abs(float(s) / n - loss.item()) <= 1e-12 * abs(loss.item())
    # closed form: c_i (softmax - onehot), c_i = w_i / N
    c = rw[:n].double() / n
    p = torch.exp(x.detach()[:n] - lse[:n, None])
    hot = (torch.arange(x.shape[1])[None, :] == lab[:n, None]).double()
    closed = c[:, None] * (p - hot)
    assert torch.allclose(x.grad[:n], closed, rtol=1e-12, atol=1e-15)
    assert bool((x.grad[n:] == 0).all())
    # and seq_loss_ref's own functions state the same numbers (f32 operands: take them from f32 copies)
    x32 = x.detach().float()
    lse32 = torch.logsumexp(x32.double(), 1).float()
    xl32 = x32.gather(1, lab.clamp(min=0)[:, None])[:, 0]
    got, bound, _ = R.seq_sum_ref(lse32, xl32, rw, n)
    assert abs(got - float((rw[:n].double() * (lse32[:n].double() - xl32[:n].double())).sum())) <= bound
    dl, _ = R.weighted_dl_ref(x32, x.shape[1], lab, lse32, rw, float(n), 1.0, None, F32, n_valid=n)
    p32 = torch.exp(x32[:n].double() - lse32[:n, None].double())
    assert torch.allclose(dl, c[:, None] * (p32 - hot), rtol=1e-12, atol=1e-18)


def test_unit_weights_are_the_mean_cross_entropy():
    ids, _, _, x = _packed_problem(12)
    plan = R.plan_ref(ids, None, torch.ones(9), 0, 7)
    n = plan["rows"]
    lab = plan["sel_labels"]
    ce = F.cross_entropy(x, lab, ignore_index=-100, reduction="mean")
    ce.backward()
    x32 = x.detach()
    lse = torch.logsumexp(x32, 1)
    xl = x32.gather(1, lab.clamp(min=0)[:, None])[:, 0]
    s = (plan["row_weight"][:n].double() * (lse[:n] - xl[:n])).sum() / n
    assert abs(float(s) - ce.item()) <= 1e-12 * abs(ce.item())
    c = plan["row_weight"][:n].double() / n
    p = torch.exp(x32[:n] - lse[:n, None])
    hot = (torch.arange(x.shape[1])[None, :] == lab[:n, None]).double()
    assert torch.allclose(x.grad[:n], c[:, None] * (p - hot), rtol=1e-12, atol=1e-15)


def _f32_emulation(x, V, labels, lse, w, count, dtype):
    """The kernel's f32 sequence with torch's IEEE f32 operations (torch.exp in place of __expf: inside the bound's exp term)."""
    sc = torch.tensor(R.GSCALE, dtype=F32) * torch.tensor(R.GSCALE_DEV, dtype=F32) / max(torch.tensor(count, dtype=F32), torch.tensor(1.0))
    c = sc * w
    xv = x[:, :V].float()
    live = ((labels >= 0) & (w != 0))[:, None]
    t = torch.where(live, xv - lse[:, None], torch.zeros_like(xv))
    hot = (torch.arange(V)[None, :] == labels[:, None]).float()
    return torch.where(live, c[:, None] * (torch.exp(t) - hot), torch.zeros_like(xv)).to(dtype)


@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", R.SMALL, ids=lambda s: "x".join(map(str, s)))
def test_bounds_accept_an_f32_emulation_and_reject_wrong_results(shape, dtype):
    rows, V, ld = shape
    x, labels, w, lse, count = R.weighted_case(rows, V, ld, dtype, seed=rows * V)
    dl, bound = R.weighted_dl_ref(x, V, labels, lse, w, count, R.GSCALE, R.GSCALE_DEV, dtype)
    good = _f32_emulation(x, V, labels, lse, w, count, dtype)
    R.check_bound(good, dl, bound, "emulation")
    ratio = float(((good.double() - dl).abs() / bound).max())
    print(f"{shape} {dtype}: emulation at {ratio:.3f} of the bound")
    assert ratio <= 0.5
    assert bool((good[R.ZERO_ROW] == 0).all()) and bool((good[R.IGNORED_ROW] == 0).all())
    # (a) the row weight dropped
    with pytest.raises(AssertionError, match="outside the bound"):
        R.check_bound(_f32_emulation(x, V, labels, lse, torch.ones_like(w), count, dtype), dl, bound, "weight dropped")
    # (b) the coefficient of the neighbouring row
    with pytest.raises(AssertionError, match="outside the bound"):
        R.check_bound(_f32_emulation(x, V, labels, lse, torch.roll(w, -1), count, dtype), dl, bound, "neighbour's c_i")
    # (c) one element off by four bf16 ulps
    bad = good.clone()
    r = 1
    col = int(dl[r].abs().argmax())
    v = float(good[r, col])
    ulp = 2.0 ** (math.floor(math.log2(abs(v))) - 7)
    bad[r, col] = v + 4 * ulp
    with pytest.raises(AssertionError, match=f"row {r}, column {col}"):
        R.check_bound(bad, dl, bound, "four ulps")


def test_sum_bound_accepts_the_kernels_order_and_rejects_a_dropped_weight():
    g = R.gen(3)
    n = 4800
    lse = (8.0 + torch.randn(n, generator=g)).float()
    xl = (lse - 6.0 * torch.rand(n, generator=g)).float()
    w = torch.randn(n, generator=g).float()
    w[::7] = 0.0
    lse[7], xl[14] = math.inf, math.nan                   # rows of weight 0: never read
    ref, bound, _ = R.seq_sum_ref(lse, xl, w, n)
    # thread t takes rows t, t + 1024, ...; then the tree
    part = torch.zeros(1024, dtype=F32)
    for i in range(n):
        if w[i] != 0:
            part[i % 1024] = part[i % 1024] + w[i] * (lse[i] - xl[i])
    o = 512
    while o:
        part[:o] = part[:o] + part[o:2 * o]
        o //= 2
    assert abs(float(part[0]) - ref) <= 0.5 * bound, (float(part[0]), ref, bound)
    plain = float((torch.where(w != 0, lse - xl, torch.zeros_like(lse))).double().sum())
    assert abs(plain - ref) > bound
    assert R.seq_sum_ref(lse, xl, w, 0)[0] == 0.0


def test_cabi_declares_binds_and_exports_the_three_entry_points():
    from mvlt_amd import _lib, ops
    hdr = open(os.path.join(ROOT, "include", "mvlt_hip.h")).read()
    for name, nargs in (("mvlt_seq_loss_plan", 17), ("mvlt_seq_loss_fwd", 7), ("mvlt_ce_bwd_weighted", 14)):
        proto = re.search(r"\bint " + name + r"\(([^;]*?)\);", hdr, re.S).group(1)
        assert len(proto.split(",")) == nargs == len(_lib.SYMBOLS[name][1]), name
        assert _lib.SYMBOLS[name][0] is _lib.i32 and hasattr(_lib.lib(), name), name
        for decl, ct in zip(proto.split(","), _lib.SYMBOLS[name][1]):
            decl = " ".join(decl.split())
            want = _lib.vp if "*" in decl else _lib.i64 if decl.startswith("int64_t") else \
                _lib.f32 if decl.startswith("float") else _lib.i32
            assert ct is want, (name, decl)
    assert int(re.search(r"#define\s+MVLT_ABI_VERSION\s+(\d+)", hdr).group(1)) == 17 == _lib.ABI_VERSION == _lib.lib().mvlt_version()
    assert re.search(r"MVLT_STRUCT_COUNT = 21\b", hdr) and len(_lib.STRUCTS) == 21
    assert (ops.SEQ_LOSS_MAX_B, ops.SEQ_LOSS_MAX_T) == (4096, 512)
    for fn in ("seq_loss_plan", "seq_loss_fwd", "ce_bwd_weighted"):
        assert callable(getattr(ops, fn))
    import mvlt_amd
    assert mvlt_amd.self_critical_loss is mvlt_amd.scst.self_critical_loss
    assert callable(mvlt_amd.MVLBertForImageCaption.sequence_loss)


@pytest.fixture(scope="module")
def cpu_model():
    import mvlt_amd as M
    cfg = M.MVLBertConfigForImageCaption(hidden_size=256, num_hidden_layers=1, num_attention_heads=4, intermediate_size=256,
                                         vocab_size=300)
    cfg.swin.update(embed_dim=32, depths=[1, 1, 1, 1], num_heads=[1, 2, 4, 8])
    return M, M.MVLBertForImageCaption(cfg)


def test_sequence_loss_refuses_before_any_launch(cpu_model):
    _, model = cpu_model
    image = torch.zeros(2, 3, 224, 224)
    seq = torch.ones(2, 5, dtype=torch.int64)
    w = torch.ones(2)
    bad = [
        (image, seq.int(), w),                                      # dtype of the sequences
        (image, seq[0], w),                                         # not [B, T]
        (image, torch.ones(3, 5, dtype=torch.int64), torch.ones(3)),          # batch mismatch with the images
        (image, torch.ones(2, 513, dtype=torch.int64), w),          # T > 512
        (image, seq, w.double()),                                   # dtype of the weights
        (image, seq, torch.ones(2, 4)),                             # neither [B] nor [B, T]
        (image, seq, torch.ones(5)),
        (image, seq, torch.ones(2, requires_grad=True)),            # weights with a gradient
    ]
    for im, s, wt in bad:
        with pytest.raises(ValueError):
            model.sequence_loss(im, s, wt)
        with pytest.raises(ValueError):
            model.sequence_loss_from_features(torch.zeros(2, 49, 256), s, wt)
    with pytest.raises(NotImplementedError):
        model.sequence_loss(image, seq, w, learning_strategy="other")


def test_self_critical_loss_refuses_before_any_launch(cpu_model):
    M, model = cpu_model
    image = torch.zeros(2, 3, 224, 224)
    refs = object.__new__(M.ReferenceSet)                  # never read: every refusal below comes first
    with pytest.raises(ValueError, match="metric"):
        M.self_critical_loss(model, image, refs, None, metric="meteor")
    with pytest.raises(ValueError, match="unknown options"):
        M.self_critical_loss(model, image, refs, None, num_beams=3)
    with pytest.raises(NotImplementedError):
        M.self_critical_loss(model, image, refs, None, learning_strategy="normal")
    with pytest.raises(ValueError, match="ReferenceSet"):
        M.self_critical_loss(model, image, [[1, 2, 3]], None)
    with pytest.raises(ValueError, match="index"):
        M.self_critical_loss(model, image, refs, [0, 1, 1])
