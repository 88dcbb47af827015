"""One BertLayer of the MVLBert encoder, forward and backward, on both host paths: bert.py _layer_fwd / _layer_bwd with
ops.NATIVE true (csrc/host.cpp bert_layer_fwd / bert_layer_bwd) and false (the Python launches), called directly on layer 1
of a two-layer encoder, so that a dropout tag taken from the wrong layer shows.

Every run is judged per element against the float64 reference of tests/bert_layer_ref.py (its docstring states the stages
and the bounds): the thirteen saved forward tensors and x2 stage by stage from the operand the kernel read, dx_in and the
twelve parameter gradients twice --
  chained   from dx through float64 values of the eight intermediates nobody returns, each bound carrying its input's bound;
            at most 1 by construction, but behind dqkv that bound exceeds the signal (tests/test_bert_layer_cpu.py measures
            it: three wiring faults pass it in bf16, two in f32);
  cut       every backward stage from the STORED intermediate of a replay: the test launches the eight backward stages one
            by one through mvlt_amd.ops, written here from the definition, on the run's own saved tensors.  The replayed
            dy2, dz2, dh, dx1, dy1, dz1, dctx and dqkv are judged one stage deep themselves, and what the layer returns
            is judged one stage deep from them.  The kernels are deterministic (no float atomics in an encoder layer,
            test_config2_step_is_bit_reproducible_*), so a layer that is wired as the definition says forms the very
            same intermediates; one that is not leaves a sharp bound (signal / bound ~250 in bf16, ~1e4 for the sums).
Before each call NaN blocks of the intermediate sizes go back to the caching allocator; with a device-side row count the rows
of x and dx at or beyond it ARE NaN; every checked output must be finite.  The attention routes a case is about are asserted
first (ops.attn_route), the GEMM route of each product is printed beside the worst ratios.
Between the two host paths of a case everything saved and returned is bit-equal (test_host_paths_agree_bit_for_bit).
test_encoder_is_the_same_on_both_host_paths runs a two-layer H = 128 encoder through the public forward / forward_autopack
and backward on both host paths: the loop, the descriptors, the neighbour-weight prefetch pointers, the deferred LayerNorm
reduce and the embedding ends, which the layer-level calls skip.
No hand-off timeout is touched, no failure path is provoked, nothing runs in a child process.

Measured on an MI355X, worst ratio to the bound over every case and both host paths (test_worst_ratios_summary prints them):
bf16 forward qkv 0.97, ctx 0.45, lse 0.01, y1 0.98, x1 / x2 0.50, mean 0.000, rstd 0.007, h 0.97, act 0.97, y2 0.95; cut
backward dy / dz 0.50, dh 0.97, dx1 0.94, dctx 0.97, dqkv 0.46, dx_in 0.96, the eight weight and bias gradients 0.002 .. 0.034,
the LayerNorm gradients at most 0.006; chained backward fc2.weight 0.18, fc2.bias 0.08, fc1 0.014, ln2 0.006 and everything
behind dx1 (ln1, o, qkv gradients, dx_in) 0.000.  f32: at most 0.11 everywhere except the replayed dh at 0.69.
The pattern is that of the Swin half: a GEMM output judged one stage deep stands at 0.94 .. 0.98 because gemm_ref's bound has no
safety factor and its leading term is the bf16 rounding of the output itself; LayerNorm and attention outputs stand at 0.5
(SAFETY = 2 over the same rounding); sums over rows and chained tensors stand far below.  The one tensor that differs is the
f32 dh: its leading term is not a rounding but ERFC_ABS = 2e-7 against the 1.5e-7 absolute error of the A&S erfc inside
gelu'(h), which the kernel does reach (3/4 of the constant, not a bug: gemm_ref states it).
The file takes 3.3 s alone (29 tests; the first case pays 1.8 s of start-up)."""
import ctypes as C
import math

import pytest
import torch

import attn_ref as A
import bert_layer_ref as H
import misc_ref as Mi
from bert_layer_ref import BF, F32

pytestmark = pytest.mark.gpu

N_IMG = 49
# name -> (H, I, dtype, B, T, seq2seq, (p_h, p_a), rows: dense | packed | autopack, forward route, backward route)
CASES = {
    "base-bidir": (768, 3072, BF, 2, 23, False, (0.1, 0.1), "dense", "BERT_FWD_KT5", "BERT_BWD2_NW5"),
    "base-s2s-step": (768, 3072, BF, 2, 80, True, (0.1, 0.1), "dense", "BERT_FWD_KT9", "BERT_BWD2_NW5"),
    "base-packed": (768, 3072, BF, 3, 80, True, (0.1, 0.1), "packed", "BERT_FWD_KT9", "BERT_BWD2_NW5"),
    "base-autopack": (768, 3072, BF, 3, 80, False, (0.1, 0.1), "autopack", "BERT_FWD_KT9", "BERT_BWD2_NW5"),
    "base-eval": (768, 3072, BF, 2, 23, False, (0.0, 0.0), "dense", "BERT_FWD_KT5", "BERT_BWD2_NW5"),
    "narrow-f32": (128, 512, F32, 3, 23, False, (0.1, 0.1), "dense", "BERT_FWD_KT5", "BERT_BWD_SPLIT_KT5"),
    "narrow-f32-packed": (128, 512, F32, 3, 80, True, (0.1, 0.1), "autopack", "BERT_FWD_KT9", "BERT_BWD_SPLIT_KT9"),
    "base-f32": (768, 3072, F32, 2, 23, True, (0.1, 0.1), "dense", "BERT_FWD_KT5", "BERT_BWD_SPLIT_KT5"),
}
CAPTION_LENS = (80, 13, 0)                  # of the packed cases
LAYER = 1
SEED = 0x5EED1234ABCD

ROWWISE = ("qkv", "ctx", "y1", "mean1", "rstd1", "x1", "h", "act", "y2", "mean2", "rstd2", "x2", "dx_in")
_encoders, _runs = {}, {}


def encoder(Hd, I, dt):
    """A two-layer MVLBert.  One-dimensional parameters away from 0 / 1, qkv weights so that scale q.k has std
    attn_ref.LOGIT_STD on unit-variance rows (peaked softmax rows: one wrong key or row stands out)."""
    if (Hd, I, dt) not in _encoders:
        import mvlt_amd as M
        from mvlt_amd.arena import Arena
        cfg = M.MVLBertPretrainConfig(hidden_size=Hd, num_hidden_layers=2, num_attention_heads=Hd // 64, intermediate_size=I,
                                      vocab_size=3000)
        torch.manual_seed(31)
        m = M.MVLBert(cfg, add_pooling_layer=False)
        g = torch.Generator().manual_seed(32)
        for n, p in m.named_parameters():
            if p.dim() == 1:
                p.data.copy_((1.0 if n.endswith("LayerNorm.weight") else 0.0) + 0.1 * torch.randn(p.shape, generator=g))
        for layer in m.encoder.layer:
            sa = layer.attention.self
            w = torch.randn(3 * Hd, Hd, generator=g) * Hd ** -0.5
            w[:2 * Hd] *= math.sqrt(A.LOGIT_STD)
            for k, lin in enumerate((sa.query, sa.key, sa.value)):
                lin.weight.data.copy_(w[k * Hd:(k + 1) * Hd])
            for lin in (layer.attention.output.dense, layer.intermediate.dense, layer.output.dense):
                lin.weight.data.copy_(torch.randn(lin.weight.shape, generator=g) * lin.weight.shape[1] ** -0.5)
        m = M.set_compute_dtype(m.cuda().train(), dt)
        ar = Arena.of(m, dt)
        ar.refresh_shadow(tail=False)
        _encoders[Hd, I, dt] = (m, ar)
    return _encoders[Hd, I, dt]


def poison(shapes, dt, device):
    ts = [torch.full(s, float("nan"), dtype=dt, device=device) for s in shapes]
    torch.cuda.synchronize()
    del ts


def gemm_route(dt, M_, N, K, b_kmajor, epi, m_dev, dev):
    """The route mvlt_gemm_route answers for a product of this shape and epilogue (nothing launched)."""
    from mvlt_amd import _lib as L, ops
    a = torch.empty((M_, K), dtype=dt, device=dev)
    b = torch.empty((K, N) if b_kmajor else (N, K), dtype=dt, device=dev)
    out = torch.empty((M_, N), dtype=dt, device=dev)
    bias = torch.empty(N, dtype=torch.float32, device=dev)
    q = L.MvltGemm()
    q.dtype, q.M, q.N, q.K = (L.BF16 if dt == BF else L.F32), M_, N, K
    q.A, q.lda, q.B, q.ldb, q.C, q.ldc = a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0), out.data_ptr(), N
    q.b_kmajor, q.epilogue = int(b_kmajor), epi
    if epi & L.EPI_BIAS:
        q.bias = bias.data_ptr()
    if epi & L.EPI_RESIDUAL:
        q.residual, q.ldr = out.data_ptr(), N
    if epi & L.EPI_SAVE_PRE:
        q.pre = out.data_ptr()
    if epi & L.EPI_MUL_GELU_GRAD:
        q.aux = out.data_ptr()
    if epi & L.EPI_DROPOUT:
        q.dropout_p, q.seed, q.tag = 0.1, 1, 1
    if m_dev is not None:
        q.m_dev = m_dev.data_ptr()
    need = L.lib().mvlt_gemm_workspace_bytes(C.byref(q))
    if need:
        ws = ops.workspace("gemm", need, dev)
        q.workspace, q.workspace_bytes = ws.data_ptr(), ws.numel()
    return "%s/%d" % L.gemm_route_name(L.lib().mvlt_gemm_route(C.byref(q)))


def inputs_of(name):
    """Everything the two host paths of a case share: (case dict for the reference, device operands)."""
    from mvlt_amd import ops
    Hd, I, dt, B, T, s2s, (p_h, p_a), rowmode, _, _ = CASES[name]
    L = N_IMG + 2 + T
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(500 + sum(map(ord, name)))
    ids = torch.randint(1, 3000, (B, T), generator=g)
    image_mask = None
    lens = None
    if rowmode != "dense":
        for b, n in enumerate(CAPTION_LENS):
            ids[b, n:] = 0
        if not s2s:
            ids[0, 5] = 0                                   # a masked key inside a kept caption
        lens = [N_IMG + 2 + n for n in CAPTION_LENS]
    elif not s2s:
        ids[1, 9:] = 0                                      # padding
        image_mask = torch.ones(B, N_IMG, dtype=torch.uint8)
        image_mask[0, 3] = image_mask[1, 0] = image_mask[1, 17] = image_mask[B - 1, 48] = 0
    ids_d = ids.cuda()
    pack = rd = None
    rows = B * L
    if rowmode == "packed":                                 # the layout MVLBert.forward_packed builds
        sl = torch.tensor(lens, dtype=torch.int32)
        st = torch.cumsum(sl, 0, dtype=torch.int32) - sl
        rows = int(sl.sum())
        pack = (st.cuda(), sl.cuda(), rows, st.to(torch.int64).cuda())
    elif rowmode == "autopack":                             # ... and MVLBert.forward_autopack: the plan and the row count on the device
        rs, sl, tot, rs64, _ = ops.pack_plan(ids_d, None, N_IMG)
        pack = (rs, sl, rows, rs64, tot)
        rd = tot
        assert sl.tolist() == lens and int(tot) == sum(lens), "mvlt_pack_plan keeps a caption up to its last non-zero id"
    rv = rows if lens is None else sum(lens)
    x = torch.randn(rows, Hd, generator=g).to(dt).to(dev)
    dx = torch.randn(rows, Hd, generator=g).to(dt).to(dev)
    x[rv:] = float("nan")
    dx[rv:] = float("nan")
    case = dict(H=Hd, nH=Hd // 64, I=I, B=B, T=T, n_img=N_IMG, dtype=dt, s2s=s2s, p_h=p_h, p_a=p_a, seed=SEED, layer=LAYER,
                eps=1e-12, ids=None if s2s else ids, image_mask=image_mask, lens=lens)
    return case, dict(x=x, dx=dx, ids=ids_d, image_mask=None if image_mask is None else image_mask.cuda(), pack=pack, rd=rd,
                      rows=rows, rv=rv, L=L)


def replay_backward(m, ar, case, io, sv):
    """The eight backward stages of the layer, launched one by one from the definition on the saved tensors sv (a dict):
    -> {name: stored intermediate}.  Parameter gradients go to scratch buffers."""
    from mvlt_amd import _lib as L, ops
    layer = m.encoder.layer[LAYER]
    so, lo, li = layer.attention.output, layer.output, layer.intermediate
    Hd, nH, p_h, p_a, rd = case["H"], case["nH"], case["p_h"], case["p_a"], io["rd"]
    dev = io["x"].device
    tmp = lambda: torch.empty(Hd, dtype=torch.float32, device=dev)                     # noqa: E731
    out = {}

    def ln_bwd(dy, y, mean, rstd, gamma, tag):
        kw = dict(branch=dict(dropout=(p_h, SEED, tag))) if p_h > 0 else {}
        r = ops.layernorm_bwd(dy, y, mean.contiguous(), rstd.contiguous(), gamma, tmp(), tmp(), rows_dev=rd, **kw)
        return r if p_h > 0 else (r, r)

    out["dy2"], out["dz2"] = ln_bwd(io["dx"], sv["y2"], sv["mean2"], sv["rstd2"], lo.LayerNorm.weight.data, 8 * LAYER + 2)
    out["dh"] = ops.gemm(out["dz2"], ar.compute(lo.dense.weight), b_kmajor=True, mul_gelu_grad=sv["h"], m_dev=rd)
    out["dx1"] = ops.gemm(out["dh"], ar.compute(li.dense.weight), b_kmajor=True, residual=out["dy2"], m_dev=rd)
    out["dy1"], out["dz1"] = ln_bwd(out["dx1"], sv["y1"], sv["mean1"], sv["rstd1"], so.LayerNorm.weight.data, 8 * LAYER + 1)
    out["dctx"] = ops.gemm(out["dz1"], ar.compute(so.dense.weight), b_kmajor=True, m_dev=rd)
    out["dqkv"] = ops.attn_bwd(out["dctx"], sv["qkv"], sv["ctx"], sv["lse"], L.ATTN_SEQ2SEQ if case["s2s"] else L.ATTN_BIDIR,
                               case["B"], io["L"], nH, 64, 64 ** -0.5, dropout=(p_a, SEED, 8 * LAYER + 0), text_ids=io["ids"],
                               image_mask=io["image_mask"], obj_end=N_IMG + 1, pack=io["pack"])
    return out


def run_case(name, native):
    from mvlt_amd import _lib as L, ops
    Hd, I, dt, B, T, s2s, (p_h, p_a), rowmode, want_fwd, want_bwd = CASES[name]
    case, io = inputs_of(name)
    m, ar = encoder(Hd, I, dt)
    layer = m.encoder.layer[LAYER]
    sa, so, li, lo = layer.attention.self, layer.attention.output, layer.intermediate, layer.output
    assert so.LayerNorm.eps == 1e-12 and lo.LayerNorm.eps == 1e-12
    dev, rows, nH, Lq = io["x"].device, io["rows"], Hd // 64, io["L"]
    mode = L.ATTN_SEQ2SEQ if s2s else L.ATTN_BIDIR
    akw = dict(text_ids=io["ids"], image_mask=io["image_mask"], obj_end=N_IMG + 1, pack=io["pack"])
    # ---- the routes this case is about
    probe = torch.empty((rows, 3 * Hd), dtype=dt, device=dev)
    for bwd, want in ((False, want_fwd), (True, want_bwd)):
        route = ops.attn_route(probe, mode, B, Lq, nH, 64, 64 ** -0.5, bwd=bwd, dropout=(p_a, SEED, 8 * LAYER), **akw)
        assert route == want, (name, "attention backward" if bwd else "attention forward", route)
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(ops, "NATIVE", native)
        c = m._layer_ctx(mode, B, Lq, io["ids"], T, io["image_mask"], N_IMG + 1, io["pack"], SEED, p_h, p_a, native)
        poison([(rows, 3 * Hd), (rows, Hd), (rows, Hd), (rows, I), (rows, I), (rows, Hd), (rows, Hd)], dt, dev)
        x2, saved = m._layer_fwd(ar, LAYER, io["x"], c, True)
        ar.begin_backward()
        c["lnq"] = lnq = ops.LnReduceQueue()
        if native:
            c["side"] = ops.side_int(dev)
        poison([(rows, Hd), (rows, Hd), (rows, I), (rows, Hd), (rows, Hd), (rows, Hd), (rows, Hd), (rows, 3 * Hd)], dt, dev)
        dx_in = m._layer_bwd(ar, LAYER, saved, io["dx"], c)
        if native:
            ops.host().lnq_flush(ops.stream_int())
        else:
            lnq.flush()
        ops.join_side(dev)
        torch.cuda.synchronize()
        if native:
            ops.host().side_release()
    # ---- the two layouts of the saved tensors (bert.py _layer_fwd), normalised
    if native:
        assert len(saved) == 11
        sx, qkv, ctx, lse, y1, st1, x1, h, act, y2, st2 = saved
        assert st1.shape == (2, rows) and st2.shape == (2, rows)
        mean1, rstd1, mean2, rstd2 = st1[0], st1[1], st2[0], st2[1]
    else:
        assert len(saved) == 13
        sx, qkv, ctx, lse, y1, mean1, rstd1, x1, h, act, y2, mean2, rstd2 = saved
    assert sx.data_ptr() == io["x"].data_ptr()
    run = dict(x=io["x"], dx=io["dx"], qkv=qkv, ctx=ctx, lse=lse, y1=y1, mean1=mean1, rstd1=rstd1, x1=x1, h=h, act=act, y2=y2,
               mean2=mean2, rstd2=rstd2, x2=x2, dx_in=dx_in,
               wq=ar.compute(sa.query.weight), wk=ar.compute(sa.key.weight), wv=ar.compute(sa.value.weight),
               bq=sa.query.bias.data, bk=sa.key.bias.data, bv=sa.value.bias.data,
               wo=ar.compute(so.dense.weight), bo=so.dense.bias.data, g1=so.LayerNorm.weight.data, b1=so.LayerNorm.bias.data,
               wi=ar.compute(li.dense.weight), bi=li.dense.bias.data, wo2=ar.compute(lo.dense.weight), bo2=lo.dense.bias.data,
               g2=lo.LayerNorm.weight.data, b2=lo.LayerNorm.bias.data)
    for k, p in (("query.weight", sa.query.weight), ("key.weight", sa.key.weight), ("value.weight", sa.value.weight),
                 ("query.bias", sa.query.bias), ("key.bias", sa.key.bias), ("value.bias", sa.value.bias),
                 ("o.weight", so.dense.weight), ("o.bias", so.dense.bias), ("ln1.weight", so.LayerNorm.weight),
                 ("ln1.bias", so.LayerNorm.bias), ("fc1.weight", li.dense.weight), ("fc1.bias", li.dense.bias),
                 ("fc2.weight", lo.dense.weight), ("fc2.bias", lo.dense.bias), ("ln2.weight", lo.LayerNorm.weight),
                 ("ln2.bias", lo.LayerNorm.bias)):
        run[k] = ar.grad_view(p).view(p.shape)
    run = {k: v.detach().clone() for k, v in run.items()}
    rv = io["rv"]
    for k, v in run.items():
        if k not in ("x", "dx", "lse"):                     # (lse: the queries a packed sample does not have are never written)
            assert bool(torch.isfinite(v[:rv] if k in ROWWISE else v).all()), (name, native, k, "not finite")
    replay = replay_backward(m, ar, case, io, run)
    torch.cuda.synchronize()
    # ---- the GEMM route of each product (the dispatch in its no-launch mode; printed once per case, beside the native run)
    routes = {}
    if native:
        drop = L.EPI_DROPOUT if p_h else 0
        products = {"qkv": (3 * Hd, Hd, False, L.EPI_BIAS), "y1": (Hd, Hd, False, L.EPI_BIAS | L.EPI_RESIDUAL | drop),
                    "act": (I, Hd, False, L.EPI_BIAS | L.EPI_GELU | L.EPI_SAVE_PRE),
                    "y2": (Hd, I, False, L.EPI_BIAS | L.EPI_RESIDUAL | drop), "dh": (I, Hd, True, L.EPI_MUL_GELU_GRAD),
                    "dx1": (Hd, I, True, L.EPI_RESIDUAL), "dctx": (Hd, Hd, True, 0), "dx_in": (Hd, 3 * Hd, True, L.EPI_RESIDUAL)}
        for k, (N, K, bk, epi) in products.items():
            routes[k] = gemm_route(dt, rows, N, K, bk, epi, io["rd"], dev)
    return case, run, replay, routes


def judged(name, native):
    """(case, run, chained reference, cut reference) of one host path of a case, run and judged once per session."""
    key = (name, native)
    if key not in _runs:
        case, run, replay, routes = run_case(name, native)
        chained = H.reference(run, case)
        cut = H.reference(dict(run, **replay), case)
        label = "%s-%s" % (name, "native" if native else "python")
        for mode, ref in (("chained", chained), ("cut", cut)):
            for k, v in H.worst_ratios(ref).items():
                if mode == "chained" or k in H.BACKWARD + H.STAGES:
                    shown = k in routes and (k in H.STAGES) == (mode == "cut")
                    print(f"{label:32s} {mode:7s} {k:11s} worst ratio to the bound {v:.3f}"
                          + (f"   GEMM route {routes[k]}" if shown else ""))
        bad = dict(H.failures(chained, label + " chained"))
        back = {k: v for k, v in cut.items() if k not in H.FORWARD}
        bad.update({"cut " + k: v for k, v in H.failures(back, label + " cut").items()})
        _runs[key] = (case, run, bad, H.worst_ratios(chained), H.worst_ratios(cut))
    return _runs[key]


@pytest.mark.parametrize("native", [True, False], ids=["native", "python"])
@pytest.mark.parametrize("name", list(CASES))
def test_layer_against_float64(name, native):
    case, run, bad, _, _ = judged(name, native)
    assert not bad, "\n".join(bad.values())
    if case["p_h"] == 0:
        assert case["p_a"] == 0           # eval: no branch output -- the reference asserts dz is dy by identity


@pytest.mark.parametrize("name", list(CASES))
def test_host_paths_agree_bit_for_bit(name):
    """The two host paths launch the same kernels on the same operands, and no encoder-layer gradient is accumulated with float
    atomics: whatever they save or return is bit-equal, over the rows that are computed."""
    (case, a, _, _, _), (_, b, _, _, _) = judged(name, True), judged(name, False)
    _, _, rv = H.layout(case)
    for k in ("x", "dx") + H.PARAMS:
        n = rv if k in ("x", "dx") else None                # (NaN beyond the row count)
        Mi.check_equal(a[k][:n], b[k][:n], f"{name}: the runs share {k}")
    for k in ROWWISE:
        Mi.check_equal(a[k][:rv], b[k][:rv], f"{name}: native against python: {k}")
    B, nH, L = a["lse"].shape
    valid = torch.ones(B, L, dtype=torch.bool) if case["lens"] is None else \
        torch.arange(L)[None, :] < torch.tensor(case["lens"])[:, None]
    valid = valid.reshape(B * L, 1).expand(B * L, nH).to(a["lse"].device)
    Mi.check_equal(H.lse_rows(a["lse"], valid), H.lse_rows(b["lse"], valid), f"{name}: native against python: lse")
    for k in H.QKV_GRADS + H.GRADS[2:]:
        Mi.check_equal(a[k], b[k], f"{name}: native against python: {k}")


def test_worst_ratios_summary():
    """Prints the worst ratio per tensor and dtype over every case judged so far (the figures of the module docstring)."""
    worst = {}
    for (name, native), (case, _, _, ch, cut) in _runs.items():
        for mode, ratios in (("chained", ch), ("cut", cut)):
            for k, v in ratios.items():
                key = (str(case["dtype"])[6:], mode, k)
                worst[key] = max(worst.get(key, 0.0), v)
    for (dt, mode, k), v in sorted(worst.items()):
        print(f"summary {dt:8s} {mode:7s} {k:11s} {v:.3f}")
        assert v <= 1.0


# ------------------------------------------------------------------ the encoder loop, both host paths
@pytest.mark.parametrize("entry", ["forward", "autopack"])
@pytest.mark.parametrize("dt", [BF, F32], ids=["bf16", "f32"])
def test_encoder_is_the_same_on_both_host_paths(dt, entry):
    """A two-layer H = 128 MVLBert in train mode through the public forward / forward_autopack and backward with ops.NATIVE
    true and false: hidden, dimg and every gradient are bit-equal, except word_embeddings.weight, whose rows are accumulated
    with float atomics (held to 1e-6 of its norm, as test_config2_step_is_bit_reproducible_* holds it)."""
    import mvlt_amd as M
    from mvlt_amd import ops
    cfg = M.MVLBertPretrainConfig(hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=512, vocab_size=3000)
    torch.manual_seed(41)
    m = M.set_compute_dtype(M.MVLBert(cfg, add_pooling_layer=True).cuda().train(), dt)
    g = torch.Generator().manual_seed(42)
    B, T = 3, 23
    ids = torch.randint(1, 3000, (B, T), generator=g)
    ids[1, 9:] = 0
    ids[2, :] = 0
    ids = ids.cuda()
    feat0 = torch.randn(B, N_IMG, 128, generator=g).cuda()
    runs = []
    for native in (True, False):
        with pytest.MonkeyPatch.context() as mp:
            mp.setattr(ops, "NATIVE", native)
            M.manual_seed(1234)
            feat = feat0.clone().requires_grad_(True)
            if entry == "forward":
                out, pooled = m(ids, ids > 0, feat, None, seq2seq_mask=False)
                hidden = out[0]
            else:
                hidden, pooled, _ = m.forward_autopack(ids, feat, seq2seq_mask=True)
            w = torch.randn(hidden.shape, generator=torch.Generator().manual_seed(43)).to(hidden.dtype).cuda()
            if entry == "autopack":
                rows = int((ids != 0).sum()) + B * (N_IMG + 2)          # captions without interior zeros: the packed total
                loss = (hidden[:rows].float() * w[:rows].float()).sum() + pooled.float().sum()
                hidden = hidden[:rows]
            else:
                loss = (hidden.float() * w.float()).sum() + pooled.float().sum()
            loss.backward()
            torch.cuda.synchronize()
            grads = {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None}
            runs.append((hidden.detach().clone(), pooled.detach().clone(), feat.grad.detach().clone(), grads))
            for p in m.parameters():
                p.grad = None
    (h0, p0, d0, g0), (h1, p1, d1, g1) = runs
    Mi.check_equal(h0.reshape(-1, 128), h1.reshape(-1, 128), "hidden")
    Mi.check_equal(p0, p1, "pooled")
    Mi.check_equal(d0.reshape(-1, 128), d1.reshape(-1, 128), "dimg")
    assert g0.keys() == g1.keys() and len(g0) > 30
    for k in g0:
        assert bool(torch.isfinite(g0[k]).all()), k
        if k == "word_embeddings.weight":
            assert float((g0[k].double() - g1[k].double()).norm()) <= 1e-6 * float(g0[k].double().norm()), k
        else:
            Mi.check_equal(g0[k], g1[k], k)
