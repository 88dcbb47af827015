"""Attention maps on the GPU.

Kernel level: mvlt_attn_probs (csrc/attnmap.hip) through ops.attn_probs against the float64 reference and PER-ELEMENT bound of
tests/attn_maps_ref.py (proven on the host in tests/test_attn_maps_cpu.py), bf16 and f32, every flag combination, on dense
and packed rows, at ranges that start off a tile boundary and at both ends of the forward's L range.  Every layout runs with
the float64 lse rounded to f32 (the new kernel alone) and with the lse ops.attn_fwd wrote for the same operands (what the
model does).  Outputs start filled with NaN; packed layouts leave NaN rows between the sequences and NaN in the lse of the
queries a sequence does not have, so one stray read poisons the output.

Model level: MVLBert.attention_maps through the three task models (tiny models, hash weights) against the probabilities the
oracle hands its attention dropout (a recording Dropper), with the answer of attention_maps bit-identical to forward's.
Tolerances there are the activation tolerances of tests/test_model_gpu.py (ACT)."""
import ctypes

import pytest
import torch

from attn_ref import U32, AttnRef, bert_bias, check_lse
from attn_maps_ref import FLAGS, MapsRef, check_maps, maps_case, recording_dropper, worst_ratio
from conftest import hash_sd, rel_err, synth_batch

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
NAN = float("nan")
ACT = {F32: 2e-4, BF: 6e-2}          # tests/test_model_gpu.py: relative Frobenius error of activations after such a pass


@pytest.fixture(scope="module")
def ops():
    from mvlt_amd import ops as o
    return o


# ------------------------------------------------------------------ kernel level
def _sel(c, q, k):
    n_img, T, L = c["n_img"], c["T"], c["L"]
    r = {"cls": (0, 1), "image": (1, n_img), "text": (n_img + 2, T), "all": (0, L)}
    return r[q], r[k]


LAYOUTS = {
    # dense BIDIR, L = 74 (no multiple of 16 or 32), captions 23 / 9 / 1, image_mask zeros on sequence 1
    "A": (dict(s2s=False), [("cls", "image"), ("text", "image"), ("all", "all")]),
    # dense SEQ2SEQ, same L
    "B": (dict(s2s=True), [("text", "all")]),
    # packed pack_layout([74, 53, 60], 74, gap=3), both modes
    "C-bidir": (dict(s2s=False, lens=(23, 2, 9), packed=True), [("all", "all")]),
    "C-s2s": (dict(s2s=True, lens=(23, 2, 9), packed=True), [("all", "all")]),
    # the ends of the forward's L range
    "D-L52": (dict(s2s=False, T=1, lens=(1, 0)), [("cls", "all"), ("all", "image")]),
    "D-L208": (dict(s2s=False, n_img=98, T=108, lens=(108, 31)), [("cls", "all"), ("all", "image")]),
}


@pytest.fixture(scope="module")
def layout():
    made = {}

    def get(name, dt):
        if (name, dt) not in made:
            made[(name, dt)] = maps_case(dtype=dt, seed=600 + len(made), **LAYOUTS[name][0])
        return made[(name, dt)]
    return get


def _device_args(c):
    from mvlt_amd._lib import ATTN_BIDIR, ATTN_SEQ2SEQ
    kw = dict(text_ids=c["ids"].cuda(), obj_end=c["n_img"] + 1)
    if c["im"] is not None:
        kw["image_mask"] = c["im"].cuda()
    if c["pack"] is not None:
        kw["pack"] = (c["pack"][0].cuda(), c["pack"][1].cuda(), c["pack"][2])
    g = c["kw"]
    return (ATTN_SEQ2SEQ if c["s2s"] else ATTN_BIDIR, g["nseq"], g["L"], g["nH"], g["hd"], g["scale"]), kw


@pytest.mark.parametrize("lse_from", ["reference", "attn_fwd"])
@pytest.mark.parametrize("dt", [BF, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("name", list(LAYOUTS))
def test_attn_probs_kernel(ops, layout, name, dt, lse_from):
    c = layout(name, dt)
    ref, g = c["ref"], c["kw"]
    nseq, L, nH = g["nseq"], g["L"], g["nH"]
    args, kw = _device_args(c)
    qkv = c["qkv"].cuda()
    if lse_from == "reference":
        lse = ref.lse.float().cuda()                                  # NaN at the queries a packed sequence does not have
        lse_err = U32 * ref.lse.abs()
    else:
        if ops.attn_route(qkv, *args, **kw) == "UNSUPPORTED":
            # f32 at 13 key tiles: the forward itself refuses (Q, K, V of a head exceed the LDS; tests/test_attn_routes_gpu.py
            # pins that), so no model can hand this kernel such an lse -- only the reference lse exists for this layout
            assert (name, dt) == ("D-L208", F32)
            with pytest.raises(RuntimeError, match="MVLT_ERR_UNSUPPORTED"):
                ops.attn_fwd(qkv, *args, **kw)
            return
        lse = torch.full((nseq, nH, L), NAN, dtype=torch.float32, device="cuda")
        ops.attn_fwd(qkv, *args, lse=lse, **kw)
        check_lse(lse, ref)
        lse_err = ref.lse_b
    pk = None if c["pack"] is None else (c["pack"][3], c["pack"][1])
    maps = MapsRef(ref, c["qkv"], lse.cpu(), lse_err, pack=pk, **g)
    valid = torch.isfinite(ref.lse)                                   # [nseq, nH, L]
    for qn, kn in LAYOUTS[name][1]:
        qr, kr = _sel(c, qn, kn)
        for hm, rn in FLAGS:
            want, bound = maps.select(qr, kr, hm, rn)
            out = torch.full(tuple(want.shape), NAN, dtype=torch.float32, device="cuda")
            got = ops.attn_probs(qkv, lse, *args, qr, kr, head_mean=hm, renorm=rn, out=out, **kw)
            assert got is out
            torch.cuda.synchronize()
            what = f"{name} {qn}->{kn} mean={hm} renorm={rn} lse from {lse_from}"
            print(f"{what}: worst |error| / bound = {worst_ratio(out, want, bound):.3f}")
            check_maps(out, want, bound, what)
            o = out.cpu()
            assert bool(torch.isfinite(o).all()), what
            qv = valid[:, :, qr[0]:qr[0] + qr[1]]
            if not bool(qv.all()):                                    # rows >= seq_len: all zero
                dead = ~(qv.all(1, keepdim=True) if hm else qv)
                assert bool((o[dead.expand(o.shape[:3])] == 0).all()), what
            if kn == "all" and not rn:                                # un-renormalised rows over all keys sum to 1
                live = qv.all(1, keepdim=True) if hm else qv
                dev = (o.double().sum(-1) - 1).abs()
                assert bool((dev <= bound.sum(-1))[live].all()), (what, float((dev / bound.sum(-1))[live].max()))
            if c["s2s"]:                                              # every entry above the causal rule is exactly 0
                ar = torch.arange(L)
                allowed = (ar[None, :] <= ar[:, None]) | (ar[None, :] <= c["n_img"] + 1)
                above = ~allowed[qr[0]:qr[0] + qr[1], kr[0]:kr[0] + kr[1]]
                assert bool((o[:, :, above] == 0).all()), what
            if rn:                                                    # renormalised rows sum to 1 (or stay 0)
                s = o.double().sum(-1)
                assert bool(((s - 1).abs() < 1e-5)[want.sum(-1) > 0].all()) and bool((s[want.sum(-1) == 0] == 0).all()), what


def test_attn_probs_allocates_its_output(ops, layout):
    c = layout("A", BF)
    args, kw = _device_args(c)
    qkv, lse = c["qkv"].cuda(), c["ref"].lse.float().cuda()
    a = ops.attn_probs(qkv, lse, *args, (0, 1), (1, 49), **kw)
    b = ops.attn_probs(qkv, lse, *args, (0, 1), (1, 49), head_mean=True, **kw)
    assert a.shape == (3, 2, 1, 49) and b.shape == (3, 1, 1, 49) and a.dtype == b.dtype == torch.float32
    full = ops.attn_probs(qkv, lse, *args, (0, 74), (0, 74), **kw)
    assert torch.equal(full[:, :, 0:1, 1:50], a)                     # a selection is a slice of the full map, bit for bit


def test_attn_probs_refusals_launch_nothing(ops, layout):
    """Every refusal of the header raises and leaves the output buffer as it was."""
    from mvlt_amd import _lib
    c = layout("A", BF)
    args, kw = _device_args(c)
    qkv, lse = c["qkv"].cuda(), c["ref"].lse.float().cuda()
    out = torch.full((3, 2, 74, 74), NAN, dtype=torch.float32, device="cuda")
    f = _lib.lib().mvlt_attn_probs
    stream = ops._stream()

    def desc(**over):
        p = ops._attn_struct(qkv, None, lse, *args, **kw)
        for k, v in over.items():
            setattr(p, k, v)
        return p
    call = lambda p, q0, nq, k0, nk, flags, o: f(ctypes.byref(p), q0, nq, k0, nk, flags, o, stream)  # noqa: E731
    o = ctypes.c_void_p(out.data_ptr())
    ARG, UNS = -1, -3
    assert call(desc(mode=_lib.ATTN_SWIN), 0, 1, 1, 49, 0, o) == UNS
    assert call(desc(hd=32), 0, 1, 1, 49, 0, o) == UNS
    for q0, nq, k0, nk in [(0, 0, 1, 49), (0, -1, 1, 49), (0, 1, 1, 0), (-1, 2, 1, 49), (74, 1, 1, 49), (0, 75, 1, 49),
                           (0, 1, 26, 49), (0, 1, 0, 75)]:
        assert call(desc(), q0, nq, k0, nk, 0, o) == ARG, (q0, nq, k0, nk)
    assert call(desc(lse=None), 0, 1, 1, 49, 0, o) == ARG
    assert call(desc(), 0, 1, 1, 49, 0, None) == ARG
    for flags in (4, 7, -1):
        assert call(desc(), 0, 1, 1, 49, flags, o) == ARG
    with pytest.raises(RuntimeError, match="MVLT_ERR_ARG"):
        ops.attn_probs(qkv, lse, *args, (71, 4), (0, 74), out=torch.empty(3, 2, 4, 74, device="cuda"), **kw)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()), "a refused call wrote to its output"


# ------------------------------------------------------------------ model level
def _oracle_cfgs():
    from oracle import mvlt_oracle as O
    scfg = O.SwinCfg(embed_dim=32, depths=(2, 2, 2, 2), num_heads=(1, 2, 4, 8), drop_path_rate=0.2)
    bcfg = O.BertCfg(vocab_size=3000, hidden_size=256, num_hidden_layers=2, num_attention_heads=4, intermediate_size=1024)
    return O, scfg, bcfg


def _probs(rec, n_layers):
    return torch.stack([rec.probs[f"MVLBert.encoder.layer.{i}.attn_drop"] for i in range(n_layers)])


@pytest.fixture(scope="module")
def M():
    import mvlt_amd
    return mvlt_amd


@pytest.fixture(scope="module")
def vqa(M, specs_hash):
    """The tiny VQA model (hash weights for the tower and the encoder, a seeded head), its inputs (B = 2, T = 9, padded tails)
    and the oracle's answer and per-layer probabilities [2 layers, B, 4 heads, 60, 60]: computed once."""
    O, scfg, bcfg = _oracle_cfgs()
    cfg = M.MVLBertConfigforVQA(hidden_size=256, num_hidden_layers=2, num_attention_heads=4, intermediate_size=1024,
                                vocab_size=3000)
    cfg.swin.update(embed_dim=32, depths=[2, 2, 2, 2], num_heads=[1, 2, 4, 8], drop_path_rate=0.2)
    cfg.result_num = 37
    model = M.MVLBertForVQA(cfg)
    _, unexpected = model.load_state_dict(hash_sd(specs_hash["hash_tiny_pretrain"]), strict=False)
    assert all(k.startswith(("MLM_head", "ITM_mlp")) for k in unexpected), unexpected
    g = torch.Generator().manual_seed(12)
    with torch.no_grad():
        model.final_mlp[1].weight.copy_(0.05 * torch.randn(model.final_mlp[1].weight.shape, generator=g))
        model.final_mlp[1].bias.copy_(0.05 * torch.randn(model.final_mlp[1].bias.shape, generator=g))
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    image, ids, _, _ = synth_batch(2, 9, seed=71, vocab=3000)
    assert bool((ids[:, -1] == 0).all())                                      # padded tails: masked keys exist
    rec = recording_dropper()
    with torch.no_grad():
        rprob, rlogits = O.vqa_forward(sd, scfg, bcfg, image, ids, drop=rec)
    keymask = O.bidir_bool_mask(ids, 2, 49)                                   # [B, L]
    return dict(cfg=cfg, sd=sd, image=image, ids=ids, probs=_probs(rec, 2), rprob=rprob, rlogits=rlogits, keymask=keymask)


def _vqa_model(M, vqa, cd):
    model = M.MVLBertForVQA(vqa["cfg"])
    model.load_state_dict(vqa["sd"])
    return M.set_compute_dtype(model.cuda().eval(), cd)


@pytest.mark.parametrize("native", [True, False], ids=["native", "python"])
@pytest.mark.parametrize("cd", [F32, BF], ids=["f32", "bf16"])
def test_vqa_attention_maps_vs_oracle(M, ops, vqa, cd, native, monkeypatch):
    monkeypatch.setattr(ops, "NATIVE", native)
    model = _vqa_model(M, vqa, cd)
    image, ids = vqa["image"].cuda(), vqa["ids"].cuda()
    with torch.no_grad():
        prob0, logits0 = model(image, ids, None)
    prob, logits, maps = model.attention_maps(image, ids, queries='all', keys='all', head_mean=False)
    prob1, logits1 = model(image, ids, None)                                  # ... and with autograd on
    assert torch.equal(prob, prob0) and torch.equal(logits, logits0)          # the same launches: bit-identical
    assert torch.equal(prob, prob1.detach()) and torch.equal(logits, logits1.detach())
    assert rel_err(logits.float().cpu(), vqa["rlogits"]) < ACT[cd]
    assert maps.shape == (2, 2, 4, 60, 60) and maps.dtype == torch.float32
    m = maps.cpu()
    for layer in range(2):
        e = rel_err(m[layer], vqa["probs"][layer])
        print(f"VQA {cd} native={native} layer {layer}: rel_err of the maps vs the oracle = {e:.3e}")
        assert e < ACT[cd], (layer, e)
    masked = ~vqa["keymask"][None, :, None, None, :].expand_as(m)
    assert bool(masked.any()) and bool((m[masked] == 0).all())                # masked entries are exactly 0
    assert float((m.double().sum(-1) - 1).abs().max()) < 1e-4


@pytest.mark.parametrize("cd", [F32, BF], ids=["f32", "bf16"])
def test_caption_attention_maps_vs_oracle(M, specs_hash, cd):
    from tiny_caption import tiny_caption
    O, scfg, bcfg = _oracle_cfgs()
    model, sd = tiny_caption(M, specs_hash, cd)
    image, ids, _, _ = synth_batch(2, 9, seed=72, vocab=3000)
    assert bool((ids[:, -1] == 0).all())
    rec = recording_dropper()
    with torch.no_grad():
        O.mvlbert_forward(sd, bcfg, ids, O.conv_layer(image, sd, scfg), True, drop=rec)
    probs = _probs(rec, 2)                                                    # [2, B, 4, 60, 60]
    maps = model.attention_maps(image.cuda(), ids.cuda())                     # default: text -> image, head mean
    assert maps.shape == (2, 2, 1, 9, 49)
    want = probs[:, :, :, 51:60, 1:50].mean(2, keepdim=True)
    e = rel_err(maps.cpu(), want)
    print(f"caption {cd}: rel_err of text -> image (head mean) vs the oracle = {e:.3e}")
    assert e < ACT[cd]
    assert M.image_heatmap(maps).shape == (2, 2, 1, 9, 1, 7, 7)
    # text -> all: the causal rule of the seq2seq mask, exactly
    full = model.attention_maps(image.cuda(), ids.cuda(), keys='all', head_mean=False).cpu()
    assert rel_err(full, probs[:, :, :, 51:60]) < ACT[cd]
    above = ~O.seq2seq_bool_mask(60, 50)[51:60]
    assert bool(above.any()) and bool((full[..., above] == 0).all())
    with pytest.raises(NotImplementedError):
        model.attention_maps(image.cuda(), ids.cuda(), learning_strategy='other')


def test_retrieval_attention_maps_answer_is_forwards(M, specs_hash):
    cfg = M.MVLBertRetrieval(hidden_size=256, num_hidden_layers=2, num_attention_heads=4, intermediate_size=1024, vocab_size=3000)
    cfg.swin.update(embed_dim=32, depths=[2, 2, 2, 2], num_heads=[1, 2, 4, 8], drop_path_rate=0.2)
    model = M.MVLBertForRetrieval(cfg)
    model.load_state_dict(hash_sd(specs_hash["hash_tiny_pretrain"]), strict=False)
    model = M.set_compute_dtype(model.cuda().eval(), BF)
    image, ids, _, _ = synth_batch(2, 9, seed=73, vocab=3000)
    with torch.no_grad():
        prob0 = model(image.cuda(), ids.cuda())
    prob, maps = model.attention_maps(image.cuda(), ids.cuda(), renorm=True)
    assert torch.equal(prob, prob0)
    assert maps.shape == (2, 2, 1, 1, 49) and float((maps.double().sum(-1) - 1).abs().max()) < 1e-5
    pair = torch.stack([image, image.flip(0)], 1).cuda()                       # two views: n_img = 98
    prob2, maps2 = model.attention_maps(pair, ids.cuda(), layers=[-1])
    assert maps2.shape == (1, 2, 1, 1, 98) and M.image_heatmap(maps2, views=2).shape == (1, 2, 1, 1, 2, 7, 7)
    with torch.no_grad():
        assert torch.equal(prob2, model(pair, ids.cuda()))


def test_selections_are_slices_and_the_head_mean_is_the_mean(M, ops, vqa, monkeypatch):
    """[CLS] -> image is the corresponding slice of all -> all within the kernel-level bound, taken from the very qkv / lse the
    model handed the kernel (recorded at ops.attn_probs); head_mean is the mean of the per-head maps within nH 2^-24 relative."""
    model = _vqa_model(M, vqa, BF)
    image, ids = vqa["image"].cuda(), vqa["ids"].cuda()
    seen = []
    real = ops.attn_probs

    def spy(qkv, lse, *a, **k):
        seen.append((qkv.clone(), lse.clone()))
        return real(qkv, lse, *a, **k)
    monkeypatch.setattr(ops, "attn_probs", spy)
    _, _, full = model.attention_maps(image, ids, queries='all', keys='all', head_mean=False)
    monkeypatch.setattr(ops, "attn_probs", real)
    _, _, cls = model.attention_maps(image, ids, head_mean=False)
    _, _, mean = model.attention_maps(image, ids)
    assert len(seen) == 2 and cls.shape == (2, 2, 4, 1, 49) and mean.shape == (2, 2, 1, 1, 49)
    B, L, nH, hd = 2, 60, 4, 64
    bias = bert_bias(False, B, L, 49, vqa["ids"], None)
    for layer, (qkv, lse) in enumerate(seen):
        ref = AttnRef(qkv.cpu(), None, nseq=B, L=L, nH=nH, hd=hd, scale=0.125, bias=bias, dtype=BF)
        check_lse(lse, ref)
        mr = MapsRef(ref, qkv.cpu(), lse.cpu(), ref.lse_b, nseq=B, L=L, nH=nH, hd=hd, scale=0.125)
        want, bound = mr.select((0, L), (0, L))
        check_maps(full[layer], want, bound, f"layer {layer} all -> all")
        want, bound = mr.select((0, 1), (1, 49))
        check_maps(cls[layer], want, bound, f"layer {layer} cls -> image")
        # both are within `bound` of one reference, so they are within twice the bound of each other
        d = (cls[layer].double() - full[layer][:, :, 0:1, 1:50].double()).abs().cpu()
        assert bool((d <= 2 * bound).all())
        want, bound = mr.select((0, 1), (1, 49), head_mean=True)
        check_maps(mean[layer], want, bound, f"layer {layer} cls -> image, head mean")
    exact = cls.double().mean(2, keepdim=True)
    # nH - 1 additions and one division in f32, all terms positive: nH roundings of at most 2^-24 each; results below the
    # smallest normal f32 may be flushed to zero (1e-37)
    assert bool(((mean.double() - exact).abs() <= nH * U32 * exact + 1e-37).all())


def test_training_mode_raises_and_layer_selection_is_a_slice(M, vqa):
    model = _vqa_model(M, vqa, BF)
    image, ids = vqa["image"].cuda(), vqa["ids"].cuda()
    _, _, every = model.attention_maps(image, ids)
    prob, _, last = model.attention_maps(image, ids, layers=[-1])
    assert last.shape == (1,) + tuple(every.shape[1:]) and torch.equal(last[0], every[-1])
    _, _, picked = model.attention_maps(image, ids, layers=(1, 0, 1))
    assert torch.equal(picked, every[[1, 0, 1]])
    with torch.no_grad():
        feat = model.conv(image)
        hidden_maps = model.MVLBert.attention_maps(ids, feat)
        out, pooled = model.MVLBert(text_idx=ids, text_mask=None, image_feature=feat, image_mask=None)
    assert torch.equal(hidden_maps[1], out.last_hidden_state) and torch.equal(hidden_maps[2], pooled)
    model.train()
    with pytest.raises(ValueError):
        model.attention_maps(image, ids)
    with pytest.raises(ValueError):
        model.MVLBert.attention_maps(ids, torch.zeros(2, 49, 256, device="cuda"))
    model.eval()
    with pytest.raises(ValueError):
        model.attention_maps(image, ids, queries='pixels')
    with pytest.raises(ValueError):
        model.attention_maps(image, ids, layers=[2])
