"""Attention maps, host side: the range resolver and the heat-map reshape (attention.py), the per-element bound of
tests/attn_maps_ref.py (it accepts an emulation of mvlt_attn_probs' arithmetic at a ratio <= 0.5 and rejects four wrong maps),
the recording Dropper the GPU model tests take the oracle's probabilities from, and the C-ABI entry (declared, bound, exported,
refusing what it must without a launch; ABI version and struct table unchanged)."""
import ctypes
import os
import re

import pytest
import torch

from attn_ref import MASK_OUT, U32, _heads
from attn_maps_ref import FLAGS, MapsRef, check_maps, maps_case, recording_dropper, worst_ratio

BF, F32 = torch.bfloat16, torch.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def A():
    from mvlt_amd import attention
    return attention


# ------------------------------------------------------------------ 1. the range resolver
@pytest.mark.parametrize("n_img", [49, 98])
@pytest.mark.parametrize("T", [0, 1, 23])
def test_resolve_range_names_and_pairs(A, n_img, T):
    L = n_img + 2 + T
    r = A.resolve_range
    assert r('cls', n_img, T) == (0, 1)
    assert r('image', n_img, T) == (1, n_img)
    assert r('sep', n_img, T) == (n_img + 1, 1)
    assert r('all', n_img, T) == (0, L)
    if T:
        assert r('text', n_img, T) == (n_img + 2, T)
    else:
        with pytest.raises(ValueError):
            r('text', n_img, T)
    # the named ranges tile the sequence: [CLS] | image | [SEP] | text
    parts = [r(n, n_img, T) for n in ('cls', 'image', 'sep')] + ([r('text', n_img, T)] if T else [])
    assert parts[0][0] == 0 and all(a[0] + a[1] == b[0] for a, b in zip(parts, parts[1:])) and sum(parts[-1]) == L
    for pair in [(0, 1), (0, L), (L - 1, 1), (n_img + 2, T) if T else (n_img + 1, 1), (7, 3), [5, 2]]:
        assert r(pair, n_img, T) == tuple(pair)
    for bad in [(0, 0), (-1, 2), (L, 1), (0, L + 1), (L - 1, 2), (3, -1), (1.0, 2), (1,), (1, 2, 3), 'img', 'CLS', None, 5,
                (True, 1)]:
        with pytest.raises(ValueError):
            r(bad, n_img, T)


def test_resolve_range_refuses_empty_image_and_negative_counts(A):
    with pytest.raises(ValueError):
        A.resolve_range('image', 0, 4)
    with pytest.raises(ValueError):
        A.resolve_range('all', -1, 4)
    assert A.resolve_range('all', 0, 0) == (0, 2)


def test_resolve_layers(A):
    assert A.resolve_layers(None, 12) == list(range(12))
    assert A.resolve_layers([-1], 12) == [11]
    assert A.resolve_layers((0, -12, 11, 3, 3), 12) == [0, 0, 11, 3, 3]
    for bad in ([12], [-13], []):
        with pytest.raises(ValueError):
            A.resolve_layers(bad, 12)


# ------------------------------------------------------------------ 2. the heat-map reshape
def test_image_heatmap_shapes_and_refusals(A):
    m = torch.arange(2 * 3 * 1 * 9 * 49, dtype=torch.float32).view(2, 3, 1, 9, 49)
    h = A.image_heatmap(m)
    assert h.shape == (2, 3, 1, 9, 1, 7, 7) and torch.equal(h.reshape(m.shape), m)
    assert h[1, 2, 0, 4, 0, 3, 5] == m[1, 2, 0, 4, 3 * 7 + 5]                    # row-major grid: token 7 y + x
    m2 = torch.arange(4 * 98, dtype=torch.float32).view(4, 98)
    h2 = A.image_heatmap(m2, views=2)
    assert h2.shape == (4, 2, 7, 7) and h2[3, 1, 0, 0] == m2[3, 49]               # the second view starts at token 49
    assert A.image_heatmap(torch.zeros(5, 16)).shape == (5, 1, 4, 4)
    for shape, views in [((3, 98), 1), ((3, 49), 2), ((3, 50), 1), ((3, 49), 0), ((3, 48), 2)]:
        with pytest.raises(ValueError):
            A.image_heatmap(torch.zeros(shape), views=views)


# ------------------------------------------------------------------ 3. the bound accepts the kernel's arithmetic, rejects wrong maps
def emulate(c, lse32, q_range, k_range, head_mean=False, renorm=False, fault=None):
    """mvlt_attn_probs' arithmetic on the host: operands as stored (bf16 / f32 values), f32 products and sums over hd, scale and
    mask in f32, f32 exp(s - lse), f32 head mean and row sum.  `fault` bends one step."""
    kw = c["kw"]
    nseq, L, nH, hd, scale = kw["nseq"], kw["L"], kw["nH"], kw["hd"], kw["scale"]
    C = nH * hd
    row_index = None if c["pack"] is None else c["pack"][3]
    Q = _heads(c["qkv"][:, :C], nseq, L, nH, hd, row_index).float()
    K = _heads(c["qkv"][:, C:2 * C], nseq, L, nH, hd, row_index).float()
    bias = c["bias"]
    if fault == "obj_end":                                  # SEQ2SEQ with obj_end one too large
        from attn_ref import bert_bias
        bias = bert_bias(True, nseq, L, c["n_img"] + 1)
    if fault == "no_key_mask":
        bias = torch.zeros_like(bias)
    b = bias.expand(nseq, nH, L, L).float().clone()
    qvalid = torch.ones(nseq, 1, L, 1, dtype=torch.bool)
    if c["pack"] is not None:
        kvalid = torch.arange(L)[None, :] < c["pack"][1].long()[:, None]
        b = torch.where(kvalid[:, None, None, :], b, torch.full_like(b, MASK_OUT))
        qvalid = kvalid[:, None, :, None]
    s = (Q @ K.transpose(-1, -2)) * (1.0 if fault == "no_scale" else scale) + b
    lse = torch.nan_to_num(lse32, nan=0.0)
    if fault == "lse_head":
        lse = lse.roll(1, dims=1)
    P = torch.exp(s - lse[..., None]) * qvalid
    (q0, nq), (k0, nk) = q_range, k_range
    P = P[:, :, q0:q0 + nq, k0:k0 + nk]
    if head_mean:
        acc = torch.zeros_like(P[:, :1])
        for h in range(nH):
            acc = acc + P[:, h:h + 1]
        P = acc / float(nH)
    if renorm:
        S = P.sum(-1, keepdim=True)
        P = torch.where(S > 0, P / torch.where(S > 0, S, torch.ones_like(S)), P)
    return P


CASES = {"A": dict(s2s=False), "B": dict(s2s=True), "C-bidir": dict(s2s=False, lens=(23, 2, 9), packed=True),
         "C-s2s": dict(s2s=True, lens=(23, 2, 9), packed=True)}


@pytest.fixture(scope="module")
def host_case():
    made = {}

    def get(name, dt):
        if (name, dt) not in made:
            c = maps_case(dtype=dt, seed=500 + len(name), **CASES[name])
            lse32 = c["ref"].lse.float()
            c["lse32"] = lse32
            c["maps"] = MapsRef(c["ref"], c["qkv"], lse32, U32 * c["ref"].lse.abs(),
                                pack=None if c["pack"] is None else (c["pack"][3], c["pack"][1]), **c["kw"])
            made[(name, dt)] = c
        return made[(name, dt)]
    return get


def _ranges(c):
    n_img, T, L = c["n_img"], c["T"], c["L"]
    return [((0, 1), (1, n_img)), ((n_img + 2, T), (1, n_img)), ((0, L), (0, L)), ((n_img + 2, T), (0, L))]


@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("dt", [BF, F32])
def test_bound_accepts_the_emulated_kernel(host_case, name, dt):
    c = host_case(name, dt)
    for qr, kr in _ranges(c):
        for hm, rn in FLAGS:
            want, bound = c["maps"].select(qr, kr, hm, rn)
            got = emulate(c, c["lse32"], qr, kr, hm, rn)
            check_maps(got, want, bound, f"{name} {qr}->{kr} mean={hm} renorm={rn}")
            assert worst_ratio(got, want, bound) <= 0.5
    # the probabilities of a row over all keys sum to 1
    want, _ = c["maps"].select((0, c["L"]), (0, c["L"]))
    valid = torch.isfinite(c["ref"].lse)
    assert float((want.sum(-1)[valid] - 1).abs().max()) < 1e-5
    assert float(want.sum(-1)[~valid].abs().max() if (~valid).any() else 0.0) == 0.0


@pytest.mark.parametrize("fault,name", [("obj_end", "B"), ("no_key_mask", "A"), ("no_scale", "A"), ("lse_head", "A")])
@pytest.mark.parametrize("dt", [BF, F32])
def test_bound_rejects_a_wrong_map(host_case, fault, name, dt):
    c = host_case(name, dt)
    L = c["L"]
    want, bound = c["maps"].select((0, L), (0, L))
    good = emulate(c, c["lse32"], (0, L), (0, L))
    assert worst_ratio(good, want, bound) <= 0.5
    bad = emulate(c, c["lse32"], (0, L), (0, L), fault=fault)
    assert worst_ratio(bad, want, bound) > 1.0
    with pytest.raises(AssertionError):
        check_maps(bad, want, bound, fault)
    # ... and the default selection ([CLS] / text -> image, head mean) sees it too, except the causal fault, which lives in the text keys
    if fault != "obj_end":
        qr, kr = (0, 1), (1, c["n_img"])
        want, bound = c["maps"].select(qr, kr, True, False)
        assert worst_ratio(emulate(c, c["lse32"], qr, kr, True, False, fault=fault), want, bound) > 1.0


def test_masked_entries_of_the_reference_are_exactly_zero(host_case):
    a, b = host_case("A", BF), host_case("B", BF)
    PA, _ = a["maps"].select((0, a["L"]), (0, a["L"]))
    masked = (a["bias"] < 0).expand_as(PA)
    assert bool((PA[masked] == 0).all()) and bool((PA[~masked] > 0).all())
    PB, _ = b["maps"].select((0, b["L"]), (0, b["L"]))
    L, oe = b["L"], b["n_img"] + 1
    ar = torch.arange(L)
    above = ~((ar[None, :] <= ar[:, None]) | (ar[None, :] <= oe))
    assert bool((PB[:, :, above] == 0).all()) and bool((PB[:, :, ~above] > 0).all())


# ------------------------------------------------------------------ 4. the oracle's probabilities through a recording Dropper
@pytest.mark.parametrize("seq2seq", [False, True])
def test_recording_dropper_yields_the_oracle_probabilities(seq2seq):
    from oracle import mvlt_oracle as O
    cfg = O.BertCfg(vocab_size=300, hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256)
    g = torch.Generator().manual_seed(7)
    H, B, n_img, T = cfg.hidden_size, 2, 4, 5
    shapes = [("MVLBert.word_embeddings.weight", (cfg.vocab_size + 1, H)), ("MVLBert.position_embeddings.weight", (512, H)),
              ("MVLBert.token_type_embeddings.weight", (3, H))]
    for i in range(2):
        p = f"MVLBert.encoder.layer.{i}."
        for n, o, k in [("attention.self.query", H, H), ("attention.self.key", H, H), ("attention.self.value", H, H),
                        ("attention.output.dense", H, H), ("intermediate.dense", 256, H), ("output.dense", H, 256)]:
            shapes += [(p + n + ".weight", (o, k)), (p + n + ".bias", (o,))]
        for n in ("attention.output.LayerNorm", "output.LayerNorm"):
            shapes += [(p + n + ".weight", (H,)), (p + n + ".bias", (H,))]
    sd = {k: (torch.ones(s) if k.endswith("LayerNorm.weight") else 0.3 * torch.randn(s, generator=g)) for k, s in shapes}
    ids = torch.tensor([[7, 9, 11, 0, 0], [5, 0, 0, 0, 0]])
    img = torch.randn(B, n_img, H, generator=g)
    rec = recording_dropper()
    out = O.mvlbert_forward(sd, cfg, ids, img, seq2seq, drop=rec, return_kv=True)
    plain = O.mvlbert_forward(sd, cfg, ids, img, seq2seq)
    assert torch.equal(out["hidden"], plain["hidden"])                            # recording changes nothing
    L = n_img + 2 + T
    assert sorted(rec.probs) == [f"MVLBert.encoder.layer.{i}.attn_drop" for i in range(2)]
    bm = O.seq2seq_bool_mask(L, n_img + 1)[None].expand(B, L, L) if seq2seq else O.bidir_bool_mask(ids, B, n_img)
    am = O.additive_mask(bm)
    x = O.vl_embeddings(sd, "MVLBert.", cfg, ids, img)
    for i in range(2):
        P = rec.probs[f"MVLBert.encoder.layer.{i}.attn_drop"]
        assert P.shape == (B, 2, L, L)
        assert float((P.sum(-1) - 1).abs().max()) < 1e-5
        # the softmax recomputed from the returned keys and this layer's input
        k = out["kv"][i][0]
        q = torch.nn.functional.linear(x, sd[f"MVLBert.encoder.layer.{i}.attention.self.query.weight"],
                                       sd[f"MVLBert.encoder.layer.{i}.attention.self.query.bias"])
        q = q.view(B, L, 2, H // 2).transpose(1, 2)
        want = ((q @ k.transpose(-1, -2)) * (H // 2) ** -0.5 + am).softmax(-1)
        assert float((P - want).abs().max()) < 1e-6
        assert bool((P[(am < 0).expand_as(P)] == 0).all())
        x, _ = O.bert_layer(x, am, sd, f"MVLBert.encoder.layer.{i}", cfg, O.EVAL)


# ------------------------------------------------------------------ 5. the C-ABI entry
def test_entry_point_is_declared_bound_and_exported():
    from mvlt_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "mvlt_hip.h")).read()
    assert re.search(r"int\s+mvlt_attn_probs\(const MvltAttn\* p, int q0, int nq, int k0, int nk, int flags, float\* out, "
                     r"void\* stream\);", hdr)
    assert re.search(r"MVLT_ATTNMAP_HEAD_MEAN = 1, MVLT_ATTNMAP_RENORM = 2", hdr)
    assert (_lib.ATTNMAP_HEAD_MEAN, _lib.ATTNMAP_RENORM) == (1, 2)
    assert len(_lib.SYMBOLS["mvlt_attn_probs"][1]) == 8 and hasattr(_lib.lib(), "mvlt_attn_probs")
    assert int(re.search(r"#define\s+MVLT_ABI_VERSION\s+(\d+)", hdr).group(1)) == 17 == _lib.ABI_VERSION == _lib.lib().mvlt_version()
    assert re.search(r"MVLT_STRUCT_COUNT = 21\b", hdr) and len(_lib.STRUCTS) == 21
    assert "attnmap.hip" in open(os.path.join(ROOT, "medical-vision-langauge-transformer_amd", "csrc", "Makefile")).read()


def _desc(_lib, **over):
    buf = (ctypes.c_char * 64)()                         # never dereferenced: every call below is refused before a launch
    addr = (ctypes.addressof(buf) + 15) & ~15
    p = _lib.MvltAttn()
    p.dtype, p.mode, p.nseq, p.L, p.nH, p.hd = _lib.BF16, _lib.ATTN_BIDIR, 2, 74, 2, 64
    p.qkv, p.lse, p.scale, p.text_ids, p.T, p.obj_end = addr, addr, 0.125, addr, 23, 50
    for k, v in over.items():
        setattr(p, k, v)
    return p, addr


def test_refusals_need_no_device():
    """Every refusal of the header is answered from the arguments alone, before any launch (there is no GPU here)."""
    from mvlt_amd import _lib
    f = _lib.lib().mvlt_attn_probs
    ARG, UNS = -1, -3
    call = lambda p, q0, nq, k0, nk, flags, out: f(ctypes.byref(p), q0, nq, k0, nk, flags, out, None)  # noqa: E731
    p, addr = _desc(_lib)
    assert call(_desc(_lib, mode=_lib.ATTN_SWIN)[0], 0, 1, 1, 49, 0, addr) == UNS
    assert call(_desc(_lib, hd=32)[0], 0, 1, 1, 49, 0, addr) == UNS
    assert call(_desc(_lib, mode=7)[0], 0, 1, 1, 49, 0, addr) == ARG
    for q0, nq, k0, nk in [(0, 0, 1, 49), (0, -1, 1, 49), (0, 1, 1, 0), (0, 1, 1, -3), (-1, 2, 1, 49), (0, 1, -1, 49),
                           (74, 1, 1, 49), (0, 75, 1, 49), (0, 1, 26, 49), (0, 1, 0, 75), (2147483647, 2, 0, 1)]:
        assert call(p, q0, nq, k0, nk, 0, addr) == ARG, (q0, nq, k0, nk)
    assert call(_desc(_lib, lse=None)[0], 0, 1, 1, 49, 0, addr) == ARG
    assert call(_desc(_lib, qkv=None)[0], 0, 1, 1, 49, 0, addr) == ARG
    assert call(p, 0, 1, 1, 49, 0, None) == ARG
    for flags in (4, 8, 7, -1, 1 << 30):
        assert call(p, 0, 1, 1, 49, flags, addr) == ARG, flags
    assert call(_desc(_lib, qkv=addr + 8)[0], 0, 1, 1, 49, 0, addr) == ARG
    assert call(_desc(_lib, T=22)[0], 0, 1, 1, 49, 0, addr) == ARG            # obj_end + 1 + T != L
    assert call(_desc(_lib, row_start=addr)[0], 0, 1, 1, 49, 0, addr) == ARG  # row_start without seq_len
    assert call(_desc(_lib, dtype=5)[0], 0, 1, 1, 49, 0, addr) == UNS
    assert call(_desc(_lib, L=300, T=249)[0], 0, 1, 0, 209, 0, addr) == UNS   # more than 13 key tiles
    assert f(None, 0, 1, 1, 49, 0, addr, None) == ARG
