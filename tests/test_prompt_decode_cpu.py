"""Host side of the prompted decode (``greedy_search(input_ids=, prompt_lengths=)``) without a GPU: the two C-ABI additions (no
new struct, no ABI bump), the tables ``decode.prompt_tables`` builds, every argument refusal, and the route table of calls
without a prompt, which stays what it was."""
import ctypes as C
import inspect
import os
import re

import pytest
import torch

from mvlt_amd import decode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mvlt_attn_cached_rows", "mvlt_embed_fwd_rows")
# ctypes sizes of _lib.STRUCTS, in registry order, as they were before these entry points
SIZES = [232, 104, 208, 32, 200, 216, 160, 80, 16, 16, 64, 112, 24, 128, 32, 64, 104, 48, 160, 208, 80]
MASK = 103


def test_new_entry_points_are_bound_and_exported_without_an_abi_bump():
    from mvlt_amd import _lib
    L = _lib.lib()
    with open(os.path.join(ROOT, "include", "mvlt_hip.h")) as f:
        hdr = f.read()
    for name in NEW:
        assert name in _lib.SYMBOLS and getattr(L, name) is not None
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
    assert int(re.search(r"#define\s+MVLT_ABI_VERSION\s+(\d+)", hdr).group(1)) == 17 == _lib.ABI_VERSION == L.mvlt_version()
    assert re.search(r"MVLT_STRUCT_COUNT = 21\b", hdr) and len(_lib.STRUCTS) == 21
    assert [C.sizeof(s) for s in _lib.STRUCTS] == SIZES == [L.mvlt_sizeof(i) for i in range(21)]


def test_new_entry_points_refuse_bad_arguments_before_any_launch():
    from mvlt_amd import _lib
    L = _lib.lib()
    ERR_ARG = next(k for k, v in _lib.ERRORS.items() if v == "MVLT_ERR_ARG")
    ERR_UNSUPPORTED = next(k for k, v in _lib.ERRORS.items() if v == "MVLT_ERR_UNSUPPORTED")
    buf = (C.c_double * 64)()
    a = C.addressof(buf)
    a += a % 16
    vp = C.c_void_p
    p = _lib.MvltAttnCached()
    p.dtype, p.B, p.nH, p.hd, p.n_new, p.cache_cap, p.past = _lib.F32, 1, 1, 64, 2, 8, 4
    p.qkv_new = p.k_cache = p.v_cache = p.out = a
    assert L.mvlt_attn_cached_rows(None, vp(a), vp(0)) == ERR_ARG
    assert L.mvlt_attn_cached_rows(C.byref(p), vp(0), vp(0)) == ERR_ARG               # no table
    p.past = 7
    assert L.mvlt_attn_cached_rows(C.byref(p), vp(a), vp(0)) == ERR_ARG               # past + n_new > cache_cap
    p.past = -1
    assert L.mvlt_attn_cached_rows(C.byref(p), vp(a), vp(0)) == ERR_ARG
    p.past, p.out = 4, None
    assert L.mvlt_attn_cached_rows(C.byref(p), vp(a), vp(0)) == ERR_ARG
    p.out, p.hd = a, 32
    assert L.mvlt_attn_cached_rows(C.byref(p), vp(a), vp(0)) == ERR_UNSUPPORTED       # no serial form
    p.hd, p.n_new, p.past = 64, 5, 0
    assert L.mvlt_attn_cached_rows(C.byref(p), vp(a), vp(0)) == ERR_UNSUPPORTED
    p.n_new, p.qkv_new = 2, a + 4
    assert L.mvlt_attn_cached_rows(C.byref(p), vp(a), vp(0)) == ERR_UNSUPPORTED       # misaligned
    e = _lib.MvltEmbed()
    e.dtype, e.B, e.n_img, e.T, e.H, e.type_override, e.pos_rows, e.pos_offset = _lib.F32, 1, -1, 2, 8, 0, 16, 3
    e.text_ids = e.word_emb = e.pos_emb = e.type_emb = e.out = a
    assert L.mvlt_embed_fwd_rows(C.byref(e), vp(0), vp(0)) == ERR_ARG                 # no table
    e.pos_rows = 0
    assert L.mvlt_embed_fwd_rows(C.byref(e), vp(a), vp(0)) == ERR_ARG                 # the clamp needs the table's size
    e.pos_rows, e.pos_offset = 16, 16
    assert L.mvlt_embed_fwd_rows(C.byref(e), vp(a), vp(0)) == ERR_ARG
    e.pos_offset, e.out = 3, None
    assert L.mvlt_embed_fwd_rows(C.byref(e), vp(a), vp(0)) == ERR_ARG


def test_prompt_tables_ragged():
    ids = torch.tensor([[7, 7, 7, 7, 7], [11, 12, 9, 9, 9], [21, 22, 23, 24, 25]])
    text, shift, col = decode.prompt_tables(ids, [0, 2, 5], MASK)
    assert text.dtype == torch.int64 and text.shape == (3, 6) and text.is_contiguous()
    assert text.tolist() == [[MASK] * 6, [11, 12, MASK, MASK, MASK, MASK], [21, 22, 23, 24, 25, MASK]]
    assert shift.dtype == torch.int32 and shift.tolist() == [-5, -3, 0]
    assert col.dtype == torch.int64 and col.tolist() == [0, 2, 5]
    for b, n in enumerate([0, 2, 5]):          # the contract: the row's own tokens, then [MASK] at its own column
        assert text[b, :n].tolist() == ids[b, :n].tolist() and text[b, n] == MASK
    assert ids.tolist()[0] == [7] * 5          # the argument is not written


def test_prompt_tables_uniform_and_none():
    ids = torch.tensor([[5, 6, 7], [8, 9, 10]])
    a = decode.prompt_tables(ids, [3, 3], MASK)
    b = decode.prompt_tables(ids, None, MASK)
    for x, y in zip(a, b):
        assert torch.equal(x, y) and x.dtype == y.dtype
    assert a[0].tolist() == [[5, 6, 7, MASK], [8, 9, 10, MASK]] and a[1].tolist() == [0, 0] and a[2].tolist() == [3, 3]
    text, shift, col = decode.prompt_tables(torch.zeros((2, 0), dtype=torch.int64), None, MASK)          # P_max = 0
    assert text.tolist() == [[MASK], [MASK]] and shift.tolist() == [0, 0] and col.tolist() == [0, 0]


def test_check_prompt_accepts_and_normalises():
    ids = torch.zeros((3, 5), dtype=torch.int64)
    assert decode.check_prompt(ids, None, 3, 49, 8, 512) == [5, 5, 5]
    assert decode.check_prompt(ids, [0, 2, 5], 3, 49, 8, 512) == [0, 2, 5]
    assert decode.check_prompt(ids, torch.tensor([0, 2, 5]), 3, 49, 8, 512) == [0, 2, 5]
    assert decode.check_prompt(ids, (1, 1, 1), 3, 49, 8, 49 + 2 + 5 + 8 + 1) == [1, 1, 1]          # the last position that exists


@pytest.mark.parametrize("lengths,B,pos_rows,what", [
    ([0, 2, 6], 3, 512, "length > P_max"),
    ([0, -1, 5], 3, 512, "negative length"),
    ([0, 2.5, 5], 3, 512, "not an integer"),
    ("meta", 3, 512, "lengths on a device"),
    ([0, 2], 3, 512, "wrong number of lengths"),
    ([0, 2, 5], 4, 512, "wrong batch"),
    ([0, 2, 5], 3, 49 + 2 + 5 + 8, "position overflow"),
    (None, 3, 49 + 2 + 5 + 8, "position overflow, dense"),
])
def test_check_prompt_refusals(lengths, B, pos_rows, what):
    ids = torch.zeros((3, 5), dtype=torch.int64)
    if lengths == "meta":
        lengths = torch.empty(3, dtype=torch.int64, device="meta")
    with pytest.raises(ValueError):
        decode.check_prompt(ids, lengths, B, 49, 8, pos_rows)


def test_check_prompt_refuses_other_id_tensors():
    for bad in (torch.zeros((3, 5), dtype=torch.int32), torch.zeros(15, dtype=torch.int64), [[1, 2]]):
        with pytest.raises(ValueError):
            decode.check_prompt(bad, None, 3, 49, 8, 512)


def _cpu_model(max_pos=512):
    import mvlt_amd as M
    cfg = M.MVLBertConfigForImageCaption(hidden_size=256, num_hidden_layers=1, num_attention_heads=4, intermediate_size=256,
                                         vocab_size=3000)
    cfg.swin.update(embed_dim=32, depths=[2, 2, 2, 2], num_heads=[1, 2, 4, 8])
    cfg.max_position_embeddings = max_pos
    cfg.max_length = 8
    return M.MVLBertForImageCaption(cfg)


def test_greedy_search_refuses_a_bad_prompt_before_any_device_work():
    """On a CPU model: a refusal that came after the first kernel launch would fail here in another way."""
    model = _cpu_model(max_pos=65)          # 49 + 2 + 5 + 8 + 1 = 65: the default max_length of 8 just fits
    assert model.MVLBert.position_embeddings.weight.shape[0] == 65
    feat = torch.zeros(3, 49, 256)
    ids = torch.zeros((3, 5), dtype=torch.int64)
    for kw, match in ((dict(input_ids=ids, prompt_lengths=[0, 2, 6]), "prompt lengths must be"),
                      (dict(input_ids=ids, prompt_lengths=[0, -2, 5]), "prompt lengths must be"),
                      (dict(input_ids=ids[:2]), "2 rows for a batch of 3"),
                      (dict(input_ids=ids, prompt_lengths=torch.empty(3, dtype=torch.int64, device="meta")), "host integers"),
                      (dict(input_ids=ids, max_length=9), "66 positions"),
                      (dict(prompt_lengths=[1, 1, 1]), "without input_ids")):
        with pytest.raises(ValueError, match=match):
            decode.greedy_search(model, feat, **kw)


def test_generate_refuses_a_prompt_with_beams_or_several_sequences():
    model = _cpu_model()
    img = torch.zeros(2, 3, 224, 224)
    ids = torch.zeros((2, 4), dtype=torch.int64)
    with pytest.raises(ValueError, match="prompt"):
        model.generate(img, num_beams=2, prompt_ids=ids)
    with pytest.raises(ValueError, match="prompt"):
        model.generate(img, sample_mode='sample', num_return_sequences=3, prompt_ids=ids)
    with pytest.raises(ValueError, match="prompt"):
        model.generate(img, prompt_lengths=[1, 1])
    sig = inspect.signature(type(model).generate).parameters
    assert sig["prompt_ids"].default is None and sig["prompt_lengths"].default is None
    fwd = list(inspect.signature(type(model).forward).parameters)          # forward() keeps the reference signature
    assert "prompt_ids" not in fwd and "input_ids" not in fwd
    gs = inspect.signature(decode.greedy_search).parameters
    assert gs["input_ids"].default is None and gs["prompt_lengths"].default is None


def test_route_of_calls_without_a_prompt_is_unchanged():
    r = decode._greedy_route
    assert list(inspect.signature(r).parameters) == ["sample_mode", "B", "filtered", "graph_on"]
    assert r('greedy', 64, False, True) == ('graph', 'greedy') and r('sample', 3, True, True) == ('graph', 'sample')
    assert r('greedy', 65, False, True) == ('eager', 'argmax') and r('greedy', 64, False, False) == ('eager', 'gemm_argmax')
    assert r('sample', 64, False, False) == ('eager', 'gemm_sample') and r('sample', 65, False, True) == ('eager', 'multinomial')
    assert r('sample', 65, True, True) == ('eager', 'filtered')
    with pytest.raises(ValueError):
        r('greedy', 3, True, True)
    with pytest.raises(ValueError):
        r('nucleus', 3, False, True)
