"""Host side of the logit rules (repetition penalty, no-repeat n-grams, min length): the restatement of tests/logit_rules_ref.py
against the installed transformers processors, the argument checks of decode.check_logit_rules / the model's forward, the routes
(unchanged) and the bookkeeping of the one new C-ABI struct."""
import ctypes
import math
import os
import re
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import logit_rules_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _history(rows, c, V, gen):
    """Random tokens with planted repeats: a bigram and a trigram that come back, a token repeated many times, a PAD tail."""
    h = torch.randint(1, V, (rows, c), generator=gen)
    if c >= 8:
        h[0, c - 2:] = h[0, 1:3]                      # the last bigram occurred at 1 .. 2 (followed by h[0, 3])
        h[1, c - 3:] = h[1, 0:3]                      # the trigram at 0 .. 2 returns at the end
        h[2, :] = 7                                   # one token, many times
        h[3, c // 2:] = 0                             # a finished row: PAD tail (PAD repeats: its n-grams count like any other)
    return h


@pytest.mark.parametrize("g", [1, 2, 3, 4])
def test_restatement_equals_the_transformers_processors(g):
    from transformers import MinLengthLogitsProcessor, NoRepeatNGramLogitsProcessor, RepetitionPenaltyLogitsProcessor
    gen = torch.Generator().manual_seed(40 + g)
    V, rows, eos = 97, 6, 11
    for c in (0, 1, g - 1, g, 12):                    # c + 1 < g (no ban yet), c + 1 == g, and a long history
        h = _history(rows, c, V, gen)
        x = torch.randn(rows, V, generator=gen) * 3
        for penalty, min_length in ((1.0, 0), (1.3, 0), (0.7, 14), (2.0, c)):
            want = RepetitionPenaltyLogitsProcessor(penalty)(h, x.clone()) if penalty != 1.0 else x.clone()
            want = NoRepeatNGramLogitsProcessor(g)(h, want)
            if min_length > 0:
                want = MinLengthLogitsProcessor(min_length, eos, device="cpu")(h, want)
            got = R.process(x, h, penalty, g, min_length, eos)
            assert torch.equal(got, want), (g, c, penalty, min_length)
    # g = 0 and min_length without an eos: nothing banned
    h = _history(rows, 12, V, gen)
    x = torch.randn(rows, V, generator=gen)
    assert torch.equal(R.process(x, h, 1.0, 0, 50, None), x)


def test_penalty_is_applied_once_and_bitmaps_pack_the_sets():
    h = torch.tensor([[3, 3, 3, 199, 0, 0]])
    x = torch.arange(200, dtype=torch.float32)[None] - 50
    y = R.process(x, h, 2.0)
    assert float(y[0, 3]) == -94.0 and float(y[0, 199]) == 74.5 and float(y[0, 0]) == -100.0 and float(y[0, 4]) == -46.0
    seen, banned = R.bitmaps(h, 200, ngram=2)          # ragged last word: 200 = 6 x 32 + 8
    assert seen.shape == (1, 7) and seen.dtype == torch.int32
    assert int(seen[0, 0]) == (1 << 3) | 1 and int(seen[0, 6]) == 1 << 7 and int(seen[0, 1:6].abs().sum()) == 0
    assert int(banned[0, 0]) == 1 and int(banned[0, 1:].abs().sum()) == 0          # the last token 0 was followed by 0
    s31 = R.bitmaps(torch.tensor([[31]]), 64)[0]
    assert int(s31[0, 0]) == -2 ** 31 and int(s31[0, 1]) == 0                       # bit 31: the int32 pattern of 0x80000000


def test_argument_checks():
    from mvlt_amd.decode import check_logit_rules
    assert check_logit_rules() == (1.0, 0, 0) and check_logit_rules(1.3, 2, 5) == (1.3, 2, 5)
    assert check_logit_rules(1, 0, 0, num_beams=4) == (1.0, 0, 0)                   # all off: beams are fine
    for bad in (dict(repetition_penalty=0.0), dict(repetition_penalty=-1.0), dict(repetition_penalty=math.nan),
                dict(no_repeat_ngram_size=-1), dict(min_length=-1), dict(no_repeat_ngram_size=1.5)):
        with pytest.raises(ValueError):
            check_logit_rules(**bad)
    for on in (dict(repetition_penalty=1.2), dict(no_repeat_ngram_size=2), dict(min_length=3)):
        with pytest.raises(ValueError, match="beam"):
            check_logit_rules(num_beams=2, **on)
        with pytest.raises(ValueError, match="vocabulary"):
            check_logit_rules(V=150, max_length=150, **on)
        check_logit_rules(V=151, max_length=150, **on)
    check_logit_rules(V=10, max_length=150)                                           # all off: no such limit


def test_model_forward_refuses_rules_with_beams():
    """The refusal comes first: nothing of the image is touched (no GPU needed)."""
    import mvlt_amd as M
    cfg = M.MVLBertConfigForImageCaption(hidden_size=256, num_hidden_layers=1, num_attention_heads=4, intermediate_size=256, vocab_size=200)
    cfg.swin.update(embed_dim=32, depths=[1, 1, 1, 1], num_heads=[1, 2, 4, 8])
    model = M.MVLBertForImageCaption(cfg, tokenizer=type("Tok", (), {"mask_token_id": 103, "sep_token_id": 102})())
    for on in (dict(repetition_penalty=1.2), dict(no_repeat_ngram_size=2), dict(min_length=3)):
        with pytest.raises(ValueError, match="beam"):
            model(None, None, 3, 'unilm', **on)
    with pytest.raises(ValueError):
        model(None, None, 1, 'unilm', repetition_penalty=0.0)


def test_greedy_route_is_unchanged():
    from mvlt_amd.decode import _greedy_route as route
    assert route('greedy', 32, False, True) == ('graph', 'greedy') and route('sample', 64, True, True) == ('graph', 'sample')
    assert route('greedy', 64, False, False) == ('eager', 'gemm_argmax') and route('greedy', 65, False, True) == ('eager', 'argmax')
    assert route('sample', 64, False, False) == ('eager', 'gemm_sample') and route('sample', 65, False, True) == ('eager', 'multinomial')
    assert route('sample', 65, True, True) == ('eager', 'filtered') and route('sample', 3, True, False) == ('eager', 'filtered')
    with pytest.raises(ValueError):
        route('greedy', 3, True, True)
    with pytest.raises(ValueError):
        route('nucleus', 3, False, True)


def test_logit_rules_struct_bookkeeping():
    """Id 20 in the header, the last ctypes mirror, the size the library and the torch extension were compiled with; the ABI
    version did not move (the change is additive)."""
    from mvlt_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "mvlt_hip.h")).read()
    assert re.search(r"MVLT_STRUCT_LOGIT_RULES = 20, MVLT_STRUCT_COUNT = 21", hdr)
    assert int(re.search(r"#define\s+MVLT_ABI_VERSION\s+(\d+)", hdr).group(1)) == 17 == _lib.ABI_VERSION
    assert _lib.STRUCTS[20] is _lib.MvltLogitRules and len(_lib.STRUCTS) == 21
    assert _lib.lib().mvlt_sizeof(20) == ctypes.sizeof(_lib.MvltLogitRules) == 80
    fields = re.search(r"typedef struct MvltLogitRules \{(.*?)\} MvltLogitRules;", hdr, re.S).group(1)
    fields = re.sub(r"/\*.*?\*/", "", fields, flags=re.S)
    names = [d.strip().split()[-1].lstrip("*") for part in fields.split(";") for d in part.split(",") if d.strip()]
    assert names == [n for n, _ in _lib.MvltLogitRules._fields_], names
    for name in ("mvlt_decode_rules_plan", "mvlt_gemm_argmax_rules", "mvlt_gemm_argmax_greedy_rules", "mvlt_gemm_sample_rules",
                 "mvlt_gemm_sample_step_rules", "mvlt_gemm_sample_filtered_rules", "mvlt_gemm_sample_filtered_step_rules"):
        assert name in _lib.SYMBOLS and hasattr(_lib.lib(), name), name
