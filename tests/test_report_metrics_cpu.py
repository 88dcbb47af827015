"""Report metrics without a GPU: the restatement of tests/report_metrics_ref.py against what the reference's own scorers returned
(tests/golden/report_metrics.npz), the segmentation rule against the string pipeline, the host-side pieces of
mvlt_amd.report_metrics on CPU tensors, and the C-ABI of the two entry points.

Tolerances: integers exactly; scores 1e-12 relative (+ 1e-15 absolute for the scores that are 0) -- the same formulas in the
same f64, summed over at most a few thousand non-negative terms in another order."""
import os
import random
import re

import numpy as np
import pytest
import torch

import report_metrics_ref as R
from conftest import GOLD, ROOT

REL, ABS = 1e-12, 1e-15


@pytest.fixture(scope="module")
def gold():
    with np.load(os.path.join(GOLD, "report_metrics.npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def restated(gold):
    return {n: R.score_corpus(*R.golden_corpus(gold, n)) for n in "ABC"}


def close(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape
    assert (np.abs(a - b) <= REL * np.abs(b) + ABS).all(), float(np.abs(a - b).max())


def test_fixture_holds_the_cases_it_is_for(gold):
    h, r = R.golden_corpus(gold, "A")
    assert len(h) == 24 and max(map(len, h + r)) == 40 and {w[0] for row in h + r for w in row} <= set(range(1, 13))
    assert any(not x for x in h) and any(len(x) == 1 for x in h) and any(x == y and x for x, y in zip(h, r))
    assert any(len(x) > len(y) > 0 for x, y in zip(h, r)) and any(not y for y in r)
    assert not any(not x and not y for x, y in zip(h, r))
    assert any(max(R.ngrams(x, 2).values(), default=0) > max(R.ngrams(y, 2).values(), default=0) > 0 for x, y in zip(h, r))
    assert any(r[i] == r[j] for i in range(24) for j in range(i)) and gold["A_df_counts"].max() > 1
    assert len(R.golden_corpus(gold, "B")[0]) == 1 and (gold["B_cider"] == 0).all()
    hc, rc = R.golden_corpus(gold, "C")
    assert len(hc) == 3 and len(hc[0]) == 512 == len(rc[0])
    assert os.path.getsize(os.path.join(GOLD, "report_metrics.npz")) < 100 * 1024


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_restatement_equals_the_reference_scorers(gold, restated, name):
    o = restated[name]
    assert np.array_equal(np.array(o["stats"]), gold[name + "_comps"])
    close(o["bleu"], gold[name + "_bleu"])
    close(o["rouge"], gold[name + "_rouge"])
    close(o["cider"], gold[name + "_cider"])
    close([o["corpus"][k] for k in R.KEYS], gold[name + "_corpus"])
    df = {tuple((int(t),) for t in g if t != 0): int(c) for g, c in zip(gold[name + "_df_grams"], gold[name + "_df_counts"])}
    assert df == dict(o["df"])


def test_segmentation_rule_equals_the_string_pipeline():
    tokens = ["[PAD]", "a", "b", "c", "-", ".", "##s", "##t"]
    flags = [0, 0, 0, 0, R.JOIN, R.BREAK, R.CONT, R.CONT]
    rng = random.Random(7)
    edge = 0
    for _ in range(20000):
        n = rng.randint(0, 9)
        ids = [rng.randint(1, 7) for _ in range(n)]
        if ids and flags[ids[0]] & R.CONT:
            ids[0] = rng.randint(1, 5)                    # the tokenizer never opens a report with a ## piece
        edge += bool(ids) and (ids[0] == 4 or ids[-1] == 4)
        words = R.segment(ids + [0, 3, 3], flags)          # junk after the stop id
        assert [R.render(w, tokens) for w in words] == R.string_pipeline([tokens[i] for i in ids]), ids
        assert [p for w in words for p in w] == ids
    assert edge > 2000
    assert R.segment([1, 4, 2, 5, 3, 6, 102, 1], flags) == [(1, 4, 2), (5,), (3, 6)]
    assert R.segment([1, 4, 4, 2], flags) == [(1, 4, 4), (2,)] and R.segment([4, 1, 4], flags) == [(4,), (1,), (4,)]
    assert R.segment([1, 4, 6, 99, -3], flags) == [(1,), (4, 6), (99,), (-3,)]
    assert R.segment([5, 6, 7, 104], None) == [(5,), (6,), (7,)]


def test_word_flags():
    from mvlt_amd import report_metrics as RM
    f = RM.word_flags(["[PAD]", "the", "##s", "-", ".", "##.", "--", "..", "3.5"])
    assert f.dtype == torch.uint8 and f.tolist() == [0, 0, RM.CONT, RM.JOIN, RM.BREAK, RM.CONT, 0, 0, 0]
    assert (RM.CONT, RM.JOIN, RM.BREAK, RM.STOP_IDS) == (R.CONT, R.JOIN, R.BREAK, R.STOP_IDS) == (1, 2, 4, (0, 102, 104))


def test_sample_scores_on_cpu_tensors_equal_the_golden(gold):
    from mvlt_amd import report_metrics as RM
    for name in "ABC":
        bleu, rouge = RM.sample_scores(torch.from_numpy(gold[name + "_comps"]))
        assert bleu.dtype == torch.float64 and rouge.dtype == torch.float64
        close(bleu.numpy(), gold[name + "_bleu"])
        close(rouge.numpy(), gold[name + "_rouge"])


def test_corpus_arithmetic_on_cpu_tensors_equals_the_golden(gold):
    from mvlt_amd import report_metrics as RM
    for name in "ABC":
        got = RM.corpus_scores(torch.from_numpy(gold[name + "_comps"]), torch.from_numpy(gold[name + "_rouge"]),
                               torch.from_numpy(gold[name + "_cider"]))
        assert tuple(got) == R.KEYS
        close([got[k] for k in R.KEYS], gold[name + "_corpus"])
    with pytest.raises(RuntimeError, match="twice, never"):
        RM._finish([0.0] * 12 + [2.0], 5)


def test_key_function_is_the_documented_one():
    assert R.mix64(0) == 0 and R.mix64(1) == 0x5692161D100B05E5           # splitmix64's finaliser
    assert R.gram_key(((7,),)) != R.gram_key(((7,), (7,))) != R.gram_key(((7, 7),))
    keys = {R.gram_key(tuple((a,) for a in g)) for g in [(a, b) for a in range(40) for b in range(40)]}
    assert len(keys) == 1600 and all(-(1 << 63) <= k < R.NO_KEY for k in keys)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "0x9E3779B97F4A7C15" in design and "2^65" in design


def test_cabi_declares_binds_and_exports_the_two_entry_points():
    from mvlt_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "mvlt_hip.h")).read()
    for name, nargs in (("mvlt_report_ngram_keys", 11), ("mvlt_report_stats", 19)):
        proto = re.search(r"\bint " + name + r"\(([^;]*?)\);", hdr, re.S).group(1)
        assert len(proto.split(",")) == nargs == len(_lib.SYMBOLS[name][1]), name
        assert _lib.SYMBOLS[name][0] is _lib.i32 and hasattr(_lib.lib(), name), name
        # pointers are void* / the host stop-id array in the mirror, scalars keep their width
        for decl, ct in zip(proto.split(","), _lib.SYMBOLS[name][1]):
            decl = " ".join(decl.split())
            want = (_lib.C.POINTER(_lib.i64) if "stop_ids" in decl else _lib.vp) if "*" in decl else \
                _lib.i64 if decl.startswith("int64_t") else _lib.i32
            assert ct is want or ct == want, (name, decl)
    assert int(re.search(r"#define\s+MVLT_ABI_VERSION\s+(\d+)", hdr).group(1)) == 17 == _lib.ABI_VERSION == _lib.lib().mvlt_version()
    assert re.search(r"MVLT_STRUCT_COUNT = 21\b", hdr) and len(_lib.STRUCTS) == 21


def test_rows_longer_than_the_limit_are_refused_before_launch():
    from mvlt_amd import ops
    assert ops.REPORT_MAX_PIECES == 512
    with pytest.raises(ValueError, match="512"):
        ops._report_rows(torch.zeros(2, 513, dtype=torch.int64), "hyp")
    ops._report_rows(torch.zeros(2, 512, dtype=torch.int64), "hyp")
