"""Report metrics on the GPU: mvlt_report_ngram_keys / mvlt_report_stats and the Python surface of mvlt_amd.report_metrics
against the reference's own scorers (tests/golden/report_metrics.npz) and the exact-tuple restatement of
tests/report_metrics_ref.py (proved against the same fixture by tests/test_report_metrics_cpu.py).

Tolerances: the 11 integers, the word counts and the document frequencies exactly.  BLEU, ROUGE-L and CIDEr 1e-9 relative +
1e-12 absolute: every sum has at most about 2 000 non-negative f64 terms (idf >= 0 because df <= N), nothing cancels, so the
error is a few ulp per libm call times the term count, about 1e-12; 1e-9 leaves three decades for the device's log / exp / sqrt."""
import os
import random

import numpy as np
import pytest
import torch

import report_metrics_ref as R
from conftest import GOLD, synth_batch
from tiny_caption import tiny_caption

pytestmark = pytest.mark.gpu

REL, ABS = 1e-9, 1e-12


@pytest.fixture(scope="module")
def gold():
    with np.load(os.path.join(GOLD, "report_metrics.npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def RM():
    from mvlt_amd import report_metrics
    return report_metrics


def close(a, b, what=""):
    a = np.asarray(a.cpu() if torch.is_tensor(a) else a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err = np.abs(a - b)
    print(f"{what}: max abs error {float(err.max()) if err.size else 0.0:.3e}")
    assert (err <= REL * np.abs(b) + ABS).all(), (what, float(err.max()))


def padded(rows, width=None):
    width = width or max(1, max(len(r) for r in rows))
    return torch.tensor([list(r) + [0] * (width - len(r)) for r in rows], dtype=torch.int64)


def check_against(RM, hyp_rows, ref_rows, flags, want, width=None):
    """score() and ReferenceSet on id rows against a score_corpus() result."""
    refs = RM.ReferenceSet(padded(ref_rows, width), None if flags is None else torch.tensor(flags, dtype=torch.uint8))
    keys, counts = R.df_table(want["df"])
    assert refs.df_keys.cpu().tolist() == keys and refs.df_counts.cpu().tolist() == counts
    assert refs.df_keys.dtype == torch.int64 and refs.df_counts.dtype == torch.int32
    assert refs.n_words.cpu().tolist() == [s[1] for s in want["stats"]]
    out = RM.score(padded(hyp_rows, width).cuda(), refs)
    assert out["stats"].dtype == torch.int32 and out["stats"].is_cuda and out["cider"].dtype == torch.float64
    assert out["stats"].cpu().tolist() == want["stats"]
    close(out["bleu"], want["bleu"], "bleu")
    close(out["rouge_l"], want["rouge"], "rouge_l")
    close(out["cider"], want["cider"], "cider")
    scorer = RM.ReportScorer(refs)
    scorer.add(padded(hyp_rows, width).cuda(), torch.arange(len(hyp_rows)))
    got = scorer.result()
    assert tuple(got) == R.KEYS
    close([got[k] for k in R.KEYS], [want["corpus"][k] for k in R.KEYS], "corpus")
    return refs, out


# ------------------------------------------------------------------------------------------------ ids = words, the golden
@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_words_as_ids_equal_the_reference_scorers(RM, gold, name):
    hyps, refs = R.golden_corpus(gold, name)
    want = R.score_corpus(hyps, refs)
    flat = lambda rows: [[w[0] for w in row] for row in rows]
    _, out = check_against(RM, flat(hyps), flat(refs), None, want)
    assert np.array_equal(out["stats"].cpu().numpy(), gold[name + "_comps"])
    close(out["bleu"], gold[name + "_bleu"], "bleu vs golden")
    close(out["rouge_l"], gold[name + "_rouge"], "rouge_l vs golden")
    close(out["cider"], gold[name + "_cider"], "cider vs golden")
    corpus = RM.corpus_scores(out["stats"], out["rouge_l"], out["cider"])
    close([corpus[k] for k in R.KEYS], gold[name + "_corpus"], "corpus vs golden")
    if name == "C":
        assert out["stats"][0, :2].tolist() == [512, 512]


# ------------------------------------------------------------------------------------------------ pieces and flags
HYPHEN, PERIOD, NFLAGS = 5, 6, 64
PIECE_FLAGS = [0] * NFLAGS
PIECE_FLAGS[HYPHEN], PIECE_FLAGS[PERIOD] = R.JOIN, R.BREAK
for _w in range(1, 13):
    PIECE_FLAGS[30 + _w] = PIECE_FLAGS[50 + _w] = R.CONT


def as_pieces(rng, words):
    """Word w becomes 1 + w % 3 pieces (10 + w, then the CONT pieces 30 + w, 50 + w); hyphens and periods drop in between."""
    row = []
    for w in words:
        row += [10 + w, 30 + w, 50 + w][:1 + w % 3]
        u = rng.random()
        if u < 0.15:
            row.append(HYPHEN)
        elif u < 0.25:
            row.append(PERIOD)
        elif u < 0.28:
            row += [HYPHEN, HYPHEN]
    return row


def test_pieces_with_flags_equal_the_restatement(RM, gold):
    rng = random.Random(99)
    hyps, refs = R.golden_corpus(gold, "A")
    hyp_rows = [as_pieces(rng, [w[0] for w in row]) for row in hyps]
    ref_rows = [as_pieces(rng, [w[0] for w in row]) for row in refs]
    alphabet = [11, 12, 13, HYPHEN, PERIOD, 31, 52]                       # a b c - . ##s ##t of the CPU test
    for _ in range(16):
        for rows in (hyp_rows, ref_rows):
            row = [rng.choice(alphabet) for _ in range(rng.randint(1, 9))]
            if PIECE_FLAGS[row[0]] & R.CONT:
                row[0] = 11
            rows.append(row)
    hyp_rows += [[HYPHEN, 11, HYPHEN], [11, HYPHEN, HYPHEN, HYPHEN, 12, PERIOD]]
    ref_rows += [[HYPHEN, 11, HYPHEN, 12], [11, HYPHEN, HYPHEN, 12, PERIOD]]
    seg = lambda rows: [R.segment(r, PIECE_FLAGS) for r in rows]
    want = R.score_corpus(seg(hyp_rows), seg(ref_rows))
    assert any(len(w) > 1 for row in seg(ref_rows) for w in row)
    assert sum(s[0] for s in want["stats"]) < sum(map(len, hyp_rows))      # the flags merge pieces
    check_against(RM, hyp_rows, ref_rows, PIECE_FLAGS, want)


def test_stop_ids_and_ids_outside_the_table(RM):
    flags = [0] * 16
    flags[3], flags[4], flags[5] = R.CONT, R.JOIN, R.BREAK
    hyp_rows = [[7, 8, 9, 102, 7, 3, 7],                  # junk after the first stop id
                [7, 8, 9, 7, 8, 9, 3],                    # no stop id: the row's end
                [7, 10 ** 6, 8, 3, 16, 3],                # ids >= V: ordinary pieces, not table look-ups
                [-5, 7, -5, 3, 104, 9],                   # ids < 0
                [104, 7, 8, 9, 1, 2, 3]]                  # a stop id first: empty
    ref_rows = [[7, 8, 9, 104, 3, 3, 3],
                [7, 8, 9, 3, 7, 8, 9],
                [7, 10 ** 6, 8, 3, 2 ** 40, 16, 3],
                [-5, 7, -5, 3, -(2 ** 40), 0, 7],
                [7, 8, 9, 1, 4, 2, 3]]
    seg = lambda rows: [R.segment(r, flags) for r in rows]
    want = R.score_corpus(seg(hyp_rows), seg(ref_rows))
    assert [s[0] for s in want["stats"]] == [3, 6, 4, 3, 0]
    check_against(RM, hyp_rows, ref_rows, flags, want, width=7)
    refs = RM.ReferenceSet(padded(ref_rows, 7), torch.tensor(flags, dtype=torch.uint8), stop_ids=(9,))
    assert refs.n_words.cpu().tolist() == [len(R.segment(r, flags, (9,))) for r in ref_rows]


def test_list_references_and_the_row_limit(RM):
    refs = RM.ReferenceSet([[7, 8, 9], [7], []])
    assert refs.ids.shape == (3, 3) and refs.n_words.cpu().tolist() == [3, 1, 0]
    with pytest.raises(ValueError, match="512"):
        RM.ReferenceSet(torch.ones(2, 513, dtype=torch.int64))
    with pytest.raises(ValueError, match="512"):
        RM.score(torch.ones(2, 513, dtype=torch.int64), refs)
    with pytest.raises(ValueError, match="index"):
        RM.score(torch.ones(4, 5, dtype=torch.int64), refs)


# ------------------------------------------------------------------------------------------------ index, visits, determinism
def test_index_order_visits_and_bitwise_repeatability(RM, gold):
    hyp = torch.from_numpy(gold["A_hyp"].astype(np.int64)).cuda()
    refs = RM.ReferenceSet(torch.from_numpy(gold["A_ref"].astype(np.int64)))
    N = hyp.shape[0]
    a, b = RM.score(hyp, refs), RM.score(hyp, refs)
    for k in ("stats", "bleu", "rouge_l", "cider"):
        assert torch.equal(a[k], b[k]), k
    one = RM.ReportScorer(refs)
    one.add(hyp, torch.arange(N))
    in_order = one.result()
    perm = torch.randperm(N, generator=torch.Generator().manual_seed(3))
    two = RM.ReportScorer(refs)
    two.add(hyp[perm[:9].cuda()], perm[:9])
    two.add(hyp[perm[9:].cuda()], perm[9:].tolist())
    assert two.result() == in_order                       # the same bits: the buffers are indexed by sample
    assert torch.equal(two.cider, one.cider) and torch.equal(two.stats, one.stats) and torch.equal(two.bleu, one.bleu)
    shuffled = RM.score(hyp[perm.cuda()], refs, perm)
    assert torch.equal(shuffled["cider"], a["cider"][perm.cuda()]) and torch.equal(shuffled["stats"], a["stats"][perm.cuda()])
    missing = RM.ReportScorer(refs)
    missing.add(hyp[:N - 1], torch.arange(N - 1))
    with pytest.raises(RuntimeError, match="twice, never"):
        missing.result()
    twice = RM.ReportScorer(refs)
    twice.add(hyp, torch.arange(N))
    twice.add(hyp[:1], [0])
    with pytest.raises(RuntimeError, match="twice, never"):
        twice.result()
    outside = RM.ReportScorer(refs)
    got = outside.add(hyp, torch.arange(N) + torch.tensor([0] * (N - 1) + [5]))
    assert got["stats"][-1, 1].item() == -1 and got["cider"][-1].item() == 0.0
    with pytest.raises(RuntimeError, match="twice, never"):
        outside.result()


# ------------------------------------------------------------------------------------------------ end to end
@pytest.mark.parametrize("num_beams", [1, 2])
def test_evaluate_equals_the_restatement_of_what_generate_returned(RM, specs_hash, num_beams):
    import mvlt_amd as M
    model, _ = tiny_caption(M, specs_hash, torch.float32, max_length=8)
    images = [synth_batch(4, 24, seed=60 + i, vocab=3000)[0].cuda() for i in range(2)]
    decoded = []
    for image in images:
        out = model.generate(image, num_beams=num_beams)
        decoded += (out if torch.is_tensor(out) else out[0]).cpu().tolist()
    flags = [R.CONT if i % 4 == 1 else R.JOIN if i % 11 == 2 else R.BREAK if i % 13 == 3 else 0 for i in range(3000)]
    rng = random.Random(5)
    ref_rows = []
    for i, row in enumerate(decoded):                     # references that share n-grams with what the model says
        row = [t for t in R.cut(row)]
        if i % 3 == 1 and row:
            row[rng.randrange(len(row))] = rng.randint(200, 2999)
        if i % 3 == 2:
            row = row[1:] + row[:2]
        ref_rows.append(row + [102])
    refs = RM.ReferenceSet(ref_rows, torch.tensor(flags, dtype=torch.uint8))
    got = RM.evaluate(model, [(image, None) for image in images], refs, num_beams=num_beams)
    want = R.score_corpus([R.segment(r, flags) for r in decoded], [R.segment(r, flags) for r in ref_rows])["corpus"]
    print(num_beams, got)
    close([got[k] for k in R.KEYS], [want[k] for k in R.KEYS], "evaluate")
    assert got["BLEU_1"] > 0.5
