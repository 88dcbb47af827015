"""Make tests/golden/report_metrics.npz: word-id corpora and what the reference's own scorers return for them.

    python tests/golden/make_report_metrics_golden.py <root of the reference tree>

Runs on a CPU host that has the reference checked out.  The reference's pycocoevalcap (Bleu, BleuScorer, Rouge, my_lcs, Cider,
CiderScorer) is imported as a library and only its inputs and outputs are recorded; none of its text is copied.  Words are
written as decimal strings joined by single spaces, which is what compute_scores hands to the scorers after its replace().

Per corpus X in A, B, C: X_hyp / X_ref int16 [N, T] (word ids >= 1, padded with 0), X_comps int32 [N, 11] (test length,
reference length, correct[4], guess[4] from BleuScorer's cooked statistics, LCS from my_lcs), X_bleu f64 [N, 4], X_rouge f64 [N],
X_cider f64 [N], X_corpus f64 [6] (BLEU_1..4, ROUGE_L, CIDEr as compute_scores reports them), X_df_grams int16 [K, 4] (0-padded
n-grams) with X_df_counts int32 [K] (CiderScorer.document_frequency)."""
import contextlib
import io
import os
import random
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def noisy(rng, ref, vocab):
    out = []
    for w in ref:
        u = rng.random()
        if u < 0.12:
            continue
        out.append(rng.randint(1, vocab) if u < 0.27 else w)
        if rng.random() < 0.1:
            out.append(rng.randint(1, vocab))
    return out


def corpus_a():
    rng = random.Random(20240611)
    V = 12
    rnd = lambda n: [rng.randint(1, V) for _ in range(n)]
    refs, hyps = [], []
    refs.append(rnd(9)); hyps.append([])                                   # empty hypothesis
    refs.append(rnd(7)); hyps.append([refs[-1][2]])                        # one word
    refs.append(rnd(15)); hyps.append(list(refs[-1]))                      # identical
    refs.append(rnd(6)); hyps.append(refs[-1] + rnd(11))                   # hypothesis longer than its reference
    refs.append([1, 2, 3, 1, 2]); hyps.append([1, 2, 1, 2, 1, 2, 1, 2])    # an n-gram more often than in the reference
    twin = rnd(12)
    refs.append(list(twin)); hyps.append(noisy(rng, twin, V))              # two identical references: df > 1
    refs.append(list(twin)); hyps.append(noisy(rng, twin, V))
    refs.append([]); hyps.append(rnd(5))                                   # empty reference
    refs.append(rnd(40)); hyps.append(noisy(rng, refs[-1], V)[:40])        # the longest
    while len(refs) < 24:
        r = rnd(rng.randint(1, 40))
        refs.append(r); hyps.append(noisy(rng, r, V)[:40])
    return hyps, refs


def corpus_b():
    return [[3, 1, 4, 1, 5, 9, 2, 6]], [[3, 1, 4, 1, 5, 2, 6, 5]]


def corpus_c():
    rng = random.Random(512)
    V = 12
    ref = [rng.randint(1, V) for _ in range(512)]
    hyp = [w if rng.random() < 0.8 else rng.randint(1, V) for w in ref]
    r1 = [rng.randint(1, V) for _ in range(20)]
    r2 = [rng.randint(1, V) for _ in range(33)]
    return [hyp, noisy(rng, r1, V), noisy(rng, r2, V)], [ref, r1, r2]


def record(name, hyps, refs, out):
    from pycocoevalcap.bleu.bleu import Bleu
    from pycocoevalcap.bleu.bleu_scorer import BleuScorer
    from pycocoevalcap.cider.cider import Cider
    from pycocoevalcap.cider.cider_scorer import CiderScorer
    from pycocoevalcap.rouge.rouge import Rouge, my_lcs
    N = len(refs)
    assert not any(len(h) == 0 and len(r) == 0 for h, r in zip(hyps, refs))
    text = lambda w: " ".join(str(t) for t in w)
    gts = {i: [text(r)] for i, r in enumerate(refs)}
    res = {i: [text(h)] for i, h in enumerate(hyps)}
    with contextlib.redirect_stdout(io.StringIO()):                       # Bleu asks for verbose=1
        bleu, bleus = Bleu(4).compute_score(gts, res)
    rouge, rouges = Rouge().compute_score(gts, res)
    cider, ciders = Cider().compute_score(gts, res)
    bs, cs = BleuScorer(n=4), CiderScorer(n=4, sigma=6.0)
    for i in range(N):
        bs += (res[i][0], gts[i])
        cs += (res[i][0], gts[i])
    cs.compute_doc_freq()
    comps = [[c["testlen"], c["reflen"][0]] + list(c["correct"]) + list(c["guess"]) +
             [my_lcs(gts[i][0].split(), res[i][0].split())] for i, c in enumerate(bs.ctest)]
    T = max(1, max(len(w) for w in hyps + refs))
    pad = lambda rows: np.array([w + [0] * (T - len(w)) for w in rows], dtype=np.int16)
    grams = sorted(cs.document_frequency.items())
    out[name + "_hyp"], out[name + "_ref"] = pad(hyps), pad(refs)
    out[name + "_comps"] = np.array(comps, dtype=np.int32)
    out[name + "_bleu"] = np.array(bleus, dtype=np.float64).T
    out[name + "_rouge"] = np.asarray(rouges, dtype=np.float64)
    out[name + "_cider"] = np.asarray(ciders, dtype=np.float64)
    out[name + "_corpus"] = np.array(list(bleu) + [rouge, cider], dtype=np.float64)
    out[name + "_df_grams"] = np.array([[int(t) for t in g] + [0] * (4 - len(g)) for g, _ in grams], dtype=np.int16).reshape(-1, 4)
    out[name + "_df_counts"] = np.array([int(c) for _, c in grams], dtype=np.int32)


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    sys.path.insert(0, sys.argv[1])
    out = {}
    for name, make in (("A", corpus_a), ("B", corpus_b), ("C", corpus_c)):
        record(name, *make(), out)
    path = os.path.join(HERE, "report_metrics.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
