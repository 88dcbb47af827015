"""The report metrics restated on exact tuples (no hashing), for tests/test_report_metrics_cpu.py and
tests/test_report_metrics_gpu.py: the word segmentation rule of include/mvlt_hip.h, the string pipeline it stands for, the
integers and scores of mvlt_report_stats in Python floats (f64), and the key function of the kernels in Python integers.

A word is a tuple of piece ids, an n-gram a tuple of words.  Formulas: BleuScorer.compute_score, Rouge.calc_score and
CiderScorer.compute_cider of pycocoevalcap with one reference per sample; tests/golden/report_metrics.npz holds what those
classes themselves returned (tests/golden/make_report_metrics_golden.py)."""
import math
from collections import Counter

CONT, JOIN, BREAK = 1, 2, 4
STOP_IDS = (0, 102, 104)
TINY, SMALL, BETA2, SIGMA = 1e-15, 1e-9, 1.2 ** 2, 6.0
KEYS = ("BLEU_1", "BLEU_2", "BLEU_3", "BLEU_4", "ROUGE_L", "CIDEr")
M64 = (1 << 64) - 1
NO_KEY = (1 << 63) - 1


# ------------------------------------------------------------------------------------------------ segmentation
def cut(ids, stop_ids=STOP_IDS):
    out = []
    for t in ids:
        if int(t) in stop_ids:
            break
        out.append(int(t))
    return out


def segment(ids, flags=None, stop_ids=STOP_IDS):
    """The words of a row of ids: a list of tuples of piece ids.  flags: a sequence indexed by id, or None (every id a word);
    an id outside it has flags 0."""
    pieces = cut(ids, stop_ids)
    n = len(pieces)
    fl = [int(flags[p]) if flags is not None and 0 <= p < len(flags) else 0 for p in pieces]
    words, was_right = [], False
    for i, p in enumerate(pieces):
        f = fl[i]
        glue = bool(f & JOIN) and 0 < i < n - 1 and not was_right and not (fl[i + 1] & CONT)
        if i == 0 or f & BREAK:
            start = True
        elif f & CONT or was_right or glue:
            start = False
        else:
            start = True
        if start:
            words.append([p])
        else:
            words[-1].append(p)
        was_right = glue
    return [tuple(w) for w in words]


def string_pipeline(tokens):
    """The words the reference scores for a list of token strings (stop tokens already cut): convert_tokens_to_string, then
    test() :346 and compute_scores :290-291, then the scorers' split()."""
    return " ".join(tokens).replace(" ##", "").strip().replace(" - ", "-").replace(".", " .").split()


def render(word, tokens):
    """A word of segment() as the string the pipeline makes of it."""
    return "".join(tokens[p][2:] if tokens[p].startswith("##") else tokens[p] for p in word)


# ------------------------------------------------------------------------------------------------ counts and scores
def ngrams(words, n):
    return Counter(tuple(words[i:i + n]) for i in range(len(words) - n + 1))


def lcs(a, b):
    prev = [0] * (len(b) + 1)
    for x in a:
        cur = [0]
        for j, y in enumerate(b):
            cur.append(prev[j] + 1 if x == y else max(prev[j + 1], cur[j]))
        prev = cur
    return prev[-1]


def doc_freq(refs):
    """{n-gram: number of references that contain it} over lists of words (compute_doc_freq)."""
    df = Counter()
    for words in refs:
        for n in range(1, 5):
            df.update(ngrams(words, n).keys())
    return df


def pair_stats(h, r):
    """The 11 integers of mvlt_report_stats for two lists of words."""
    correct, guess = [], []
    for n in range(1, 5):
        ch, cr = ngrams(h, n), ngrams(r, n)
        correct.append(sum(min(c, cr.get(g, 0)) for g, c in ch.items()))
        guess.append(max(0, len(h) - n + 1))
    return [len(h), len(r)] + correct + guess + [lcs(h, r)]


def cider(h, r, df, N):
    log_n = math.log(float(N))
    delta = float(max(0, len(h) - 1) - max(0, len(r) - 1))
    total = 0.0
    for n in range(1, 5):
        vh = {g: c * (log_n - math.log(max(1.0, df.get(g, 0)))) for g, c in ngrams(h, n).items()}
        vr = {g: c * (log_n - math.log(max(1.0, df.get(g, 0)))) for g, c in ngrams(r, n).items()}
        val = sum(min(v, vr.get(g, 0.0)) * vr.get(g, 0.0) for g, v in vh.items())
        nh, nr = math.sqrt(sum(v * v for v in vh.values())), math.sqrt(sum(v * v for v in vr.values()))
        if nh != 0 and nr != 0:
            val /= nh * nr
        total += val * math.exp(-(delta ** 2) / (2 * SIGMA ** 2))
    return total / 4 * 10.0


def bleu_from(hyp_len, ref_len, correct, guess):
    out, b = [], 1.0
    ratio = (hyp_len + TINY) / (ref_len + SMALL)
    for k in range(4):
        b *= (float(correct[k]) + TINY) / (float(guess[k]) + SMALL)
        out.append(b ** (1.0 / (k + 1)) * (math.exp(1 - 1 / ratio) if ratio < 1 else 1.0))
    return out


def rouge_from(hyp_len, ref_len, lcs_len):
    if lcs_len == 0 or hyp_len == 0 or ref_len == 0:
        return 0.0
    p, r = lcs_len / float(hyp_len), lcs_len / float(ref_len)
    return ((1 + BETA2) * p * r) / float(r + BETA2 * p)


def score_corpus(hyps, refs):
    """hyps, refs: lists of lists of words, pair i against pair i.  -> dict(stats [N][11], bleu [N][4], rouge [N], cider [N],
    corpus {BLEU_1 ..: float}, df Counter)."""
    N = len(refs)
    df = doc_freq(refs)
    stats = [pair_stats(h, r) for h, r in zip(hyps, refs)]
    out = {"stats": stats, "df": df,
           "bleu": [bleu_from(s[0], s[1], s[2:6], s[6:10]) for s in stats],
           "rouge": [rouge_from(s[0], s[1], s[10]) for s in stats],
           "cider": [cider(h, r, df, N) for h, r in zip(hyps, refs)]}
    col = [sum(s[c] for s in stats) for c in range(10)]
    corpus = dict(zip(KEYS[:4], bleu_from(col[0], col[1], col[2:6], col[6:10])))
    corpus["ROUGE_L"] = sum(out["rouge"]) / N
    corpus["CIDEr"] = sum(out["cider"]) / N
    out["corpus"] = corpus
    return out


# ------------------------------------------------------------------------------------------------ the kernels' keys
def mix64(x):
    x &= M64
    x ^= x >> 30
    x = (x * 0xBF58476D1CE4E5B9) & M64
    x ^= x >> 27
    x = (x * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def fold(h, v):
    return mix64(h + 0x9E3779B97F4A7C15 + (v & M64))


def word_key(word):
    h = 0x243F6A8885A308D3
    for p in word:
        h = fold(h, p)
    return h


def gram_key(gram):
    """The int64 the kernels store for an n-gram (a tuple of words)."""
    h = 0x13198A2E03707344 + len(gram)
    for w in gram:
        h = fold(h, word_key(w))
    k = h - (1 << 64) if h >> 63 else h
    return NO_KEY - 1 if k == NO_KEY else k


def df_table(df):
    """(sorted keys, counts in that order) of a doc_freq() result, as ReferenceSet holds them."""
    pairs = sorted((gram_key(g), c) for g, c in df.items())
    return [k for k, _ in pairs], [c for _, c in pairs]


# ------------------------------------------------------------------------------------------------ golden fixture access
def golden_corpus(z, name):
    """(hyps, refs) as lists of lists of one-piece words from the padded id arrays of the fixture (0 pads)."""
    rows = lambda a: [[(int(t),) for t in row if t != 0] for row in a]
    return rows(z[name + "_hyp"]), rows(z[name + "_ref"])
