"""Plain restatement of the three logit rules of constrained decoding (HF RepetitionPenaltyLogitsProcessor,
NoRepeatNGramLogitsProcessor, MinLengthLogitsProcessor) as include/mvlt_hip.h words them, on a [rows, V] tensor plus a history.

    c = history.shape[1] tokens generated so far, h = history[m] exactly as stored (PAD of a finished row included)
    seen(n)     n occurs in h:  x' = x < 0 ? x * penalty : x / penalty, once however often n occurs
    banned(n)   g = ngram >= 1 and c + 1 >= g: some i <= c - g has h[i .. i+g-2] == h[c-g+1 .. c-1] and h[i+g-1] == n
                eos given and c < min_length: n == eos
    a banned column is -inf after `process` and takes part in nothing

`bitmaps` packs the two sets the way the device plan does (bit n & 31 of uint32 word n >> 5, stored as int32 bit patterns);
`processed` turns a sample_ref.sample_ref result into the reference of a rule-aware pick with per-element bounds:
a penalised column carries e_x max(p, 1 / p) + 2^-24 |x'| (the logit's own bound scaled, plus the one extra f32 rounding).
`bounded_history` / `RULE_SETS` are the inputs the GPU test and the CPU near-tie count share."""
import math

import torch

import sample_ref as S
from gemm_ref import U32

RULE_SETS = [(1.3, 0, 0), (1.0, 2, 0), (2.0, 3, 20), (1.0, 1, 0)]          # (penalty, ngram, min_length) of the bounded tests
EOS = 5                                                                    # eos of the head-level tests (banned while c < min_length)


def sets(history, V, ngram=0, min_length=0, eos=None):
    """history: int64 [rows, c] -> (seen, banned) bool [rows, V].  Ids outside [0, V) set nothing."""
    rows, c = history.shape
    seen = torch.zeros((rows, V), dtype=torch.bool)
    banned = torch.zeros((rows, V), dtype=torch.bool)
    for m in range(rows):
        h = history[m].tolist()
        for t in h:
            if 0 <= t < V:
                seen[m, t] = True
        g = ngram
        if g >= 1 and c + 1 >= g:
            last = h[c - g + 1:c] if g > 1 else []
            for i in range(0, c - g + 1):
                if h[i:i + g - 1] == last and 0 <= h[i + g - 1] < V:
                    banned[m, h[i + g - 1]] = True
        if eos is not None and c < min_length and 0 <= eos < V:
            banned[m, eos] = True
    return seen, banned


def process(x, history, penalty=1.0, ngram=0, min_length=0, eos=None):
    """x: float [rows, V] (the arithmetic runs in x's dtype) -> the processed logits, -inf in banned columns."""
    seen, banned = sets(history, x.shape[1], ngram, min_length, eos)
    out = torch.where(seen, torch.where(x < 0, x * penalty, x / penalty), x)
    return torch.where(banned, torch.full_like(out, -math.inf), out)


def bitmaps(history, V, ngram=0, min_length=0, eos=None):
    """(seen, banned) as int32 [rows, ceil(V / 32)] bit patterns, the layout of MvltLogitRules."""
    nw = (V + 31) // 32
    out = []
    for s in sets(history, V, ngram, min_length, eos):
        pad = torch.zeros((s.shape[0], nw * 32), dtype=torch.int64)
        pad[:, :V] = s.long()
        words = (pad.view(-1, nw, 32) << torch.arange(32, dtype=torch.int64)).sum(-1)          # < 2^32
        out.append(torch.where(words >= 2 ** 31, words - 2 ** 32, words).to(torch.int32))
    return out


def processed(base, history, penalty, ngram, min_length, eos, seed, tag, row0=0):
    """base: a sample_ref.sample_ref result at temperature 1 (not changed).  Returns the same kind of dict for the processed
    logits: x (-inf where banned), e_x, y, bound_y, tok (sampled), gtok (greedy), banned, bound_lp."""
    x0, e0 = base["x"], base["e_x"]
    M, N = x0.shape
    seen, banned = sets(history, N, ngram, min_length, eos)
    x = process(x0, history, penalty, ngram, min_length, eos)
    fin = torch.where(banned, torch.zeros_like(x), x)
    e_x = torch.where(seen, e0 * max(penalty, 1.0 / penalty) + U32 * fin.abs(), e0)
    g = S.gumbel_ref(S.u01_ref(seed, tag, row0 + M, N)[row0:])
    y = x + g
    bound_y = S.SAFETY * (e_x + S.e_g(g) + U32 * torch.where(banned, torch.zeros_like(y), y).abs())
    lse = torch.logsumexp(x, 1)
    e_max = torch.where(banned, torch.zeros_like(e_x), e_x).max(1).values
    e_lse = S.LSE_SUM * U32 + S.E_LOG * (lse - x.max(1).values).abs() + U32 * lse.abs()

    def bound_lp(t):
        xt = fin.gather(1, t.view(-1, 1)).squeeze(1)
        return S.SAFETY * (e_x.gather(1, t.view(-1, 1)).squeeze(1) + e_max + e_lse + U32 * (xt - lse).abs())

    return dict(x=x, e_x=e_x, g=g, y=y, bound_y=bound_y, bound_x=S.SAFETY * e_x, tok=y.argmax(1), gtok=x.argmax(1), lse=lse,
                banned=banned, seen=seen, bound_lp=bound_lp)


def bounded_history(base, seed=11):
    """The 12-token history of the bounded head tests, per row [q, a, q, s, z, q, a, z, q, s, z, q] with a = the row's own
    unprocessed argmax, s = its unprocessed sampled token and q, z two other tokens: a and s are seen (penalised), follow q
    (banned at g = 2) and follow (z, q) (banned at g = 3), so every rule set bears on the picks the row would make without it."""
    x, M, N = base["x"], base["x"].shape[0], base["x"].shape[1]
    a, s = x.argmax(1), base["tok"]
    gen = torch.Generator().manual_seed(seed)
    rows = []
    for m in range(M):
        while True:
            q, z = (int(v) for v in torch.randint(0, N, (2,), generator=gen))
            if len({q, z, int(a[m]), int(s[m]), EOS}) == 5 or (int(a[m]) == int(s[m]) and len({q, z, int(a[m]), EOS}) == 4):
                break
        am, sm = int(a[m]), int(s[m])
        rows.append([q, am, q, sm, z, q, am, z, q, sm, z, q])
    return torch.tensor(rows, dtype=torch.int64)


def at_risk(ref, which):
    """Rows whose reference pick is itself a near-tie: the top two of `which` ('x' greedy with bound_x, 'y' sampled with bound_y)
    lie within the sum of their bounds."""
    v, b = ref[which], ref["bound_x" if which == "x" else "bound_y"]
    top = torch.topk(v, 2, dim=1)
    gap = top.values[:, 0] - top.values[:, 1]
    return int((gap <= b.gather(1, top.indices).sum(1)).sum())
