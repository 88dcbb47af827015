"""Scoring of decoded reports on the device, in place of the host loop of ``test()`` and of ``compute_scores`` in the reference's
``run_report_generation_cxr.py`` (:274-379): BLEU-1..4, ROUGE-L and CIDEr, the R2Gen path.  METEOR and the PTB-tokenizer path
(``MVLBertEvalCap``) need Java and are not here.

The reference turns every row of ids into a string (``convert_ids_to_tokens``, ``convert_tokens_to_string``, two ``replace``
calls) and hands the strings to ``pycocoevalcap``.  Here hypotheses and references stay WordPiece ids: three flag bits per
vocabulary id (``word_flags``) say how pieces form words, ``mvlt_report_ngram_keys`` gives the document frequencies of the
reference set once, and ``mvlt_report_stats`` scores one (hypothesis, reference) pair per workgroup -- the integers behind BLEU
and ROUGE-L, and CIDEr in f64.  The per-sample scores are device tensors (``score``); ``ReportScorer`` gathers them per sample and
crosses to the host once (``result``).

What differs from the string pipeline: references enter as ids and are segmented by the same rule as the
hypotheses, so the numbers are the reference's when the ground-truth string is what the tokenizer round-trips (lower case, no
[UNK], punctuation inside a word already split); one reference per sample; a pair of two empty reports has ROUGE-L 0."""
import math

import torch

from . import ops

__all__ = ["CONT", "JOIN", "BREAK", "STOP_IDS", "word_flags", "ReferenceSet", "score", "sample_scores", "corpus_scores",
           "ReportScorer", "evaluate"]

CONT, JOIN, BREAK = 1, 2, 4
STOP_IDS = (0, 102, 104)            # [PAD], [SEP], [END] of the reference's vocabulary (test() :341)
NO_KEY = (1 << 63) - 1
TINY, SMALL = 1e-15, 1e-9           # BleuScorer.compute_score
BETA2 = 1.2 ** 2                    # Rouge.beta ** 2
KEYS = ("BLEU_1", "BLEU_2", "BLEU_3", "BLEU_4", "ROUGE_L", "CIDEr")


def word_flags(tokens):
    """uint8 [V] (host) from a vocabulary's token strings in id order: ``##...`` -> CONT, ``-`` -> JOIN, ``.`` -> BREAK."""
    return torch.tensor([CONT if t.startswith("##") else JOIN if t == "-" else BREAK if t == "." else 0 for t in tokens],
                        dtype=torch.uint8)


class ReferenceSet:
    """The N untruncated reference reports as ids on the device, with the document-frequency table of their n-grams.

    ``ref_ids``: int64 [N, Tr] or a list of id lists (padded with 0, which then has to be a stop id).  ``flags``: the table of
    ``word_flags`` or None (every id is a word).  ``df_keys`` (sorted int64) / ``df_counts`` (int32): the number of references
    that contain each n-gram, n = 1..4."""

    def __init__(self, ref_ids, flags=None, stop_ids=STOP_IDS, device="cuda"):
        self.device = torch.device(device)
        self.stop_ids = tuple(int(s) for s in stop_ids)
        if not torch.is_tensor(ref_ids):
            rows = [list(r) for r in ref_ids]
            width = max(1, max((len(r) for r in rows), default=1))
            if any(len(r) != width for r in rows) and 0 not in self.stop_ids:
                raise ValueError("ragged id lists are padded with 0: 0 must be a stop id")
            ref_ids = torch.tensor([r + [0] * (width - len(r)) for r in rows], dtype=torch.int64).reshape(len(rows), width)
        if ref_ids.dim() != 2 or ref_ids.shape[0] < 1:
            raise ValueError("ref_ids must be [N, Tr] with N >= 1")
        self.ids = ref_ids.to(self.device, torch.int64).contiguous()
        self.flags = None if flags is None else torch.as_tensor(flags, dtype=torch.uint8).to(self.device).contiguous()
        self.N = self.ids.shape[0]
        keys, self.n_words = ops.report_ngram_keys(self.ids, self.flags, self.stop_ids)
        uniq, counts = torch.unique_consecutive(keys.reshape(-1).sort().values, return_counts=True)
        if uniq.numel() and int(uniq[-1]) == NO_KEY:          # "no key" sorts last
            uniq, counts = uniq[:-1], counts[:-1]
        self.df_keys, self.df_counts = uniq.contiguous(), counts.to(torch.int32).contiguous()

    def __len__(self):
        return self.N


def sample_scores(stats):
    """(bleu f64 [B, 4], rouge_l f64 [B]) from the integer rows of ``mvlt_report_stats``, on the tensor's device.  BLEU per sample
    as ``BleuScorer.compute_score`` appends it (reflen = the one reference's length), ROUGE-L as ``Rouge.calc_score``."""
    s = stats.to(torch.float64)
    hyp_len, ref_len, lcs = s[:, 0], s[:, 1].clamp(min=0.0), s[:, 10]
    frac = (s[:, 2:6] + TINY) / (s[:, 6:10] + SMALL)
    root = torch.tensor([1.0, 1.0 / 2, 1.0 / 3, 1.0 / 4], dtype=torch.float64, device=stats.device)
    bleu = torch.cumprod(frac, dim=1) ** root
    ratio = (hyp_len + TINY) / (ref_len + SMALL)
    bleu = bleu * torch.where(ratio < 1, torch.exp(1 - 1 / ratio), torch.ones_like(ratio))[:, None]
    hit = lcs > 0                                          # P or R is 0 exactly when the LCS is empty
    p, r = lcs / hyp_len.clamp(min=1.0), lcs / ref_len.clamp(min=1.0)
    rouge = torch.where(hit, (1 + BETA2) * p * r / torch.where(hit, r + BETA2 * p, torch.ones_like(p)), torch.zeros_like(p))
    return bleu, rouge


@torch.no_grad()
def score(hyp_ids, refs, index=None):
    """Per-row scores of ``hyp_ids`` [B, T] against ``refs`` (row i against reference ``index[i]``, or reference i): device
    tensors ``stats`` int32 [B, 11] (hypothesis words, reference words, correct[4], guess[4], LCS), ``bleu`` f64 [B, 4],
    ``rouge_l`` f64 [B], ``cider`` f64 [B].  No host synchronisation."""
    hyp = torch.as_tensor(hyp_ids).to(refs.device, torch.int64)
    if hyp.dim() != 2:
        raise ValueError("hyp_ids must be [B, T]")
    if hyp.stride(1) != 1:
        hyp = hyp.contiguous()
    if index is not None:
        index = torch.as_tensor(index).to(refs.device, torch.int32).contiguous()
    stats, cider = ops.report_stats(hyp, refs.ids, index, refs.flags, refs.stop_ids, refs.df_keys, refs.df_counts)
    bleu, rouge = sample_scores(stats)
    return {"stats": stats, "bleu": bleu, "rouge_l": rouge, "cider": cider}


def _pack(stats, rouge_l, cider, n_bad):
    """f64 [13]: the int64 column sums of hypothesis words, reference words, correct[4], guess[4] (exact in f64: far below 2^53),
    the two score sums and the count of samples that are not covered exactly once."""
    sums = stats[:, :10].to(torch.int64).sum(dim=0).to(torch.float64)
    return torch.cat([sums, rouge_l.sum().reshape(1), cider.sum().reshape(1), n_bad.to(torch.float64).reshape(1)])


def _finish(v, n):
    if v[12] != 0:
        raise RuntimeError(f"{int(v[12])} of {n} samples were added twice, never, or under an index outside the reference set")
    hyp_len, ref_len, correct, guess = v[0], v[1], v[2:6], v[6:10]
    out, bleu = {}, 1.0
    ratio = (hyp_len + TINY) / (ref_len + SMALL)
    for k in range(4):
        bleu *= (correct[k] + TINY) / (guess[k] + SMALL)
        out[KEYS[k]] = bleu ** (1.0 / (k + 1)) * (math.exp(1 - 1 / ratio) if ratio < 1 else 1.0)
    out["ROUGE_L"], out["CIDEr"] = v[10] / n, v[11] / n
    return out


def corpus_scores(stats, rouge_l, cider):
    """The dict of ``compute_scores`` from one row per sample: corpus BLEU from the summed integers (``BleuScorer.compute_score``
    over the whole set), the means of ROUGE-L and CIDEr.  One copy to the host."""
    zero = torch.zeros((), dtype=torch.int64, device=stats.device)
    return _finish(_pack(stats, rouge_l, cider, zero).cpu().tolist(), stats.shape[0])


class ReportScorer:
    """Collects the scores of a test set batch by batch in [N, ...] device buffers; ``result()`` is the only host copy."""

    def __init__(self, refs):
        self.refs = refs
        N, dev = refs.N, refs.device
        self.stats = torch.zeros((N, 11), dtype=torch.int32, device=dev)
        self.bleu = torch.zeros((N, 4), dtype=torch.float64, device=dev)
        self.rouge_l = torch.zeros(N, dtype=torch.float64, device=dev)
        self.cider = torch.zeros(N, dtype=torch.float64, device=dev)
        self.visits = torch.zeros(N, dtype=torch.int32, device=dev)
        self.outside = torch.zeros((), dtype=torch.int64, device=dev)

    @torch.no_grad()
    def add(self, hyp_ids, index):
        """Score the batch's rows against references ``index`` (one sample id per row) and store them under those ids."""
        idx = torch.as_tensor(index).to(self.refs.device, torch.int64).reshape(-1)
        out = score(hyp_ids, self.refs, idx)
        ok = (idx >= 0) & (idx < self.refs.N)
        slot = idx.clamp(0, self.refs.N - 1)
        self.visits.index_add_(0, slot, ok.to(torch.int32))
        self.outside += (~ok).sum()
        for buf, new in ((self.stats, out["stats"]), (self.bleu, out["bleu"]), (self.rouge_l, out["rouge_l"]),
                         (self.cider, out["cider"])):
            keep = ok if new.dim() == 1 else ok[:, None]
            buf.index_copy_(0, slot, torch.where(keep, new, buf[slot]))      # a row outside the set rewrites what is there
        return out

    def result(self):
        """{"BLEU_1" .. "BLEU_4", "ROUGE_L", "CIDEr"}; raises when a sample was added twice or never."""
        n_bad = (self.visits != 1).sum() + self.outside
        return _finish(_pack(self.stats, self.rouge_l, self.cider, n_bad).cpu().tolist(), self.refs.N)


@torch.no_grad()
def evaluate(model, batches, refs, num_beams=1, **generate_options):
    """Decode and score a test set: ``batches`` yields ``(image, caption_ids)`` in sample order (``CaptionBatches(split='test')``),
    every batch goes through ``model.generate(image, num_beams=num_beams, **generate_options)`` and its sequences are scored
    against the next rows of ``refs``.  Returns ``ReportScorer.result()``; the loop itself never reads back."""
    scorer = ReportScorer(refs)
    start = 0
    for batch in batches:
        out = model.generate(batch[0], num_beams=num_beams, **generate_options)
        seq = out if torch.is_tensor(out) else out[0]
        n = seq.shape[0]
        scorer.add(seq, torch.arange(start, start + n, dtype=torch.int64, device=refs.device))
        start += n
    return scorer.result()
