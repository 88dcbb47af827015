"""Self-critical sequence training (Rennie et al. 2017) of the report generator on the device: the ``--scst`` path the reference's
``run_report_generation.py`` (:315-361) leaves commented out -- decode greedily, sample, reward the sample with its metric minus
the greedy row's, and weight the sampled tokens' log-probabilities with that advantage.

Everything is device work on the pieces the project already has: both decodes are ``decode.greedy_search`` on ONE pass of the
image tower, both id tensors are scored by ``report_metrics.score`` (no strings, no host loop that cuts rows at [END]), and the
loss is ``MVLBertForImageCaption.sequence_loss_from_features`` (mvlt_seq_loss_plan -> teacher-forced encoder -> fused MLM head ->
mvlt_seq_loss_fwd, backward through mvlt_ce_bwd_weighted): logits never reach torch and nothing is read back."""
import torch

from . import decode, report_metrics
from .arena import Arena
from .runtime import compute_dtype_of

__all__ = ["METRICS", "self_critical_loss"]

METRICS = ("cider", "bleu4", "rouge_l")


def _metric(scores, metric):
    return scores["bleu"][:, 3] if metric == "bleu4" else scores[metric]


def self_critical_loss(model, image, refs, index, seed=None, temperature=1.0, top_k=0, top_p=1.0, metric='cider', max_length=None,
                       learning_strategy='unilm', **logit_rules):
    """One self-critical step's loss: ``(loss, info)``.

    ``refs``: a ``report_metrics.ReferenceSet``; ``index``: the reference of every image (int [B], or None: image i against
    reference i).  ``seed`` / ``temperature`` / ``top_k`` / ``top_p``: the sampled decode's options (``decode.greedy_search``);
    ``metric``: 'cider', 'bleu4' or 'rouge_l'; ``logit_rules``: ``repetition_penalty`` / ``no_repeat_ngram_size`` /
    ``min_length``, applied to both decodes.  ``learning_strategy='normal'`` raises NotImplementedError as the decode does
    (``sequence_loss`` itself takes both strategies).

    The image tower runs once, with autograd.  The greedy and the sampled decode read its output under ``no_grad``; the
    advantage ``metric(sample) - metric(greedy)`` is cast to f32 and carries no gradient; the loss is
    ``model.sequence_loss_from_features(feature, sample_ids, advantage)``, i.e. ``-sum advantage_b log p(sample tokens) / N``
    over the sampled rows up to and including their [END].

    Dropout.  The image tower and the teacher-forced pass follow ``model.training`` (DropPath in Swin, hidden and attention
    dropout in the encoder).  The decode loops are not all dropout-free in training mode: their step 0 -- the full pass over
    [CLS] image [SEP] [MASK] that fills the KV cache -- is the encoder's ordinary forward and applies hidden and attention
    dropout when ``model.training`` (each decode with a seed of its own), while every cached step after it applies none.  So in
    training mode the greedy baseline is the argmax under one dropout mask on the prefix; put the model in eval mode around
    the call for a dropout-free baseline.

    ``info``: device tensors only -- ``sample_ids``, ``greedy_ids`` (int64 [B, <= max_length]), ``reward_sample``,
    ``reward_greedy`` (f64 [B]), ``advantage`` (f32 [B]).  Nothing is read back to the host."""
    if metric not in METRICS:
        raise ValueError(f"metric {metric!r}: one of {METRICS}")
    unknown = set(logit_rules) - {"repetition_penalty", "no_repeat_ngram_size", "min_length"}
    if unknown:
        raise ValueError(f"unknown options {sorted(unknown)}: the logit rules are repetition_penalty, no_repeat_ngram_size, min_length")
    if learning_strategy != 'unilm':
        raise NotImplementedError("only learning_strategy='unilm' is coherent with the KV cache (SURVEY.md 3.3)")
    if not isinstance(refs, report_metrics.ReferenceSet):
        raise ValueError("refs must be a report_metrics.ReferenceSet")
    if index is not None and len(index) != image.shape[0]:
        raise ValueError(f"index names {len(index)} references for {image.shape[0]} images")
    Arena.of(model, compute_dtype_of(model))
    feature = model.conv(image)
    with torch.no_grad():
        detached = feature.detach()
        greedy_ids, _ = decode.greedy_search(model, detached, learning_strategy=learning_strategy, max_length=max_length,
                                             **logit_rules)
        sample_ids, _ = decode.greedy_search(model, detached, learning_strategy=learning_strategy, sample_mode='sample',
                                             max_length=max_length, seed=seed, temperature=temperature, top_k=top_k, top_p=top_p,
                                             **logit_rules)
        reward_greedy = _metric(report_metrics.score(greedy_ids, refs, index), metric)
        reward_sample = _metric(report_metrics.score(sample_ids, refs, index), metric)
        advantage = (reward_sample - reward_greedy).to(torch.float32).detach()
    loss = model.sequence_loss_from_features(feature, sample_ids, advantage)
    return loss, {"sample_ids": sample_ids, "greedy_ids": greedy_ids, "reward_sample": reward_sample,
                  "reward_greedy": reward_greedy, "advantage": advantage}
