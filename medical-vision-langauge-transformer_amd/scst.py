"""Self-critical sequence training (Rennie et al. 2017) of the report generator on the device: the ``--scst`` path the reference's
``run_report_generation.py`` (:315-361) leaves commented out -- decode greedily, sample, reward the sample with its metric minus
the greedy row's, and weight the sampled tokens' log-probabilities with that advantage.

Everything is device work on the pieces the project already has: both decodes are ``decode.greedy_search`` on ONE pass of the
image tower, both id tensors are scored by ``report_metrics.score`` (no strings, no host loop that cuts rows at [END]), and the
loss is ``MVLBertForImageCaption.sequence_loss_from_features`` (mvlt_seq_loss_plan -> teacher-forced encoder -> fused MLM head ->
mvlt_seq_loss_fwd, backward through mvlt_ce_bwd_weighted): logits never reach torch and nothing is read back."""
import torch

from . import decode, ops, report_metrics
from .arena import Arena
from .runtime import compute_dtype_of

__all__ = ["METRICS", "BASELINES", "advantages", "self_critical_loss"]

METRICS = ("cider", "bleu4", "rouge_l")
BASELINES = ("greedy", "mean")


def _metric(scores, metric):
    return scores["bleu"][:, 3] if metric == "bleu4" else scores[metric]


def advantages(reward_sample, reward_greedy=None, baseline='greedy'):
    """f32 [B, K] advantages of the K samples of every image from their f64 rewards ``reward_sample`` [B, K], detached; works
    on CPU and device tensors alike.  ``baseline='greedy'``: ``r[b, k] - reward_greedy[b]`` (f64 [B]).  ``baseline='mean'``: the
    leave-one-out mean of the image's other samples, ``r[b, k] - (sum_j r[b, j] - r[b, k]) / (K - 1)`` (K >= 2; the rows sum to 0
    up to f64 rounding).  The arithmetic is f64, the cast to f32 comes last."""
    if baseline not in BASELINES:
        raise ValueError(f"baseline {baseline!r}: one of {BASELINES}")
    r = reward_sample.detach().to(torch.float64)
    if r.dim() != 2:
        raise ValueError("reward_sample must be [B, K]")
    if baseline == 'greedy':
        if reward_greedy is None or tuple(reward_greedy.shape) != (r.shape[0],):
            raise ValueError("the greedy baseline needs reward_greedy [B]")
        return (r - reward_greedy.detach().to(torch.float64)[:, None]).to(torch.float32)
    K = r.shape[1]
    if K < 2:
        raise ValueError("baseline='mean' is the mean reward of the OTHER samples of an image: it needs num_samples >= 2")
    return (r - (r.sum(1, keepdim=True) - r) / (K - 1)).to(torch.float32)


def self_critical_loss(model, image, refs, index, seed=None, temperature=1.0, top_k=0, top_p=1.0, metric='cider', max_length=None,
                       learning_strategy='unilm', num_samples=1, baseline='greedy', one_pass=None, **logit_rules):
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
    ``reward_greedy`` (f64 [B]), ``advantage`` (f32 [B]).  Nothing is read back to the host.

    Several samples per image.  ``num_samples=K`` draws K samples per image and ``baseline`` names what their reward is
    measured against (``advantages``): 'greedy', the greedy row's reward, or 'mean', the mean reward of the image's OTHER samples
    (K >= 2; no greedy row is decoded).  ``one_pass`` (None: True exactly when K > 1 or baseline == 'mean') decodes the greedy row
    and the samples of every image in ONE pass over B * (K + greedy) rows (``decode.sample_many``) in place of one decode after
    the other; it has no ``top_k`` / ``top_p`` (ValueError).  The default call (K = 1, 'greedy', one_pass None) is the two decodes
    described above, unchanged.  The loss is one ``sequence_loss_from_features`` call over the B * K sampled rows on
    ``feature.repeat_interleave(K, 0)`` -- autograd sums the K gradients back into the image tower -- and the rewards one
    ``report_metrics.score`` call per id tensor, with ``index`` repeated; B * K must stay within ``ops.SEQ_LOSS_MAX_B``.
    With K > 1 ``info`` holds ``sample_ids`` [B, K, n], ``reward_sample`` and ``advantage`` [B, K], and ``greedy_ids`` [B, n] /
    ``reward_greedy`` [B] only with the greedy baseline; with K = 1 the shapes above on either path.
    In training mode the ONE step 0 of a one-pass decode means the greedy row and the samples of an image share one dropout mask
    on the prefix, where the two decodes of the default path each have their own."""
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
    if baseline not in BASELINES:
        raise ValueError(f"baseline {baseline!r}: one of {BASELINES}")
    if int(num_samples) != num_samples or num_samples < 1:
        raise ValueError("num_samples must be a positive integer")
    K = int(num_samples)
    if baseline == 'mean' and K < 2:
        raise ValueError("baseline='mean' is the mean reward of the OTHER samples of an image: it needs num_samples >= 2")
    if one_pass is None:
        one_pass = K > 1 or baseline == 'mean'
    if not one_pass and (K > 1 or baseline == 'mean'):
        raise ValueError("num_samples > 1 and baseline='mean' decode in one pass: one_pass=False is the two decodes of one sample")
    if one_pass:
        k_, p_ = ops.check_sample_filter(top_k, top_p)
        if k_ != 0 or p_ < 1.0:
            raise ValueError("the one-pass decode has no top_k / top_p filter")
        if image.shape[0] * K > ops.SEQ_LOSS_MAX_B:
            raise ValueError(f"{image.shape[0]} images x {K} samples: the loss takes at most {ops.SEQ_LOSS_MAX_B} sequences")
    Arena.of(model, compute_dtype_of(model))
    feature = model.conv(image)
    if one_pass:
        return _one_pass_loss(model, feature, refs, index, seed, temperature, metric, max_length, K, baseline, logit_rules)
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


def _one_pass_loss(model, feature, refs, index, seed, temperature, metric, max_length, K, baseline, logit_rules):
    """self_critical_loss over one ``decode.sample_many`` pass: K samples per image (and the greedy row with that baseline)."""
    B = feature.shape[0]
    greedy = baseline == 'greedy'
    with torch.no_grad():
        ids, _ = decode.sample_many(model, feature.detach(), K, include_greedy=greedy, seed=seed, temperature=temperature,
                                    max_length=max_length, **logit_rules)
        n = ids.shape[2]
        sample_ids = ids[:, int(greedy):].contiguous()          # [B, K, n]
        idx = torch.arange(B, device=feature.device) if index is None else torch.as_tensor(index).reshape(-1)
        reward_sample = _metric(report_metrics.score(sample_ids.view(B * K, n), refs, idx.repeat_interleave(K)), metric).view(B, K)
        info = {}
        reward_greedy = None
        if greedy:
            greedy_ids = ids[:, 0].contiguous()
            reward_greedy = _metric(report_metrics.score(greedy_ids, refs, index), metric)
            info.update(greedy_ids=greedy_ids, reward_greedy=reward_greedy)
        advantage = advantages(reward_sample, reward_greedy, baseline)
    loss = model.sequence_loss_from_features(feature.repeat_interleave(K, 0), sample_ids.view(B * K, n), advantage.reshape(-1))
    if K == 1:          # the shapes of the two-decode path
        sample_ids, reward_sample, advantage = sample_ids[:, 0], reward_sample[:, 0], advantage[:, 0]
    info.update(sample_ids=sample_ids, reward_sample=reward_sample, advantage=advantage)
    return loss, info
