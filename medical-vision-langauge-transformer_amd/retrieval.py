"""Retrieval evaluation on the device, in place of ``testRetrieval`` + ``compute_ranks`` + ``evaluate`` of the reference's
``run_retrieval.py`` (:192-296).

The reference scores an N x N test set pair by pair: every pair carries its own image through the Swin tower, every probability
crosses to the host with ``.item()`` and the ranks come from Python loops over ``np.argsort``.  Here the image tower runs once
per image (``MVLBertForRetrieval.encode_images``), the single-stream encoder -- which has to run per pair -- runs over chunks of
pairs on packed rows (``score_pairs``), each chunk's probabilities go straight into the score matrix on the device (with
``MVLT_RETRIEVAL_HEAD=1`` from inside the one-launch scoring head ``mvlt_retrieval_head``), and the ranks and recall counts are
computed from that matrix on the device (``mvlt_recall_ranks``, ``mvlt_recall_counts``): one copy of ``2 * len(ks)`` integers
to the host at the end.

Rank rule (the reference's ``np.argsort(sim)[::-1]`` leaves ties to an unstable sort; bf16 scores do tie): the stable ascending
sort reversed -- among equal scores the higher index comes first; NaN counts as smaller than every number.  The rank of a line
is the number of entries that sort before its best match, or the line's length when it has no match."""
import torch

from . import ops

__all__ = ["score_all_pairs", "recall_ranks", "evaluate"]


@torch.no_grad()
def score_all_pairs(model, images, captions, *, pair_chunk=512, image_chunk=64, out=None):
    """f32 [Ni, Nc] on the device: scores[i, j] = the class-1 probability ``model(images[i:i+1], captions[j:j+1])[0, 1]``.
    images [Ni, 3, S, S] on the host or the device, captions int64 [Nc, T].  Pairs are walked image-major in chunks of
    ``pair_chunk``; no chunk synchronises with the host.  ``out``: a contiguous f32 [Ni, Nc] device tensor to fill."""
    if model.training:
        raise ValueError("score_all_pairs needs model.eval(): dropout would make a pair's score depend on the chunk it is scored in")
    dev = next(model.parameters()).device
    captions = captions.to(dev, non_blocking=True).to(torch.int64).contiguous()
    Ni, Nc = images.shape[0], captions.shape[0]
    features = model.encode_images(images, image_chunk=image_chunk)
    if out is None:
        out = torch.empty((Ni, Nc), dtype=torch.float32, device=dev)
    if out.shape != (Ni, Nc) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != dev:
        raise ValueError("out must be a contiguous float32 [Ni, Nc] tensor on the model's device")
    total = Ni * Nc
    flat = torch.arange(total, dtype=torch.int64, device=dev)
    ii = torch.div(flat, Nc, rounding_mode="floor")
    jj = flat - ii * Nc
    for p0 in range(0, total, int(pair_chunk)):
        p1 = min(total, p0 + int(pair_chunk))
        model.score_pairs(features, captions, ii[p0:p1], jj[p0:p1], out=out, out_index=flat[p0:p1])
    model.check_device_errors()
    return out


def recall_ranks(scores, image_group, caption_group):
    """(i2t_rank int32 [Ni], t2i_rank int32 [Nc]) on the device.  Pair (i, j) is a match exactly when
    ``image_group[i] == caption_group[j]`` (int64 ids, the reference's ``cap_id``); see the module docstring for the order."""
    dev = scores.device
    ig = torch.as_tensor(image_group, dtype=torch.int64).to(dev).contiguous()
    cg = torch.as_tensor(caption_group, dtype=torch.int64).to(dev).contiguous()
    if scores.dim() != 2 or ig.numel() != scores.shape[0] or cg.numel() != scores.shape[1]:
        raise ValueError("scores must be [Ni, Nc] with one group id per image and per caption")
    s = scores if (scores.dtype == torch.float32 and scores.stride(1) == 1) else scores.float().contiguous()
    return ops.recall_ranks(s, ig, cg)


def evaluate(scores, image_group, caption_group, ks=(1, 5, 10)):
    """{"i2t_retrieval": {"R@1": ..}, "t2i_retrieval": {..}}: the fraction of images (captions) whose best match ranks
    below k, as the reference's ``evaluate`` reports it.  The counts are reduced on the device and cross to the host once."""
    i2t, t2i = recall_ranks(scores, image_group, caption_group)
    ks = [int(k) for k in ks]
    counts = torch.empty(2 * len(ks), dtype=torch.int32, device=scores.device)
    ops.recall_counts(i2t, ks, out=counts[:len(ks)])
    ops.recall_counts(t2i, ks, out=counts[len(ks):])
    c = counts.cpu().tolist()
    return {"i2t_retrieval": {f"R@{k}": c[n] / i2t.numel() for n, k in enumerate(ks)},
            "t2i_retrieval": {f"R@{k}": c[len(ks) + n] / t2i.numel() for n, k in enumerate(ks)}}
