"""Cross-modal attention maps: which positions of the single stream ``[CLS] img * n_img [SEP] text * T`` (model.py:110-160)
a selection names, and the image-token axis of a map as a grid.

The maps themselves come from ``MVLBert.attention_maps`` (bert.py) and the ``attention_maps`` methods of the task models
(model.py): the probabilities of HF ``output_attentions`` (modeling_bert.py:130), recomputed by ``mvlt_attn_probs`` from the
qkv / lse each layer's forward keeps.  This module is host logic only."""
import math
import operator

SELECTIONS = ('cls', 'image', 'sep', 'text', 'all')


def resolve_range(sel, n_img, T):
    """(start, count) of a query / key selection in a sequence of n_img image tokens and T text tokens: one of SELECTIONS or an
    explicit (start, count) pair.  Every selection is one contiguous range.  ValueError for an unknown name, an empty
    selection ('text' with T == 0, 'image' with n_img == 0) or a pair that leaves [0, n_img + 2 + T)."""
    n_img, T = int(n_img), int(T)
    if n_img < 0 or T < 0:
        raise ValueError(f"n_img = {n_img}, T = {T}: counts cannot be negative")
    L = n_img + 2 + T
    if isinstance(sel, str):
        named = {'cls': (0, 1), 'image': (1, n_img), 'sep': (n_img + 1, 1), 'text': (n_img + 2, T), 'all': (0, L)}
        if sel not in named:
            raise ValueError(f"unknown selection {sel!r}: one of {SELECTIONS} or a (start, count) pair")
        start, count = named[sel]
        if count < 1:
            raise ValueError(f"selection {sel!r} is empty (n_img = {n_img}, T = {T})")
        return start, count
    try:
        start, count = sel
        if isinstance(start, bool) or isinstance(count, bool):
            raise TypeError
        start, count = operator.index(start), operator.index(count)
    except (TypeError, ValueError):
        raise ValueError(f"a selection is one of {SELECTIONS} or a (start, count) pair of ints, not {sel!r}") from None
    if start < 0 or count < 1 or start + count > L:
        raise ValueError(f"(start, count) = ({start}, {count}) leaves the sequence [0, {L})")
    return start, count


def resolve_layers(layers, n_layers):
    """Layer indices as a list: None = every layer, negative indices count from the end.  ValueError outside the encoder."""
    if layers is None:
        return list(range(n_layers))
    out = []
    for i in layers:
        j = int(i)
        if not -n_layers <= j < n_layers:
            raise ValueError(f"layer {j} of an encoder with {n_layers} layers")
        out.append(j % n_layers)
    if not out:
        raise ValueError("layers selects nothing")
    return out


def image_heatmap(maps, views=1):
    """[..., n_img] (keys = 'image') -> [..., views, g, g] with g = isqrt(n_img // views): the image tokens of each view as the
    g x g grid the Swin tower ends in (7 x 7 at 224 pixels; two views for 5-D image input).  A reshape and nothing else:
    up-sampling to pixels is the caller's business.  ValueError when n_img // views is not a square."""
    n, views = int(maps.shape[-1]), int(views)
    if views < 1 or n % views != 0:
        raise ValueError(f"{n} image tokens do not split into {views} views")
    g = math.isqrt(n // views)
    if g * g != n // views:
        raise ValueError(f"{n // views} image tokens per view are not a square grid")
    return maps.reshape(tuple(maps.shape[:-1]) + (views, g, g))
