"""Greedy report generation with a KV cache, drop-in for the reference's UniLM
decode loop (``modules/model.py:82-108`` cache branch of ``get_embedding``,
``:577-604`` prepare_inputs, ``:826-984`` greedy_search, ``:890-894`` cache trim).

Layout: one preallocated cache ``[layers][B, nH, cap, hd]`` per K and V
(``_alloc_cache``: the prefix, max_length tokens and the [MASK] slot).  Step 0 (``_step0``) runs the full seq2seq forward
over ``[CLS] img [SEP] [MASK]``; every later step (``_step2``) feeds the 2 tokens
``[last_token, [MASK]]`` at positions ``past, past+1`` (type 0), appends their
K/V in place and attends causally (``mvlt_attn_cached``).  "Trimming the [MASK]
slot" (model.py:890-894) is just ``past += 1``: the next step overwrites it.
Every search is argument resolution (``_resolve``), a route (``_greedy_route`` / ``_beam_route``: pure functions of the call's
arguments and of the switches ``_env`` reads per call) and one loop per route; the replayed graphs share ``_DecodeGraph``.
A non-beam search (``greedy_search``, ``sample_many``) is its argument checks and three choices: a row layout (``_Plain`` /
``_Prompted`` / ``_SharedPrefix``: which first pass fills the caches, how the rows find their K / V in ``_step2``), a pick
(``_PICKS``: eager form and captured form per name, row chunks of 64 in ``_pick`` alone) and the logit rules.  The token loop
exists once per kind -- ``_graph_loop`` (a ``_TokenGraph`` over a ``_TokenState``, replayed by ``_replay``, which the beam graph
shares) and ``_eager_loop`` -- so what is wired into a layout or a pick reaches both; ``_graph_slot_key`` names a graph's slot and key.
Greedy mode replays one captured HIP graph per token (``_GreedyGraph``: position,
output column and finished flags live on the device; ``MVLT_DECODE_GRAPH=0`` selects
the eager loop).  'sample' mode (B <= 64) is the same graph with the Gumbel-max pick of ``mvlt_gemm_sample_step`` as
its head: the token of output column c is ``argmax_n (logit_n / T + G_n)`` with the noise a pure function of
``(seed, SAMPLE_TAG0 + c, row * V + n)``, so the graph loop and the eager loop draw the same tokens from the same seed.
``top_k`` / ``top_p`` ('sample' mode only) put ``mvlt_gemm_sample_filtered_step`` in the head's place: the logits of the row go
through a workspace, a workgroup per row selects the threshold (top-k with ties kept, then the nucleus over what is left) and
draws among the kept tokens with the same noise; the score is the log-probability under the renormalised distribution.  The
eager loop calls the stand-alone entry point, for B > 64 in row chunks of 64 whose noise is indexed by the row of the batch.
Logit rules (``repetition_penalty`` / ``no_repeat_ngram_size`` / ``min_length``, HF's three processors on the raw logits): a plan
kernel rebuilds two bitmaps per row (tokens seen, tokens banned) from the device-side history before every pick and the ``_rules``
forms of the head entry points apply them in their epilogues (``ops.LogitRules``) -- in the graph and in the eager loop alike, any B
(rows in chunks of 64; rules never fall back to torch picks).  All rules off is the code path without them.
Several reports per image (``sample_many``): K sampled rows and, optionally, the greedy row of every image decode in ONE pass over
B * S rows.  Step 0 runs once per image, the cached steps read the shared prefix through ``mvlt_attn_cached_beam`` with a constant
slot table (no cache row is copied), and ``mvlt_gemm_pick_rows(_step)`` picks for all rows at once: two device tables say per row
whether it is greedy or sampled, which noise row it draws with, and its temperature.  Eager loop or ``_MultiSampleGraph``.
Beam search (``beam_search``): same cached steps over B*beams rows, scorer bookkeeping on the host restated from HF
transformers 4.16 (parity with the reference unpinned).  Default route (beams <= 8, head_dim 64): the candidates of a token come
from ``mvlt_gemm_beam_candidates`` (head + log-softmax + beam score + top 2*beams per sample, f32 logits through a workspace) and
the cache is never reordered -- ``mvlt_attn_cached_beam`` follows an int32 table [rows, max_length] that names, per hypothesis and
generated position, the cache row (within the sample) that holds it; the image prefix is stored once per sample.
``MVLT_BEAM_FUSED=0`` (and any other shape) takes the route of the reference: bf16 logits, ``log_softmax``, ``topk`` and a
gather of every layer's cache by beam index per token.  ``MVLT_BEAM_DEVICE=1`` / ``beam_search(device_scorer=True)`` (off by default,
shapes of the fused route): the scorer's ``process`` runs on the device too (``mvlt_beam_step`` on a ``BeamDeviceState``), so the loop
has no per-token read-back and is replayed as one HIP graph per token (``_BeamGraph``; ``MVLT_DECODE_GRAPH=0``: eager); ``finalize``
stays on the host, after one read-back.
Text prompts (``greedy_search(input_ids=, prompt_lengths=)``, the reference's ``input_ids`` argument, here with a length per row):
``prompt_tables`` lays the rows out as ``prompt_b [MASK] filler`` [B, P_max + 1], ``_prefill`` runs ONE dense seq2seq pass over
``[CLS] img [SEP]`` + that text (causal over the text: row b's [MASK] sees its own prompt only), takes every row's own [MASK] row and
fills the caches; from then on the common position ``past`` starts at n_img + 2 + P_max and a table ``row_shift[b] = P_b - P_max``
places row b at its own position in the two kernels of the cached step that know positions (``mvlt_embed_fwd_rows``,
``mvlt_attn_cached_rows``: slots behind a row's position are never read, so the filler needs no clean-up).  The picks, their device
state and ``past`` / ``col`` are untouched; the prompted graphs live in slots of their own, keyed by the cache capacity too.  The
ids and scores returned are the continuation's; the logit rules see the continuation only.  No prompt: today's calls, byte for byte.
Logit rules in beam search (``beam_search(repetition_penalty=, no_repeat_ngram_size=, min_length=)``): HF 4.16 places the processors
on the log-probabilities, ahead of the beam score.  The fused and the device route run ``mvlt_beam_rules_plan`` over the int32 live
sequences (the hypotheses' own tokens after the beam reorder: ``BeamDeviceState.seq`` on the device route) and the rule-aware
selection of ``mvlt_gemm_beam_candidates_rules`` (``ops.BeamLogitRules``); the plain route applies the same rules as torch ops on
its ``log_softmax`` rows and uses neither kernel.  All rules off is the code path, and the graph, without them.
"""
from __future__ import annotations

import os
from types import SimpleNamespace

import torch

from . import _lib as L
from . import ops
from .arena import Arena
from .bert import EncoderOutput
from .runtime import compute_dtype_of


# the two N = H products of a decode layer split their reduction over workgroups; the k-slices meet in f32 slabs that the
# LayerNorm launch behind them adds in slice order (round 5: no float atomics -- bf16 greedy decoding is reproducible run to run)
_SKINNY_SPLIT = True
_SPLITS = (2, 4)      # reduction splits of (attention output, FFN-out) projections: the fastest of the round-2 sweep
# noise tags of sampled decoding: output column c draws with tag SAMPLE_TAG0 + c (the seed is the call's own, so the range
# cannot meet the dropout / DropPath / MLM-mask tags of a training step, which hash their step seed)
SAMPLE_TAG0 = 0x53000000
BEAM_STEP_STAGE = 8192          # num_beams * max_length int32 words mvlt_beam_step stages in LDS (csrc/beam.hip BS_STAGE)
# The reference asks the device "all finished?" after every token (model.py:954), which serialises host and GPU.  Finished
# sequences only emit PAD, so running a few steps past the end changes nothing that is kept: the flag of every column is
# recorded on the device, read back every SYNC_EVERY columns, and the outputs are cut where the reference would have stopped.
SYNC_EVERY = 8


# ----------------------------------------------------------------------------- host-only rules (tests/test_decode_host_cpu.py)
def _env():
    """The switches of this module, read per call: (graph_on, fused_on, device_on)."""
    env = os.environ.get
    return env("MVLT_DECODE_GRAPH", "1") == "1", env("MVLT_BEAM_FUSED", "1") != "0", env("MVLT_BEAM_DEVICE", "0") == "1"


def _greedy_route(sample_mode, B, filtered, graph_on):
    """(loop, pick) of greedy_search, a pure function of its arguments.  ('graph', 'greedy' | 'sample'): the replayed graph, whose
    fused head holds the whole batch in one 64-row tile (a filter only swaps the sampled head's entry point).  ('eager', pick):
    'gemm_argmax' / 'gemm_sample' (the fused picks, B <= 64), 'filtered' (the fused filtered pick, rows in chunks of 64),
    'argmax' / 'multinomial' (B > 64: torch on the logits)."""
    if filtered and sample_mode != 'sample':
        raise ValueError("top_k / top_p filter the sampled pick: they need sample_mode='sample'")
    if sample_mode not in ('greedy', 'sample'):
        raise ValueError("sample mode error!")
    if graph_on and B <= 64:
        return 'graph', sample_mode
    if filtered:
        return 'eager', 'filtered'
    if sample_mode == 'greedy':
        return 'eager', 'gemm_argmax' if B <= 64 else 'argmax'
    return 'eager', 'gemm_sample' if B <= 64 else 'multinomial'


def _graph_slot_key(B, n_img, max_length, cd, pad, eos, mask_id, arena, device, mode='greedy', temperature=1.0, top_k=0, top_p=1.0,
                    rules=(1.0, 0, 0), p_max=None, S=None):
    """(slot, key) of the replayed graph of a non-beam search, a pure function of its arguments: the name under which the graph
    lives in ``model.__dict__`` and what a call must share with it to replay it.  A sampled graph lives beside the greedy one,
    the prompted graphs (``p_max``, keyed by the cache capacity too) beside both and the multi-sample graph (``S`` rows per image;
    temperature and the split of S are data) beside all four, so no call recaptures another's graph; a filter or a rule set takes
    the slot of its mode, like a new temperature.  ``arena`` / ``device``: the address of the weights, the device index."""
    if S is not None:
        slot, key = "_mvlt_multi_sample_graph", (B, S, n_img, max_length, cd, pad, eos, mask_id, arena, device)
    else:
        slot, key = "_mvlt_greedy_graph", (B, n_img, max_length, cd, pad, eos, mask_id, arena, device)
        if mode != 'greedy':
            slot, key = "_mvlt_sample_graph", key + (mode, float(temperature))
            if (top_k, top_p) != (0, 1.0):
                key = key + (top_k, top_p)
    if rules != (1.0, 0, 0):
        key = key + ("rules",) + tuple(rules)
    if p_max is not None:
        slot = "_mvlt_prompt_graph" if mode == 'greedy' else "_mvlt_prompt_sample_graph"
        key = key + ("prompt", n_img + 2 + p_max + max_length + 1)
    return slot, key


def _default_seed():
    """A 63-bit seed from torch's default CPU generator: torch.manual_seed makes an unseeded sampled decode reproducible."""
    return int(torch.randint(0, 2 ** 63 - 1, (1,), dtype=torch.int64).item())


def _check_temperature(temperature, finite=False):
    if not float(temperature) > 0.0 or (finite and float(temperature) == float("inf")):
        raise ValueError("temperature must be positive")


def check_logit_rules(repetition_penalty=1.0, no_repeat_ngram_size=0, min_length=0, num_beams=1, V=None, max_length=None):
    """(float penalty, int ngram, int min_length) of a constrained decode, or ValueError: penalty > 0 (1.0 = off, no NaN),
    ngram >= 0 (0 = off), min_length >= 0 (0 = off); any rule switched on needs num_beams <= 1 (the rules of this function are
    those of the greedy and sampled picks, on the raw logits; ``beam_search`` takes its own, on the log-probabilities, and checks
    them here with num_beams = 1) and, when ``V`` / ``max_length`` are given, V > max_length: a history of max_length - 1 tokens
    plus eos can ban max_length columns, and a row must keep one."""
    pen = float(repetition_penalty)
    if not pen > 0.0 or pen == float("inf"):
        raise ValueError("repetition_penalty must be a positive number (1.0 switches it off)")
    for name, v in (("no_repeat_ngram_size", no_repeat_ngram_size), ("min_length", min_length)):
        if (isinstance(v, float) and v != v) or int(v) != v or int(v) < 0:
            raise ValueError(f"{name} must be a non-negative integer (0 switches it off)")
    rules = pen, int(no_repeat_ngram_size), int(min_length)
    if rules != (1.0, 0, 0):
        if num_beams > 1:
            raise ValueError("repetition_penalty / no_repeat_ngram_size / min_length with beam search (num_beams > 1) go through "
                             "decode.beam_search or MVLBertForImageCaption.generate")
        if V is not None and max_length is not None and V <= max_length:
            raise ValueError(f"logit rules can ban up to max_length = {max_length} columns: the vocabulary ({V}) must be larger")
    return rules


def check_beam_rules(repetition_penalty, no_repeat_ngram_size, min_length, num_beams, V, max_length):
    """The rules of a beam search, or ValueError: the argument checks of ``check_logit_rules`` and, with a rule switched on,
    V >= max(max_length + 2, 2 * num_beams + 1).  A row bans at most c + 1 <= max_length columns, which leaves every sample
    2 * num_beams unbanned entries at every step -- at step 0, where ONE row is scored, and later, where each of the num_beams
    rows keeps two -- so the scorer always finds its num_beams tokens."""
    rules = check_logit_rules(repetition_penalty, no_repeat_ngram_size, min_length)
    need = max(max_length + 2, 2 * num_beams + 1)
    if rules != (1.0, 0, 0) and V < need:
        raise ValueError(f"logit rules can ban up to max_length = {max_length} columns of a row: {num_beams} beams need a vocabulary "
                         f"of at least {need} tokens, not {V}")
    return rules


def _beam_route(num_beams, head_dim, max_length, fused_on, device_scorer, device_on=False):
    """'plain' | 'fused' | 'device', a pure function of its arguments (``device_scorer`` None: ``device_on``, the env value).
    The fused route needs what its two entry points need, the device scorer also the LDS stage of mvlt_beam_step; everything
    else decodes the way the reference does."""
    fused = fused_on and 1 <= num_beams <= ops.BEAM_MAX_BEAMS and 2 * num_beams <= ops.BEAM_MAX_CAND and head_dim == 64
    if device_scorer is None:
        device_scorer = device_on
    if device_scorer and fused and num_beams * max_length <= BEAM_STEP_STAGE:
        return 'device'
    return 'fused' if fused else 'plain'


def check_prompt(input_ids, prompt_lengths, B, n_img, max_length, pos_rows):
    """The prompt lengths of a prompted decode as a list of B host integers, or ValueError: ``input_ids`` int64 [B, P_max],
    ``prompt_lengths`` None (every row has P_max tokens) or B host integers (list / tuple / CPU tensor: a device tensor would
    have to be read back) with 0 <= P_b <= P_max, and the last position the decode can write, that of the [MASK] behind
    max_length new tokens, inside the position table: n_img + 2 + P_max + max_length + 1 <= pos_rows."""
    if not torch.is_tensor(input_ids) or input_ids.dim() != 2 or input_ids.dtype != torch.int64:
        raise ValueError("input_ids must be an int64 tensor [B, P_max]")
    if input_ids.shape[0] != B:
        raise ValueError(f"input_ids has {input_ids.shape[0]} rows for a batch of {B} images")
    p_max = input_ids.shape[1]
    if prompt_lengths is None:
        lens = [p_max] * B
    else:
        if torch.is_tensor(prompt_lengths):
            if prompt_lengths.device.type != 'cpu':
                raise ValueError("prompt_lengths are host integers (a list or a CPU tensor): the decode reads nothing back")
            if prompt_lengths.dtype.is_floating_point or prompt_lengths.dtype == torch.bool:
                raise ValueError("prompt_lengths must be integers")
            prompt_lengths = prompt_lengths.reshape(-1).tolist()
        lens = list(prompt_lengths)
        if len(lens) != B:
            raise ValueError(f"{len(lens)} prompt lengths for a batch of {B} images")
        for v in lens:
            if isinstance(v, bool) or int(v) != v or not 0 <= int(v) <= p_max:
                raise ValueError(f"prompt lengths must be integers in [0, P_max = {p_max}], not {v!r}")
        lens = [int(v) for v in lens]
    need = n_img + 2 + p_max + max_length + 1
    if need > pos_rows:
        raise ValueError(f"{n_img} image tokens + 2 + a prompt of {p_max} + {max_length} new tokens + [MASK] need {need} positions: "
                         f"the position table has {pos_rows}")
    return lens


def prompt_tables(input_ids, prompt_lengths, mask_id):
    """The tables of a prompted decode, a pure function of its arguments (on the device of ``input_ids``, nothing read back):
    ``text`` int64 [B, P_max + 1], row b = its P_b prompt tokens, [MASK] at column P_b and [MASK] in every column behind it (what
    lies there is seen by nothing that is kept; the mask id keeps it a valid word row); ``row_shift`` int32 [B] = P_b - P_max, the
    distance of row b's position from the common one; ``mask_col`` int64 [B] = P_b, the text column of row b's [MASK].
    ``prompt_lengths``: None (every row P_max) or B host integers, as ``check_prompt`` returns them."""
    B, p_max = input_ids.shape
    lens = [p_max] * B if prompt_lengths is None else [int(v) for v in prompt_lengths]
    mask_col = torch.tensor(lens, dtype=torch.int64).to(input_ids.device)
    cols = torch.arange(p_max + 1, dtype=torch.int64, device=input_ids.device)[None, :]
    padded = torch.cat([input_ids, input_ids.new_full((B, 1), mask_id)], dim=1)
    text = torch.where(cols < mask_col[:, None], padded, torch.full_like(padded, mask_id)).contiguous()
    return text, (mask_col - p_max).to(torch.int32), mask_col


def _sync_due(eos, done, last=None):
    """Read the finished flags back after ``done`` columns?  One host sync per SYNC_EVERY tokens (and at column ``last``)."""
    return eos is not None and (done % SYNC_EVERY == 0 or done == last)


def _cut(alive, n_cols):
    """(n_out, n_scores) of a greedy decode that produced ``n_cols`` columns; ``alive``: the per-column "a sample is unfinished"
    flags as a list (empty without eos).  The reference's per-token check stops at the first 0, before appending that step's
    score."""
    if 0 in alive:
        n_out = alive.index(0) + 1
        return n_out, n_out - 1
    return n_cols, n_cols


def _layers_cached(mv, ar, x, kc, vc, past, n_new, out_last=None, beam=None, row_shift=None):
    """x: [B*n_new, H] embeddings of the new tokens -> last hidden [B*n_new, H] (written into ``out_last`` when given).
    ``beam`` = (num_beams, prefix, slot table): the attention follows beam ancestry through the table (ops.attn_cached_beam).
    ``row_shift`` (int32 [B], device; not with ``beam``): batch row b sits at ``past + row_shift[b]`` (ops.attn_cached(row_shift=))."""
    cfg = mv.config
    H = cfg.hidden_size
    nH = cfg.num_attention_heads
    rows = x.shape[0]
    # the two N = H products of a layer (attention output, FFN-out) split their reduction over workgroups, every k-slice into
    # an f32 slab of its own; bias + residual + LayerNorm add the slabs (read only: every product OVERWRITES its slabs, nothing
    # is zeroed) in the launch that follows anyway
    # (bf16 only: the exact-f32 parity mode keeps the deterministic summation order of the plain skinny kernel)
    split = _SKINNY_SPLIT and rows <= 64 and x.dtype == torch.bfloat16
    acc = None
    if split:
        key = ("decode_acc", rows, H, x.device.index)
        acc = ar._views.get(key)
        if acc is None:
            acc = ar._views[key] = torch.empty((max(_SPLITS), rows, H), dtype=torch.float32, device=x.device)
    nl = len(mv.encoder.layer)
    for i, layer in enumerate(mv.encoder.layer):
        last_out = out_last if i == nl - 1 else None
        sa, so = layer.attention.self, layer.attention.output
        qkv = ops.gemm(x, ar.compute(sa.query.weight, 3 * H), bias=ar.master_span(sa.query.bias, 3 * H))
        if beam is None:
            ctx = ops.attn_cached(qkv, kc[i], vc[i], past, (H // nH) ** -0.5, row_shift=row_shift)
        else:
            ctx = ops.attn_cached_beam(qkv, kc[i], vc[i], past, (H // nH) ** -0.5, beam[0], beam[1], beam[2])
        if split:
            ops.gemm_skinny_accum(ctx, ar.compute(so.dense.weight), acc[:_SPLITS[0]], _SPLITS[0])
            x1 = ops.layernorm_acc_fwd(acc[:_SPLITS[0]], so.dense.bias.data, x, so.LayerNorm.weight.data, so.LayerNorm.bias.data,
                                       so.LayerNorm.eps, x.dtype)
        else:
            y1 = ops.gemm(ctx, ar.compute(so.dense.weight), bias=so.dense.bias.data, residual=x)
            x1, _, _, _ = ops.layernorm_fwd(y1, so.LayerNorm.weight.data, so.LayerNorm.bias.data, so.LayerNorm.eps,
                                            save_stats=False)
        a = ops.gemm(x1, ar.compute(layer.intermediate.dense.weight), bias=layer.intermediate.dense.bias.data, gelu=True)
        lo = layer.output
        if split:
            ops.gemm_skinny_accum(a, ar.compute(lo.dense.weight), acc[:_SPLITS[1]], _SPLITS[1])
            x = ops.layernorm_acc_fwd(acc[:_SPLITS[1]], lo.dense.bias.data, x1, lo.LayerNorm.weight.data, lo.LayerNorm.bias.data,
                                      lo.LayerNorm.eps, x1.dtype, out=last_out)
        else:
            y2 = ops.gemm(a, ar.compute(lo.dense.weight), bias=lo.dense.bias.data, residual=x1)
            x, _, _, _ = ops.layernorm_fwd(y2, lo.LayerNorm.weight.data, lo.LayerNorm.bias.data, lo.LayerNorm.eps,
                                           save_stats=False, out=last_out)
    return x


def _embed_new(mv, ids, past, dtype, row_shift=None):
    cfg = mv.config
    return ops.embed_fwd(ids.contiguous(), None, mv.word_embeddings.weight.data, mv.position_embeddings.weight.data,
                         mv.token_type_embeddings.weight.data, cfg.cls_token_id, cfg.sep_token_id, dtype=dtype,
                         pos_offset=past, type_override=0, row_shift=row_shift)


def _fill_cache_from_qkv(qkv, B, Lq, nH, hd, kc, vc, keep):
    v5 = qkv.view(B, Lq, 3, nH, hd)
    kc[:, :, :keep].copy_(v5[:, :keep, 1].permute(0, 2, 1, 3))
    vc[:, :, :keep].copy_(v5[:, :keep, 2].permute(0, 2, 1, 3))


def _resolve(model, image_feature, max_length, pad_token_id, eos_token_id):
    """The arguments every search starts from: (compute dtype, arena (refreshed), max_length, pad, eos, mask_id, feat)."""
    cfg = model.config
    cd = compute_dtype_of(model)
    ar = Arena.of(model, cd)
    ar.refresh_shadow()
    max_length = max_length if max_length is not None else cfg.max_length
    pad = pad_token_id if pad_token_id is not None else cfg.pad_token_id
    eos = eos_token_id if eos_token_id is not None else cfg.eos_token_id
    tok = getattr(model, "tokenizer", None)
    mask_id = tok.mask_token_id if tok is not None else cfg.mask_token_id
    return cd, ar, max_length, pad, eos, mask_id, image_feature.to(cd).contiguous()


def _alloc_cache(model, rows, n_img, max_length, cd, device):
    """Zeroed K and V caches ``[layers][rows, nH, cap, hd]``: the prefix, max_length tokens and the [MASK] slot."""
    cfg = model.config
    nH = cfg.num_attention_heads
    shape = (rows, nH, n_img + 2 + max_length + 1, cfg.hidden_size // nH)
    nl = len(model.MVLBert.encoder.layer)
    return ([torch.zeros(shape, dtype=cd, device=device) for _ in range(nl)],
            [torch.zeros(shape, dtype=cd, device=device) for _ in range(nl)])


def _step0(mv, feat, mask_col, kc, vc, stride=1):
    """Step 0: [CLS] img [SEP] [MASK], the full seq2seq forward on the B images (model.py:110-160), eager.  The prefix goes
    into every ``stride``-th row of the caller's caches, in place (stride = num_beams: the first row of every sample).
    Returns (last hidden row [B, H], a view; prefix length = the position the first 2-token step writes)."""
    B, n_img, H = feat.shape
    nH = mv.config.num_attention_heads
    hidden, _, saved = mv._forward(feat, mask_col, mask_col, None, True, True)
    L0 = n_img + 3
    for i in range(len(mv.encoder.layer)):
        _fill_cache_from_qkv(saved["layers"][i][1], B, L0, nH, H // nH, kc[i][::stride], vc[i][::stride], L0 - 1)
    return hidden[:, -1], L0 - 1


def _prefill(mv, feat, text, mask_col, kc, vc):
    """Step 0 of a prompted decode: ONE dense seq2seq forward over [CLS] img [SEP] text, ``text`` [B, P_max + 1] of
    ``prompt_tables``.  The mask is causal over the text, so row b's [MASK] at text column P_b sees its own prompt and nothing
    behind it.  Positions [0, n_img + 2 + P_max) go into the caches: those of row b at and beyond n_img + 2 + P_b hold its
    [MASK] and the filler, which the cached steps overwrite or never read (mvlt_attn_cached_rows reads below the row's own
    position only).  Returns (the hidden row of every sample's own [MASK] [B, H]; the common position n_img + 2 + P_max)."""
    B, n_img, H = feat.shape
    nH = mv.config.num_attention_heads
    hidden, _, saved = mv._forward(feat, text, text, None, True, True)
    Lq = n_img + 2 + text.shape[1]
    for i in range(len(mv.encoder.layer)):
        _fill_cache_from_qkv(saved["layers"][i][1], B, Lq, nH, H // nH, kc[i], vc[i], Lq - 1)
    rows = torch.arange(B, dtype=torch.int64, device=feat.device)
    return hidden[rows, mask_col + (n_img + 2)], Lq - 1


def _step2(mv, ar, new_ids, past, kc, vc, cd, out_last=None, beam=None, row_shift=None):
    """The cached forward of the 2 tokens ``new_ids`` [rows, 2] = [last token, MASK] at positions past, past + 1
    (model.py:82-108, :587-591) -> the [MASK] rows [rows, H], a view of the [rows * 2, H] output (``out_last`` when given).
    ``row_shift`` (prompted decode): row b's two positions are past + row_shift[b] and the one behind it."""
    rows, H = new_ids.shape[0], mv.config.hidden_size
    x = _embed_new(mv, new_ids, past, cd, row_shift).view(rows * 2, H)
    return _layers_cached(mv, ar, x, kc, vc, past, 2, out_last=out_last, beam=beam, row_shift=row_shift).view(rows, 2, H)[:, -1]


def _head(model, ar, hlast):
    """(t2, W, bias): the head transform of ``hlast`` and the decoder's operands.  ``hlast`` is read where it lies: the graphs
    hand over the [MASK] rows of their [rows, 2, H] buffer at row stride 2 H."""
    hd = model.MLM_head_seq2seq
    _, _, t2, _, _ = hd._transform(ar, hlast, False)
    return t2, ar.compute(hd.predictions.decoder.weight), hd.predictions.decoder.bias.data


@torch.no_grad()
def cached_forward(mv, text_idx, image_feature, past_key_values, seq2seq_mask):
    """``MVLBert.forward(..., past_key_values=..., use_cache=True)`` API (model.py:59-62):
    returns ``(EncoderOutput(last_hidden_state, past_key_values), pooler_output)``."""
    cd = compute_dtype_of(mv)
    ar = Arena.of(mv, cd)
    ar.refresh_shadow()
    cfg = mv.config
    H, nH = cfg.hidden_size, cfg.num_attention_heads
    hd = H // nH
    nl = len(mv.encoder.layer)
    if past_key_values is None:
        feat = image_feature.to(cd).contiguous()
        B, n_img, _ = feat.shape
        ids = text_idx.contiguous() if text_idx is not None else None
        hidden, pooled, saved = mv._forward(feat, ids, ids, None, bool(seq2seq_mask), True)
        Lq = hidden.shape[1]
        pkv = []
        for i in range(nl):
            v5 = saved["layers"][i][1].view(B, Lq, 3, nH, hd)
            pkv.append((v5[:, :, 1].permute(0, 2, 1, 3).contiguous(), v5[:, :, 2].permute(0, 2, 1, 3).contiguous()))
        return EncoderOutput(hidden, tuple(pkv)), pooled
    if not seq2seq_mask:
        raise NotImplementedError("the reference only uses the cache with seq2seq_mask=True (model.py:604)")
    B, n_new = text_idx.shape
    past = past_key_values[0][0].shape[2]
    cap = past + n_new
    kc = [torch.empty((B, nH, cap, hd), dtype=cd, device=text_idx.device) for _ in range(nl)]
    vc = [torch.empty((B, nH, cap, hd), dtype=cd, device=text_idx.device) for _ in range(nl)]
    for i in range(nl):
        kc[i][:, :, :past].copy_(past_key_values[i][0])
        vc[i][:, :, :past].copy_(past_key_values[i][1])
    x = _embed_new(mv, text_idx, past, cd).view(B * n_new, H)
    h = _layers_cached(mv, ar, x, kc, vc, past, n_new).view(B, n_new, H)
    return EncoderOutput(h, tuple((kc[i], vc[i]) for i in range(nl))), None


def _no_graph():
    return None


class _DecodeGraph:
    """What the replayed decode graphs share.  A subclass keeps its static device buffers and ``body()``, the per-token work; the
    graph of a model lives in ``model.__dict__[slot]`` until a call arrives with another ``key``."""

    def __reduce__(self):                 # captured graphs do not survive pickling: rebuilt on the next call
        return (_no_graph, ())

    @classmethod
    def of(cls, model, slot, key, *args):
        g = model.__dict__.get(slot)
        if g is None or g.key != key:
            g = cls(model, key, *args)
            g.capture()
            model.__dict__[slot] = g
        return g

    def capture(self):
        # scratch buffers (split-K workspace) used inside the graph get their own tag: the captured pointers must
        # never be freed or handed to other work by a later, larger request on the main stream
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side), ops.on_stream(side, "graph"):     # warm-up outside the capture (allocator, lazy state)
            self.body()
        torch.cuda.current_stream().wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            with ops.on_stream(torch.cuda.current_stream(), "graph"):
                self.body()
        self.graph = g


def _replay(graph, alive, tail, max_length, eos):
    """Token loop of a captured graph: a replay per token (token t, then the forward that prepares token t + 1), ``tail()`` for
    the last token, which needs no forward; ``alive`` (the per-column flags on the device) is read back every SYNC_EVERY
    columns.  Returns the number of columns produced."""
    for t in range(max_length - 1):
        graph.replay()
        if _sync_due(eos, t + 1) and 0 in alive[t + 1 - SYNC_EVERY:t + 1].tolist():
            return t + 1
    tail()
    return max_length


# ----------------------------------------------------------------------------- the non-beam searches: a row layout, a pick, one loop
class _TokenState:
    """The device side of a token loop over ``rows`` rows, in static buffers, with the prepared ``L.MvltGreedyState`` /
    ``L.MvltSampleState`` (``state``) that the ``_step`` heads take: the cache position (``past``: read by the embedding and
    attention kernels through ``pos_offset_dev`` / ``past_dev``), the output column, the ids fed to the next step, the unfinished
    flags, the [rows, max_length] outputs, the per-column "a row is unfinished" flags, the seed cell and the ticket of the
    finishing launch, which advances all of them.  ``past`` / ``inv_temperature``: what the state holds from construction --
    the warm-up pass of a capture really runs on it, so the position must lie inside the cache."""

    def __init__(self, rows, max_length, pad, eos, mask_id, dev, sampled, past=0, inv_temperature=1.0):
        self.past = torch.full((1,), past, dtype=torch.int32, device=dev)
        self.col = torch.zeros(1, dtype=torch.int64, device=dev)
        self.new_ids = torch.full((rows, 2), mask_id, dtype=torch.int64, device=dev)       # [last token, MASK]
        self.unfinished = torch.ones(rows, dtype=torch.int64, device=dev)
        self.ids = torch.zeros((rows, max_length), dtype=torch.int64, device=dev)
        self.scores = torch.zeros((rows, max_length), dtype=torch.float32, device=dev)
        self.alive = torch.ones(max_length, dtype=torch.int64, device=dev)
        self.seed = torch.zeros(1, dtype=torch.int64, device=dev)
        self.ticket = torch.zeros(1, dtype=torch.int32, device=dev)
        st = self.state = L.MvltSampleState() if sampled else L.MvltGreedyState()
        if sampled:
            st.seed, st.tag0, st.inv_temperature = self.seed.data_ptr(), SAMPLE_TAG0, inv_temperature
        st.unfinished, st.eos_id, st.pad_id, st.has_eos = self.unfinished.data_ptr(), (eos if eos is not None else -1), pad, int(eos is not None)
        st.col, st.past = self.col.data_ptr(), self.past.data_ptr()
        st.ids, st.ld_ids, st.scores, st.ld_scores = self.ids.data_ptr(), max_length, self.scores.data_ptr(), max_length
        st.alive, st.new_ids, st.ld_new, st.ticket = self.alive.data_ptr(), self.new_ids.data_ptr(), 2, self.ticket.data_ptr()

    def reset(self, past):
        """Start of a decode whose first pass ended at position ``past`` (the first pick advances `past`; the picks raise `alive`)."""
        self.past.fill_(past - 1); self.col.zero_(); self.unfinished.fill_(1); self.alive.zero_(); self.ticket.zero_()

    def set_seed(self, seed):
        self.seed.fill_(ops.s64(int(seed) & ((1 << 64) - 1)))


class _Plain:
    """Row layout: how the rows of a search find their K / V -- which first pass fills the caches (``first_pass`` -> the [MASK]
    rows [R, H] and the common position) and the keywords ``_step2`` attends with (``attn(table)``; ``table``: the layout's
    int32 device table, the call's own or the static copy of a graph).  Plain: a row per image, every row at the common position.
    ``S`` rows per image, ``p_max`` cache slots in front of the new tokens, ``warm_past``: a valid position before any first pass."""
    S, p_max, table, warm_past = 1, 0, None, 0

    def first_pass(self, mv, feat, kc, vc, mask_ids):
        return _step0(mv, feat, mask_ids.contiguous(), kc, vc)

    def attn(self, table):
        return {}


class _Prompted(_Plain):
    """Row b behind its own P_b prompt tokens (the tables of ``prompt_tables``): one dense prefill, then ``row_shift[b]`` places
    the row at its own position."""

    def __init__(self, text, row_shift, mask_col):
        self.text, self.table, self.mask_col, self.p_max = text, row_shift, mask_col, text.shape[1] - 1

    def first_pass(self, mv, feat, kc, vc, mask_ids):
        return _prefill(mv, feat, self.text, self.mask_col, kc, vc)

    def attn(self, table):
        return {'row_shift': table}


class _SharedPrefix(_Plain):
    """S rows per image that share its prefix: step 0 once per image into every S-th cache row, the cached steps read it through
    ``mvlt_attn_cached_beam`` with the constant table ``slot`` int32 [R, max_length] (no cache row is copied)."""

    def __init__(self, S, prefix, slot):
        self.S, self.prefix, self.table, self.warm_past = S, prefix, slot, prefix - 1

    def first_pass(self, mv, feat, kc, vc, mask_ids):
        hlast, past = _step0(mv, feat, mask_ids[:feat.shape[0]].contiguous(), kc, vc, stride=self.S)
        return hlast.repeat_interleave(self.S, 0), past

    def attn(self, table):
        return {'beam': (self.S, self.prefix, table)}


def _pick_argmax(t2, W, bias, p, tag, row0, rules):
    logits = p.logits(t2)
    nxt = ops.argmax(logits, p.V)
    return nxt, logits[:, :p.V].float().gather(1, nxt[:, None]).squeeze(1)


def _pick_multinomial(t2, W, bias, p, tag, row0, rules):
    probs = ops.softmax_rows(p.logits(t2), p.V)
    nxt = torch.multinomial(probs, num_samples=1, replacement=True).squeeze(1)
    return nxt, torch.log(probs.gather(1, nxt[:, None])).squeeze(1)


# pick -> (eager form (t2, W, bias, p, tag, row0, rules) -> (tokens, scores); captured form (t2, W, bias, state, p, rules), which
# keeps the books on the device; rows per call).  ``p``: the call's parameters (seed, temperature, top_k, top_p, the row tables
# noise_row / inv_t of 'rows'; logits / V for the torch picks, which have no captured form and no rules).
_PICKS = {
    'gemm_argmax': (lambda a, W, b, p, tag, r0, rs: ops.gemm_argmax(a, W, b, rules=rs),
                    lambda a, W, b, st, p, rs: ops.gemm_argmax_greedy(a, W, b, st, rules=rs), 64),
    # the pick of the graph loop, stand-alone: same seed, tag and column -> same tokens
    'gemm_sample': (lambda a, W, b, p, tag, r0, rs: ops.gemm_sample(a, W, b, p.seed, tag, p.temperature, rules=rs),
                    lambda a, W, b, st, p, rs: ops.gemm_sample_step(a, W, b, st, rules=rs), 64),
    # rows beyond 64 in chunks, the noise indexed by the batch row
    'filtered': (lambda a, W, b, p, tag, r0, rs: ops.gemm_sample_filtered(a, W, b, p.seed, tag, p.temperature, p.top_k, p.top_p, row0=r0, rules=rs),
                 lambda a, W, b, st, p, rs: ops.gemm_sample_filtered_step(a, W, b, st, p.top_k, p.top_p, rules=rs), 64),
    'rows': (lambda a, W, b, p, tag, r0, rs: ops.gemm_pick_rows(a, W, b, p.noise_row, p.inv_t, p.seed, tag, rules=rs),
             lambda a, W, b, st, p, rs: ops.gemm_pick_rows_step(a, W, b, st, p.noise_row, p.inv_t, rules=rs), None),
    'argmax': (_pick_argmax, None, None),
    'multinomial': (_pick_multinomial, None, None),
}


def _pick(pick, t2, W, bias, p, tag, lr):
    """The eager form of ``pick`` over all rows of ``t2``, in row chunks where its entry point takes 64 rows; ``lr``: the
    ``ops.LogitRules`` of the call (the bitmaps of this token first) or None."""
    eager, _, chunk = _PICKS[pick]
    if lr is not None:
        lr.plan()
    if chunk is None or t2.shape[0] <= chunk:
        return eager(t2, W, bias, p, tag, 0, lr.struct() if lr is not None else None)
    parts = [eager(t2[r0:r0 + 64], W, bias, p, tag, r0, lr.struct(r0) if lr is not None else None) for r0 in range(0, t2.shape[0], 64)]
    return torch.cat([a for a, _ in parts]), torch.cat([b for _, b in parts])


class _TokenGraph(_DecodeGraph, _TokenState):
    """The whole per-token work of a non-beam search -- last-row MLM head + pick + [END]/PAD bookkeeping (the captured form of
    ``pick``) + the 2-token cached forward under ``layout`` -- captured ONCE as a HIP graph and replayed per token: one stream, no
    parallel branches.  Everything a replay needs lives in static device buffers: the ``_TokenState``, the caches, the hidden
    rows, and what a call brings as DATA (the layout's table, the row tables of the 'rows' pick), which the loop fills per call.
    The host only replays and, every 8 tokens, reads the all-finished flags back."""

    def __init__(self, model, key, rows, layout, pick, p, n_img, max_length, cd, pad, eos, mask_id, rules=(1.0, 0, 0)):
        dev = next(model.parameters()).device
        H = model.config.hidden_size
        self.key, self.model, self.cd, self.graph, self.pick = key, model, cd, None, pick
        # layout.p_max (prompted decode): room for the longest prompt in front of the new tokens
        self.kc, self.vc = _alloc_cache(model, rows, n_img, max_length + layout.p_max, cd, dev)
        # zero tables, no noise rows, temperature 1, a position inside the cache: valid for the warm-up pass, which really runs
        self.table = None if layout.table is None else torch.zeros(tuple(layout.table.shape), dtype=torch.int32, device=dev)
        self.attn = layout.attn(self.table)
        _TokenState.__init__(self, rows, max_length, pad, eos, mask_id, dev, pick != 'gemm_argmax', layout.warm_past, 1.0 / float(p.temperature))
        # last hidden states of the two new tokens of every row; the MLM head reads the [MASK] rows in place (row stride 2 H)
        self.hfull = torch.zeros((rows * 2, H), dtype=cd, device=dev)
        self.hlast = self.hfull.view(rows, 2, H)[:, 1]
        self.p = SimpleNamespace(top_k=p.top_k, top_p=p.top_p)          # (top_k, top_p) = (0, 1.0): no filter
        if pick == 'rows':
            self.p.noise_row = torch.full((rows,), -1, dtype=torch.int32, device=dev)
            self.p.inv_t = torch.ones(rows, dtype=torch.float32, device=dev)
        # logit rules: the graph owns the bitmaps; the plan reads the history where the picks write it (ids, col)
        self.rules = None
        if rules != (1.0, 0, 0):
            V = model.MLM_head_seq2seq.predictions.decoder.out_features
            self.rules = ops.LogitRules(V, *rules, eos, self.ids, self.col)

    def head(self):
        """token <- pick(MLM head(hlast)); record it in column `col`; past += 1; col += 1 (all on the device)."""
        # decoder GEMM fused with the pick and its bookkeeping: the [rows, 30522] logits are never written
        t2, W, bias = _head(self.model, Arena.of(self.model, self.cd), self.hlast)
        rules = None
        if self.rules is not None:          # the bitmaps of this token, then the rule-aware form of the same head
            self.rules.plan()
            rules = self.rules.struct()
        _PICKS[self.pick][1](t2, W, bias, self.state, self.p, rules)

    def body(self):
        """The pick, then the 2-token cached forward of [last token, MASK] at positions past, past+1.  `past` was advanced by the
        pick that produced the token: the previous step's [MASK] slot is overwritten (model.py:890-894)."""
        self.head()
        _step2(self.model.MVLBert, Arena.of(self.model, self.cd), self.new_ids, self.past, self.kc, self.vc, self.cd, out_last=self.hfull,
               **self.attn)


class _GreedyGraph(_TokenGraph):
    """The graph of ``greedy_search``: ``mode`` 'greedy' (``mvlt_gemm_argmax_greedy``) or 'sample' (``mvlt_gemm_sample_step``, with
    a filter ``mvlt_gemm_sample_filtered_step``: the same state plus the seed cell), plain or prompted (``row_shift``: the static
    table of the rows' distances from the common position, None without a prompt)."""
    mode = property(lambda self: 'greedy' if self.pick == 'gemm_argmax' else 'sample')
    row_shift = property(lambda self: self.table)


class _MultiSampleGraph(_TokenGraph):
    """The graph of ``sample_many`` over R = B * S rows that share the image prefix of their image: the per-row pick
    (``mvlt_gemm_pick_rows_step``: greedy and sampled rows in one head, any R) and the cached forward through
    ``mvlt_attn_cached_beam`` with the constant slot table.  What a row does (greedy or sampled, its noise row, its temperature)
    is DATA in two device tables, so one capture serves every num_samples / include_greedy / temperature with the same S."""


def _graph_loop(graph, model, feat, layout, pick, p, rules, max_length, pad, eos, mask_id, cd, flat):
    """``graph`` = (class, slot, key): the model's graph of that slot (captured when the key is new), the call's data into its
    static buffers, the first pass, then a replay per token.  Returns what ``_eager_loop`` returns."""
    cls, slot, key = graph
    gg = cls.of(model, slot, key, feat.shape[0] * layout.S, layout, pick, p, feat.shape[1], max_length, cd, pad, eos, mask_id, rules)
    if gg.table is not None:
        gg.table.copy_(layout.table)
    gg.set_seed(p.seed)
    if pick == 'rows':
        gg.p.noise_row.copy_(p.noise_row)
        gg.p.inv_t.copy_(p.inv_t)
    hlast, past = layout.first_pass(model.MVLBert, feat, gg.kc, gg.vc, gg.new_ids[:, 1:2])
    gg.reset(past)
    gg.hlast.copy_(hlast)
    done = _replay(gg.graph, gg.alive, gg.head, max_length, eos)
    n_out, n_scores = _cut(gg.alive[:done].tolist() if eos is not None else [], done)
    if not flat:
        return gg.ids[:, :n_out].clone(), gg.scores[:, :n_out].clone()
    return gg.ids[:, :n_out].clone(), gg.scores[:, :n_scores].t().reshape(-1).clone() if n_scores > 0 else torch.empty(0, device=feat.device)


def _eager_loop(model, ar, feat, layout, pick, p, rules, max_length, pad, eos, mask_id, cd, flat):
    """The token loop launch by launch over R = B * layout.S rows: ``(ids [R, n_out], scores)``, cut where the reference's
    per-token check would have stopped (``_cut``).  ``flat``: the scores of all but the column that ended the decode, concatenated
    column after column (``greedy_search``); else [R, n_out], a score per id (``sample_many``)."""
    mv = model.MVLBert
    dev, R = feat.device, feat.shape[0] * layout.S
    attn = layout.attn(layout.table)
    kc, vc = _alloc_cache(model, R, feat.shape[1], max_length + layout.p_max, cd, dev)
    mask_col = torch.full((R, 1), mask_id, dtype=torch.int64, device=dev)
    lr = None
    if rules != (1.0, 0, 0):          # the history the plan reads: the id matrix as the graph keeps it, and the column count
        V = model.MLM_head_seq2seq.predictions.decoder.out_features
        lr = ops.LogitRules(V, *rules, eos, torch.zeros((R, max_length), dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.int64, device=dev))
    hlast, past = layout.first_pass(mv, feat, kc, vc, mask_col)
    unfinished = torch.ones(R, dtype=torch.int64, device=dev)
    ids_cols, scores, alive, flags = [], [], [], []        # `alive`: device scalars, one per column; `flags`: what was read back
    while len(ids_cols) < max_length:
        t2, W, bias = _head(model, ar, hlast.contiguous())
        nxt, score = _pick(pick, t2, W, bias, p, SAMPLE_TAG0 + len(ids_cols), lr)
        if eos is not None:
            nxt = nxt * unfinished + pad * (1 - unfinished)
            unfinished = unfinished * (nxt != eos).long()
            alive.append(unfinished.max())
        if lr is not None:
            lr.ids[:, len(ids_cols)] = nxt
            lr.col.fill_(len(ids_cols) + 1)
        ids_cols.append(nxt[:, None])
        scores.append(score if flat else score[:, None])
        if _sync_due(eos, len(ids_cols), last=max_length):
            block = torch.stack(alive[-SYNC_EVERY:]).tolist()
            flags[len(alive) - len(block):] = block
            if 0 in block:
                break
        if len(ids_cols) >= max_length:
            break
        new_ids = torch.cat([nxt[:, None], mask_col], dim=1)              # [last_token, MASK] (model.py:587-591)
        hlast = _step2(mv, ar, new_ids, past, kc, vc, cd, **attn)
        past += 1                                                         # drop the [MASK] slot (model.py:890-894)
    n_out, n_scores = _cut(flags, len(ids_cols))
    scores = scores[:n_scores] if flat else scores[:n_out]
    return (torch.cat(ids_cols[:n_out], dim=-1) if ids_cols else None,
            torch.cat(scores, dim=-1) if scores else torch.empty(0, device=dev))


@torch.no_grad()
def greedy_search(model, image_feature, learning_strategy='unilm', sample_mode='greedy', max_length=None,
                  pad_token_id=None, eos_token_id=None, seed=None, temperature=1.0, top_k=0, top_p=1.0,
                  repetition_penalty=1.0, no_repeat_ngram_size=0, min_length=0, input_ids=None, prompt_lengths=None):
    """Returns ``(input_ids [B, n_steps], token_scores)`` like the reference
    (model.py:984: scores of all but the final step, concatenated along dim -1).
    ``sample_mode='sample'``, B <= 64: Gumbel-max draws from softmax(logits / temperature), reproducible from ``seed``
    (None: a 63-bit seed from torch's default CPU generator, so torch.manual_seed makes a run reproducible); the graph
    loop and the eager loop give the same tokens.  B > 64 without a filter samples with torch.multinomial (seed / temperature
    unused).
    ``top_k`` (0 = off) / ``top_p`` (1.0 = off), 'sample' mode only: keep the top_k largest logits (ties at the threshold all
    kept), then the tokens whose probability mass strictly above them is below top_p of what is left; draw among those, score =
    log-probability under the renormalised distribution.  Any B (rows in chunks of 64 beyond that, same draws); a filter in
    another mode, top_k < 0, top_p <= 0 or a NaN raises ValueError.
    ``repetition_penalty`` (1.0 = off) / ``no_repeat_ngram_size`` (0 = off) / ``min_length`` (0 = off): HF's
    RepetitionPenaltyLogitsProcessor, NoRepeatNGramLogitsProcessor and MinLengthLogitsProcessor on the raw logits, ahead of the
    temperature and the filters, over the history as stored (PAD of a finished row included); a banned token takes part in
    nothing and the scores follow the processed logits.  Both modes, any B, graph and eager loop the same tokens; with all
    three off the call is the one without them.  The vocabulary must exceed max_length (ValueError).
    ``input_ids`` (int64 [B, P_max], device) / ``prompt_lengths`` (None: every row P_max tokens, the reference's dense prefix;
    or B host integers 0 <= P_b <= P_max, nothing is read back): the decode continues row b's own P_b prompt tokens --
    ``[CLS] img [SEP] prompt_b [MASK]`` on the first pass (model.py:583-591), row b at position n_img + 2 + P_b from then on;
    what ``input_ids`` holds behind a row's length is never looked at.  ``max_length`` counts NEW tokens, the returned ids and
    scores are those of the continuation only (the reference returns the dense prefix in front; a ragged batch has no such
    matrix), and the logit rules see the continuation as stored: the prompt is no part of their history.  Both loops, every
    pick, any B.  ValueError: the cases of ``check_prompt`` (n_img + 2 + P_max + max_length + 1 positions must exist).  The
    first pass is the dense forward and has its reach: n_img + 2 + P_max + 1 <= 208 positions (mvlt_attn_fwd refuses more)."""
    top_k, top_p = ops.check_sample_filter(top_k, top_p)
    rules = check_logit_rules(repetition_penalty, no_repeat_ngram_size, min_length)
    if learning_strategy != 'unilm':
        raise NotImplementedError("only learning_strategy='unilm' is coherent with the KV cache (SURVEY.md 3.3)")
    if input_ids is None and prompt_lengths is not None:
        raise ValueError("prompt_lengths without input_ids")
    lens = None
    if input_ids is not None:          # refused before any device work
        lens = check_prompt(input_ids, prompt_lengths, image_feature.shape[0], image_feature.shape[1],
                            max_length if max_length is not None else model.config.max_length,
                            model.MVLBert.position_embeddings.weight.shape[0])
    cd, ar, max_length, pad, eos, mask_id, feat = _resolve(model, image_feature, max_length, pad_token_id, eos_token_id)
    V = model.MLM_head_seq2seq.predictions.decoder.out_features
    top_k, top_p = (top_k if top_k < V else 0), min(top_p, 1.0)          # the values that mean "off" in one spelling each
    loop, pick = _greedy_route(sample_mode, feat.shape[0], (top_k, top_p) != (0, 1.0), _env()[0])
    if rules != (1.0, 0, 0):
        check_logit_rules(*rules, V=V, max_length=max_length)
        # rules live in the fused heads only: the two torch picks of B > 64 become their chunked fused forms (a filtered pick with
        # both filters off draws the unfiltered token bit for bit)
        pick = {'argmax': 'gemm_argmax', 'multinomial': 'filtered'}.get(pick, pick)
    if sample_mode == 'greedy':
        seed, temperature = 0, 1.0               # unused by the greedy pick, and no part of its graph's key
    elif pick != 'multinomial':
        _check_temperature(temperature)
        seed = _default_seed() if seed is None else seed
    head = model.MLM_head_seq2seq
    p = SimpleNamespace(seed=seed, temperature=temperature, top_k=top_k, top_p=top_p, V=V, logits=lambda t2: head._logits(ar, t2)[0])
    layout = _Plain() if input_ids is None else _Prompted(*prompt_tables(input_ids.to(feat.device), lens, mask_id))
    if loop == 'eager':
        return _eager_loop(model, ar, feat, layout, pick, p, rules, max_length, pad, eos, mask_id, cd, True)
    # the fused head of the graph holds the whole batch in one 64-row tile; a filter only swaps the sampled head's entry point
    pick = 'gemm_argmax' if sample_mode == 'greedy' else 'filtered' if (top_k, top_p) != (0, 1.0) else 'gemm_sample'
    slot, key = _graph_slot_key(feat.shape[0], feat.shape[1], max_length, cd, pad, eos, mask_id, ar.flat.data_ptr(), feat.device.index,
                                sample_mode, temperature, top_k, top_p, rules, None if input_ids is None else layout.p_max)
    return _graph_loop((_GreedyGraph, slot, key), model, feat, layout, pick, p, rules, max_length, pad, eos, mask_id, cd, True)


# ----------------------------------------------------------------------------- K sampled reports per image in one pass
def multi_sample_tables(B, num_samples, include_greedy, temperature, max_length):
    """The row tables of ``sample_many`` as CPU tensors, a pure function of its arguments: rows r = b * S + s with
    S = num_samples + include_greedy; ``noise_row`` int32 [R] (-1 on the greedy row s = 0, else b * num_samples + k: the draws do
    not depend on include_greedy), ``inv_t`` f32 [R] (1 on greedy rows, the f32 value of 1 / temperature elsewhere) and ``slot``
    int32 [R, max_length] with slot[r, :] = r % S (every row reads its own generated positions; the prefix comes from row b * S)."""
    g = int(bool(include_greedy))
    S = num_samples + g
    s = torch.arange(B * S, dtype=torch.int64) % S
    b = torch.arange(B * S, dtype=torch.int64) // S
    sampled = s >= g
    noise_row = torch.where(sampled, b * num_samples + (s - g), torch.full_like(s, -1)).to(torch.int32)
    inv_t = torch.where(sampled, torch.tensor(1.0 / float(temperature), dtype=torch.float64), torch.tensor(1.0, dtype=torch.float64))
    slot = s.to(torch.int32)[:, None].expand(B * S, max_length).contiguous()
    return noise_row, inv_t.to(torch.float32), slot


@torch.no_grad()
def sample_many(model, image_feature, num_samples, include_greedy=True, seed=None, temperature=1.0, max_length=None,
                pad_token_id=None, eos_token_id=None, repetition_penalty=1.0, no_repeat_ngram_size=0, min_length=0):
    """``num_samples`` sampled reports per image, and the greedy report when ``include_greedy``, in ONE decode pass over
    R = B * S rows, S = num_samples + include_greedy: ``(ids int64 [B, S, n], scores f32 [B, S, n])``.  Row s = 0 of an image
    is the greedy row when included (decoded at temperature 1), the samples follow (decoded at ``temperature``).
    ``scores[b, s, c]`` is the log-probability of ``ids[b, s, c]`` at the row's temperature -- for the greedy row too, where
    ``greedy_search`` records the raw logit; the entries of a row behind its eos (where ``ids`` holds PAD) are unspecified.
    The outputs are cut at the column where the last row finished, like ``greedy_search``; ``scores`` has as many columns as ``ids``.

    Sample k of image b draws with the noise ``greedy_search(sample_mode='sample')`` gives batch row ``b * num_samples + k``
    (tag SAMPLE_TAG0 + column), whatever ``include_greedy`` says: ``sample_many(num_samples=1, include_greedy=False, seed=s)``
    draws the tokens of ``greedy_search(sample_mode='sample', seed=s)``.  ``seed=None``: a 63-bit seed from torch's default CPU
    generator.  Step 0 (the pass over [CLS] image [SEP] [MASK]) runs once per image and its K / V are stored once per image; the
    cached steps read them through ``mvlt_attn_cached_beam`` with a constant table, no cache row is ever copied, and one head
    (``mvlt_gemm_pick_rows``) picks for all R rows.  ``MVLT_DECODE_GRAPH=0`` runs the eager loop, anything else a replayed graph
    of its own (it never recaptures the greedy, sampled or beam graph); both give the same ids.
    Only the 'unilm' strategy; no ``top_k`` / ``top_p`` (a filter needs the whole row in a workspace and a finish of its own);
    the logit rules are ``greedy_search``'s (the vocabulary must exceed max_length); head_dim must be 64 (ValueError)."""
    if int(num_samples) != num_samples or num_samples < 1:
        raise ValueError("num_samples must be a positive integer")
    num_samples = int(num_samples)
    _check_temperature(temperature, finite=True)
    rules = check_logit_rules(repetition_penalty, no_repeat_ngram_size, min_length)
    cfg = model.config
    if cfg.hidden_size // cfg.num_attention_heads != 64:
        raise ValueError("sample_many reads the shared prefix through mvlt_attn_cached_beam, which needs head_dim 64")
    cd, ar, max_length, pad, eos, mask_id, feat = _resolve(model, image_feature, max_length, pad_token_id, eos_token_id)
    V = model.MLM_head_seq2seq.predictions.decoder.out_features
    if rules != (1.0, 0, 0):
        check_logit_rules(*rules, V=V, max_length=max_length)
    B = feat.shape[0]
    S = num_samples + int(bool(include_greedy))
    if B * S * V >= 2 ** 32:
        raise ValueError(f"{B * S} rows of {V} logits: the noise index rows * V must stay below 2^32")
    seed = _default_seed() if seed is None else seed
    graph_on, n_img = _env()[0], feat.shape[1]
    tables = multi_sample_tables(B, num_samples, include_greedy, temperature, max_length)
    if not graph_on:          # the eager loop reads the tables where they lie; a graph copies them into its own
        tables = [t.to(feat.device) for t in tables]
    # what a row does is data (noise_row, inv_t): the state's own temperature stays 1, and no part of the graph's key
    p = SimpleNamespace(seed=seed, temperature=1.0, top_k=0, top_p=1.0, noise_row=tables[0], inv_t=tables[1])
    layout = _SharedPrefix(S, n_img + 2, tables[2])
    if graph_on:
        slot, key = _graph_slot_key(B, n_img, max_length, cd, pad, eos, mask_id, ar.flat.data_ptr(), feat.device.index, rules=rules, S=S)
        ids, scores = _graph_loop((_MultiSampleGraph, slot, key), model, feat, layout, 'rows', p, rules, max_length, pad, eos, mask_id, cd, False)
    else:
        ids, scores = _eager_loop(model, ar, feat, layout, 'rows', p, rules, max_length, pad, eos, mask_id, cd, False)
    n = ids.shape[1]
    return ids.view(B, S, n), scores.view(B, S, n)


# ----------------------------------------------------------------------------- beam search (model.py:636-816)
class BeamHypotheses:
    """n-best list of finished hypotheses of one sample (HF transformers 4.16 ``BeamHypotheses``)."""

    def __init__(self, num_beams, length_penalty, early_stopping):
        self.num_beams, self.length_penalty, self.early_stopping = num_beams, length_penalty, early_stopping
        self.beams = []
        self.worst_score = 1e9

    def __len__(self):
        return len(self.beams)

    def add(self, hyp, sum_logprobs):
        score = sum_logprobs / (len(hyp) ** self.length_penalty)
        if len(self) < self.num_beams or score > self.worst_score:
            self.beams.append((score, hyp))
            if len(self) > self.num_beams:
                ranked = sorted((s, i) for i, (s, _) in enumerate(self.beams))
                del self.beams[ranked[0][1]]
                self.worst_score = ranked[1][0]
            else:
                self.worst_score = min(score, self.worst_score)

    def is_done(self, best_sum_logprobs, cur_len):
        if len(self) < self.num_beams:
            return False
        if self.early_stopping:
            return True
        return self.worst_score >= best_sum_logprobs / cur_len ** self.length_penalty


class BeamScorer:
    """The bookkeeping of HF ``BeamSearchScorer`` as of transformers 4.16 (``process`` / ``finalize``) with the
    reference's construction arguments (model.py:505-507: length_penalty 1.0, early stopping off, one hypothesis
    kept per sample).  The reference pins transformers only as ``>=4.16.0`` and the installed 5.x no longer has
    the class, so this is restated from the 4.16 semantics: parity with the reference is UNPINNED.
    Works on host lists; the device tensors are read back once per step, as the HF scorer does (`.item()`)."""

    def __init__(self, batch_size, num_beams, length_penalty=1.0, do_early_stopping=False):
        self.num_beams = num_beams
        self.hyps = [BeamHypotheses(num_beams, length_penalty, do_early_stopping) for _ in range(batch_size)]
        self.done = [False] * batch_size

    @property
    def is_done(self):
        return all(self.done)

    def process(self, input_ids, next_scores, next_tokens, next_indices, pad_token_id, eos_token_id):
        """input_ids: list[B*beams] of token lists; next_*: [B][2*beams] lists.  Returns three flat lists."""
        nb = self.num_beams
        cur_len = len(input_ids[0])
        out_s, out_t, out_i = [], [], []
        for b, hyp in enumerate(self.hyps):
            if self.done[b]:
                out_s += [0.0] * nb; out_t += [pad_token_id] * nb; out_i += [0] * nb
                continue
            kept = 0
            for rank, (tok, sc, idx) in enumerate(zip(next_tokens[b], next_scores[b], next_indices[b])):
                row = b * nb + idx
                if eos_token_id is not None and tok == eos_token_id:
                    if rank >= nb:
                        continue
                    hyp.add(list(input_ids[row]), sc)
                else:
                    out_s.append(sc); out_t.append(tok); out_i.append(row)
                    kept += 1
                if kept == nb:
                    break
            if kept < nb:
                raise ValueError(f"At most {nb} tokens in {next_tokens[b]} can be equal to `eos_token_id`")
            self.done[b] = self.done[b] or hyp.is_done(max(next_scores[b]), cur_len)
        return out_s, out_t, out_i

    def finalize(self, input_ids, final_beam_scores, max_length, pad_token_id, eos_token_id):
        nb = self.num_beams
        for b, hyp in enumerate(self.hyps):
            if self.done[b]:
                continue
            for k in range(nb):
                hyp.add(list(input_ids[b * nb + k]), final_beam_scores[b * nb + k])
        best = [sorted(h.beams, key=lambda x: x[0])[-1][1] for h in self.hyps]
        lengths = [len(h) for h in best]
        width = min(max(lengths) + 1, max_length)
        out = [[pad_token_id] * width for _ in best]
        for i, h in enumerate(best):
            out[i][:len(h)] = h[:width]
            if len(h) < max_length and len(h) < width:
                out[i][len(h)] = eos_token_id
        return out


class BeamDeviceState:
    """Everything ``mvlt_beam_step`` reads and writes for B samples x num_beams beams, in static device buffers, with the prepared
    ``L.MvltBeamStep`` (``self.struct``).  The pool, the flags, the live sequences and the beam scores share ONE allocation, so
    ``finalize`` needs one read-back.  ``cand`` is the int32 [3, B, 2 * num_beams] buffer ``ops.gemm_beam_candidates(out=...)``
    fills; ``cand_log`` (int32 [max_length, B, 3, 2 * num_beams] or None) receives the lists every step consumed."""

    def __init__(self, B, num_beams, max_length, pad, eos, mask_id, device, cand_log=None):
        nb, ml, rows, nc = num_beams, max_length, B * num_beams, 2 * num_beams
        self.B, self.nb, self.max_length, self.pad, self.eos = B, nb, ml, pad, eos
        layout, off = {}, 0
        for name, shape, dt in (("hyp_score", (B, nb + 1), torch.float64), ("worst", (B,), torch.float64), ("col", (1,), torch.int64),
                                ("beam_scores", (rows,), torch.float32), ("hyp_len", (B, nb + 1), torch.int32),
                                ("hyp_tokens", (B, nb + 1, ml), torch.int32), ("n_hyp", (B,), torch.int32), ("done", (B,), torch.int32),
                                ("seq", (rows, ml), torch.int32)):
            n = 1
            for s in shape:
                n *= s
            layout[name] = (off, n * dt.itemsize, shape, dt)
            off += (n * dt.itemsize + 15) // 16 * 16
        self._layout = layout
        self.flat = torch.zeros(off, dtype=torch.uint8, device=device)
        for name, v in self._views(self.flat).items():
            setattr(self, name, v)
        self.slot = torch.zeros((rows, ml), dtype=torch.int32, device=device)
        self.past = torch.zeros(1, dtype=torch.int32, device=device)
        self.ticket = torch.zeros(1, dtype=torch.int32, device=device)
        self.alive = torch.zeros(ml, dtype=torch.int64, device=device)
        self.new_ids = torch.full((rows, 2), mask_id, dtype=torch.int64, device=device)
        self.beam_idx = torch.zeros(rows, dtype=torch.int32, device=device)
        self.cand = torch.zeros((3, B, nc), dtype=torch.int32, device=device)
        self.cand_log = cand_log
        if cand_log is not None:
            assert cand_log.dtype == torch.int32 and cand_log.is_contiguous() and tuple(cand_log.shape) == (ml, B, 3, nc)
        st = self.struct = L.MvltBeamStep()
        st.G, st.num_beams, st.n_cand, st.src_beams, st.max_length = B, nb, nc, nb, ml
        st.has_eos, st.eos_id, st.pad_id, st.mask_id = int(eos is not None), (eos if eos is not None else -1), pad, mask_id
        st.cand_score, st.cand_beam, st.cand_tok = self.cand[0].data_ptr(), self.cand[1].data_ptr(), self.cand[2].data_ptr()
        for name in ("hyp_score", "hyp_len", "hyp_tokens", "n_hyp", "worst", "done", "seq", "slot", "col", "past", "ticket", "alive",
                     "beam_scores", "new_ids", "beam_idx"):
            setattr(st, name, getattr(self, name).data_ptr())
        st.ld_slot = ml
        st.cand_log = cand_log.data_ptr() if cand_log is not None else None
        self.reset(0)

    def _views(self, flat):
        return {name: flat[off:off + nbytes].view(dt).view(shape) for name, (off, nbytes, shape, dt) in self._layout.items()}

    def reset(self, past):
        """Start of a decode: empty pools (worst = 1e9), nothing done, column 0, the cache position of the step before the first
        cached forward (the first beam step advances it)."""
        self.flat.zero_()
        self.worst.fill_(1e9)
        self.slot.zero_(); self.alive.zero_(); self.ticket.zero_()
        self.past.fill_(past)

    def scorer(self):
        """One read-back -> (BeamScorer holding the pools and done flags, live sequences as lists, beam scores as a list)."""
        host = self._views(self.flat.cpu())
        nb = self.nb
        sc = BeamScorer(self.B, nb)
        for b, hyp in enumerate(sc.hyps):
            sc.done[b] = bool(host["done"][b])
            hyp.worst_score = float(host["worst"][b])
            hyp.beams = [(float(host["hyp_score"][b, i]), host["hyp_tokens"][b, i, :int(host["hyp_len"][b, i])].tolist())
                         for i in range(int(host["n_hyp"][b]))]
        n = max(1, min(int(host["col"][0]), self.max_length))
        return sc, host["seq"][:, :n].tolist(), host["beam_scores"].tolist()


class _BeamGraph(_DecodeGraph):
    """Beam search per token as one replayed HIP graph, after the model of ``_GreedyGraph``: [mvlt_beam_step, the 2-token cached
    forward over the B * beams rows, the head transform, (with logit rules: mvlt_beam_rules_plan over the state's live sequences,)
    mvlt_gemm_beam_candidates(_rules)], captured on one stream (no parallel branches).  All state is static: ``BeamDeviceState``, the caches, the hidden rows, the logits workspace.  The captured
    beam step carries src_beams = num_beams also for the lists of step 0 (their beam index is 0, which both values admit)."""

    def __init__(self, model, key, B, nb, n_img, max_length, cd, pad, eos, mask_id, log, rules=(1.0, 0, 0)):
        dev = next(model.parameters()).device
        H = model.config.hidden_size
        rows = B * nb
        self.key, self.model, self.nb, self.cd, self.graph = key, model, nb, cd, None
        self.prefix = n_img + 2
        self.kc, self.vc = _alloc_cache(model, rows, n_img, max_length, cd, dev)
        self.log = torch.zeros((max_length, B, 3, 2 * nb), dtype=torch.int32, device=dev) if log else None
        self.st = BeamDeviceState(B, nb, max_length, pad, eos, mask_id, dev, cand_log=self.log)
        self.hfull = torch.zeros((rows * 2, H), dtype=cd, device=dev)
        self.hlast = self.hfull.view(rows, 2, H)[:, 1]
        V = model.MLM_head_seq2seq.predictions.decoder.out_features
        self.ws = torch.empty(rows * ((V + 3) // 4 * 4), dtype=torch.float32, device=dev)
        # logit rules: the graph owns the bitmaps; the plan reads the live sequences where the beam step writes them (seq, col)
        self.rules = ops.BeamLogitRules(V, *rules, eos, self.st.seq, self.st.col) if rules != (1.0, 0, 0) else None
        self.st.reset(self.prefix - 1)          # a valid position for the warm-up and the capture pass: both really run

    def step(self):
        ops.beam_step(self.st.struct)

    def body(self):
        """The beam step, the cached forward of [kept token, MASK] at positions past, past + 1, the candidates of the next token."""
        model, st = self.model, self.st
        ar = Arena.of(model, self.cd)
        self.step()
        _step2(model.MVLBert, ar, st.new_ids, st.past, self.kc, self.vc, self.cd, out_last=self.hfull, beam=(self.nb, self.prefix, st.slot))
        t2, W, bias = _head(model, ar, self.hlast)
        if self.rules is not None:          # the bitmaps of the reordered histories, then the rule-aware selection
            self.rules.plan()
        ops.gemm_beam_candidates(t2, W, bias, st.beam_scores, self.nb, 2 * self.nb, out=st.cand, ws=self.ws,
                                 rules=self.rules.struct if self.rules is not None else None)


def _beam_device(model, ar, feat, nb, max_length, pad, eos, mask_id, cd, graph_on, cand_log, rules=(1.0, 0, 0)):
    """beam_search with the scorer on the device (``mvlt_beam_step``): no per-token read-back.  ``graph_on``: one graph replay per
    token (``_BeamGraph``), else the eager loop.  The host reads ``alive`` back every 8 tokens; the steps that run past the
    point where every sample is done change no pool (done samples are skipped).  ``finalize`` is the host scorer's."""
    B, n_img, _ = feat.shape
    dev = feat.device
    if graph_on:
        key = (B, nb, n_img, max_length, cd, pad, eos, mask_id, ar.flat.data_ptr(), dev.index, cand_log is not None)
        if rules != (1.0, 0, 0):          # a graph with rules takes the beam graph's slot, like another max_length
            key = key + ("rules",) + tuple(rules)
        bg = _BeamGraph.of(model, "_mvlt_beam_graph", key, B, nb, n_img, max_length, cd, pad, eos, mask_id, cand_log is not None, rules)
        st, kc, vc, ws, lr = bg.st, bg.kc, bg.vc, bg.ws, bg.rules
        if bg.log is not None:
            bg.log.zero_()
    else:
        st = BeamDeviceState(B, nb, max_length, pad, eos, mask_id, dev, cand_log=cand_log)
        kc, vc = _alloc_cache(model, B * nb, n_img, max_length, cd, dev)
        ws = None
        V = model.MLM_head_seq2seq.predictions.decoder.out_features
        lr = ops.BeamLogitRules(V, *rules, eos, st.seq, st.col) if rules != (1.0, 0, 0) else None
    rs = lr.struct if lr is not None else None
    # ---- step 0: the prefix into the first cache row of every sample, the candidates of the one scored row per sample
    hlast, prefix = _step0(model.MVLBert, feat, st.new_ids[::nb, 1:2].contiguous(), kc, vc, stride=nb)
    st.reset(prefix - 1)
    t2, W, bias = _head(model, ar, hlast.contiguous())
    if lr is not None:
        lr.plan(B)                               # one row per sample, column 0: the empty history (only min_length bears)
    ops.gemm_beam_candidates(t2, W, bias, torch.zeros(B, dtype=torch.float32, device=dev), 1, 2 * nb, out=st.cand, ws=ws, rules=rs)

    def all_done(t):          # after the beam step of token t
        return _sync_due(eos, t + 1) and 0 in st.alive[t + 1 - SYNC_EVERY:t + 1].tolist()

    if graph_on:          # a replay: the beam step of token t, then the forward and candidates of token t + 1; last token: the beam step only
        _replay(bg.graph, st.alive, bg.step, max_length, eos)
        if cand_log is not None:
            cand_log.copy_(bg.log)
    else:
        for t in range(max_length):
            ops.beam_step(st.struct, 1 if t == 0 else nb)
            if t + 1 >= max_length or all_done(t):
                break
            hlast = _step2(model.MVLBert, ar, st.new_ids, st.past, kc, vc, cd, beam=(nb, prefix, st.slot))
            t2, W, bias = _head(model, ar, hlast.contiguous())
            if lr is not None:
                lr.plan()
            ops.gemm_beam_candidates(t2, W, bias, st.beam_scores, nb, 2 * nb, out=st.cand, rules=rs)
    scorer, seqs, scores = st.scorer()
    out = scorer.finalize(seqs, scores, model.config.max_length, pad, eos)
    return torch.tensor(out, dtype=torch.int64, device=dev)


def _host_beam_step(scorer, input_ids, cur_len, cands, pad, eos, dev):
    """The host scorer over the candidates ``cands`` = (scores, tokens, beams) of a token, as [B][2 * beams] lists, and the lines
    the reference runs behind it (:743-756) -> (grown hypotheses, beam scores, kept tokens, beam indices: device tensors)."""
    s_l, t_l, i_l = scorer.process(input_ids, *cands, pad, eos)
    input_ids = [[t] for t in t_l] if cur_len == 0 else [input_ids[i] + [t] for i, t in zip(i_l, t_l)]
    return (input_ids, torch.tensor(s_l, dtype=torch.float32, device=dev), torch.tensor(t_l, dtype=torch.int64, device=dev),
            torch.tensor(i_l, dtype=torch.int64, device=dev))


def _beam_fused(model, ar, feat, nb, max_length, pad, eos, mask_id, cd, mask_col, mask2, rules=(1.0, 0, 0)):
    """The default route: candidates from ``mvlt_gemm_beam_candidates``, the cache never reordered (the attention follows the slot
    table), the scorer on the host with one read-back per token."""
    mv = model.MVLBert
    B, n_img, _ = feat.shape
    dev = feat.device
    scorer = BeamScorer(B, nb)
    lr = None
    if rules != (1.0, 0, 0):          # the history the plan reads: the hypotheses' own tokens, kept in step with the beam reorder
        V = model.MLM_head_seq2seq.predictions.decoder.out_features
        hist = torch.zeros((B * nb, max_length), dtype=torch.int32, device=dev)
        lr = ops.BeamLogitRules(V, *rules, eos, hist, torch.zeros(1, dtype=torch.int64, device=dev))

    def candidates(hlast, scores, beams):
        """-> (scores, tokens, beams) of the 2 * nb candidates per sample as host lists: one read-back."""
        t2, W, bias = _head(model, ar, hlast.contiguous())
        if lr is not None:
            lr.plan(t2.shape[0])
        out, _ = ops.gemm_beam_candidates(t2, W, bias, scores, beams, 2 * nb, rules=lr.struct if lr is not None else None)
        host = out.cpu()
        return host[0].view(torch.float32).tolist(), host[2].tolist(), host[1].tolist()

    # ---- step 0 on the B images: only beam 0 of a sample carries score 0 (:681-682), so its candidates are those of ONE row,
    # and the prefix lives in the first row of every sample, once
    kc, vc = _alloc_cache(model, B * nb, n_img, max_length, cd, dev)
    hlast, prefix = _step0(mv, feat, mask_col, kc, vc, stride=nb)
    past = prefix
    own = (torch.arange(B * nb, device=dev) % nb).to(torch.int32)
    slot = torch.zeros((B * nb, max_length), dtype=torch.int32, device=dev)      # [row, generated position] -> cache row in the sample
    cands = candidates(hlast, torch.zeros(B, dtype=torch.float32, device=dev), 1)
    input_ids = [[mask_id] for _ in range(B * nb)]        # what the reference hands the scorer at step 0 (:701-702)
    for cur_len in range(max_length):
        input_ids, beam_scores, beam_tok, beam_idx = _host_beam_step(scorer, input_ids, cur_len, cands, pad, eos, dev)
        if scorer.is_done or cur_len + 1 >= max_length:
            break
        # the beam reorder (model.py:758-763) moves table rows, not cache rows.  A finished sample gets beam_idx 0 (a row of
        # sample 0): only the slot VALUES travel, and the kernel clamps them into the sample
        slot = slot.index_select(0, beam_idx)
        if lr is not None:                               # h of every kept hypothesis: its parent's tokens, then its own
            lr.seq.copy_(lr.seq.index_select(0, beam_idx))
            lr.seq[:, cur_len] = beam_tok
            lr.col.fill_(cur_len + 1)
        hlast = _step2(mv, ar, torch.cat([beam_tok[:, None], mask2], dim=1), past, kc, vc, cd, beam=(nb, prefix, slot))
        slot[:, past - prefix] = own                     # position `past` of every hypothesis now lives in its own row
        past += 1
        cands = candidates(hlast, beam_scores, nb)
    seqs = scorer.finalize(input_ids, beam_scores.tolist(), model.config.max_length, pad, eos)
    return torch.tensor(seqs, dtype=torch.int64, device=dev)


def _rules_torch(logp, hists, rules, eos):
    """The three rules as torch ops on log-probability rows ``logp`` [rows, V] (changed in place and returned): ``hists`` = the
    rows' own generated tokens as host lists of one length c.  The placement of HF 4.16 beam_search, with none of the kernels."""
    penalty, g, min_length = rules
    c = len(hists[0])
    if penalty != 1.0 and c > 0:
        h = torch.tensor(hists, dtype=torch.int64, device=logp.device)
        sc = logp.gather(1, h)
        p = torch.full_like(sc, penalty)                 # a tensor divisor: a Python scalar would be turned into its reciprocal
        logp.scatter_(1, h, torch.where(sc < 0, sc * p, sc / p))
    if g >= 1 and c + 1 >= g:
        rows, cols = [], []
        for m, h in enumerate(hists):
            last = h[c - g + 1:]
            for i in range(c - g + 1):
                if h[i:i + g - 1] == last:
                    rows.append(m); cols.append(h[i + g - 1])
        if rows:
            logp[torch.tensor(rows, device=logp.device), torch.tensor(cols, device=logp.device)] = -float("inf")
    if eos is not None and c < min_length:
        logp[:, eos] = -float("inf")
    return logp


def _beam_plain(model, ar, feat, nb, max_length, pad, eos, mask_id, cd, mask_col, mask2, rules=(1.0, 0, 0)):
    """The route of the reference: bf16 logits, ``log_softmax``, ``topk`` and a gather of every layer's cache by beam index per
    token (model.py:758-763), the scorer on the host."""
    mv = model.MVLBert
    B, n_img, _ = feat.shape
    dev = feat.device
    head = model.MLM_head_seq2seq
    V = head.predictions.decoder.out_features
    scorer = BeamScorer(B, nb)

    def logp_of(hlast):
        t2, _, _ = _head(model, ar, hlast.contiguous())
        logits, _ = head._logits(ar, t2)
        return torch.log_softmax(logits[:, :V].float(), dim=-1)

    on = rules != (1.0, 0, 0)
    # ---- step 0 on the B images; caches replicated to the beams afterwards
    kc, vc = _alloc_cache(model, B, n_img, max_length, cd, dev)
    hlast, past = _step0(mv, feat, mask_col, kc, vc)
    rep = torch.arange(B, device=dev).repeat_interleave(nb)
    kc, vc = [k.index_select(0, rep) for k in kc], [v.index_select(0, rep) for v in vc]
    logp = logp_of(hlast)
    if on:                                                                    # step 0: the empty history of the one scored row
        logp = _rules_torch(logp, [[] for _ in range(B)], rules, eos)
    logp = logp.index_select(0, rep)                                          # [B*nb, V]
    beam_scores = torch.zeros((B, nb), dtype=torch.float32, device=dev)
    beam_scores[:, 1:] = -1e9
    beam_scores = beam_scores.view(-1)
    input_ids = [[mask_id] for _ in range(B * nb)]        # what the reference hands the scorer at step 0 (:701-702)
    for cur_len in range(max_length):
        scores = (logp + beam_scores[:, None]).view(B, nb * V)
        top_s, top_t = torch.topk(scores, 2 * nb, dim=1, largest=True, sorted=True)
        top_i = torch.div(top_t, V, rounding_mode="floor")
        top_t = top_t % V
        cands = top_s.tolist(), top_t.tolist(), top_i.tolist()
        input_ids, beam_scores, beam_tok, beam_idx = _host_beam_step(scorer, input_ids, cur_len, cands, pad, eos, dev)
        if scorer.is_done or cur_len + 1 >= max_length:
            break
        for i in range(len(kc)):                             # beam reorder of the cache (model.py:758-763)
            kc[i] = kc[i].index_select(0, beam_idx)
            vc[i] = vc[i].index_select(0, beam_idx)
        logp = logp_of(_step2(mv, ar, torch.cat([beam_tok[:, None], mask2], dim=1), past, kc, vc, cd))
        if on:                                               # input_ids: the hypotheses' own tokens after the reorder
            logp = _rules_torch(logp, input_ids, rules, eos)
        past += 1
    seqs = scorer.finalize(input_ids, beam_scores.tolist(), model.config.max_length, pad, eos)
    return torch.tensor(seqs, dtype=torch.int64, device=dev)


@torch.no_grad()
def beam_search(model, image_feature, num_beams, learning_strategy='unilm', max_length=None, pad_token_id=None,
                eos_token_id=None, device_scorer=None, cand_log=None, repetition_penalty=1.0, no_repeat_ngram_size=0, min_length=0):
    """``MVLBertForImageCaption.beam_search`` (model.py:636-816) with the KV cache: scores = log_softmax(logits) +
    beam score, top 2*beams over (beam, token), scorer bookkeeping, cache rows gathered by ``beam_idx`` (:758-763).
    Step 0 runs once per image (all beams of a sample start identical and only beam 0 carries score 0, :681-682),
    then 2-token cached steps over the B*beams rows.  Returns the sequences [B, <= max_length] (:795-815).
    ``device_scorer`` (None: MVLT_BEAM_DEVICE=1 switches it on; default off): the scorer bookkeeping runs on the device
    (``mvlt_beam_step``) and the loop has no per-token read-back; as a replayed graph unless MVLT_DECODE_GRAPH=0.  Same shapes as
    the fused route (anything else decodes as without the switch), same sequences.  ``cand_log`` (device-scorer route only): an
    int32 device tensor [max_length, B, 3, 2 * num_beams] that receives the candidate lists every step consumed.
    ``repetition_penalty`` (1.0 = off) / ``no_repeat_ngram_size`` (0 = off) / ``min_length`` (0 = off): HF's three processors where
    transformers 4.16 beam_search places them, on the LOG-PROBABILITIES of a hypothesis ahead of its beam score (greedy_search
    applies them to the raw logits), over the hypothesis' own tokens after the beam reorder.  A banned token is never a
    candidate and stays inside the log-sum-exp.  Every route returns the same sequences in f32 (the plain route applies the
    rules as torch ops, the other two in the candidate head); with all three off the call is the one without them.  The
    vocabulary must hold max(max_length + 2, 2 * num_beams + 1) tokens (ValueError): a row bans at most max_length columns, so
    every sample keeps 2 * num_beams candidates at every step."""
    rules = check_beam_rules(repetition_penalty, no_repeat_ngram_size, min_length, num_beams,
                             model.MLM_head_seq2seq.predictions.decoder.out_features,
                             max_length if max_length is not None else model.config.max_length)
    if learning_strategy != 'unilm':
        raise NotImplementedError("only learning_strategy='unilm' is coherent with the KV cache (SURVEY.md 3.3)")
    cd, ar, max_length, pad, eos, mask_id, feat = _resolve(model, image_feature, max_length, pad_token_id, eos_token_id)
    cfg = model.config
    B, nb = feat.shape[0], num_beams
    # the [MASK] columns of step 0 and of the cached steps (filled ahead of the route; the device route has its own in its state)
    mask_col = torch.full((B, 1), mask_id, dtype=torch.int64, device=feat.device)
    mask2 = torch.full((B * nb, 1), mask_id, dtype=torch.int64, device=feat.device)
    graph_on, fused_on, device_on = _env()
    route = _beam_route(nb, cfg.hidden_size // cfg.num_attention_heads, max_length, fused_on, device_scorer, device_on)
    if route == 'device':
        return _beam_device(model, ar, feat, nb, max_length, pad, eos, mask_id, cd, graph_on, cand_log, rules)
    search = _beam_fused if route == 'fused' else _beam_plain
    return search(model, ar, feat, nb, max_length, pad, eos, mask_id, cd, mask_col, mask2, rules)
