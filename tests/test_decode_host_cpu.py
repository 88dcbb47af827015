"""The host-only rules of mvlt_amd.decode without a GPU: the rule that cuts a greedy decode where the reference's per-token check
would have stopped (against a restatement of that loop, written here), the rule that says when the finished flags are read back,
and the route tables of greedy_search and beam_search at every boundary of their conditions."""
import pytest

from mvlt_amd import decode, ops

ML = 20          # max_length of the cut-rule cases: three read-backs (columns 8, 16 and the last)


def _reference_loop(unfinished_after, max_length):
    """model.py:940-960 on the flags alone: append the id, stop if no sample is alive, otherwise append the score.
    ``unfinished_after[c]``: whether any sample is unfinished after column c (None: no eos, the check never fires)."""
    ids, scores = 0, 0
    for c in range(max_length):
        ids += 1
        if unfinished_after is not None and not unfinished_after[c]:
            break
        scores += 1
    return ids, scores


def _polled_decode(unfinished_after, max_length, last=None):
    """What the loops do with the two rules: produce columns, read the flags back when ``_sync_due`` says so (a block of the last
    SYNC_EVERY columns), stop at a block holding a 0, cut with ``_cut``.  ``last`` = max_length: the eager greedy loop, which also
    reads at the last column; None: the graph loop, which reads every column it produced once it is through.
    Returns ((n_out, n_scores), columns produced)."""
    eos = None if unfinished_after is None else 2
    flags, done = [], 0
    while done < max_length:
        done += 1
        if decode._sync_due(eos, done, last):
            block = [int(f) for f in unfinished_after[max(0, done - decode.SYNC_EVERY):done]]
            flags[done - len(block):] = block
            if 0 in block:
                break
    if last is None and eos is not None:
        flags = [int(f) for f in unfinished_after[:done]]
    return decode._cut(flags, done), done


def _flags(first_zero, max_length=ML):
    return [c < first_zero for c in range(max_length)]


@pytest.mark.parametrize("last", [None, ML], ids=["graph", "eager"])
@pytest.mark.parametrize("first_zero", [0, 5, 7, 8, 11, 15, 16, ML - 1, ML], ids=lambda z: f"zero_at_{z}")
def test_cut_rule_equals_the_per_token_loop(first_zero, last):
    """First 0 at column 0, in the middle of a block, at a block's last and first column, at the last column, and nowhere (all
    alive through max_length).  Columns 5 and 11 are seen only when their block is read back, columns later."""
    alive = _flags(first_zero)
    got, produced = _polled_decode(alive, ML, last)
    assert got == _reference_loop(alive, ML)
    if first_zero in (5, 11):
        assert produced == (first_zero // 8 + 1) * 8 > first_zero + 1          # the loop ran on until the read-back


def test_cut_rule_without_eos():
    assert _polled_decode(None, ML) == ((ML, ML), ML) and _reference_loop(None, ML) == (ML, ML)
    assert decode._cut([], 0) == (0, 0)


def test_cut_rule_on_plain_lists():
    assert decode._cut([1, 1, 1], 3) == (3, 3)
    assert decode._cut([0, 0, 0], 3) == (1, 0)
    assert decode._cut([1, 1, 0, 0], 8) == (3, 2)          # found in a block read back late: 8 columns were produced
    assert decode._cut([1, 1, 1, 0], 4) == (4, 3)


def test_sync_rule():
    due = [d for d in range(1, 21) if decode._sync_due(2, d)]
    assert due == [8, 16] and decode.SYNC_EVERY == 8
    assert [d for d in range(1, 21) if decode._sync_due(2, d, last=20)] == [8, 16, 20]
    assert decode._sync_due(0, 8)                                                  # token id 0 is an eos
    assert not any(decode._sync_due(None, d, last=20) for d in range(1, 21))


@pytest.mark.parametrize("args, route", [
    (('greedy', 64, False, True), ('graph', 'greedy')),
    (('greedy', 65, False, True), ('eager', 'argmax')),
    (('greedy', 64, False, False), ('eager', 'gemm_argmax')),
    (('greedy', 65, False, False), ('eager', 'argmax')),
    (('sample', 64, False, True), ('graph', 'sample')),
    (('sample', 65, False, True), ('eager', 'multinomial')),
    (('sample', 64, False, False), ('eager', 'gemm_sample')),
    (('sample', 65, False, False), ('eager', 'multinomial')),
    (('sample', 64, True, True), ('graph', 'sample')),
    (('sample', 65, True, True), ('eager', 'filtered')),
    (('sample', 70, True, True), ('eager', 'filtered')),
    (('sample', 3, True, False), ('eager', 'filtered')),
    (('sample', 70, True, False), ('eager', 'filtered')),
])
def test_greedy_route_table(args, route):
    assert decode._greedy_route(*args) == route


@pytest.mark.parametrize("graph_on", [True, False])
def test_greedy_route_refusals(graph_on):
    with pytest.raises(ValueError, match="need sample_mode='sample'"):
        decode._greedy_route('greedy', 3, True, graph_on)
    with pytest.raises(ValueError, match="sample mode error!"):
        decode._greedy_route('beam', 3, False, graph_on)


# (B, n_img, max_length, cd, pad, eos, mask_id, address of the weights, device index): what every graph key starts from
_KEY = (3, 49, 8, "bf16", 0, None, 103, 1234, 0)
_RULES = (1.2, 3, 10)


@pytest.mark.parametrize("kw, slot, key", [
    (dict(), "_mvlt_greedy_graph", (3, 49, 8, "bf16", 0, None, 103, 1234, 0)),
    (dict(mode='sample', temperature=0.8), "_mvlt_sample_graph", (3, 49, 8, "bf16", 0, None, 103, 1234, 0, 'sample', 0.8)),
    (dict(mode='sample', temperature=2, top_k=5, top_p=0.9), "_mvlt_sample_graph", (3, 49, 8, "bf16", 0, None, 103, 1234, 0, 'sample', 2.0, 5, 0.9)),
    (dict(rules=_RULES), "_mvlt_greedy_graph", (3, 49, 8, "bf16", 0, None, 103, 1234, 0, "rules", 1.2, 3, 10)),
    (dict(p_max=6), "_mvlt_prompt_graph", (3, 49, 8, "bf16", 0, None, 103, 1234, 0, "prompt", 66)),
    (dict(p_max=0), "_mvlt_prompt_graph", (3, 49, 8, "bf16", 0, None, 103, 1234, 0, "prompt", 60)),          # an empty prompt is a prompt
    (dict(mode='sample', temperature=0.8, p_max=6), "_mvlt_prompt_sample_graph", (3, 49, 8, "bf16", 0, None, 103, 1234, 0, 'sample', 0.8, "prompt", 66)),
    (dict(mode='sample', temperature=0.8, top_k=5, top_p=0.9, rules=_RULES, p_max=6), "_mvlt_prompt_sample_graph",
     (3, 49, 8, "bf16", 0, None, 103, 1234, 0, 'sample', 0.8, 5, 0.9, "rules", 1.2, 3, 10, "prompt", 66)),
    (dict(S=3), "_mvlt_multi_sample_graph", (3, 3, 49, 8, "bf16", 0, None, 103, 1234, 0)),
    (dict(S=3, rules=_RULES), "_mvlt_multi_sample_graph", (3, 3, 49, 8, "bf16", 0, None, 103, 1234, 0, "rules", 1.2, 3, 10)),
], ids=["greedy", "sampled", "sampled+filter", "greedy+rules", "prompted", "empty-prompt", "prompted-sampled", "prompted-all", "multi", "multi+rules"])
def test_graph_slot_and_key(kw, slot, key):
    """The slot names and the key tuples as the loops built them before they shared ``_graph_slot_key``, written out: the key
    starts with B, a prompted key ends with the cache capacity (n_img + 2 + p_max + max_length + 1), the multi-sample key holds S
    and neither the temperature nor the split of S."""
    got = decode._graph_slot_key(*_KEY, **kw)
    assert got == (slot, key)
    assert type(got[1][10]) is float if kw.get("mode") == 'sample' else True          # float(temperature): 2 and 2.0 are one key


@pytest.mark.parametrize("args, route", [
    # (num_beams, head_dim, max_length, fused_on, device_scorer, device_on)
    ((8, 64, 150, True, False, False), 'fused'),
    ((9, 64, 150, True, False, False), 'plain'),
    ((0, 64, 150, True, False, False), 'plain'),
    ((1, 64, 150, True, False, False), 'fused'),
    ((5, 32, 150, True, False, False), 'plain'),
    ((5, 64, 150, False, False, False), 'plain'),
    ((8, 64, 150, True, True, False), 'device'),
    ((9, 64, 150, True, True, False), 'plain'),
    ((5, 32, 150, True, True, False), 'plain'),
    ((8, 64, 1024, True, True, False), 'device'),          # nb * max_length = 8192
    ((1, 64, 8193, True, True, False), 'fused'),           # 8193
    ((8, 64, 1025, True, True, False), 'fused'),
    ((5, 64, 150, False, True, False), 'plain'),           # fused switched off: no device scorer either
    ((5, 64, 150, False, True, True), 'plain'),
    ((5, 64, 150, True, None, True), 'device'),            # None follows the env value
    ((5, 64, 150, True, None, False), 'fused'),
    ((5, 64, 150, True, False, True), 'fused'),            # an explicit False beats the env value
    ((5, 64, 150, True, True, False), 'device'),
])
def test_beam_route_table(args, route):
    assert decode.BEAM_STEP_STAGE == 8192 and (ops.BEAM_MAX_BEAMS, ops.BEAM_MAX_CAND) == (8, 16)
    assert decode._beam_route(*args) == route


def test_switches_are_read_per_call(monkeypatch):
    for name in ("MVLT_DECODE_GRAPH", "MVLT_BEAM_FUSED", "MVLT_BEAM_DEVICE"):
        monkeypatch.delenv(name, raising=False)
    assert decode._env() == (True, True, False)
    monkeypatch.setenv("MVLT_DECODE_GRAPH", "0")
    monkeypatch.setenv("MVLT_BEAM_FUSED", "0")
    monkeypatch.setenv("MVLT_BEAM_DEVICE", "1")
    assert decode._env() == (False, False, True)
