"""Host side of the mvlt_beam_step tests: synthetic candidate streams and a driver that runs decode.BeamScorer over them exactly as
decode.beam_search does (process, then the beam_scores / input_ids lines behind it).  No GPU, no kernels.

A stream is a list of steps; a step is (scores, beams, tokens), each [G][2 * num_beams]: scores are f32 values (as Python floats)
sorted descending, (beam, token) pairs are distinct within a sample, the beams of step 0 are all 0 (one row per sample was
scored).  A sample follows one of the plans below; `coverage` checks, on the driver's own output, that a plan did what it is for."""
import struct

import numpy as np

VOCAB, EOS, PAD, MASK = 50, 7, 0, 3


def _sample_step(rng, nb, t, top, gaps, eos_ranks, equal):
    """One sample's lists: scores = top - cumulative gaps (f32), ranks listed in `equal` repeat the score of the rank before, EOS at
    `eos_ranks` (each on a beam of its own, so the pairs stay distinct)."""
    n = 2 * nb
    scores, cur = [], np.float32(top)
    for r in range(n):
        if r and r not in equal:
            cur = np.float32(cur - np.float32(gaps[r]))
        scores.append(float(cur))
    assert all(a >= b for a, b in zip(scores, scores[1:]))
    eos_ranks = sorted({r for r in eos_ranks if r < n})
    assert len(eos_ranks) <= (1 if t == 0 else nb)
    eos_beams = iter(rng.permutation(nb).tolist())
    # distinct (beam, non-EOS token) pairs; step 0 has one beam, so there the tokens themselves are distinct
    flat = rng.choice((1 if t == 0 else nb) * (VOCAB - 1), size=n, replace=False).tolist()
    beams, toks = [], []
    for r in range(n):
        if r in eos_ranks:
            beams.append(0 if t == 0 else next(eos_beams)); toks.append(EOS)
        else:
            tok = flat[r] % (VOCAB - 1)
            beams.append(0 if t == 0 else flat[r] // (VOCAB - 1)); toks.append(tok if tok < EOS else tok + 1)
    assert len({(b, k) for b, k in zip(beams, toks)}) == n
    return scores, beams, toks


# plan(nb, t) -> (top score, EOS ranks, ranks whose score repeats the one before; "all-dyadic" gaps when the plan needs exact ties)
def plan_eos0(nb, t):
    """[END] at rank 0 of step 0 (the [mask_id] hypothesis), one more later."""
    return -1.0 - t, ([0] if t in (0, 2) else []), [], False


def plan_skipped(nb, t):
    """[END] only at ranks >= num_beams: skipped, the sample never finishes."""
    return -0.5 - 0.75 * t, ([nb, 2 * nb - 1] if t else [nb]), [nb + 1] if nb > 1 else [], False


def plan_overflow(nb, t):
    """The pool fills with bit-equal scores at step 1 (-2 / 1), step 2 offers -3 / 2 = -1.5 num_beams - 1 times: every offer beats
    `worst` and evicts the tied entry with the lowest insertion index.  Rank 0 is never [END], so the sample is not done."""
    if t in (1, 2):
        return -1.0, list(range(1, nb)), list(range(2, nb)), True
    return -0.5 - 0.01 * t, [], [], False          # (a top score that keeps best / L above `worst`: never done)


def plan_done2(nb, t):
    """num_beams bit-equal [END] candidates at ranks 0 .. num_beams - 1 of step 2: the pool is full and worst == best / 2: done."""
    if t == 2:
        return -3.0, list(range(nb)), list(range(1, nb)), True
    return -1.0 - 0.5 * t, [], [], False


def plan_none(nb, t):
    return -0.25 - 1.25 * t, [], ([2] if nb > 1 else []), False


PLANS = dict(eos0=plan_eos0, skipped=plan_skipped, overflow=plan_overflow, done2=plan_done2, none=plan_none)


def make_stream(plans, nb, max_length, seed):
    """plans: one plan name per sample -> max_length steps."""
    rng = np.random.default_rng(seed)
    steps = []
    for t in range(max_length):
        rows = []
        for name in plans:
            top, eos_ranks, equal, dyadic = PLANS[name](nb, t)
            if t == 0:
                eos_ranks = eos_ranks[:1]
            if dyadic:          # -1 at rank 0, then one step of 1 (step 1) or 2 (step 2) down to the tied block, then eighths
                gaps = [0.0] + [0.125] * (2 * nb - 1)
                if name == "overflow":
                    gaps[1] = 1.0 if t == 1 else 2.0
            else:
                gaps = rng.uniform(0.01, 0.5, size=2 * nb).tolist()
            rows.append(_sample_step(rng, nb, t, top, gaps, eos_ranks, equal))
        steps.append(tuple([r[i] for r in rows] for i in range(3)))
    return steps


def cases():
    """(id, plans, num_beams, max_length, has_eos, seed): G in {1, 3}, num_beams in {1, 2, 5, 8}, max_length in {4, 12}."""
    out = []
    seed = 100
    for nb in (1, 2, 5, 8):
        for ml in (4, 12):
            out.append((f"G3-nb{nb}-ml{ml}", ("done2", "skipped", "overflow"), nb, ml, True, seed)); seed += 1
            out.append((f"G3b-nb{nb}-ml{ml}", ("eos0", "none", "done2"), nb, ml, True, seed)); seed += 1
        out.append((f"G1-eos0-nb{nb}", ("eos0",), nb, 4, True, seed)); seed += 1
        out.append((f"G1-overflow-nb{nb}", ("overflow",), nb, 12, True, seed)); seed += 1
        out.append((f"G1-noeos-nb{nb}", ("done2",), nb, 4, False, seed)); seed += 1          # has_eos = 0: [END] is a token like any other
        out.append((f"G3-noeos-nb{nb}", ("eos0", "overflow", "done2"), nb, 12, False, seed)); seed += 1
    return out


def f64_bits(v):
    return struct.unpack("<q", struct.pack("<d", float(v)))[0]


def f32_bits(v):
    return struct.unpack("<i", struct.pack("<f", float(v)))[0]


def drive(BeamScorer, stream, G, nb, max_length, eos, pad=PAD, mask=MASK):
    """decode.beam_search's host loop over a stream, for every step of it (a done sample emits pad / 0 / 0, as `process` does).
    -> dict(steps = [(scores, tokens, rows, done flags)], pools = [[(score, tokens)]], worst, seqs (input_ids at the end),
    final = finalize's output)."""
    scorer = BeamScorer(G, nb)
    input_ids = [[mask] for _ in range(G * nb)]
    steps = []
    s_l = [0.0] * (G * nb)
    for t, (scores, beams, toks) in enumerate(stream):
        s_l, t_l, i_l = scorer.process(input_ids, scores, toks, beams, pad, eos)
        input_ids = [[k] for k in t_l] if t == 0 else [input_ids[i] + [k] for i, k in zip(i_l, t_l)]
        steps.append((list(s_l), list(t_l), list(i_l), list(scorer.done)))
    pools = [[(s, list(h)) for s, h in hyp.beams] for hyp in scorer.hyps]
    worst = [hyp.worst_score for hyp in scorer.hyps]
    seqs = [list(r) for r in input_ids]
    final = scorer.finalize(input_ids, s_l, max_length, pad, eos)
    return dict(steps=steps, pools=pools, worst=worst, seqs=seqs, final=final)


def first_done(res, g):
    for t, st in enumerate(res["steps"]):
        if st[3][g]:
            return t
    return None


def coverage(BeamScorer):
    """Every property the streams are there for, checked on the driver's output: [mask_id] hypothesis, skipped [END], eviction among
    tied scores, done at step 2 beside a sample that never finishes, has_eos = 0, a run that ends at max_length."""
    seen = set()
    for cid, plans, nb, ml, has_eos, seed in cases():
        stream = make_stream(plans, nb, ml, seed)
        res = drive(BeamScorer, stream, len(plans), nb, ml, EOS if has_eos else None)
        assert len(res["steps"]) == ml
        for g, name in enumerate(plans):
            fd = first_done(res, g)
            if not has_eos:
                assert fd is None and all(len(h) == ml for _, h in res["pools"][g]), cid
                seen.add("noeos")
                continue
            if name == "eos0" and nb > 1:
                assert any(h == [MASK] for _, h in res["pools"][g]) or fd is not None, cid
                seen.add("mask-hyp")
            if name == "eos0" and nb == 1:
                assert fd == 0 and res["pools"][g][0][1] == [MASK], cid
                seen.add("mask-hyp")
            if name == "skipped":
                assert fd is None and len(res["seqs"][g * nb]) == ml, cid
                seen.add("skipped"); seen.add("max-length")
            if name == "done2":
                assert fd == 2, (cid, fd)
                if "skipped" in plans:
                    seen.add("done2-beside-live")
            if name == "overflow" and nb > 1 and fd is None:
                sc = [s for s, _ in res["pools"][g]]
                assert len(sc) == nb and sc.count(-1.5) >= nb - 1, (cid, sc)          # the offers of step 2 pushed the -2.0 entries out
                seen.add("tied-eviction")
    assert seen == {"noeos", "mask-hyp", "skipped", "max-length", "done2-beside-live", "tied-eviction"}, seen
