"""Sequence loss (self-critical fine-tuning): the two measurements of profiles/seq_loss.md.  PART=kernel | step | all (default).

kernel: mvlt_ce_bwd_weighted against mvlt_ce_bwd_ragged -- the existing kernel, one scalar for all rows -- at ROWS x V (4800 x
  30522, ld 30528) bf16, in place.  Three arms run interleaved, window by window: ragged (a), weighted, ragged (b); a window is
  CALLS back-to-back calls between two HIP events, the logits are restored from a master copy ahead of every window (untimed).
  The difference between the two ragged arms is the spread the existing kernel shows against itself; the weighted arm is
  expected inside it.  Bytes = rows x ld x 2 B read + the same written; GB/s = bytes / time.  ROUNDS (40), CALLS (5).

step: one self_critical_loss + backward on the full-size caption model (Swin-S + BERT-base, bf16, train mode), B (32) images,
  MAXLEN (150), references = the model's own greedy reports (random weights agree with no other text; every advantage is then
  non-zero), split into tower, greedy decode, sampled decode, scoring, teacher-forced forward + backward (a host clock around
  each part, every part ending in a device synchronise), and the whole call.  Baseline: the same loss from the pieces the
  project had before -- logits [B, V, T] from forward(image, ids, 0, 'unilm') into torch, log_softmax, gather, weights, mask --
  on the same sampled ids; it runs the tower itself, so it is set against tower + teacher-forced part.  Time and peak allocated
  memory for both.  STEP_ROUNDS (3 timed after 1 warm-up)."""
import os, statistics, sys, time
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mvlt_amd as M                      # noqa: E402
from mvlt_amd import decode, ops, report_metrics as RM  # noqa: E402

assert torch.cuda.is_available(), "seq_loss_bench.py measures on the GPU only"
PART = os.environ.get("PART", "all")


def kernel_part():
    rows, V = int(os.environ.get("ROWS", 4800)), int(os.environ.get("V", 30522))
    rounds, calls = int(os.environ.get("ROUNDS", 40)), int(os.environ.get("CALLS", 5))
    ld = (V + 63) // 64 * 64
    g = torch.Generator(device="cuda").manual_seed(0)
    master = (3.0 * torch.randn(rows, ld, device="cuda", generator=g)).to(torch.bfloat16)
    labels = torch.randint(0, V, (rows,), device="cuda", generator=g)
    lse = torch.logsumexp(master[:, :V].float(), 1)
    w = torch.randn(rows, device="cuda", generator=g)
    acc = torch.tensor([0.0, float(rows)], device="cuda")
    gs = torch.ones(1, device="cuda")
    rd = torch.tensor([rows], dtype=torch.int32, device="cuda")
    x = master.clone()
    arms = {"ragged (a)": lambda: ops.ce_bwd(x, V, labels, lse, acc, grad_scale_dev=gs, rows_dev=rd),
            "weighted": lambda: ops.ce_bwd_weighted(x, V, labels, lse, w, acc, grad_scale_dev=gs, rows_dev=rd),
            "ragged (b)": lambda: ops.ce_bwd(x, V, labels, lse, acc, grad_scale_dev=gs, rows_dev=rd)}
    # the two kernels compute the same numbers where the weights are 1 (the timed runs use random weights)
    ones = torch.ones(rows, device="cuda")
    a = ops.ce_bwd(master.clone(), V, labels, lse, acc, grad_scale_dev=gs, rows_dev=rd)
    b = ops.ce_bwd_weighted(master.clone(), V, labels, lse, ones, acc, grad_scale_dev=gs, rows_dev=rd)
    same = torch.equal(a[:, :V].view(torch.int16), b[:, :V].view(torch.int16))
    ms = {k: [] for k in arms}
    for r in range(rounds + 2):                                   # two warm-up rounds
        for name, fn in arms.items():
            x.copy_(master)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                fn()
            e1.record()
            torch.cuda.synchronize()
            if r >= 2:
                ms[name].append(e0.elapsed_time(e1) / calls)
    gb = 2.0 * rows * ld * 2 / 1e9
    print(f"kernel: {rows} x {V} (ld {ld}) bf16 in place, {rounds} windows of {calls} calls per arm, interleaved; "
          f"{gb:.3f} GB moved per call; unit weights bit-identical to ragged: {same}")
    med = {}
    for name, v in ms.items():
        v = sorted(v)
        med[name] = statistics.median(v)
        q1, q3 = v[len(v) // 4], v[(3 * len(v)) // 4]
        print(f"  {name:11s} median {med[name] * 1e3:8.1f} us  (min {v[0] * 1e3:.1f}, quartiles {q1 * 1e3:.1f} .. {q3 * 1e3:.1f}, max {v[-1] * 1e3:.1f})"
              f"  {gb / (med[name] * 1e-3):7.0f} GB/s")
    spread = abs(med["ragged (a)"] - med["ragged (b)"])
    ragged = 0.5 * (med["ragged (a)"] + med["ragged (b)"])
    diff = med["weighted"] - ragged
    print(f"  ragged against itself: {spread * 1e3:.1f} us between the medians of its two arms; weighted - ragged: {diff * 1e3:+.1f} us "
          f"({100 * diff / ragged:+.1f} %): {'inside' if diff <= spread else 'OUTSIDE (slower than)'} that spread", flush=True)


def timed(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    t = time.time()
    out = fn()
    torch.cuda.synchronize()
    return (time.time() - t) * 1e3, torch.cuda.max_memory_allocated() / 2 ** 30, out


def step_part():
    B, maxlen = int(os.environ.get("B", 32)), int(os.environ.get("MAXLEN", 150))
    rounds = int(os.environ.get("STEP_ROUNDS", 3))
    torch.manual_seed(0)
    cfg = M.MVLBertConfigForImageCaption()
    tok = type("Tok", (), {"mask_token_id": 103, "sep_token_id": 102})()
    model = M.set_compute_dtype(M.MVLBertForImageCaption(cfg, tokenizer=tok).cuda().train(), torch.bfloat16)
    M.manual_seed(1)
    from mvlt_amd.arena import Arena
    Arena.of(model, torch.bfloat16)                     # what forward() / generate() do ahead of the tower
    g = torch.Generator().manual_seed(2)
    image = torch.randn(B, 3, 224, 224, generator=g).cuda()
    # a model with random weights agrees with no text: its own greedy reports are the references, so the greedy reward is
    # high, the sampled one is not, and every advantage is non-zero (a zero-weight row would skip the backward's exponentials)
    with torch.no_grad():
        own = decode.greedy_search(model, model.conv(image), max_length=maxlen)[0]
    refs = RM.ReferenceSet(own)
    index = torch.arange(B)
    eos = cfg.eos_token_id
    opts = dict(seed=7, temperature=1.0, top_k=0, top_p=1.0)

    def zero():
        for p in model.parameters():
            p.grad = None

    def split():
        out = {}
        out["tower"] = timed(lambda: model.conv(image))
        feat = out["tower"][2]
        det = feat.detach()
        out["greedy decode"] = timed(lambda: decode.greedy_search(model, det, max_length=maxlen)[0])
        out["sampled decode"] = timed(lambda: decode.greedy_search(model, det, sample_mode="sample", max_length=maxlen, **opts)[0])
        gi, si = out["greedy decode"][2], out["sampled decode"][2]
        out["scoring"] = timed(lambda: (RM.score(si, refs, index)["cider"] - RM.score(gi, refs, index)["cider"]).float())
        adv = out["scoring"][2]

        def tf():
            loss = model.sequence_loss_from_features(feat, si, adv)
            loss.backward()
            return loss
        out["teacher-forced forward + backward"] = timed(tf)
        zero()
        return out, si, adv

    def whole():
        loss, _ = M.self_critical_loss(model, image, refs, index, max_length=maxlen, **opts)
        loss.backward()
        return loss

    def baseline(si, adv):
        # the parent's public pieces: logits into torch, the cut at [END] / PAD with tensor ops (no host loop)
        end = (si == eos) if eos is not None else torch.zeros_like(si, dtype=torch.bool)
        stop = end | (si <= 0)
        first = torch.where(stop.any(1), stop.float().argmax(1), torch.full((si.shape[0],), si.shape[1], device=si.device))
        lens = torch.where(stop.any(1) & end.gather(1, first.clamp(max=si.shape[1] - 1)[:, None])[:, 0], first + 1, first)
        mask = torch.arange(si.shape[1], device=si.device)[None, :] < lens[:, None]
        tf_ids = torch.where(mask, si, torch.zeros_like(si))
        logits = model(image, tf_ids, 0, "unilm")                                   # [B, V, T]
        logp = torch.log_softmax(logits.float(), 1).gather(1, si.clamp(min=0)[:, None, :])[:, 0]
        loss = -(adv[:, None] * logp * mask).sum() / mask.sum()
        loss.backward()
        return loss

    parts, totals, base = {}, [], []
    for r in range(rounds + 1):
        out, si, adv = split()
        t_whole = timed(whole)
        zero()
        t_base = timed(lambda: baseline(si, adv))
        zero()
        if r:
            for k, v in out.items():
                parts.setdefault(k, []).append(v[:2])
            totals.append(t_whole[:2] + (float(t_whole[2].detach()),))
            base.append(t_base[:2] + (float(t_base[2].detach()),))
        lens_note = f"sampled ids [{si.shape[0]}, {si.shape[1]}], {int((adv != 0).sum())} of {B} advantages non-zero"
    mean = lambda v: sum(v) / len(v)
    print(f"step: B = {B}, max_length = {maxlen}, bf16, train mode, {rounds} timed rounds after 1 warm-up; {lens_note}")
    for k, v in parts.items():
        print(f"  {k:34s} {mean([a for a, _ in v]):9.1f} ms  (min {min(a for a, _ in v):.1f} max {max(a for a, _ in v):.1f})  peak {max(b for _, b in v):.2f} GiB")
    print(f"  {'self_critical_loss + backward':34s} {mean([a for a, _, _ in totals]):9.1f} ms  (min {min(a for a, _, _ in totals):.1f} "
          f"max {max(a for a, _, _ in totals):.1f})  peak {max(b for _, b, _ in totals):.2f} GiB  loss {totals[-1][2]:.6f}")
    ours = mean([a for a, _ in parts["tower"]]) + mean([a for a, _ in parts["teacher-forced forward + backward"]])
    print(f"  {'baseline: logits into torch + bwd':34s} {mean([a for a, _, _ in base]):9.1f} ms  (min {min(a for a, _, _ in base):.1f} "
          f"max {max(a for a, _, _ in base):.1f})  peak {max(b for _, b, _ in base):.2f} GiB  loss {base[-1][2]:.6f}   "
          f"[against tower + teacher-forced part: {ours:.1f} ms]", flush=True)


if PART in ("kernel", "all"):
    kernel_part()
if PART in ("step", "all"):
    step_part()
