"""Cost of parameter groups in the AdamW sweep on config #2 (the bench.py replica: B = 32, T = 80, bf16, train mode; 182 M updated
parameters), over the runs of the live gradient set of one real step.  Three arms, in ONE process, in alternating order
(a b c a b c ...), every arm timed with HIP events around its own launches:

  (a) plain     mvlt_adamw per run of the plan: what the optimizer launches without param_groups
  (b) grouped   mvlt_adamw_groups per run of the plan with no_decay_rules() + a backbone lr_scale (four groups): the same number
                of launches, the groups resolved inside the kernel
  (c) split     the same four groups as ONE mvlt_adamw launch per maximal same-group piece of every run -- the alternative the
                design rejects; its launch count and host enqueue time (a host clock around the launch loop, nothing synchronised
                inside) are what it costs

    python scripts/adamw_groups_time.py [--rounds 9] [--reps 20]
prints one JSON line per arm and round, then one summary line per arm (median, min, max over the rounds)."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    import mvlt_amd as M
    from mvlt_amd import ops
    from mvlt_amd.arena import ALIGN, Arena
    from mvlt_amd.ddp import seed_coin_flip
    from mvlt_amd.optim import no_decay_rules, param_groups_by_name
    from mvlt_amd.runtime import compute_dtype_of
    from mvlt_amd.train import PretrainStep, synthetic_batch

    torch.manual_seed(1234)
    cfg = M.MVLBertPretrainConfig()
    cfg.ITM_task = True
    cfg.mlm_max_labels_per_sample = None
    model = M.MVLBertForPretraining(cfg).cuda().train()
    groups = param_groups_by_name(model, [(r"^conv\.", dict(lr_scale=0.1))] + no_decay_rules())
    step = PretrainStep(model, param_groups=groups)
    batch = synthetic_batch(32, 80, "cuda", 1234)[:4]
    M.manual_seed(4321)
    seed_coin_flip(5678)
    for _ in range(5):
        step(batch)
    torch.cuda.synchronize()

    opt = step.opt
    ar = Arena.of(model, compute_dtype_of(model))
    plan = opt._plan_runs(ar, [p for p in ar.params if ar.has_grad[id(p)]])
    live = sum(hi - lo for lo, hi, _ in plan)
    t = opt._group_tables(ar)
    bmap = t["map"].cpu()
    scale, decay = t["lr_scale"].tolist(), t["weight_decay"].tolist()
    pieces = []                       # (lo, hi, group): maximal same-group pieces of every run
    for lo, hi, _ in plan:
        ids = bmap[lo // ALIGN:hi // ALIGN].tolist()
        a = 0
        for b in range(1, len(ids) + 1):
            if b == len(ids) or ids[b] != ids[a]:
                pieces.append((lo + a * ALIGN, lo + b * ALIGN, ids[a]))
                a = b
    LR, HYPER = 0.0, (0.9, 0.999, 1e-6)          # lr = 0: the probe leaves the parameters where they are

    def bufs(lo, hi):
        return (ar.flat[lo:hi], ar.grad[lo:hi], ar.exp_avg[lo:hi], ar.exp_avg_sq[lo:hi], ar.shadow[lo:hi] if ar.shadow is not None else None)

    def plain():
        for lo, hi, _ in plan:
            ops.adamw(*bufs(lo, hi), LR, *HYPER, opt.weight_decay, 100, 1.0)
        return len(plan)

    def grouped():
        for lo, hi, _ in plan:
            ops.adamw_groups(*bufs(lo, hi), t["map"][lo // ALIGN:hi // ALIGN], t["lr_scale"], t["weight_decay"], LR, *HYPER, 100, 1.0)
        return len(plan)

    def split():
        for lo, hi, g in pieces:
            ops.adamw(*bufs(lo, hi), LR * scale[g], *HYPER, decay[g], 100, 1.0)
        return len(pieces)

    arms = (("plain", plain), ("grouped", grouped), ("split", split))
    for _, fn in arms:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    seen = {name: dict(ms=[], host_ms=[]) for name, _ in arms}
    for r in range(args.rounds):
        for name, fn in arms:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            t0 = time.perf_counter()
            for _ in range(args.reps):
                launches = fn()
            host = 1e3 * (time.perf_counter() - t0) / args.reps
            e1.record()
            torch.cuda.synchronize()
            ms = e0.elapsed_time(e1) / args.reps
            seen[name]["ms"].append(ms)
            seen[name]["host_ms"].append(host)
            print(json.dumps(dict(round=r, arm=name, launches=launches, ms=round(ms, 4), host_enqueue_ms=round(host, 4),
                                  tb_per_s=round(30 * live / ms / 1e9, 3))), flush=True)
    for name, _ in arms:
        ms, host = seen[name]["ms"], seen[name]["host_ms"]
        print(json.dumps(dict(summary=name, runs=len(plan), pieces=len(pieces), groups=len(scale), live_elements=live,
                              ms_median=round(statistics.median(ms), 4), ms_min=round(min(ms), 4), ms_max=round(max(ms), 4),
                              host_enqueue_ms_median=round(statistics.median(host), 4),
                              tb_per_s_median=round(30 * live / statistics.median(ms) / 1e9, 3))), flush=True)


if __name__ == "__main__":
    main()
