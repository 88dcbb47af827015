"""Cost of FusedAdamW(max_grad_norm=, skip_nonfinite=) on config #2 (the bench.py replica: B = 32, T = 80, bf16, train mode).

1. stand-alone: mvlt_grad_sumsq + mvlt_grad_norm_finish over the runs of the live gradient set of one step (HIP events around
   `reps` repetitions), beside the plain and the guarded AdamW sweep over the same runs;
2. the step: PretrainStep with the options off / clip / clip + skip, interleaved in rounds in ONE process (same box, same
   minute), ms per step from a host clock around `steps` steps that end in a device synchronise.

    python scripts/grad_clip_ab.py [--rounds 5] [--steps 40] [--reps 50]
prints one JSON line per measurement."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--reps", type=int, default=50)
    args = ap.parse_args()
    import mvlt_amd as M
    from mvlt_amd import ops
    from mvlt_amd.arena import Arena
    from mvlt_amd.ddp import seed_coin_flip
    from mvlt_amd.runtime import compute_dtype_of
    from mvlt_amd.train import PretrainStep, synthetic_batch

    def replica(**kw):
        torch.manual_seed(1234)
        cfg = M.MVLBertPretrainConfig()
        cfg.ITM_task = True
        cfg.mlm_max_labels_per_sample = None
        model = M.MVLBertForPretraining(cfg).cuda().train()
        return model, PretrainStep(model, **kw)

    arms = {"off": {}, "clip": dict(max_grad_norm=1.0), "clip+skip": dict(max_grad_norm=1.0, skip_nonfinite=True)}
    built = {k: replica(**kw) for k, kw in arms.items()}
    batch = synthetic_batch(32, 80, "cuda", 1234)[:4]
    M.manual_seed(4321)
    seed_coin_flip(5678)
    for model, step in built.values():
        for _ in range(10):
            step(batch)
    torch.cuda.synchronize()

    # ---- the step, interleaved
    for r in range(args.rounds):
        for name, (model, step) in built.items():
            for _ in range(3):
                step(batch)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                step(batch)
            torch.cuda.synchronize()
            ms = 1e3 * (time.perf_counter() - t0) / args.steps
            print(json.dumps(dict(round=r, arm=name, ms_per_step=round(ms, 4), steps=args.steps,
                                  skipped=step.opt.steps_skipped)), flush=True)

    # ---- stand-alone (last: the probe sweeps write the moments), over the runs of the last step of the "clip" arm
    model, step = built["clip"]
    ar = Arena.of(model, compute_dtype_of(model))
    opt = step.opt
    plan = opt._plan_runs(ar, [p for p in ar.params if ar.has_grad[id(p)]])
    live = sum(hi - lo for lo, hi, _ in plan)
    ws = opt._guard_buffers(ar)
    one = torch.ones(1, device="cuda")
    zero = torch.zeros(1, dtype=torch.int32, device="cuda")

    def norm():
        for k, (lo, hi, _) in enumerate(plan):
            ops.grad_sumsq(ar.grad[lo:hi], ws["partial"], accumulate=k > 0)
        ops.grad_norm_finish(ws["partial"], 1.0, 1.0, True, ws["out"], ws["flags"])

    def sweep(guarded):
        for lo, hi, _ in plan:
            a = (ar.flat[lo:hi], ar.grad[lo:hi], ar.exp_avg[lo:hi], ar.exp_avg_sq[lo:hi], ar.shadow[lo:hi] if ar.shadow is not None else None,
                 0.0, 0.9, 0.999, 1e-6, 0.0, 100)          # lr = 0: the probe leaves the parameters where they are
            ops.adamw_guarded(*a, 1.0, one, zero) if guarded else ops.adamw(*a, 1.0)

    for name, fn, nbytes in (("grad_sumsq+finish", norm, 4 * live), ("adamw", lambda: sweep(False), 30 * live),
                             ("adamw_guarded", lambda: sweep(True), 30 * live)):
        for _ in range(5):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / args.reps
        print(json.dumps(dict(probe=name, runs=len(plan), live_elements=live, ms=round(ms, 4),
                              tb_per_s=round(nbytes / ms / 1e9, 3))), flush=True)


if __name__ == "__main__":
    main()
