"""Config #4 shape (Swin-S + BERT-base, B = 32, max_length = 150, bf16, graph path): sampled decoding behind a top-k / top-p filter
next to the unfiltered sampled decode and the greedy decode, all in ONE process and interleaved round by round (the unfiltered
and greedy routes launch the kernels they launched before the filter existed, so they are the parent's figures on the same box).
Prints one line per configuration: the mean of every round and the spread over the rounds.  ROUNDS (5), MAXLEN (150)."""
import os, sys, time
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mvlt_amd as M
torch.manual_seed(0)
cfg = M.MVLBertConfigForImageCaption(); cfg.max_length = int(os.environ.get("MAXLEN", 150)); cfg.eos_token_id = None   # never stop early: fixed work
tok = type("Tok", (), {"mask_token_id": 103, "sep_token_id": 102})()
model = M.MVLBertForImageCaption(cfg, tokenizer=tok).cuda().eval()
img = torch.randn(32, 3, 224, 224, device="cuda")
CONFIGS = [("greedy", {}), ("sample", dict(sample_mode="sample", seed=1))]
CONFIGS += [(f"sample top_k={k} top_p={p}", dict(sample_mode="sample", seed=1, top_k=k, top_p=p)) for k, p in ((50, 1.0), (0, 0.9), (50, 0.9))]
times = {name: [] for name, _ in CONFIGS}
for r in range(int(os.environ.get("ROUNDS", 5)) + 1):          # round 0 warms up (and captures: the sampled graphs share one slot)
    for name, kw in CONFIGS:
        model(img, None, 1, "unilm", **kw)                      # recapture where the slot held another filter
        torch.cuda.synchronize(); t = time.time()
        ids, _ = model(img, None, 1, "unilm", **kw)
        torch.cuda.synchronize()
        if r:
            times[name].append((time.time() - t) * 1e3)
base = sum(times["sample"]) / len(times["sample"])
for name, _ in CONFIGS:
    v = times[name]; mean = sum(v) / len(v)
    print(f"{name:32s} {mean:7.2f} ms/batch (min {min(v):.2f} max {max(v):.2f} over {len(v)} rounds)  {1e3 * (mean - base) / cfg.max_length:+6.1f} us/token vs sample", flush=True)
