"""The decodes of a self-critical step at config #4 shapes (Swin-S + BERT-base, B = 32 images, bf16, eos_token_id = None, 150
tokens), from the image tower's output, one mode per process:
  two     the greedy graph, then the sampled graph: the two decodes of self_critical_loss's default path (2 x 32 rows)
  one     sample_many(num_samples=1): greedy row + one sample per image in one pass (64 rows)
  five    sample_many(num_samples=5): greedy row + five samples per image in one pass (192 rows)
2 warm-up decodes, mean of 3.  MAXLEN=40 shortens the decode (kernel traces)."""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mvlt_amd as M  # noqa: E402
from mvlt_amd import decode  # noqa: E402
from mvlt_amd.arena import Arena  # noqa: E402
from mvlt_amd.runtime import compute_dtype_of  # noqa: E402

mode = sys.argv[1] if len(sys.argv) > 1 else "one"
assert mode in ("two", "one", "five"), mode
torch.manual_seed(0)
cfg = M.MVLBertConfigForImageCaption()
cfg.max_length = int(os.environ.get("MAXLEN", 150))
cfg.eos_token_id = None          # never stop early: fixed work
tok = type("Tok", (), {"mask_token_id": 103, "sep_token_id": 102})()
model = M.MVLBertForImageCaption(cfg, tokenizer=tok).cuda().eval()
img = torch.randn(32, 3, 224, 224, device="cuda")
with torch.no_grad():
    Arena.of(model, compute_dtype_of(model))
    feat = model.conv(img)


def run():
    if mode == "two":
        g, _ = decode.greedy_search(model, feat)
        s, _ = decode.greedy_search(model, feat, sample_mode="sample", seed=1)
        return g.shape[0] + s.shape[0], s.shape[1]
    ids, _ = decode.sample_many(model, feat, 1 if mode == "one" else 5, include_greedy=True, seed=1)
    return ids.shape[0] * ids.shape[1], ids.shape[2]


for _ in range(2):
    run()
torch.cuda.synchronize()
t = time.time()
n = 3
for _ in range(n):
    rows, steps = run()
torch.cuda.synchronize()
dt = (time.time() - t) / n
print(f"multi-sample decode [{mode}] images=32 rows={rows} max_length={steps}: {dt * 1e3:.1f} ms per batch of images, "
      f"{dt / steps * 1e6:.0f} us per token column, {rows * steps / dt:.0f} tokens/s", flush=True)
