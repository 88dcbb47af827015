"""Report-generation fine-tuning step (run_report_generation_cxr.py:469-471) on the full-size caption model (Swin-S + BERT-base),
bf16, train mode, B = 32, T = 150, fused AdamW: the parent route -- F.cross_entropy(model(image, ids, 0, s), labels) over the
[B, V, T] logits -- against model(image, ids, 0, s, labels=labels) (labelled rows gathered first, mvlt_mlm_head_ce).
Both routes run in ONE process, interleaved block by block (the parent route launches the kernels it launched before the new
one existed); per route and strategy: mean ms/step, the spread of the block means, and peak allocated memory.
'unilm': <= 10 labels per sample as the dataset's _random_mask_word makes them; 'normal': every real token labelled.
ROUNDS (5 timed blocks per route), STEPS (8 steps per block), B (32), T (150)."""
import os, sys, time
import torch
import torch.nn.functional as F
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mvlt_amd as M
from mvlt_amd.optim import FusedAdamW
from mvlt_amd.train import synthetic_batch
B, T = int(os.environ.get("B", 32)), int(os.environ.get("T", 150))
ROUNDS, STEPS = int(os.environ.get("ROUNDS", 5)), int(os.environ.get("STEPS", 8))
torch.manual_seed(0)
cfg = M.MVLBertConfigForImageCaption()
tok = type("Tok", (), {"mask_token_id": 103, "sep_token_id": 102})()
model = M.set_compute_dtype(M.MVLBertForImageCaption(cfg, tokenizer=tok).cuda().train(), torch.bfloat16)
M.manual_seed(1)
opt = FusedAdamW(model, lr=4e-5)
image, ids, sparse, _ = synthetic_batch(B, T, "cuda", 1234)
LABELS = {"unilm": sparse, "normal": torch.where(ids > 0, ids, torch.full_like(ids, -100))}


def step(strategy, fused):
    lab = LABELS[strategy]
    if fused:
        loss = model(image, ids, 0, strategy, labels=lab)
    else:
        loss = F.cross_entropy(model(image, ids, 0, strategy), lab, ignore_index=-100)
    loss.backward()
    opt.step()
    return loss


def block(strategy, fused, n):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    t = time.time()
    for _ in range(n):
        loss = step(strategy, fused)
    torch.cuda.synchronize()
    return (time.time() - t) * 1e3 / n, torch.cuda.max_memory_allocated() / 2 ** 30, float(loss)


for strategy in ("unilm", "normal"):
    res = {False: [], True: []}
    mem, last = {}, {}
    for r in range(ROUNDS + 1):          # round 0 warms both routes up
        for fused in (False, True):
            ms, gib, loss = block(strategy, fused, STEPS if r else 3)
            if r:
                res[fused].append(ms)
                mem[fused] = max(mem.get(fused, 0.0), gib)
                last[fused] = loss
    n_lab = int((LABELS[strategy] >= 0).sum())
    for fused in (False, True):
        v = res[fused]
        print(f"{strategy:7s} {'labels= (fused head)' if fused else 'logits + F.cross_entropy'}: {sum(v) / len(v):7.2f} ms/step "
              f"(blocks min {min(v):.2f} max {max(v):.2f}, {len(v)} x {STEPS} steps)  peak {mem[fused]:.2f} GiB  "
              f"loss {last[fused]:.3f}  [{n_lab} labelled of {B * T} rows]", flush=True)
