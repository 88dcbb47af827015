"""What attention maps cost: MVLBertForVQA (Swin-S + BERT-base, bf16, eval) at B = 32, T = 23 on one MI355X.

Three calls, alternated round by round in one process (device events around each call, medians over the rounds):
    forward                                   the plain answer
    attention_maps()                          default selection: all 12 layers, [CLS] -> image tokens, mean over heads
    attention_maps('all', 'all', per head)    the full 74 x 74 matrix of every head and layer
and mvlt_attn_probs alone at both selections on operands of the same shape (device events around REPS back-to-back launches).
The answer of attention_maps is compared with forward's (bit-identical) before anything is timed.  Results: profiles/attention_maps.md."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mvlt_amd as M  # noqa: E402
from mvlt_amd import _lib, ops  # noqa: E402


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--text", type=int, default=23)
    ap.add_argument("--rounds", type=int, default=40)
    ap.add_argument("--reps", type=int, default=200)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: nothing here is measured on the host"
    torch.manual_seed(0)
    B, T = a.batch, a.text
    model = M.set_compute_dtype(M.MVLBertForVQA(M.MVLBertConfigforVQA()).cuda().eval(), torch.bfloat16)
    img = torch.randn(B, 3, 224, 224, device="cuda")
    q = torch.randint(1000, 30000, (B, T), device="cuda")
    q[:, T - T // 4:] = 0                                             # padded tails, as real questions have
    calls = {
        "forward": lambda: model(img, q, None),
        "maps cls->image, head mean": lambda: model.attention_maps(img, q),
        "maps all->all, per head": lambda: model.attention_maps(img, q, queries='all', keys='all', head_mean=False),
    }
    with torch.no_grad():
        prob, logits = model(img, q, None)
        p2, l2, maps = model.attention_maps(img, q)
        assert torch.equal(prob, p2) and torch.equal(logits, l2), "attention_maps changed the answer"
        print(f"answer bit-identical to forward; maps {tuple(maps.shape)}, row sums within the image tokens "
              f"{float(maps.sum(-1).min()):.3f} .. {float(maps.sum(-1).max()):.3f}")
        for fn in calls.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in calls}
        for _ in range(a.rounds):
            for k, fn in calls.items():
                ms[k].append(timed(fn))
    base = statistics.median(ms["forward"])
    for k, v in ms.items():
        v.sort()
        med = statistics.median(v)
        print(f"{k:32s} median {med:7.3f} ms  (min {v[0]:7.3f}, p90 {v[int(0.9 * len(v))]:7.3f}; {med - base:+7.3f} ms vs forward; {a.rounds} rounds)")

    # the kernel alone
    cfg = model.config
    nH, L = cfg.num_attention_heads, 49 + 2 + T
    hd = cfg.hidden_size // nH
    qkv = torch.randn(B * L, 3 * nH * hd, device="cuda").to(torch.bfloat16)
    kw = dict(text_ids=q, obj_end=50)
    _, lse = ops.attn_fwd(qkv, _lib.ATTN_BIDIR, B, L, nH, hd, hd ** -0.5, **kw)
    for name, qr, kr, hm in (("cls->image, head mean", (0, 1), (1, 49), True), ("all->all, per head", (0, L), (0, L), False)):
        out = torch.empty((B, 1 if hm else nH, qr[1], kr[1]), dtype=torch.float32, device="cuda")
        run = lambda: ops.attn_probs(qkv, lse, _lib.ATTN_BIDIR, B, L, nH, hd, hd ** -0.5, qr, kr, head_mean=hm, out=out, **kw)  # noqa: E731
        for _ in range(10):
            run()
        torch.cuda.synchronize()
        per = []
        for _ in range(5):
            per.append(timed(lambda: [run() for _ in range(a.reps)]) / a.reps * 1e3)
        flops = 2.0 * B * nH * qr[1] * kr[1] * hd
        rd = B * nH * (qr[1] + kr[1]) * hd * 2 + B * nH * qr[1] * 4
        print(f"mvlt_attn_probs {name:24s} {statistics.median(per):7.2f} us per launch back to back "
              f"(min {min(per):.2f}; {flops / 1e6:.1f} MFLOP, reads {rd / 1e6:.2f} MB, writes {out.numel() * 4 / 1e6:.2f} MB)")


if __name__ == "__main__":
    main()
