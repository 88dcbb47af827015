"""Attention kernel microbenchmark at the pre-training step's shapes (B=32, bf16).
    python scripts/bench_attn.py [stage]      # stage 0..3: only that Swin stage (for counter runs), no BERT part
    python scripts/bench_attn.py bert         # only the MVLBert part: dense L = 131, then the step's packed rows
The packed lines draw the caption lengths of bench.py's batch (synthetic_batch(32, 80, seed 1234)) and lay the sequences
out back to back (row_start / seq_len) as the step does, so the figure is taken at the shape the step runs."""
import os, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mvlt_amd import ops, _lib as L
torch.manual_seed(0)
dt = torch.bfloat16
B = 32


def timeit(f, n=20):
    for _ in range(3): f()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n): f()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


tot = 0.0
BERT_ONLY = len(sys.argv) > 1 and sys.argv[1] == "bert"
ONLY = int(sys.argv[1]) if len(sys.argv) > 1 and not BERT_ONLY else None
for st, (res, C, nH, nblk) in enumerate([(56, 96, 3, 2), (28, 192, 6, 2), (14, 384, 12, 18), (7, 768, 24, 2)]):
    if BERT_ONLY or (ONLY is not None and st != ONLY):
        continue
    nW = (res // 7) ** 2
    nseq = B * nW
    qkv = (torch.randn(nseq * 49, 3 * C, device="cuda") * 0.5).to(dt)
    tbl = torch.randn(169, nH, device="cuda") * 0.02
    dtbl = torch.zeros_like(tbl)
    for shift in ((0, 3) if res > 7 else (0,)):
        kw = dict(bias_table=tbl, nW=nW, win_res=res, shift=shift)
        out, lse = ops.attn_fwd(qkv, L.ATTN_SWIN, nseq, 49, nH, 32, 32 ** -0.5, **kw)
        dout = torch.randn_like(out)
        tf = timeit(lambda: ops.attn_fwd(qkv, L.ATTN_SWIN, nseq, 49, nH, 32, 32 ** -0.5, **kw))
        tb = timeit(lambda: ops.attn_bwd(dout, qkv, out, lse, L.ATTN_SWIN, nseq, 49, nH, 32, 32 ** -0.5, dbias_table=dtbl, **kw))
        byt_f = qkv.numel() * 2 + out.numel() * 2
        byt_b = 2 * qkv.numel() * 2 + 2 * out.numel() * 2
        cnt = nblk / (2 if res > 7 else 1)
        tot += (tf + tb) * cnt
        print(f"swin s{st} res={res} C={C} nH={nH} shift={shift}: fwd {tf:6.1f} us ({byt_f/tf/1e6:5.2f} TB/s)  bwd {tb:6.1f} us ({byt_b/tb/1e6:5.2f} TB/s)  x{cnt:g}", flush=True)
if ONLY is not None:
    sys.exit(0)
Lq, H, nH = 131, 768, 12
from mvlt_amd.train import synthetic_batch
ids_step = synthetic_batch(B, 80, "cpu", 1234)[1]                    # bench.py's batch (rank 0)
seq_len = (51 + (ids_step != 0).sum(1)).to(torch.int32)
row_start = (torch.cumsum(seq_len, 0) - seq_len).to(torch.int32)
rows_packed = int(seq_len.sum())
ids_dense = torch.randint(1000, 30000, (B, 80)); ids_dense[:, 50:] = 0
for layout in ("dense", "packed"):
    packed = layout == "packed"
    rows = rows_packed if packed else B * Lq
    ids = (ids_step if packed else ids_dense).cuda()
    qkv = (torch.randn(rows, 3 * H, device="cuda") * 0.5).to(dt)
    for mode, name in ((L.ATTN_BIDIR, "bidir"), (L.ATTN_SEQ2SEQ, "seq2seq")):
        for pd in (0.0, 0.1):
            kw = dict(text_ids=ids, obj_end=50, dropout=(pd, 1234, 3))
            if packed:
                kw["pack"] = (row_start.cuda(), seq_len.cuda(), rows)
            out, lse = ops.attn_fwd(qkv, mode, B, Lq, nH, 64, 0.125, **kw)
            dout = torch.randn_like(out)
            tf = timeit(lambda: ops.attn_fwd(qkv, mode, B, Lq, nH, 64, 0.125, **kw))
            tb = timeit(lambda: ops.attn_bwd(dout, qkv, out, lse, mode, B, Lq, nH, 64, 0.125, **kw))
            byt_f = qkv.numel() * 2 + out.numel() * 2
            byt_b = 2 * qkv.numel() * 2 + 2 * out.numel() * 2
            if pd > 0 and mode == L.ATTN_BIDIR and not packed: tot += (tf + tb) * 12
            print(f"bert {layout} ({rows} rows) {name} p={pd}: fwd {tf:6.1f} us ({byt_f/tf/1e6:5.2f} TB/s)  bwd {tb:6.1f} us ({byt_b/tb/1e6:5.2f} TB/s)  x12", flush=True)
if not BERT_ONLY:
    print(f"TOTAL per step (standalone, dense BERT rows): {tot/1e3:.2f} ms")
