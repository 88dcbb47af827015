"""Retrieval evaluation (run_retrieval.py:192-296) on the full-size model (Swin-S + BERT-base, bf16, eval): N images x N captions
of T = 80 with caption lengths drawn as tests/conftest.py:synth_batch draws them (uniform in [T / 4, T)).

Part 1, pairs/s of the N^2-pair score matrix, two routes interleaved block by block in ONE process:
  parent route     batches of 32 pairs through model(images[ii], captions[jj]), as testRetrieval issues them -- the whole Swin
                   tower per pair, dense caption rows.  The images stay on the device and the probabilities are not read back
                   per item, so the reference's 600 KB of pixels per pair over PCIe and its .item() per pair are NOT charged.
  score_all_pairs  the tower once per image, packed rows, chunks of PAIR_CHUNK pairs; once with the scoring head on its separate
                   launches (the default) and once on mvlt_retrieval_head (MVLT_RETRIEVAL_HEAD=1).
  All end in a device synchronise; the max abs difference of the score matrices against the parent route's is printed.
Part 2, the scoring head alone at P = PAIR_CHUNK pairs: mvlt_retrieval_head against the nine launches it replaces ([CLS] gather,
  pooler product, tanh, transform product + GELU, LayerNorm, Linear(H, 2), cast, softmax, scatter), HIP events around blocks of
  REPS calls, interleaved.  Through Python both are host-enqueue-bound at this size: the figure is what a caller sees, not a
  kernel time.
N (64), PAIR_CHUNK (512), ROUNDS (5 timed blocks per route), REPS (200); HEAD_ONLY=1 skips part 1 (for a kernel trace of part 2:
rocprofv3 --kernel-trace --stats gives the device time of retrieval_head_kernel and of the nine launches' kernels)."""
import os, sys, time
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mvlt_amd as M
from mvlt_amd import ops
from mvlt_amd.arena import Arena

N, T = int(os.environ.get("N", 64)), 80
CHUNK, ROUNDS, REPS = int(os.environ.get("PAIR_CHUNK", 512)), int(os.environ.get("ROUNDS", 5)), int(os.environ.get("REPS", 200))
assert torch.cuda.is_available(), "bench_retrieval.py measures on the GPU only"
g = torch.Generator().manual_seed(7)
images = torch.randn(N, 3, 224, 224, generator=g).cuda()
ids = torch.zeros(N, T, dtype=torch.long)
for b in range(N):
    ln = int(torch.randint(T // 4, T, (1,), generator=g))
    ids[b, :ln] = torch.randint(1000, 30522, (ln,), generator=g)
ids = ids.cuda()
torch.manual_seed(0)
model = M.set_compute_dtype(M.MVLBertForRetrieval(M.MVLBertRetrieval()).cuda().eval(), torch.bfloat16)
flat = torch.arange(N * N, device="cuda")
II, JJ = flat // N, flat % N


@torch.no_grad()
def parent_route():
    out = torch.empty(N * N, device="cuda")
    for p0 in range(0, N * N, 32):
        out[p0:p0 + 32] = model(images[II[p0:p0 + 32]], ids[JJ[p0:p0 + 32]])[:, 1]
    return out.view(N, N)


def new_route():
    M.model._RETRIEVAL_HEAD = False
    return M.score_all_pairs(model, images, ids, pair_chunk=CHUNK)


def new_route_fused():
    M.model._RETRIEVAL_HEAD = True
    return M.score_all_pairs(model, images, ids, pair_chunk=CHUNK)


def timed(fn):
    torch.cuda.synchronize()
    t = time.time()
    out = fn()
    torch.cuda.synchronize()
    return time.time() - t, out


HEAD_ONLY = os.environ.get("HEAD_ONLY", "0") == "1"
ROUTES = (("parent", parent_route, "model(images[ii], captions[jj]), 32 pairs per call"),
          ("new", new_route, f"score_all_pairs, pair_chunk {CHUNK}, separate head launches"),
          ("fused", new_route_fused, f"score_all_pairs, pair_chunk {CHUNK}, mvlt_retrieval_head"))
res = {name: [] for name, _, _ in ROUTES}
for r in range(0 if HEAD_ONLY else ROUNDS + 1):          # round 0 warms both routes up
    for name, fn, _ in ROUTES:
        s, out = timed(fn)
        if r:
            res[name].append(s)
        res[name + "_out"] = out
for name, _, label in ROUTES:
    if HEAD_ONLY:
        break
    v = res[name]
    print(f"N = {N} ({N * N} pairs)  {label}: {N * N / (sum(v) / len(v)):9.0f} pairs/s  "
          f"({sum(v) / len(v) * 1e3:.1f} ms per matrix, blocks min {min(v) * 1e3:.1f} max {max(v) * 1e3:.1f}, {len(v)} blocks)", flush=True)
if not HEAD_ONLY:
    for name in ("new", "fused"):
        print(f"max abs difference against the parent route's matrix, {name}: {float((res['parent_out'] - res[name + '_out']).abs().max()):.3g}", flush=True)

# ---- part 2: the head alone
H = model.config.hidden_size
P = CHUNK
ar = Arena.of(model, torch.bfloat16)
ar.refresh_shadow()
pd, tr, lin = model.MVLBert.pooler.dense, model.final_mlp[0], model.final_mlp[1]
lens = torch.randint(60, 131, (P,), generator=g, dtype=torch.int32)
row_start = (torch.cumsum(lens, 0) - lens).to(torch.int32).cuda()
rs64 = row_start.to(torch.int64)
hidden = torch.randn(int(lens.sum()), H, generator=g).to(torch.bfloat16).cuda()
out_index = torch.randperm(P, generator=g).cuda()
scores = torch.zeros(2, P, device="cuda")


def fused():
    ops.retrieval_head(hidden, row_start, ar.compute(pd.weight), pd.bias.data, ar.compute(tr.dense.weight), tr.dense.bias.data,
                       tr.LayerNorm.weight.data, tr.LayerNorm.bias.data, tr.LayerNorm.eps, ar.compute(lin.weight), lin.bias.data,
                       out_index, scores[0])


def nine():
    cls = hidden.index_select(0, rs64)
    pooled = ops.tanh_fwd(ops.gemm(cls, ar.compute(pd.weight), bias=pd.bias.data))
    t1 = ops.gemm(pooled, ar.compute(tr.dense.weight), bias=tr.dense.bias.data, gelu=True)
    t2 = ops.layernorm_fwd(t1, tr.LayerNorm.weight.data, tr.LayerNorm.bias.data, tr.LayerNorm.eps)[0]
    logits = ops.cast(ops.gemm(t2, ar.compute(lin.weight), bias=lin.bias.data, ldc=4), torch.float32)
    prob = ops.softmax_rows(logits, 2)
    scores[1].index_copy_(0, out_index, prob[:, 1])


def events(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(REPS):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / REPS


with torch.no_grad():
    hres = {"fused": [], "nine": []}
    for r in range(ROUNDS + 1):
        for name, fn in (("nine", nine), ("fused", fused)):
            us = events(fn)
            if r:
                hres[name].append(us)
for name, label in (("nine", "nine launches"), ("fused", "mvlt_retrieval_head")):
    v = hres[name]
    print(f"head, P = {P}, H = {H}  {label}: {sum(v) / len(v):7.1f} us per call (blocks min {min(v):.1f} max {max(v):.1f}, "
          f"{len(v)} x {REPS} calls)", flush=True)
print(f"max abs difference of the two heads' scores: {float((scores[0] - scores[1]).abs().max()):.3g}", flush=True)
