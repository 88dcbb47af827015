"""Report metrics (BLEU-1..4, ROUGE-L, CIDEr) of N = 3 000 decoded reports of 60 to 100 words, one reference each: the device
path (mvlt_amd.report_metrics: ReferenceSet once, then ReportScorer.add in batches of BATCH rows and one result()) against the
host restatement on exact tuples (tests/report_metrics_ref.py: score_corpus), on the same box, same ids.

Words come from a Zipf-like draw over 2 000 word ids; a hypothesis is its reference with words dropped, replaced and inserted.
With PIECES=1 (default) every word is 1 to 3 WordPiece ids and the flag table merges them, as on a real vocabulary; PIECES=0
scores ids as words.  The device figure ends in result() (the one host copy); the ReferenceSet build is timed separately, and so
are one score() call over all N rows and one mvlt_report_ngram_keys call over all references (HIP events, 20 calls each).
N (3000), BATCH (32), ROUNDS (5).  The two results are printed side by side with their largest relative difference."""
import os, random, sys, time
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mvlt_amd as M                      # noqa: E402
from mvlt_amd import report_metrics as RM  # noqa: E402
import report_metrics_ref as R            # noqa: E402

N, BATCH, ROUNDS = int(os.environ.get("N", 3000)), int(os.environ.get("BATCH", 32)), int(os.environ.get("ROUNDS", 5))
PIECES = os.environ.get("PIECES", "1") == "1"
assert torch.cuda.is_available(), "bench_report_metrics.py measures on the GPU only"
rng = random.Random(11)
NW = 2000
weights = [1.0 / (r + 1) for r in range(NW)]
word = lambda: rng.choices(range(NW), weights)[0]
V = 1000 + 3 * NW
flags = [0] * V
for w in range(NW):
    flags[1000 + 3 * w + 1] = flags[1000 + 3 * w + 2] = R.CONT
pieces = lambda w: [1000 + 3 * w + j for j in range(1 + w % 3)] if PIECES else [1000 + w]


def noisy(ref):
    out = []
    for w in ref:
        u = rng.random()
        if u < 0.1:
            continue
        out.append(word() if u < 0.25 else w)
        if rng.random() < 0.08:
            out.append(word())
    return out[:100]


ref_words = [[word() for _ in range(rng.randint(60, 100))] for _ in range(N)]
hyp_words = [noisy(r) for r in ref_words]
enc = lambda rows: [[p for w in row for p in pieces(w)] + [102] for row in rows]
ref_rows, hyp_rows = enc(ref_words), enc(hyp_words)
T = max(map(len, hyp_rows))
hyp = torch.tensor([r + [0] * (T - len(r)) for r in hyp_rows], dtype=torch.int64).cuda()
table = torch.tensor(flags, dtype=torch.uint8) if PIECES else None


def timed(fn):
    torch.cuda.synchronize()
    t = time.time()
    out = fn()
    torch.cuda.synchronize()
    return time.time() - t, out


def device():
    scorer = RM.ReportScorer(refs)
    for s in range(0, N, BATCH):
        scorer.add(hyp[s:s + BATCH], torch.arange(s, min(N, s + BATCH), device="cuda"))
    return scorer.result()


def host():
    f = flags if PIECES else None
    return R.score_corpus([R.segment(r, f) for r in hyp_rows], [R.segment(r, f) for r in ref_rows])["corpus"]


build, dev = [], []
for r in range(ROUNDS + 1):
    s, refs = timed(lambda: RM.ReferenceSet(ref_rows, table))
    build.append(s)
    s, got = timed(device)
    dev.append(s)
build, dev = build[1:], dev[1:]
def events(fn, reps=20):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


one_launch = events(lambda: RM.score(hyp, refs))          # all N pairs in one mvlt_report_stats launch + the element-wise tail
keys_launch = events(lambda: M.ops.report_ngram_keys(refs.ids, refs.flags, refs.stop_ids))
t = time.time()
want = host()
host_s = time.time() - t
print(f"N = {N}, rows of <= {T} pieces, pieces={int(PIECES)}, {refs.df_keys.numel()} distinct reference n-grams")
print(f"ReferenceSet (DF table): {sum(build) / len(build) * 1e3:8.1f} ms (min {min(build) * 1e3:.1f} max {max(build) * 1e3:.1f}, {len(build)} runs)")
print(f"device, add x {(N + BATCH - 1) // BATCH} + result(): {sum(dev) / len(dev) * 1e3:8.1f} ms (min {min(dev) * 1e3:.1f} max {max(dev) * 1e3:.1f}, {len(dev)} runs)")
print(f"score() of all {N} rows in one call: {one_launch:.3f} ms; mvlt_report_ngram_keys of all references: {keys_launch:.3f} ms (HIP events, 20 calls)")
print(f"host restatement:       {host_s * 1e3:8.1f} ms (1 run)")
for k in R.KEYS:
    print(f"  {k:8s} device {got[k]:.12f}  host {want[k]:.12f}")
print(f"largest relative difference: {max(abs(got[k] - want[k]) / abs(want[k]) for k in R.KEYS):.3g}")
