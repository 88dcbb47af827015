"""For the kernels matching PATTERN in a rocprofv3 kernel trace: launches, mean duration, and how much of that time a kernel
of ANOTHER queue was running (a kernel that runs alone on the chip shows ~0).  The first skip_fraction of the trace (warm-up)
is left out.
    python scripts/trace_overlap.py <trace dir or kernel_trace.csv> PATTERN [skip_fraction]"""
import bisect, collections, csv, glob, re, sys
path = sys.argv[1] if sys.argv[1].endswith(".csv") else glob.glob(sys.argv[1] + "/**/*_kernel_trace.csv", recursive=True)[0]
pat = re.compile(sys.argv[2])
skip = float(sys.argv[3]) if len(sys.argv) > 3 else 0.5
rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
rows = rows[int(len(rows) * skip):]
iv = [(int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Queue_Id"]) for r in rows]
starts = [a for a, _, _ in iv]
def short(n): return re.sub(r"\(anonymous namespace\)::|^void |\(.*$", "", n)[:70]
n = collections.Counter(); dur = collections.Counter(); ovl = collections.Counter()
for r in rows:
    if not pat.search(r["Kernel_Name"]):
        continue
    a, b, q = int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Queue_Id"]
    k = short(r["Kernel_Name"])
    n[k] += 1; dur[k] += b - a
    # kernels of other queues that start before b; those that ended before a do not count (no kernel here lasts > 2 ms)
    lo = bisect.bisect_left(starts, a - 2_000_000)
    hi = bisect.bisect_left(starts, b)
    ovl[k] += sum(max(0, min(b, e) - max(a, s)) for s, e, qq in iv[lo:hi] if qq != q)
for k in n:
    print(f"{k:70s} launches {n[k]:5d}  mean {dur[k] / n[k] / 1e3:6.1f} us  overlapped by another queue {ovl[k] / n[k] / 1e3:5.2f} us")
