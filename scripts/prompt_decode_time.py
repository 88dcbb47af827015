"""Decoding behind a text prompt at the report-generation shape (config #4: Swin-S + BERT-base, bf16, B = 32 x 150 NEW tokens,
eos_token_id = None so every run has the same length), from the image tower's output:

  plain      greedy_search without a prompt on the replayed graph, greedy and sample: the code path that must not have changed
  prompt     the same decodes behind ragged prompts, P_b ~ U{4..32} (seeded), on the prompted graph (mvlt_attn_cached_rows /
             mvlt_embed_fwd_rows in every cached step, one dense prefill)
  recompute  what a user had before: no cache, one dense teacher-forced forward per token over [prompt_b, y_<t, MASK, filler] for
             the whole batch, the hidden row of every sample's own [MASK], the fused greedy head.  The dense forward stops at 208
             positions, so this route ends after 208 - 51 - 32 - 1 = 124 new tokens: it is timed over those

The driver (no argument) starts every GPU step as a child process under a time limit of its own and stops at the first that fails:
  1  `cases`: plain / prompt / recompute interleaved round by round in ONE process after a warm-up round; median, min, max ms per
     batch; the first token (step 0 or prefill + one pick: a decode of max_length 1) the same way, and from the two the time per
     later token
  2  --old DIR (a built checkout of the parent commit): `plain` in DIR and here, alternating, PAIRS times -- the same code path, so
     the medians must agree within the spread of the rounds
  3  --trace: one rocprofv3 kernel-trace run (its own process: no counters, nothing else traced) of a 40-token decode without a
     prompt and of one with an EMPTY prompt (input_ids [B, 0]: all shifts zero, the same positions, so the two attention kernels do
     the same work); prints calls and mean duration of the cached attention and the new-token embedding with and without the table
     (--no-cases: skip part 1)
B (32), MAXLEN (150), ROUNDS (5), PAIRS (3), TRACE_DIR (a temporary directory)."""
import csv, glob, json, os, statistics, subprocess, sys, tempfile, time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, MAXLEN, ROUNDS = int(os.environ.get("B", 32)), int(os.environ.get("MAXLEN", 150)), int(os.environ.get("ROUNDS", 5))
P_LO, P_HI = 4, 32
N_RC = min(MAXLEN, 208 - 49 - 2 - P_HI - 1)          # new tokens the teacher-forced route can reach (the dense forward's 208 positions)


def child(mode):
    import torch
    sys.path.insert(0, os.environ.get("MVLT_TREE", HERE))
    import mvlt_amd as M
    from mvlt_amd import decode, ops
    torch.manual_seed(0)
    cfg = M.MVLBertConfigForImageCaption(); cfg.max_length = MAXLEN; cfg.eos_token_id = None
    tok = type("Tok", (), {"mask_token_id": 103, "sep_token_id": 102})()
    model = M.set_compute_dtype(M.MVLBertForImageCaption(cfg, tokenizer=tok).cuda().eval(), torch.bfloat16)
    os.environ["MVLT_DECODE_GRAPH"] = "1"
    with torch.no_grad():
        ar = decode.Arena.of(model, torch.bfloat16)
        feat = model.conv(torch.randn(B, 3, 224, 224, device="cuda"))
    g = torch.Generator().manual_seed(1)
    lens = torch.randint(P_LO, P_HI + 1, (B,), generator=g).tolist()
    prompts = torch.randint(1000, 30000, (B, P_HI), generator=g).cuda()
    empty = torch.zeros((B, 0), dtype=torch.int64, device="cuda")

    def recompute(n):
        """The teacher-forced route: token t from a dense forward over every row's prompt and its t tokens so far."""
        mv = model.MVLBert
        cols = torch.tensor(lens, dtype=torch.int64, device="cuda")
        rows = torch.arange(B, device="cuda")
        text = decode.prompt_tables(prompts, lens, 103)[0]
        out = []
        for t in range(n):
            hidden, _, _ = mv._forward(feat, text, text, None, True, False)
            t2, W, bias = decode._head(model, ar, hidden[rows, cols + t + feat.shape[1] + 2].contiguous())
            nxt, _ = ops.gemm_argmax(t2, W, bias)
            out.append(nxt)
            text = torch.cat([text, text.new_full((B, 1), 103)], 1)
            text[rows, cols + t] = nxt
        return torch.stack(out, 1)

    def run(case, sample_mode, n):
        kw = dict(sample_mode=sample_mode, seed=7) if sample_mode == "sample" else {}
        if case == "prompt":
            kw.update(input_ids=prompts, prompt_lengths=lens)
        if case == "empty":
            kw.update(input_ids=empty)
        torch.cuda.synchronize(); t = time.time()
        with torch.no_grad():
            ids = recompute(n) if case == "recompute" else decode.greedy_search(model, feat, max_length=n, **kw)[0]
        torch.cuda.synchronize()
        return (time.time() - t) * 1e3, ids

    cases = {"plain": ("plain",), "cases": ("plain", "prompt", "recompute"), "trace": ("plain", "empty")}[mode]
    lengths = (MAXLEN,) if mode != "cases" else (MAXLEN, 1)
    rounds = 2 if mode == "trace" else ROUNDS
    times, outs = {}, {}
    for n in lengths:                                 # one length after the other: a graph is keyed by its max_length
        for r in range(rounds + 1):                   # round 0 warms up (and captures the graphs)
            for sm in ("greedy", "sample"):
                for case in cases:
                    if case == "recompute" and sm == "sample":
                        continue
                    ms, outs[case, sm, n] = run(case, sm, min(n, N_RC) if case == "recompute" else n)
                    if r:
                        times.setdefault((case, sm, n), []).append(ms)
    for (case, sm, n), v in times.items():
        print(json.dumps(dict(case=case, mode=sm, B=B, tokens=n, median_ms=round(statistics.median(v), 2), min_ms=round(min(v), 2),
                              max_ms=round(max(v), 2), rounds=len(v))), flush=True)
    if mode == "cases":
        same = float((outs["prompt", "greedy", MAXLEN][:, :N_RC] == outs["recompute", "greedy", MAXLEN]).float().mean())
        print(json.dumps(dict(prompt_vs_recompute_same_tokens=round(same, 4), recompute_tokens=N_RC, mean_prompt_length=sum(lens) / B)), flush=True)
        for case, sm in (("plain", "greedy"), ("prompt", "greedy"), ("plain", "sample"), ("prompt", "sample"), ("recompute", "greedy")):
            full, one = statistics.median(times[case, sm, MAXLEN]), statistics.median(times[case, sm, 1])
            later = (N_RC if case == "recompute" else MAXLEN) - 1
            print(json.dumps(dict(case=case, mode=sm, first_token_ms=round(one, 2), per_later_token_us=round((full - one) / later * 1e3, 1))),
                  flush=True)
    if mode == "trace":
        assert bool((outs["plain", "greedy", MAXLEN] == outs["empty", "greedy", MAXLEN]).all())


def step(cmd, limit, env=None):
    """One GPU step: a fresh child under its own time limit; a failure ends the script (nothing more is started)."""
    print("+", " ".join(cmd), flush=True)
    p = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, env=dict(os.environ, **(env or {})), capture_output=True, text=True)
    sys.stdout.write(p.stdout)
    if p.returncode != 0:
        sys.stdout.write(p.stderr[-2000:])
        sys.exit(f"step failed with status {p.returncode}: stopping")
    return [json.loads(l) for l in p.stdout.splitlines() if l.startswith("{")]


def main():
    me = [sys.executable, os.path.abspath(__file__)]
    args = sys.argv[1:]
    if args and args[0] == "child":
        return child(args[1])
    if "--no-cases" not in args:
        step(me + ["child", "cases"], 420)
    if "--old" in args:
        old = os.path.abspath(args[args.index("--old") + 1])
        res = {"parent": [], "this": []}
        for i in range(int(os.environ.get("PAIRS", 3))):
            for k in (("parent", "this"), ("this", "parent"))[i % 2]:          # who goes first alternates too
                res[k] += step(me + ["child", "plain"], 240, env={"MVLT_TREE": old} if k == "parent" else None)
        for sm in ("greedy", "sample"):
            for k, v in res.items():
                m = [r["median_ms"] for r in v if r.get("mode") == sm]
                print(f"no prompt, {sm:6s} {k:6s}: medians {m}  median of medians {statistics.median(m):.2f} ms", flush=True)
    if "--trace" in args:
        out = os.environ.get("TRACE_DIR") or tempfile.mkdtemp(prefix="prompt_trace_")
        step(["rocprofv3", "--kernel-trace", "--stats", "-d", out, "-o", "prompt", "--output-format", "csv", "--"] + me + ["child", "trace"],
             420, env={"MAXLEN": "40"})
        for path in glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True):
            for row in csv.DictReader(open(path)):
                name = row.get("Name", "")
                if any(k in name for k in ("attn_cached_kernel", "embed_fwd_kernel")):
                    print(f"{name[:150]}: calls {row.get('Calls')}, mean {float(row.get('AverageNs', 'nan')) / 1e3:.2f} us", flush=True)


if __name__ == "__main__":
    main()
