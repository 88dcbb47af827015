"""Constrained decoding at the report-generation shape (config #4: Swin-S + BERT-base, bf16, B = 32 x 150 tokens, eos_token_id = None
so every run has the same length -- the min-length rule, which bans the eos, is therefore idle here), greedy and sample:

  off    rules off on the replayed graph: the code path without the rules
  on     repetition_penalty 1.2, no_repeat_ngram_size 3, min_length 10 on the replayed graph (plan kernel + rule-aware head)
  torch  what a user had before the rule-aware heads: the eager loop with materialised logits and the same rules as torch ops on
         the device (gather / scatter for the penalty, unfold + scatter_reduce for the n-grams), then argmax / the Gumbel-max draw

The driver (no argument) starts every GPU step as a child process under a time limit of its own and stops at the first that fails:
  1  `cases`: off / on / torch interleaved round by round in ONE process after a warm-up round; median, min, max ms per batch
  2  --old DIR (a built checkout of the parent commit): `off` in DIR and here, alternating, PAIRS times -- the same code path, so the
     medians must agree within the spread of the rounds
  3  --trace: one rocprofv3 kernel-trace run of `off` and `on` (its own process: no counters, nothing else traced); prints calls and
     mean duration of the plan kernel and of the head products with and without rules (--no-cases: skip part 1)
B (32), MAXLEN (150), ROUNDS (5), PAIRS (3), TRACE_DIR (a temporary directory)."""
import csv, glob, json, os, statistics, subprocess, sys, tempfile, time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, MAXLEN, ROUNDS = int(os.environ.get("B", 32)), int(os.environ.get("MAXLEN", 150)), int(os.environ.get("ROUNDS", 5))
RULES = dict(repetition_penalty=1.2, no_repeat_ngram_size=3, min_length=10)


def child(mode):
    import torch
    sys.path.insert(0, os.environ.get("MVLT_TREE", HERE))
    import mvlt_amd as M
    from mvlt_amd import decode, ops
    torch.manual_seed(0)
    cfg = M.MVLBertConfigForImageCaption(); cfg.max_length = MAXLEN; cfg.eos_token_id = None
    tok = type("Tok", (), {"mask_token_id": 103, "sep_token_id": 102})()
    model = M.set_compute_dtype(M.MVLBertForImageCaption(cfg, tokenizer=tok).cuda().eval(), torch.bfloat16)
    img = torch.randn(B, 3, 224, 224, device="cuda")
    head = model.MLM_head_seq2seq
    V = head.predictions.decoder.out_features

    def torch_rules(logits, hist):
        """HF's three processors as device-side torch ops on materialised f32 logits [B, V]; hist: int64 [B, c]."""
        pen, g = RULES["repetition_penalty"], RULES["no_repeat_ngram_size"]
        c = hist.shape[1]
        if c:
            sc = logits.gather(1, hist)
            logits.scatter_(1, hist, torch.where(sc < 0, sc * pen, sc / pen))
        if c >= g:
            win = hist.unfold(1, g, 1)                                        # [B, c - g + 1, g]
            match = (win[:, :, :g - 1] == hist[:, None, c - g + 1:]).all(-1)
            ban = torch.zeros_like(logits).scatter_reduce_(1, win[:, :, -1], match.to(logits.dtype), reduce="amax")
            logits.masked_fill_(ban > 0, float("-inf"))
        return logits

    def run(case, sample_mode):
        kw = dict(sample_mode=sample_mode, seed=7) if sample_mode == "sample" else {}
        saved = {}
        if case == "on":
            kw.update(RULES)
        if case == "torch":
            os.environ["MVLT_DECODE_GRAPH"] = "0"
            hist = []
            ar = decode.Arena.of(model, torch.bfloat16)

            def pick(t2, W, bias, seed=None, tag=None, temperature=1.0):
                logits = head._logits(ar, t2)[0][:, :V].float()
                h = torch.stack(hist, 1) if hist else torch.zeros((t2.shape[0], 0), dtype=torch.int64, device=t2.device)
                x = torch_rules(logits, h)
                if seed is None:
                    nxt = x.argmax(1); score = x.gather(1, nxt[:, None]).squeeze(1)
                else:
                    nxt = (x + ops.gumbel_noise(seed, tag, x.shape[0], V, x.device)).argmax(1)
                    score = torch.log_softmax(x, 1).gather(1, nxt[:, None]).squeeze(1)
                hist.append(nxt)
                return nxt, score
            for name in ("gemm_argmax", "gemm_sample"):
                saved[name] = getattr(ops, name); setattr(ops, name, pick)
        else:
            os.environ["MVLT_DECODE_GRAPH"] = "1"
        torch.cuda.synchronize(); t = time.time()
        ids, _ = model(img, None, 1, "unilm", **kw)
        torch.cuda.synchronize()
        ms = (time.time() - t) * 1e3
        for name, fn in saved.items():
            setattr(ops, name, fn)
        return ms, ids

    cases = {"off": ("off",), "cases": ("off", "on", "torch"), "trace": ("off", "on")}[mode]
    rounds = 2 if mode == "trace" else ROUNDS
    times, outs = {}, {}
    for r in range(rounds + 1):                       # round 0 warms up (and captures the graphs)
        for sm in ("greedy", "sample"):
            for case in cases:
                ms, outs[case, sm] = run(case, sm)
                if r:
                    times.setdefault((case, sm), []).append(ms)
    for (case, sm), v in times.items():
        print(json.dumps(dict(case=case, mode=sm, B=B, tokens=MAXLEN, median_ms=round(statistics.median(v), 2), min_ms=round(min(v), 2),
                              max_ms=round(max(v), 2), rounds=len(v))), flush=True)
    for sm in ("greedy", "sample"):
        if ("on", sm) in outs and ("torch", sm) in outs:
            a, b = outs["on", sm], outs["torch", sm]
            same = float((a == b).float().mean())
            print(json.dumps(dict(mode=sm, on_vs_torch_same_tokens=round(same, 4), on_vs_off_same_tokens=round(
                float((a == outs["off", sm]).float().mean()), 4))), flush=True)


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
        for _ in range(int(os.environ.get("PAIRS", 3))):
            res["parent"] += step(me + ["child", "off"], 240, env={"MVLT_TREE": old})
            res["this"] += step(me + ["child", "off"], 240)
        for sm in ("greedy", "sample"):
            for k, v in res.items():
                m = [r["median_ms"] for r in v if r.get("mode") == sm]
                print(f"rules off, {sm:6s} {k:6s}: medians {m}  median of medians {statistics.median(m):.2f} ms", flush=True)
    if "--trace" in args:
        out = os.environ.get("TRACE_DIR") or tempfile.mkdtemp(prefix="rules_trace_")
        step(["rocprofv3", "--kernel-trace", "--stats", "-d", out, "-o", "rules", "--output-format", "csv", "--"] + me + ["child", "trace"], 420)
        for path in glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True):
            for row in csv.DictReader(open(path)):
                name = row.get("Name", "")
                if any(k in name for k in ("decode_rules_plan", "argmax128", "sample128", "greedy_pick", "sample_pick")):
                    print(f"{name[:150]}: calls {row.get('Calls')}, mean {float(row.get('AverageNs', 'nan')) / 1e3:.2f} us", flush=True)


if __name__ == "__main__":
    main()
