"""Beam search at the report-generation shape (Swin-S + BERT-base, bf16, beams = 5, max_length = 150, eos_token_id = None so every
run has the same length), B = 8 and 32: the fused route (mvlt_gemm_beam_candidates + mvlt_attn_cached_beam, the default) next to
MVLT_BEAM_FUSED=0 (log_softmax + topk + a gather of every layer's cache per token: what beam_search did before the fused route
existed), interleaved round by round in ONE process after a warm-up round.  Prints per batch size and route the median ms per
batch with min / max over the rounds, then -- from one extra instrumented run per route -- the per-token split: head (device time
from the head product to the candidates), attention (the cached-attention launches), cache gather (plain route only), scorer
(host time in BeamScorer.process) and host sync (host time waiting in the read-back).
Two more routes run in the same rounds: the device scorer (mvlt_beam_step, MVLT_BEAM_DEVICE=1) as an eager loop
(MVLT_DECODE_GRAPH=0, "device") and as one replayed HIP graph per token ("graph"); both are compared with the fused host-scorer
route.  A replayed graph makes no per-token Python calls, so it has no per-token split.
RULES ("penalty,ngram,min_length", e.g. "1.2,3,10"; unset: none) adds every route once more with the logit rules switched on
("fused+rules", ...: model.generate, the plan launch and the rule-aware selection), interleaved with the rules-off decodes in the
same rounds of the same process, and prints on against off per route with the share of tokens the rules changed.
BATCHES ("8,32"), ROUNDS (5), MAXLEN (150), BEAMS (5), ROUTES ("fused,plain,device,graph"), SPLIT ("1"; "0": no per-token split)."""
import os, statistics, sys, time
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mvlt_amd as M
from mvlt_amd import decode, ops

torch.manual_seed(0)
BEAMS, MAXLEN, ROUNDS = int(os.environ.get("BEAMS", 5)), int(os.environ.get("MAXLEN", 150)), int(os.environ.get("ROUNDS", 5))
cfg = M.MVLBertConfigForImageCaption(); cfg.max_length = MAXLEN; cfg.eos_token_id = None
tok = type("Tok", (), {"mask_token_id": 103, "sep_token_id": 102})()
model = M.MVLBertForImageCaption(cfg, tokenizer=tok).cuda().eval()
ENV = {"fused": dict(MVLT_BEAM_FUSED="1", MVLT_BEAM_DEVICE="0", MVLT_DECODE_GRAPH="1"),
       "plain": dict(MVLT_BEAM_FUSED="0", MVLT_BEAM_DEVICE="0", MVLT_DECODE_GRAPH="1"),
       "device": dict(MVLT_BEAM_FUSED="1", MVLT_BEAM_DEVICE="1", MVLT_DECODE_GRAPH="0"),
       "graph": dict(MVLT_BEAM_FUSED="1", MVLT_BEAM_DEVICE="1", MVLT_DECODE_GRAPH="1")}
ROUTES = tuple((n, n) for n in os.environ.get("ROUTES", "fused,plain,device,graph").split(","))
RULES = os.environ.get("RULES")
RULES = (float(RULES.split(",")[0]), int(RULES.split(",")[1]), int(RULES.split(",")[2])) if RULES else None
RULED = tuple((n + "+rules", n) for n, _ in ROUTES) if RULES else ()


def run(img, flag, rules=None):
    os.environ.update(ENV[flag])
    torch.cuda.synchronize(); t = time.time()
    if rules is None:
        out = model(img, None, BEAMS, "unilm")
    else:
        out = model.generate(img, num_beams=BEAMS, repetition_penalty=rules[0], no_repeat_ngram_size=rules[1], min_length=rules[2])
    torch.cuda.synchronize()
    return (time.time() - t) * 1e3, out


class Split:
    """Device segments by event pairs, host segments by wall clock, for ONE run."""

    def __init__(self):
        self.ev, self.host = {"head": [], "attention": [], "cache gather": []}, {"scorer": 0.0, "host sync": 0.0}
        self.saved = []

    def device(self, name, fn):
        def wrapped(*a, **kw):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); out = fn(*a, **kw); e1.record()
            self.ev[name].append((e0, e1))
            return out
        return wrapped

    def wall(self, name, fn):
        def wrapped(*a, **kw):
            t = time.time(); out = fn(*a, **kw); self.host[name] += time.time() - t
            return out
        return wrapped

    def patch(self, obj, attr, new):
        self.saved.append((obj, attr, getattr(obj, attr)))
        setattr(obj, attr, new)

    def __enter__(self):
        head = model.MLM_head_seq2seq
        self.patch(ops, "gemm_beam_candidates", self.device("head", ops.gemm_beam_candidates))
        self.patch(ops, "attn_cached_beam", self.device("attention", ops.attn_cached_beam))
        self.patch(ops, "attn_cached", self.device("attention", ops.attn_cached))
        # plain route: the head segment runs from the logits product to the end of topk
        self.t0 = None
        real_logits, real_topk, real_sel = head._logits, torch.topk, torch.Tensor.index_select

        def logits(*a, **kw):
            self.t0 = torch.cuda.Event(enable_timing=True); self.t0.record()
            return real_logits(*a, **kw)

        def topk(*a, **kw):
            out = real_topk(*a, **kw)
            if self.t0 is not None:
                e1 = torch.cuda.Event(enable_timing=True); e1.record()
                self.ev["head"].append((self.t0, e1)); self.t0 = None
            return out

        def sel(t, *a, **kw):
            return (self.device("cache gather", real_sel) if t.dim() == 4 else real_sel)(t, *a, **kw)

        self.patch(head, "_logits", logits)
        self.patch(torch, "topk", topk)
        self.patch(torch.Tensor, "index_select", sel)
        self.patch(decode.BeamScorer, "process", self.wall("scorer", decode.BeamScorer.process))
        self.patch(torch.Tensor, "cpu", self.wall("host sync", torch.Tensor.cpu))
        self.patch(torch.Tensor, "tolist", self.wall("host sync", torch.Tensor.tolist))
        return self

    def __exit__(self, *exc):
        for obj, attr, old in reversed(self.saved):
            setattr(obj, attr, old)
        torch.cuda.synchronize()

    def per_token(self):
        out = {k: 1e3 * sum(a.elapsed_time(b) for a, b in v) / MAXLEN for k, v in self.ev.items()}
        out.update({k: 1e6 * v / MAXLEN for k, v in self.host.items()})
        return out


for B in [int(b) for b in os.environ.get("BATCHES", "8,32").split(",")]:
    img = torch.randn(B, 3, 224, 224, device="cuda")
    times, outs = {name: [] for name, _ in ROUTES + RULED}, {}
    for r in range(ROUNDS + 1):                       # round 0 warms up
        for name, flag in ROUTES + RULED:
            ms, outs[name] = run(img, flag, RULES if name.endswith("+rules") else None)
            if r:
                times[name].append(ms)
    def same_as_fused(name):
        return outs["fused"].shape == outs[name].shape and bool((outs["fused"] == outs[name]).all())

    for name, _ in ROUTES + RULED:
        v = times[name]
        print(f"B={B:3d} beams={BEAMS} {name:12s} median {statistics.median(v):8.2f} ms/batch  (min {min(v):.2f} max {max(v):.2f}, spread "
              f"{max(v) - min(v):.2f} over {len(v)} rounds)", flush=True)
    if "plain" in times and "fused" in times:
        gain = statistics.median(times["plain"]) - statistics.median(times["fused"])
        print(f"B={B:3d} fused is {gain:+.2f} ms/batch ({1e3 * gain / MAXLEN:+.1f} us/token) against a plain-route spread of "
              f"{max(times['plain']) - min(times['plain']):.2f} ms; same sequences on both routes (random weights, bf16 against f32 logits): "
              f"{same_as_fused('plain')}", flush=True)
    for name in ("device", "graph"):          # the device scorer against the host scorer on the same (fused) kernels
        if name in times and "fused" in times:
            gain = statistics.median(times["fused"]) - statistics.median(times[name])
            print(f"B={B:3d} {name} is {gain:+.2f} ms/batch ({1e3 * gain / MAXLEN:+.1f} us/token) against fused, whose spread is "
                  f"{max(times['fused']) - min(times['fused']):.2f} ms ({name}: {max(times[name]) - min(times[name]):.2f}); same sequences as "
                  f"fused: {same_as_fused(name)}", flush=True)
    for name, _ in RULED:          # rules on against off, the same route in the same rounds
        off = name[:-len("+rules")]
        cost = statistics.median(times[name]) - statistics.median(times[off])
        a, b = outs[name], outs[off]
        w = min(a.shape[1], b.shape[1])
        print(f"B={B:3d} {name} {RULES} is {cost:+.2f} ms/batch ({1e3 * cost / MAXLEN:+.1f} us/token) against {off}, whose spread is "
              f"{max(times[off]) - min(times[off]):.2f} ms; tokens changed by the rules: {100.0 * float((a[:, :w] != b[:, :w]).float().mean()):.1f} %; "
              f"same sequences as fused+rules: {outs['fused+rules'].shape == a.shape and bool((outs['fused+rules'] == a).all()) if 'fused+rules' in outs else None}",
              flush=True)
    for name, flag in ROUTES:
        if name == "graph" or os.environ.get("SPLIT", "1") == "0":
            continue
        with Split() as sp:
            run(img, flag)
        print(f"B={B:3d} {name:6s} per token [us]: " + "  ".join(f"{k} {v:7.1f}" for k, v in sp.per_token().items()), flush=True)
