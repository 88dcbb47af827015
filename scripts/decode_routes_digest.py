"""One SHA-256 line per decode route over the raw bytes of the ids and scores it returns: the tiny caption model of the tests
(Swin 32 / [2, 2, 2, 2] + BERT 256 x 2 layers x 4 heads, 3000 tokens, the hash weights of tests/golden/specs_hash.json) in f32
and bf16, through public calls only (``greedy_search``, ``sample_many``, ``generate``), so the script runs unchanged on any
commit that has them.  Run it once per tree on one GPU and ``diff`` the outputs: a refactor of the host loops must leave every
line as it was (``profiles/decode_one_loop.md``).

  --list            print the route names and exit
  --only NAME ...   run only these routes (one decode per process under a kernel trace: ``--only`` with one name)
  --dtype f32|bf16  one dtype only (default: both)
``MVLT_TREE``: the root of the built tree to import (default: the tree this file lies in).

Routes: greedy / sampled / filtered, each with and without a rule set, with and without a ragged prompt, under both values of
MVLT_DECODE_GRAPH (B = 3, 8 tokens); B = 66 on the eager loop (torch argmax, torch.multinomial behind ``torch.manual_seed``,
filtered, greedy + rules, sampled + rules); ``sample_many`` with and without the greedy row and the rules under both switch values;
an eos that stops the decode early for ``greedy_search`` and ``sample_many`` (20 tokens; the eos is taken from an eos-free run);
beam search with the scorer on the device under both switch values."""
import argparse
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RULES = dict(repetition_penalty=1.2, no_repeat_ngram_size=2, min_length=3)
FILTER = dict(top_k=5, top_p=0.9)


def routes():
    """name -> (kind, graph switch, keyword arguments)."""
    out = {}
    for g in ("1", "0"):
        for mode, kw in (("greedy", {}), ("sampled", dict(sample_mode='sample', seed=7)),
                         ("filtered", dict(sample_mode='sample', seed=7, temperature=0.8, **FILTER))):
            for rules in (False, True):
                for prompt in (False, True):
                    name = f"{mode}{'+rules' if rules else ''}{'+prompt' if prompt else ''}/graph={g}"
                    out[name] = ("prompt" if prompt else "greedy_search", g, dict(kw, **(RULES if rules else {})))
        for greedy_row in (True, False):
            for rules in (False, True):
                name = f"sample_many{'+greedy' if greedy_row else ''}{'+rules' if rules else ''}/graph={g}"
                out[name] = ("sample_many", g, dict(num_samples=2, include_greedy=greedy_row, seed=7, temperature=0.9, **(RULES if rules else {})))
        out[f"greedy+eos/graph={g}"] = ("eos_greedy", g, {})
        out[f"sample_many+eos/graph={g}"] = ("eos_many", g, dict(num_samples=2, include_greedy=True, temperature=0.05))
        out[f"beam_device/graph={g}"] = ("beam", g, dict(num_beams=3, device_scorer=True))
    for name, kw in (("greedy", {}), ("sampled", dict(sample_mode='sample')), ("filtered", dict(sample_mode='sample', seed=7, **FILTER)),
                     ("greedy+rules", dict(RULES)), ("sampled+rules", dict(sample_mode='sample', seed=7, **RULES))):
        out[f"B66/{name}"] = ("b66", "1", kw)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--list", action="store_true")
    ap.add_argument("--only", nargs="*")
    ap.add_argument("--dtype", choices=("f32", "bf16"))
    args = ap.parse_args()
    table = routes()
    if args.list:
        print("\n".join(table))
        return
    import torch
    sys.path.insert(0, os.environ.get("MVLT_TREE", HERE))
    import mvlt_amd as M
    from mvlt_amd import decode
    from mvlt_amd.arena import Arena
    from oracle.mvlt_oracle import hash_fill
    with open(os.path.join(HERE, "tests", "golden", "specs_hash.json")) as f:
        spec = json.load(f)["hash_tiny_caption"]
    sd = hash_fill([(k, tuple(s), getattr(torch, d)) for k, s, d in spec])
    g = torch.Generator().manual_seed(63)
    images = torch.randn(66, 3, 224, 224, generator=g)
    prompts = torch.randint(1000, 3000, (3, 5), generator=g)
    lens = [5, 0, 3]
    for dname, cd in (("f32", torch.float32), ("bf16", torch.bfloat16)):
        if args.dtype not in (None, dname):
            continue
        cfg = M.MVLBertConfigForImageCaption(hidden_size=256, num_hidden_layers=2, num_attention_heads=4, intermediate_size=1024,
                                             vocab_size=3000)
        cfg.swin.update(embed_dim=32, depths=[2, 2, 2, 2], num_heads=[1, 2, 4, 8], drop_path_rate=0.2)
        cfg.max_length, cfg.eos_token_id = 8, None
        tok = type("Tok", (), {"mask_token_id": 103, "sep_token_id": 102})()
        model = M.MVLBertForImageCaption(cfg, tokenizer=tok)
        model.load_state_dict(sd, strict=False)
        model = M.set_compute_dtype(model.cuda().eval(), cd)
        with torch.no_grad():
            Arena.of(model, cd)
            feat66 = model.conv(images.cuda())
        feat = feat66[:3].contiguous()
        pad = cfg.pad_token_id

        def common_eos(ids):
            """The token every row of an eos-free run reaches, the last row soonest; not all in one column where there is a choice."""
            rows = ids.reshape(-1, ids.shape[-1]).cpu().tolist()
            common = set(rows[0]).intersection(*rows[1:]) - {pad}
            if not common:
                return None
            return min(common, key=lambda c: (len({r.index(c) for r in rows}) == 1, max(r.index(c) for r in rows), c))

        for name, (kind, graph, kw) in table.items():
            if args.only and name not in args.only:
                continue
            os.environ["MVLT_DECODE_GRAPH"] = graph
            note = ""
            if kind == "greedy_search":
                out = decode.greedy_search(model, feat, **kw)
            elif kind == "prompt":
                out = decode.greedy_search(model, feat, input_ids=prompts.cuda(), prompt_lengths=lens, **kw)
            elif kind == "b66":
                torch.manual_seed(5)          # the multinomial route draws from torch's device generator
                out = decode.greedy_search(model, feat66, **kw)
            elif kind == "sample_many":
                out = decode.sample_many(model, feat, **kw)
            elif kind == "eos_greedy":          # images 0 and 2 twice: rows that share an image share an eos
                f4 = feat66[[0, 2, 0, 2]].contiguous()
                eos = common_eos(decode.greedy_search(model, f4, max_length=20)[0])
                out = decode.greedy_search(model, f4, max_length=20, eos_token_id=eos) if eos is not None else None
                note = f" eos={eos} columns={None if out is None else out[0].shape[1]}"
            elif kind == "eos_many":
                f2 = feat66[[0, 2]].contiguous()
                eos = seed = None
                for seed in range(16):
                    eos = common_eos(decode.sample_many(model, f2, seed=seed, max_length=20, **kw)[0])
                    if eos is not None:
                        break
                out = decode.sample_many(model, f2, seed=seed, max_length=20, eos_token_id=eos, **kw) if eos is not None else None
                note = f" eos={eos} seed={seed} columns={None if out is None else out[0].shape[-1]}"
            else:
                out = (model.generate(images[:3].cuda(), max_length=8, **kw),)
            torch.cuda.synchronize()
            h = hashlib.sha256()
            for t in (out or ()):
                h.update(t.contiguous().cpu().view(torch.uint8).numpy().tobytes())
            shapes = [tuple(t.shape) for t in (out or ())]
            print(f"{dname} {name}: {h.hexdigest() if out is not None else 'no common eos'} {shapes}{note}", flush=True)


if __name__ == "__main__":
    main()
