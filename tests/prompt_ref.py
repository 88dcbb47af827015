"""Inputs and the CPU oracle of the prompted-decode tests: row b's pick t is checked against the oracle's full recompute on
``[CLS] img_b [SEP] prompt_b y_<t [MASK]`` (``O.mvlbert_forward`` + ``O.mlm_head``, one row at a time: the rows' texts have
different lengths), the way tests/test_multi_sample_gpu.py checks its rows."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sample_ref as S  # noqa: E402
from conftest import synth_batch  # noqa: E402

B, MAX_LENGTH, P_MAX = 3, 8, 5
LENGTHS = [0, 2, 5]
IMAGE_SEED, PROMPT_SEED = 63, 4242
F32_TOL = 2e-4          # near-tie margin of an f32 logit, relative to the logits' spread (the f32 margin of the model tests)


def image():
    return synth_batch(B, 24, seed=IMAGE_SEED, vocab=3000)[0]


def prompts():
    """int64 [B, P_MAX] drawn from 1000..2999; row b's prompt is its first LENGTHS[b] ids, the rest is never looked at."""
    g = torch.Generator().manual_seed(PROMPT_SEED)
    return torch.randint(1000, 3000, (B, P_MAX), generator=g)


def oracle_cfgs():
    from oracle import mvlt_oracle as O
    scfg = O.SwinCfg(embed_dim=32, depths=(2, 2, 2, 2), num_heads=(1, 2, 4, 8), drop_path_rate=0.2)
    bcfg = O.BertCfg(vocab_size=3000, hidden_size=256, num_hidden_layers=2, num_attention_heads=4, intermediate_size=1024)
    return O, scfg, bcfg


def row_logits(O, sd, bcfg, feat_b, prefix):
    """f64 logits [V] of the [MASK] behind ``prefix`` (1-D int64: prompt + what was generated) for one image feature [1, n, H]."""
    inp = torch.cat([prefix.view(1, -1), torch.full((1, 1), bcfg.mask_token_id)], 1)
    o = O.mvlbert_forward(sd, bcfg, inp, feat_b, True)
    return O.mlm_head(o["hidden"][:, -1], sd, "MLM_head_seq2seq", bcfg).double()[0]


def teacher_forced(O, sd, bcfg, feat, prompt_ids, lengths, ids, seed=None, temperature=1.0, tol=F32_TOL, eos=None):
    """Every pick of ``ids`` [B, n] against the oracle on the row's own prompt and generated prefix.  seed None: greedy, the pick
    must be the argmax of the logits or within tol x (top - mean) of it and ``at`` holds the oracle's logit at the pick;
    otherwise the Gumbel-max pick of logits / temperature + the host noise of (seed, TAG0 + t, row b) and ``at`` holds the
    log-probability of the pick.  Rows stop being checked behind their eos.  Returns (exact, near, bad, at [B, n])."""
    Bn, n = ids.shape
    V = bcfg.vocab_size
    it = S.inv_t_f32(temperature)
    exact = near = 0
    bad, at = [], torch.zeros(Bn, n, dtype=torch.float64)
    noise = None if seed is None else [S.gumbel_ref(S.u01_ref(seed, S.TAG0 + t, Bn, V)) for t in range(n)]
    for b in range(Bn):
        for t in range(n):
            x = row_logits(O, sd, bcfg, feat[b:b + 1], torch.cat([prompt_ids[b, :lengths[b]], ids[b, :t]]))
            if seed is None:
                y = x
                at[b, t] = x[ids[b, t]]
            else:
                x = x * it
                y = x + noise[t][b]
                at[b, t] = torch.log_softmax(x, -1)[ids[b, t]]
            m = float(y.max() - y[ids[b, t]])
            spread = float(x.max() - x.mean())
            if m == 0.0:
                exact += 1
            elif m <= tol * spread:
                near += 1
            else:
                bad.append((b, t, m, spread))
            if eos is not None and int(ids[b, t]) == eos:
                break
    return exact, near, bad, at


def oracle_greedy(O, sd, bcfg, feat, prompt_ids, lengths, n, tol=F32_TOL):
    """The oracle's own greedy continuation [B, n] and the number of picks whose top-2 gap is inside the near-tie margin."""
    out = torch.zeros(len(lengths), n, dtype=torch.int64)
    close = 0
    for b in range(len(lengths)):
        for t in range(n):
            x = row_logits(O, sd, bcfg, feat[b:b + 1], torch.cat([prompt_ids[b, :lengths[b]], out[b, :t]]))
            top = torch.topk(x, 2).values
            close += int(float(top[0] - top[1]) <= tol * float(x.max() - x.mean()))
            out[b, t] = int(x.argmax())
    return out, close


def first_difference_is_a_near_tie(O, sd, bcfg, feat_b, prefix, got, want, tol=F32_TOL):
    """Sequences ``got`` / ``want`` behind the common ``prefix`` of one row: equal, or at the first difference both tokens are
    within the near-tie margin of each other under the oracle."""
    n = min(len(got), len(want))
    diff = (got[:n] != want[:n]).nonzero()
    if diff.numel() == 0:
        return True
    t = int(diff[0])
    x = row_logits(O, sd, bcfg, feat_b, torch.cat([prefix, want[:t]]))
    return abs(float(x[got[t]] - x[want[t]])) <= tol * float(x.max() - x.mean())
