"""The joints of the BERT side, per element, in the models' own calls: what happens BETWEEN the kernels in bert.py
MVLBert._forward / _backward and in model.py -- the embedding ends, the pooler and its dgrad into the [CLS] rows, the
labelled-row gather / scatter, _MlmLossFn on both loss routes, _LinearCEFn, _LinearFn, _TransformLinearFn, _FeatureProjFn,
Conv_layer's pair reshaping and the row arithmetic of the heads -- which the suite judged by whole-model norms only.

A recorder wraps MVLBert._forward / _backward / _layer_fwd / _layer_bwd on the test's model instance and the forward / backward
of _MlmLossFn, _GatherRowsFn, _LinearCEFn, _LinearFn, _TransformLinearFn and _FeatureProjFn on their classes for the duration
of a run; it taps arguments and results and changes nothing (it clones what a later kernel overwrites in place: the logits,
which the cross-entropy backward turns into dl, and the dx a layer's backward is handed).  The image tower is a stub that
returns a leaf image_feature [B, 49, H]; dimg is its .grad.  Every joint is judged by tests/bert_joints_ref.py (its docstring
states the joints and the bounds; no tolerance of its own) one stage deep from the tensors that were really handed over.  The
three intermediates of a head's backward that nobody stores (dt2, dt1, dpre) come from a replay of those launches through
mvlt_amd.ops on the run's own saved tensors, as tests/test_bert_layer_gpu.py replays a layer; the kernels are deterministic.
Every encoder layer's recorded call is also judged by bert_layer_ref.reference (chained).

Shapes: two layers, vocab_size 3000 (ld = 3008: 8 pad columns, the last 64-column group straddles V), n_img = 49, B = 4,
T = 80 with caption lengths (80, 13, 0, 41), T = 23 for the dense cases; H = 768 / I = 3072 in bf16 and f32, H = 128 / I = 512
in f32.  The labels (bert_joints_ref.make_batch, asserted by check_label_requirements): sample 1 has none, sample 2 has no
caption, sample 0 is labelled at its last kept position, id 777 stands four times, 19 labels in all (not a multiple of 16,
below one row tile).  Every pretraining run backs up from 0.75 loss, so a dloss that does not reach a branch shows.

Runs (RUNS; each on both host paths, the coin flip chosen per run and asserted from last_seq2seq): the default route (autopack,
labelled rows first, early label plan) in bf16 768 / f32 128 / f32 768; the fused loss route (model._HEAD_CE_AB); labelled rows
first off; mlm_max_labels_per_sample below the real count (NaN loss, asserted, no backward) and above; text_lengths right and
one too short (NaN); auto_pack_rows off; image_mask; MLM_task off; ITM_task off (pooler.dense keeps grad None); the label_sync
fake (2.5 x count, no process group); the encoder alone with a gradient on every row of hidden (the heads leave the [CLS] rows
of dhidden zero, where adding the pooler's dgrad and overwriting with it are the same); caption forward(..., labels=) 'unilm'
and 'normal' and the slots of caption_logprobs; VQA train / eval; retrieval with and without labels; a pair batch through the
real Conv_layer with feature_proj around a stubbed Swin tower.
Before each run NaN blocks go back to the caching allocator; every checked output must be finite; rows that must not be written
are compared with zero bit for bit; the two host paths of a case are bit-equal in everything recorded except the float-atomic
word table (1e-6 of its norm, as test_encoder_is_the_same_on_both_host_paths holds it).
The cross-entropy loss sums are added by float atomics too (misc_ref: arbitrary order): acc[0], the losses and the total are held to
their float64 bounds in every run and to 1e-6 between the host paths, not bit for bit.
Not pinned here: that the rows of `hidden` at or beyond the packed total keep a sentinel -- the encoder allocates them itself, so
the test has nothing to fill them with; what is read from them would show as a non-finite or out-of-bound value downstream.
No hand-off timeout is touched, no failure path is provoked, nothing runs in a child process.

Measured on an MI355X, worst ratio to the bound over every run and both host paths (test_worst_ratios_summary prints them).
bf16: GEMM outputs one stage deep (mlm pre / t1 / logits / dt2 / dx, itm logits / dx, vqa logits / dx, retrieval pre / t1 / dt2 /
dx, feature_proj y / dx) 0.84 .. 0.995; LayerNorm, elementwise and cross-entropy outputs (t2, dt1, dpre, dl) 0.50; pooled 0.57
(pre's bound carried); the pooler's dgrad on the [CLS] rows 0.15, pooler.weight / .bias 0.48 / 0.38 (dpre's bound carried);
decoder.weight 0.16, every other head gradient at most 0.08; lse / nll 0.016 / 0.016 (0.03 for the ITM head), loss 0.71; the
embedding tables word 0.07, position / token_type at most 0.01; the encoder layers as the chained judgement of
tests/test_bert_layer_gpu.py (qkv / h / act / y1 / y2 0.96 .. 0.98, x1 / x2 0.50, fc2.weight 0.42, everything behind dx1 0.000).
f32: at most 0.40 (dpre and dl: ERFC_ABS and the exponential, as in the sibling files) except _LinearFn's dropped-out input 0.58
and the loss 0.93 -- its bound is ONE rounding of the division acc[0] / acc[1], which a correctly rounded quotient may reach.
The pattern is the siblings': a GEMM output judged one stage deep stands just below 1 because gemm_ref has no safety factor.
The file takes 8.3 s alone (99 tests; the first run pays 3.2 s of start-up, no other test more than 0.4 s) and 4.6 s inside the
whole suite, where the start-up is already paid."""
import random

import pytest
import torch

import bert_joints_ref as J
import bert_layer_ref as H
import gemm_ref as G
import misc_ref as Mi
from bert_joints_ref import BF, F32
from test_bert_layer_gpu import poison

pytestmark = pytest.mark.gpu

N_IMG, B, V = 49, 4, 3000
SEED, DLOSS, SYNC = 4321, 0.75, 2.5
WIDTHS = {"bf16-768": (768, 3072, BF), "f32-128": (128, 512, F32), "f32-768": (768, 3072, F32)}
# run -> (width, seq2seq flip, T, settings)
RUNS = {
    "default-bf16": ("bf16-768", True, 80, {}),
    "default-f32": ("f32-128", False, 80, {}),
    "default-f32-768": ("f32-768", True, 80, {}),
    "fused-bf16": ("bf16-768", True, 80, dict(fused=True)),                   # (the flips of the default runs: the same operands)
    "fused-f32": ("f32-128", False, 80, dict(fused=True)),
    "allrows-bf16": ("bf16-768", False, 80, dict(cfg=dict(mlm_labelled_rows_first=False))),
    "allrows-f32": ("f32-128", True, 80, dict(cfg=dict(mlm_labelled_rows_first=False))),
    "cap-above-f32": ("f32-128", False, 80, dict(cfg=dict(mlm_max_labels_per_sample=8), cap=8)),
    "cap-below-f32": ("f32-128", True, 80, dict(cfg=dict(mlm_max_labels_per_sample=4), cap=4, nan=True)),
    "lengths-bf16": ("bf16-768", True, 80, dict(lengths="right")),
    "lengths-f32": ("f32-128", False, 80, dict(lengths="right")),
    "lengths-short-f32": ("f32-128", True, 80, dict(lengths="short", nan=True)),
    "dense-bf16": ("bf16-768", False, 23, dict(cfg=dict(auto_pack_rows=False))),
    "dense-f32": ("f32-128", True, 23, dict(cfg=dict(auto_pack_rows=False))),
    "image-mask-f32": ("f32-128", False, 23, dict(image_mask=True)),
    "mlm-off-f32": ("f32-128", True, 80, dict(cfg=dict(MLM_task=False))),
    "itm-off-bf16": ("bf16-768", True, 80, dict(cfg=dict(ITM_task=False))),
    "itm-off-f32": ("f32-128", False, 80, dict(cfg=dict(ITM_task=False))),
    "sync-bf16": ("bf16-768", True, 80, dict(sync=True)),                     # (the flips of the default runs again)
    "sync-f32": ("f32-128", False, 80, dict(sync=True)),
}
_models, _runs, _worst = {}, {}, {}


class Stub(torch.nn.Module):
    """Stands where the image tower stands: returns a leaf that requires grad, keeps what it was called with."""

    def __init__(self):
        super().__init__()
        self.feat = self.out = self.seen = None

    def forward(self, image, **kw):
        self.seen = image
        self.out = self.feat.clone().requires_grad_(True)
        return self.out


def init_weights(m):
    """One-dimensional parameters away from 0 / 1, weights with unit-variance outputs, qkv as tests/test_bert_layer_gpu.py."""
    import math

    import attn_ref as A
    g = torch.Generator().manual_seed(72)
    for n, p in m.named_parameters():
        if p.dim() == 1:
            p.data.copy_((1.0 if n.endswith("LayerNorm.weight") else 0.0) + 0.1 * torch.randn(p.shape, generator=g))
        elif "embeddings" not in n:
            p.data.copy_(torch.randn(p.shape, generator=g) * p.shape[1] ** -0.5)
    for layer in m.MVLBert.encoder.layer:
        sa = layer.attention.self
        for lin in (sa.query, sa.key):
            lin.weight.data.mul_(math.sqrt(A.LOGIT_STD))


def model_of(kind, width):
    if (kind, width) not in _models:
        import mvlt_amd as M
        Hd, I, dt = WIDTHS[width]
        cls, ccls = {"pretrain": (M.MVLBertForPretraining, M.MVLBertPretrainConfig), "vqa": (M.MVLBertForVQA, M.MVLBertConfigforVQA),
                     "retrieval": (M.MVLBertForRetrieval, M.MVLBertRetrieval),
                     "caption": (M.MVLBertForImageCaption, M.MVLBertConfigForImageCaption)}[kind]
        cfg = ccls(hidden_size=Hd, num_hidden_layers=2, num_attention_heads=Hd // 64, intermediate_size=I, vocab_size=V)
        cfg.ITM_task = True
        cfg.hidden_dropout_prob = cfg.attention_probs_dropout_prob = 0.1
        cfg.swin.update(embed_dim=32, depths=[2, 2, 2, 2], num_heads=[1, 2, 4, 8])          # (replaced below: never run)
        cfg.swin_feature_proj = True
        torch.manual_seed(71)
        m = cls(cfg)
        m.conv = Stub()
        init_weights(m)
        from mvlt_amd.arena import Arena
        _models[kind, width] = M.set_compute_dtype(m.cuda().train(), dt)
        Arena.of(m, dt)                                  # one arena for the whole model, as the models' forward makes it
    return _models[kind, width]


# ------------------------------------------------------------------ the recorder
def fn_classes():
    from mvlt_amd import model as MM
    return (MM._MlmLossFn, MM._GatherRowsFn, MM._LinearCEFn, MM._LinearFn, MM._TransformLinearFn, MM._FeatureProjFn)


def tap_function(mp, cls, store):
    f0, b0 = cls.forward, cls.backward
    logits_at = {"_MlmLossFn": 8, "_LinearCEFn": 3}.get(cls.__name__)

    def fwd(ctx, *a):
        out = f0(ctx, *a)
        e = dict(args=a, out=out, saved=getattr(ctx, "saved", None))
        if logits_at is not None and e["saved"] is not None and e["saved"][logits_at] is not None:
            e["logits0"] = e["saved"][logits_at].detach().clone()          # the backward overwrites the buffer with dl
        ctx._joints_entry = e
        store.setdefault(cls.__name__, []).append(e)
        return out

    def bwd(ctx, *g):
        e = ctx._joints_entry
        e["grads"] = tuple(None if t is None else t.detach().clone() for t in g)
        out = b0(ctx, *g)
        e["bwd_out"] = out
        return out

    mp.setattr(cls, "forward", staticmethod(fwd))
    mp.setattr(cls, "backward", staticmethod(bwd))


def tap_encoder(mp, enc, rec):
    f0, b0, lf0, lb0 = enc._forward, enc._backward, enc._layer_fwd, enc._layer_bwd

    def t_forward(*a, **k):
        out = f0(*a, **k)
        rec["enc_fwd"].append(dict(args=a, kw=k, out=out))
        return out

    def t_backward(sv, dhidden, dpooled):
        e = dict(sv=sv, dhidden=None if dhidden is None else dhidden.detach().clone(),
                 dpooled=None if dpooled is None else dpooled.detach().clone())
        e["dimg"] = b0(sv, dhidden, dpooled)
        rec["enc_bwd"].append(e)
        return e["dimg"]

    def t_lf(ar, i, x, c, save):
        out = lf0(ar, i, x, c, save)
        rec["lf"].append(dict(i=i, x=x, c=c, x2=out[0], sv=None if out[1] is None else list(out[1])))
        return out

    def t_lb(ar, i, saved, dx, c):
        e = dict(i=i, dx=dx.detach().clone())
        e["dx_in"] = lb0(ar, i, saved, dx, c)
        rec["lb"].append(e)
        return e["dx_in"]

    for name, fn in (("_forward", t_forward), ("_backward", t_backward), ("_layer_fwd", t_lf), ("_layer_bwd", t_lb)):
        mp.setattr(enc, name, fn)


def seed_for_flip(want):
    s = next(s for s in range(64) if (random.Random(s).random() < 0.5) == want)
    random.seed(s)


def grads_of(m, ar):
    return {n: ar.grad_view(p).view(p.shape).detach().clone() for n, p in m.named_parameters() if p.grad is not None}


def recorded(m, native, call, backward_of=None, dout=None, extra=None):
    """One forward (and backward) of `m` with the recorder on.  call(m) -> the model's output; backward_of(out) -> the scalar or
    tensor to back up from (None: no backward).  -> the raw record."""
    import mvlt_amd as M
    from mvlt_amd import ops
    from mvlt_amd.arena import Arena
    from mvlt_amd.runtime import compute_dtype_of
    rec = dict(enc_fwd=[], enc_bwd=[], lf=[], lb=[], fn={})
    dt = compute_dtype_of(m)
    Hd, I = m.config.hidden_size, m.config.intermediate_size
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(ops, "NATIVE", native)
        for k, v in (extra or {}).items():
            mp.setattr(*k, v, raising=False)
        tap_encoder(mp, m.MVLBert, rec)
        for cls in fn_classes():
            tap_function(mp, cls, rec["fn"])
        M.manual_seed(SEED)
        m.zero_grad(set_to_none=True)
        rows = B * (N_IMG + 2 + 80)
        poison([(rows, 3 * Hd), (rows, Hd), (rows, I), (rows, Hd), (B * 80, J.ceil_to(V, 64)), (B * 80, Hd)], dt, torch.device("cuda"))
        out = call(m)
        rec["out"] = out
        if backward_of is not None:
            t = backward_of(out)
            t.backward(dout if dout is not None else torch.tensor(DLOSS, device=t.device))
        torch.cuda.synchronize()
        if native:
            ops.host().side_release()
        rec["ar"] = Arena.of(m, dt)
        rec["grads"] = grads_of(m, rec["ar"]) if backward_of is not None else {}
        rec["none_grads"] = {n for n, p in m.named_parameters() if p.grad is None}
        rec["dimg"] = None if m.conv.out is None or m.conv.out.grad is None else m.conv.out.grad.detach().clone()
        rec["replay"] = replay_heads(m, rec)
        torch.cuda.synchronize()
    rec.update(dt=dt, native=native)
    return rec


def replay_heads(m, rec):
    """The three backward stages of a transform head that nobody stores, launched one by one from the definition on the run's
    own saved tensors: {Function name: dict(dt2, dt1, dpre)}.  Parameter gradients go to scratch buffers."""
    from mvlt_amd import ops
    out = {}
    for name in ("_MlmLossFn", "_TransformLinearFn"):
        for e in rec["fn"].get(name, []):
            if "bwd_out" not in e or e["saved"] is None:
                continue
            if name == "_MlmLossFn":
                ar, Vn, x, pre, t1, t2, mean, rstd, logits, labels, lse, acc, rd = e["saved"]
                pr = e["args"][2].predictions
                ln, wdec = pr.transform.LayerNorm, pr.decoder.weight
                dl = logits[:, :Vn]                                       # after the backward: dl, in place
                dt2 = ops.gemm(dl, ar.compute(wdec), b_kmajor=True, m_dev=rd, split_k=8 if rd is not None else 0)
            else:
                ar, Vn, x, pre, t1, t2, mean, rstd = e["saved"]
                tr, lin = e["args"][2], e["args"][3]
                ln, rd = tr.LayerNorm, None
                dl = e["grads"][0].to(x.dtype).contiguous()
                dt2 = ops.gemm(dl, ar.compute(lin.weight), b_kmajor=True)
            tmp = lambda: torch.empty(x.shape[1], dtype=torch.float32, device=x.device)          # noqa: E731
            dt1 = ops.layernorm_bwd(dt2, t1, mean, rstd, ln.weight.data, tmp(), tmp(), rows_dev=rd)
            dpre = ops.gelu_bwd(pre, dt1)
            out[name] = dict(dt2=dt2, dt1=dt1, dpre=dpre)
    return out


# ------------------------------------------------------------------ from the raw record to what bert_joints_ref judges
def head_params(ar, head):
    pr = head.predictions
    return dict(wt=ar.compute(pr.transform.dense.weight), bt=pr.transform.dense.bias.data, gamma=pr.transform.LayerNorm.weight.data,
                beta=pr.transform.LayerNorm.bias.data, wd=ar.compute(pr.decoder.weight), bd=pr.decoder.bias.data)


def head_grad_names(prefix):
    p = prefix + ".predictions."
    return {"decoder.weight": p + "decoder.weight", "decoder.bias": p + "decoder.bias", "ln.weight": p + "transform.LayerNorm.weight",
            "ln.bias": p + "transform.LayerNorm.bias", "transform.weight": p + "transform.dense.weight",
            "transform.bias": p + "transform.dense.bias"}


def record_of(raw, m, ids, labels, *, layout, lab_first, fused, T, seq_len=None, row_start=None, cap=None, sync=None, first=None,
              head_name=None, nan=False):
    """The normalised record bert_joints_ref.judge_pretrain reads."""
    enc = m.MVLBert
    ar, dt, g = raw["ar"], raw["dt"], raw["grads"]
    Hd = m.config.hidden_size
    ef = raw["enc_fwd"][0]
    hidden, pooled, sv = ef["out"]
    rec = dict(dt=dt, B=B, T=T, n_img=N_IMG, V=V, eps=1e-12, dloss=DLOSS, fused=fused, lab_first=lab_first, layout=layout, cap=cap,
               sync=sync, first=first, nan=nan, ids=ids, labels=labels, seq_len=seq_len, row_start=row_start, image=m.conv.feat,
               word=enc.word_embeddings.weight.data, pos=enc.position_embeddings.weight.data, typ=enc.token_type_embeddings.weight.data,
               hidden=hidden.detach().reshape(-1, Hd), x0=raw["lf"][0]["x"])
    alloc = rec["hidden"].shape[0]
    if pooled is not None:
        rec.update(cls=sv["cls"], wp=ar.compute(enc.pooler.dense.weight), bp=enc.pooler.dense.bias.data, pooled=pooled.detach())
    back = bool(raw["enc_bwd"])
    if back:
        eb = raw["enc_bwd"][0]
        dh = eb["dhidden"]
        rec["dhidden"] = torch.zeros(alloc, Hd, dtype=dt, device=hidden.device) if dh is None else dh.reshape(-1, Hd)
        rec["dpooled"] = eb["dpooled"]
        last = next(e for e in raw["lb"] if e["i"] == len(enc.encoder.layer) - 1)
        rec["dx_last"] = last["dx"]
        rec["dx0"] = next(e for e in raw["lb"] if e["i"] == 0)["dx_in"].detach().reshape(-1, Hd)
        rec["dimg"] = raw["dimg"]
        rec.update(g_word=g["MVLBert.word_embeddings.weight"], g_pos=g["MVLBert.position_embeddings.weight"],
                   g_typ=g["MVLBert.token_type_embeddings.weight"])
        if eb["dpooled"] is not None:
            rec.update(g_wp=g["MVLBert.pooler.dense.weight"], g_bp=g["MVLBert.pooler.dense.bias"])
    ml = raw["fn"].get("_MlmLossFn")
    if ml:
        e = ml[0]
        _, x, head, lab, _, rd, _, _ = e["args"]
        sar, Vn, sx, pre, t1, t2, mean, rstd, logits, slab, lse, acc, srd = e["saved"]
        assert Vn == V and sx.data_ptr() == x.data_ptr()
        mrec = dict(head_params(sar, head), x=x.detach(), labels=lab, gather_row=None, rd=None if rd is None else int(rd),
                    pre=pre, t1=t1, t2=t2, mean=mean, rstd=rstd, logits=e["logits0"], lse=lse, acc=acc, nll=acc[0], loss=e["out"].detach())
        ga = raw["fn"].get("_GatherRowsFn")
        if ga:
            mrec["gather_row"] = ga[0]["args"][1]
            assert ga[0]["out"].data_ptr() == x.data_ptr() or torch.equal(ga[0]["out"], x)
        if "bwd_out" in e:
            mrec.update(dl=logits, dx=e["bwd_out"][1], dloss_seen=float(e["grads"][0]), **raw["replay"]["_MlmLossFn"])
            for k, n in head_grad_names(head_name).items():
                mrec[k] = g[n]
        rec["mlm"] = detached(mrec)
    it = raw["fn"].get("_LinearCEFn")
    if it:
        e = it[0]
        _, x, lin, lab, _ = e["args"]
        sar, Vn, sx, logits, slab, lse, acc = e["saved"]
        irec = dict(x=x.detach(), w=sar.compute(lin.weight), b=lin.bias.data, labels=lab, logits=e["logits0"], lse=lse, acc=acc,
                    loss=e["out"].detach())
        if "bwd_out" in e:
            irec.update(dl=logits, dx=e["bwd_out"][1], dloss_seen=float(e["grads"][0]), weight=g["ITM_mlp.weight"], bias=g["ITM_mlp.bias"])
        rec["itm"] = detached(irec)
    if ml and it:
        rec["total"] = raw["out"].detach()
    return detached(rec)


def layer_judgement(raw, m, ids, *, s2s, T, seq_len, image_mask=None):
    """bert_layer_ref.reference (chained) of every recorded encoder-layer call -> (failures, worst ratios)."""
    enc = m.MVLBert
    ar, dt, g, native = raw["ar"], raw["dt"], raw["grads"], raw["native"]
    Hd, I = m.config.hidden_size, m.config.intermediate_size
    train = m.training
    bad, ratios = {}, {}
    for f in raw["lf"]:
        i = f["i"]
        b = next(e for e in raw["lb"] if e["i"] == i)
        layer = enc.encoder.layer[i]
        sa, so, li, lo = layer.attention.self, layer.attention.output, layer.intermediate, layer.output
        if native:
            sx, qkv, ctx, lse, y1, st1, x1, h, act, y2, st2 = f["sv"]
            mean1, rstd1, mean2, rstd2 = st1[0], st1[1], st2[0], st2[1]
        else:
            sx, qkv, ctx, lse, y1, mean1, rstd1, x1, h, act, y2, mean2, rstd2 = f["sv"]
        run = dict(x=f["x"], dx=b["dx"], qkv=qkv, ctx=ctx, lse=lse, y1=y1, mean1=mean1, rstd1=rstd1, x1=x1, h=h, act=act, y2=y2,
                   mean2=mean2, rstd2=rstd2, x2=f["x2"], dx_in=b["dx_in"],
                   wq=ar.compute(sa.query.weight), wk=ar.compute(sa.key.weight), wv=ar.compute(sa.value.weight),
                   bq=sa.query.bias.data, bk=sa.key.bias.data, bv=sa.value.bias.data,
                   wo=ar.compute(so.dense.weight), bo=so.dense.bias.data, g1=so.LayerNorm.weight.data, b1=so.LayerNorm.bias.data,
                   wi=ar.compute(li.dense.weight), bi=li.dense.bias.data, wo2=ar.compute(lo.dense.weight), bo2=lo.dense.bias.data,
                   g2=lo.LayerNorm.weight.data, b2=lo.LayerNorm.bias.data)
        pre = f"MVLBert.encoder.layer.{i}."
        for k, n in (("query.weight", "attention.self.query.weight"), ("key.weight", "attention.self.key.weight"),
                     ("value.weight", "attention.self.value.weight"), ("query.bias", "attention.self.query.bias"),
                     ("key.bias", "attention.self.key.bias"), ("value.bias", "attention.self.value.bias"),
                     ("o.weight", "attention.output.dense.weight"), ("o.bias", "attention.output.dense.bias"),
                     ("ln1.weight", "attention.output.LayerNorm.weight"), ("ln1.bias", "attention.output.LayerNorm.bias"),
                     ("fc1.weight", "intermediate.dense.weight"), ("fc1.bias", "intermediate.dense.bias"),
                     ("fc2.weight", "output.dense.weight"), ("fc2.bias", "output.dense.bias"),
                     ("ln2.weight", "output.LayerNorm.weight"), ("ln2.bias", "output.LayerNorm.bias")):
            run[k] = g[pre + n]
        p = 0.1 if train else 0.0
        case = dict(H=Hd, nH=Hd // 64, I=I, B=B, T=T, n_img=N_IMG, dtype=dt, s2s=s2s, p_h=p, p_a=p, seed=enc.last_seed, layer=i,
                    eps=1e-12, ids=None if s2s else ids, image_mask=image_mask, lens=seq_len)
        run = {k: v.detach().reshape(-1, v.shape[-1]) if k in ("x", "dx", "x2", "dx_in") else v.detach() for k, v in run.items()}
        ref = H.reference(run, case)
        for k, v in H.worst_ratios(ref).items():
            ratios[f"layer{i} {k}"] = v
        for k, msg in H.failures(ref, f"layer {i}").items():
            bad[f"layer{i} {k}"] = msg
    return bad, ratios


def detached(r):
    return {k: v.detach() if torch.is_tensor(v) else v for k, v in r.items()}


def note(label, dt, ratios):
    for k, v in ratios.items():
        key = ("bf16" if dt == BF else "f32", k.split(" ", 1)[0].rstrip("01"), k.split(" ", 1)[1])
        _worst[key] = max(_worst.get(key, 0.0), v)
        print(f"{label:28s} {k:30s} worst ratio to the bound {v:.3f}")


# ------------------------------------------------------------------ pretraining
def pretrain_run(name, native):
    if (name, native) in _runs:
        return _runs[name, native]
    from mvlt_amd import model as MM
    width, s2s, T, opt = RUNS[name]
    Hd, I, dt = WIDTHS[width]
    m = model_of("pretrain", width)
    ids, labels, itm, lens = J.make_batch(T)
    total = J.check_label_requirements(ids, labels, list(lens))
    assert total == 19
    g = torch.Generator().manual_seed(900 + T)
    m.conv.feat = torch.randn(B, N_IMG, Hd, generator=g).to(dt).cuda()
    cfg = dict(dict(mlm_labelled_rows_first=True, auto_pack_rows=True, MLM_task=True, ITM_task=True, mlm_max_labels_per_sample=None),
               **opt.get("cfg", {}))
    extra = {(m.config, k): v for k, v in cfg.items()}
    extra[(MM, "_HEAD_CE_AB")] = bool(opt.get("fused"))
    kw = {}
    image_mask = None
    if opt.get("image_mask"):
        image_mask = torch.ones(B, N_IMG, dtype=torch.uint8)
        image_mask[0, 3] = image_mask[1, 0] = image_mask[1, 17] = image_mask[B - 1, 48] = 0
        kw["image_mask"] = image_mask.cuda()
    text_lengths = None
    if opt.get("lengths"):
        text_lengths = list(lens)
        if opt["lengths"] == "short":
            text_lengths[3] -= 1                                     # sample 3 is labelled at its last kept position
        kw["text_lengths"] = torch.tensor(text_lengths)
    dummy = torch.zeros(B, 3, 8, 8).cuda()
    ids_d, labels_d, itm_d = ids.cuda(), labels.cuda(), itm.cuda()

    def call(model):
        if opt.get("sync"):
            model.__dict__["_mvlt_label_sync"] = lambda count: SYNC * count
        try:
            seed_for_flip(s2s)
            return model(dummy, ids_d, labels_d, itm_d, **kw)
        finally:
            model.__dict__.pop("_mvlt_label_sync", None)

    raw = recorded(m, native, call, None if opt.get("nan") else (lambda out: out), extra=extra)
    assert m.last_seq2seq == s2s, "the coin flip of this run"
    auto = cfg["auto_pack_rows"] and image_mask is None and text_lengths is None
    layout = "auto" if auto else "packed" if (text_lengths is not None and image_mask is None) else "dense"
    seq_len = row_start = None
    if layout == "auto":
        row_start, seq_len, _, _ = J.pack_plan_host(ids, labels, N_IMG)
    elif layout == "packed":
        seq_len = [n + N_IMG + 2 for n in text_lengths]
        row_start = [sum(seq_len[:b]) for b in range(B)]
    cap = opt.get("cap")
    lab_first = auto and cfg["mlm_labelled_rows_first"] and not (cap is not None and cap * B < B * T)
    rec = record_of(raw, m, ids, labels, layout=layout, lab_first=lab_first, fused=bool(opt.get("fused")), T=T, seq_len=seq_len,
                    row_start=row_start, cap=cap, sync=SYNC if opt.get("sync") else None,
                    head_name="MLM_head_seq2seq" if s2s else "MLM_head_bidir", nan=bool(opt.get("nan")))
    label = "%s-%s" % (name, "native" if native else "python")
    bad, ratios = J.judge_pretrain(rec, label)
    if not opt.get("nan"):
        lbad, lratios = layer_judgement(raw, m, ids, s2s=s2s, T=T, seq_len=seq_len, image_mask=image_mask)
        bad.update(lbad)
        ratios.update(lratios)
    note(label, dt, ratios)
    _runs[name, native] = dict(raw=raw, rec=rec, bad=bad, ratios=ratios, opt=opt, cfg=cfg, s2s=s2s, dt=dt)
    return _runs[name, native]


@pytest.mark.parametrize("native", [True, False], ids=["native", "python"])
@pytest.mark.parametrize("name", list(RUNS))
def test_pretraining_joints_against_float64(name, native):
    r = pretrain_run(name, native)
    assert not r["bad"], "\n".join(r["bad"].values())
    raw, rec, opt, cfg = r["raw"], r["rec"], r["opt"], r["cfg"]
    out = raw["out"]
    if opt.get("nan"):
        assert bool(torch.isnan(out).all()), "too many labels for the capacity / a label beyond the stated length: the loss is NaN"
        assert bool(torch.isfinite(rec["mlm"]["loss"]).all())          # (the head's own loss is ordinary arithmetic)
        return
    assert bool(torch.isfinite(out).all())
    for k, v in raw["grads"].items():
        assert bool(torch.isfinite(v).all()), (k, "not finite")
    other = "MLM_head_bidir" if r["s2s"] else "MLM_head_seq2seq"
    assert all(n in raw["none_grads"] for n in head_grad_names(other).values()), "the head of the other flip gets no gradient"
    if not cfg["ITM_task"]:
        assert rec["dpooled"] is None, "ITM off: the pooler gets dpooled = None"
        assert {"MVLBert.pooler.dense.weight", "MVLBert.pooler.dense.bias", "ITM_mlp.weight"} <= raw["none_grads"]
        assert "itm" not in rec and torch.equal(out, rec["mlm"]["loss"])
    if not cfg["MLM_task"]:
        assert "mlm" not in rec and raw["enc_bwd"][0]["dhidden"] is None
        assert all(n in raw["none_grads"] for n in head_grad_names("MLM_head_seq2seq").values())
    if opt.get("sync"):
        base = pretrain_run(name.replace("sync", "default"), native)["rec"]
        assert float(rec["mlm"]["acc"][1]) == SYNC * 19
        for k in ("logits", "lse", "dl", "dx", "weight", "bias"):      # (the loss sums are added by float atomics: see their bounds)
            a_, b_ = rec["itm"][k], base["itm"][k]
            if k in ("logits", "dl"):                              # (ld = 4: the two pad columns are never written)
                a_, b_ = a_[:, :2], b_[:, :2]
            Mi.check_equal(a_, b_, f"label_sync leaves the ITM branch alone: {k}")
        n = rec["mlm"]["rd"]                                  # (the nll sum itself is added by float atomics: held to its bound, not bit for bit)
        Mi.check_equal(rec["mlm"]["logits"][:n, :V], base["mlm"]["logits"][:n, :V], "label_sync rescales the count, not the forward")
        Mi.check_equal(rec["mlm"]["lse"][:n], base["mlm"]["lse"][:n], "label_sync rescales the count, not the forward")


@pytest.mark.parametrize("name", [n for n in RUNS])
def test_host_paths_agree_bit_for_bit(name):
    """The two host paths launch the same kernels on the same operands: everything recorded is bit-equal over the rows that exist,
    except what float atomics add up in arbitrary order: word_embeddings.weight and the cross-entropy loss sums (acc[0], hence
    the losses and the total), held to 1e-6 of their size as test_encoder_is_the_same_on_both_host_paths holds the table; each of
    them is inside its own float64 bound in both runs."""
    def close(x, y, what):
        x, y = x.double().reshape(-1), y.double().reshape(-1)
        assert bool((torch.isnan(x) == torch.isnan(y)).all()), what
        x, y = torch.nan_to_num(x), torch.nan_to_num(y)
        assert float((x - y).norm()) <= 1e-6 * float(x.norm()), (what, x, y)

    a, b = pretrain_run(name, True), pretrain_run(name, False)
    ra, rb = a["rec"], b["rec"]
    rows = B * (N_IMG + 2 + RUNS[name][2]) if ra["seq_len"] is None else sum(ra["seq_len"])
    for k in ("hidden", "x0", "dx_last", "dx0", "dhidden"):
        if k in ra:
            Mi.check_equal(ra[k][:rows], rb[k][:rows], f"{name}: native against python: {k}")
    if ra.get("total") is not None:
        close(ra["total"], rb["total"], "total")
    for k in ("cls", "pooled", "dpooled", "dimg", "g_pos", "g_typ", "g_wp", "g_bp"):
        if ra.get(k) is not None:
            Mi.check_equal(ra[k], rb[k], f"{name}: native against python: {k}")
    for part in ("mlm", "itm"):
        if part in ra:
            n = ra[part].get("rd")
            for k, v in ra[part].items():
                if torch.is_tensor(v) and v.is_floating_point() and k not in ("wt", "bt", "gamma", "beta", "wd", "bd", "w", "b"):
                    rowwise = v.dim() >= 1 and v.shape[0] == ra[part]["x"].shape[0] and k != "x"
                    lim = n if (rowwise and n is not None and k != "dx") else None
                    w = rb[part][k]
                    if k in ("acc", "nll", "loss"):
                        close(v, w, f"{part} {k}")
                        continue
                    if k in ("logits", "dl"):                      # (the pad columns are never written)
                        v, w = v[:, :V if part == "mlm" else 2], w[:, :V if part == "mlm" else 2]
                    Mi.check_equal(v[:lim] if v.dim() else v.reshape(1), w[:lim] if v.dim() else w.reshape(1),
                                   f"{name}: native against python: {part} {k}")
    ga, gb = a["raw"]["grads"], b["raw"]["grads"]
    assert ga.keys() == gb.keys()
    for k in ga:
        if k == "MVLBert.word_embeddings.weight":
            assert float((ga[k].double() - gb[k].double()).norm()) <= 1e-6 * float(ga[k].double().norm()), k
        else:
            Mi.check_equal(ga[k], gb[k], f"{name}: native against python: {k}")


@pytest.mark.parametrize("width", ["bf16-768", "f32-128"])
def test_both_loss_routes_describe_the_same_numbers(width):
    """The fused route and the plain one of the same flip and seed read the same t2, bit for bit: the float64 logits, lse and loss
    their bounds stand around are the same numbers, and each route is inside its own bounds of them (lse, nll, loss, dl and every
    gradient: test_pretraining_joints_against_float64)."""
    tag = width.split("-")[0]
    for native in (True, False):
        a, b = pretrain_run("default-" + tag, native), pretrain_run("fused-" + tag, native)
        assert not a["bad"] and not b["bad"]
        ma, mb = a["rec"]["mlm"], b["rec"]["mlm"]
        n = ma["rd"]
        assert n == mb["rd"] == 19 and float(ma["acc"][1]) == float(mb["acc"][1]) == 19
        for k in ("x", "labels"):
            Mi.check_equal(ma[k], mb[k], f"both routes read the same {k}")
        Mi.check_equal(ma["t2"][:n], mb["t2"][:n], "both routes read the same t2")
        Mi.check_equal(a["rec"]["itm"]["logits"][:, :2], b["rec"]["itm"]["logits"][:, :2], "the ITM branch does not depend on the route")


# ------------------------------------------------------------------ the encoder alone: a gradient on every row of hidden
@pytest.mark.parametrize("native", [True, False], ids=["native", "python"])
@pytest.mark.parametrize("entry", ["dense", "autopack"])
@pytest.mark.parametrize("width", ["bf16-768", "f32-128"])
def test_pooler_dgrad_is_added_to_live_cls_rows(width, entry, native):
    Hd, I, dt = WIDTHS[width]
    m = model_of("pretrain", width)
    T = 23 if entry == "dense" else 80
    ids, labels, _, lens = J.make_batch(T)
    g = torch.Generator().manual_seed(950 + T)
    m.conv.feat = torch.randn(B, N_IMG, Hd, generator=g).to(dt).cuda()
    ids_d = ids.cuda()
    enc = m.MVLBert
    w = torch.randn(B * (N_IMG + 2 + T), Hd, generator=g).to(dt).cuda()
    wp = torch.randn(B, Hd, generator=g).to(dt).cuda()
    seq_len = row_start = None
    if entry == "autopack":
        row_start, seq_len, total, _ = J.pack_plan_host(ids, None, N_IMG)

    def call(model):
        feat = model.conv(None)
        if entry == "dense":
            out, pooled = enc(ids_d, None, feat, None, seq2seq_mask=False)
            hidden = out[0].reshape(-1, Hd)
        else:
            hidden, pooled, _ = enc.forward_autopack(ids_d, feat, seq2seq_mask=True)
            hidden = hidden[:total]
        return (hidden.float() * w[:hidden.shape[0]].float()).sum() + (pooled.float() * wp.float()).sum()

    raw = recorded(m, native, call, lambda out: out, dout=None)
    rec = record_of(raw, m, ids, labels, layout="auto" if seq_len else "dense", lab_first=False, fused=False, T=T, seq_len=seq_len,
                    row_start=row_start)
    label = "encoder-%s-%s-%s" % (width, entry, "native" if native else "python")
    crow = J.cls_rows(B, N_IMG + 2 + T, row_start).cuda()
    assert bool((rec["dhidden"][crow] != 0).any(1).all()), "the [CLS] rows of dhidden are live in this run"
    bad, ratios = J.judge_pretrain(rec, label)
    lbad, lratios = layer_judgement(raw, m, ids, s2s=entry == "autopack", T=T, seq_len=seq_len)
    bad.update(lbad)
    ratios.update(lratios)
    note(label, dt, ratios)
    assert not bad, "\n".join(bad.values())


# ------------------------------------------------------------------ caption rows
@pytest.mark.parametrize("native", [True, False], ids=["native", "python"])
@pytest.mark.parametrize("strategy", ["unilm", "normal"])
@pytest.mark.parametrize("width", ["bf16-768", "f32-128"])
def test_caption_loss_rows(width, strategy, native):
    Hd, I, dt = WIDTHS[width]
    m = model_of("caption", width)
    T = 23
    ids, labels, _, lens = J.make_batch(T)
    g = torch.Generator().manual_seed(960)
    m.conv.feat = torch.randn(B, N_IMG, Hd, generator=g).to(dt).cuda()
    ids_d, labels_d = ids.cuda(), labels.cuda()
    dummy = torch.zeros(B, 3, 8, 8).cuda()
    raw = recorded(m, native, lambda model: model(dummy, ids_d, 0, strategy, labels=labels_d), lambda out: out)
    first = N_IMG + (2 if strategy == "unilm" else 1)
    rec = record_of(raw, m, ids, labels, layout="dense", lab_first=True, fused=True, T=T, first=first, head_name="MLM_head_seq2seq")
    Mi.check_equal(J.caption_text_row(B, T, N_IMG, strategy)[:2], torch.tensor([first, first + 1]), "the row table starts at `first`")
    label = "caption-%s-%s-%s" % (width, strategy, "native" if native else "python")
    bad, ratios = J.judge_pretrain(rec, label)
    lbad, lratios = layer_judgement(raw, m, ids, s2s=True, T=T, seq_len=None)
    bad.update(lbad)
    ratios.update(lratios)
    note(label, dt, ratios)
    assert not bad, "\n".join(bad.values())
    assert rec["dpooled"] is None and "MVLBert.pooler.dense.weight" in raw["none_grads"]


@pytest.mark.parametrize("strategy", ["unilm", "normal"])
def test_caption_logprobs_slots(strategy):
    """caption_logprobs scatters the packed scores back by slot = the number of scored positions before a position.  The same
    launches (label plan, gather, transform, fused head; deterministic) on the HOST statement of the row table give the packed
    scores; the host statement of the slots puts them into caption order: bit-equal, 0 where the caption holds 0.  (What the
    fused head computes is held to float64 by tests/test_head_ce_gpu.py and by the caption loss runs above.)"""
    from mvlt_amd import ops
    Hd, I, dt = WIDTHS["f32-128"]
    m = model_of("caption", "f32-128")
    T = 23
    ids, _, _, lens = J.make_batch(T)
    m.conv.feat = torch.randn(B, N_IMG, Hd, generator=torch.Generator().manual_seed(961)).to(dt).cuda()
    dummy = torch.zeros(B, 3, 8, 8).cuda()
    m.eval()
    try:
        raw = recorded(m, True, lambda model: model.caption_logprobs(dummy, ids.cuda(), strategy))
    finally:
        m.train()
    out = raw["out"]
    assert out.shape == (B, T) and out.dtype == torch.float32
    hidden = raw["enc_fwd"][0]["out"][0].reshape(-1, Hd)
    flat = torch.where(ids > 0, ids, torch.full_like(ids, J.IGNORE)).reshape(-1)
    text_row = J.caption_text_row(B, T, N_IMG, strategy)
    grow, sel, n = J.label_plan_host(flat, text_row)
    assert n == sum(lens)
    gather_row, sel_d, rd = ops.label_plan(flat.cuda(), text_row.cuda())
    Mi.check_equal(gather_row.cpu(), grow, "gather_row of the host row table")
    Mi.check_equal(sel_d.cpu(), sel, "sel_labels")
    head, ar = m.MLM_head_seq2seq, raw["ar"]
    dec = head.predictions.decoder
    x = ops.rows_transform(hidden.contiguous(), rowmap=gather_row)
    _, _, t2, _, _ = head._transform(ar, x, False, rd)
    _, lse, x_label, _ = ops.mlm_head_ce(t2, ar.compute(dec.weight), dec.bias.data, sel_d, V, rows_dev=rd, want_logits=False)
    torch.cuda.synchronize()
    want = torch.zeros(B * T, dtype=torch.float32, device=out.device)
    want[(flat >= 0).cuda()] = (x_label - lse)[:n]                  # slot i is the i-th scored position, in caption order
    Mi.check_equal(out.reshape(-1), want, f"caption_logprobs '{strategy}': scores in caption order")
    assert bool(torch.isfinite(out).all()) and bool((out.reshape(-1)[(flat >= 0).cuda()] < 0).all())


# ------------------------------------------------------------------ the fine-tuning heads
@pytest.mark.parametrize("native", [True, False], ids=["native", "python"])
@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("width", ["bf16-768", "f32-128"])
def test_vqa_head(width, train, native):
    Hd, I, dt = WIDTHS[width]
    m = model_of("vqa", width)
    T = 23
    ids, _, _, _ = J.make_batch(T)
    m.conv.feat = torch.randn(B, N_IMG, Hd, generator=torch.Generator().manual_seed(970)).to(dt).cuda()
    dummy = torch.zeros(B, 3, 8, 8).cuda()
    Vr = m.config.result_num
    dout = torch.randn(B, Vr, generator=torch.Generator().manual_seed(971)).cuda()
    m.train(train)
    try:
        raw = recorded(m, native, lambda model: model(dummy, ids.cuda(), None), (lambda out: out[1]) if train else None, dout=dout)
    finally:
        m.train()
    prob, logits = raw["out"]
    e = raw["fn"]["_LinearFn"][0]
    _, x, lin, p, _ = e["args"]
    assert p == (m.final_mlp[0].p if train else 0.0) and (p > 0) == train
    ar = raw["ar"]
    r = dict(x=x.detach(), w=ar.compute(lin.weight), b=lin.bias.data, logits=logits.detach())
    seed = 0
    if train:
        sar, Vn, xd, sp, seed = e["saved"]
        r.update(xd=xd, dlogits=e["grads"][0], dx=e["bwd_out"][1], weight=raw["grads"]["final_mlp.1.weight"],
                 bias=raw["grads"]["final_mlp.1.bias"])
        Mi.check_equal(raw["enc_bwd"][0]["dpooled"], e["bwd_out"][1], "dpooled is the head's dx")
        assert raw["enc_bwd"][0]["dhidden"] is None
    else:
        r["xd"] = x.detach()
    ref = J.linear(detached(r), dt, p=p, seed=seed)
    label = "vqa-%s-%s-%s" % (width, "train" if train else "eval", "native" if native else "python")
    note(label, dt, {"vqa " + k: v for k, v in J.worst_ratios(ref).items()})
    bad = J.failures(ref, label)
    assert not bad, "\n".join(bad.values())
    Mi.check_equal(x.detach(), raw["enc_fwd"][0]["out"][1].detach(), "the head reads pooled")
    # prob = softmax of the f32 logits: every row sums to 1 within an f32 sum of V terms (C_ACC sqrt(V) 2^-24) and the two
    # roundings of a term (the exponential's is relative to the term, the division's too)
    s = prob.double().sum(1)
    assert float((s - 1.0).abs().max()) <= (G.C_ACC * Vr ** 0.5 + 2.0) * G.U32
    want = torch.softmax(logits.detach().double(), 1)
    # each probability: the exponential is good to (2 |t| + 3) 2^-24 relative (misc_ref's cross-entropy analysis) with |t| at most
    # twice the largest |logit|, in the term and again in the sum, an f32 sum of V terms, one division
    xmax = float(logits.detach().abs().max())
    assert float((prob.double() - want).abs().max()) <= (2.0 * (4.0 * xmax + 3.0) + G.C_ACC * Vr ** 0.5 + 1.0) * G.U32


@pytest.mark.parametrize("native", [True, False], ids=["native", "python"])
@pytest.mark.parametrize("with_labels", [True, False], ids=["labels", "prob"])
@pytest.mark.parametrize("width", ["bf16-768", "f32-128"])
def test_retrieval_head(width, with_labels, native):
    Hd, I, dt = WIDTHS[width]
    m = model_of("retrieval", width)
    T = 23
    ids, _, itm, _ = J.make_batch(T)
    m.conv.feat = torch.randn(B, N_IMG, Hd, generator=torch.Generator().manual_seed(980)).to(dt).cuda()
    dummy = torch.zeros(B, 3, 8, 8).cuda()
    dout = torch.randn(B, 2, generator=torch.Generator().manual_seed(981)).cuda()
    raw = recorded(m, native, lambda model: model(dummy, ids.cuda(), itm.cuda() if with_labels else None),
                   (lambda out: out) if with_labels else None, dout=dout)
    e = raw["fn"]["_TransformLinearFn"][0]
    _, x, tr, lin, _ = e["args"]
    sar, Vn, sx, pre, t1, t2, mean, rstd = e["saved"]
    r = dict(x=sx, wt=sar.compute(tr.dense.weight), bt=tr.dense.bias.data, gamma=tr.LayerNorm.weight.data, beta=tr.LayerNorm.bias.data,
             w=sar.compute(lin.weight), b=lin.bias.data, pre=pre, t1=t1, t2=t2, mean=mean, rstd=rstd, logits=e["out"].detach())
    if with_labels:
        g = raw["grads"]
        r.update(dlogits=e["grads"][0], dx=e["bwd_out"][1], weight=g["final_mlp.1.weight"], bias=g["final_mlp.1.bias"],
                 **{"ln.weight": g["final_mlp.0.LayerNorm.weight"], "ln.bias": g["final_mlp.0.LayerNorm.bias"],
                    "transform.weight": g["final_mlp.0.dense.weight"], "transform.bias": g["final_mlp.0.dense.bias"]},
                 **raw["replay"]["_TransformLinearFn"])
        Mi.check_equal(raw["enc_bwd"][0]["dpooled"], e["bwd_out"][1], "dpooled is the head's dx")
    else:
        s = raw["out"].double().sum(1)
        assert raw["out"].shape == (B, 2) and float((s - 1.0).abs().max()) <= (G.C_ACC * 2 ** 0.5 + 2.0) * G.U32
    ref = J.transform_linear(detached(r), dt, eps=1e-12)
    label = "retrieval-%s-%s-%s" % (width, "labels" if with_labels else "prob", "native" if native else "python")
    note(label, dt, {"retrieval " + k: v for k, v in J.worst_ratios(ref).items()})
    bad = J.failures(ref, label)
    assert not bad, "\n".join(bad.values())
    Mi.check_equal(x.detach().contiguous(), raw["enc_fwd"][0]["out"][1].detach(), "the head reads pooled")


# ------------------------------------------------------------------ pair batch + feature_proj through the real Conv_layer
@pytest.mark.parametrize("dt", [BF, F32], ids=["bf16", "f32"])
def test_pair_batch_and_feature_proj(dt, monkeypatch):
    import mvlt_amd as M
    from mvlt_amd.arena import Arena
    cfg = M.MVLBertPretrainConfig(hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=512, vocab_size=V)
    cfg.swin.update(embed_dim=96, depths=[2, 2], num_heads=[3, 6])                             # num_features 192, never run
    cfg.swin_feature_proj = True
    torch.manual_seed(73)
    cl = M.Conv_layer(cfg)
    assert cl.feature_proj is not None and cl.feature_proj.in_features == 192
    stub = Stub()
    cl.conv[0] = stub
    g = torch.Generator().manual_seed(990)
    cl.feature_proj.weight.data.copy_(torch.randn(128, 192, generator=g) * 192 ** -0.5)
    cl.feature_proj.bias.data.copy_(0.1 * torch.randn(128, generator=g))
    cl = M.set_compute_dtype(cl.cuda().train(), dt)
    ar = Arena.of(cl, dt)                                # one arena for the whole module, as the models' forward makes it
    n = 2
    v = torch.randn(B, n, 3, 8, 8, generator=g).cuda()
    stub.feat = torch.randn(n * B, N_IMG, 192, generator=g).to(dt).cuda()
    store = {}
    for c in fn_classes():
        tap_function(monkeypatch, c, store)
    poison([(n * B * N_IMG, 192), (n * B * N_IMG, 128)], dt, torch.device("cuda"))
    out = cl(v)
    dout = torch.randn(out.shape, generator=g).to(dt).cuda()
    out.backward(dout)
    torch.cuda.synchronize()
    Mi.check_equal(stub.seen, J.pair_flatten(v), "the tower sees the pair batch in (n, B) order")
    e = store["_FeatureProjFn"][0]
    assert e["saved"][0] is ar
    lin = cl.feature_proj
    y = e["out"].detach()
    Mi.check_equal(e["args"][1].detach(), stub.out.detach().reshape(n * B * N_IMG, 192), "feature_proj reads the tower's rows in its order")
    Mi.check_equal(out.detach(), J.pair_unflatten(y.view(n * B, N_IMG, 128), B, n), "the views of a sample side by side")
    dy = dout.view(B, n, N_IMG, 128).transpose(0, 1).reshape(n * B * N_IMG, 128)          # the same statement, backwards
    Mi.check_equal(e["grads"][0].reshape(-1, 128), dy, "dy reaches feature_proj in (n, B) order")
    r = dict(x=e["args"][1].detach(), w=ar.compute(lin.weight), b=lin.bias.data, y=y, dy=e["grads"][0].reshape(-1, 128), dx=e["bwd_out"][1],
             weight=ar.grad_view(lin.weight).view(lin.weight.shape), bias=ar.grad_view(lin.bias))
    ref = J.feature_proj(detached(r), dt)
    note("pair-%s" % str(dt)[6:], dt, {"feature_proj " + k: v for k, v in J.worst_ratios(ref).items()})
    bad = J.failures(ref, "feature_proj")
    assert not bad, "\n".join(bad.values())
    Mi.check_equal(stub.out.grad.reshape(-1, 192), e["bwd_out"][1], "the tower's output gradient is feature_proj's dx, (n, B) order")


def test_worst_ratios_summary():
    """Prints the worst ratio per quantity and dtype over every run judged so far (the figures of the module docstring)."""
    for (dt, joint, k), v in sorted(_worst.items()):
        print(f"summary {dt:5s} {joint:14s} {k:18s} {v:.3f}")
        assert v <= 1.0
