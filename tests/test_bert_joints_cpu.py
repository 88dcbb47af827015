"""tests/bert_joints_ref.py discriminates: a plain torch emulation of the joints of the BERT side (f32 arithmetic with the
products summed in another order than a @ b, stored tensors rounded to the compute dtype) sits inside every bound at the shapes
of tests/test_bert_joints_gpu.py -- B = 4, n_img = 49, T = 80 packed with caption lengths (80, 13, 0, 41), V = 3000 (ld = 3008),
H = 768 in bf16 and H = 128 in f32, both loss routes, labelled rows first and the all-rows head, dense and packed rows -- and each
of a named list of wiring faults is rejected by the cut reference with the tensor named.

The encoder itself is not emulated (tests/test_bert_layer_cpu.py does that): `hidden` and the dx layer 0 returns are random
stand-ins, the joints around them are computed from the definition.

For every fault test_fault_table also prints what the criteria the suite had for this code say of the same run, against the
fault-free run: the loss within 1e-4 (f32) / 1e-3 (bf16), every gradient within 5e-3 of its own norm (f32 model test), the whole
gradient within 3e-2 (bf16 model test) -- over the gradients of the joints themselves and the dx handed to the last layer (the
encoder's gradients follow that one; the encoder is not emulated).  Measured here (OLD_ACCEPTS holds the record true):
  f32   "dx rows at or beyond rd hold the stale product": the scatter stops at the count, so no gradient and no loss moves at
        all; what is wrong is an intermediate that the next change of the scatter would start to read
  bf16  that one, and three that a norm over the whole gradient cannot see because the decoder's gradient dominates it:
        "pooler dgrad at pack[3] shifted by one sample" (four rows of 338: 3.4e-4 of the whole gradient, 1.04 of its own
        tensor), "dloss applied to MLM only" (3.0e-3; the ITM head's own gradients are off by a third) and "label_sync count
        not handed to ce_bwd" (5.0e-3; every MLM gradient is off by the factor 2.5)
The other fifteen (f32) / twelve (bf16) of the sixteen in FAULTS are rejected by the old criteria too.  That list is the justification for this file: norms do not see a
fault in four rows, in a small head beside a large one, or in rows that are dropped later.
Two faults of the list live outside the pretraining step and have tests of their own below: the VQA backward that replays
dropout with another tag, and the pair batch flattened (B, n) instead of (n, B)."""
import math

import pytest
import torch

import bert_joints_ref as J
import head_ce_ref as HC
import ln_ref as R
import misc_ref as Mi
from bert_joints_ref import BF, F32
from test_bert_layer_cpu import gelu32, gelu_grad32, mm

N_IMG, B, V = 49, 4, 3000
LD = J.ceil_to(V, 64)
SEED, P_DROP, DLOSS, SYNC = 0x5EED77, 0.1, 0.75, 2.5
SHAPES = {BF: 768, F32: 128}
# fault -> (the variant it is injected into, the names under which judge_pretrain / the small judges must reject it)
FAULTS = {
    "pooler dgrad overwrites the [CLS] rows": ("encoder", ("pooler dx_cls",)),
    "pooler dgrad at pack[3] shifted by one sample": ("packed", ("pooler dx_cls",)),
    "cls from row b Lq + 1": ("dense", ("cls",)),
    "sel_labels in caption order": ("packed", ("sel_labels",)),
    "gather_row without text_row": ("packed", ("gather_row", "mlm x")),
    "dx rows at or beyond rd hold the stale product": ("packed", ("mlm dx beyond rd",)),
    "decoder.bias sums the ld pad columns": ("packed", ("mlm decoder.bias",)),
    "loss divided by rows": ("packed", ("count",)),
    "dloss applied to MLM only": ("packed", ("itm dloss", "itm dl")),
    "seq2seq head on a bidirectional flip": ("packed", ("mlm pre", "mlm t1")),
    "'normal' reads the rows of 'unilm'": ("caption-normal", ("mlm x",)),
    "label_sync count not handed to ce_bwd": ("sync", ("mlm dl",)),
    "position table without the sample's row offset": ("packed", ("embed position",)),
    "type-1 rows receive the image rows' sum": ("packed", ("embed token_type",)),
    "dhidden scatter ignores the count": ("packed", ("dhidden rows nobody gathered",)),
    "total drops the ITM loss": ("packed", ("total",)),
}
# measured: the faults the old whole-model criteria accept (test_fault_table prints the figures)
OLD_ACCEPTS = {
    F32: {"dx rows at or beyond rd hold the stale product"},
    BF: {"dx rows at or beyond rd hold the stale product", "pooler dgrad at pack[3] shifted by one sample",
         "dloss applied to MLM only", "label_sync count not handed to ce_bwd"},
}
GRADS = ("g_wp", "g_bp", "g_word", "g_pos", "g_typ", "dimg")
HEAD_GRADS = ("decoder.weight", "decoder.bias", "ln.weight", "ln.bias", "transform.weight", "transform.bias")


def params(Hd, dt):
    g = torch.Generator().manual_seed(11 + Hd)
    rn = lambda *s: torch.randn(*s, generator=g)                    # noqa: E731
    def head():
        return dict(wt=(rn(Hd, Hd) * Hd ** -0.5).to(dt), bt=0.1 * rn(Hd), gamma=1.0 + 0.1 * rn(Hd), beta=0.1 * rn(Hd),
                    wd=(rn(V, Hd) * Hd ** -0.5).to(dt), bd=0.1 * rn(V))
    return dict(wp=(rn(Hd, Hd) * Hd ** -0.5).to(dt), bp=0.1 * rn(Hd), bidir=head(), s2s=head(), wi=(rn(2, Hd) * Hd ** -0.5).to(dt),
                bi=0.1 * rn(2), word=0.5 * rn(V + 1, Hd), pos=0.5 * rn(512, Hd), typ=0.5 * rn(3, Hd))


def ce_emulate(logits, Vn, labels, n, count, dloss, dt):
    """f32 cross entropy over the first n rows of the stored logits -> (lse [rows], nll sum, dl written in place into a copy)."""
    x = logits[:n, :Vn].float()
    lab = labels[:n]
    on = lab >= 0
    mx = x.max(1, keepdim=True).values
    lse = (mx[:, 0] + torch.log(torch.exp(x - mx).sum(1))).float()
    nll = torch.where(on, lse - x.gather(1, lab.clamp(min=0)[:, None])[:, 0], torch.zeros_like(lse)).sum()
    sc = torch.tensor(1.0 * dloss, dtype=torch.float32) / max(float(count), 1.0)
    hot = torch.arange(Vn)[None, :] == lab[:, None]
    dl = torch.where(on[:, None], sc * (torch.exp(x - lse[:, None]) - hot.float()), torch.zeros_like(x))
    out = logits.clone()
    out[:n, :Vn] = dl.to(dt)
    full = torch.zeros(logits.shape[0])
    full[:n] = torch.where(on, lse, torch.zeros_like(lse))
    return full, nll.float(), out


def emulate(dt, fault=None, variant="packed", fused=False, lab_first=True):
    """-> the record bert_joints_ref.judge_pretrain reads.  variant: packed (autopack rows, T = 80) | dense (T = 23) | sync
    (packed with the label-count factor SYNC) | caption-normal (dense, no pooler / ITM, the 'normal' row table, fused route) |
    encoder (dense, no heads: random dhidden and dpooled, as a caller that reads every row of hidden hands them back -- the
    heads leave the [CLS] rows of dhidden zero, where adding and overwriting are the same)."""
    Hd = SHAPES[dt]
    caption = variant == "caption-normal"
    packed = variant in ("packed", "sync")
    T = 80 if packed else 23
    Lq = N_IMG + 2 + T
    P = params(Hd, dt)
    ids, labels, itm, lens = J.make_batch(T)
    J.check_label_requirements(ids, labels, list(lens))
    g = torch.Generator().manual_seed(21 + T + Hd)
    rn = lambda *s: torch.randn(*s, generator=g)                    # noqa: E731
    rd_ = lambda t: t.to(dt)                                        # noqa: E731
    image = rd_(rn(B, N_IMG, Hd))
    row_start = seq_len = None
    if packed:
        row_start, seq_len, total, text_row = J.pack_plan_host(ids, labels, N_IMG)
    else:
        total = B * Lq
        text_row = J.dense_text_row(B, T, N_IMG, N_IMG + 1 if caption else None)
    alloc = B * Lq
    hidden = rd_(rn(alloc, Hd))
    rec = dict(dt=dt, B=B, T=T, n_img=N_IMG, V=V, eps=1e-12, dloss=DLOSS, fused=fused or caption, lab_first=lab_first or caption,
               sync=SYNC if variant == "sync" else None, layout="auto" if packed else "dense", ids=ids, labels=labels, seq_len=seq_len, row_start=row_start,
               image=image, word=P["word"], pos=P["pos"], typ=P["typ"], hidden=hidden, first=N_IMG + 1 if caption else None)
    x0 = torch.zeros(alloc, Hd, dtype=dt)
    x0[:total] = J.embed_rows(ids, image, P["word"], P["pos"], P["typ"], dt, N_IMG, seq_len)
    rec["x0"] = x0
    crow = J.cls_rows(B, Lq, row_start)
    # ---- pooler and ITM head, forward
    if not caption:
        cls = hidden[crow + 1] if fault == "cls from row b Lq + 1" else hidden[crow]
        pooled = rd_(torch.tanh(rd_(mm(cls.float(), P["wp"].float().t()) + P["bp"]).float()))
        lg = torch.full((B, 4), 7.0, dtype=dt)
        lg[:, :2] = rd_(mm(pooled.float(), P["wi"].float().t()) + P["bi"])
        lse_i, nll_i, dl_i = ce_emulate(lg, 2, itm, B, B, 1.0 if fault == "dloss applied to MLM only" else DLOSS, dt)
        itm_loss = nll_i / B
        dpooled = rd_(mm(dl_i[:, :2].float(), P["wi"].float()))
        rec["itm"] = dict(x=pooled, w=P["wi"], b=P["bi"], labels=itm, logits=lg, lse=lse_i, acc=torch.tensor([float(nll_i), float(B)]),
                          loss=itm_loss, dl=dl_i, dx=dpooled, weight=mm(dl_i[:, :2].float().t().contiguous(), pooled.float()),
                          bias=dl_i[:, :2].float().sum(0), dloss_seen=1.0 if fault == "dloss applied to MLM only" else DLOSS)
        if variant == "encoder":
            del rec["itm"]
            dpooled = rd_(rn(B, Hd))
        rec.update(cls=cls, wp=P["wp"], bp=P["bp"], pooled=pooled, dpooled=dpooled)
    # ---- MLM head: the rows, the plan
    flat = labels.reshape(-1)
    count = int((flat >= 0).sum())
    if rec["lab_first"]:
        tr = None if fault == "gather_row without text_row" else text_row
        if fault == "'normal' reads the rows of 'unilm'":
            tr = J.dense_text_row(B, T, N_IMG)
        grow, sel, n = J.label_plan_host(flat, tr)
        if fault == "gather_row without text_row":
            grow = (grow.long() % alloc).to(torch.int32)
        if fault == "sel_labels in caption order":
            sel = flat.clone()
        src = grow.long()
    else:
        grow, sel, n, src = None, flat, flat.numel(), text_row
    x = hidden[src]
    hp, used = P["bidir"], P["s2s" if fault == "seq2seq head on a bidirectional flip" else "bidir"]
    N = x.shape[0]
    pre32 = mm(x[:n].float(), used["wt"].float().t()) + used["bt"]
    junk = lambda c, s_: rd_(torch.randn(N, c, generator=torch.Generator().manual_seed(s_)))          # noqa: E731
    pre, t1 = junk(Hd, 1), junk(Hd, 2)
    pre[:n], t1[:n] = rd_(pre32), rd_(gelu32(pre32))
    t1f = t1[:n].float()
    mean = t1f.mean(1)
    d = t1f - mean[:, None]
    rstd = torch.rsqrt((d * d).mean(1) + 1e-12)
    t2 = junk(Hd, 3)
    t2[:n] = rd_(d * rstd[:, None] * used["gamma"] + used["beta"])
    mean_f, rstd_f = torch.zeros(N), torch.ones(N)
    mean_f[:n], rstd_f[:n] = mean, rstd
    logits = torch.full((N, LD), 7.0, dtype=dt)
    logits[:n, :V] = rd_(mm(t2[:n].float(), used["wd"].float().t()) + used["bd"])
    factor = rec["sync"] or 1.0
    div = N if fault == "loss divided by rows" else factor * count
    bwd_count = count if fault == "label_sync count not handed to ce_bwd" else div
    if rec["fused"]:
        lse_n, _, nll, _ = HC.emulate_f32(t2, used["wd"], used["bd"], sel, rows=n)
        lse = torch.zeros(N)
        lse[:n] = torch.where(sel[:n] >= 0, lse_n, torch.zeros_like(lse_n))
        nll = torch.tensor(nll, dtype=torch.float32)
        _, _, dl = ce_emulate(logits, V, sel, n, bwd_count, DLOSS, dt)
    else:
        lse, nll, dl = ce_emulate(logits, V, sel, n, bwd_count, DLOSS, dt)
    loss = nll / torch.tensor(float(div), dtype=torch.float32)
    # ---- MLM head, backward
    dlv = dl[:n, :V].float()
    dt2 = rd_(mm(dlv, used["wd"].float(), chunk=500)).float()
    g_wd = mm(dlv.t().contiguous(), t2[:n].float())
    g_bd = dlv.sum(0)
    if fault == "decoder.bias sums the ld pad columns":
        g_bd = dl.reshape(-1)[:n * V].view(n, V).float().sum(0)
    xh = d * rstd[:, None]
    gg = dt2 * used["gamma"]
    dt1 = rd_(rstd[:, None] * (gg - gg.mean(1, keepdim=True) - xh * (gg * xh).mean(1, keepdim=True))).float()
    dpre = rd_(dt1 * gelu_grad32(pre[:n].float())).float()
    dx = torch.zeros(N, Hd, dtype=dt)
    if fault == "dx rows at or beyond rd hold the stale product":
        dx = junk(Hd, 4)
    dx[:n] = rd_(mm(dpre, used["wt"].float()))
    stages = {}
    for k, v in (("dt2", dt2), ("dt1", dt1), ("dpre", dpre)):          # the stored stages of a replay (the GPU test launches them)
        stages[k] = junk(Hd, 6)
        stages[k][:n] = rd_(v)
    rec["mlm"] = dict(hp, x=x, labels=sel, gather_row=grow, rd=n if grow is not None else None, pre=pre, t1=t1, t2=t2, mean=mean_f,
                      rstd=rstd_f, logits=logits, lse=lse, acc=torch.tensor([float(nll), float(div)]), nll=nll, loss=loss, dl=dl,
                      dx=dx, dloss_seen=DLOSS, **stages, **{"decoder.weight": g_wd, "decoder.bias": g_bd, "ln.weight": (dt2 * xh).sum(0),
                                                  "ln.bias": dt2.sum(0), "transform.weight": mm(dpre.t().contiguous(), x[:n].float()),
                                                  "transform.bias": dpre.sum(0)})
    # ---- the gather's backward, the pooler's
    dhidden = torch.zeros(alloc, Hd, dtype=dt)
    m = N if fault == "dhidden scatter ignores the count" else n
    if fault == "dhidden scatter ignores the count":
        dxs = dx.clone()
        dxs[n:] = junk(Hd, 5)[n:]
        dhidden[src[:m]] = dxs[:m]
    else:
        dhidden[src[:m]] = dx[:m]
    if variant == "encoder":
        del rec["mlm"]
        dhidden = rd_(rn(alloc, Hd))
    rec["dhidden"] = dhidden
    if not caption:
        dpre_p = rd_(dpooled.float() * (1.0 - pooled.float() ** 2))
        rec["g_wp"], rec["g_bp"] = mm(dpre_p.float().t().contiguous(), cls.float()), dpre_p.float().sum(0)
        add = mm(dpre_p.float(), P["wp"].float())
        dx_last = dhidden.clone()
        at = torch.roll(crow, 1) if fault == "pooler dgrad at pack[3] shifted by one sample" else crow
        if fault == "pooler dgrad overwrites the [CLS] rows":
            dx_last[at] = rd_(add)
        elif packed:
            dx_last[at] = rd_(dx_last[at].float() + rd_(add).float())
        else:
            dx_last[at] = rd_(dx_last[at].float() + add)
        rec["dx_last"] = dx_last
        if variant != "encoder":
            rec["total"] = loss if fault == "total drops the ITM loss" else loss + itm_loss
    # ---- embedding backward from a stand-in for what layer 0 returned
    dx0 = rd_(rn(alloc, Hd))
    dense, valid = J.to_dense(dx0[:total], B, Lq, seq_len)
    gf = dense.float() * valid[:, :, None].float()
    wid = Mi.embed_word_ids(ids, B, N_IMG, T, J.CLS_ID, J.SEP_ID)
    on = ((wid >= 0) & valid).reshape(-1)
    g_word = torch.zeros(V + 1, Hd).index_add_(0, wid.reshape(-1)[on], gf.reshape(-1, Hd)[on])
    g_pos = torch.zeros(512, Hd)
    if fault == "position table without the sample's row offset":
        for r in range(total):                                   # the packed row number taken as the position
            if r < 512:
                g_pos[r] += dx0[r].float()
    else:
        g_pos[:Lq] = gf.sum(0)
    g_typ = torch.zeros(3, Hd)
    ty = Mi.embed_types(Lq, N_IMG, -1)
    g_typ[0], g_typ[1] = gf[:, ty == 0].sum((0, 1)), gf[:, ty == 1].sum((0, 1))
    if fault == "type-1 rows receive the image rows' sum":
        g_typ[1] = gf[:, 1:1 + N_IMG].sum((0, 1))
    rec.update(dx0=dx0, dimg=dense[:, 1:1 + N_IMG].contiguous(), g_word=g_word, g_pos=g_pos, g_typ=g_typ)
    return rec


CLEAN = [(BF, "packed", False, True), (F32, "packed", False, True), (BF, "packed", True, True), (F32, "packed", True, True),
         (F32, "packed", False, False), (BF, "dense", False, False), (F32, "dense", False, False), (BF, "sync", False, True),
         (F32, "sync", True, True), (BF, "caption-normal", True, True), (F32, "caption-normal", True, True),
         (BF, "encoder", False, True), (F32, "encoder", False, True)]


@pytest.mark.parametrize("dt,variant,fused,lab_first", CLEAN,
                         ids=["%s-%s-%s-%s" % (str(c[0])[6:], c[1], "fused" if c[2] else "ce", "labfirst" if c[3] else "allrows") for c in CLEAN])
def test_emulation_sits_inside_every_bound(dt, variant, fused, lab_first):
    rec = emulate(dt, None, variant, fused, lab_first)
    bad, ratios = J.judge_pretrain(rec, "emulation")
    for k, v in sorted(ratios.items()):
        print(f"emulation {str(dt)[6:]:8s} {variant:14s} {k:28s} worst ratio to the bound {v:.3f}")
    assert not bad, "\n".join(bad.values())
    assert max(ratios.values()) <= 1.0


def test_chained_bounds_and_their_signal():
    """Without the stored dl the head's backward is judged chained from the logits: the emulation stays inside, and the measured
    signal / bound says what that judgement can still see (below ~1: nothing of the tensor's own size)."""
    for dt in (BF, F32):
        rec = emulate(dt, None, "packed")
        m = dict(rec["mlm"], dloss=DLOSS)
        cut = J.mlm_head(m, dt, V=V, n=m["rd"], fused=False, eps=1e-12)
        for k in ("dl", "dt2", "dt1", "dpre"):
            del m[k]
        chained = J.mlm_head(m, dt, V=V, n=m["rd"], fused=False, eps=1e-12)
        assert not J.failures(chained) and not J.failures(cut)
        sc, sk = J.signal_to_bound(chained), J.signal_to_bound(cut)
        for k in ("dx",) + HEAD_GRADS:
            print(f"{str(dt)[6:]:8s} {k:18s} signal / bound chained {sc[k]:10.3g}   cut {sk[k]:10.3g}")
            assert sk[k] >= sc[k] * 0.999
        assert sk["decoder.weight"] > 50 and sk["dx"] > 50, "the cut judgement sees a fault of 2 % of the tensor everywhere"


# ------------------------------------------------------------------ the small heads
def small_head_runs(dt, fault=None):
    Hd = SHAPES[dt]
    g = torch.Generator().manual_seed(31 + Hd)
    rn = lambda *s: torch.randn(*s, generator=g)                    # noqa: E731
    rd_ = lambda t: t.to(dt)                                        # noqa: E731
    x = rd_(rn(B, Hd))
    # VQA: dropout -> Linear(H, 224), f32 logits
    w, b = rd_(rn(224, Hd) * Hd ** -0.5), 0.1 * rn(224)
    keep = R.dropout_keep(SEED, J.DROP_TAG, P_DROP, B, Hd).float() / (1.0 - P_DROP)
    keep_b = R.dropout_keep(SEED, J.DROP_TAG + (1 if fault == "VQA backward replays dropout with another tag" else 0), P_DROP, B,
                            Hd).float() / (1.0 - P_DROP)
    xd = rd_(x.float() * keep)
    logits = rd_(mm(xd.float(), w.float().t()) + b).float()
    dlogits = rn(B, 224)
    dl = rd_(dlogits).float()
    vqa = dict(x=x, xd=xd, w=w, b=b, logits=logits, dlogits=dlogits, dx=rd_(mm(dl, w.float(), chunk=50) * keep_b),
               weight=mm(dl.t().contiguous(), xd.float()), bias=dl.sum(0))
    # retrieval: transform + Linear(H, 2)
    wt, bt, gamma, beta = rd_(rn(Hd, Hd) * Hd ** -0.5), 0.1 * rn(Hd), 1.0 + 0.1 * rn(Hd), 0.1 * rn(Hd)
    w2, b2 = rd_(rn(2, Hd) * Hd ** -0.5), 0.1 * rn(2)
    pre32 = mm(x.float(), wt.float().t()) + bt
    pre, t1 = rd_(pre32), rd_(gelu32(pre32))
    mean = t1.float().mean(1)
    d = t1.float() - mean[:, None]
    rstd = torch.rsqrt((d * d).mean(1) + 1e-12)
    xh = d * rstd[:, None]
    t2 = rd_(xh * gamma + beta)
    lg2 = rd_(mm(t2.float(), w2.float().t()) + b2).float()
    dlg2 = rn(B, 2)
    dl2 = rd_(dlg2).float()
    dt2 = rd_(dl2 @ w2.float()).float()
    gg = dt2 * gamma
    dt1 = rd_(rstd[:, None] * (gg - gg.mean(1, keepdim=True) - xh * (gg * xh).mean(1, keepdim=True))).float()
    dpre = rd_(dt1 * gelu_grad32(pre.float())).float()
    ret = dict(x=x, wt=wt, bt=bt, gamma=gamma, beta=beta, w=w2, b=b2, pre=pre, t1=t1, t2=t2, mean=mean, rstd=rstd, logits=lg2,
               dlogits=dlg2, dx=rd_(mm(dpre, wt.float())), weight=dl2.t() @ t2.float(), bias=dl2.sum(0),
               **{"ln.weight": (dt2 * xh).sum(0), "ln.bias": dt2.sum(0), "transform.weight": mm(dpre.t().contiguous(), x.float()),
                  "transform.bias": dpre.sum(0)})
    # feature projection 192 -> H on n B rows of 49 tokens
    xf = rd_(rn(2 * B * N_IMG, 192))
    wf, bf = rd_(rn(Hd, 192) * 192 ** -0.5), 0.1 * rn(Hd)
    dy = rd_(rn(2 * B * N_IMG, Hd))
    fp = dict(x=xf, w=wf, b=bf, y=rd_(mm(xf.float(), wf.float().t()) + bf), dy=dy, dx=rd_(mm(dy.float(), wf.float(), chunk=100)),
              weight=mm(dy.float().t().contiguous(), xf.float(), chunk=100), bias=dy.float().sum(0))
    return vqa, ret, fp


@pytest.mark.parametrize("dt", [BF, F32], ids=["bf16", "f32"])
def test_small_heads_sit_inside_every_bound(dt):
    vqa, ret, fp = small_head_runs(dt)
    for name, ref in (("vqa", J.linear(vqa, dt, p=P_DROP, seed=SEED)), ("retrieval", J.transform_linear(ret, dt, eps=1e-12)),
                      ("feature_proj", J.feature_proj(fp, dt))):
        for k, v in J.worst_ratios(ref).items():
            print(f"emulation {str(dt)[6:]:8s} {name:12s} {k:18s} worst ratio to the bound {v:.3f}")
        bad = J.failures(ref, name)
        assert not bad, bad


@pytest.mark.parametrize("dt", [BF, F32], ids=["bf16", "f32"])
def test_vqa_dropout_replayed_with_another_tag_is_rejected(dt):
    vqa, _, _ = small_head_runs(dt, "VQA backward replays dropout with another tag")
    with pytest.raises(AssertionError, match="dx where the forward dropped"):
        J.linear(vqa, dt, p=P_DROP, seed=SEED)
    print("VQA backward replays dropout with another tag: rejected at dx (the elements the forward dropped are not 0)")


def test_pair_batch_flattened_sample_major_is_rejected():
    v = torch.randn(B, 2, 3, 8, 8, generator=torch.Generator().manual_seed(5))
    Mi.check_equal(J.pair_flatten(v)[B], v[0, 1], "row B of the tower's batch is view 1 of sample 0")
    with pytest.raises(AssertionError):
        Mi.check_equal(v.reshape(2 * B, 3, 8, 8), J.pair_flatten(v), "the tower's batch")
    f = torch.randn(2 * B, N_IMG, 16, generator=torch.Generator().manual_seed(6))
    out = J.pair_unflatten(f, B, 2)
    Mi.check_equal(out[1, N_IMG:], f[B + 1], "sample 1's second view follows its first")
    print("pair batch flattened (B, n): rejected at the tower's input (row 1 holds view 1 of sample 0, not sample 1's view 0)")


# ------------------------------------------------------------------ named wiring faults
@pytest.fixture(scope="module")
def fault_runs():
    out = {}
    for dt in (BF, F32):
        for variant in ("packed", "dense", "sync", "caption-normal", "encoder"):
            for fault in [None] + [f for f, (v, _) in FAULTS.items() if v == variant]:
                rec = emulate(dt, fault, variant)
                out[fault, variant, dt] = (rec,) + J.judge_pretrain(rec, str(fault))
    return out


@pytest.mark.parametrize("fault", list(FAULTS))
def test_fault_is_rejected_by_name(fault_runs, fault):
    variant, must = FAULTS[fault]
    for dt in (F32, BF):
        _, bad, ratios = fault_runs[fault, variant, dt]
        _, clean_bad, _ = fault_runs[None, variant, dt]
        assert not clean_bad, clean_bad
        first = next(k for k in bad)
        print(f"{fault}, {str(dt)[6:]}: rejected at {first}" + (f" ({ratios[first]:.3g} of its bound)" if first in ratios else "")
              + f"; all: {', '.join(bad)}")
        for k in must:
            assert k in bad, (fault, str(dt), k, "was accepted", sorted(bad))
            assert fault in bad[k], bad[k]


def rel(a, b):
    a, b = a.double().reshape(-1), b.double().reshape(-1)
    return float((a - b).norm()), float(b.norm())


def old_criteria(rec, clean):
    """(loss error, worst per-tensor relative error, whole-gradient relative error) of a run against the fault-free one: what
    a whole-model comparison with an oracle measures."""
    pairs = [(rec[k], clean[k]) for k in GRADS + ("dx_last",) if k in rec]          # (dx_last: every gradient below it follows it)
    if "mlm" not in rec:
        nd = [rel(a, b) for a, b in pairs]
        return 0.0, max(n / d for n, d in nd if d > 0), math.sqrt(sum(n * n for n, _ in nd) / sum(d * d for _, d in nd))
    pairs += [(rec["mlm"][k], clean["mlm"][k]) for k in HEAD_GRADS]
    if "itm" in rec:
        pairs += [(rec["itm"][k], clean["itm"][k]) for k in ("weight", "bias")]
    nd = [rel(a, b) for a, b in pairs]
    per = max(n / d for n, d in nd if d > 0)
    whole = math.sqrt(sum(n * n for n, _ in nd) / sum(d * d for _, d in nd))
    lk = "total" if "total" in rec else None
    la, lb = (rec[lk], clean[lk]) if lk else (rec["mlm"]["loss"], clean["mlm"]["loss"])
    return abs(float(la) - float(lb)) / abs(float(lb)), per, whole


def test_fault_table(fault_runs):
    accepted = {F32: set(), BF: set()}
    for (fault, variant, dt), (rec, bad, _) in fault_runs.items():
        if fault is None:
            continue
        lerr, per, whole = old_criteria(rec, fault_runs[None, variant, dt][0])
        old = (lerr < 1e-4 and per < 5e-3) if dt == F32 else (lerr < 1e-3 and whole < 3e-2)
        print(f"{str(dt)[6:]:8s} {variant:14s} {fault:52s} rejected at {next(iter(bad))!s:30s} | loss {lerr:8.2e} worst tensor "
              f"{per:8.2e} whole gradient {whole:8.2e}: old criteria {'ACCEPT' if old else 'reject'}")
        assert bad, (fault, "accepted by the cut reference")
        if old:
            accepted[dt].add(fault)
    print("accepted by the old f32 criteria (loss 1e-4, 5e-3 per tensor):", sorted(accepted[F32]))
    print("accepted by the old bf16 criteria (loss 1e-3, 3e-2 whole gradient):", sorted(accepted[BF]))
    assert accepted == OLD_ACCEPTS, "the record of what the old criteria cannot see"
