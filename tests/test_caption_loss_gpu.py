"""Report-generation fine-tuning through the caption model's public interface: MVLBertForImageCaption.forward(..., labels=) --
the loss of run_report_generation_cxr.py:469-471 computed on the labelled rows with the fused head (mvlt_mlm_head_ce) -- and
caption_logprobs, against the oracle and against the logits route of the same model."""
import math
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import hash_sd, rel_err, synth_batch  # noqa: E402
from test_model_gpu import (ACT, GRAD, HASH_ACT, HASH_GRAD, HASH_LOSS, LOSS, _grad_check, _tiny_caption,  # noqa: E402
                            _tiny_oracle_cfgs, tiny_cfg)

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
B, T = 3, 12
KEYS = ["MLM_head_seq2seq.predictions.decoder.weight", "MLM_head_seq2seq.predictions.decoder.bias",
        "MLM_head_seq2seq.predictions.transform.dense.weight", "MLM_head_seq2seq.predictions.transform.LayerNorm.weight",
        "MVLBert.encoder.layer.1.intermediate.dense.weight", "MVLBert.encoder.layer.0.attention.self.value.weight",
        "MVLBert.position_embeddings.weight", "conv.conv.0.layers.3.blocks.0.attn.qkv.weight",
        "conv.conv.0.layers.1.downsample.reduction.weight", "conv.conv.0.norm.weight"]


@pytest.fixture(scope="module")
def M():
    import mvlt_amd
    return mvlt_amd


def _model(M, specs, specs_hash, cd):
    """(model, state dict, (loss, gradient, activation) tolerances) as tests/test_model_gpu.py pairs them: f32 on the sin()-formula
    weights, bf16 on the full-rank integer-hash weights -- the formula fixture's rank-2 matrices amplify bf16 rounding in the
    gradients and are an f32 pin only (the comment above TINY_GRAD there), so bf16 gradients are held to HASH_GRAD."""
    if cd == F32:
        model, sd = _tiny_caption(M, specs, cd)
        return model, sd, (LOSS[cd], GRAD[cd], ACT[cd])
    cfg = tiny_cfg(M, cls=M.MVLBertConfigForImageCaption)
    cfg.max_length = 10
    tok = type("Tok", (), {"mask_token_id": 103, "sep_token_id": 102})()
    model = M.MVLBertForImageCaption(cfg, tokenizer=tok)
    _, unexpected = model.load_state_dict(hash_sd(specs_hash["hash_tiny_caption"]), strict=False)
    assert not unexpected
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    return M.set_compute_dtype(model.cuda().eval(), cd), sd, (HASH_LOSS[cd], HASH_GRAD[cd], HASH_ACT[cd])


def _inputs():
    image, ids, _, _ = synth_batch(B, T, seed=61, vocab=3000)
    ids = ids.clone()
    ids[:, -1] = torch.tensor([5, 7, 9])          # every caption runs to t = T - 1, so a label can sit there
    pair = torch.stack([image, image.flip(0)], 1)                 # [B, 2, 3, 224, 224]
    return pair, ids


def _targets(ids, kind):
    if kind == "dense":
        return torch.where(ids > 0, ids, torch.full_like(ids, -100))
    t = torch.full_like(ids, -100)
    t[0, 2] = ids[0, 2]                               # one label
    t[1, 0], t[1, 5], t[1, T - 1] = ids[1, 0], ids[1, 5], ids[1, T - 1]          # three, the first and the last position among them
    return t                                          # (sample 2: none)


def _oracle_logits(sd, strategy):
    """[B, V, T] float32 oracle logits with their graph (fresh leaves per call: gradients are compared per test)."""
    O, scfg, bcfg = _tiny_oracle_cfgs()
    pair, ids = _inputs()
    osd = {k: (v.clone().requires_grad_(True) if v.dtype.is_floating_point else v) for k, v in sd.items()}
    feat = O.conv_layer(pair, osd, scfg)
    hidden = O.mvlbert_forward(osd, bcfg, ids, feat, True)["hidden"]
    n_img = feat.shape[1]
    text, sep = hidden[:, n_img + 2:], hidden[:, n_img + 1]
    src = text if strategy == "unilm" else torch.cat([sep[:, None], text[:, :-1]], 1)
    return O.mlm_head(src, osd, "MLM_head_seq2seq", bcfg).transpose(1, 2), osd


@pytest.mark.parametrize("cd", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("kind", ["sparse", "dense"])
@pytest.mark.parametrize("strategy", ["unilm", "normal"])
def test_caption_loss_and_gradients_vs_oracle(M, specs, specs_hash, strategy, kind, cd):
    model, sd, (tol_loss, tol_grad, _) = _model(M, specs, specs_hash, cd)
    pair, ids = _inputs()
    target = _targets(ids, kind)
    loss = model(pair.cuda(), ids.cuda(), 0, strategy, labels=target.cuda())
    assert loss.dim() == 0 and loss.dtype == torch.float32
    loss.backward()
    ref_logits, osd = _oracle_logits(sd, strategy)
    ref = F.cross_entropy(ref_logits, target, ignore_index=-100)
    ref.backward()
    print(f"{strategy} {kind} {cd}: loss {loss.item():.7f} oracle {ref.item():.7f}")
    assert abs(loss.item() - ref.item()) < tol_loss * abs(ref.item()), (loss.item(), ref.item())
    _grad_check(model, osd, KEYS, tol=tol_grad)


@pytest.mark.parametrize("kind", ["sparse", "dense"])
@pytest.mark.parametrize("strategy", ["unilm", "normal"])
def test_caption_loss_agrees_with_the_logits_route(M, specs, strategy, kind):
    pair, ids = _inputs()
    target = _targets(ids, kind).cuda()
    model, _ = _tiny_caption(M, specs, F32)
    new = model(pair.cuda(), ids.cuda(), 0, strategy, labels=target)
    new.backward()
    other, _ = _tiny_caption(M, specs, F32)          # the same weights, fresh gradients
    old = F.cross_entropy(other(pair.cuda(), ids.cuda(), 0, strategy).float(), target, ignore_index=-100)
    old.backward()
    assert abs(new.item() - old.item()) < 1e-5 * abs(old.item()), (new.item(), old.item())
    g_new, g_old = dict(model.named_parameters()), dict(other.named_parameters())
    for k in KEYS:
        assert rel_err(g_new[k].grad.cpu(), g_old[k].grad.cpu()) < 1e-4, k
    # evaluation: the same value without a graph and without logits
    with torch.no_grad():
        val = model(pair.cuda(), ids.cuda(), 0, strategy, labels=target)
    assert not val.requires_grad and abs(val.item() - new.item()) <= 1e-6 * abs(new.item())


def test_caption_loss_edge_cases(M, specs):
    model, _ = _tiny_caption(M, specs, F32)
    pair, ids = _inputs()
    none = torch.full_like(ids, -100).cuda()
    loss = model(pair.cuda(), ids.cuda(), 0, "unilm", labels=none)
    torch.cuda.synchronize()
    assert math.isnan(loss.item())
    with pytest.raises(ValueError):
        model(pair.cuda(), ids.cuda(), 1, "unilm", labels=none)
    with pytest.raises(ValueError):
        model(pair.cuda(), ids.cuda(), 2, "unilm", labels=none)
    with pytest.raises(NotImplementedError):
        model(pair.cuda(), ids.cuda(), 0, "other", labels=none)
    # labels=None dispatches to encode_forward as before (that the VALUES are the parent's is the unchanged
    # test_caption_encode_forward_gradients_vs_oracle's to show, not this comparison of one build with itself)
    with torch.no_grad():
        for strategy in ("unilm", "normal"):
            a = model(pair.cuda(), ids.cuda(), 0, strategy, labels=None)
            b = model.encode_forward(model.conv(pair.cuda()), ids.cuda(), strategy)
            assert a.shape == (B, 3000, T) and torch.equal(a, b)


@pytest.mark.parametrize("cd", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("strategy", ["unilm", "normal"])
def test_caption_logprobs_vs_oracle(M, specs, specs_hash, strategy, cd):
    model, sd, (_, _, tol_act) = _model(M, specs, specs_hash, cd)
    pair, ids = _inputs()
    ids[2, 7:] = 0                                    # a padded tail
    ids[0, 4] = 0                                     # and a pad in the middle
    lp = model.caption_logprobs(pair.cuda(), ids.cuda(), strategy)
    assert lp.shape == (B, T) and lp.dtype == torch.float32 and not lp.requires_grad
    O, scfg, bcfg = _tiny_oracle_cfgs()
    with torch.no_grad():
        feat = O.conv_layer(pair, sd, scfg)
        hidden = O.mvlbert_forward(sd, bcfg, ids, feat, True)["hidden"]
        n_img = feat.shape[1]
        text, sep = hidden[:, n_img + 2:], hidden[:, n_img + 1]
        src = text if strategy == "unilm" else torch.cat([sep[:, None], text[:, :-1]], 1)
        logp = torch.log_softmax(O.mlm_head(src, sd, "MLM_head_seq2seq", bcfg), -1)          # [B, T, V]
        ref = logp.gather(2, ids.clamp(min=0)[..., None])[..., 0]
    real = ids > 0
    got = lp.cpu()
    assert bool((got[~real] == 0).all())
    # log-probabilities are the logits shifted by their row's lse: held to the tolerance the logits themselves are held to
    err = rel_err(got[real], ref[real])
    print(f"{strategy} {cd}: log p relative error {err:.3g}")
    assert err < tol_act


def test_caption_loss_divides_by_the_synced_label_count(M, specs, monkeypatch):
    """Data parallel: the loss is this rank's nll sum over N_global / world (GradReducer.label_sync), in grad mode only."""
    model, _ = _tiny_caption(M, specs, F32)
    pair, ids = _inputs()
    target = _targets(ids, "sparse").cuda()          # 4 labels on this rank
    alone = model(pair.cuda(), ids.cuda(), 0, "unilm", labels=target)
    seen = []

    def fake_sync(count):
        seen.append(float(count))
        return (count + 8.0) / 2.0                    # the other rank holds 8 labels, world = 2

    monkeypatch.setitem(model.__dict__, "_mvlt_label_sync", fake_sync)
    synced = model(pair.cuda(), ids.cuda(), 0, "unilm", labels=target)
    assert seen == [4.0]
    assert abs(synced.item() - alone.item() * 4.0 / 6.0) < 1e-6 * abs(alone.item())
    synced.backward()
    with torch.no_grad():
        quiet = model(pair.cuda(), ids.cuda(), 0, "unilm", labels=target)
    assert seen == [4.0] and abs(quiet.item() - alone.item()) < 1e-6 * abs(alone.item())
