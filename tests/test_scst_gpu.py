"""Self-critical fine-tuning through the public interface: MVLBertForImageCaption.sequence_loss against the oracle (loss and
gradients, both strategies, both weight layouts) and against the cross-entropy route, and scst.self_critical_loss against the
pieces it is made of (generate, report_metrics.score, sequence_loss)."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import seq_loss_ref as R  # noqa: E402
from conftest import rel_err, synth_batch  # noqa: E402
from test_caption_loss_gpu import KEYS, _inputs, _model  # noqa: E402
from test_model_gpu import _grad_check, _tiny_caption, _tiny_oracle_cfgs  # noqa: E402
from tiny_caption import tiny_caption  # noqa: E402

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
B, T = 3, 12
EOS = R.EOS


@pytest.fixture(scope="module")
def M():
    import mvlt_amd
    return mvlt_amd


def _sequences():
    """Row 0: an [END] in the middle with ids behind it (they must not count); row 1: neither [END] nor PAD; row 2: PAD-terminated."""
    g = torch.Generator().manual_seed(71)
    seq = torch.randint(1000, 3000, (B, T), generator=g)
    seq[0, 5] = EOS
    seq[2, 7:] = 0
    return seq


def _weights(layout):
    if layout == "b":
        return torch.tensor([1.5, 0.0, -0.25])               # mixed sign, one exact 0
    g = torch.Generator().manual_seed(72)
    w = 1.0 + 0.5 * torch.randn(B, T, generator=g)
    w[0, 2], w[1, 3], w[2, 0] = 0.0, -0.4, -1.1
    return w


def _oracle_logits(sd, strategy, pair, ids):
    """test_caption_loss_gpu._oracle_logits on the given teacher-forcing ids: [B, V, T] float32 with its graph."""
    O, scfg, bcfg = _tiny_oracle_cfgs()
    osd = {k: (v.clone().requires_grad_(True) if v.dtype.is_floating_point else v) for k, v in sd.items()}
    feat = O.conv_layer(pair, osd, scfg)
    hidden = O.mvlbert_forward(osd, bcfg, ids, feat, True)["hidden"]
    n_img = feat.shape[1]
    text, sep = hidden[:, n_img + 2:], hidden[:, n_img + 1]
    src = text if strategy == "unilm" else torch.cat([sep[:, None], text[:, :-1]], 1)
    return O.mlm_head(src, osd, "MLM_head_seq2seq", bcfg).transpose(1, 2), osd


def _reference_loss(logits, seq, w, eos):
    """The issue's definition in torch: log_softmax -> gather -> weights -> mask, over N = sum of the lengths."""
    lens = torch.tensor([R.seq_len(r, eos) for r in seq.tolist()])
    mask = (torch.arange(T)[None, :] < lens[:, None]).to(logits.dtype)
    logp = torch.log_softmax(logits, 1).gather(1, seq.clamp(min=0)[:, None, :])[:, 0]           # [B, T]
    wt = w if w.dim() == 2 else w[:, None]
    return -(wt * logp * mask).sum() / lens.sum(), lens


@pytest.mark.parametrize("cd", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("layout", ["b", "bt"])
@pytest.mark.parametrize("strategy", ["unilm", "normal"])
def test_sequence_loss_and_gradients_vs_oracle(M, specs, specs_hash, strategy, layout, cd):
    model, sd, (tol_loss, tol_grad, _) = _model(M, specs, specs_hash, cd)
    pair, _ = _inputs()
    seq, w = _sequences(), _weights(layout)
    loss = model.sequence_loss(pair.cuda(), seq.cuda(), w.cuda(), strategy, eos_token_id=EOS)
    assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.requires_grad
    loss.backward()
    lens = torch.tensor([R.seq_len(r, EOS) for r in seq.tolist()])
    assert lens.tolist() == [6, 12, 7]
    tf_ids = torch.where(torch.arange(T)[None, :] < lens[:, None], seq, torch.zeros_like(seq))
    ref_logits, osd = _oracle_logits(sd, strategy, pair, tf_ids)
    ref, _ = _reference_loss(ref_logits, seq, w, EOS)
    ref.backward()
    print(f"{strategy} {layout} {cd}: loss {loss.item():.7f} oracle {ref.item():.7f}")
    assert abs(loss.item() - ref.item()) < tol_loss * abs(ref.item()), (loss.item(), ref.item())
    _grad_check(model, osd, KEYS, tol=tol_grad)
    # evaluation: the same value without a graph
    with torch.no_grad():
        val = model.sequence_loss(pair.cuda(), seq.cuda(), w.cuda(), strategy, eos_token_id=EOS)
    assert not val.requires_grad and abs(val.item() - loss.item()) <= 1e-6 * abs(loss.item())


@pytest.mark.parametrize("strategy", ["unilm", "normal"])
def test_unit_weights_agree_with_the_cross_entropy_route(M, specs, strategy):
    pair, _ = _inputs()
    g = torch.Generator().manual_seed(73)
    ids = torch.randint(1000, 3000, (B, T), generator=g)          # captions that fill their rows, no [END]
    ids[ids == EOS] = EOS + 1
    model, _ = _tiny_caption(M, specs, F32)
    new = model.sequence_loss(pair.cuda(), ids.cuda(), torch.ones(B, device="cuda"), strategy, eos_token_id=-1)
    new.backward()
    other, _ = _tiny_caption(M, specs, F32)
    old = other(pair.cuda(), ids.cuda(), 0, strategy, labels=ids.cuda())
    old.backward()
    assert abs(new.item() - old.item()) < 1e-5 * abs(old.item()), (new.item(), old.item())
    g_new, g_old = dict(model.named_parameters()), dict(other.named_parameters())
    for k in KEYS:
        assert rel_err(g_new[k].grad.cpu(), g_old[k].grad.cpu()) < 1e-4, k


def test_a_batch_of_empty_sequences_gives_nan_and_raises_nothing(M, specs):
    model, _ = _tiny_caption(M, specs, F32)
    pair, _ = _inputs()
    loss = model.sequence_loss(pair.cuda(), torch.zeros(B, T, dtype=torch.int64, device="cuda"), torch.ones(B, device="cuda"))
    torch.cuda.synchronize()
    assert math.isnan(loss.item())


def test_sequence_loss_divides_by_the_synced_count(M, specs, monkeypatch):
    """Data parallel: N is replaced by what _mvlt_label_sync returns, in grad mode only (as loss_forward)."""
    model, _ = _tiny_caption(M, specs, F32)
    pair, _ = _inputs()
    seq, w = _sequences().cuda(), _weights("b").cuda()
    alone = model.sequence_loss(pair.cuda(), seq, w, eos_token_id=EOS)
    seen = []

    def fake_sync(count):
        seen.append(float(count))
        return (count + 75.0) / 2.0                   # the other rank scored 75 tokens, world = 2

    monkeypatch.setitem(model.__dict__, "_mvlt_label_sync", fake_sync)
    synced = model.sequence_loss(pair.cuda(), seq, w, eos_token_id=EOS)
    assert seen == [25.0]
    assert abs(synced.item() - alone.item() * 25.0 / 50.0) < 1e-6 * abs(alone.item())
    synced.backward()
    with torch.no_grad():
        quiet = model.sequence_loss(pair.cuda(), seq, w, eos_token_id=EOS)
    assert seen == [25.0] and abs(quiet.item() - alone.item()) < 1e-6 * abs(alone.item())


# ------------------------------------------------------------------ self_critical_loss
OPTS = dict(seed=1234, temperature=1.3, top_k=50, top_p=0.95)
INDEX = [2, 0, 3]


def _scst_setup(M, specs_hash, cd):
    """Model, images and a ReferenceSet made from the model's OWN decodes, so that the rewards are not zero and differ between
    the two decodes (unrelated references share no word with either row: every reward, the advantage, the loss and every
    gradient would be exactly 0 and nothing below would tell a right implementation from a wrong one).  Image 0's reference is
    its greedy row (the greedy reward wins: a negative advantage), image 1's its sampled row (a positive one), image 2's the
    first half of its greedy row followed by the second half of its sampled row; one reference is unrelated ids."""
    model, _ = tiny_caption(M, specs_hash, cd, max_length=8, eos=EOS)
    image, _, _, _ = synth_batch(B, 24, seed=91, vocab=3000)
    image = image.cuda()
    greedy, _ = model.generate(image)
    sample, _ = model.generate(image, sample_mode="sample", **OPTS)
    g, s = greedy.tolist(), sample.tolist()
    for b in range(B):
        assert g[b] != s[b] and R.seq_len(g[b], EOS) >= 2 and R.seq_len(s[b], EOS) >= 2, (b, g[b], s[b])
    gen = torch.Generator().manual_seed(92)
    half = len(g[2]) // 2
    ref_rows = [s[1], torch.randint(1000, 3000, (6,), generator=gen).tolist(), g[0], g[2][:half] + s[2][half:]]
    return model, image, M.ReferenceSet(ref_rows), torch.tensor(INDEX), greedy, sample


def _pick(scores, metric):
    return scores["bleu"][:, 3] if metric == "bleu4" else scores[metric]


@pytest.mark.parametrize("cd", [F32, BF16], ids=["f32", "bf16"])
def test_self_critical_loss_is_made_of_its_pieces(M, specs_hash, cd):
    model, image, refs, index, greedy, sample = _scst_setup(M, specs_hash, cd)
    loss, info = M.self_critical_loss(model, image, refs, index, **OPTS)
    assert set(info) == {"sample_ids", "greedy_ids", "reward_sample", "reward_greedy", "advantage"}
    assert all(v.is_cuda for v in info.values())
    assert torch.equal(info["greedy_ids"], greedy) and torch.equal(info["sample_ids"], sample)
    s_s, s_g = M.report_metrics.score(sample, refs, index), M.report_metrics.score(greedy, refs, index)
    assert torch.equal(info["reward_sample"], s_s["cider"]) and torch.equal(info["reward_greedy"], s_g["cider"])
    adv = (s_s["cider"] - s_g["cider"]).to(torch.float32)
    print(f"{cd}: reward sample {s_s['cider'].tolist()} greedy {s_g['cider'].tolist()} loss {loss.item():.6f}")
    assert info["advantage"].dtype == torch.float32 and not info["advantage"].requires_grad
    assert torch.equal(info["advantage"], adv)
    # the rewards say something: both signs are present (sample minus greedy, not the reverse), and CIDEr is not another column
    assert float(adv[0]) < 0 < float(adv[1]) and bool((adv != 0).all())
    assert not torch.equal(adv, (_pick(s_s, "bleu4") - _pick(s_g, "bleu4")).to(torch.float32))
    # eval mode: the loss is sequence_loss on the SAMPLED rows, bit for bit -- and not on the greedy ones
    direct = model.sequence_loss(image, sample, adv)
    assert loss.item() != 0.0 and torch.equal(loss.detach(), direct.detach())
    if greedy.shape == sample.shape:
        assert not torch.equal(model.sequence_loss(image, greedy, adv).detach(), loss.detach())
    loss.backward()
    named = dict(model.named_parameters())
    for k in KEYS:
        assert named[k].grad is not None and bool(torch.isfinite(named[k].grad).all()), k
        assert bool((named[k].grad != 0).any()), k
    # the same seed gives the same bits
    again, info2 = M.self_critical_loss(model, image, refs, index, **OPTS)
    assert torch.equal(again.detach(), loss.detach())
    for k in info:
        assert torch.equal(info[k], info2[k]), k


def test_self_critical_loss_other_metrics_and_refusals(M, specs_hash):
    model, image, refs, index, greedy, sample = _scst_setup(M, specs_hash, BF16)
    seen = {}
    for metric in ("cider", "bleu4", "rouge_l"):
        loss, info = M.self_critical_loss(model, image, refs, index, metric=metric, **OPTS)
        s_s = M.report_metrics.score(info["sample_ids"], refs, index)
        s_g = M.report_metrics.score(info["greedy_ids"], refs, index)
        adv = (_pick(s_s, metric) - _pick(s_g, metric)).to(torch.float32)
        assert torch.equal(info["advantage"], adv), metric
        assert torch.equal(info["reward_sample"], _pick(s_s, metric)) and torch.equal(info["reward_greedy"], _pick(s_g, metric))
        assert float(adv[0]) < 0 < float(adv[1]), (metric, adv.tolist())
        assert loss.item() != 0.0 and torch.equal(loss.detach(), model.sequence_loss(image, sample, adv).detach()), metric
        seen[metric] = adv
    assert not torch.equal(seen["cider"], seen["bleu4"]) and not torch.equal(seen["cider"], seen["rouge_l"])
    assert not torch.equal(seen["bleu4"], seen["rouge_l"])
    with pytest.raises(NotImplementedError):
        M.self_critical_loss(model, image, refs, index, learning_strategy="normal")
    with pytest.raises(ValueError):
        M.self_critical_loss(model, image, refs, index, metric="meteor")
