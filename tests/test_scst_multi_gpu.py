"""Multi-sample self-critical training on the GPU: ``scst.self_critical_loss(num_samples=, baseline=, one_pass=)`` against the pieces
it is made of -- ``decode.sample_many``, ``report_metrics.score``, ``scst.advantages`` and ``sequence_loss_from_features`` over the
B * K sampled rows -- with references made from the model's own decodes, so that the rewards differ (the reason is given at
test_scst_gpu._scst_setup)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import multi_sample_ref as MR  # noqa: E402
import sample_ref as S  # noqa: E402
import seq_loss_ref as R  # noqa: E402
from conftest import synth_batch  # noqa: E402
from test_caption_loss_gpu import KEYS  # noqa: E402
from test_sample_gpu import _tiny_oracle_cfgs  # noqa: E402
from tiny_caption import tiny_caption  # noqa: E402

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
B, K = 3, 3
EOS = R.EOS
OPTS = dict(seed=1234, temperature=1.3)
INDEX = [2, 0, 3]


@pytest.fixture(scope="module")
def M():
    import mvlt_amd
    return mvlt_amd


def _feature(model, image):
    from mvlt_amd.arena import Arena
    from mvlt_amd.runtime import compute_dtype_of
    Arena.of(model, compute_dtype_of(model))
    return model.conv(image)


def _setup(M, specs_hash, cd):
    """Model, images, the one-pass decode the loss will repeat (greedy row + K samples) and a ReferenceSet made from it: image 0's
    reference is its greedy row (no sample can beat the baseline), image 1's its first sample (a positive advantage), image 2's
    the first half of its greedy row followed by the second half of its second sample; one reference is unrelated ids."""
    model, sd = tiny_caption(M, specs_hash, cd, max_length=8, eos=EOS)
    image, _, _, _ = synth_batch(B, 24, seed=91, vocab=3000)
    image = image.cuda()
    with torch.no_grad():
        ids, _ = M.sample_many(model, _feature(model, image), K, include_greedy=True, **OPTS)
    rows = ids.tolist()
    for b in range(B):
        assert len({tuple(r) for r in rows[b]}) > 1 and all(R.seq_len(r, EOS) >= 2 for r in rows[b]), (b, rows[b])
    gen = torch.Generator().manual_seed(92)
    half = ids.shape[2] // 2
    ref_rows = [rows[1][1], torch.randint(1000, 3000, (6,), generator=gen).tolist(), rows[0][0], rows[2][0][:half] + rows[2][2][half:]]
    return model, sd, image, M.ReferenceSet(ref_rows), torch.tensor(INDEX), ids


@pytest.mark.parametrize("cd", [F32, BF16], ids=["f32", "bf16"])
def test_greedy_baseline_is_made_of_its_pieces(M, specs_hash, cd):
    model, _, image, refs, index, ids = _setup(M, specs_hash, cd)
    loss, info = M.self_critical_loss(model, image, refs, index, num_samples=K, baseline='greedy', **OPTS)
    assert set(info) == {"sample_ids", "greedy_ids", "reward_sample", "reward_greedy", "advantage"}
    assert all(v.is_cuda for v in info.values())
    n = ids.shape[2]
    assert torch.equal(info["greedy_ids"], ids[:, 0]) and torch.equal(info["sample_ids"], ids[:, 1:])
    assert info["sample_ids"].shape == (B, K, n) and info["reward_sample"].shape == (B, K) and info["advantage"].shape == (B, K)
    flat = ids[:, 1:].reshape(B * K, n)
    s_s = M.report_metrics.score(flat, refs, index.repeat_interleave(K))["cider"].view(B, K)
    s_g = M.report_metrics.score(ids[:, 0], refs, index)["cider"]
    assert torch.equal(info["reward_sample"], s_s) and torch.equal(info["reward_greedy"], s_g)
    adv = (s_s - s_g[:, None]).to(torch.float32)
    print(f"{cd}: reward samples {s_s.tolist()} greedy {s_g.tolist()} loss {loss.item():.6f}")
    assert info["advantage"].dtype == torch.float32 and not info["advantage"].requires_grad and torch.equal(info["advantage"], adv)
    assert torch.equal(adv, M.scst.advantages(s_s, s_g, 'greedy'))
    assert bool((adv < 0).any()) and bool((adv > 0).any())
    # eval mode: ONE sequence loss over the B * K sampled rows on the repeated features, bit for bit
    direct = model.sequence_loss_from_features(_feature(model, image).repeat_interleave(K, 0), flat, adv.view(-1))
    assert loss.item() != 0.0 and torch.equal(loss.detach(), direct.detach())
    loss.backward()
    named = dict(model.named_parameters())
    for k in KEYS:
        assert named[k].grad is not None and bool(torch.isfinite(named[k].grad).all()), k
        assert bool((named[k].grad != 0).any()), k
    again, info2 = M.self_critical_loss(model, image, refs, index, num_samples=K, baseline='greedy', **OPTS)
    assert torch.equal(again.detach(), loss.detach())
    for k in info:
        assert torch.equal(info[k], info2[k]), k


def test_mean_baseline_leaves_one_out(M, specs_hash):
    model, _, image, refs, index, ids = _setup(M, specs_hash, F32)
    loss, info = M.self_critical_loss(model, image, refs, index, num_samples=K, baseline='mean', **OPTS)
    assert set(info) == {"sample_ids", "reward_sample", "advantage"}                  # no greedy row was decoded
    assert torch.equal(info["sample_ids"], ids[:, 1:])                                 # the draws do not depend on the greedy row
    r = info["reward_sample"]
    assert r.dtype == torch.float64 and r.shape == (B, K)
    want = torch.stack([r[:, k] - (r.sum(1) - r[:, k]) / (K - 1) for k in range(K)], 1)
    assert torch.equal(info["advantage"], want.to(torch.float32))
    assert float(want.sum(1).abs().max()) <= 16 * 2.0 ** -52 * max(float(r.abs().max()), 1.0)
    assert float(info["advantage"].double().sum(1).abs().max()) <= K * 2.0 ** -23 * max(float(r.abs().max()), 1.0)
    assert bool((info["advantage"] != 0).any())
    greedy_loss, _ = M.self_critical_loss(model, image, refs, index, num_samples=K, baseline='greedy', **OPTS)
    assert loss.item() != 0.0 and not torch.equal(loss.detach(), greedy_loss.detach())
    n = ids.shape[2]
    direct = model.sequence_loss_from_features(_feature(model, image).repeat_interleave(K, 0), ids[:, 1:].reshape(B * K, n),
                                               info["advantage"].view(-1))
    assert torch.equal(loss.detach(), direct.detach())


def test_one_pass_with_one_sample_has_the_shapes_of_today(M, specs_hash):
    model, sd, image, refs, index, _ = _setup(M, specs_hash, F32)
    loss, info = M.self_critical_loss(model, image, refs, index, one_pass=True, **OPTS)
    assert set(info) == {"sample_ids", "greedy_ids", "reward_sample", "reward_greedy", "advantage"}
    n = info["sample_ids"].shape[1]
    assert info["sample_ids"].shape == (B, n) and info["greedy_ids"].shape == (B, n)
    assert info["reward_sample"].shape == (B,) and info["reward_greedy"].shape == (B,) and info["advantage"].shape == (B,)
    assert bool(torch.isfinite(loss)) and loss.item() != 0.0
    assert torch.equal(info["advantage"], (info["reward_sample"] - info["reward_greedy"]).to(torch.float32))
    # the 2 B rows of the pass, pick by pick against the oracle: greedy rows without noise, sample b with the noise of row b
    from mvlt_amd import decode
    noise_row, inv_t, _ = decode.multi_sample_tables(B, 1, True, OPTS["temperature"], 8)
    ids = torch.stack([info["greedy_ids"], info["sample_ids"]], 1).cpu()
    O, scfg, bcfg = _tiny_oracle_cfgs()
    with torch.no_grad():
        exact, near, bad, _ = MR.teacher_forced_rows(O, sd, scfg, bcfg, image.cpu(), ids, OPTS["seed"], noise_row, inv_t, eos=EOS)
    msg = f"{exact} exact, {near} near-ties, wrong {bad} of {ids.numel()} picks"
    assert not bad and near <= S.NEAR_TIE_CAP * ids.numel() and exact > 0, msg
    # and the default call is still the two decodes: the same samples (noise row b either way), its own greedy decode
    _, two = M.self_critical_loss(model, image, refs, index, **OPTS)
    assert two["sample_ids"].dim() == 2 and two["advantage"].shape == (B,)


def test_refusals(M, specs_hash):
    model, _, image, refs, index, _ = _setup(M, specs_hash, BF16)
    for kw in (dict(num_samples=K, top_k=50), dict(num_samples=K, top_p=0.9), dict(one_pass=True, top_k=5), dict(baseline='mean'),
               dict(baseline='mean', num_samples=1, one_pass=True), dict(baseline='median'), dict(num_samples=0),
               dict(num_samples=K, one_pass=False)):
        with pytest.raises(ValueError):
            M.self_critical_loss(model, image, refs, index, **kw)
