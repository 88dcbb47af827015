"""Global-norm clipping under data parallelism: the norm is taken at step() time over the REDUCED gradients, so every rank computes
it from the same bytes -- all ranks clip alike without a collective of their own.  Two worker processes
(tests/grad_clip_ddp_worker.py), one per GPU over RCCL when the box has >= 2 GPUs; on a one-GPU box both share cuda:0 and exchange
through gloo, like tests/test_ddp_gpu.py."""
import os
import random
import socket
import subprocess
import sys

import pytest
import torch

from conftest import rel_err, synth_batch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_NORM = 0.01


def _run_two_ranks(tmp_path):
    ndev = torch.cuda.device_count()
    backend = "nccl" if ndev >= 2 else "gloo"
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    out = str(tmp_path / "clip")
    procs = []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "grad_clip_ddp_worker.py"), backend,
                                       str(rank if ndev >= 2 else 0), out, repr(MAX_NORM)],
                                      env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    logs = []
    for p in procs:
        try:
            o, _ = p.communicate(timeout=300)
        except subprocess.TimeoutExpired:
            p.kill()
            o, _ = p.communicate()
        logs.append(o)
    assert all(p.returncode == 0 for p in procs), "\n".join(l[-3000:] for l in logs)
    return [torch.load(f"{out}.rank{r}.pt") for r in range(2)]


def test_two_ranks_clip_alike_and_equal_the_single_process_clipped_step(tmp_path, monkeypatch):
    r0, r1 = _run_two_ranks(tmp_path)
    # every rank read the same reduced gradients: same norm, same coefficient, same parameters -- to the bit
    assert torch.equal(r0["norm"], r1["norm"])
    assert r0["params"].keys() == r1["params"].keys() and len(r0["params"]) > 150
    assert all(torch.equal(r0["params"][k], r1["params"][k]) for k in r0["params"])
    # ... and they are the single-process step over the global batch of 4, clipped at the same norm
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import mvlt_amd as M
    from ddp_gpu_worker import build_model
    from mvlt_amd.train import PretrainStep
    model = build_model(M)
    before = {k: p.detach().cpu().clone() for k, p in model.named_parameters()}
    image, ids, labels, itm = synth_batch(4, 24, seed=71, vocab=3000)
    monkeypatch.setattr(random, "random", lambda: 0.9)
    step = PretrainStep(model, lr=1e-3, max_grad_norm=MAX_NORM)
    step((image.cuda(), ids.cuda(), labels.cuda(), itm.cuda()))
    torch.cuda.synchronize()
    norm = step.opt.last_grad_norm.item()
    assert norm > 10 * MAX_NORM                                   # the step WAS clipped
    assert abs(r0["norm"].item() - norm) <= 2e-4 * norm           # (the gradient bound of tests/test_ddp_gpu.py)
    after = {k: p.detach().cpu() for k, p in model.named_parameters()}
    assert any(not torch.equal(after[k], before[k]) for k in after)
    bad = [(k, rel_err(r0["params"][k], after[k])) for k in after if rel_err(r0["params"][k], after[k]) > 1e-5]
    assert not bad, bad[:10]
