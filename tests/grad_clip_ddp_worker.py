"""Worker of tests/test_grad_clip_ddp_gpu.py: one data-parallel rank takes ONE clipped optimizer step on the tiny pre-training model.
    RANK / WORLD_SIZE / MASTER_ADDR / MASTER_PORT from the environment; argv: backend device_index out_prefix max_grad_norm
Every rank stores its gradient norm (opt.last_grad_norm) and its parameters after the step in <out_prefix>.rank<r>.pt."""
import os
import random
import sys

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    backend, dev, out, max_norm = sys.argv[1], int(sys.argv[2]), sys.argv[3], float(sys.argv[4])
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    torch.cuda.set_device(dev)
    dist.init_process_group(backend, rank=rank, world_size=world)
    import mvlt_amd as M
    from mvlt_amd.ddp import GradReducer
    from mvlt_amd.train import PretrainStep
    from conftest import synth_batch
    from ddp_gpu_worker import build_model
    model = build_model(M)
    red = GradReducer(model, bucket_bytes=256 << 10)
    image, ids, labels, itm = synth_batch(2 * world, 24, seed=71, vocab=3000)
    sl = slice(2 * rank, 2 * rank + 2)
    random.random = lambda: 0.9
    batch = (image[sl].cuda(), ids[sl].cuda(), labels[sl].cuda(), itm[sl].cuda())
    step = PretrainStep(model, lr=1e-3, reducer=red, world_size=world, max_grad_norm=max_norm, skip_nonfinite=True)
    loss = step(batch)
    torch.cuda.synchronize()
    assert len(red.launched) > 2 and step.opt.steps_skipped == 0
    torch.save({"norm": step.opt.last_grad_norm.detach().cpu().clone(), "loss": float(loss),
                "params": {k: p.detach().cpu().clone() for k, p in model.named_parameters()}}, f"{out}.rank{rank}.pt")
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
