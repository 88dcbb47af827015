"""fp64 restatement of the grouped optimizer step (mvlt_adamw_groups behind FusedAdamW(param_groups=...)): RefAdamW of
tests/grad_clip_ref.py with a learning-rate VECTOR and a weight-decay VECTOR in place of the two scalars -- one entry per element of
the flat parameter vector -- and the same clip and skip (grad_clip_ref.sumsq / clip_coef / skip)."""
import math

import numpy as np
import torch

import grad_clip_ref as R


class RefGroupedAdamW:
    """``lr`` and ``weight_decay``: fp64 vectors over the flat parameter vector (a scalar is broadcast).  ``step(grad, live, lr=)``
    updates the elements of ``live``; ``lr`` there replaces the vector for that step (an LR schedule: pass base vector * factor)."""

    def __init__(self, flat, lr, weight_decay, betas=(0.9, 0.999), eps=1e-6, grad_scale=1.0, max_grad_norm=None, skip_nonfinite=False):
        self.p = flat.detach().double().cpu().clone()
        n = self.p.numel()
        self.lr = torch.as_tensor(lr, dtype=torch.float64).expand(n).clone()
        self.wd = torch.as_tensor(weight_decay, dtype=torch.float64).expand(n).clone()
        self.m = torch.zeros_like(self.p)
        self.v = torch.zeros_like(self.p)
        self.steps = torch.zeros(n, dtype=torch.int64)
        self.betas, self.eps, self.gs = betas, eps, grad_scale
        self.max_grad_norm, self.skip_nonfinite = max_grad_norm, skip_nonfinite
        self.skipped = 0
        self.last_norm = None

    def step(self, grad, live=None, lr=None):
        g = grad.detach().double().cpu().reshape(-1)
        live = torch.ones_like(g, dtype=torch.bool) if live is None else live.cpu().reshape(-1)
        lr_v = (self.lr if lr is None else torch.as_tensor(lr, dtype=torch.float64).expand(g.numel()))[live]
        wd_v = self.wd[live]
        ssq = R.sumsq([g[live]])
        self.last_norm = abs(self.gs) * math.sqrt(ssq)
        if R.skip(ssq, self.skip_nonfinite):
            self.skipped += 1
            return
        coef = float(R.clip_coef(self.last_norm, self.max_grad_norm))
        scale = float(np.float32(self.gs) * np.float32(coef))          # one f32 product, as the kernel forms it
        b1, b2 = self.betas
        t = (self.steps[live] + 1).double()
        gr = g[live] * scale
        p = self.p[live] * (1.0 - lr_v * wd_v)
        m = b1 * self.m[live] + (1.0 - b1) * gr
        v = b2 * self.v[live] + (1.0 - b2) * gr * gr
        bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
        p = p - (lr_v / bc1) * m / (v.sqrt() / bc2.sqrt() + self.eps)
        self.p[live], self.m[live], self.v[live] = p, m, v
        self.steps[live] += 1


def element_hyper(ar, opt):
    """(lr_scale vector, weight-decay vector) over the arena ``ar`` from the read-only view ``opt.param_groups`` (the padding
    keeps 0: it is never live)."""
    lr = torch.zeros(ar.total, dtype=torch.float64)
    wd = torch.zeros(ar.total, dtype=torch.float64)
    of = {n: g for g in opt.param_groups for n in g["names"]}
    for name, p in zip(ar.names, ar.params):
        o, n = ar.offset[id(p)], p.numel()
        lr[o:o + n] = of[name]["lr_scale"]
        wd[o:o + n] = of[name]["weight_decay"]
    return lr, wd
