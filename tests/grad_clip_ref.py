"""fp64 restatement of what the guarded optimizer step computes (mvlt_grad_sumsq, mvlt_grad_norm_finish, mvlt_adamw_guarded):
global L2 norm of a gradient set, the clip coefficient of torch.nn.utils.clip_grad_norm_, the non-finite skip, and
torch.optim.AdamW's single-tensor update.  Everything is fp64 except the coefficient, which the kernel forms in f32 from the f32
norm -- restated here with numpy f32 scalars so that a test can ask for it bit for bit."""
import math

import numpy as np
import torch


def sumsq(grads):
    """Sum of squares of every element of ``grads`` (iterable of tensors), each widened to fp64 first."""
    s = 0.0
    for g in grads:
        g = g.detach().double().reshape(-1)
        s += float((g * g).sum())
    return s


def grad_norm(grads, grad_scale=1.0):
    return abs(float(grad_scale)) * math.sqrt(sumsq(grads))


def clip_coef(norm, max_norm):
    """f32: min(1, max_norm / (norm + 1e-6)); 1 when max_norm <= 0 (or None).  A NaN norm gives NaN, as torch.clamp keeps it."""
    if max_norm is None or max_norm <= 0:
        return np.float32(1.0)
    with np.errstate(all="ignore"):
        c = np.float32(max_norm) / (np.float32(norm) + np.float32(1e-6))
    return np.float32(1.0) if c > np.float32(1.0) else c


def skip(ssq, skip_nonfinite):
    return bool(skip_nonfinite) and not math.isfinite(ssq)


class RefAdamW:
    """AdamW over one flat fp64 parameter vector with per-element step counts; ``step`` updates the elements of ``live`` (bool mask:
    the parameters that received a gradient) from ``grad`` scaled by grad_scale * clip coefficient, or nothing when skipped."""

    def __init__(self, flat, lr=4e-5, betas=(0.9, 0.999), eps=1e-6, weight_decay=1e-4, grad_scale=1.0,
                 max_grad_norm=None, skip_nonfinite=False):
        self.p = flat.detach().double().cpu().clone()
        self.m = torch.zeros_like(self.p)
        self.v = torch.zeros_like(self.p)
        self.steps = torch.zeros(self.p.numel(), dtype=torch.int64)
        self.lr, self.betas, self.eps, self.wd, self.gs = lr, betas, eps, weight_decay, grad_scale
        self.max_grad_norm, self.skip_nonfinite = max_grad_norm, skip_nonfinite
        self.skipped = 0
        self.last_norm = None

    def step(self, grad, live=None):
        g = grad.detach().double().cpu().reshape(-1)
        live = torch.ones_like(g, dtype=torch.bool) if live is None else live.cpu().reshape(-1)
        ssq = sumsq([g[live]])
        self.last_norm = abs(self.gs) * math.sqrt(ssq)
        if skip(ssq, self.skip_nonfinite):
            self.skipped += 1
            return
        coef = float(clip_coef(self.last_norm, self.max_grad_norm))
        scale = float(np.float32(self.gs) * np.float32(coef))          # one f32 product, as the kernel forms it
        b1, b2 = self.betas
        t = (self.steps[live] + 1).double()
        gr = g[live] * scale
        p = self.p[live] * (1.0 - self.lr * self.wd)
        m = b1 * self.m[live] + (1.0 - b1) * gr
        v = b2 * self.v[live] + (1.0 - b2) * gr * gr
        bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
        p = p - (self.lr / bc1) * m / (v.sqrt() / bc2.sqrt() + self.eps)
        self.p[live], self.m[live], self.v[live] = p, m, v
        self.steps[live] += 1
