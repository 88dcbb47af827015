"""Fused AdamW over the flat parameter arena (reference: torch.optim.AdamW at
run_pretrain.py:165-166 -- lr 4e-5, betas (0.9, 0.999), eps 1e-6, weight_decay 1e-4).

One ``mvlt_adamw`` launch per contiguous run of parameters that received a
gradient this step (typically 4-6 launches for 208.9 M parameters); the same
pass refreshes the bf16 compute copy.  Parameters without a gradient are
skipped entirely -- no weight decay, no moment update, own step counter --
exactly like torch.optim.AdamW treats ``p.grad is None`` (idle MLM head,
unused ``head`` / ``resnet_fc`` / ``embedding_LayerNorm``).

``overlap_with_backward``: AdamW is HBM-bound (30 B/parameter) while the
backward pass is MFMA-bound, so the update of a finished slice of the arena
(everything above the backward watermark; under DDP: a bucket whose
all-reduce has been issued) is queued on a third HIP stream while the
backward pass continues below it.  ``step()`` then only handles what is left
and joins the stream.  Same arithmetic, same result; only for loops that call
``backward(); step()`` once each per batch (mvlt_amd.train.PretrainStep).

``max_grad_norm`` / ``skip_nonfinite`` (opt-in; the reference does neither): the L2 norm of the live gradient set is
taken on the device (``mvlt_grad_sumsq`` over the runs of the sweep, ``mvlt_grad_norm_finish``) and the sweep becomes
``mvlt_adamw_guarded``, which reads the clip coefficient and the skip flag from device memory: global-norm clipping
as ``torch.nn.utils.clip_grad_norm_`` defines it, and a step whose gradients hold a NaN or an Inf is not applied --
no host synchronisation in either case.  With both options off the launches are the ones described above.

``param_groups`` (opt-in): per-group learning-rate scale and weight decay -- no weight decay on biases / LayerNorm weights / Swin's
relative-position tables (``no_decay_rules()``), a smaller learning rate for a pretrained backbone (``param_groups_by_name``).  Weights
and biases alternate along the arena, so the groups are resolved INSIDE the sweep (``mvlt_adamw_groups``: one byte per ALIGN-element
block names its group, two f32 tables hold the constants): the step stays 4-6 launches on every route above.  ``LRSchedule`` moves
``opt.lr`` on the host between steps (warm-up, then linear / cosine / constant).  Without ``param_groups`` nothing changes.
"""
import math

import torch

from . import ops
from .arena import ALIGN, Arena
from .runtime import compute_dtype_of


MAX_GROUPS = 256          # a uint8 per arena block names its group (mvlt_adamw_groups)


def _named(model):
    """(name, parameter) as the arena names them: state-dict names, a shared parameter once."""
    return list(model.named_parameters())


def _hyper_value(what, v, where):
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or v < 0:
        raise ValueError(f"{what} must be a finite number >= 0, got {v!r} ({where})")
    return float(v)


def _resolve_groups(model, groups):
    """param_groups as the user wrote them -> [dict(names=(...), lr_scale=float, weight_decay=float or None)], every complaint
    raised here: construction needs no arena and no GPU."""
    named = _named(model)
    name_of = {id(p): n for n, p in named}
    known = set(name_of.values())
    owner, out = {}, []
    for k, g in enumerate(groups):
        if not isinstance(g, dict):
            raise ValueError(f"param_groups[{k}] must be a dict, got {type(g).__name__}")
        extra = set(g) - {"params", "names", "lr_scale", "weight_decay"}
        if extra:
            raise ValueError(f"param_groups[{k}]: unknown keys {sorted(extra)} (params, names, lr_scale, weight_decay)")
        names = []
        for p in g.get("params") or ():
            if id(p) not in name_of:
                raise ValueError(f"param_groups[{k}]: a tensor of shape {tuple(getattr(p, 'shape', ()))} is not a parameter of the model")
            names.append(name_of[id(p)])
        for n in g.get("names") or ():
            if n not in known:
                raise KeyError(f"param_groups[{k}]: unknown parameter name {n!r}")
            names.append(n)
        for n in names:
            if n in owner:
                raise ValueError(f"parameter {n!r} is in param_groups[{owner[n]}] and in param_groups[{k}]"
                                 if owner[n] != k else f"parameter {n!r} is listed twice in param_groups[{k}]")
            owner[n] = k
        wd = g.get("weight_decay")
        out.append(dict(names=tuple(names), lr_scale=_hyper_value("lr_scale", g.get("lr_scale", 1.0), f"param_groups[{k}]"),
                        weight_decay=None if wd is None else _hyper_value("weight_decay", wd, f"param_groups[{k}]")))
    return out


def _no_decay(name, p):
    return p.dim() <= 1 or name.endswith(".bias") or "relative_position_bias_table" in name or "absolute_pos_embed" in name


def no_decay_rules():
    """Rules for param_groups_by_name: weight decay 0 for biases, LayerNorm weights (every parameter with dim() <= 1) and Swin's
    relative_position_bias_table / absolute_pos_embed -- HF's ``no_decay`` list and Swin's no_weight_decay().  Everything else,
    embedding tables included, keeps the optimizer's weight decay, as HF does for BERT."""
    return [(_no_decay, dict(weight_decay=0.0))]


def param_groups_by_name(model, rules):
    """param_groups for FusedAdamW from ``rules`` = [(regex, dict(lr_scale=..., weight_decay=...))].  The regex is searched in the
    state-dict name (re.search; a callable (name, parameter) -> bool is taken as is: no_decay_rules() tests dim()).  The FIRST
    matching rule that sets a value wins, per value -- so rule lists compose: [(r"^conv[.]", dict(lr_scale=0.1))] +
    no_decay_rules() gives a backbone bias lr_scale 0.1 AND weight decay 0, four groups in all.  Parameters that resolve to the same
    (lr_scale, weight_decay) share a group; parameters no rule touches are left out (FusedAdamW keeps them at its own values)."""
    import re
    tests = []
    for k, (pat, sets) in enumerate(rules):
        extra = set(sets) - {"lr_scale", "weight_decay"}
        if extra:
            raise ValueError(f"rule {k}: unknown keys {sorted(extra)} (lr_scale, weight_decay)")
        for key, v in sets.items():
            _hyper_value(key, v, f"rule {k}")
        tests.append((pat if callable(pat) else (lambda n, p, rx=re.compile(pat): rx.search(n) is not None), sets))
    groups = {}
    for name, p in _named(model):
        got = {}
        for test, sets in tests:
            if test(name, p):
                for key, v in sets.items():
                    got.setdefault(key, float(v))
        if got:
            groups.setdefault((got.get("lr_scale"), got.get("weight_decay")), []).append(name)
    return [dict(names=names, **{k: v for k, v in (("lr_scale", ls), ("weight_decay", wd)) if v is not None})
            for (ls, wd), names in groups.items()]


class LRSchedule:
    """Warm-up and decay of FusedAdamW's learning rate (torch.optim.lr_scheduler refuses anything that is not a torch Optimizer).
    ``step()`` -- once after every opt.step() -- advances t and sets opt.lr = base_lr * factor(t) on the host, in fp64; the value is a
    scalar argument of the next step's launches (a deferred optimizer tail keeps the lr of the step it belongs to), so nothing is
    synchronised.  Per-group lr_scale factors multiply it on the device.  factor(t):
        t < warmup_steps             t / warmup_steps                       (the first step runs at factor(0), as torch's LambdaLR)
        "constant"                   1
        "linear"                     max(min_ratio, (total_steps - t) / (total_steps - warmup_steps))
        "cosine"                     min_ratio + (1 - min_ratio) * 0.5 * (1 + cos(pi * (t - warmup_steps) / (total_steps - warmup_steps)))
        t >= total_steps             min_ratio, whatever the kind (the schedule is over; "constant" drops from 1 to it)
    The schedule counts CALLS: it also advances on a step that skip_nonfinite refused (whether the device refused it is not known
    on the host when step() returns), exactly as a torch scheduler beside a GradScaler-skipped step."""
    KINDS = ("linear", "cosine", "constant")

    def __init__(self, opt, warmup_steps, total_steps, kind="linear", min_ratio=0.0):
        if kind not in self.KINDS:
            raise ValueError(f"kind must be one of {self.KINDS}, got {kind!r}")
        if int(warmup_steps) != warmup_steps or int(total_steps) != total_steps or not 0 <= warmup_steps < total_steps:
            raise ValueError(f"need integers 0 <= warmup_steps < total_steps, got {warmup_steps!r}, {total_steps!r}")
        if not (isinstance(min_ratio, (int, float)) and 0.0 <= min_ratio <= 1.0):
            raise ValueError(f"min_ratio must be in [0, 1], got {min_ratio!r}")
        self.opt, self.warmup_steps, self.total_steps = opt, int(warmup_steps), int(total_steps)
        self.kind, self.min_ratio = kind, float(min_ratio)
        self.base_lr, self.t = float(opt.lr), 0
        opt.lr = self.base_lr * self.factor(0)

    def factor(self, t: int) -> float:
        w, n = self.warmup_steps, self.total_steps
        if t < w:
            return t / w
        if t >= n:
            return self.min_ratio
        if self.kind == "constant":
            return 1.0
        if self.kind == "linear":
            return max(self.min_ratio, (n - t) / (n - w))
        return self.min_ratio + (1.0 - self.min_ratio) * 0.5 * (1.0 + math.cos(math.pi * (t - w) / (n - w)))

    def step(self) -> float:
        self.t += 1
        self.opt.lr = self.base_lr * self.factor(self.t)
        return self.opt.lr

    def state_dict(self):
        return dict(t=self.t, base_lr=self.base_lr)

    def load_state_dict(self, sd) -> None:
        self.t, self.base_lr = int(sd["t"]), float(sd["base_lr"])
        self.opt.lr = self.base_lr * self.factor(self.t)


class _OptTail:
    """The part of one optimizer step that FusedAdamW(defer_tail=True) has NOT launched yet: the runs of the arena above
    ``split`` (BertLayers 1.. and the heads), in chunks.  The next forward pass launches them on the optimizer stream
    beside the encoder (``launch``: MVLBert._forward, behind the Swin tower) and waits for a chunk right before the first
    layer that reads its parameters (``wait_for``); anything else that is about to read parameters applies what is left in
    stream order (``flush``: Arena.refresh_shadow, the next step(), state_dict, PretrainStep.flush)."""

    def __init__(self, opt, ar, chunks):
        self.opt = opt
        self.ar = ar
        self.chunks = chunks            # [dict(lo=, runs=[(lo, hi, step)], event=None, waited=False)] in arena order
        self.launched = False
        # the hyper-parameters of the step this tail belongs to (an LR schedule may move opt.lr before the tail runs)
        self.hyper = opt._hyper()

    def _run(self, ch):
        for lo, hi, st in ch["runs"]:
            self.opt._launch(self.ar, lo, hi, st + 1, self.hyper)

    def launch(self):
        """Queue every chunk on the optimizer stream behind what the current stream has queued so far."""
        if self.launched:
            return
        self.launched = True
        dev = self.ar.flat.device
        st = ops.opt_stream(dev)
        st.wait_stream(torch.cuda.current_stream())
        with ops.on_stream(st, "opt"):
            for ch in self.chunks:
                self._run(ch)
                ch["event"] = torch.cuda.Event()
                ch["event"].record(st)

    def wait_for(self, offset=None):
        """The current stream waits for every chunk that holds parameters below ``offset`` (None: all of them)."""
        done = True
        for ch in self.chunks:
            if ch["waited"]:
                continue
            if offset is None or ch["lo"] < offset:
                torch.cuda.current_stream().wait_event(ch["event"])
                ch["waited"] = True
            else:
                done = False
        if done:
            self.ar.__dict__["_opt_tail"] = None

    def flush(self):
        """Apply what has not been launched in stream order on the CURRENT stream; wait for what has."""
        if not self.launched:
            self.launched = True
            for ch in self.chunks:
                self._run(ch)
                ch["waited"] = True
            self.ar.__dict__["_opt_tail"] = None
        else:
            self.wait_for(None)


class FusedAdamW:
    def __init__(self, model, lr=4e-5, betas=(0.9, 0.999), eps=1e-6, weight_decay=1e-4, grad_scale=1.0, defer_tail=False,
                 max_grad_norm=None, skip_nonfinite=False, param_groups=None):
        self.model = model
        # param_groups (opt-in): [dict(params=[Parameter, ...] and / or names=[state-dict name, ...], lr_scale=1.0, weight_decay=<the
        # optimizer's>)]; parameters that no dict lists keep the optimizer's lr and weight decay.  The groups are resolved INSIDE the
        # sweep (mvlt_adamw_groups: a byte per ALIGN-element block of the arena names its group), so the step stays 4-6 launches on
        # every route -- plain, guarded, overlap_with_backward(), defer_tail.  None: the launches are exactly the ungrouped ones.
        self._groups, self._tables = None, None
        # defer_tail (opt-in, mvlt_amd.train.PretrainStep(defer_optimizer_tail=True)): step() updates the parameters the next
        # forward pass reads FIRST (Swin tower, embeddings, BertLayer 0) and leaves the rest -- BertLayers 1.., pooler, heads:
        # 102 M of the 182 M updated parameters, 3.1 GB of the sweep's 5.5 GB -- to the next forward pass, which runs them on the
        # optimizer stream BESIDE the encoder: the sweep is HBM-bound (6 TB/s, no LDS, 57 registers), the BertLayer forward is
        # bound by its GEMMs' L2 -> LDS traffic and moves < 1 TB/s of HBM bytes.  (Not beside the Swin tower: its fused W-MSA
        # workgroups take a whole CU's registers and would queue behind the sweep's waves.)  Same arithmetic, same result:
        # tests/test_model_gpu.py::test_deferred_optimizer_tail_equals_plain_steps.
        self.defer_tail = bool(defer_tail)
        self.lr, self.betas, self.eps, self.weight_decay = lr, betas, eps, weight_decay
        self.grad_scale = grad_scale           # 1/world_size under DDP (gradients are summed, not averaged)
        self._arena = None
        self._overlap = None                   # dict(reducer=, chunk=) when enabled
        self._stepped = set()                  # id(param) already updated during the current backward pass
        self._pending_hi = 0
        # max_grad_norm: clip the global L2 norm of the gradients (grad_scale folded in, i.e. of the rank-averaged gradient under
        # DDP) to this value, torch.nn.utils.clip_grad_norm_ semantics.  skip_nonfinite: a step whose norm is not finite never
        # happened -- parameters, moments, bf16 copy and step counts stay as they were; ``steps_skipped`` counts them.  Both need
        # every gradient of the step before the first update, so neither combines with overlap_with_backward() or defer_tail
        # (ValueError, whichever is asked for first); both can be assigned later (opt.max_grad_norm = 1.0).
        self._max_grad_norm, self._skip_nonfinite = None, False
        self.last_grad_norm = None             # f32 device tensor [] of the last guarded step (no sync to obtain it)
        self._guard_ws = None                  # dict(partial=, out=, flags=, host=) on the arena's device
        self._guard_pending = None             # (arena, event, ids bumped by the last guarded step): see _reconcile
        self._skipped = 0
        self.max_grad_norm = max_grad_norm
        self.skip_nonfinite = skip_nonfinite
        self._set_groups(param_groups)

    @property
    def max_grad_norm(self):
        return self._max_grad_norm

    @max_grad_norm.setter
    def max_grad_norm(self, value):
        if value is not None:
            if isinstance(value, bool) or not isinstance(value, (int, float)) or not math.isfinite(value) or value <= 0:
                raise ValueError(f"max_grad_norm must be a finite number > 0 (or None: no clipping), got {value!r}")
            self._refuse_guard_beside_partial_sweeps()
            value = float(value)
        self._max_grad_norm = value

    @property
    def skip_nonfinite(self):
        return self._skip_nonfinite

    @skip_nonfinite.setter
    def skip_nonfinite(self, value):
        if value:
            self._refuse_guard_beside_partial_sweeps()
        self._skip_nonfinite = bool(value)

    def _refuse_guard_beside_partial_sweeps(self) -> None:
        if self.defer_tail:
            raise ValueError("max_grad_norm / skip_nonfinite cannot be combined with defer_tail=True: the deferred part of the "
                             "sweep runs after the next forward pass has started")
        if self._overlap is not None:
            raise ValueError("max_grad_norm / skip_nonfinite cannot be combined with overlap_with_backward(): the overlapped "
                             "sweep starts before all gradients of the step exist")

    @property
    def _guarded(self) -> bool:
        return self._max_grad_norm is not None or self._skip_nonfinite

    @property
    def steps_skipped(self) -> int:
        """Steps that skip_nonfinite refused so far (waits for the last step's flag: may synchronise)."""
        self._reconcile()
        return self._skipped

    def _reconcile(self) -> None:
        """The step counts live on the host and are bumped when a step is LAUNCHED; whether the device applied it is known one
        copy later.  The skip flag of the last guarded step travelled to pinned host memory behind its sweep: wait for it (in
        steady state it is a whole step old) and take the bump back if that step was refused."""
        pend = self._guard_pending
        if pend is None:
            return
        self._guard_pending = None
        ar, ev, bumped = pend
        ev.synchronize()
        if int(self._guard_ws["host"][0]):
            self._skipped += 1
            for pid in bumped:
                ar.steps[pid] -= 1

    def _guard_buffers(self, ar: Arena):
        ws = self._guard_ws
        if ws is None or ws["out"].device != ar.flat.device:
            dev = ar.flat.device
            ws = self._guard_ws = dict(partial=torch.zeros(ops.grad_sumsq_parts(), dtype=torch.float64, device=dev),
                                       out=torch.zeros(2, dtype=torch.float32, device=dev),
                                       flags=torch.zeros(2, dtype=torch.int32, device=dev),
                                       host=torch.zeros(1, dtype=torch.int32).pin_memory())
            self.last_grad_norm = ws["out"][0]
        return ws

    def _state(self) -> Arena:
        self._reconcile()                # (before a rebuilt arena inherits the step counts)
        ar = Arena.of(self.model, compute_dtype_of(self.model))
        if ar is not self._arena or ar.exp_avg is None:
            ar.exp_avg = torch.zeros_like(ar.flat)
            ar.exp_avg_sq = torch.zeros_like(ar.flat)
            old = self._arena
            if old is not None and old is not ar and old.exp_avg is not None:
                # the arena was rebuilt (dtype switch, .cuda()/.to() after first use): carry the moments and step
                # counts over, parameter by parameter, instead of silently restarting Adam
                for p in ar.params:
                    pid = id(p)
                    if pid in old.offset and old.numel[pid] == p.numel():
                        o, oo, n = ar.offset[pid], old.offset[pid], p.numel()
                        ar.exp_avg[o:o + n].copy_(old.exp_avg[oo:oo + n])
                        ar.exp_avg_sq[o:o + n].copy_(old.exp_avg_sq[oo:oo + n])
                        ar.steps[pid] = old.steps[pid]
                old.exp_avg = old.exp_avg_sq = None
            self._arena = ar
            self.__dict__["_plans"] = {}          # cached (lo, hi) sweep ranges are offsets into the OLD arena layout
            self._tables = self._build_group_tables(ar) if (self._groups is not None and ar.flat.is_cuda) else None
            if self._overlap is not None:
                self._hook(ar)
        return ar

    def zero_grad(self, set_to_none=True):
        """Gradients are overwritten (not accumulated) by every backward pass and
        parameters without a gradient are tracked per step, so nothing to clear; the call only tells the
        arena that the caller is done with the last backward pass's gradients."""
        if self._arena is not None:
            self._arena.note_grads_consumed()

    # ------------------------------------------------------------------ checkpoint / resume (absent in the reference)
    def state_dict(self):
        """Moments and per-parameter step counts keyed by parameter NAME (independent of the arena layout)."""
        ar = self._state()
        self.flush()
        out = {"hyper": dict(lr=self.lr, betas=tuple(self.betas), eps=self.eps, weight_decay=self.weight_decay),
               "state": {}}
        if self._groups is not None:             # by parameter name; weight_decay None = the optimizer's
            out["hyper"]["param_groups"] = [dict(names=list(g["names"]), lr_scale=g["lr_scale"], weight_decay=g["weight_decay"])
                                            for g in self._groups]
        for name, p in zip(ar.names, ar.params):
            o, n = ar.offset[id(p)], p.numel()
            if ar.steps[id(p)] > 0:
                out["state"][name] = dict(step=ar.steps[id(p)],
                                          exp_avg=ar.exp_avg[o:o + n].view(p.shape).detach().cpu().clone(),
                                          exp_avg_sq=ar.exp_avg_sq[o:o + n].view(p.shape).detach().cpu().clone())
        return out

    def load_state_dict(self, sd):
        ar = self._state()
        self.flush()
        hp = sd.get("hyper", {})
        self.lr = hp.get("lr", self.lr)
        self.betas = tuple(hp.get("betas", self.betas))
        self.eps = hp.get("eps", self.eps)
        self.weight_decay = hp.get("weight_decay", self.weight_decay)
        if "param_groups" in hp:                 # (a checkpoint without the key leaves the groups of this optimizer as they are)
            self._set_groups(hp["param_groups"])
        byname = dict(zip(ar.names, ar.params))
        unknown = [k for k in sd["state"] if k not in byname]
        if unknown:
            raise KeyError(f"optimizer state for unknown parameters: {unknown[:5]}")
        ar.exp_avg.zero_(); ar.exp_avg_sq.zero_()
        for p in ar.params:
            ar.steps[id(p)] = 0
        for name, st in sd["state"].items():
            p = byname[name]
            o, n = ar.offset[id(p)], p.numel()
            ar.exp_avg[o:o + n].copy_(st["exp_avg"].reshape(-1))
            ar.exp_avg_sq[o:o + n].copy_(st["exp_avg_sq"].reshape(-1))
            ar.steps[id(p)] = int(st["step"])

    # ------------------------------------------------------------------ parameter groups
    @property
    def param_groups(self):
        """Read-only view for logging: [dict(lr=opt.lr * lr_scale, lr_scale=, weight_decay=, names=[...])], the parameters that no
        group lists first (when there are any).  Without param_groups: one entry that holds every parameter."""
        listed = set(n for g in self._groups or () for n in g["names"])
        rest = [n for n, _ in _named(self.model) if n not in listed]
        out = [dict(lr=self.lr, lr_scale=1.0, weight_decay=self.weight_decay, names=rest)] if rest else []
        for g in self._groups or ():
            wd = self.weight_decay if g["weight_decay"] is None else g["weight_decay"]
            out.append(dict(lr=self.lr * g["lr_scale"], lr_scale=g["lr_scale"], weight_decay=wd, names=list(g["names"])))
        return out

    def _set_groups(self, groups) -> None:
        self._groups = _resolve_groups(self.model, groups) if groups is not None else None
        self._tables = None
        if len(self.param_groups) > MAX_GROUPS:
            self._groups = None
            raise ValueError(f"{len(groups)} param_groups (+ the parameters none of them lists): at most {MAX_GROUPS} groups")

    def _build_group_tables(self, ar: Arena):
        """dict(map=uint8 [ar.total / ALIGN], lr_scale=f32 [g], weight_decay=f32 [g]) on the arena's device: the group of every
        ALIGN-element block of the arena -- a parameter's padding carries the parameter's group -- and the two constants of every
        group.  Group 0 is the parameters no group lists (optimizer's lr and weight decay) when there are any."""
        if ops.adamw_groups_block() != ALIGN:
            raise RuntimeError(f"mvlt_adamw_groups maps blocks of {ops.adamw_groups_block()} elements, the arena aligns to {ALIGN}")
        view = self.param_groups
        gid = {n: k for k, g in enumerate(view) for n in g["names"]}
        bmap = torch.zeros(ar.total // ALIGN, dtype=torch.uint8)
        for name, p in zip(ar.names, ar.params):
            o = ar.offset[id(p)]
            bmap[o // ALIGN:(o + p.numel() + ALIGN - 1) // ALIGN] = gid[name]
        dev = ar.flat.device
        return dict(map=bmap.to(dev), lr_scale=torch.tensor([g["lr_scale"] for g in view], dtype=torch.float32).to(dev),
                    weight_decay=torch.tensor([g["weight_decay"] for g in view], dtype=torch.float32).to(dev),
                    key=(ar, self.weight_decay))

    def _group_tables(self, ar: Arena):
        t = self._tables
        if t is None or t["key"][0] is not ar or t["key"][1] != self.weight_decay:
            t = self._tables = self._build_group_tables(ar)          # (first use, a rebuilt arena, opt.weight_decay assigned)
        return t

    # ------------------------------------------------------------------ the one place that launches the sweep
    def _hyper(self, extra_scale: float = 1.0):
        """(lr, beta1, beta2, eps, weight_decay, grad_scale) of the step that is being launched NOW: a deferred tail keeps its own copy,
        because an LR schedule moves ``lr`` before the tail runs."""
        return (self.lr, self.betas[0], self.betas[1], self.eps, self.weight_decay, self.grad_scale * extra_scale)

    def _launch(self, ar: Arena, lo: int, hi: int, step: int, hyper, guard=None) -> None:
        """One sweep launch over arena elements [lo, hi): plain or grouped (param_groups), plain or guarded (``guard`` = (coef, skip)
        on the device).  Without param_groups these are exactly the mvlt_adamw / mvlt_adamw_guarded launches of before."""
        lr, b1, b2, eps, wd, gs = hyper
        sh = ar.shadow[lo:hi] if ar.shadow is not None else None
        if self._groups is not None:
            t = self._group_tables(ar)
            coef, skip = guard if guard is not None else (None, None)
            ops.adamw_groups(ar.flat[lo:hi], ar.grad[lo:hi], ar.exp_avg[lo:hi], ar.exp_avg_sq[lo:hi], sh,
                             t["map"][lo // ALIGN:hi // ALIGN], t["lr_scale"], t["weight_decay"], lr, b1, b2, eps, step, gs, coef, skip)
        elif guard is not None:
            ops.adamw_guarded(ar.flat[lo:hi], ar.grad[lo:hi], ar.exp_avg[lo:hi], ar.exp_avg_sq[lo:hi], sh,
                              lr, b1, b2, eps, wd, step, gs, guard[0], guard[1])
        else:
            ops.adamw(ar.flat[lo:hi], ar.grad[lo:hi], ar.exp_avg[lo:hi], ar.exp_avg_sq[lo:hi], sh, lr, b1, b2, eps, wd, step, gs)

    # ------------------------------------------------------------------ update of a set of element ranges
    def _apply(self, ar: Arena, params, extra_scale: float = 1.0) -> None:
        """AdamW over ``params`` (arena order): one launch per contiguous run with equal step count."""
        run = None
        runs = []
        for p in params:
            pid = id(p)
            o = ar.offset[pid]
            e = o + (p.numel() + ALIGN - 1) // ALIGN * ALIGN
            st = ar.steps[pid]
            if run is not None and run[1] == o and run[2] == st:
                run[1] = e
            else:
                run = [o, e, st]
                runs.append(run)
        hyper = self._hyper(extra_scale)
        for lo, hi, st in runs:
            self._launch(ar, lo, hi, st + 1, hyper)

    def _plan_runs(self, ar: Arena, params):
        """[(lo, hi, ids of the parameters of the run)]: maximal contiguous arena ranges of ``params`` that
        currently share one step count."""
        runs, run = [], None
        for p in params:
            pid = id(p)
            o = ar.offset[pid]
            e = o + (p.numel() + ALIGN - 1) // ALIGN * ALIGN
            st = ar.steps[pid]
            if run is not None and run[1] == o and run[3] == st:
                run[1] = e
                run[2].append(pid)
            else:
                run = [o, e, [pid], st]
                runs.append(run)
        return [(lo, hi, tuple(ids)) for lo, hi, ids, _ in runs]

    # ------------------------------------------------------------------ overlap with the backward pass
    def overlap_with_backward(self, reducer=None, chunk_bytes: int = 64 << 20) -> "FusedAdamW":
        if self._guarded:
            raise ValueError("overlap_with_backward() cannot be combined with max_grad_norm / skip_nonfinite: the overlapped sweep "
                             "starts before all gradients of the step exist")
        self._overlap = dict(reducer=reducer, chunk=chunk_bytes // 4)
        self._hook(self._state())
        return self

    def _hook(self, ar: Arena) -> None:
        red = self._overlap["reducer"]
        if red is not None:
            red.on_bucket = self._on_bucket
            prev_begin = red._begin

            def begin(arena, prev_begin=prev_begin):
                prev_begin(arena)
                self._begin(arena)
            ar._on_backward_begin = begin
        else:
            ar._on_backward_begin = self._begin
            ar._on_watermark = self._on_watermark

    def _begin(self, ar: Arena) -> None:
        self._stepped = set()
        self._pending_hi = ar.total

    def _on_watermark(self, ar: Arena, lo: int) -> None:
        # single GPU: everything at or above the watermark has its final gradient queued
        if self._pending_hi - lo < self._overlap["chunk"]:
            return
        hi, self._pending_hi = self._pending_hi, lo
        params = [p for p in ar.params_between(lo, hi) if ar.has_grad[id(p)] and id(p) not in self._stepped]
        if not params:
            return
        ops.LnReduceQueue.flush_all()                       # deferred LayerNorm gamma/beta gradients
        st = ops.opt_stream(ar.device)
        st.wait_stream(torch.cuda.current_stream())         # dgrad chain + flushed reductions
        st.wait_stream(ops.side_stream(ar.device))          # weight gradients
        with ops.on_stream(st, "opt"):
            self._apply(ar, params)
        self._stepped.update(id(p) for p in params)

    def _on_bucket(self, ar: Arena, ranges, handles, owed_scale: float = 1.0) -> None:
        # DDP: the bucket's all-reduce has been issued; the update waits for it on the optimizer stream
        params = [p for a, b in ranges for p in ar.params_between(a, b)
                  if ar.has_grad[id(p)] and id(p) not in self._stepped]
        if not params or not ar.flat.is_cuda:
            return
        st = ops.opt_stream(ar.device)
        st.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(st):
            for h in handles:
                h.wait()
        with ops.on_stream(st, "opt"):
            self._apply(ar, params, owed_scale)
        self._stepped.update(id(p) for p in params)

    # ------------------------------------------------------------------ the torch.optim-style entry point
    def flush(self):
        """Apply a deferred optimizer tail now (in stream order); settle the step counts of a guarded step.  No-op otherwise."""
        self._reconcile()
        ar = self._arena
        if ar is not None and ar.__dict__.get("_opt_tail") is not None:
            ar._opt_tail.flush()

    def _tail_bounds(self, ar: Arena):
        """Arena offsets that cut the deferred tail into chunks: [BertLayer 1, BertLayer 4, BertLayer 8, behind the last
        BertLayer]; None when the model has no such layers (nothing is deferred then)."""
        key = id(ar)
        cached = self.__dict__.get("_tail_cache")
        if cached is not None and cached[0] == key:
            return cached[1]
        first = {}
        last_enc = 0
        for name, p in zip(ar.names, ar.params):
            k = name.find("encoder.layer.")
            if k >= 0:
                i = int(name[k + 14:].split(".")[0])
                o = ar.offset[id(p)]
                first[i] = min(first.get(i, o), o)
                last_enc = max(last_enc, o + (p.numel() + ALIGN - 1) // ALIGN * ALIGN)
        bounds = None
        if len(first) >= 2 and all(first[i] < first[i + 1] for i in range(len(first) - 1)):
            n = len(first)
            cuts = sorted({1, min(4, n - 1), min(8, n - 1)} - {0})
            bounds = [first[c] for c in cuts] + [last_enc]
        self._tail_cache = (key, bounds)
        return bounds

    def _guarded_sweep(self, ar: Arena, plan) -> None:
        """Norm of the step's live gradients, clip coefficient and skip flag on the device, then the sweep that obeys them: all on
        the current stream, no host sync.  The runs include the ALIGN padding of the gradient arena, which is allocated zeroed and
        never written.  Every rank of a data-parallel run reads the same reduced bytes, so all ranks clip and skip alike."""
        ws = self._guard_buffers(ar)
        steps = ar.steps
        for k, (lo, hi, _) in enumerate(plan):
            ops.grad_sumsq(ar.grad[lo:hi], ws["partial"], accumulate=k > 0)
        ops.grad_norm_finish(ws["partial"], self.grad_scale, self.max_grad_norm or 0.0, self.skip_nonfinite, ws["out"], ws["flags"])
        guard, hyper = (ws["out"][1:], ws["flags"][:1]), self._hyper()
        for lo, hi, ids in plan:
            self._launch(ar, lo, hi, steps[ids[0]] + 1, hyper, guard)
        if self.skip_nonfinite:
            # (the pinned word is free: _state() has waited for the previous step's copy)
            ws["host"].copy_(guard[1], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream())
            self._guard_pending = (ar, ev, tuple(id(p) for p in ar._marked))

    @torch.no_grad()
    def step(self):
        ar = self._state()
        self.flush()                     # (a tail no forward pass has picked up: apply it before this step's update)
        if self._overlap is None:
            # the set of parameters with a gradient takes two values in pre-training (seq2seq / bidirectional head):
            # the contiguous runs are planned once per set, not rebuilt from 582 parameters every step
            key = ar._published
            plan = self.__dict__.setdefault("_plans", {}).get(key) if key is not None else None
            if plan is None:
                params = [p for p in ar.params if ar.has_grad[id(p)]]
                plan = self._plan_runs(ar, params)
                if key is not None and len(self._plans) < 16:
                    self._plans[key] = plan
            steps = ar.steps
            if not all(steps[ids[0]] == steps[i] for _, _, ids in plan for i in ids):
                # step counts inside a planned run have drifted apart (a parameter that belongs to several sets, a
                # resumed checkpoint): plan again for the current counts
                plan = self._plan_runs(ar, [p for p in ar.params if ar.has_grad[id(p)]])
                if key is not None:
                    self._plans[key] = plan
            hyper = self._hyper()
            if self._guarded and plan:
                self._guarded_sweep(ar, plan)
                plan = ()
            bounds = self._tail_bounds(ar) if (self.defer_tail and ar.flat.is_cuda) else None
            tail = []                    # (lo, hi, step) pieces above the split, in arena order
            for lo, hi, ids in plan:
                st = steps[ids[0]]
                if bounds is not None and hi > bounds[0]:
                    cut = max(lo, bounds[0])
                    tail.append((cut, hi, st))
                    hi = cut
                if hi > lo:
                    self._launch(ar, lo, hi, st + 1, hyper)
            if tail:
                edges = bounds + [ar.total]
                chunks = []
                for c in range(len(edges) - 1):
                    a, b = edges[c], edges[c + 1]
                    runs = [(max(lo, a), min(hi, b), st) for lo, hi, st in tail if min(hi, b) > max(lo, a)]
                    if runs:
                        chunks.append(dict(lo=a, runs=runs, event=None, waited=False))
                ar.__dict__["_opt_tail"] = _OptTail(self, ar, chunks)
        else:
            self._apply(ar, [p for p in ar.params if ar.has_grad[id(p)] and id(p) not in self._stepped])
            torch.cuda.current_stream().wait_stream(ops.opt_stream(ar.device))
            self._stepped = set()
        ar.bump_steps()
        ar.note_params_written_by_kernel()
        ar.note_grads_consumed()
