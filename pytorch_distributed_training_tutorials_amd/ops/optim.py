"""Fused SGD / Adam(W) optimizers on native kernels (csrc/kernels/optim.hip).

Reference: ``torch.optim.SGD(model.parameters(), lr=1e-2)`` ddp_gpus.py:82,
SGD lr=1e-3 NB03:534,977 (161 ResNet tensors over two devices), and
``torch.optim.Adam(lr=1e-3)`` NB01:287.

Semantics match ``torch.optim.SGD`` / ``Adam`` / ``AdamW`` (same hyper-parameter
names, per-parameter state keys ``momentum_buffer`` / ``exp_avg`` /
``exp_avg_sq``) so state_dicts interchange. Execution:
  * parameters that are back-to-back views of one flat buffer (FlatParameters,
    or DDP's grad buckets on the gradient side) -> ONE flat launch;
  * otherwise -> multi-tensor launches of <= 32 tensors each;
  * the "first momentum step" and Adam's bias-correction step count live in
    device int32 counters, so ``step()`` is hipGraph-capturable (no host reads);
    one counter per cohort (:class:`_StepCounters`), so every parameter counts
    its own updates as in ``torch.optim`` and a group may mix dtypes;
  * CPU parameters use eager ATen math (plumbing tests);
  * a gradient-clipping coefficient (:mod:`.clip`, fused mode) can be armed for the next
    ``step()``: a device float per device that the kernels multiply into the gradient as
    they load it, so the clipped gradients are never written;
  * a learning-rate schedule (:mod:`.lr_scheduler`) can be bound: a device float per
    (group, device) that the kernels load in place of ``group["lr"]``, so the learning rate
    moves inside a captured step.
"""
from __future__ import annotations

import torch
from torch.optim import Optimizer

from .._ext import native
from .flat import contiguous_span, dense_like, same_layout


def _split_by_device(params, with_grad_only: bool = True):
    out = {}
    for p in params:
        if with_grad_only and p.grad is None:
            continue
        out.setdefault((p.device, p.dtype), []).append(p)
    return out


def _bf16_shadow(p: torch.Tensor) -> torch.Tensor:
    sh = getattr(p, "_ptdt_bf16", None)
    if sh is None or sh.shape != p.shape or sh.stride() != p.stride() or sh.device != p.device:
        sh = torch.empty_like(p, dtype=torch.bfloat16)
        p._ptdt_bf16 = sh
    return sh


class _StepCounters:
    """Device step counters, one per cohort: the parameters of one (group, device, dtype)
    that have been updated in exactly the same steps. Parameters that start together stay
    one cohort (one counter, one launch); a parameter that gets its first gradient later,
    or misses a step, counts on its own from then on."""

    def __init__(self):
        self.counters: dict = {}  # cohort id -> int32[1] tensor on the cohort's device
        self._of: dict = {}       # parameter -> cohort id
        self._size: dict = {}     # cohort id -> number of member parameters

    def _add(self, counter, members):
        cid = len(self.counters)
        self.counters[cid] = counter
        self._size[cid] = len(members)
        for p in members:
            self._of[p] = cid
        return counter

    def count(self, p):
        cid = self._of.get(p)
        return None if cid is None else self.counters[cid]

    def cohorts(self, ps, initial):
        """Partition ``ps`` (the parameters of one (device, dtype) updated in this step) into
        ``[(counter, members)]``. New parameters join one cohort per ``initial(p)`` value; a
        cohort only partly in ``ps`` is split, the present part taking a copy of the count."""
        old, new = {}, {}
        for p in ps:
            cid = self._of.get(p)
            if cid is None:
                new.setdefault(initial(p), []).append(p)
            else:
                old.setdefault(cid, []).append(p)
        out = []
        for cid, members in old.items():
            counter = self.counters[cid]
            if len(members) != self._size[cid]:
                self._size[cid] -= len(members)
                counter = self._add(counter.clone(), members)
            out.append((counter, members))
        for value, members in new.items():
            counter = torch.full((1,), value, dtype=torch.int32, device=members[0].device)
            out.append((self._add(counter, members), members))
        return out


class _GradCoef:
    """Fused gradient clipping: :meth:`arm_grad_coef` hands the next ``step()`` one float32
    tensor per device, the clip coefficient; that step multiplies every gradient by it where
    ``maximize``'s sign is applied (``p.grad`` itself keeps the unclipped values) and disarms.
    A ``step()`` that was not armed is unchanged."""

    _grad_coef: dict | None = None

    def arm_grad_coef(self, coefs: dict) -> None:
        """``coefs``: {torch.device: 1-element float32 tensor on that device}."""
        self._grad_coef = dict(coefs)

    def _take_grad_coef(self) -> dict:
        coefs, self._grad_coef = self._grad_coef, None
        return coefs or {}


class _DeviceLr:
    """Device learning rates: while a scheduler of :mod:`.lr_scheduler` is bound, ``step()`` hands
    the update kernels of each (group, device) that group's slot of the scheduler's ``lr`` buffer on
    that device, and the kernels use it in place of ``group["lr"]`` (which stays a Python float; the
    scheduler refreshes it at its host-read points). CPU parameters keep using ``group["lr"]``. An
    optimizer with no scheduler bound is unchanged."""

    _lr_scheduler = None
    _lr_views: dict | None = None

    def bind_lr_scheduler(self, scheduler, views: dict) -> None:
        """``views``: {torch.device: [one 1-element float32 view per parameter group]}. A scheduler
        bound earlier is released (its ``step()`` then raises)."""
        old = self._lr_scheduler
        if old is not None and old is not scheduler:
            old._released()
        self._lr_scheduler = scheduler
        self._lr_views = dict(views)

    def _lr_dev(self, gi: int, device):
        if self._lr_views is None or device.type != "cuda":
            return None
        views = self._lr_views.get(device)
        if views is None or gi >= len(views):
            raise RuntimeError(f"the bound learning-rate scheduler has no buffer for group {gi} on {device}: "
                               "parameters or groups were added after it was constructed")
        return views[gi]


class FusedSGD(_GradCoef, _DeviceLr, Optimizer):
    """``bf16_shadow=True``: every f32 GPU parameter also gets a bf16 copy of its
    updated value, written by the same update kernel (``p._ptdt_bf16``); under bf16
    autocast :func:`ops.conv.cast_weight` uses it instead of casting the weight in
    every forward (one cast kernel per conv per step)."""

    def __init__(self, params, lr: float = 1e-3, momentum: float = 0.0, dampening: float = 0.0,
                 weight_decay: float = 0.0, nesterov: bool = False, maximize: bool = False,
                 bf16_shadow: bool = False):
        if lr < 0.0:
            raise ValueError(f"Invalid learning rate: {lr}")
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        defaults = dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay,
                        nesterov=nesterov, maximize=maximize)
        super().__init__(params, defaults)
        self._cohorts = _StepCounters()
        self.bf16_shadow = bf16_shadow

    @property
    def _counters(self) -> dict:
        """The live device counters (a counter reads 0 until its cohort's first update)."""
        return self._cohorts.counters

    def _started(self, p) -> int:
        """1 when a parameter new to this optimizer object already has a (loaded) momentum buffer."""
        return int("momentum_buffer" in self.state[p])

    def _momentum_buffers(self, gi, ps):
        """Per-parameter momentum buffers; for flat parameter spans they are views
        of one flat buffer so the update stays a single launch."""
        if all("momentum_buffer" in self.state[p] for p in ps):
            return [self.state[p]["momentum_buffer"] for p in ps]
        total = sum(p.numel() for p in ps)
        flat = torch.zeros(total, device=ps[0].device, dtype=torch.float32)
        out, off = [], 0
        for p in ps:
            v = dense_like(flat[off:off + p.numel()], p)
            old = self.state[p].get("momentum_buffer")
            if old is not None:
                v.copy_(old)
            self.state[p]["momentum_buffer"] = v
            out.append(v)
            off += p.numel()
        return out

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        coefs = self._take_grad_coef()
        for gi, group in enumerate(self.param_groups):
            lr, mu, damp, wd, nest = (group["lr"], group["momentum"], group["dampening"],
                                      group["weight_decay"], group["nesterov"])
            gscale = -1.0 if group["maximize"] else 1.0
            for (device, dtype), ps in _split_by_device(group["params"]).items():
                gcoef = coefs.get(device)
                if device.type != "cuda":
                    self._cpu_step(ps, lr, mu, damp, wd, nest, gscale, gcoef)
                    continue
                lr_dev = self._lr_dev(gi, device)
                # before creating buffers: a parameter's "first step" is decided here
                for step, cps in self._cohorts.cohorts(ps, self._started):
                    self._gpu_step(gi, cps, dtype, step, lr, mu, damp, wd, nest, gscale, gcoef, lr_dev)
        return loss

    def _gpu_step(self, gi, ps, dtype, step, lr, mu, damp, wd, nest, gscale, gcoef=None, lr_dev=None):
        grads = [p.grad for p in ps]
        moms = self._momentum_buffers(gi, ps) if mu != 0.0 else []
        C = native()
        pflat = contiguous_span([p.data for p in ps])
        gflat = contiguous_span(grads)
        mflat = contiguous_span(moms) if moms else None
        pdata = [p.data for p in ps]
        aligned = same_layout(pdata, grads) and (not moms or same_layout(pdata, moms))
        shadows = [_bf16_shadow(p) for p in ps] if (self.bf16_shadow and dtype == torch.float32) else []
        if (dtype == torch.float32 and aligned and pflat is not None and gflat is not None
                and (not moms or mflat is not None) and not shadows):
            # one launch for the whole cohort (also increments the device counter)
            C.sgd_flat_(pflat, gflat, mflat, step, lr, mu, damp, wd, nest, gscale, gcoef, lr_dev)
        else:
            C.sgd_multi_(pdata, grads, moms, step, lr, mu, damp, wd, nest, gscale, shadows, gcoef, lr_dev)
            step.add_(1)
        for p in ps if shadows else ():
            p._ptdt_bf16_version = p._version  # the shadow is current until p changes

    def _cpu_step(self, ps, lr, mu, damp, wd, nest, gscale, gcoef=None):
        for p in ps:
            d = p.grad * gscale
            if gcoef is not None:
                d = d * gcoef
            if wd != 0:
                d = d.add(p, alpha=wd)
            if mu != 0:
                buf = self.state[p].get("momentum_buffer")
                if buf is None:
                    buf = d.clone()
                    self.state[p]["momentum_buffer"] = buf
                else:
                    buf.mul_(mu).add_(d, alpha=1 - damp)
                d = d.add(buf, alpha=mu) if nest else buf
            p.add_(d, alpha=-lr)


class FusedAdam(_GradCoef, _DeviceLr, Optimizer):
    """Adam / AdamW (``decoupled_weight_decay=True``) with fp32 state."""

    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 0.0, decoupled_weight_decay: bool = False, maximize: bool = False):
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay,
                        decoupled_weight_decay=decoupled_weight_decay, maximize=maximize)
        super().__init__(params, defaults)
        self._cohorts = _StepCounters()

    def _loaded_step(self, p) -> int:
        """Updates a parameter new to this optimizer object already has behind it (a loaded state)."""
        return int(float(self.state[p].get("step", 0)))

    def _state_lists(self, ps):
        need = [p for p in ps if "exp_avg" not in self.state[p]]
        if need:
            total = sum(p.numel() for p in need)
            fm = torch.zeros(total, device=need[0].device, dtype=torch.float32)
            fv = torch.zeros(total, device=need[0].device, dtype=torch.float32)
            off = 0
            for p in need:
                self.state[p]["exp_avg"] = dense_like(fm[off:off + p.numel()], p)
                self.state[p]["exp_avg_sq"] = dense_like(fv[off:off + p.numel()], p)
                off += p.numel()
        return [self.state[p]["exp_avg"] for p in ps], [self.state[p]["exp_avg_sq"] for p in ps]

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        coefs = self._take_grad_coef()
        for gi, group in enumerate(self.param_groups):
            b1, b2 = group["betas"]
            gscale = -1.0 if group["maximize"] else 1.0
            for (device, dtype), sub in _split_by_device(group["params"]).items():
                gcoef = coefs.get(device)
                lr_dev = self._lr_dev(gi, device)
                for step, ps in self._cohorts.cohorts(sub, self._loaded_step):
                    step.add_(1)
                    ms, vs = self._state_lists(ps)
                    if device.type != "cuda":
                        self._cpu_step(ps, ms, vs, step, group, gscale, gcoef)
                        continue
                    C = native()
                    grads = [p.grad for p in ps]
                    pflat, gflat = contiguous_span([p.data for p in ps]), contiguous_span(grads)
                    mflat, vflat = contiguous_span(ms), contiguous_span(vs)
                    pdata = [p.data for p in ps]
                    aligned = same_layout(pdata, grads) and same_layout(pdata, ms) and same_layout(pdata, vs)
                    if dtype == torch.float32 and aligned and None not in (pflat, gflat, mflat, vflat):
                        C.adam_flat_(pflat, gflat, mflat, vflat, step, group["lr"], b1, b2, group["eps"],
                                     group["weight_decay"], group["decoupled_weight_decay"], gscale, gcoef, lr_dev)
                    else:
                        C.adam_multi_(pdata, grads, ms, vs, step, group["lr"], b1, b2, group["eps"],
                                      group["weight_decay"], group["decoupled_weight_decay"], gscale, gcoef, lr_dev)
        return loss

    def state_dict(self):
        """torch.optim.Adam layout: per parameter ``exp_avg``, ``exp_avg_sq`` and the
        bias-correction ``step`` (a float32 scalar tensor) -- the kernels keep the step
        in one device counter per cohort; it is copied into the state here."""
        for group in self.param_groups:
            for p in group["params"]:
                if p in self.state:
                    step = self._cohorts.count(p)
                    self.state[p]["step"] = torch.tensor(float(step.item()) if step is not None
                                                         else float(self._loaded_step(p)))
        return super().state_dict()

    def load_state_dict(self, state_dict):
        """Restores moments and the bias-correction step (a state_dict of this class or of
        torch.optim.Adam/AdamW), so a resumed run continues the same trajectory."""
        super().load_state_dict(state_dict)
        self._cohorts = _StepCounters()  # the next step() starts each parameter at its loaded ``step``
        for group in self.param_groups:
            for ps in _split_by_device(group["params"], False).values():
                # the kernels need the flat-state layout: pop every loaded moment of the split first,
                # then re-home them in ONE flat allocation (per-parameter allocations would leave the
                # group without a contiguous span and every later step on the slower multi-tensor path)
                loaded = {}
                for p in ps:
                    st = self.state.get(p, {})
                    if "exp_avg" in st:
                        loaded[p] = (st.pop("exp_avg"), st.pop("exp_avg_sq"))
                if loaded:
                    ms, vs = self._state_lists(ps)
                    for p, m, v in zip(ps, ms, vs):
                        if p in loaded:
                            m.copy_(loaded[p][0])
                            v.copy_(loaded[p][1])

    @staticmethod
    def _cpu_step(ps, ms, vs, step, group, gscale, gcoef=None):
        t = float(step.item())
        b1, b2 = group["betas"]
        lr, eps, wd = group["lr"], group["eps"], group["weight_decay"]
        bc1 = 1 - b1 ** t
        bc2s = (1 - b2 ** t) ** 0.5
        for p, m, v in zip(ps, ms, vs):
            g = p.grad.float() * gscale
            if gcoef is not None:
                g = g * gcoef
            if group["decoupled_weight_decay"]:
                p.mul_(1 - lr * wd)
            elif wd != 0:
                g = g.add(p, alpha=wd)
            m.mul_(b1).add_(g, alpha=1 - b1)
            v.mul_(b2).addcmul_(g, g, value=1 - b2)
            denom = v.sqrt() / bc2s + eps
            p.addcdiv_(m, denom, value=-lr / bc1)
