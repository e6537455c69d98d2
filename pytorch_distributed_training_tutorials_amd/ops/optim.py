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
    moves inside a captured step;
  * :class:`FusedLARS` / :class:`FusedLAMB` put a layer-wise trust ratio on top of the two
    (csrc/kernels/layerwise.hip): norms, ratio and update stay on the device, so the step
    remains capturable; :func:`layerwise_param_groups` builds their usual two groups.
"""
from __future__ import annotations

from collections import namedtuple

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


# What one update launches over: the parameters of one (group, device, dtype) that share a step counter
# (None where the class keeps none: FusedSGD on the CPU), with the operands step() looked up for them.
_Cohort = namedtuple("_Cohort", "gi group device dtype params step gcoef lr_dev")


def _gscale(group) -> float:
    return -1.0 if group["maximize"] else 1.0


def _effective(c, g):
    """The gradient the CPU updates see: ``maximize``'s sign and the armed clip coefficient applied."""
    g = g * _gscale(c.group)
    return g if c.gcoef is None else g * c.gcoef


# The scalars the SGD-shaped and the Adam-shaped bindings share, in the bindings' order: they go by position
# (wrappers around the four older bindings read operands by index), the rest of lars_multi_ / lamb_multi_ by keyword.
def _sgd_hyper(group) -> tuple:
    return (group["lr"], group["momentum"], group["dampening"], group["weight_decay"], group["nesterov"],
            _gscale(group))


def _adam_hyper(group) -> tuple:
    return (group["lr"], *group["betas"], group["eps"], group["weight_decay"])


class _FusedOptimizer(_GradCoef, _DeviceLr, Optimizer):
    """The one ``step()`` of the fused optimizers: closure, grad coefficients, then per group and
    (device, dtype) the operands and the cohorts, each handed to the class's CPU or GPU update.
    Subclasses say what a new parameter's count starts at (:meth:`_initial_count`), whether CPU
    parameters are counted (``_counts_cpu``), and supply :meth:`_gpu_update` / :meth:`_cpu_update`."""

    _counts_cpu = True

    def __init__(self, params, defaults):
        super().__init__(params, defaults)
        self._cohorts = _StepCounters()

    @property
    def _counters(self) -> dict:
        """The live device counters (a counter reads 0 until its cohort's first update)."""
        return self._cohorts.counters

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        coefs = self._take_grad_coef()
        for gi, group in enumerate(self.param_groups):
            for (device, dtype), ps in _split_by_device(group["params"]).items():
                gcoef, lr_dev = coefs.get(device), self._lr_dev(gi, device)
                on_gpu = device.type == "cuda"
                update = self._gpu_update if on_gpu else self._cpu_update
                # before any state buffer is created: a parameter's first step is decided here
                counted = on_gpu or self._counts_cpu
                for step, cps in self._cohorts.cohorts(ps, self._initial_count) if counted else [(None, ps)]:
                    update(_Cohort(gi, group, device, dtype, cps, step, gcoef, lr_dev))
        return loss


class FusedSGD(_FusedOptimizer):
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
        self.bf16_shadow = bf16_shadow

    _counts_cpu = False  # on the CPU the first step is decided by the presence of ``momentum_buffer``

    def _initial_count(self, p) -> int:
        """1 when a parameter new to this optimizer object already has a (loaded) momentum buffer."""
        return int("momentum_buffer" in self.state[p])

    def _momentum_buffers(self, ps):
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

    def _gpu_update(self, c):
        ps = c.params
        grads = [p.grad for p in ps]
        moms = self._momentum_buffers(ps) if c.group["momentum"] != 0.0 else []
        shadows = [_bf16_shadow(p) for p in ps] if (self.bf16_shadow and c.dtype == torch.float32) else []
        self._launch(c, grads, moms, shadows)
        for p in ps if shadows else ():
            p._ptdt_bf16_version = p._version  # the shadow is current until p changes

    def _launch(self, c, grads, moms, shadows):
        """One flat launch when the cohort is one aligned f32 span (it also advances the counter),
        else the multi-tensor form, the counter advanced after it."""
        pdata = [p.data for p in c.params]
        hyper = _sgd_hyper(c.group)
        if c.dtype == torch.float32 and not shadows and same_layout(pdata, grads) and (
                not moms or same_layout(pdata, moms)):
            pflat, gflat = contiguous_span(pdata), contiguous_span(grads)
            mflat = contiguous_span(moms) if moms else None
            if pflat is not None and gflat is not None and (not moms or mflat is not None):
                return native().sgd_flat_(pflat, gflat, mflat, c.step, *hyper, c.gcoef, c.lr_dev)
        native().sgd_multi_(pdata, grads, moms, c.step, *hyper, shadows, c.gcoef, c.lr_dev)
        c.step.add_(1)

    def _cpu_ratio(self, group, p, g):
        """The factor on the decayed gradient before the momentum step: none for plain SGD."""
        return None

    def _cpu_update(self, c):
        group = c.group
        lr, mu, damp, wd = group["lr"], group["momentum"], group["dampening"], group["weight_decay"]
        for p in c.params:
            g = _effective(c, p.grad)
            ratio = self._cpu_ratio(group, p, g)
            d = g.add(p, alpha=wd) if wd != 0 else g
            if ratio is not None:
                d = d * ratio.to(d.dtype)
            if mu != 0:
                buf = self.state[p].get("momentum_buffer")
                if buf is None:
                    buf = d.clone()
                    self.state[p]["momentum_buffer"] = buf
                else:
                    buf.mul_(mu).add_(d, alpha=1 - damp)
                d = d.add(buf, alpha=mu) if group["nesterov"] else buf
            p.add_(d, alpha=-lr)


class FusedAdam(_FusedOptimizer):
    """Adam / AdamW (``decoupled_weight_decay=True``) with fp32 state."""

    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 0.0, decoupled_weight_decay: bool = False, maximize: bool = False):
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay,
                        decoupled_weight_decay=decoupled_weight_decay, maximize=maximize)
        super().__init__(params, defaults)

    def _initial_count(self, p) -> int:
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

    def _advance(self, c):
        """Counts this update (CPU and GPU cohorts alike, ahead of the update), then the moments."""
        c.step.add_(1)
        return self._state_lists(c.params)

    def _gpu_update(self, c):
        ms, vs = self._advance(c)
        self._launch(c, [p.grad for p in c.params], ms, vs)

    def _launch(self, c, grads, ms, vs):
        """One flat launch when parameters, gradients and moments are aligned f32 spans, else multi-tensor."""
        pdata = [p.data for p in c.params]
        tail = (*_adam_hyper(c.group), c.group["decoupled_weight_decay"], _gscale(c.group), c.gcoef, c.lr_dev)
        if c.dtype == torch.float32 and all(same_layout(pdata, ts) for ts in (grads, ms, vs)):
            flat = [contiguous_span(ts) for ts in (pdata, grads, ms, vs)]
            if all(t is not None for t in flat):
                return native().adam_flat_(*flat, c.step, *tail)
        native().adam_multi_(pdata, grads, ms, vs, c.step, *tail)

    def state_dict(self):
        """torch.optim.Adam layout: per parameter ``exp_avg``, ``exp_avg_sq`` and the
        bias-correction ``step`` (a float32 scalar tensor) -- the kernels keep the step
        in one device counter per cohort; it is copied into the state here."""
        for group in self.param_groups:
            for p in group["params"]:
                if p in self.state:
                    step = self._cohorts.count(p)
                    self.state[p]["step"] = torch.tensor(float(step.item()) if step is not None
                                                         else float(self._initial_count(p)))
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

    def _cpu_update(self, c):
        ms, vs = self._advance(c)
        group = c.group
        b1, b2 = group["betas"]
        t = float(c.step.item())
        correct = group.get("bias_correction", True)
        bc1 = 1 - b1 ** t if correct else 1.0
        bc2s = (1 - b2 ** t) ** 0.5 if correct else 1.0
        for p, m, v in zip(c.params, ms, vs):
            g = self._cpu_decay(group, p, _effective(c, p.grad.float()))
            m.mul_(b1).add_(g, alpha=1 - b1)
            v.mul_(b2).addcmul_(g, g, value=1 - b2)
            self._cpu_apply(group, p, m, v.sqrt() / bc2s + group["eps"], bc1)

    def _cpu_decay(self, group, p, g):
        """Adam's weight decay, ahead of the moments: on the parameter (AdamW) or into the gradient."""
        if group["decoupled_weight_decay"]:
            p.mul_(1 - group["lr"] * group["weight_decay"])
        elif group["weight_decay"] != 0:
            g = g.add(p, alpha=group["weight_decay"])
        return g

    def _cpu_apply(self, group, p, m, denom, bc1):
        p.addcdiv_(m, denom, value=-group["lr"] / bc1)


# ---------------------------------------------------------------------------- layer-wise rates
_CHUNK = 4096  # kChunk


class _TrustPlan:
    """Launch plan of one adapted cohort: the workspace (two float32 slots per 4096-element chunk)
    and the record ``rec[3, T]`` = (ratio, ||p||, ||g'|| or ||u||) per tensor, valid while the
    parameters and gradients stay where ``key`` saw them."""

    def __init__(self, ps, key):
        self.params = list(ps)
        self.key = key
        device = ps[0].device
        chunks = sum(-(-p.numel() // _CHUNK) for p in ps)
        self.ws = torch.empty(2 * max(chunks, 1), dtype=torch.float32, device=device)
        self.rec = torch.ones(3, len(ps), dtype=torch.float32, device=device)


class _TrustRatios:
    """Launch plans and the trust-ratio record of the layer-wise optimizers. A plan per (group,
    device, dtype, cohort) is cached and keyed on the tensors' (data_ptr, numel); it is built on the
    first eager step -- :class:`utils.graphs.GraphedStep`'s warm-up creates it before capture -- and
    rebuilt when a parameter or a gradient moves. After that ``step()`` allocates nothing."""

    def _init_trust(self):
        self._trust_plans: dict = {}  # (group index, id of the cohort's counter) -> (counter, _TrustPlan)
        self._trust_cpu: dict = {}    # CPU parameters: parameter -> (ratio, w, n)

    def _trust_plan(self, c, grads) -> _TrustPlan:
        ps, at = c.params, (c.gi, id(c.step))
        key = [(p.data_ptr(), g.data_ptr(), p.numel()) for p, g in zip(ps, grads)]
        held = self._trust_plans.get(at)
        if held is not None and held[1].key == key:
            return held[1]
        plan = _TrustPlan(ps, key)
        mine = set(ps)  # a parameter reports through one plan: drop the plans it has left
        self._trust_plans = {k: v for k, v in self._trust_plans.items() if mine.isdisjoint(v[1].params)}
        self._trust_plans[at] = (c.step, plan)  # holding the counter keeps its id unique
        return plan

    def _record_cpu(self, p, ratio, w, n):
        self._trust_cpu[p] = (float(ratio), float(w), float(n))
        return ratio

    def trust_ratios(self) -> dict:
        """``{parameter: (ratio, w, n)}`` as the latest update of each parameter computed them:
        ``w = ||p||`` before that update, ``n = ||g'||`` (LARS) or ``||u||`` (LAMB). Parameters of
        unadapted LARS groups (``trust_coefficient=0``) take plain SGD and are not listed. Reads the
        device records back, so call it outside the step (and outside a capture): for logging."""
        out = {}
        for _, plan in self._trust_plans.values():
            rec = plan.rec.cpu()
            for i, p in enumerate(plan.params):
                out[p] = (float(rec[0, i]), float(rec[1, i]), float(rec[2, i]))
        out.update(self._trust_cpu)
        return out

    def _restore_group_keys(self, before) -> None:
        """After ``load_state_dict``: a checkpoint of the parent class has no layer-wise group keys;
        those keep the values this optimizer was constructed with."""
        for group, old in zip(self.param_groups, before):
            for k, v in old.items():
                group.setdefault(k, v)


def _norm64(x: torch.Tensor) -> torch.Tensor:
    return torch.linalg.vector_norm(x.double())


class FusedLARS(_TrustRatios, FusedSGD):
    """LARS (You et al. 2017, as apex LARC / lightning-bolts scale it) on :class:`FusedSGD`: with the
    effective gradient ``g' = gscale * gcoef * g``, ``w = ||p||`` and ``n = ||g'||``, every tensor's
    decayed gradient is scaled by ``ratio = trust_coefficient * w / (n + weight_decay * w + eps)``
    (1 when ``w`` or ``n`` is not positive) before the momentum-SGD step. Three capturable launches
    per 32 tensors: per-chunk partial sums, a fixed-order float64 finalise per tensor, the update
    (csrc/kernels/layerwise.hip); the ratios stay on the device (:meth:`trust_ratios` reads them).

    A group with ``trust_coefficient=0`` is not adapted: it takes exactly :class:`FusedSGD`'s launches.
    Adapted groups always take the multi-tensor form, even when their parameters form one flat span:
    the flat kernels have no tensor index. State and ``state_dict`` layout are ``FusedSGD``'s, so
    checkpoints interchange; fused clipping, the schedulers and ``bf16_shadow`` work as there."""

    def __init__(self, params, lr: float = 1e-3, momentum: float = 0.0, dampening: float = 0.0,
                 weight_decay: float = 0.0, nesterov: bool = False, maximize: bool = False,
                 bf16_shadow: bool = False, trust_coefficient: float = 1e-3, eps: float = 1e-8):
        if trust_coefficient < 0.0:
            raise ValueError(f"Invalid trust_coefficient: {trust_coefficient}")
        if eps < 0.0:
            raise ValueError(f"Invalid eps: {eps}")
        super().__init__(params, lr, momentum, dampening, weight_decay, nesterov, maximize, bf16_shadow)
        self.defaults.update(trust_coefficient=trust_coefficient, eps=eps)
        for group in self.param_groups:
            group.setdefault("trust_coefficient", trust_coefficient)
            group.setdefault("eps", eps)
            if group["trust_coefficient"] < 0.0 or group["eps"] < 0.0:
                raise ValueError("trust_coefficient and eps must not be negative")
        self._init_trust()

    def load_state_dict(self, state_dict):
        before = [{k: g[k] for k in ("trust_coefficient", "eps")} for g in self.param_groups]
        super().load_state_dict(state_dict)
        self._restore_group_keys(before)

    def _launch(self, c, grads, moms, shadows):
        group = c.group
        if group["trust_coefficient"] == 0:
            return super()._launch(c, grads, moms, shadows)
        plan = self._trust_plan(c, grads)
        native().lars_multi_([p.data for p in c.params], grads, moms, c.step, *_sgd_hyper(group),
                             trust_coefficient=group["trust_coefficient"], eps=group["eps"], shadows=shadows,
                             ws=plan.ws, rec=plan.rec, gcoef=c.gcoef, lr_dev=c.lr_dev)
        c.step.add_(1)

    def _cpu_ratio(self, group, p, g):
        tc, wd = group["trust_coefficient"], group["weight_decay"]
        if tc == 0:
            return None
        w, n = _norm64(p), _norm64(g)
        ratio = tc * w / (n + wd * w + group["eps"]) if (w > 0 and n > 0) else torch.ones((), dtype=torch.float64)
        return self._record_cpu(p, ratio, w, n)


class FusedLAMB(_TrustRatios, FusedAdam):
    """LAMB (You et al. 2019; apex ``FusedLAMB`` without its built-in global clip, which
    :class:`ops.clip.GradClipper` provides) on :class:`FusedAdam`'s state: Adam moments of the
    effective gradient, ``u = (m / bc1) / (sqrt(v) / sqrt(bc2) + eps) + weight_decay * p``,
    ``ratio = ||p|| / ||u||`` (1 when a norm is not positive, or ``adapt=False``) and
    ``p -= lr * ratio * u``. Three capturable launches per 32 tensors (csrc/kernels/layerwise.hip):
    the moment update with per-chunk partial sums, a fixed-order float64 finalise per tensor, the
    update, which recomputes ``u`` from the stored moments.

    Every GPU group takes the multi-tensor form, even when its parameters form one flat span: the
    flat kernels have no tensor index. State keys, ``state_dict`` layout and the per-parameter
    ``step`` are ``FusedAdam``'s."""

    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-6,
                 weight_decay: float = 0.0, bias_correction: bool = True, adapt: bool = True,
                 maximize: bool = False):
        if eps < 0.0:
            raise ValueError(f"Invalid eps: {eps}")
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, maximize=maximize)
        self.defaults.update(bias_correction=bias_correction, adapt=adapt)
        for group in self.param_groups:
            group.setdefault("bias_correction", bias_correction)
            group.setdefault("adapt", adapt)
            if group["eps"] < 0.0:
                raise ValueError(f"Invalid eps: {group['eps']}")
        self._init_trust()

    def load_state_dict(self, state_dict):
        before = [{k: g[k] for k in ("bias_correction", "adapt")} for g in self.param_groups]
        super().load_state_dict(state_dict)
        self._restore_group_keys(before)

    def _launch(self, c, grads, ms, vs):
        group = c.group
        plan = self._trust_plan(c, grads)
        native().lamb_multi_([p.data for p in c.params], grads, ms, vs, c.step, *_adam_hyper(group),
                             bias_correction=group["bias_correction"], adapt=group["adapt"],
                             grad_scale=_gscale(group), ws=plan.ws, rec=plan.rec, gcoef=c.gcoef, lr_dev=c.lr_dev)

    def _cpu_decay(self, group, p, g):
        return g  # LAMB decays in the direction, not in the gradient

    def _cpu_apply(self, group, p, m, denom, bc1):
        u = (m / bc1) / denom
        if group["weight_decay"] != 0:
            u = u.add(p, alpha=group["weight_decay"])
        w, n = _norm64(p), _norm64(u)
        ratio = w / n if (group["adapt"] and w > 0 and n > 0) else torch.ones((), dtype=torch.float64)
        self._record_cpu(p, ratio, w, n)
        p.add_(u.to(p.dtype), alpha=-group["lr"] * float(ratio))


def layerwise_param_groups(module: torch.nn.Module, weight_decay: float = 0.0, **adapt_off) -> list:
    """The standard two parameter groups of a layer-wise optimizer: parameters with ``ndim > 1``
    (conv and linear weights) are adapted and decayed with ``weight_decay``; BatchNorm weights and
    all biases (``ndim <= 1``) get ``weight_decay=0`` and the options in ``adapt_off``, which switch
    the adaptation off: ``trust_coefficient=0`` for :class:`FusedLARS` (the default when nothing is
    given), ``adapt=False`` for :class:`FusedLAMB`. Parameters that need no gradient are left out."""
    if not adapt_off:
        adapt_off = {"trust_coefficient": 0.0}
    params = [p for p in module.parameters() if p.requires_grad]
    return [{"params": [p for p in params if p.ndim > 1], "weight_decay": weight_decay},
            {"params": [p for p in params if p.ndim <= 1], "weight_decay": 0.0, **adapt_off}]
