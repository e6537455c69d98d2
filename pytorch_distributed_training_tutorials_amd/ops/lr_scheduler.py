"""Learning-rate schedules for ``FusedSGD`` / ``FusedAdam`` that move inside a captured step
(csrc/kernels/lr_schedule.hip).

A whole-step hipGraph (:class:`utils.graphs.GraphedStep`) replays kernel arguments, so a learning
rate passed as a Python float stays what it was at capture. Here it lives on the device, like the
optimizers' step counters and the clip coefficient: per device one int32 counter ``t`` and one
float32 buffer ``lr[G]`` (a value per parameter group). ``scheduler.step()`` is one single-wave
kernel per device that increments ``t`` and writes ``lr(t)``; the update kernels load their
group's slot. Nothing in ``step()`` reads the host, so it can sit in the captured step after
``optimizer.step()``.

Classes, constructor arguments and call order follow ``torch.optim.lr_scheduler``: construct after
the optimizer, call ``scheduler.step()`` after ``optimizer.step()``; ``lr(0)`` is in force for the
first update. ``ConstantLR``, ``LinearLR``, ``CosineAnnealingLR``, ``StepLR``, ``MultiStepLR``,
``ExponentialLR``, ``PolynomialLR`` evaluate torch's closed forms at the step count; and
``SequentialLR`` chains up to 4 of them at ascending milestones, each evaluated at the time since
its own start. The kernel computes in fp64 and rounds once to float32.

``group["lr"]`` stays a Python float (``optimizer.state_dict()`` keeps torch's layout). With GPU
parameters it is NOT updated by ``step()``: ``get_last_lr()``, ``sync()`` and ``state_dict()`` read
the device (the host cannot count graph replays) and refresh it. **These three read the host and
must stay outside a captured step.** CPU parameters take the host evaluator (:meth:`value_at`,
the same closed forms in Python floats), and ``step()`` writes ``group["lr"]``, as the plumbing
paths elsewhere in ``ops``.

Caps (a program is a by-value kernel argument): 4 segments, 16 milestones per ``MultiStepLR``,
64 parameter groups. Larger programs raise ``ValueError``. Only ``FusedSGD`` / ``FusedAdam`` can be
bound (``TypeError`` otherwise: use ``torch.optim.lr_scheduler`` with torch's optimizers).
"""
from __future__ import annotations

import math

import torch

from .._ext import native
from .optim import FusedAdam, FusedSGD

MAX_SEGMENTS = 4     # kLrMaxSegments
MAX_MILESTONES = 16  # kLrMaxMilestones
MAX_GROUPS = 64      # kLrMaxGroups: one lane of the kernel's wave per parameter group
_INT32_MAX = 2 ** 31 - 1

_KINDS = ("constant", "linear", "cosine", "step", "multistep", "exponential", "polynomial")  # LrKind
_DIVIDES = ("linear", "cosine", "step", "polynomial")  # n is a divisor: >= 1


def _segment(kind: str, n: int = 0, a: float = 0.0, b: float = 0.0, milestones=()) -> dict:
    """One validated segment ``{kind, n, a, b, milestones}`` (see LrKind in kernels.h for the fields)."""
    if kind not in _KINDS:
        raise ValueError(f"unknown schedule kind {kind!r}")
    n = int(n)
    milestones = [int(m) for m in milestones]
    if not 0 <= n <= _INT32_MAX or (kind in _DIVIDES and n < 1):
        raise ValueError(f"{kind} schedule: the iteration count must be a positive int32, got {n}")
    if len(milestones) > MAX_MILESTONES:
        raise ValueError(f"at most {MAX_MILESTONES} milestones per MultiStepLR, got {len(milestones)}")
    if any(m < 0 or m > _INT32_MAX for m in milestones) or any(x > y for x, y in zip(milestones, milestones[1:])):
        raise ValueError(f"milestones must be ascending non-negative int32 values (repeats allowed), got {milestones}")
    return {"kind": kind, "n": n, "a": float(a), "b": float(b), "milestones": milestones}


def _check_program(segments, bounds) -> None:
    if not 1 <= len(segments) <= MAX_SEGMENTS:
        raise ValueError(f"a schedule has 1..{MAX_SEGMENTS} segments, got {len(segments)}")
    if len(bounds) != len(segments) - 1:
        raise ValueError(f"{len(segments)} segments need {len(segments) - 1} milestones, got {len(bounds)}")
    if any(b <= a for a, b in zip([0] + list(bounds), bounds)) or any(b > _INT32_MAX for b in bounds):
        raise ValueError(f"segment milestones must be ascending positive int32 values, got {list(bounds)}")


def _factor(seg: dict, tl: int, base: float) -> float:
    """f(t') of one segment in Python floats (fp64): the specification of the kernel's lr_factor."""
    kind, n, a, b = seg["kind"], seg["n"], seg["a"], seg["b"]
    if kind == "constant":
        return a if tl < n else 1.0
    if kind == "linear":
        return a + (b - a) * min(tl, n) / n
    if kind == "cosine":
        r = a / base if base != 0.0 else 0.0
        return r + (1.0 - r) * (1.0 + math.cos(math.pi * tl / n)) / 2.0
    if kind == "step":
        return a ** (tl // n)
    if kind == "multistep":
        return a ** sum(m <= tl for m in seg["milestones"])
    if kind == "exponential":
        return a ** tl
    return (1.0 - min(tl, n) / n) ** b  # polynomial


def evaluate(segments, bounds, base_lrs, t: int) -> list:
    """The schedule at step ``t`` for every base learning rate, in fp64."""
    k = 0
    while k + 1 < len(segments) and t >= bounds[k]:
        k += 1
    tl = max(0, t - (bounds[k - 1] if k else 0))
    return [base * _factor(segments[k], tl, base) for base in base_lrs]


class LRScheduler:
    """A piecewise schedule bound to a ``FusedSGD`` / ``FusedAdam``. Subclasses only build the
    program; everything else is here.

    Device state, per device that holds parameters of the optimizer: ``counters[device]`` (int32[1])
    and ``lrs[device]`` (float32[G]). ``step()`` launches the schedule kernel once per device and
    reads nothing from the host. ``get_last_lr()``, ``sync()`` and ``state_dict()`` read the device:
    keep them outside a captured step."""

    def __init__(self, optimizer, segments, bounds=(), last_epoch: int = -1):
        if not isinstance(optimizer, (FusedSGD, FusedAdam)):
            raise TypeError("these schedulers keep the learning rate on the device for FusedSGD / FusedAdam; "
                            f"for {type(optimizer).__name__} use torch.optim.lr_scheduler")
        segments, bounds = list(segments), [int(b) for b in bounds]
        _check_program(segments, bounds)
        groups = optimizer.param_groups
        if len(groups) > MAX_GROUPS:
            raise ValueError(f"at most {MAX_GROUPS} parameter groups per scheduler (one launch), got {len(groups)}")
        if last_epoch < -1:
            raise ValueError(f"last_epoch must be >= -1, got {last_epoch}")
        self.optimizer = optimizer
        self.segments, self.bounds = segments, bounds
        for g in groups:  # torch's convention: sub-schedulers of a SequentialLR share the base rates
            g.setdefault("initial_lr", g["lr"])
        self.base_lrs = [float(g["initial_lr"]) for g in groups]
        self._bound = True
        self._allocate(last_epoch + 1)

    # ------------------------------------------------------------ binding
    def _allocate(self, t: int) -> None:
        params = [p for g in self.optimizer.param_groups for p in g["params"]]
        devices = []
        for p in params:
            if p.device.type == "cuda" and p.device not in devices:
                devices.append(p.device)
        self._host = any(p.device.type != "cuda" for p in params) or not devices
        self._t = int(t)  # the host's count: in force only while CPU parameters make step() count here
        G = len(self.base_lrs)
        self.counters = {d: torch.full((1,), int(t), dtype=torch.int32, device=d) for d in devices}
        self.lrs = {d: torch.empty(G, dtype=torch.float32, device=d) for d in devices}
        self._pack()
        self._launch(increment=False)
        self.optimizer.bind_lr_scheduler(self, {d: [lr[i:i + 1] for i in range(G)] for d, lr in self.lrs.items()})
        if self._host:
            self._write_groups(self.value_at(self._t))

    def rebind(self) -> None:
        """Place the device state again, at the current ``t``, after the optimizer's parameters moved
        to another device (``model.to(device)`` after construction). Reads the host."""
        if not self._bound:
            raise RuntimeError("this scheduler no longer drives its optimizer")
        self._allocate(self.last_epoch)

    def _pack(self) -> None:
        s = self.segments
        self._args = (list(self.base_lrs), list(self.bounds), [_KINDS.index(x["kind"]) for x in s],
                      [x["n"] for x in s], [x["a"] for x in s], [x["b"] for x in s], [x["milestones"] for x in s])

    def _launch(self, increment: bool) -> None:
        if not self.counters:
            return
        C = native()
        for d, t in self.counters.items():
            C.lr_schedule_step_(t, self.lrs[d], *self._args, increment)

    def _released(self) -> None:
        self._bound = False

    def _write_groups(self, values) -> None:
        for g, v in zip(self.optimizer.param_groups, values):
            g["lr"] = float(v)

    # ------------------------------------------------------------ the schedule
    def value_at(self, t: int) -> list:
        """The learning rate of every group at step ``t``: the closed forms in Python floats (fp64).
        The CPU path uses it; it is the specification of the kernel."""
        return evaluate(self.segments, self.bounds, self.base_lrs, int(t))

    def step(self) -> None:
        """``t += 1`` and ``lr = lr(t)``, on every device. Call it after ``optimizer.step()``. Reads
        nothing from the host: capturable. (With CPU parameters the host counts too and writes
        ``group["lr"]``.)"""
        if not self._bound:
            raise RuntimeError("this scheduler no longer drives its optimizer (another one was bound, e.g. a "
                               "SequentialLR built from it)")
        self._launch(increment=True)
        if self._host:
            self._t += 1
            self._write_groups(self.value_at(self._t))

    # ------------------------------------------------------------ host-read points
    @property
    def last_epoch(self) -> int:
        """The step count ``t``. Reads the device: outside a captured step only."""
        if self.counters:
            return int(next(iter(self.counters.values())).item())
        return self._t

    def sync(self) -> list:
        """Refresh ``group["lr"]`` from the device and return the values. Reads the host's copy of
        the device buffer: outside a captured step only."""
        if self.lrs and not self._host:
            self._write_groups(next(iter(self.lrs.values())).tolist())
        return [g["lr"] for g in self.optimizer.param_groups]

    def get_last_lr(self) -> list:
        """The learning rates now in force (``sync()``). Outside a captured step only."""
        return self.sync()

    def state_dict(self) -> dict:
        """``{"t", "base_lrs", "program"}``; ``t`` is read from the device (graph replays advance it
        without the host). Outside a captured step only."""
        self.sync()
        return {"t": self.last_epoch, "base_lrs": list(self.base_lrs),
                "program": {"bounds": list(self.bounds), "segments": [dict(s, milestones=list(s["milestones"]))
                                                                      for s in self.segments]}}

    def load_state_dict(self, state: dict) -> None:
        """Restore the program, the base rates and ``t``, then write ``lr(t)`` on every device (the
        no-increment launch): a resumed run continues the same trajectory. Ends with ``sync()``, a
        host read: outside a captured step only."""
        prog = state["program"]
        segments = [_segment(s["kind"], s["n"], s["a"], s["b"], s["milestones"]) for s in prog["segments"]]
        bounds = [int(b) for b in prog["bounds"]]
        _check_program(segments, bounds)
        base = [float(b) for b in state["base_lrs"]]
        if len(base) != len(self.base_lrs):
            raise ValueError(f"loaded state has {len(base)} parameter groups, the optimizer has {len(self.base_lrs)}")
        self.segments, self.bounds, self.base_lrs = segments, bounds, base
        for g, b in zip(self.optimizer.param_groups, base):
            g["initial_lr"] = b
        self._t = int(state["t"])
        for t in self.counters.values():
            t.fill_(self._t)
        self._pack()
        self._launch(increment=False)
        if self._host:
            self._write_groups(self.value_at(self._t))
        else:
            self.sync()


class ConstantLR(LRScheduler):
    def __init__(self, optimizer, factor: float = 1.0 / 3, total_iters: int = 5, last_epoch: int = -1):
        if factor > 1.0 or factor < 0:
            raise ValueError("Constant multiplicative factor expected to be between 0 and 1.")
        super().__init__(optimizer, [_segment("constant", total_iters, factor)], (), last_epoch)


class LinearLR(LRScheduler):
    def __init__(self, optimizer, start_factor: float = 1.0 / 3, end_factor: float = 1.0, total_iters: int = 5,
                 last_epoch: int = -1):
        if start_factor > 1.0 or start_factor <= 0:
            raise ValueError("Starting multiplicative factor expected to be greater than 0 and less or equal to 1.")
        if end_factor > 1.0 or end_factor < 0:
            raise ValueError("Ending multiplicative factor expected to be between 0 and 1.")
        super().__init__(optimizer, [_segment("linear", total_iters, start_factor, end_factor)], (), last_epoch)


class CosineAnnealingLR(LRScheduler):
    def __init__(self, optimizer, T_max: int, eta_min: float = 0.0, last_epoch: int = -1):
        super().__init__(optimizer, [_segment("cosine", T_max, eta_min)], (), last_epoch)


class StepLR(LRScheduler):
    def __init__(self, optimizer, step_size: int, gamma: float = 0.1, last_epoch: int = -1):
        super().__init__(optimizer, [_segment("step", step_size, gamma)], (), last_epoch)


class MultiStepLR(LRScheduler):
    """``milestones`` ascending; a repeated milestone multiplies by ``gamma`` once per repeat, as in torch."""

    def __init__(self, optimizer, milestones, gamma: float = 0.1, last_epoch: int = -1):
        milestones = list(milestones)
        super().__init__(optimizer, [_segment("multistep", len(milestones), gamma, milestones=milestones)], (),
                         last_epoch)


class ExponentialLR(LRScheduler):
    def __init__(self, optimizer, gamma: float, last_epoch: int = -1):
        super().__init__(optimizer, [_segment("exponential", 0, gamma)], (), last_epoch)


class PolynomialLR(LRScheduler):
    def __init__(self, optimizer, total_iters: int = 5, power: float = 1.0, last_epoch: int = -1):
        super().__init__(optimizer, [_segment("polynomial", total_iters, 0.0, power)], (), last_epoch)


class SequentialLR(LRScheduler):
    """``schedulers[i]`` is in force from ``milestones[i-1]`` (0 for the first) up to ``milestones[i]``
    and is evaluated at the time since its start. The given schedulers only hand over their programs:
    this object drives the optimizer from then on, and their ``step()`` raises."""

    def __init__(self, optimizer, schedulers, milestones, last_epoch: int = -1):
        schedulers, milestones = list(schedulers), [int(m) for m in milestones]
        if not schedulers:
            raise ValueError("SequentialLR expects at least one scheduler")
        for i, s in enumerate(schedulers):
            if not isinstance(s, LRScheduler):
                raise TypeError(f"SequentialLR chains the schedulers of this module, got {type(s).__name__} at index {i}")
            if s.optimizer is not optimizer:
                raise ValueError(f"SequentialLR expects all schedulers to belong to the same optimizer, but got "
                                 f"scheduler at index {i} bound to another one")
        if len(milestones) != len(schedulers) - 1:
            raise ValueError(f"SequentialLR expects {len(schedulers) - 1} milestones for {len(schedulers)} schedulers, "
                             f"got {len(milestones)}")
        if any(b <= a for a, b in zip([0] + milestones, milestones)):
            raise ValueError(f"SequentialLR milestones must be ascending and positive, got {milestones}")
        starts, segments = [], []
        for i, s in enumerate(schedulers):  # flatten: a chained scheduler may itself have several segments
            begin = milestones[i - 1] if i else 0
            end = milestones[i] if i < len(milestones) else math.inf
            for j, seg in enumerate(s.segments):
                at = begin + (s.bounds[j - 1] if j else 0)
                if at < end:
                    starts.append(at)
                    segments.append(seg)
        super().__init__(optimizer, segments, starts[1:], last_epoch)
