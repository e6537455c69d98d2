"""Gradient clipping on native kernels (csrc/kernels/gradclip.hip), hipGraph-capturable.

``clip_grad_norm_`` / ``clip_grad_value_`` with ``torch.nn.utils`` semantics, built for the two
properties of this code base:

  * nothing in the step reads the host: the total norm and the clip coefficient live in a
    device record ``{total_norm, clip_coef}`` (float32[2]), so a :class:`GradClipper` call can sit
    inside :class:`utils.graphs.GraphedStep` between ``backward()`` and ``optimizer.step()``;
  * gradients that lie back to back (DDP bucket slots, flat gradient buffers) are read as a few
    contiguous spans, not as one tensor each.

Kernels per call: norm partials (one fp32 value per 4096-element chunk, each in its own workspace
slot), one finalise workgroup (fixed-order float64 sum, ``clip_coef = min(1, max_norm /
(total_norm + 1e-6))``), then either the scale pass (skipped on the device when the coefficient is
exactly 1) or, in *fused mode*, nothing: the coefficient is handed to ``FusedSGD`` / ``FusedAdam``,
whose next ``step()`` multiplies it into every gradient as the update kernel loads it.

**Fused mode leaves ``p.grad`` unclipped.** Only the update sees the clipped values; code that
reads ``p.grad`` after the call (logging, a second optimizer) sees the raw gradient.

**DDP.** This project's DDP gradients are rank-averaged when ``backward()`` returns, so the local
norm is the global norm and every rank computes the same bits: no collective is added. Call it
after ``backward()`` and outside ``no_sync()`` (inside, the gradients are local partial sums).

Norm types 2 and inf on dense float32 / bfloat16 GPU gradients run on the kernels. Other norm
types, CPU tensors, sparse or non-dense gradients and other dtypes take plain torch ops, as the
CPU paths elsewhere in ``ops``. On a GPU machine without the extension the call raises.
"""
from __future__ import annotations

import math
from typing import Iterable

import torch

from .._ext import native
from .flat import is_dense
from .optim import FusedAdam, FusedSGD

_MAX_SPANS = 32  # kMaxTensorsPerLaunch
_CHUNK = 4096    # kChunk
_NORM_KINDS = {2.0: 0, math.inf: 1}


def _params(parameters) -> list:
    if isinstance(parameters, torch.Tensor):
        return [parameters]
    return list(parameters)


def _kernel_ok(g: torch.Tensor) -> bool:
    return (g.is_cuda and not g.is_sparse and g.dtype in (torch.float32, torch.bfloat16) and is_dense(g))


def _spans(grads) -> dict:
    """{(device, dtype): [1-D span tensors]}: the gradients of each (device, dtype) sorted by address,
    neighbours that lie back to back in one storage merged into one view."""
    groups: dict = {}
    for g in grads:
        groups.setdefault((g.device, g.dtype), []).append(g)
    out = {}
    for key, gs in groups.items():
        gs = sorted(gs, key=lambda t: t.data_ptr())
        spans, run = [], [gs[0]]
        for g in gs[1:]:
            last = run[-1]
            if (g.untyped_storage().data_ptr() == last.untyped_storage().data_ptr()
                    and g.data_ptr() == last.data_ptr() + last.numel() * last.element_size()):
                run.append(g)
            else:
                spans.append(run)
                run = [g]
        spans.append(run)
        out[key] = [torch.empty(0, dtype=r[0].dtype, device=r[0].device).set_(
            r[0].untyped_storage(), r[0].storage_offset(), (sum(t.numel() for t in r),), (1,)) for r in spans]
    return out


def _launches(spans: dict) -> dict:
    """{device: [span lists of <= 32 spans, one dtype each]}"""
    out: dict = {}
    for (device, _), sp in spans.items():
        out.setdefault(device, []).extend(sp[i:i + _MAX_SPANS] for i in range(0, len(sp), _MAX_SPANS))
    return out


class _Plan:
    """Launch plan of one gradient set: spans, workspace slots and records per device."""

    def __init__(self, grads, primary):
        self.primary = primary
        self.launches = _launches(_spans(grads))
        self.num_spans = sum(len(l) for ls in self.launches.values() for l in ls)
        self.others = [d for d in self.launches if d != primary]
        self.slots = {d: sum(-(-s.numel() // _CHUNK) for l in ls for s in l) for d, ls in self.launches.items()}
        # the first device's workspace ends with one slot per other device (its reduced value)
        self.ws = {d: torch.empty(n + (len(self.others) if d == primary else 0), dtype=torch.float32, device=d)
                   for d, n in self.slots.items()}
        self.rec = {d: torch.empty(2, dtype=torch.float32, device=d) for d in self.launches}
        self.coefs = {d: rec[1] for d, rec in self.rec.items()}


class GradClipper:
    """Reusable ``clip_grad_norm_``: ``clipper()`` computes the total norm of the parameters'
    gradients, applies the clip and returns the norm (a 0-d tensor on the first gradient's device).

    ``clipper.norm`` / ``clipper.coef`` are views of the device record of the last call. The launch
    plan (gradients grouped per (device, dtype), coalesced into maximal back-to-back spans, the
    workspace) is cached and keyed on the gradients' (data_ptr, numel, dtype); it is rebuilt when
    they change. Parameters whose ``.grad`` is None, and zero-element gradients, are skipped.

    ``optimizer=FusedSGD/FusedAdam``: fused mode. The gradients are not rewritten (``p.grad`` holds
    the UNCLIPPED gradient afterwards); the optimizer's next ``step()``, and only that one, applies
    the coefficient inside its update kernels. The clipper's parameters with gradients must be
    exactly the optimizer's parameters with gradients, else ``ValueError``.

    Multi-device gradients: partials are reduced per device, each other device's value is copied
    into a slot of the first device's workspace (device-to-device, no host read), the finalise runs
    there and the record is copied back to every device for its scale pass.

    Under DDP call it after ``backward()`` and outside ``no_sync()``."""

    def __init__(self, parameters, max_norm: float, norm_type: float = 2.0, *, optimizer=None):
        self.params = _params(parameters)
        self.max_norm = float(max_norm)
        self.norm_type = float(norm_type)
        if optimizer is not None and not isinstance(optimizer, (FusedSGD, FusedAdam)):
            raise ValueError("fused clipping needs a FusedSGD or FusedAdam optimizer, got "
                             f"{type(optimizer).__name__}")
        self.optimizer = optimizer
        self._opt_ids: set | None = None  # the optimizer's parameter ids, when last looked at
        self._key = None
        self._plan: _Plan | None = None
        self._rec: torch.Tensor | None = None

    # ------------------------------------------------------------ record views
    @property
    def norm(self) -> torch.Tensor:
        return self._rec[0]

    @property
    def coef(self) -> torch.Tensor:
        return self._rec[1]

    @property
    def num_spans(self) -> int:
        """Spans in the current kernel plan (0 before the first kernel call)."""
        return self._plan.num_spans if self._plan is not None else 0

    # ------------------------------------------------------------ call
    def _check_optimizer(self, with_grad) -> None:
        groups = self.optimizer.param_groups
        if self._opt_ids is None or len(self._opt_ids) != sum(len(g["params"]) for g in groups):
            self._opt_ids = {id(p) for g in groups for p in g["params"]}
            self._same_params = self._opt_ids == {id(p) for p in self.params}
        if self._same_params:  # one parameter set: the parameters with gradients are the same too
            return
        mine = {id(p) for p in with_grad}
        theirs = {id(p) for group in self.optimizer.param_groups for p in group["params"]
                  if p.grad is not None and p.grad.numel() > 0}
        if mine != theirs:
            raise ValueError("fused clipping: the clipper's parameters with gradients must be exactly the "
                             f"optimizer's ({len(mine)} vs {len(theirs)}, {len(mine & theirs)} shared)")

    @torch.no_grad()
    def __call__(self, error_if_nonfinite: bool = False) -> torch.Tensor:
        with_grad, grads, key = [], [], []
        for p in self.params:  # one pass: this loop is the call's host cost
            g = p.grad
            if g is not None and g.numel() > 0:
                with_grad.append(p)
                grads.append(g)
                key.append((g.data_ptr(), g.numel(), g.dtype))
        if self.optimizer is not None:
            self._check_optimizer(with_grad)
        if not grads:
            return torch.tensor(0.0)
        if key != self._key:  # a gradient moved, appeared or went away: plan again
            self._key = key
            kernels = self.norm_type in _NORM_KINDS and all(_kernel_ok(g) for g in grads)
            self._plan = _Plan(grads, grads[0].device) if kernels else None
        coefs = self._norm_kernels() if self._plan is not None else self._norm_torch(grads)
        if error_if_nonfinite and not bool(torch.isfinite(self.norm)):
            raise RuntimeError(f"The total norm of order {self.norm_type} for gradients from `parameters` is "
                               "non-finite, so it cannot be clipped. To disable this error and scale the "
                               "gradients by the non-finite norm anyway, set `error_if_nonfinite=False`")
        if self.optimizer is not None:
            self.optimizer.arm_grad_coef(coefs)
        elif self._plan is not None:
            C = native()
            for device, launches in self._plan.launches.items():
                for spans in launches:
                    C.clip_scale_(spans, self._plan.rec[device])
        else:
            for g in grads:
                if g.element_size() < 4 and not g.is_sparse:  # 16-bit: multiply in float32, round once
                    g.copy_(g.float() * coefs[g.device])
                else:
                    g.mul_(coefs[g.device])
        return self.norm

    def _norm_kernels(self) -> dict:
        C = native()
        plan = self._plan
        kind = _NORM_KINDS[self.norm_type]
        first = plan.primary
        for device, launches in plan.launches.items():
            slot = 0
            for spans in launches:
                slot += C.clip_norm_partials_(spans, plan.ws[device], slot, kind)
        for i, device in enumerate(plan.others):
            C.clip_norm_finalize_(plan.ws[device], plan.slots[device], kind, self.max_norm, True, plan.rec[device])
            plan.ws[first][plan.slots[first] + i].copy_(plan.rec[device][0], non_blocking=True)
        C.clip_norm_finalize_(plan.ws[first], plan.ws[first].numel(), kind, self.max_norm, False, plan.rec[first])
        for device in plan.others:
            plan.rec[device].copy_(plan.rec[first], non_blocking=True)
        self._rec = plan.rec[first]
        return plan.coefs

    def _norm_torch(self, grads) -> dict:
        first = grads[0].device
        dense = [g.coalesce().values() if g.is_sparse else g for g in grads]
        # accumulated in float64 (the kernels' finalise does the same), the record in float32 as there
        norms = [torch.linalg.vector_norm(g, self.norm_type, dtype=torch.float64).to(first) for g in dense]
        total = torch.linalg.vector_norm(torch.stack(norms), self.norm_type).float()
        coef = torch.clamp(self.max_norm / (total + 1e-6), max=1.0)
        self._rec = torch.stack([total, coef])
        return {device: self._rec[1].to(device) for device in {g.device for g in grads}}


def clip_grad_norm_(parameters, max_norm: float, norm_type: float = 2.0, error_if_nonfinite: bool = False,
                    foreach: bool | None = None, *, optimizer=None) -> torch.Tensor:
    """``torch.nn.utils.clip_grad_norm_`` on the native kernels; returns the total norm (0-d tensor on
    the first gradient's device). With ``error_if_nonfinite=False`` nothing is read back to the host.
    ``foreach`` is accepted for signature compatibility (the kernels are always multi-tensor).
    ``optimizer=``: fused mode, see :class:`GradClipper` -- ``p.grad`` stays unclipped and the
    optimizer's next ``step()`` applies the coefficient. Under DDP: after ``backward()``, outside
    ``no_sync()``. Builds a :class:`GradClipper` per call; keep one to reuse its launch plan."""
    del foreach
    return GradClipper(parameters, max_norm, norm_type, optimizer=optimizer)(error_if_nonfinite)


@torch.no_grad()
def clip_grad_value_(parameters: Iterable[torch.Tensor] | torch.Tensor, clip_value: float,
                     foreach: bool | None = None) -> None:
    """``torch.nn.utils.clip_grad_value_``: every gradient clamped to [-clip_value, clip_value] in
    place (NaN kept). Dense f32 / bf16 GPU gradients run on the clamp kernel over coalesced spans."""
    del foreach
    grads = [p.grad for p in _params(parameters) if p.grad is not None and p.grad.numel() > 0]
    clip_value = float(clip_value)
    fast = [g for g in grads if _kernel_ok(g)]
    for g in grads:
        if not _kernel_ok(g):
            g.clamp_(min=-clip_value, max=clip_value)
    if fast:
        C = native()
        for launches in _launches(_spans(fast)).values():
            for spans in launches:
                C.clip_clamp_(spans, clip_value)
