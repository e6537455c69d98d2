"""Capturable weight averaging: EMA / SWA copies of a model (csrc/kernels/averaging.hip).

``AveragedModel(model, decay=None)`` keeps the equal-weight running mean of SWA, ``decay=d`` an
exponential moving average; the public surface and the state_dict (``n_averaged``, ``module.*``)
are those of ``torch.optim.swa_utils.AveragedModel``. What differs is the execution:

  * ``update_parameters`` reads nothing on the host. One single-wave launch per device turns the
    device counter ``n_averaged`` into this update's weight ``w`` (1 for the first update, then
    ``1 / (n + 1)`` or ``1 - decay``) and advances the counter; the update launches read ``w``.
    So the update sits inside a captured step (``utils.graphs.GraphedStep``) and never stalls an
    eager loop;
  * the average is fp32 whatever the model's dtype. fp32 parameters are views of one flat fp32
    buffer per device; a bf16 parameter has a private fp32 master and the module holds its
    rounding, written by the same kernel (with ``decay >= 0.999`` the step ``(1 - d)(p - a)`` is
    below a bf16 ulp, so an average kept in bf16 would stop moving);
  * ``bf16_shadow=True`` also writes ``p._ptdt_bf16`` of every fp32 averaged parameter in that
    pass (the contract of ``FusedSGD(bf16_shadow=True)``): evaluating the averaged model under bf16
    autocast casts no weight;
  * launches follow the optimizers: one flat launch when sources and averages are both one span
    (``FlatParameters``), else multi-tensor launches of at most 32 tensors.

Buffers: ``use_buffers=False`` copies every buffer of the model in each update (the same kernel
against a constant-one weight, which copies bits; integer buffers that are not whole 32-bit words
with ``copy_``), ``use_buffers=True`` averages the floating ones with ``w`` and copies the rest. CPU tensors take eager ATen math with the same formulae.

The fp32 masters of a bf16 model are not part of the state_dict (its keys are torch's): after
``load_state_dict`` they restart from the loaded bf16 values.
"""
from __future__ import annotations

import copy

import numpy as np
import torch
import torch.nn as nn

from .._ext import native
from .flat import contiguous_span, dense_like, same_layout

_WRAPPERS = ("DistributedDataParallel", "DataParallel")


def unwrap(model: nn.Module) -> nn.Module:
    """The module inside DistributedDataParallel / DataParallel wrappers (torch's or this package's)."""
    while type(model).__name__ in _WRAPPERS and isinstance(getattr(model, "module", None), nn.Module):
        model = model.module
    return model


def averaging_weight(n: int, decay: float | None = None, warmup: bool = False) -> float:
    """The weight of update number ``n`` (``n`` updates applied before it), as the device computes it:
    the float64 formula rounded once to float32."""
    if n == 0:
        w = 1.0
    elif decay is None:
        w = 1.0 / (n + 1.0)
    else:
        d = min(decay, (1.0 + n) / (10.0 + n)) if warmup else decay
        w = 1.0 - d
    return float(np.float32(w))


def _words(t: torch.Tensor) -> torch.Tensor:
    """A contiguous int32 / int64 tensor as a 1-D tensor of float32 words over the same memory."""
    return t.reshape(-1).view(torch.float32)


class _Group:
    """The floating tensors of one (device, source dtype, parameters | buffers): one launch sequence."""

    def __init__(self, device, dtype, params: bool):
        self.device, self.dtype, self.params = device, dtype, params
        self.idx: list = []      # positions in the model's parameters() + buffers() sequence
        self.owners: list = []   # the module's tensors (parameters or buffers)
        self.avgs: list = []     # fp32 averages (the owners' data for fp32 sources)
        self.shadows: list = []  # bf16 autocast copies of fp32 parameters (bf16_shadow=True)
        self.copies: list = []   # bf16 owners' data, the rounding of their fp32 master
        self.bits = False        # integer buffers seen as float32 words: copied (weight one), never averaged
        self.src_words: dict = {}  # bits: position -> (source data_ptr, its float32 view), remade when it moves
        self.avg_span = self.shadow_span = self.copy_span = None

    def words_of(self, i: int, src: torch.Tensor) -> torch.Tensor:
        """The float32 view of the integer source at position ``i``, for where it lies now."""
        if not src.is_contiguous():
            raise ValueError("AveragedModel: an integer buffer of the model is not contiguous")
        hit = self.src_words.get(i)
        if hit is None or hit[0] != src.data_ptr() or hit[1].numel() * 4 != src.numel() * src.element_size():
            hit = self.src_words[i] = (src.data_ptr(), _words(src))
        return hit[1]


class AveragedModel(nn.Module):
    def __init__(self, model: nn.Module, *, decay: float | None = None, warmup: bool = False,
                 use_buffers: bool = False, bf16_shadow: bool = False):
        super().__init__()
        if decay is not None and not (0.0 < float(decay) < 1.0):
            raise ValueError(f"decay must lie in (0, 1) (None: the equal-weight mean of SWA), got {decay}")
        if warmup and decay is None:
            raise ValueError("warmup applies to an exponential moving average: give a decay")
        model = unwrap(model)
        self.module = copy.deepcopy(model)
        first = next(iter(model.parameters()), None)
        if first is None:
            first = next(iter(model.buffers()), None)
        device = first.device if first is not None else torch.device("cpu")
        self.register_buffer("n_averaged", torch.tensor(0, dtype=torch.long, device=device))
        self.decay = None if decay is None else float(decay)
        self.warmup = bool(warmup)
        self.use_buffers = bool(use_buffers)
        self.bf16_shadow = bool(bf16_shadow)
        self._masters: dict = {}  # name -> fp32 master of a bf16 tensor of the module
        self._plan = None
        self._slots: dict = {}    # device -> {"n": counter or None (n_averaged), "w", "one"}
        self._cpu_w = None
        self._build_plan()

    def forward(self, *args, **kwargs):
        return self.module(*args, **kwargs)

    # ------------------------------------------------------------ layout
    def _apply(self, fn, recurse=True):
        out = super()._apply(fn, recurse)
        self._plan, self._slots = None, {}  # the tensors may have moved: laid out again at the next update
        return out

    def load_state_dict(self, state_dict, *args, **kwargs):
        out = super().load_state_dict(state_dict, *args, **kwargs)
        self._masters, self._plan, self._slots = {}, None, {}
        return out

    def _named_tensors(self):
        ps = [("p." + k, v, True) for k, v in self.module.named_parameters()]
        bs = [("b." + k, v, False) for k, v in self.module.named_buffers()]
        return ps + bs

    def _build_plan(self):
        """Lay the module's floating tensors out (flat fp32 parameter buffers, fp32 masters, shadows)
        and group them for the launches. Runs at construction and again after the module moved."""
        entries = self._named_tensors()
        groups: dict = {}
        plain = []  # (index, owner): integer (and any non-floating) tensors, copied with copy_
        for i, (name, t, is_param) in enumerate(entries):
            if not t.is_floating_point():
                if t.is_cuda and t.element_size() % 4 == 0 and t.is_contiguous():
                    # 53 copy_ calls of ResNet-50's num_batches_tracked cost three times the averaging of its
                    # 25 M weights (profiles/averaging.md): int32 / int64 buffers go through the update
                    # kernel as float32 words against the constant-one weight, whose a = p branch moves bits
                    g = groups.setdefault((t.device, "bits"), _Group(t.device, torch.float32, False))
                    g.bits = True
                    g.idx.append(i)
                    g.owners.append(t)
                else:
                    plain.append((i, t))
                continue
            if t.is_cuda and t.dtype not in (torch.float32, torch.bfloat16):
                raise TypeError(f"AveragedModel: GPU tensors must be float32 or bfloat16, {name[2:]} is {t.dtype}")
            g = groups.setdefault((t.device, t.dtype, is_param), _Group(t.device, t.dtype, is_param))
            g.idx.append(i)
            g.owners.append(t)
        for g in groups.values():
            if g.bits:
                g.avgs = [_words(t.data) for t in g.owners]
                continue
            names = [entries[i][0] for i in g.idx]
            total = sum(t.numel() for t in g.owners)
            if g.dtype in (torch.float32, torch.float64):  # averaged in place (float64: CPU only)
                if g.params and g.dtype == torch.float32:  # views of one flat buffer, shape and memory order kept
                    flat, off = torch.empty(total, device=g.device, dtype=torch.float32), 0
                    for t in g.owners:
                        v = dense_like(flat[off:off + t.numel()], t.data)
                        v.copy_(t.data)
                        t.data = v
                        off += t.numel()
                g.avgs = [t.data for t in g.owners]
                if self.bf16_shadow and g.params and g.device.type == "cuda":
                    flat, off = torch.empty(total, device=g.device, dtype=torch.bfloat16), 0
                    for t in g.owners:
                        sh = dense_like(flat[off:off + t.numel()], t.data)
                        sh.copy_(t.data)
                        t._ptdt_bf16, t._ptdt_bf16_version = sh, t._version
                        g.shadows.append(sh)
                        off += t.numel()
            else:  # the fp32 average is a private master, the module's tensor its rounding
                flat, off = torch.empty(total, device=g.device, dtype=torch.float32), 0
                low = torch.empty(total, device=g.device, dtype=g.dtype) if g.params else None
                for name, t in zip(names, g.owners):
                    m = dense_like(flat[off:off + t.numel()], t.data)
                    old = self._masters.get(name)
                    m.copy_(old if old is not None and old.shape == t.shape else t.data)
                    self._masters[name] = m
                    g.avgs.append(m)
                    if low is not None:
                        v = dense_like(low[off:off + t.numel()], t.data)
                        v.copy_(t.data)
                        t.data = v
                    g.copies.append(t.data)
                    off += t.numel()
            g.avg_span = contiguous_span(g.avgs)
            g.shadow_span = contiguous_span(g.shadows) if g.shadows else None
            g.copy_span = contiguous_span(g.copies) if g.copies else None
        self._plan = (len(entries), list(groups.values()), plain)
        return self._plan

    def _slot(self, device):
        s = self._slots.get(device)
        if s is None:
            n = None if device == self.n_averaged.device else self.n_averaged.to(device).clone()
            s = {"n": n, "w": torch.zeros(1, device=device), "one": torch.ones(1, device=device)}
            self._slots[device] = s
        return s

    # ------------------------------------------------------------ the update
    @torch.no_grad()
    def update_parameters(self, model: nn.Module) -> None:
        """One averaging step from ``model`` (wrappers are looked through). No host read and, after
        the first call, no allocation: capturable. Source pointers are taken now, not cached."""
        model = unwrap(model)
        count, groups, plain = self._plan or self._build_plan()
        srcs = [p.data for p in model.parameters()] + [b for b in model.buffers()]
        if len(srcs) != count:
            raise ValueError(f"update_parameters: the model has {len(srcs)} parameters and buffers, "
                             f"the averaged copy {count}")
        devices = {g.device for g in groups} | {self.n_averaged.device}
        n_before = None
        for d in devices:
            if d.type != "cuda":  # CPU tensors: eager math on the host's copy of the weight
                n_before = int(self.n_averaged) if n_before is None else n_before
                self._cpu_w = averaging_weight(n_before, self.decay, self.warmup)
        for d in devices:
            if d.type == "cuda":
                s = self._slot(d)
                native().avg_prepare_(self.n_averaged if s["n"] is None else s["n"], s["w"], self.decay, self.warmup)
        for g in groups:
            ps = [g.words_of(i, srcs[i]) for i in g.idx] if g.bits else [srcs[i] for i in g.idx]
            averaged = not g.bits and (g.params or self.use_buffers)
            if g.device.type != "cuda":
                self._cpu_update(g, ps, self._cpu_w if averaged else 1.0)
            else:
                slot = self._slot(g.device)
                self._gpu_update(g, ps, slot["w"] if averaged else slot["one"])
        for i, t in plain:
            t.copy_(srcs[i])
        if not self.n_averaged.is_cuda:
            self.n_averaged += 1

    def _gpu_update(self, g: _Group, ps, w):
        C = native()
        pspan = None
        if (g.avg_span is not None and (not g.shadows or g.shadow_span is not None)
                and (not g.copies or g.copy_span is not None)):
            pspan = contiguous_span(ps)  # None at the first tensor that is not back to back
            if pspan is not None and not same_layout(ps, g.avgs):
                pspan = None
        if pspan is not None:  # sources and averages are one span each: one launch
            C.avg_update_flat_(g.avg_span, pspan, w, g.shadow_span, g.copy_span)
        else:
            C.avg_update_multi_(g.avgs, ps, w, g.shadows, g.copies)
        for t in g.owners if g.shadows else ():
            t._ptdt_bf16_version = t._version  # the shadow is current until the parameter changes

    @staticmethod
    def _cpu_update(g: _Group, ps, w: float):
        for k, (a, p) in enumerate(zip(g.avgs, ps)):
            p = p.to(device=a.device, dtype=a.dtype)
            if w == 1.0:
                a.copy_(p)
            else:
                a.add_(p - a, alpha=w)
            if g.copies:
                g.copies[k].copy_(a)

    def averages(self) -> list:
        """``(name, average)`` of every floating parameter and buffer of the module, parameters first:
        the fp32 tensors the updates act on (a bf16 tensor's master, an fp32 tensor itself)."""
        _, groups, _ = self._plan or self._build_plan()
        names = [name[2:] for name, _, _ in self._named_tensors()]
        pairs = sorted((i, a) for g in groups if not g.bits for i, a in zip(g.idx, g.avgs))
        return [(names[i], a) for i, a in pairs]

    def last_weight(self) -> float | None:
        """The weight ``w`` of the latest update (None before the first). A host read: for logs and
        tests, outside a capture."""
        if self.n_averaged.is_cuda:
            s = self._slots.get(self.n_averaged.device)
            return None if s is None else float(s["w"].item())
        return self._cpu_w
