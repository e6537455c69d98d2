"""Capturable evaluation: cross-entropy and top-k accuracy of a classifier, kept on the device
(csrc/kernels/eval_metrics.hip).

``classification_rows(logits, target)`` gives, per row of ``[B, C]`` logits, the cross-entropy
``lse - z_y`` and the *rank* of the target: the number of logits greater than the target's plus the
number equal to it at a smaller class index, i.e. the target's position in a stable descending sort.
``rank < k`` is top-k correctness for every k at once, with ties resolved towards the smaller class
index. Special rows:

  * ``target == ignore_index``: ``(0, -1)``;
  * any other target outside ``[0, C)``: ``(0, -2)``; the row is never read at that index;
  * the target's logit NaN: rank ``C`` (correct at no k), loss NaN;
  * NaNs elsewhere do not count as greater; the loss is NaN as the arithmetic makes it.

``ClassificationMeter`` accumulates those rows into two device tensors -- int64 counters
``[rows, valid, ignored, bad_target, nonfinite, correct@k...]`` and one float64 loss sum (the finite
losses of valid rows). ``update`` reads nothing on the host and, on the GPU, is two launches on the
current stream that read each logit once and add in a fixed order (no atomics): it sits inside a
``torch.cuda.graph`` capture, and the same inputs give the same bits. ``compute`` is the only host
read.

float32 and bfloat16 logits on the GPU take the native kernels; CPU tensors and other dtypes take a
torch implementation of the same rules, as in ops/loss.py.
"""
from __future__ import annotations

import torch

from .._ext import native, use_native

_BASE = ("rows", "valid", "ignored", "bad_target", "nonfinite")
_NATIVE_DTYPES = (torch.float32, torch.bfloat16)
MAX_TOPK = 8  # the ks travel by value in the launch arguments (kEvalMaxK)


def _check_rows(logits: torch.Tensor, target: torch.Tensor):
    if logits.dim() != 2 or logits.size(0) < 1 or logits.size(1) < 1:
        raise ValueError(f"logits must be [B, C] with B, C >= 1, got {tuple(logits.shape)}")
    if not logits.is_floating_point():
        raise TypeError(f"logits must be floating point, got {logits.dtype}")
    if target.dtype != torch.int64 or target.dim() != 1 or target.numel() != logits.size(0):
        raise ValueError(f"target must be int64[{logits.size(0)}] class indices, got {target.dtype} "
                         f"{tuple(target.shape)}")
    if target.device != logits.device:
        raise ValueError(f"logits are on {logits.device}, target on {target.device}")


def _rows_torch(logits: torch.Tensor, target: torch.Tensor, ignore_index: int):
    z = logits if logits.dtype == torch.float64 else logits.float()
    C = z.size(1)
    ignored = target == ignore_index
    bad = ~ignored & ((target < 0) | (target >= C))
    ok = ~(ignored | bad)
    y = torch.where(ok, target, torch.zeros_like(target)).unsqueeze(1)  # never gathers outside the row
    zy = z.gather(1, y)
    before = torch.arange(C, device=z.device).unsqueeze(0) < y
    rank = (z > zy).sum(1) + ((z == zy) & before).sum(1)
    rank = torch.where(torch.isnan(zy.squeeze(1)), torch.full_like(rank, C), rank)
    loss = (torch.logsumexp(z, 1) - zy.squeeze(1)).float()
    rank = torch.where(ignored, torch.full_like(rank, -1), torch.where(bad, torch.full_like(rank, -2), rank))
    return torch.where(ok, loss, torch.zeros_like(loss)), rank.to(torch.int32)


def classification_rows(logits: torch.Tensor, target: torch.Tensor, ignore_index: int = -100):
    """``(row_loss float32[B], rank int32[B])`` of ``[B, C]`` logits and int64 ``[B]`` targets (module
    docstring). Native on the GPU for float32 / bfloat16 logits whose rows are contiguous (column
    stride 1; any row stride, e.g. ``logits[:, :C]`` of a padded head)."""
    _check_rows(logits, target)
    if use_native(logits) and logits.dtype in _NATIVE_DTYPES:
        return native().eval_rows(logits, target, int(ignore_index))
    return _rows_torch(logits, target, int(ignore_index))


class ClassificationMeter:
    """Summed cross-entropy and top-k correct counts for several k at once, on the device.

    ``device=None`` places the state on the device of the first ``update``'s logits."""

    def __init__(self, topk=(1, 5), ignore_index: int = -100, device=None):
        topk = tuple(int(k) for k in topk)
        if not 1 <= len(topk) <= MAX_TOPK:
            raise ValueError(f"topk takes 1 to {MAX_TOPK} values, got {len(topk)}")
        if topk[0] < 1 or any(b <= a for a, b in zip(topk, topk[1:])):
            raise ValueError(f"topk must be strictly increasing values >= 1, got {topk}")
        self.topk = topk
        self.ignore_index = int(ignore_index)
        self._follow = device is None  # the state moves to the first logits' device
        device = torch.device("cpu") if device is None else torch.device(device)
        self.counters = torch.zeros(len(_BASE) + len(topk), dtype=torch.int64, device=device)
        self.loss_sum = torch.zeros(1, dtype=torch.float64, device=device)
        self._ws: dict = {}  # B -> (row_loss, rank) workspaces of the native update

    @property
    def device(self) -> torch.device:
        return self.counters.device

    def to(self, device):
        device = torch.device(device)
        if device != self.device:
            self.counters, self.loss_sum, self._ws = self.counters.to(device), self.loss_sum.to(device), {}
        self._follow = False
        return self

    def reset(self) -> None:
        """Zero the state on its device (no host synchronisation)."""
        self.counters.zero_()
        self.loss_sum.zero_()

    @torch.no_grad()
    def update(self, logits: torch.Tensor, target: torch.Tensor) -> None:
        _check_rows(logits, target)
        B, C = logits.shape
        if self.topk[-1] > C:
            raise ValueError(f"topk {self.topk}: k = {self.topk[-1]} exceeds the {C} classes of the logits")
        if self._follow:
            self.to(logits.device)
        if logits.device != self.device:
            raise ValueError(f"the meter's state is on {self.device}, the logits on {logits.device}")
        if use_native(logits) and logits.dtype in _NATIVE_DTYPES:
            ws = self._ws.get(B)
            if ws is None:
                ws = self._ws[B] = (torch.empty(B, dtype=torch.float32, device=self.device),
                                    torch.empty(B, dtype=torch.int32, device=self.device))
            native().eval_update_(logits, target, self.ignore_index, list(self.topk), self.counters, self.loss_sum,
                                  ws[0], ws[1])
            return
        loss, rank = _rows_torch(logits, target, self.ignore_index)
        valid = rank >= 0
        finite = valid & torch.isfinite(loss)
        parts = [valid.sum(), (rank == -1).sum(), (rank == -2).sum(), (valid & ~finite).sum()]
        parts += [(valid & (rank < k)).sum() for k in self.topk]
        self.counters[0] += B
        self.counters[1:] += torch.stack(parts)
        self.loss_sum += torch.where(finite, loss.double(), torch.zeros_like(loss, dtype=torch.float64)).sum()

    def compute(self, comm=None) -> dict:
        """The metrics so far: the only host read. With a communicator of more than one rank the
        counters (int64) and the loss sum (float64) are summed over its ranks first; the meter's own
        state stays local. Raises if any target was neither ``ignore_index`` nor a class."""
        counters, loss_sum = self.counters.clone(), self.loss_sum.clone()
        if comm is not None and getattr(comm, "world", 1) > 1:
            comm.all_reduce(counters, "sum")
            comm.all_reduce(loss_sum, "sum")
        c = dict(zip(_BASE + tuple(f"top{k}" for k in self.topk), counters.tolist()))
        total = loss_sum.item()
        if c["bad_target"]:
            raise ValueError(f"{c['bad_target']} of {c['rows']} targets lie outside [0, C) and are not "
                             f"ignore_index = {self.ignore_index}")
        valid, finite = c["valid"], c["valid"] - c["nonfinite"]
        out = {"loss": total / finite if finite else float("nan")}
        for k in self.topk:
            out[f"top{k}"] = c[f"top{k}"] / valid if valid else float("nan")
        out.update(count=valid, ignored=c["ignored"], nonfinite=c["nonfinite"])
        return out

    def state_dict(self) -> dict:
        return {"counters": self.counters.clone(), "loss_sum": self.loss_sum.clone(), "topk": self.topk}

    def load_state_dict(self, state: dict) -> None:
        if tuple(state["topk"]) != self.topk:
            raise ValueError(f"the state was kept for topk = {tuple(state['topk'])}, this meter has {self.topk}")
        self.counters.copy_(state["counters"])
        self.loss_sum.copy_(state["loss_sum"])
