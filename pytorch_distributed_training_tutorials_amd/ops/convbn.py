"""1x1 convolution + training BatchNorm with the statistics computed in the convolution's
epilogue: ``ReLU?(BN(conv1x1(x)) + residual?)``.

A stride-1 1x1 convolution over an NHWC (channels_last) activation is a GEMM,
``Y[N*H*W, Cout] = X[N*H*W, Cin] . W[Cout, Cin]^T``, with both operands already
K-contiguous in memory. Two native kernels run it and, while each output value is
still in registers, reduce the output to per-channel sums for the BatchNorm:

* ``conv1x1_bn.hip`` (streaming; ResNet-50's layer1 shapes and, with the weights in
  <= 64 KiB slabs, 128 -> 512 and 256 -> 1024): persistent workgroups, weights
  resident in LDS, activation row blocks LDS-DMA'd ahead, 16-B output stores,
  per-lane sums about running-mean pivots;
* ``gemm_bn_stats`` in ``gemm_big.hip`` (tiled, any K % 64 == 0 shape): the
  LDS-DMA GEMM with centred per-wave partials in its epilogue.

Partials are merged in fixed order by the last workgroups to finish (two ticket
levels, sc1 hand-off), which also write the BN coefficients and update the running
statistics. The BN then runs only its apply pass (``bn_fwd_apply``): the separate
statistics pass -- a full read of the conv output -- is gone (bf16, batch 128:
-214 us per ResNet-50 step, profiles/r3_convbn.md).

Backward (``PTDT_CONVBN_BWD``): ``1`` (default) links the BN's backward to the conv's where the
streaming kernel ``conv1x1_bwd.hip`` has an instance and this module ran the forward: the BN runs
only its reduce pass and the conv's backward forms ``dY = A g + B y + C`` inside its data- and
weight-gradient products (:class:`ConvBwdLink`). ``all`` does so for every other shape the K/N-tiled
kernels of ``conv1x1_bwd_tiled.hip`` take (K, N multiples of 64 up to 4096: ResNet-50's layer2-4),
whoever ran the forward: where MIOpen's forward wins the timing, it runs inside a small autograd
Function with the same linked backward. ``0``, and any shape without a kernel: the BN's native
backward, then the convolution's gradients on MIOpen (``aten.convolution_backward``, as autograd
would call it). ``PTDT_CONVBN_BWD_SKIP`` keeps single shapes unlinked. Forward numerics: the
statistics are those of the stored bf16 output (what the separate pass would read), merged in double.

Input BatchNorm (``PTDT_CONVBN_PRE=1``, default 0): ``conv_bn_act(..., pre_bn=bn2)`` takes the RAW input of
``pre_bn`` and computes ``bn(conv(ReLU(pre_bn(x))))`` without ``pre_bn``'s apply pass: its statistics pass runs
alone (``bn_fwd_stats``) and ``conv1x1_pre.hip`` forms ``bf16(max(x * scale + shift, 0))`` on its operand path,
with the output's statistics in its epilogue as above. The backward is the tiled link, whose weight-gradient
kernel recomputes the same operand from ``x`` (``pre=``), then ``pre_bn``'s own backward: the normalised
activation is neither written, re-read nor saved (ResNet-50's conv2 -> bn2 -> ReLU -> conv3).
``PTDT_CONVBN_PRE_SKIP=KxN,...`` keeps single shapes on the composed path.

3x3 convolutions (``PTDT_CONV3X3=0|on|auto``, default 0): a stride-1, padding-1 3x3 ``conv`` with channel counts
that are multiples of 64 up to 1024 runs on ``conv3x3_bn.hip``, an implicit GEMM over the NHWC activation
(K = 9 Cin, no im2col buffer) with the same statistics epilogue, and the BN runs only its apply pass. The
backward is the BN's native backward, then ``aten.convolution_backward`` on MIOpen. ``auto`` times
the pair against MIOpen + ``bn_fwd_train`` once per (N, H, W, Cin, Cout) (tuning family ``conv3x3bn``).
Not combined with ``PTDT_CONVBN_PRE`` (profiles/conv3x3_bn.md).

3x3 backward (``PTDT_CONV3X3_BWD=0|1``, default 0): the same convolutions get a :class:`ConvBwdLink`, behind the
native forward or, where ``PTDT_CONV3X3`` is 0 or ``auto`` chose MIOpen, behind MIOpen's forward with the BN's own
statistics: the BN runs only its reduce pass and ``conv3x3_bwd.hip`` forms ``dY = A g + B y + C`` on the operand
paths of its data- and weight-gradient kernels, so ``dY`` is neither written nor read back.
``PTDT_CONV3X3_BWD_SKIP=CinxCout,...`` keeps single shapes on MIOpen's backward (profiles/conv3x3_bwd.md).

Stride-2 1x1 convolutions (``PTDT_CONVBN_S2=0|1``, default 0): a stride-(2, 2), padding-0 1x1 ``conv`` with
channel counts that are multiples of 64 up to 4096 (the downsample branches of ResNet-50's layer2-4) runs on
``conv1x1_s2.hip``: the stride-1 GEMM with the activation's rows gathered, the statistics in its epilogue, and
the BN runs only its apply pass. Its backward follows ``PTDT_CONVBN_BWD`` / ``PTDT_CONVBN_BWD_SKIP``: linked (not
``0``), the BN runs only its reduce pass, the data-gradient kernel writes every pixel of the dense ``dX`` once --
a gathered row's gradient or zeros, no memset -- and the weight gradient gathers the same rows; else the BN's
native backward and ``aten.convolution_backward``. No timing arm: ``1`` always takes the kernels
(profiles/conv1x1_s2.md).

Anything else -- other strides, eval mode, fp32, NCHW, odd channel counts, CPU --
takes the unfused ``bn_act(bn, conv(x))``. Where both apply, ``PTDT_CONVBN=auto`` (default)
times the two once per shape on the live operands and keeps the faster (MIOpen's 1x1
forward kernels run close to HBM speed on some shapes, profiles/r3_convbn.md); ``on``
always fuses, ``off`` never does.

Reference call sites: the Bottleneck convolutions + BatchNorms of torchvision's
ResNet-50 (NB03:560-570, NB03:807-833).
"""
from __future__ import annotations

import os

import torch
import torch.nn as nn

from .._ext import native
from .conv import cast_weight
from .norm import BatchNorm2d, _like, _rows_layout_ok, _tickets_of, batch_norm_act, synchronizing

_MODE = os.environ.get("PTDT_CONVBN", "auto")  # auto: per-shape timing decides; on / 1: always; off / 0: never
_ENABLED = _MODE not in ("0", "off")
_STREAM = os.environ.get("PTDT_CONVBN_STREAM", "1") != "0"
# fused backward (BN apply + 1x1 data and weight gradients, csrc/kernels/conv1x1_bwd.hip) where an
# instance exists; 0: the BN's full backward, then MIOpen's convolution_backward; all: also the tiled
# kernels (conv1x1_bwd_tiled.hip) for every other shape they take, behind either forward
_BWD = os.environ.get("PTDT_CONVBN_BWD", "1") != "0"
_BWD_TILED = os.environ.get("PTDT_CONVBN_BWD", "1") == "all"
# A/B of single shapes: "KxN,KxN" (input x output channels) keep the unfused backward
_BWD_SKIP = {tuple(int(v) for v in t.split("x")) for t in os.environ.get("PTDT_CONVBN_BWD_SKIP", "").split(",") if t}
# the input BN's apply + ReLU inside the 1x1 conv's operand loads (csrc/kernels/conv1x1_pre.hip); no timing
_PRE = os.environ.get("PTDT_CONVBN_PRE", "0") == "1"
_PRE_SKIP = {tuple(int(v) for v in t.split("x")) for t in os.environ.get("PTDT_CONVBN_PRE_SKIP", "").split(",") if t}
_CHOICE: dict[tuple, bool] = {}  # (M, K, N, tile) -> fused is faster (PTDT_CONVBN=auto)
# stride-1 3x3 convolutions on the native implicit GEMM with the BN statistics in its epilogue
# (csrc/kernels/conv3x3_bn.hip): 0 (default) never, on always, auto per-shape timing against MIOpen
_C3X3 = os.environ.get("PTDT_CONV3X3", "0")
if _C3X3 not in ("0", "on", "auto"):
    raise ValueError(f"PTDT_CONV3X3={_C3X3!r}: expected 0, on or auto")
# the same convolutions' backward linked to the BN's (csrc/kernels/conv3x3_bwd.hip), behind either forward
_C3X3_BWD = os.environ.get("PTDT_CONV3X3_BWD", "0")
if _C3X3_BWD not in ("0", "1"):
    raise ValueError(f"PTDT_CONV3X3_BWD={_C3X3_BWD!r}: expected 0 or 1")
_C3X3_BWD = _C3X3_BWD == "1"
_C3X3_BWD_SKIP = {tuple(int(v) for v in t.split("x"))
                  for t in os.environ.get("PTDT_CONV3X3_BWD_SKIP", "").split(",") if t}
# stride-2 1x1 convolutions on the native gathered-row kernels, forward and backward (csrc/kernels/conv1x1_s2.hip)
_S2 = os.environ.get("PTDT_CONVBN_S2", "0")
if _S2 not in ("0", "1"):
    raise ValueError(f"PTDT_CONVBN_S2={_S2!r}: expected 0 or 1")
_S2 = _S2 == "1"


def _tile(M: int, N: int, K: int) -> int:
    """0: the streaming kernel (memory-bound (K, N) instances: weights resident in LDS); else the
    tiled GEMM's block tile: 256x256 when those tiles fill the chip (>= 192 of them), else 128x128."""
    if _STREAM and native().conv1x1_bn_stream_supported(K, N):
        return 0
    return 256 if (-(-M // 256)) * (-(-N // 256)) >= 192 else 128


class ConvBwdLink:
    """Hand-over from a fused BN's backward to its producing 1x1 conv's backward (the fused backward,
    csrc/kernels/conv1x1_bwd.hip): the BN runs only its reduce pass and passes the masked gradient g
    down as "the gradient of y", leaving here the coefficients of its apply (dY = A g + B y + C); the
    conv's backward then computes dY on the fly inside its data- and weight-gradient GEMMs. None:
    the BN ran its full backward (the conv receives dY itself)."""

    __slots__ = ("coef", "tiled")

    def __init__(self, tiled: bool = False):
        self.coef = None
        self.tiled = tiled  # conv1x1_bwd_tiled.hip instead of the streaming instance


def _bwd_link(cin: int, cout: int) -> ConvBwdLink | None:
    """The link for a cin -> cout convolution, or None: no kernel for the shape, or switched off."""
    if not (_BWD and torch.is_grad_enabled()) or (cin, cout) in _BWD_SKIP:
        return None
    if native().conv1x1_bwd_supported(cin, cout):
        return ConvBwdLink()
    if _BWD_TILED and native().conv1x1_bwd_tiled_supported(cin, cout):
        return ConvBwdLink(tiled=True)
    return None


def _conv_backward(ctx, gy, x, w, y2):
    """(dx, dw) of y = conv1x1(x, w): linked (gy is the BN's masked gradient g, ctx.link holds the
    coefficients) or plain (gy is dY: MIOpen)."""
    link = ctx.link
    if link is not None and link.coef is not None:
        coef, link.coef = link.coef, None
        n, cin, h, wd = x.shape
        cout = w.shape[0]
        g2 = gy.permute(0, 2, 3, 1).reshape(-1, cout)
        if not g2.is_contiguous():
            g2 = g2.contiguous()
        x2 = x.permute(0, 2, 3, 1).reshape(-1, cin)
        bwd = native().conv1x1_bwd_tiled if link.tiled else native().conv1x1_bwd
        dx2, dw2 = bwd(g2, y2, x2, w.reshape(cout, cin), coef)
        dx = dx2.view(n, h, wd, cin).permute(0, 3, 1, 2) if ctx.needs_input_grad[0] else None
        dw = dw2.view(cout, cin, 1, 1) if ctx.needs_input_grad[1] else None
        return dx, dw
    gy = gy.contiguous(memory_format=torch.channels_last)
    mask = [ctx.needs_input_grad[0], ctx.needs_input_grad[1], False]
    dx, dw, _ = torch.ops.aten.convolution_backward(gy, x, w, None, [1, 1], [0, 0], [1, 1], False, [0, 0], 1, mask)
    return dx, dw


class _Conv1x1StatsFn(torch.autograd.Function):
    """y = conv1x1(x, w) (NHWC bf16) and the [4, Cout] BN statistics of y (non-differentiable)."""

    @staticmethod
    def forward(ctx, x, w, bn_weight, bn_bias, running_mean, running_var, nbt, momentum: float, eps: float,
                tickets, tile: int, link=None):
        n, cin, h, wd = x.shape
        cout = w.shape[0]
        x2 = x.permute(0, 2, 3, 1).reshape(n * h * wd, cin)  # channels_last storage: a view
        y2, stats = native().conv1x1_bn_stats(x2, w.reshape(cout, cin), bn_weight, bn_bias, running_mean,
                                              running_var, nbt, momentum, eps, tickets, tile)
        ctx.link = link
        ctx.save_for_backward(x, w, y2 if link is not None else None)
        ctx.mark_non_differentiable(stats)
        return y2.view(n, h, wd, cout).permute(0, 3, 1, 2), stats

    @staticmethod
    def backward(ctx, gy, _gstats):
        x, w, y2 = ctx.saved_tensors
        return *_conv_backward(ctx, gy, x, w, y2), *([None] * 10)


class _Conv1x1LinkedFn(torch.autograd.Function):
    """y = conv1x1(x, w) on MIOpen (NHWC bf16) with the linked backward (PTDT_CONVBN_BWD=all where
    MIOpen's forward wins the timing): the backward does not depend on who computed y."""

    @staticmethod
    def forward(ctx, x, w, link):
        y = torch.nn.functional.conv2d(x, w).contiguous(memory_format=torch.channels_last)
        ctx.link = link
        ctx.save_for_backward(x, w, y)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, w, y = ctx.saved_tensors
        y2 = y.permute(0, 2, 3, 1).reshape(-1, w.shape[0])
        return *_conv_backward(ctx, gy, x, w, y2), None


class _PreConv1x1StatsFn(torch.autograd.Function):
    """y = conv1x1(ReLU(pre_bn(x)), w) with pre_bn's training statistics, and the [4, Cout] BN statistics
    of y (non-differentiable); the normalised activation exists only inside the kernels. Backward: the
    tiled link (gy is the consuming BN's masked gradient g), then pre_bn's backward with its ReLU mask
    recomputed from x."""

    @staticmethod
    def forward(ctx, x, pre_weight, pre_bias, pre_rm, pre_rv, pre_nbt, pre_momentum: float, pre_eps: float,
                pre_tickets, w, bn_weight, bn_bias, running_mean, running_var, nbt, momentum: float, eps: float,
                tickets, link):
        C = native()
        n, cin, h, wd = x.shape
        cout = w.shape[0]
        pstats = C.bn_fwd_stats(x, pre_weight, pre_bias, pre_rm, pre_rv, pre_nbt, pre_momentum, pre_eps, pre_tickets)
        x2 = x.permute(0, 2, 3, 1).reshape(n * h * wd, cin)  # channels_last storage: a view
        y2, stats = C.conv1x1_pre_bn_stats(x2, pstats, w.reshape(cout, cin), bn_weight, bn_bias, running_mean,
                                           running_var, nbt, momentum, eps, tickets)
        ctx.link = link
        ctx.pre_tickets = pre_tickets
        ctx.params = (pre_weight, pre_bias)
        ctx.save_for_backward(x, pre_weight, w, pstats, y2)
        ctx.mark_non_differentiable(stats)
        return y2.view(n, h, wd, cout).permute(0, 3, 1, 2), stats

    @staticmethod
    def backward(ctx, gy, _gstats):
        x, pre_weight, w, pstats, y2 = ctx.saved_tensors
        link = ctx.link
        if link.coef is None:
            raise RuntimeError("conv_bn_act(pre_bn=): the consuming BN's linked backward did not run")
        coef, link.coef = link.coef, None
        C = native()
        n, cin, h, wd = x.shape
        cout = w.shape[0]
        g2 = gy.permute(0, 2, 3, 1).reshape(-1, cout)
        if not g2.is_contiguous():
            g2 = g2.contiguous()
        x2 = x.permute(0, 2, 3, 1).reshape(-1, cin)
        da2, dw2 = C.conv1x1_bwd_tiled(g2, y2, x2, w.reshape(cout, cin), coef, pstats[2:4])
        da = _like(da2.view(n, h, wd, cin).permute(0, 3, 1, 2), x)  # the gradient of ReLU(pre_bn(x))
        want_dw = pre_weight is not None and (ctx.needs_input_grad[1] or ctx.needs_input_grad[2])
        sinks = [None, None]
        if want_dw:  # DDP grad sinks, as ops/norm.py's _bwd_inputs
            for k, p in enumerate(ctx.params):
                if p is not None and p.grad is None and getattr(p, "_ptdt_grad_sink", None) is not None:
                    sinks[k] = p._ptdt_grad_sink()
        dx, dpw, dpb, _ = C.bn_bwd(da, x, None, pre_weight, pstats, True, False, want_dw, ctx.pre_tickets, sinks[0],
                                   sinks[1], None, None)
        return (dx if ctx.needs_input_grad[0] else None, dpw if want_dw else None, dpb if want_dw else None,
                *([None] * 6), dw2.view(cout, cin, 1, 1) if ctx.needs_input_grad[9] else None, *([None] * 9))


class _Conv1x1S2StatsFn(torch.autograd.Function):
    """y = conv1x1(x, w, stride 2) (NHWC bf16, csrc/kernels/conv1x1_s2.hip) and the [4, Cout] BN statistics of y
    (non-differentiable). Backward: linked (gy is the BN's masked gradient g, ctx.link holds the coefficients) on
    the same file's kernels, whose dx is dense; or plain (gy is dY: MIOpen, as autograd would call it)."""

    @staticmethod
    def forward(ctx, x, w, bn_weight, bn_bias, running_mean, running_var, nbt, momentum: float, eps: float, tickets,
                link=None):
        y, stats = native().conv1x1_s2_bn_stats(x, w.reshape(w.shape[0], w.shape[1]), bn_weight, bn_bias,
                                                running_mean, running_var, nbt, momentum, eps, tickets)
        ctx.link = link
        ctx.save_for_backward(x, w, y if link is not None else None)
        ctx.mark_non_differentiable(stats)
        return y, stats

    @staticmethod
    def backward(ctx, gy, _gstats):
        x, w, y = ctx.saved_tensors
        link = ctx.link
        gy = gy.contiguous(memory_format=torch.channels_last)
        if link is not None and link.coef is not None:
            coef, link.coef = link.coef, None
            dx, dw = native().conv1x1_s2_bwd(gy, y, x, w.reshape(w.shape[0], w.shape[1]), coef)
            dw = dw.view_as(w)
        else:
            mask = [ctx.needs_input_grad[0], ctx.needs_input_grad[1], False]
            dx, dw, _ = torch.ops.aten.convolution_backward(gy, x, w, None, [2, 2], [0, 0], [1, 1], False, [0, 0], 1,
                                                            mask)
        return (dx if ctx.needs_input_grad[0] else None), (dw if ctx.needs_input_grad[1] else None), *([None] * 9)


def _pre_fusable(conv: nn.Conv2d, pre_bn: nn.Module, x: torch.Tensor) -> bool:
    """conv_bn_act(pre_bn=) on top of _fusable(conv, bn, x, residual): a local training BatchNorm2d over the
    native layout, grad mode (the fusion's point is the backward's saved activation), a shape with a kernel."""
    if not (_PRE and torch.is_grad_enabled() and isinstance(pre_bn, BatchNorm2d) and pre_bn.training
            and pre_bn.momentum is not None and not synchronizing(pre_bn)):
        return False
    cin, cout = conv.in_channels, conv.out_channels
    if pre_bn.num_features != cin or not _rows_layout_ok(x) or (cin, cout) in _PRE_SKIP:
        return False
    return native().conv1x1_pre_supported(cin, cout)


def _fusable(conv: nn.Conv2d, bn: nn.Module, x: torch.Tensor, residual, stride=(1, 1)) -> bool:
    if not (_ENABLED and isinstance(bn, BatchNorm2d) and bn.training and bn.momentum is not None):
        return False
    if synchronizing(bn):  # the epilogue's statistics (and the ConvBwdLink backward) are this rank's only
        return False
    if not (isinstance(conv, nn.Conv2d) and conv.kernel_size == (1, 1) and conv.stride == stride
            and conv.padding == (0, 0) and conv.dilation == (1, 1) and conv.groups == 1 and conv.bias is None
            and conv.padding_mode == "zeros"):
        return False
    if not (x.is_cuda and x.dim() == 4 and torch.is_autocast_enabled("cuda")
            and torch.get_autocast_dtype("cuda") == torch.bfloat16 and x.dtype == torch.bfloat16
            and x.is_contiguous(memory_format=torch.channels_last) and x.data_ptr() % 16 == 0):
        return False
    cin, cout = conv.in_channels, conv.out_channels
    if cin % 64 or cout % 8 or x.shape[0] * x.shape[2] * x.shape[3] >= 2 ** 31:
        return False
    if residual is not None:  # the BN's native path needs the residual in the output's layout
        n, _, h, w = x.shape
        if not (residual.dtype == torch.bfloat16 and tuple(residual.shape) == (n, cout, h, w)
                and residual.is_contiguous(memory_format=torch.channels_last) and residual.data_ptr() % 16 == 0):
            return False
    return True


def _time_us(fn, reps: int = 3) -> float:
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    best = float("inf")
    for _ in range(reps):
        s.record()
        fn()
        e.record()
        e.synchronize()
        best = min(best, s.elapsed_time(e) * 1e3)
    return best


def _timed_choice(family: str, key: tuple, mode: str, device, arms) -> bool:
    """``mode`` on: fused. auto: time, once per ``key``, the fused conv + statistics kernel + the BN apply
    pass against MIOpen's convolution + the BN's statistics and apply passes on the live operands
    (``arms()`` builds the two callables: scratch statistics, no running-stat side effects), and keep the
    faster. Inside a graph capture an unseen shape keeps the unfused path."""
    if mode in ("1", "on"):
        return True
    from ..utils import tuning

    hit = tuning.lookup(family, key)  # (a decision valid here: see tuning.lookup)
    if hit is not None:
        return hit == "fused"
    pin = tuning.pinned(family, key)
    if pin is not None:
        return pin == "fused"
    if torch.cuda.is_current_stream_capturing():
        return False
    local = tuning.local_choice(family, key)
    if local is not None:  # timed before outside any scope: agree it, no second timing
        return tuning.agree(family, key, local, ("unfused", "fused"), device) == "fused"
    fused, plain = arms()
    with torch.no_grad():  # interleaved, best of 5 each; near-ties (< 3 %) keep MIOpen's path
        tf, tp = float("inf"), float("inf")
        for _ in range(5):
            tf, tp = min(tf, _time_us(fused, 1)), min(tp, _time_us(plain, 1))
    local = "fused" if tf < 0.97 * tp else "unfused"
    # rank 0's choice on every rank: DDP replicas must run the same BN statistics path (utils/tuning.py)
    return tuning.agree(family, key, local, ("unfused", "fused"), device) == "fused"


def _fused_wins(x: torch.Tensor, w: torch.Tensor, tile: int) -> bool:
    """PTDT_CONVBN for a 1x1 convolution, per (M, K, N, tile): :func:`_timed_choice`."""
    n, cin, h, wd = x.shape
    cout = w.shape[0]
    key = (n * h * wd, cin, cout, tile)

    def arms():
        C = native()
        x2 = x.detach().permute(0, 2, 3, 1).reshape(-1, cin)
        w2 = w.detach().reshape(cout, cin)
        tickets = torch.zeros(C.conv1x1_bn_num_tickets(key[0], cout, tile, cin), dtype=torch.int32, device=x.device)

        def fused():
            y2, st = C.conv1x1_bn_stats(x2, w2, None, None, None, None, None, 0.1, 1e-5, tickets, tile)
            C.bn_fwd_apply(y2, st, None, True, False)

        def plain():
            y = torch.nn.functional.conv2d(x.detach(), w.detach())
            C.bn_fwd_train(y, None, None, None, None, None, None, True, 0.1, 1e-5, None, False)

        return fused, plain

    return _timed_choice("convbn", key, _MODE, x.device, arms)


def _conv3x3_link(cin: int, cout: int) -> ConvBwdLink | None:
    """The link for a cin -> cout 3x3 convolution (PTDT_CONV3X3_BWD), or None."""
    if not (_C3X3_BWD and torch.is_grad_enabled()) or (cin, cout) in _C3X3_BWD_SKIP:
        return None
    return ConvBwdLink() if native().conv3x3_bwd_supported(cin, cout) else None


def _conv3x3_backward(ctx, gy, x, w, y):
    """(dx, dw) of y = conv3x3(x, w): linked (gy is the BN's masked gradient g, ctx.link holds the coefficients:
    csrc/kernels/conv3x3_bwd.hip) or plain (gy is dY: MIOpen, as autograd would call it)."""
    link = ctx.link
    gy = gy.contiguous(memory_format=torch.channels_last)
    if link is not None and link.coef is not None:
        coef, link.coef = link.coef, None
        dx, dw = native().conv3x3_bwd(gy, y, x, w, coef)
        return (dx if ctx.needs_input_grad[0] else None), (dw if ctx.needs_input_grad[1] else None)
    mask = [ctx.needs_input_grad[0], ctx.needs_input_grad[1], False]
    dx, dw, _ = torch.ops.aten.convolution_backward(gy, x, w, None, [1, 1], [1, 1], [1, 1], False, [0, 0], 1, mask)
    return dx, dw


class _Conv3x3StatsFn(torch.autograd.Function):
    """y = conv3x3(x, w), stride 1, padding 1 (NHWC bf16, csrc/kernels/conv3x3_bn.hip), and the [4, Cout] BN
    statistics of y (non-differentiable). Backward: :func:`_conv3x3_backward`."""

    @staticmethod
    def forward(ctx, x, w, bn_weight, bn_bias, running_mean, running_var, nbt, momentum: float, eps: float, tickets,
                link=None):
        y, stats = native().conv3x3_bn_stats(x, w, bn_weight, bn_bias, running_mean, running_var, nbt, momentum, eps,
                                             tickets)
        ctx.link = link
        ctx.save_for_backward(x, w, y if link is not None else None)
        ctx.mark_non_differentiable(stats)
        return y, stats

    @staticmethod
    def backward(ctx, gy, _gstats):
        x, w, y = ctx.saved_tensors
        return *_conv3x3_backward(ctx, gy, x, w, y), *([None] * 9)


class _Conv3x3LinkedFn(torch.autograd.Function):
    """y = conv3x3(x, w) on MIOpen (NHWC bf16) with the linked backward (PTDT_CONV3X3_BWD where PTDT_CONV3X3 is 0 or
    MIOpen's forward won the timing): the backward does not depend on who computed y."""

    @staticmethod
    def forward(ctx, x, w, link):
        y = torch.nn.functional.conv2d(x, w, padding=1).contiguous(memory_format=torch.channels_last)
        ctx.link = link
        ctx.save_for_backward(x, w, y)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, w, y = ctx.saved_tensors
        return *_conv3x3_backward(ctx, gy, x, w, y), None


def _conv3x3_fusable(conv: nn.Conv2d, bn: nn.Module, x: torch.Tensor) -> bool:
    """PTDT_CONV3X3 / PTDT_CONV3X3_BWD: a plain stride-1 3x3 convolution feeding a local training BatchNorm2d over
    the native layout, a shape csrc/kernels/conv3x3_bn.hip and conv3x3_bwd.hip take."""
    if (_C3X3 == "0" and not _C3X3_BWD) or not (isinstance(bn, BatchNorm2d) and bn.training
                                                 and bn.momentum is not None):
        return False
    if synchronizing(bn):
        return False
    if not (isinstance(conv, nn.Conv2d) and conv.kernel_size == (3, 3) and conv.stride == (1, 1)
            and conv.padding == (1, 1) and conv.dilation == (1, 1) and conv.groups == 1 and conv.bias is None
            and conv.padding_mode == "zeros"):
        return False
    if not (x.is_cuda and x.dim() == 4 and torch.is_autocast_enabled("cuda")
            and torch.get_autocast_dtype("cuda") == torch.bfloat16 and x.dtype == torch.bfloat16
            and x.is_contiguous(memory_format=torch.channels_last) and x.data_ptr() % 16 == 0):
        return False
    if x.shape[0] * x.shape[2] * x.shape[3] >= 2 ** 31:
        return False
    return native().conv3x3_bn_supported(conv.in_channels, conv.out_channels)


def _conv3x3_wins(x: torch.Tensor, conv: nn.Conv2d) -> bool:
    """PTDT_CONV3X3 for a 3x3 convolution, per (N, H, W, Cin, Cout): :func:`_timed_choice`. The weight is cast
    only where a shape is timed: a cached choice costs no copy."""
    n, cin, h, wd = x.shape
    cout = conv.out_channels

    def arms():
        C = native()
        xd = x.detach()
        wdt = conv.weight.detach().to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
        tickets = torch.zeros(C.conv3x3_bn_num_tickets(n * h * wd, cin, cout), dtype=torch.int32, device=x.device)

        def fused():
            y, st = C.conv3x3_bn_stats(xd, wdt, None, None, None, None, None, 0.1, 1e-5, tickets)
            C.bn_fwd_apply(y, st, None, True, False)

        def plain():
            y = torch.nn.functional.conv2d(xd, wdt, padding=1)
            C.bn_fwd_train(y, None, None, None, None, None, None, True, 0.1, 1e-5, None, False)

        return fused, plain

    return _timed_choice("conv3x3bn", (n, h, wd, cin, cout), _C3X3, x.device, arms)


def _conv3x3_bn_act(conv: nn.Conv2d, bn: nn.Module, x: torch.Tensor, relu: bool, link: bool):
    """The native 3x3 paths of conv_bn_act: the fused forward (PTDT_CONV3X3) and / or the linked backward
    (PTDT_CONV3X3_BWD); None: neither applies (the knob is 0 or MIOpen won the timing; no link)."""
    clink = _conv3x3_link(conv.in_channels, conv.out_channels)
    fused = _C3X3 != "0" and _conv3x3_wins(x, conv)
    if not fused and clink is None:
        return None
    w = cast_weight(conv.weight)
    if not w.is_contiguous(memory_format=torch.channels_last):
        w = w.contiguous(memory_format=torch.channels_last)  # [Cout, 3, 3, Cin] storage: a tiny copy
    if not fused:  # MIOpen's forward, the BN's own statistics, the linked backward
        return batch_norm_act(_Conv3x3LinkedFn.apply(x, w, clink), bn, None, relu, link, conv_link=clink)
    M = x.shape[0] * x.shape[2] * x.shape[3]
    tickets = bn._gemm_tickets
    need = native().conv3x3_bn_num_tickets(M, conv.in_channels, conv.out_channels)
    if tickets.numel() < need or tickets.device != x.device:
        raise RuntimeError(f"conv_bn_act: BN ticket buffer too small ({tickets.numel()} < {need}) or off-device")
    track = bn.track_running_stats
    y, stats = _Conv3x3StatsFn.apply(x, w, bn.weight, bn.bias, bn.running_mean if track else None,
                                     bn.running_var if track else None, bn.num_batches_tracked if track else None,
                                     float(bn.momentum), float(bn.eps), tickets, clink)
    return batch_norm_act(y, bn, None, relu, link, stats=stats, conv_link=clink)


def _conv1x1_s2_bn_act(conv: nn.Conv2d, bn: nn.Module, x: torch.Tensor, relu: bool, link: bool):
    """The native stride-2 1x1 path of conv_bn_act (PTDT_CONVBN_S2): the gathered-row forward with the statistics
    in its epilogue, the BN's apply pass, and the linked backward where PTDT_CONVBN_BWD allows."""
    cin, cout = conv.in_channels, conv.out_channels
    Mout = x.shape[0] * ((x.shape[2] + 1) // 2) * ((x.shape[3] + 1) // 2)
    tickets = bn._gemm_tickets
    need = native().conv1x1_s2_num_tickets(Mout, cin, cout)
    if tickets.numel() < need or tickets.device != x.device:
        raise RuntimeError(f"conv_bn_act: BN ticket buffer too small ({tickets.numel()} < {need}) or off-device")
    clink = ConvBwdLink() if _BWD and torch.is_grad_enabled() and (cin, cout) not in _BWD_SKIP else None
    track = bn.track_running_stats
    y, stats = _Conv1x1S2StatsFn.apply(x, cast_weight(conv.weight), bn.weight, bn.bias,
                                       bn.running_mean if track else None, bn.running_var if track else None,
                                       bn.num_batches_tracked if track else None, float(bn.momentum), float(bn.eps),
                                       tickets, clink)
    return batch_norm_act(y, bn, None, relu, link, stats=stats, conv_link=clink)


def conv_bn_act(conv: nn.Conv2d, bn: nn.Module, x: torch.Tensor, residual: torch.Tensor | None = None,
                relu: bool = False, link: bool = False, pre_bn: nn.Module | None = None) -> torch.Tensor:
    """``ReLU?(bn(conv(x)) + residual)``; a stride-1 1x1 ``conv`` feeding an ops.norm.BatchNorm2d in
    training under bf16 autocast computes the BN statistics in its GEMM epilogue. ``pre_bn``: ``x`` is the raw
    input of that BatchNorm and ``conv`` takes ``ReLU(pre_bn(x))``, applied inside the convolution's kernels
    where PTDT_CONVBN_PRE allows (module docstring), else composed. A stride-1 3x3 ``conv`` (no residual, no
    ``pre_bn``) takes the native implicit GEMM where PTDT_CONV3X3 allows, and the native linked backward where
    PTDT_CONV3X3_BWD does. A stride-2, padding-0 1x1 ``conv`` (no residual, no ``pre_bn``) takes the native
    gathered-row kernels where PTDT_CONVBN_S2 allows."""
    if pre_bn is not None:
        if not (_fusable(conv, bn, x, residual) and _pre_fusable(conv, pre_bn, x)):
            from ..models.resnet import bn_act

            return conv_bn_act(conv, bn, bn_act(pre_bn, x, relu=True), residual, relu, link)
        M = x.shape[0] * x.shape[2] * x.shape[3]
        cin, cout = conv.in_channels, conv.out_channels
        tickets = bn._gemm_tickets
        need = native().conv1x1_pre_num_tickets(M, cin, cout)
        if tickets.numel() < need or tickets.device != x.device:
            raise RuntimeError(f"conv_bn_act: BN ticket buffer too small ({tickets.numel()} < {need}) or off-device")
        clink = ConvBwdLink(tiled=True)
        ptrack, track = pre_bn.track_running_stats, bn.track_running_stats
        y, stats = _PreConv1x1StatsFn.apply(
            x, pre_bn.weight, pre_bn.bias, pre_bn.running_mean if ptrack else None,
            pre_bn.running_var if ptrack else None, pre_bn.num_batches_tracked if ptrack else None,
            float(pre_bn.momentum), float(pre_bn.eps), _tickets_of(pre_bn, x), cast_weight(conv.weight), bn.weight,
            bn.bias, bn.running_mean if track else None, bn.running_var if track else None,
            bn.num_batches_tracked if track else None, float(bn.momentum), float(bn.eps), tickets, clink)
        return batch_norm_act(y, bn, residual, relu, link, stats=stats, conv_link=clink)
    if residual is None and _conv3x3_fusable(conv, bn, x):
        out = _conv3x3_bn_act(conv, bn, x, relu, link)
        if out is not None:
            return out
    if (_S2 and residual is None and _fusable(conv, bn, x, None, stride=(2, 2))
            and native().conv1x1_s2_supported(conv.in_channels, conv.out_channels)):
        return _conv1x1_s2_bn_act(conv, bn, x, relu, link)
    if not _fusable(conv, bn, x, residual):
        from ..models.resnet import bn_act

        return bn_act(bn, conv(x), residual, relu, link)
    M = x.shape[0] * x.shape[2] * x.shape[3]
    tile = _tile(M, conv.out_channels, conv.in_channels)
    w = cast_weight(conv.weight)
    cin, cout = conv.in_channels, conv.out_channels
    if not _fused_wins(x, w, tile):
        clink = _bwd_link(cin, cout) if _BWD_TILED else None
        if clink is not None:  # MIOpen's forward, the BN's own statistics, the linked backward
            y = _Conv1x1LinkedFn.apply(x, w, clink)
            return batch_norm_act(y, bn, residual, relu, link, conv_link=clink)
        from ..models.resnet import bn_act

        return bn_act(bn, conv._conv_forward(x, w, None), residual, relu, link)
    track = bn.track_running_stats
    tickets = bn._gemm_tickets
    need = native().conv1x1_bn_num_tickets(M, conv.out_channels, tile, conv.in_channels)
    if tickets.numel() < need or tickets.device != x.device:
        raise RuntimeError(f"conv_bn_act: BN ticket buffer too small ({tickets.numel()} < {need}) or off-device")
    clink = _bwd_link(cin, cout)
    y, stats = _Conv1x1StatsFn.apply(x, w, bn.weight, bn.bias, bn.running_mean if track else None,
                                     bn.running_var if track else None, bn.num_batches_tracked if track else None,
                                     float(bn.momentum), float(bn.eps), tickets, tile, clink)
    return batch_norm_act(y, bn, residual, relu, link, stats=stats, conv_link=clink)


def conv1x1_stats_probe(x2: torch.Tensor, w2: torch.Tensor, tile: int | None = None):
    """Callable running the fused GEMM + statistics kernel alone on [M, K] x [N, K]^T (benchmarks)."""
    M, N, K = x2.shape[0], w2.shape[0], x2.shape[1]
    t = _tile(M, N, K) if tile is None else tile
    tickets = torch.zeros(native().conv1x1_bn_num_tickets(M, N, t, K), dtype=torch.int32, device=x2.device)
    return lambda: native().conv1x1_bn_stats(x2, w2, None, None, None, None, None, 0.1, 1e-5, tickets, t)
