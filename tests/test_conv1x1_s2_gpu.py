"""Stride-2 1x1 convolution + BN statistics and its linked backward (csrc/kernels/conv1x1_s2.hip, PTDT_CONVBN_S2)
against float64 PyTorch on the bf16 operands, the rejections, and the stride-2 Bottleneck with the knob on against
the knob off."""
import copy

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

CL = dict(memory_format=torch.channels_last)
SHAPES = [(1, 2, 3, 64, 64), (3, 5, 7, 64, 128), (2, 9, 9, 128, 192), (2, 9, 9, 192, 128), (7, 23, 19, 64, 64),
          (8, 14, 14, 1024, 2048)]


def _operands(dev, Nb, H, W, Cin, Cout):
    """x, w, and the backward's g, y, coef (rows scaled 1, 0.3, 0.1: C != 0)."""
    g = torch.Generator(device=dev).manual_seed(Nb + H + W + Cin + Cout)
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    x = torch.randn(Nb, Cin, H, W, device=dev, generator=g).to(torch.bfloat16).contiguous(**CL)
    w = (torch.randn(Cout, Cin, device=dev, generator=g) * Cin ** -0.5).to(torch.bfloat16)
    gy = torch.randn(Nb, Cout, Ho, Wo, device=dev, generator=g).to(torch.bfloat16).contiguous(**CL)
    y = torch.randn(Nb, Cout, Ho, Wo, device=dev, generator=g).to(torch.bfloat16).contiguous(**CL)
    coef = torch.randn(3, Cout, device=dev, generator=g) * torch.tensor([[1.0], [0.3], [0.1]], device=dev)
    return x, w, gy, y, coef


@pytest.mark.parametrize("shape", SHAPES)
def test_conv1x1_s2_forward_matches_reference(native, dev, shape):
    """y against conv2d(stride=2) in float64; statistics, coefficients and running buffers against float64
    statistics of the kernel's own stored y at the bounds of test_conv1x1_pre_forward_matches_reference; tickets
    re-armed; two launches bit-identical."""
    Nb, H, W, K, N = shape
    assert native.conv1x1_s2_supported(K, N)
    x, w = _operands(dev, *shape)[:2]
    weight, bias = torch.rand(N, device=dev) + 0.5, torch.randn(N, device=dev)
    rm, rv = torch.randn(N, device=dev), torch.rand(N, device=dev) + 0.5
    rm0, rv0 = rm.clone(), rv.clone()
    nbt = torch.zeros((), dtype=torch.long, device=dev)
    M = Nb * ((H + 1) // 2) * ((W + 1) // 2)
    tickets = torch.zeros(native.conv1x1_s2_num_tickets(M, K, N), dtype=torch.int32, device=dev)
    y, stats = native.conv1x1_s2_bn_stats(x, w, weight, bias, rm, rv, nbt, 0.1, 1e-5, tickets)
    assert y.dtype == torch.bfloat16 and y.shape == (Nb, N, (H + 1) // 2, (W + 1) // 2) and y.is_contiguous(**CL)
    y_ref = F.conv2d(x.cpu().double(), w.cpu().double()[:, :, None, None], stride=2)
    torch.testing.assert_close(y.cpu().double(), y_ref, rtol=2e-2, atol=2e-2)
    yd = y.double()
    mean = yd.mean((0, 2, 3))
    var = ((yd - mean.view(1, -1, 1, 1)) ** 2).mean((0, 2, 3))
    invstd = torch.rsqrt(var + 1e-5)
    torch.testing.assert_close(stats[0].double(), mean, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(stats[1].double(), invstd, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(stats[2], (weight.double() * invstd).float(), rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(stats[3], (bias.double() - mean * weight.double() * invstd).float(), rtol=1e-5,
                               atol=1e-5)
    torch.testing.assert_close(rm, (0.9 * rm0.double() + 0.1 * mean).float(), rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(rv, (0.9 * rv0.double() + 0.1 * var * M / (M - 1)).float(), rtol=1e-5, atol=1e-6)
    assert int(nbt) == 1 and int(tickets.abs().sum()) == 0
    y2, stats2 = native.conv1x1_s2_bn_stats(x, w, weight, bias, rm0.clone(), rv0.clone(), None, 0.1, 1e-5, tickets)
    assert torch.equal(y, y2) and torch.equal(stats, stats2) and int(tickets.abs().sum()) == 0


@pytest.mark.parametrize("shape", SHAPES + [(1, 1, 1, 64, 64)])
def test_conv1x1_s2_bwd_matches_reference(native, dev, shape):
    """dx, dw against the float64 gradients of dy = bf16(A g + B y + C) at the bounds of
    test_conv1x1_bwd_tiled_matches_reference; every pixel of dx that no output row reads is exactly zero (C != 0
    would show there); two launches bit-identical."""
    x, w, gy, y, coef = _operands(dev, *shape)
    k = coef.view(3, 1, -1, 1, 1)
    dy = torch.addcmul(torch.addcmul(k[2], k[1], y.float()), k[0], gy.float()).to(torch.bfloat16).cpu().double()
    w4 = w.cpu().double()[:, :, None, None]
    dx_ref = torch.nn.grad.conv2d_input(x.shape, w4, dy, stride=2)
    dw_ref = torch.nn.grad.conv2d_weight(x.cpu().double(), w4.shape, dy, stride=2)[:, :, 0, 0]
    dx, dw = native.conv1x1_s2_bwd(gy, y, x, w, coef)
    assert dx.shape == x.shape and dx.is_contiguous(**CL) and dw.shape == w.shape
    assert dx.dtype == dw.dtype == torch.bfloat16
    torch.testing.assert_close(dx.cpu().double(), dx_ref, rtol=2e-2, atol=2e-2)
    assert float((dw.cpu().double() - dw_ref).abs().max()) <= 1e-2 * float(dw_ref.abs().max())
    assert not dx[:, :, 1::2, :].any() and not dx[:, :, :, 1::2].any()
    dx2, dw2 = native.conv1x1_s2_bwd(gy, y, x, w, coef)
    assert torch.equal(dx, dx2) and torch.equal(dw, dw2)


def test_conv1x1_s2_rejects(native, dev):
    for K, N in [(96, 64), (64, 72), (32, 64), (8192, 64)]:
        assert not native.conv1x1_s2_supported(K, N)
    x, w, gy, y, coef = _operands(dev, 2, 9, 9, 128, 128)
    tickets = torch.zeros(64, dtype=torch.int32, device=dev)
    with pytest.raises(RuntimeError):  # NCHW-contiguous x
        native.conv1x1_s2_bn_stats(x.contiguous(), w, None, None, None, None, None, 0.1, 1e-5, tickets)
    with pytest.raises(RuntimeError):
        native.conv1x1_s2_bwd(gy, y, x.contiguous(), w, coef)
    with pytest.raises(RuntimeError):  # coef of another shape
        native.conv1x1_s2_bwd(gy, y, x, w, coef[:2].contiguous())
    with pytest.raises(RuntimeError):  # y of another spatial size
        native.conv1x1_s2_bwd(gy, y[:, :, :4].contiguous(**CL), x, w, coef)


@pytest.mark.parametrize("inplanes,planes,side", [(256, 128, 28), (512, 256, 13)])
def test_bottleneck_conv1x1_s2_matches_composed(native, dev, monkeypatch, inplanes, planes, side):
    """PTDT_CONVBN_S2 on vs off, set up as test_bottleneck_conv3x3_bwd_matches_composed: output and every gradient
    within 3e-2 of max-abs (the input gradient sums conv1's with the downsample branch's dense dx, which passed
    through grad_link); on, each new binding runs once and the downsample BN runs bn_bwd_reduce instead of bn_bwd;
    off, neither binding runs."""
    from pytorch_distributed_training_tutorials_amd.models.resnet import Bottleneck, conv1x1
    from pytorch_distributed_training_tutorials_amd.ops import convbn
    from pytorch_distributed_training_tutorials_amd.ops.norm import BatchNorm2d

    torch.manual_seed(3)
    ds = nn.Sequential(conv1x1(inplanes, planes * 4, 2), BatchNorm2d(planes * 4))
    a = Bottleneck(inplanes, planes, stride=2, downsample=ds).to(dev).to(**CL)
    for m in a.modules():
        if isinstance(m, nn.BatchNorm2d):
            nn.init.uniform_(m.weight, 0.5, 1.5)
            nn.init.uniform_(m.bias, -0.2, 0.2)
    b = copy.deepcopy(a)
    x = torch.randn(8, inplanes, side, side, device=dev).to(torch.bfloat16).contiguous(**CL)
    calls = {}
    for name in ("conv1x1_s2_bn_stats", "conv1x1_s2_bwd", "bn_bwd_reduce", "bn_bwd"):
        def counted(*args, _real=getattr(native, name), _name=name):
            calls[_name] = calls.get(_name, 0) + 1
            return _real(*args)

        monkeypatch.setattr(native, name, counted)
    for flag, value in (("_ENABLED", True), ("_MODE", "on"), ("_BWD", True), ("_BWD_TILED", True), ("_PRE", False),
                        ("_C3X3", "0"), ("_C3X3_BWD", False), ("_BWD_SKIP", set())):
        monkeypatch.setattr(convbn, flag, value)
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)  # MIOpen's stride-2 3x3 sums with atomics
    outs, grads, counts = [], [], []
    for blk, knob in ((a, True), (b, False)):
        monkeypatch.setattr(convbn, "_S2", knob)
        calls.clear()
        xi = x.clone().requires_grad_()
        with torch.autocast("cuda", torch.bfloat16):
            yv = blk(xi)
        (yv.float() ** 2).mean().backward()
        outs.append(yv.detach().float())
        grads.append([xi.grad.float()] + [p.grad.float() for p in blk.parameters()])
        counts.append(dict(calls))
    assert counts[0]["conv1x1_s2_bn_stats"] == 1 and counts[0]["conv1x1_s2_bwd"] == 1
    assert "conv1x1_s2_bn_stats" not in counts[1] and "conv1x1_s2_bwd" not in counts[1]
    assert counts[0].get("bn_bwd", 0) == counts[1]["bn_bwd"] - 1
    assert counts[0]["bn_bwd_reduce"] == counts[1]["bn_bwd_reduce"] + 1
    for ga, gb in zip([outs[0]] + grads[0], [outs[1]] + grads[1]):
        assert float((ga - gb).abs().max()) / max(float(gb.abs().max()), 1e-6) < 3e-2
