"""3x3 convolution + BN statistics on the native implicit GEMM (csrc/kernels/conv3x3_bn.hip, PTDT_CONV3X3) against
a float64 convolution: the output and its statistics, the rejections, and the Bottleneck with the knob on against
the knob off."""
import copy

import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

CL = dict(memory_format=torch.channels_last)


def _operands(dev, N, H, W, Cin, Cout):
    g = torch.Generator(device=dev).manual_seed(N + H + W + Cin + Cout)
    x = torch.randn(N, Cin, H, W, device=dev, generator=g).to(torch.bfloat16).contiguous(**CL)
    w = (torch.randn(Cout, Cin, 3, 3, device=dev, generator=g) * (9 * Cin) ** -0.5).to(torch.bfloat16).contiguous(**CL)
    return x, w


@pytest.mark.parametrize("tile", [0, 128])
@pytest.mark.parametrize("N,H,W,Cin,Cout", [(1, 1, 1, 64, 64), (3, 1, 6, 64, 64), (3, 5, 7, 64, 128),
                                            (2, 9, 9, 128, 192), (5, 14, 14, 256, 256), (8, 7, 7, 512, 512)])
def test_conv3x3_bn_stats_matches_reference(native, dev, N, H, W, Cin, Cout, tile):
    """Y against a float64 convolution of the bf16 operands at the bf16-product bound of
    test_conv1x1_pre_forward_matches_reference; mean / invstd / scale / shift / running buffers against float64
    statistics of the kernel's own stored Y at that test's bounds (M = 1: the biased variance, as the kernel calls
    bn_finish_channel); two launches bit-identical; tickets re-armed. tile 0 is the shape's own channel tile (64
    for every case here), 128 the other instance (at Cout = 64 and 192 its tile sticks out of Cout)."""
    assert native.conv3x3_bn_supported(Cin, Cout)
    x, w = _operands(dev, N, H, W, Cin, Cout)
    M = N * H * W
    weight, bias = torch.rand(Cout, device=dev) + 0.5, torch.randn(Cout, device=dev)
    rm, rv = torch.randn(Cout, device=dev), torch.rand(Cout, device=dev) + 0.5
    rm0, rv0 = rm.clone(), rv.clone()
    nbt = torch.zeros((), dtype=torch.long, device=dev)
    tickets = torch.zeros(native.conv3x3_bn_num_tickets(M, Cin, Cout, tile), dtype=torch.int32, device=dev)
    y, stats = native.conv3x3_bn_stats(x, w, weight, bias, rm, rv, nbt, 0.1, 1e-5, tickets, tile)
    assert y.dtype == torch.bfloat16 and y.shape == (N, Cout, H, W) and y.is_contiguous(**CL)
    assert stats.shape == (4, Cout)
    ref = torch.nn.functional.conv2d(x.double().cpu(), w.double().cpu(), padding=1)
    torch.testing.assert_close(y.double().cpu(), ref, rtol=2e-2, atol=2e-2)
    yd = y.double().permute(0, 2, 3, 1).reshape(M, Cout)
    mean = yd.mean(0)
    var = ((yd - mean) ** 2).mean(0)
    invstd = torch.rsqrt(var + 1e-5)
    torch.testing.assert_close(stats[0].double(), mean, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(stats[1].double(), invstd, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(stats[2], (weight.double() * invstd).float(), rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(stats[3], (bias.double() - mean * weight.double() * invstd).float(), rtol=1e-5,
                               atol=1e-5)
    unbiased = var * M / (M - 1) if M > 1 else var
    torch.testing.assert_close(rm, (0.9 * rm0.double() + 0.1 * mean).float(), rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(rv, (0.9 * rv0.double() + 0.1 * unbiased).float(), rtol=1e-5, atol=1e-6)
    assert int(nbt) == 1 and int(tickets.abs().sum()) == 0
    y2, stats2 = native.conv3x3_bn_stats(x, w, weight, bias, rm0.clone(), rv0.clone(), None, 0.1, 1e-5, tickets, tile)
    assert torch.equal(y, y2) and torch.equal(stats, stats2) and int(tickets.abs().sum()) == 0


def test_conv3x3_bn_rejects(native, dev):
    for cin, cout in [(96, 64), (64, 72), (32, 64), (2048, 64)]:
        assert not native.conv3x3_bn_supported(cin, cout)
    tickets = torch.zeros(64, dtype=torch.int32, device=dev)

    def run(x, w, tk=tickets):
        return native.conv3x3_bn_stats(x, w, None, None, None, None, None, 0.1, 1e-5, tk)

    with pytest.raises(RuntimeError):  # unsupported shape
        run(*_operands(dev, 2, 5, 5, 96, 64))
    x, w = _operands(dev, 2, 9, 9, 128, 128)
    with pytest.raises(RuntimeError):  # NCHW-contiguous x
        run(x.contiguous(), w)
    with pytest.raises(RuntimeError):  # weight not channels_last-contiguous
        run(x, w.contiguous())
    with pytest.raises(RuntimeError):  # tickets one short
        run(x, w, tickets[:native.conv3x3_bn_num_tickets(2 * 9 * 9, 128, 128) - 1])
    assert int(tickets.abs().sum()) == 0


@pytest.mark.parametrize("inplanes,planes,side,stride", [(256, 64, 14, 1), (512, 128, 7, 1), (256, 128, 28, 2)])
def test_bottleneck_conv3x3_matches_composed(native, dev, monkeypatch, inplanes, planes, side, stride):
    """PTDT_CONV3X3 on vs off (fused 1x1 forwards, as test_bottleneck_pre_matches_composed): output and every
    gradient within 3e-2 of max-abs, bn2's buffers equal; on, the new kernel runs once and bn2 launches no
    bn_fwd_train. A stride-2 block never reaches the kernel and its output is the knob-off output bit for bit."""
    from pytorch_distributed_training_tutorials_amd.models.resnet import Bottleneck, conv1x1
    from pytorch_distributed_training_tutorials_amd.ops import convbn
    from pytorch_distributed_training_tutorials_amd.ops.norm import BatchNorm2d

    torch.manual_seed(3)
    ds = nn.Sequential(conv1x1(inplanes, planes * 4, stride), BatchNorm2d(planes * 4)) if stride == 2 else None
    a = Bottleneck(inplanes, planes, stride=stride, downsample=ds).to(dev).to(**CL)
    for m in a.modules():
        if isinstance(m, nn.BatchNorm2d):
            nn.init.uniform_(m.weight, 0.5, 1.5)
            nn.init.uniform_(m.bias, -0.2, 0.2)
    b = copy.deepcopy(a)
    x = torch.randn(8, inplanes, side, side, device=dev).to(torch.bfloat16).contiguous(**CL)
    calls = {}
    for name in ("conv3x3_bn_stats", "bn_fwd_train"):
        def counted(*args, _real=getattr(native, name), _name=name):
            calls[_name] = calls.get(_name, 0) + 1
            return _real(*args)

        monkeypatch.setattr(native, name, counted)
    monkeypatch.setattr(convbn, "_ENABLED", True)
    monkeypatch.setattr(convbn, "_MODE", "on")
    monkeypatch.setattr(convbn, "_BWD", True)
    monkeypatch.setattr(convbn, "_BWD_TILED", True)
    monkeypatch.setattr(convbn, "_PRE", False)
    # MIOpen's default stride-2 3x3 forward at this shape sums with atomics: 27 distinct results in 30 calls on
    # one input, 1 with the deterministic attribute (measured). The bit-for-bit comparison needs the latter.
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    outs, grads, counts = [], [], []
    for blk, knob in ((a, "on"), (b, "0")):
        monkeypatch.setattr(convbn, "_C3X3", knob)
        calls.clear()
        xi = x.clone().requires_grad_()
        with torch.autocast("cuda", torch.bfloat16):
            yv = blk(xi)
        (yv.float() ** 2).mean().backward()
        outs.append(yv.detach().float())
        grads.append([xi.grad.float()] + [p.grad.float() for p in blk.parameters()])
        counts.append(dict(calls))
    assert "conv3x3_bn_stats" not in counts[1]
    if stride == 2:
        assert "conv3x3_bn_stats" not in counts[0] and counts[0] == counts[1]
        assert torch.equal(outs[0], outs[1])
        return
    # off: bn2 is the block's one bn_fwd_train; on: every BN of the block only applies
    assert counts[0]["conv3x3_bn_stats"] == 1 and counts[0].get("bn_fwd_train", 0) == 0
    assert counts[1]["bn_fwd_train"] == 1
    for ga, gb in zip([outs[0]] + grads[0], [outs[1]] + grads[1]):
        assert float((ga - gb).abs().max()) / max(float(gb.abs().max()), 1e-6) < 3e-2
    for (na, ta), (_, tb) in zip(a.named_buffers(), b.named_buffers()):
        if "tickets" in na:
            assert int(ta.abs().sum()) == 0, na
        elif na.startswith("bn2."):
            torch.testing.assert_close(ta, tb, msg=na)
