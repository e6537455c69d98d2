"""Linked backward of BN(conv3x3(x)) (csrc/kernels/conv3x3_bwd.hip, PTDT_CONV3X3_BWD) against float64 gradients
of the bf16 operands, its rejections, and the Bottleneck with the knob on against the knob off."""
import copy
import functools

import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

CL = dict(memory_format=torch.channels_last)


def _operands(dev, N, H, W, Cin, Cout):
    g = torch.Generator().manual_seed(N + H + W + Cin + Cout)

    def act(c):
        return torch.randn(N, c, H, W, generator=g).to(torch.bfloat16).to(dev).contiguous(**CL)

    gy, y, x = act(Cout), act(Cout), act(Cin)
    w = (torch.randn(Cout, Cin, 3, 3, generator=g) * (9 * Cout) ** -0.5).to(torch.bfloat16).to(dev).contiguous(**CL)
    coef = (torch.randn(3, Cout, generator=g) * torch.tensor([[1.0], [0.3], [0.1]])).to(dev)
    return gy, y, x, w, coef


@functools.lru_cache(maxsize=None)
def _reference(shape):
    """float64 on the CPU, once per shape: dy = bf16(A g + B y + C), then the convolution's two gradients."""
    gy, y, x, w, coef = _operands("cpu", *shape)
    k = coef.view(3, 1, -1, 1, 1)
    dy = torch.addcmul(torch.addcmul(k[2], k[1], y.float()), k[0], gy.float()).to(torch.bfloat16).double()
    return (torch.nn.grad.conv2d_input(x.shape, w.double(), dy, padding=1),
            torch.nn.grad.conv2d_weight(x.double(), w.shape, dy, padding=1))


@pytest.mark.parametrize("tile", [64, 128])
@pytest.mark.parametrize("shape", [(1, 1, 1, 64, 64), (3, 1, 6, 64, 64), (3, 5, 7, 64, 128), (2, 9, 9, 128, 192),
                                   (2, 9, 9, 192, 128), (7, 23, 19, 64, 64), (5, 14, 14, 256, 256),
                                   (8, 7, 7, 512, 512)])
def test_conv3x3_bwd_matches_reference(native, dev, shape, tile):
    """(N, H, W, Cin, Cout) against the float64 gradients at the bounds of test_conv1x1_bwd_tiled_matches_reference;
    C != 0 would show an outside tap that leaked into dX. tile: the weight-gradient instance (64: three taps per
    workgroup, 128: one). Two launches bit-identical."""
    assert native.conv3x3_bwd_supported(*shape[3:])
    gy, y, x, w, coef = _operands(dev, *shape)
    dx_ref, dw_ref = _reference(shape)
    dx, dw = native.conv3x3_bwd(gy, y, x, w, coef, tile)
    assert dx.shape == x.shape and dw.shape == w.shape and dx.dtype == dw.dtype == torch.bfloat16
    assert dx.is_contiguous(**CL) and dw.is_contiguous(**CL)
    torch.testing.assert_close(dx.double().cpu(), dx_ref, rtol=2e-2, atol=2e-2)
    assert float((dw.double().cpu() - dw_ref).abs().max()) <= 1e-2 * float(dw_ref.abs().max())
    dx2, dw2 = native.conv3x3_bwd(gy, y, x, w, coef, tile)
    assert torch.equal(dx, dx2) and torch.equal(dw, dw2)


def test_conv3x3_bwd_rejects(native, dev):
    for cin, cout in [(96, 64), (64, 72), (32, 64), (2048, 64)]:
        assert not native.conv3x3_bwd_supported(cin, cout)
    with pytest.raises(RuntimeError):  # unsupported shape
        native.conv3x3_bwd(*_operands(dev, 2, 5, 5, 96, 64))
    gy, y, x, w, coef = _operands(dev, 2, 9, 9, 128, 128)
    with pytest.raises(RuntimeError):  # NCHW-contiguous x
        native.conv3x3_bwd(gy, y, x.contiguous(), w, coef)
    with pytest.raises(RuntimeError):  # weight not channels_last-contiguous
        native.conv3x3_bwd(gy, y, x, w.contiguous(), coef)
    with pytest.raises(RuntimeError):  # coef of another shape
        native.conv3x3_bwd(gy, y, x, w, coef[:2].contiguous())


@pytest.mark.parametrize("inplanes,planes,side,stride,fwd", [
    (256, 64, 14, 1, "on"), (256, 64, 14, 1, "0"), (512, 128, 7, 1, "on"), (512, 128, 7, 1, "0"),
    (256, 128, 28, 2, "0")])
def test_bottleneck_conv3x3_bwd_matches_composed(native, dev, monkeypatch, inplanes, planes, side, stride, fwd):
    """PTDT_CONV3X3_BWD on vs off behind the native forward (fwd on) and behind MIOpen's (fwd 0), set up as
    test_bottleneck_conv3x3_matches_composed: output and every gradient within 3e-2 of max-abs; on, the kernel runs
    once and bn2 runs bn_bwd_reduce instead of bn_bwd. A stride-2 block never reaches the kernel and its gradients
    are the knob-off ones bit for bit."""
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
    for name in ("conv3x3_bwd", "bn_bwd_reduce", "bn_bwd"):
        def counted(*args, _real=getattr(native, name), _name=name):
            calls[_name] = calls.get(_name, 0) + 1
            return _real(*args)

        monkeypatch.setattr(native, name, counted)
    for flag, value in (("_ENABLED", True), ("_MODE", "on"), ("_BWD", True), ("_BWD_TILED", True), ("_PRE", False),
                        ("_C3X3", fwd), ("_C3X3_BWD_SKIP", set())):
        monkeypatch.setattr(convbn, flag, value)
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)  # MIOpen's stride-2 3x3 sums with atomics
    outs, grads, counts = [], [], []
    for blk, knob in ((a, True), (b, False)):
        monkeypatch.setattr(convbn, "_C3X3_BWD", knob)
        calls.clear()
        xi = x.clone().requires_grad_()
        with torch.autocast("cuda", torch.bfloat16):
            yv = blk(xi)
        (yv.float() ** 2).mean().backward()
        outs.append(yv.detach().float())
        grads.append([xi.grad.float()] + [p.grad.float() for p in blk.parameters()])
        counts.append(dict(calls))
    assert "conv3x3_bwd" not in counts[1]
    if stride == 2:
        assert counts[0] == counts[1]
        assert all(torch.equal(ga, gb) for ga, gb in zip([outs[0]] + grads[0], [outs[1]] + grads[1]))
        return
    assert counts[0]["conv3x3_bwd"] == 1
    assert counts[0]["bn_bwd_reduce"] == counts[1]["bn_bwd_reduce"] + 1  # bn2 moved from bn_bwd ...
    assert counts[0].get("bn_bwd", 0) == 0 and counts[1]["bn_bwd"] == 1   # ... the block's only full backward
    for ga, gb in zip([outs[0]] + grads[0], [outs[1]] + grads[1]):
        assert float((ga - gb).abs().max()) / max(float(gb.abs().max()), 1e-6) < 3e-2
