"""1x1 convolution with the input BatchNorm + ReLU applied on its operand path (csrc/kernels/conv1x1_pre.hip,
PTDT_CONVBN_PRE=1) against float64 PyTorch: the forward and its output statistics, the weight gradient with
the recomputed operand, the statistics-only BN pass, the rejections, and the Bottleneck with the knob on
against the knob off."""
import copy

import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu


def _operands(dev, M, K, N):
    """x, w, the producing BN's [4, K] statistics (negative scales, one all-zero channel) and the reference
    operand a = bf16(max(x * scale + shift, 0)); a bf16 times an fp32 value is exact in double."""
    g = torch.Generator(device=dev).manual_seed(M + K + N)
    x = torch.randn(M, K, device=dev, generator=g).to(torch.bfloat16)
    w = (torch.randn(N, K, device=dev, generator=g) * K ** -0.5).to(torch.bfloat16)
    pre = torch.randn(4, K, device=dev, generator=g)
    pre[3] *= 0.5
    pre[2:, 3] = 0.0
    a_ref = (x.double() * pre[2].double() + pre[3].double()).float().clamp_min(0).to(torch.bfloat16)
    return x, w, pre, a_ref


@pytest.mark.parametrize("M,K,N", [(37, 64, 64), (131, 128, 192), (1000, 192, 128), (4099, 64, 256),
                                   (1568, 512, 2048)])
def test_conv1x1_pre_forward_matches_reference(native, dev, M, K, N):
    """Y against a_ref . W^T in float64 at the bf16-product bound of test_conv1x1_bwd_tiled_matches_reference;
    mean / invstd / running buffers against float64 statistics of the kernel's own stored Y at the bounds of
    test_gemm_bn_stats_matches_reference (tests/test_convbn_gpu.py); two launches bit-identical; tickets
    re-armed."""
    assert native.conv1x1_pre_supported(K, N)
    x, w, pre, a_ref = _operands(dev, M, K, N)
    weight, bias = torch.rand(N, device=dev) + 0.5, torch.randn(N, device=dev)
    rm, rv = torch.randn(N, device=dev), torch.rand(N, device=dev) + 0.5
    rm0, rv0 = rm.clone(), rv.clone()
    nbt = torch.zeros((), dtype=torch.long, device=dev)
    tickets = torch.zeros(native.conv1x1_pre_num_tickets(M, K, N), dtype=torch.int32, device=dev)
    y, stats = native.conv1x1_pre_bn_stats(x, pre, w, weight, bias, rm, rv, nbt, 0.1, 1e-5, tickets)
    assert y.dtype == torch.bfloat16 and y.shape == (M, N) and stats.shape == (4, N)
    torch.testing.assert_close(y.double(), a_ref.double() @ w.double().t(), rtol=2e-2, atol=2e-2)
    mean = y.double().mean(0)
    var = ((y.double() - mean) ** 2).mean(0)
    invstd = torch.rsqrt(var + 1e-5)
    torch.testing.assert_close(stats[0].double(), mean, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(stats[1].double(), invstd, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(stats[2], (weight.double() * invstd).float(), rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(stats[3], (bias.double() - mean * weight.double() * invstd).float(), rtol=1e-5,
                               atol=1e-5)
    torch.testing.assert_close(rm, (0.9 * rm0.double() + 0.1 * mean).float(), rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(rv, (0.9 * rv0.double() + 0.1 * var * M / (M - 1)).float(), rtol=1e-5, atol=1e-6)
    assert int(nbt) == 1 and int(tickets.abs().sum()) == 0
    y2, stats2 = native.conv1x1_pre_bn_stats(x, pre, w, weight, bias, rm0.clone(), rv0.clone(), None, 0.1, 1e-5,
                                             tickets)
    assert torch.equal(y, y2) and torch.equal(stats, stats2) and int(tickets.abs().sum()) == 0


@pytest.mark.parametrize("M,K,N", [(37, 64, 64), (131, 128, 192), (1000, 192, 128), (100003, 128, 512)])
def test_conv1x1_bwd_tiled_pre_matches_reference(native, dev, M, K, N):
    """dW = dY^T . a_ref in float64 within 1e-2 of max-abs (test_conv1x1_bwd_tiled_matches_reference's bound);
    dX, the operand's gradient, is the call's without pre, bit for bit."""
    x, w, pre, a_ref = _operands(dev, M, K, N)
    gy = torch.randn(M, N, device=dev).to(torch.bfloat16)
    y = torch.randn(M, N, device=dev).to(torch.bfloat16)
    coef = (torch.randn(3, N, device=dev) * torch.tensor([[1.0], [0.3], [0.1]], device=dev)).contiguous()
    dx, dw = native.conv1x1_bwd_tiled(gy, y, x, w, coef, pre[2:4])
    dx0, _ = native.conv1x1_bwd_tiled(gy, y, x, w, coef)
    assert torch.equal(dx, dx0)
    dy = (coef[0] * gy.float() + coef[1] * y.float() + coef[2]).to(torch.bfloat16)
    dw_ref = dy.t().double() @ a_ref.double()
    assert dw.shape == (N, K) and dw.dtype == torch.bfloat16
    assert float((dw.double() - dw_ref).abs().max()) <= 1e-2 * float(dw_ref.abs().max())


@pytest.mark.parametrize("shape", [(8, 64, 28, 28), (3, 136, 7, 5)])
def test_bn_fwd_stats_is_the_statistics_pass(native, dev, shape):
    """The same kernels as bn_fwd_train: statistics, running buffers and counter bit for bit."""
    x = torch.randn(*shape, device=dev).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    C = shape[1]
    weight, bias = torch.rand(C, device=dev) + 0.5, torch.randn(C, device=dev)
    bufs = [[torch.randn(C, device=dev).abs() + 0.1 for _ in range(2)] for _ in range(2)]
    bufs[1] = [b.clone() for b in bufs[0]]
    nbt = [torch.zeros((), dtype=torch.long, device=dev) for _ in range(2)]
    _, ref, _ = native.bn_fwd_train(x, weight, bias, bufs[0][0], bufs[0][1], nbt[0], None, True, 0.1, 1e-5)
    stats = native.bn_fwd_stats(x, weight, bias, bufs[1][0], bufs[1][1], nbt[1], 0.1, 1e-5)
    assert torch.equal(stats, ref) and int(nbt[1]) == 1
    assert torch.equal(bufs[0][0], bufs[1][0]) and torch.equal(bufs[0][1], bufs[1][1])


@pytest.mark.parametrize("K,N", [(96, 128), (128, 72), (32, 64)])
def test_conv1x1_pre_rejects(native, dev, K, N):
    assert not native.conv1x1_pre_supported(K, N)
    tickets = torch.zeros(64, dtype=torch.int32, device=dev)
    x, w, pre, _ = _operands(dev, 100, K, N)
    with pytest.raises(RuntimeError):
        native.conv1x1_pre_bn_stats(x, pre, w, None, None, None, None, None, 0.1, 1e-5, tickets)
    x, w, pre, _ = _operands(dev, 1000, 128, 128)
    with pytest.raises(RuntimeError):  # non-contiguous x
        native.conv1x1_pre_bn_stats(x.t().contiguous().t(), pre, w, None, None, None, None, None, 0.1, 1e-5, tickets)
    short = tickets[:native.conv1x1_pre_num_tickets(1000, 128, 128) - 1]
    with pytest.raises(RuntimeError):
        native.conv1x1_pre_bn_stats(x, pre, w, None, None, None, None, None, 0.1, 1e-5, short)


@pytest.mark.parametrize("inplanes,planes,downsample", [(256, 64, False), (512, 128, False), (256, 128, True)])
def test_bottleneck_pre_matches_composed(native, dev, monkeypatch, inplanes, planes, downsample):
    """PTDT_CONVBN_PRE on vs off (both at PTDT_CONVBN_BWD=all, fused forwards): output, every gradient (bn2's
    parameters included) within 3e-2 of max-abs, bn2's and bn3's buffers equal; on, the new forward runs once and
    bn2 launches neither bn_fwd_train nor an apply pass."""
    from pytorch_distributed_training_tutorials_amd.models.resnet import Bottleneck, conv1x1
    from pytorch_distributed_training_tutorials_amd.ops import convbn
    from pytorch_distributed_training_tutorials_amd.ops.norm import BatchNorm2d

    torch.manual_seed(3)
    ds = nn.Sequential(conv1x1(inplanes, planes * 4), BatchNorm2d(planes * 4)) if downsample else None
    a = Bottleneck(inplanes, planes, downsample=ds).to(dev).to(memory_format=torch.channels_last)
    for m in a.modules():
        if isinstance(m, nn.BatchNorm2d):
            nn.init.uniform_(m.weight, 0.5, 1.5)
            nn.init.uniform_(m.bias, -0.2, 0.2)
    b = copy.deepcopy(a)
    side = 28 if downsample else 14
    x = torch.randn(8, inplanes, side, side, device=dev).to(torch.bfloat16).contiguous(
        memory_format=torch.channels_last)
    calls = {}
    for name in ("conv1x1_pre_bn_stats", "bn_fwd_train", "bn_fwd_apply"):
        def counted(*args, _real=getattr(native, name), _name=name):
            calls[_name] = calls.get(_name, 0) + 1
            return _real(*args)

        monkeypatch.setattr(native, name, counted)
    monkeypatch.setattr(convbn, "_ENABLED", True)
    monkeypatch.setattr(convbn, "_MODE", "on")
    monkeypatch.setattr(convbn, "_BWD", True)
    monkeypatch.setattr(convbn, "_BWD_TILED", True)
    outs, grads, counts = [], [], []
    for blk, pre in ((a, True), (b, False)):
        monkeypatch.setattr(convbn, "_PRE", pre)
        calls.clear()
        xi = x.clone().requires_grad_()
        with torch.autocast("cuda", torch.bfloat16):
            yv = blk(xi)
        (yv.float() ** 2).mean().backward()
        outs.append(yv.detach().float())
        grads.append([xi.grad.float()] + [p.grad.float() for p in blk.parameters()])
        counts.append(dict(calls))
    # off: bn2 is the block's one bn_fwd_train; bn1, bn3 (and the downsample BN) only apply
    assert counts[0].get("conv1x1_pre_bn_stats", 0) == 1 and "conv1x1_pre_bn_stats" not in counts[1]
    assert counts[0].get("bn_fwd_train", 0) == 0 and counts[1]["bn_fwd_train"] == 1
    assert counts[0]["bn_fwd_apply"] == counts[1]["bn_fwd_apply"]
    for ga, gb in zip([outs[0]] + grads[0], [outs[1]] + grads[1]):
        assert float((ga - gb).abs().max()) / max(float(gb.abs().max()), 1e-6) < 3e-2
    for (na, ta), (_, tb) in zip(a.named_buffers(), b.named_buffers()):
        if "tickets" in na:
            assert int(ta.abs().sum()) == 0, na
        elif na.startswith(("bn2.", "bn3.")):
            torch.testing.assert_close(ta, tb, msg=na)
