"""SyncBatchNorm on the GPU: the kernel protocol (partial statistics -> merge -> apply; raw sums ->
coefficients -> apply) against a full-batch reference, merge stability, world-1 / eval equality with
BatchNorm2d, the forced path inside a small Bottleneck model, conversion, and two ranks sharing one
GPU. Tolerances: tests/test_norm.py::test_native_bn_train_fwd_bwd's, for the same kernels."""
import functools
import os

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from pytorch_distributed_training_tutorials_amd import native
from pytorch_distributed_training_tutorials_amd.ops import SyncBatchNorm
from pytorch_distributed_training_tutorials_amd.ops.norm import BatchNorm2d
from pytorch_distributed_training_tutorials_amd.parallel.env import free_port
from pytorch_distributed_training_tutorials_amd.parallel.launcher import spawn

from . import _syncbn_workers as W

pytestmark = pytest.mark.gpu

EPS, MOM = 1e-5, 0.1
SHAPES = [(5, 24, 3, 3), (3, 2048, 2, 2), (4, 64, 14, 14), (128, 64, 28, 28)]


def _chunks(M, world):
    """Uneven row counts summing to M: one row each, the remainder spread 1 : 2 : 3 ... over chunks
    1.. (chunk 0 stays exactly one row)."""
    weights = list(range(1, world))
    rest, out = M - world, [1] * world
    for k, w in enumerate(weights[:-1]):
        out[k + 1] += rest * w // sum(weights)
    out[-1] += M - sum(out)
    assert sum(out) == M and min(out) >= 1 and out[0] == 1
    return out


@functools.lru_cache(maxsize=None)
def _case(shape, dtype, relu, res):
    """Inputs (rounded to dtype, NHWC) and the fp32 nn.BatchNorm2d results on the whole batch; computed
    once per (shape, dtype, epilogue) and shared by the world sizes. Nothing here is modified later."""
    dev = torch.device("cuda", 0)
    C = shape[1]
    torch.manual_seed(sum(shape))
    cl = torch.channels_last
    x = (torch.randn(shape, device=dev) * 2 + 3).to(dtype).contiguous(memory_format=cl)
    r = torch.randn(shape, device=dev).to(dtype).contiguous(memory_format=cl) if res else None
    g = torch.randn(shape, device=dev).to(dtype).contiguous(memory_format=cl)
    ref = nn.BatchNorm2d(C, eps=EPS, momentum=MOM).to(dev)
    with torch.no_grad():
        ref.weight.uniform_(0.5, 1.5)
        ref.bias.uniform_(-0.5, 0.5)
        ref.running_mean.uniform_(-1, 1)
    w, b, rm = ref.weight.detach().clone(), ref.bias.detach().clone(), ref.running_mean.detach().clone()
    xr = x.float().clone().requires_grad_()
    rr = r.float().clone().requires_grad_() if res else None
    pre = ref(xr) + (rr if res else 0)
    yr = F.relu(pre) if relu else pre
    yr.backward(g.float())
    return dict(x=x, r=r, g=g, w=w, b=b, rm=rm, pre=pre.detach(), y=yr.detach(), dx=xr.grad,
                dr=rr.grad if res else None, dw=ref.weight.grad, db=ref.bias.grad, running_mean=ref.running_mean,
                running_var=ref.running_var)


def _rows(t):
    """[N, C, H, W] channels_last -> its [M, C] row view."""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


@pytest.mark.parametrize("world", [2, 3, 8])
@pytest.mark.parametrize("relu,res", [(False, False), (True, False), (True, True)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("shape", SHAPES)
def test_kernel_protocol_matches_full_batch(shape, dtype, relu, res, world):
    C = shape[1]  # every channel count here vector-aligns in both dtypes (4 x fp32, 8 x bf16)
    K = native()
    c = _case(shape, dtype, relu, res)
    dev = c["x"].device
    x2, g2 = _rows(c["x"]), _rows(c["g"])
    r2 = _rows(c["r"]) if res else None
    M = x2.shape[0]
    sizes = _chunks(M, world)
    bounds = [(sum(sizes[:k]), sum(sizes[:k + 1])) for k in range(world)]
    # forward: one record per chunk, merge, apply per chunk
    rec = torch.full((world, 2 * C + 1), float("nan"), dtype=torch.float64, device=dev)
    for k, (lo, hi) in enumerate(bounds):
        K.bn_sync_stats(x2[lo:hi], rec[k])
    assert rec[:, 2 * C].tolist() == [float(s) for s in sizes]
    rm, rv = c["rm"].clone(), torch.ones(C, device=dev)
    nbt = torch.zeros((), dtype=torch.long, device=dev)
    stats, count = K.bn_sync_merge(rec, c["w"], c["b"], rm, rv, nbt, MOM, EPS)
    assert float(count) == M and int(nbt) == 1
    ys, masks = [], []
    for lo, hi in bounds:
        y, mask = K.bn_fwd_apply(x2[lo:hi], stats, r2[lo:hi] if res else None, relu, relu and res)
        ys.append(y)
        masks.append(mask if (relu and res) else None)
    y = torch.cat(ys)
    tol = 2e-5 if dtype == torch.float32 else 2e-2
    torch.testing.assert_close(y.float(), _rows(c["y"]), rtol=tol, atol=tol)
    torch.testing.assert_close(rm, c["running_mean"], rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(rv, c["running_var"], rtol=1e-4, atol=1e-5)
    # backward: raw sums per chunk, summed (the all-reduce), coefficients, apply per chunk
    gs, total, dw, db = [], torch.zeros(2, C, dtype=torch.float64, device=dev), 0, 0
    for k, (lo, hi) in enumerate(bounds):
        g, dwk, dbk, sums = K.bn_sync_bwd_reduce(g2[lo:hi], x2[lo:hi], c["w"], stats, relu, True, mask=masks[k])
        gs.append(g)
        total += sums
        dw, db = dw + dwk, db + dbk
    coef = K.bn_sync_coef(total, count, c["w"], stats)
    dx = torch.cat([K.bn_bwd_apply_g(gs[k], x2[lo:hi], coef) for k, (lo, hi) in enumerate(bounds)])
    gtol = 1e-4 if dtype == torch.float32 else 5e-2
    # with ReLU, elements whose reference pre-activation is within 1e-3 of 0 may flip their mask
    keep = (_rows(c["pre"]).abs() > 1e-3) | (not relu)
    left_out = 1.0 - keep.float().mean().item()
    print(f"left out of the dx comparison: {100 * left_out:.4f} %")
    assert left_out < 0.01
    torch.testing.assert_close(dx.float()[keep], _rows(c["dx"])[keep], rtol=gtol, atol=gtol)
    if res:  # the materialised g is the residual gradient
        torch.testing.assert_close(torch.cat(gs).float()[keep], _rows(c["dr"])[keep], rtol=gtol, atol=gtol)
    wtol = 1e-3 * M ** 0.5 if dtype == torch.bfloat16 else 1e-3
    torch.testing.assert_close(dw, c["dw"], rtol=1e-3, atol=wtol)
    torch.testing.assert_close(db, c["db"], rtol=1e-3, atol=wtol)


def test_merge_is_stable_for_large_and_different_chunk_means():
    """Chunk r ~ N(1000 + 10 r, 1): neither the per-chunk shifted sums nor Chan's merge may cancel."""
    K = native()
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    C, sizes = 32, [1, 700, 2500, 895]
    chunks = [torch.randn(m, C, device=dev) + 1000.0 + 10.0 * r for r, m in enumerate(sizes)]
    rec = torch.empty(len(sizes), 2 * C + 1, dtype=torch.float64, device=dev)
    for r, xc in enumerate(chunks):
        K.bn_sync_stats(xc, rec[r])
    stats, count = K.bn_sync_merge(rec, None, None, None, None, None, MOM, EPS)
    x = torch.cat(chunks)
    y = torch.cat([K.bn_fwd_apply(xc, stats, None, False, False)[0] for xc in chunks])
    xd = x.double()
    mean, var = xd.mean(0), xd.var(0, unbiased=False)
    ref = ((xd - mean) / torch.sqrt(var + EPS)).float()
    assert float(count) == sum(sizes)
    torch.testing.assert_close(y, ref, rtol=1e-3, atol=1e-3)
    torch.testing.assert_close(stats[0].double(), mean, rtol=1e-6, atol=0)
    torch.testing.assert_close((1.0 / stats[1].double() ** 2 - EPS), var, rtol=1e-3, atol=0)


@pytest.mark.parametrize("mode", ["train_world1", "eval"])
def test_world_one_and_eval_equal_batchnorm2d(mode, monkeypatch):
    monkeypatch.delenv("PTDT_SYNCBN_FORCE", raising=False)
    dev = torch.device("cuda", 0)
    torch.manual_seed(1)
    x = torch.randn(4, 32, 6, 6, device=dev).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    r = torch.randn_like(x)
    a, b = SyncBatchNorm(32).to(dev), BatchNorm2d(32).to(dev)
    with torch.no_grad():
        a.weight.uniform_(0.5, 1.5)
        a.running_mean.uniform_(-1, 1)
    b.load_state_dict(a.state_dict())
    if mode == "eval":
        a.eval(), b.eval()
    outs = []
    for bn in (a, b):
        xi, ri = x.clone().requires_grad_(), r.clone().requires_grad_()
        y = bn(xi, ri, relu=True)
        y.backward(torch.ones_like(y))
        outs.append((y.detach(), xi.grad, ri.grad, bn.weight.grad, bn.bias.grad, bn.running_mean, bn.running_var))
    assert a.sync_forwards == 0
    for u, v in zip(*outs):
        assert torch.equal(u, v)


class _Stack(nn.Module):
    """Stem + a downsample Bottleneck + an identity-shortcut Bottleneck, as models/resnet.py wires them."""

    def __init__(self):
        super().__init__()
        from pytorch_distributed_training_tutorials_amd.models import resnet as R

        self.conv1 = R.Conv2d(3, 64, kernel_size=3, stride=2, padding=1, bias=False)
        self.bn1 = BatchNorm2d(64)
        self.maxpool = R.MaxPool2d(kernel_size=3, stride=2, padding=1)
        down = nn.Sequential(R.conv1x1(64, 256), BatchNorm2d(256))
        self.blocks = nn.Sequential(R.Bottleneck(64, 64, downsample=down), R.Bottleneck(256, 64))

    def forward(self, x):
        from pytorch_distributed_training_tutorials_amd.ops.norm import bn_relu_maxpool

        self.stem_out = self.conv1(x)  # kept for its gradient: the dx of the first (deepest) BN
        if self.stem_out.requires_grad:
            self.stem_out.retain_grad()
        return self.blocks(bn_relu_maxpool(self.stem_out, self.bn1, self.maxpool))


def test_forced_sync_path_in_a_bottleneck_model(monkeypatch):
    """PTDT_SYNCBN_FORCE=1 at world 1: every converted layer runs the synchronised path through real
    collectives (so neither the conv-epilogue statistics nor the fused stem may serve it) and, the
    world being this one rank, reproduces the unconverted model.

    Which statistics kernel the unconverted 1x1 conv + BN pairs run is decided by a one-off timing
    (PTDT_CONVBN=auto), so the reference would differ from run to run in the last bit of its
    statistics -- enough to flip single ReLU masks in bf16, each of which moves ~600 elements of the
    stem gradient through the 3x3 convolutions. The reference run therefore pins the composed
    path; the converted run pins the fused one ("on"), so that only the layer's own decline keeps
    the conv epilogue out. For the same reason one discarded pass warms the convolutions up, so
    that both compared passes run the same convolution kernels.

    The convolution library's default backward solvers here accumulate with atomics: repeated passes
    of one and the same model then land, pass by pass, on one of a few bf16 outcomes (stem-gradient
    sums of -4.15, -3.99, -2.05 seen within one process), which no warm-up settles and which made
    this comparison pass or fail by what else had run in the process. Both compared passes
    therefore ask for the deterministic solvers; eight repeated passes are then bit-identical."""
    from pytorch_distributed_training_tutorials_amd.ops import convbn, norm
    from pytorch_distributed_training_tutorials_amd.parallel import comm as comm_mod

    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    dev = torch.device("cuda", 0)
    calls = {"conv_epilogue": 0, "stem": 0}

    def counted(cls, key):
        orig = cls.apply

        def apply(*a, **k):
            calls[key] += 1
            return orig(*a, **k)

        monkeypatch.setattr(cls, "apply", staticmethod(apply))

    counted(convbn._Conv1x1StatsFn, "conv_epilogue")
    counted(norm._BnReluPoolFn, "stem")
    torch.manual_seed(2)
    model = _Stack().to(dev).to(memory_format=torch.channels_last)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.weight.uniform_(0.5, 1.5)
                m.bias.uniform_(-0.5, 0.5)
    state = {k: v.clone() for k, v in model.state_dict().items()}
    x0 = torch.randn(4, 3, 32, 32, device=dev).contiguous(memory_format=torch.channels_last)
    gy = torch.randn(4, 256, 8, 8, device=dev).contiguous(memory_format=torch.channels_last)

    def run():
        with torch.autocast("cuda", dtype=torch.bfloat16):
            y = model(x0)
        (y.float() * gy).sum().backward()
        grads = {n: p.grad.clone() for n, p in model.named_parameters()}
        model.zero_grad()
        return y.detach().float(), model.stem_out.grad.float(), grads

    monkeypatch.setattr(convbn, "_ENABLED", False)
    run()  # untimed first pass: the convolution library may settle on another solver after a first call
    model.load_state_dict(state)
    calls.update(conv_epilogue=0, stem=0)
    y_ref, dx_ref, g_ref = run()
    assert calls == {"conv_epilogue": 0, "stem": 1}  # the unconverted model does take the fused stem
    monkeypatch.setattr(convbn, "_ENABLED", True)
    monkeypatch.setattr(convbn, "_MODE", "on")
    stats_ref = {k: v.clone() for k, v in model.state_dict().items()}
    model.load_state_dict(state)
    calls.update(conv_epilogue=0, stem=0)
    monkeypatch.setenv("PTDT_SYNCBN_FORCE", "1")
    comm = comm_mod.new_communicator(device=dev, name="syncbn_test")
    SyncBatchNorm.convert_sync_batchnorm(model, comm=comm)
    layers = [m for m in model.modules() if isinstance(m, SyncBatchNorm)]
    assert len(layers) == 8
    y, dx, g = run()
    assert calls == {"conv_epilogue": 0, "stem": 0}
    assert [m.sync_forwards for m in layers] == [1] * 8
    print("max |y - ref|", float((y - y_ref).abs().max()), "max |dx - ref|", float((dx - dx_ref).abs().max()),
          "max |dx ref|", float(dx_ref.abs().max()))
    torch.testing.assert_close(y, y_ref, rtol=2e-2, atol=2e-2)
    torch.testing.assert_close(dx, dx_ref, rtol=5e-2, atol=5e-2)
    for n, p in model.named_parameters():
        if p.dim() == 1:  # BN weight / bias gradients: test_norm.py's wtol rule, rows = batch x spatial
            wtol = 1e-3 * 1024 ** 0.5
            torch.testing.assert_close(g[n], g_ref[n], rtol=1e-3, atol=wtol)
    for k, v in model.state_dict().items():
        if "running" in k:
            torch.testing.assert_close(v, stats_ref[k], rtol=1e-4, atol=1e-5)
        elif "num_batches" in k:
            assert int(v) == int(stats_ref[k]) == 1
    comm.destroy()


def test_convert_sync_batchnorm_keeps_tensors_keys_and_flags():
    model = W.conversion_checks("cuda:0")
    assert all(m._bn_tickets.is_cuda for m in model.modules() if isinstance(m, SyncBatchNorm))


def test_two_ranks_sharing_the_gpu_match_full_batch(tmp_path):
    """Rank 0 holds 3 images and rank 1 holds 5 of one (8, 64, 7, 7) batch; both on cuda:0, the
    exchange on host copies (HostStagedComm), the kernels native."""
    spawn(W.gpu_shared_device, args=(2, free_port(), str(tmp_path)), nprocs=2)
    res = [torch.load(os.path.join(tmp_path, f"r{r}.pt"), weights_only=True) for r in range(2)]
    W.assert_matches_full_batch(res, 0.1)
