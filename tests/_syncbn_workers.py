"""Spawned ranks of the SyncBatchNorm tests (tests/test_syncbn_cpu.py, tests/test_syncbn_gpu.py).

Each rank takes its slice of one deterministic batch, runs one forward and one backward through
``ops.norm.SyncBatchNorm`` and saves what the parent test compares with the full-batch reference.
Straight-line code: the first error ends the rank (and, through the launcher, the test)."""
import os

import torch

SHAPE = (8, 64, 7, 7)
SPLIT = (3, 5)  # images of rank 0, rank 1


def make_case(seed=5):
    """(x, grad of y, weight, bias, initial running_mean) of the whole batch, fp32 NCHW on the CPU."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(SHAPE, generator=g) * 2 + 3
    gy = torch.randn(SHAPE, generator=g)
    w = torch.rand(SHAPE[1], generator=g) + 0.5
    b = torch.rand(SHAPE[1], generator=g) - 0.5
    rm = torch.rand(SHAPE[1], generator=g) * 2 - 1
    return x, gy, w, b, rm


def _init(rank, world, port):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch.distributed as dist

    dist.init_process_group("gloo", rank=rank, world_size=world)
    return dist


def _run(bn, x, gy, out):
    x = x.clone().requires_grad_()
    y = bn(x)
    y.backward(gy)
    out.update(y=y.detach().float().cpu(), dx=x.grad.float().cpu(), dw=bn.weight.grad.cpu(), db=bn.bias.grad.cpu(),
               running_mean=bn.running_mean.cpu(), running_var=bn.running_var.cpu(),
               nbt=int(bn.num_batches_tracked), sync_forwards=bn.sync_forwards)


def _layer(momentum, comm, dev):
    from pytorch_distributed_training_tutorials_amd.ops.norm import SyncBatchNorm

    _, _, w, b, rm = make_case()
    bn = SyncBatchNorm(SHAPE[1], momentum=momentum, comm=comm).to(dev)
    with torch.no_grad():
        bn.weight.copy_(w)
        bn.bias.copy_(b)
        bn.running_mean.copy_(rm)
    return bn


def _slice(rank, split):
    lo = sum(split[:rank])
    return slice(lo, lo + split[rank])


def cpu_reference_path(rank, world, port, out_dir, momentum, split):
    """gloo ranks, CPU tensors, NCHW: the plain-torch protocol. ``split`` with a 0 is the empty-rank case."""
    dist = _init(rank, world, port)
    from pytorch_distributed_training_tutorials_amd.parallel.comm import Communicator

    comm = Communicator(device=torch.device("cpu"))
    assert comm.world == world
    x, gy, *_ = make_case()
    sl = _slice(rank, split)
    bn = _layer(momentum, comm, torch.device("cpu"))
    out = {}
    if 0 in split:
        try:
            bn(x[sl])
        except ValueError as e:
            out["error"] = str(e)
    else:
        _run(bn, x[sl], gy[sl], out)
    torch.save(out, os.path.join(out_dir, f"r{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def gpu_shared_device(rank, world, port, out_dir):
    """Two ranks sharing cuda:0 (gloo control plane, HostStagedComm): the native kernels with the
    exchange carried on host copies; channels_last fp32."""
    dist = _init(rank, world, port)
    torch.cuda.set_device(0)
    from pytorch_distributed_training_tutorials_amd.parallel.comm import HostStagedComm

    dev = torch.device("cuda", 0)
    comm = HostStagedComm(dev)
    x, gy, *_ = make_case()
    sl = _slice(rank, SPLIT)
    bn = _layer(0.1, comm, dev)
    out = {}
    _run(bn, x[sl].to(dev).contiguous(memory_format=torch.channels_last),
         gy[sl].to(dev).contiguous(memory_format=torch.channels_last), out)
    torch.cuda.synchronize()
    torch.save(out, os.path.join(out_dir, f"r{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def assert_matches_full_batch(res, momentum, split=SPLIT):
    """The parent test's assertions on the two saved ranks: y and dx slices against an fp32
    ``nn.BatchNorm2d`` over the whole batch (the tolerances of test_norm.py's fp32 cases), running
    buffers bitwise equal across ranks, parameter gradients summing to the full-batch ones."""
    x, gy, w, b, rm = make_case()
    ref = torch.nn.BatchNorm2d(SHAPE[1], momentum=momentum)
    with torch.no_grad():
        ref.weight.copy_(w)
        ref.bias.copy_(b)
        ref.running_mean.copy_(rm)
    xr = x.clone().requires_grad_()
    yr = ref(xr)
    yr.backward(gy)
    for rank, r in enumerate(res):
        sl = _slice(rank, split)
        assert r["sync_forwards"] == 1
        torch.testing.assert_close(r["y"], yr.detach()[sl], rtol=2e-5, atol=2e-5)
        torch.testing.assert_close(r["dx"], xr.grad[sl], rtol=1e-4, atol=1e-4)
        torch.testing.assert_close(r["running_mean"], ref.running_mean, rtol=1e-5, atol=1e-5)
        torch.testing.assert_close(r["running_var"], ref.running_var, rtol=1e-4, atol=1e-5)
        assert r["nbt"] == int(ref.num_batches_tracked) == 1
    assert torch.equal(res[0]["running_mean"], res[1]["running_mean"])
    assert torch.equal(res[0]["running_var"], res[1]["running_var"])
    torch.testing.assert_close(res[0]["dw"] + res[1]["dw"], ref.weight.grad, rtol=1e-3, atol=1e-3)
    torch.testing.assert_close(res[0]["db"] + res[1]["db"], ref.bias.grad, rtol=1e-3, atol=1e-3)


def conversion_checks(dev):
    """``SyncBatchNorm.convert_sync_batchnorm`` on ``dev``: same parameter / buffer tensor objects, same
    state_dict keys, ``training`` flags kept, idempotent. Shared by the CPU and GPU test files."""
    import torch.nn as nn

    from pytorch_distributed_training_tutorials_amd.ops.norm import BatchNorm2d, SyncBatchNorm

    inner = nn.Sequential(nn.Conv2d(8, 8, 1), BatchNorm2d(8))
    inner[1].eval()  # a frozen layer inside a training model
    model = nn.Sequential(nn.Conv2d(3, 8, 3), nn.BatchNorm2d(8), nn.ReLU(), inner, BatchNorm2d(8, affine=False),
                          nn.BatchNorm1d(8)).to(dev)
    before = {k: v for k, v in model.state_dict(keep_vars=True).items()}
    tensors = {n: t for n, t in list(model.named_parameters()) + list(model.named_buffers())}
    flags = {n: m.training for n, m in model.named_modules()}
    out = SyncBatchNorm.convert_sync_batchnorm(model)
    assert out is model
    bns = [m for m in model.modules() if isinstance(m, nn.BatchNorm2d)]
    assert len(bns) == 3 and all(type(m) is SyncBatchNorm for m in bns)
    assert type(model[5]) is nn.BatchNorm1d  # 1-D layers are out of scope: untouched
    after = model.state_dict(keep_vars=True)
    assert list(after) == list(before)
    assert all(after[k] is before[k] for k in before)
    now = {n: t for n, t in list(model.named_parameters()) + list(model.named_buffers())}
    assert all(now[n] is t for n, t in tensors.items())  # the non-persistent ticket buffers included
    assert all(t.device.type == torch.device(dev).type for t in now.values())
    assert {n: m.training for n, m in model.named_modules()} == flags
    assert model[4].weight is None and not model[4].affine
    mods = list(model.modules())
    again = SyncBatchNorm.convert_sync_batchnorm(model)
    assert again is model and all(a is b for a, b in zip(mods, model.modules()))
    root = nn.BatchNorm2d(4).to(dev)  # a bare layer: the converted layer is returned
    conv = SyncBatchNorm.convert_sync_batchnorm(root)
    assert type(conv) is SyncBatchNorm and conv.weight is root.weight and conv.running_var is root.running_var
    assert SyncBatchNorm.convert_sync_batchnorm(conv) is conv
    return model
