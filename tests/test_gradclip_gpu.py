"""Gradient clipping inside the training loops (GPU): DDP bucket views with grad sinks, whole-step
hipGraph capture, the Trainer, and gradients on two devices. Tolerances as tests/test_gradclip.py."""
import copy
import gc
import math

import pytest
import torch

from ._edge_ref import f64

pytestmark = pytest.mark.gpu
RTOL, ATOL = 1e-5, 1e-6


@pytest.fixture(scope="module")
def pg():
    from pytorch_distributed_training_tutorials_amd.parallel import env

    env.init_process_group("nccl")
    yield
    env.destroy_process_group()


@pytest.fixture
def deterministic():
    old = torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
    yield
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = old


class _Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        from pytorch_distributed_training_tutorials_amd.ops.conv import Conv2d
        from pytorch_distributed_training_tutorials_amd.ops.linear import Linear
        from pytorch_distributed_training_tutorials_amd.ops.norm import BatchNorm2d

        self.conv = Conv2d(8, 32, 3, padding=1, bias=False)
        self.bn = BatchNorm2d(32)
        self.fc = Linear(32, 10)

    def forward(self, x):
        x = self.bn(self.conv(x), relu=True)
        return self.fc(x.mean((2, 3)))


def _init_state():
    torch.manual_seed(0)
    return copy.deepcopy(_Net().state_dict())


class _Loop:
    """zero_grad, forward (bf16 autocast), backward, clip, FusedSGD.step on the small DDP model."""

    def __init__(self, dev, init, mode, max_norm=0.05):
        from pytorch_distributed_training_tutorials_amd.ops import GradClipper
        from pytorch_distributed_training_tutorials_amd.ops.optim import FusedSGD
        from pytorch_distributed_training_tutorials_amd.parallel import comm as comm_mod
        from pytorch_distributed_training_tutorials_amd.parallel.ddp import DistributedDataParallel

        self.comm = comm_mod.get_default(dev)
        self.model = _Net().to(dev).to(memory_format=torch.channels_last)
        self.model.load_state_dict(init)
        self.ddp = DistributedDataParallel(self.model, device_ids=[dev.index], comm=self.comm)
        self.opt = FusedSGD(self.model.parameters(), lr=0.05, momentum=0.9, weight_decay=1e-2)
        self.clipper = GradClipper(list(self.model.parameters()), max_norm,
                                   optimizer=self.opt if mode == "fused" else None)
        g = torch.Generator().manual_seed(7)
        self.x = torch.randn(16, 8, 8, 8, generator=g).to(dev).contiguous(memory_format=torch.channels_last)
        self.y = torch.randint(0, 10, (16,), generator=g).to(dev)
        self.after_backward = None  # test hook, eager steps only

    def step(self):
        from pytorch_distributed_training_tutorials_amd.ops.loss import cross_entropy

        self.ddp.zero_grad()
        with torch.autocast("cuda", dtype=torch.bfloat16, cache_enabled=False):
            out = self.ddp(self.x)
        loss = cross_entropy(out.float(), self.y)
        loss.backward()
        if self.after_backward is not None:
            self.after_backward(self)  # the loop is passed in: a closure over it would be a reference cycle
        norm = self.clipper()
        self.opt.step()
        return loss, norm

    def params(self):
        return [p.detach().clone() for p in self.model.parameters()]


def _assert_same(a, b):
    for p, q in zip(a, b):
        torch.testing.assert_close(p, q, rtol=RTOL, atol=ATOL)


def test_ddp_bucket_views_collapse_to_spans_and_fused_equals_inplace(pg, dev, deterministic):
    init = _init_state()
    loops = {mode: _Loop(dev, init, mode) for mode in ("fused", "inplace")}
    seen = {}

    def check(loop):
        grads = [p.grad for p in loop.model.parameters()]
        assert all(g is not None for g in grads)
        seen["ref"] = math.sqrt(sum(float(f64(g).pow(2).sum()) for g in grads))
        seen["n"] = len(grads)

    norms = {}
    for mode, loop in loops.items():
        loop.after_backward = check
        out = []
        for _ in range(3):
            _, norm = loop.step()
            torch.testing.assert_close(float(norm), seen["ref"], rtol=RTOL, atol=0.0)
            assert float(loop.clipper.coef) < 1.0
            out.append(float(norm))
        assert 0 < loop.clipper.num_spans < seen["n"], (loop.clipper.num_spans, seen["n"])
        norms[mode] = out
    torch.testing.assert_close(torch.tensor(norms["fused"]), torch.tensor(norms["inplace"]), rtol=RTOL, atol=ATOL)
    _assert_same(loops["fused"].params(), loops["inplace"].params())


@pytest.mark.parametrize("mode", ["fused", "inplace"])
def test_graph_replays_match_eager_steps(pg, dev, deterministic, mode):
    """One warm-up step and 4 replays of the captured step (clipper included) against the same 5
    steps launched eagerly: parameters and the recorded norms."""
    from pytorch_distributed_training_tutorials_amd.utils.graphs import GraphedStep

    init = _init_state()
    eager = _Loop(dev, init, mode)
    want = [float(eager.step()[1]) for _ in range(5)]
    graphed = _Loop(dev, init, mode)
    # torch.cuda.graph no longer collects garbage before a capture: a dead cycle holding an earlier
    # test's DDP wrapper could otherwise be collected, and its destructors run, inside the capture
    gc.collect()
    gs = GraphedStep(graphed.step, dev, comm=graphed.comm, warmup=1)
    got = []
    for _ in range(4):
        _, norm = gs()
        got.append(float(norm))
    torch.cuda.synchronize(dev)
    assert all(n > 0.05 for n in got)  # every replayed step clipped
    torch.testing.assert_close(torch.tensor(got), torch.tensor(want[1:]), rtol=RTOL, atol=ATOL)
    _assert_same(graphed.params(), eager.params())


def _toy(dev, **kw):
    from pytorch_distributed_training_tutorials_amd.data import DeviceDataLoader, DeviceTensorDataset, DistributedSampler
    from pytorch_distributed_training_tutorials_amd.ops.loss import mse_loss
    from pytorch_distributed_training_tutorials_amd.ops.optim import FusedSGD
    from pytorch_distributed_training_tutorials_amd.utils.trainer import Trainer

    g = torch.Generator().manual_seed(40)
    X, Y = torch.randn(64, 20, generator=g).to(dev), (3.0 * torch.randn(64, 1, generator=g)).to(dev)
    ds = DeviceTensorDataset(X, Y)
    loader = DeviceDataLoader(ds, batch_size=16, sampler=DistributedSampler(ds, 1, 0, shuffle=False))
    torch.manual_seed(3)
    model = torch.nn.Linear(20, 1)
    ref = copy.deepcopy(model).to(dev)
    t = Trainer(model, loader, FusedSGD(model.parameters(), lr=0.1, momentum=0.9), 0, loss_fn=mse_loss, verbose=False,
                **kw)
    return t, model, ref, X, Y


def test_trainer_max_grad_norm(pg, dev):
    t, model, ref, X, Y = _toy(dev, max_grad_norm=0.5)
    assert t.engine_name == "autograd"
    t.train(1)
    ropt = torch.optim.SGD(ref.parameters(), lr=0.1, momentum=0.9)
    for i in range(4):
        ropt.zero_grad()
        torch.nn.functional.mse_loss(ref(X[16 * i:16 * i + 16]), Y[16 * i:16 * i + 16]).backward()
        assert float(torch.nn.utils.clip_grad_norm_(ref.parameters(), 0.5)) > 0.5
        ropt.step()
    for p, r in zip(model.parameters(), ref.parameters()):
        torch.testing.assert_close(p.detach(), r.detach(), rtol=RTOL, atol=ATOL)
    with pytest.raises(ValueError):
        _toy(dev, max_grad_norm=0.5, engine="persistent")
    assert _toy(dev)[0].engine_name == "persistent"


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs 2 GPUs")
@pytest.mark.parametrize("norm_type", [2.0, math.inf])
def test_gradients_on_two_devices(norm_type):
    from pytorch_distributed_training_tutorials_amd.ops import GradClipper

    g = torch.Generator().manual_seed(50)
    shapes = [("cuda:0", (4097,), torch.float32), ("cuda:1", (33, 7), torch.float32),
              ("cuda:1", (5000,), torch.bfloat16), ("cuda:0", (9,), torch.bfloat16)]
    ps = []
    for device, shape, dtype in shapes:
        p = torch.zeros(shape, dtype=dtype, device=device, requires_grad=True)
        p.grad = torch.randn(shape, generator=g).to(dtype).to(device)
        ps.append(p)
    g64 = [f64(p.grad) for p in ps]
    total = (max(float(x.abs().max()) for x in g64) if norm_type == math.inf
             else math.sqrt(sum(float(x.pow(2).sum()) for x in g64)))
    coef = min(1.0, 1.0 / (total + 1e-6))
    clipper = GradClipper(ps, 1.0, norm_type)
    norm = clipper()
    assert norm.device == ps[0].grad.device and norm.dim() == 0
    torch.testing.assert_close(float(norm), total, rtol=RTOL, atol=0.0)
    from ._edge_ref import assert_within_bf16_ulp

    for p, x in zip(ps, g64):
        if p.dtype == torch.bfloat16:
            assert_within_bf16_ulp(p.grad, x * coef, "two devices")
        else:
            torch.testing.assert_close(f64(p.grad), x * coef, rtol=RTOL, atol=ATOL)
