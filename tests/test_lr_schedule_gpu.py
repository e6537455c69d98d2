"""Device learning-rate schedules on the GPU (csrc/kernels/lr_schedule.hip and the ``lr_dev`` argument
of the update kernels): kernel values against torch's schedulers, bit-for-bit twin optimizers, the
whole-step hipGraph, the Trainer, resume, and parameters on two devices.

Value bound: ``|lr_dev - float32(lr_torch)| <= 2**-23 * |lr_torch| + 1e-12 * base_lr`` -- one float32
ulp for the kernel's single rounding plus the fp64 slack of tests/test_lr_schedule.py. Parameter
tolerances as tests/test_gradclip_gpu.py."""
import copy
import gc
import warnings

import numpy as np
import pytest
import torch

from . import _lr_configs as cfg

pytestmark = pytest.mark.gpu
RTOL, ATOL = 1e-5, 1e-6
SIZES = (1, 3, 257, 4099)  # scalar tail, not a multiple of 4, and past the 4096-element chunk


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


def _assert_lr(got, want, bases, what):
    """Bound (1) of the module docstring, every group."""
    for g, (lr, ref) in enumerate(zip(got, want)):
        err, bound = abs(lr - float(np.float32(ref))), 2.0 ** -23 * abs(ref) + cfg.FP64_SLACK * bases[g]
        print(f"{what} group {g}: lr_dev={lr!r} torch={ref!r} err={err:.3e} bound={bound:.3e}")
        assert err <= bound, (what, g, lr, ref, err, bound)


# ------------------------------------------------------------------ 1. kernel values
@pytest.mark.parametrize("name", list(cfg.CONFIGS))
def test_kernel_values_match_torch(dev, name):
    from pytorch_distributed_training_tutorials_amd.ops import FusedSGD

    want = cfg.torch_lrs(name)
    opt = FusedSGD([{"params": [torch.zeros(3, device=dev, requires_grad=True)], "lr": b} for b in cfg.BASES])
    sched = cfg.ours(name, opt)
    seen = [sched.lrs[dev].tolist()]
    for _ in range(cfg.STEPS):
        sched.step()
        seen.append(sched.lrs[dev].tolist())
    worst = 0.0
    for t, (got, ref) in enumerate(zip(seen, want)):
        for g in range(len(cfg.BASES)):
            err = abs(got[g] - float(np.float32(ref[g])))
            bound = 2.0 ** -23 * abs(ref[g]) + cfg.FP64_SLACK * cfg.BASES[g]
            worst = max(worst, err / bound)
            assert err <= bound, (name, t, g, got[g], ref[g], err, bound)
    print(f"{name}: worst err/bound over {cfg.STEPS + 1} steps = {worst:.3f}")
    assert int(sched.counters[dev]) == cfg.STEPS == sched.last_epoch
    assert sched.get_last_lr() == seen[-1] == [g["lr"] for g in opt.param_groups]


def test_binding_checks_lr_dev(native, dev):
    p, g = torch.zeros(8, device=dev), torch.ones(8, device=dev)
    args = (p, g, None, None, 0.5, 0.0, 0.0, 0.0, False, 1.0, None)
    for bad in (torch.ones(2, device=dev), torch.ones(1, device=dev, dtype=torch.float64), torch.ones(1),
                torch.ones(4, device=dev)[::2]):
        with pytest.raises(RuntimeError, match="lr_dev"):
            native.sgd_flat_(*args, bad)
    assert torch.equal(p, torch.zeros(8, device=dev))
    native.sgd_flat_(*args, torch.full((1,), 0.25, device=dev))
    assert torch.equal(p, torch.full((8,), -0.25, device=dev))  # the device value, not the float 0.5
    with pytest.raises(RuntimeError, match="segments"):
        native.lr_schedule_step_(torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(1, device=dev), [0.1],
                                 [1, 2, 3, 4], [0] * 5, [1] * 5, [0.5] * 5, [0.0] * 5, [[]] * 5, True)


# ------------------------------------------------------------------ 2. update kernels honour lr_dev
def _flat(ps):
    from pytorch_distributed_training_tutorials_amd.ops.flat import FlatParameters

    FlatParameters(ps, with_grads=True)  # p.data and p.grad become back-to-back views of one buffer each
    return ps


TWINS = {
    # name: (optimizer, kwargs, parameter dtype, flat layout, the native launch that must carry the update)
    "sgd_flat": ("sgd", dict(weight_decay=1e-2), torch.float32, True, "sgd_flat_"),
    "sgd_flat_momentum": ("sgd", dict(momentum=0.9, weight_decay=1e-2), torch.float32, True, "sgd_flat_"),
    "sgd_multi_f32_shadow": ("sgd", dict(momentum=0.9, weight_decay=1e-2, bf16_shadow=True), torch.float32, False,
                             "sgd_multi_"),
    "sgd_multi_bf16": ("sgd", dict(momentum=0.9, nesterov=True), torch.bfloat16, False, "sgd_multi_"),
    "adam_flat": ("adam", dict(), torch.float32, True, "adam_flat_"),
    "adam_multi_bf16": ("adam", dict(weight_decay=1e-2), torch.bfloat16, False, "adam_multi_"),
    "adamw_flat": ("adam", dict(weight_decay=0.1, decoupled_weight_decay=True), torch.float32, True, "adam_flat_"),
    "adamw_multi_bf16": ("adam", dict(weight_decay=0.1, decoupled_weight_decay=True), torch.bfloat16, False,
                         "adam_multi_"),
}
# two groups with different base rates; every group holds a chunk-crossing tensor and a tiny one. Flat layout:
# group 0 spans 4102 elements from an aligned start (vector body + tail of 2), group 1 starts unaligned
GROUPS = ((3, 4099), (1, 257))


def _twin(dev, kind, kw, dtype, flat):
    from pytorch_distributed_training_tutorials_amd.ops import FusedAdam, FusedSGD

    gen = torch.Generator().manual_seed(11)
    ps = [[torch.randn(n, generator=gen).to(dtype).to(dev).requires_grad_(True) for n in sizes] for sizes in GROUPS]
    if flat:
        _flat([p for group in ps for p in group])
    else:
        for group in ps:
            for p in group:
                p.grad = torch.zeros_like(p)
    cls = FusedSGD if kind == "sgd" else FusedAdam
    return cls([{"params": group, "lr": b} for group, b in zip(ps, cfg.BASES)], **kw), ps


def _spy(monkeypatch, native):
    """{binding name: [lr_dev argument of each launch]} for the four update bindings."""
    calls = {}
    for name, at in (("sgd_flat_", 11), ("sgd_multi_", 12), ("adam_flat_", 13), ("adam_multi_", 13)):
        def counted(*a, _real=getattr(native, name), _name=name, _at=at):
            calls.setdefault(_name, []).append(a[_at] if len(a) > _at else None)
            return _real(*a)
        monkeypatch.setattr(native, name, counted)
    return calls


def _state_tensors(opt, ps):
    out = []
    for group in ps:
        for p in group:
            out.append(p.detach())
            out += [v for k, v in sorted(opt.state[p].items()) if torch.is_tensor(v) and k != "step"]
            if getattr(p, "_ptdt_bf16", None) is not None:
                out.append(p._ptdt_bf16)
    return out


@pytest.mark.parametrize("case", list(TWINS))
def test_update_kernels_use_the_device_learning_rate_bit_for_bit(native, dev, monkeypatch, case):
    """Twin A has the scheduler bound; twin B gets group["lr"] set, before each step, to the float32 value
    read back from A's buffer (exact in fp64, so the binding's cast is exact). 6 steps of a 0.1 -> 1 linear
    warm-up: parameters, momentum buffers / moments and bf16 shadows must be equal bit for bit."""
    kind, kw, dtype, flat, launch = TWINS[case]
    (oa, pa), (ob, pb) = _twin(dev, kind, kw, dtype, flat), _twin(dev, kind, kw, dtype, flat)
    sched = cfg.ours("warmup6", oa)
    calls = _spy(monkeypatch, native)
    gen = torch.Generator().manual_seed(12)
    seen = []
    for _ in range(6):
        lrs = sched.lrs[dev].tolist()
        seen.append(lrs)
        for ga, gb in zip(pa, pb):
            for p, q in zip(ga, gb):
                g = torch.randn(p.shape, generator=gen).to(dtype).to(dev)
                p.grad.copy_(g)
                q.grad.copy_(g)
        n = len(calls.get(launch, []))
        oa.step()
        sched.step()
        assert set(calls) == {launch} and len(calls[launch]) == n + len(GROUPS), (case, {k: len(v) for k, v in calls.items()})
        assert all(v is not None for v in calls[launch][n:])
        for group, lr in zip(ob.param_groups, lrs):
            group["lr"] = lr
        ob.step()
        assert all(v is None for v in calls[launch][n + len(GROUPS):])
    want = cfg.torch_lrs("warmup6", 6)
    for t, lrs in enumerate(seen):
        _assert_lr(lrs, want[t], cfg.BASES, f"{case} t={t}")
    assert seen[0][0] != seen[5][0] and seen[0][0] != seen[0][1]  # the rate moved, and differs between the groups
    ta, tb = _state_tensors(oa, pa), _state_tensors(ob, pb)
    expect = {"sgd": 1 + ("momentum" in kw) + bool(kw.get("bf16_shadow")), "adam": 3}[kind]
    assert len(ta) == len(tb) == expect * sum(len(g) for g in GROUPS)
    for x, y in zip(ta, tb):
        assert torch.equal(x, y), (case, x.shape, (x.float() - y.float()).abs().max())
    assert [g["lr"] for g in oa.param_groups] == list(cfg.BASES)  # the host float is untouched until a host read
    assert sched.get_last_lr() == sched.lrs[dev].tolist()


# ------------------------------------------------------------------ 3. the captured step
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
    """zero_grad, forward (bf16 autocast), backward, [clip,] FusedSGD.step, [scheduler.step] on the small
    DDP model of tests/test_gradclip_gpu.py."""

    def __init__(self, dev, init, scheduled=True, clip=False):
        from pytorch_distributed_training_tutorials_amd.ops import GradClipper
        from pytorch_distributed_training_tutorials_amd.ops.optim import FusedSGD
        from pytorch_distributed_training_tutorials_amd.parallel import comm as comm_mod
        from pytorch_distributed_training_tutorials_amd.parallel.ddp import DistributedDataParallel

        self.comm = comm_mod.get_default(dev)
        self.model = _Net().to(dev).to(memory_format=torch.channels_last)
        self.model.load_state_dict(init)
        self.ddp = DistributedDataParallel(self.model, device_ids=[dev.index], comm=self.comm)
        self.opt = FusedSGD(self.model.parameters(), lr=0.05, momentum=0.9, weight_decay=1e-2)
        self.sched = cfg.ours("loop_warmup_cosine", self.opt) if scheduled else None
        self.clipper = GradClipper(list(self.model.parameters()), 0.05, optimizer=self.opt) if clip else None
        g = torch.Generator().manual_seed(7)
        self.x = torch.randn(16, 8, 8, 8, generator=g).to(dev).contiguous(memory_format=torch.channels_last)
        self.y = torch.randint(0, 10, (16,), generator=g).to(dev)

    def step(self):
        from pytorch_distributed_training_tutorials_amd.ops.loss import cross_entropy

        self.ddp.zero_grad()
        with torch.autocast("cuda", dtype=torch.bfloat16, cache_enabled=False):
            out = self.ddp(self.x)
        loss = cross_entropy(out.float(), self.y)
        loss.backward()
        if self.clipper is not None:
            self.clipper()
        self.opt.step()
        if self.sched is not None:
            self.sched.step()
        return loss

    def params(self):
        return [p.detach().clone() for p in self.model.parameters()]


@pytest.mark.parametrize("clip", [False, True], ids=["plain", "fused_clip"])
def test_graph_replays_follow_the_schedule(pg, dev, deterministic, clip):
    """GraphedStep(warmup=1) + 8 replays against 9 eager steps of the same scheduled loop; and, against
    a vacuous pass, the same 9 steps at the constant base rate must NOT match."""
    from pytorch_distributed_training_tutorials_amd.utils.graphs import GraphedStep

    init = _init_state()
    eager = _Loop(dev, init, clip=clip)
    for _ in range(9):
        eager.step()
    graphed = _Loop(dev, init, clip=clip)
    gc.collect()  # as tests/test_gradclip_gpu.py: no destructor of an earlier test's wrapper inside the capture
    gs = GraphedStep(graphed.step, dev, comm=graphed.comm, warmup=1)
    for _ in range(8):
        gs()
    torch.cuda.synchronize(dev)
    for p, q in zip(graphed.params(), eager.params()):
        torch.testing.assert_close(p, q, rtol=RTOL, atol=ATOL)
    want = cfg.torch_lrs("loop_warmup_cosine", 9, (0.05,))
    for loop, what in ((graphed, "graphed"), (eager, "eager")):
        assert int(loop.sched.counters[dev]) == 9, what
        _assert_lr(loop.sched.lrs[dev].tolist(), want[9], (0.05,), what)
    assert graphed.opt.param_groups[0]["lr"] == 0.05  # no host read so far ...
    assert graphed.sched.get_last_lr() == [graphed.opt.param_groups[0]["lr"]] == graphed.sched.lrs[dev].tolist()
    const = _Loop(dev, init, scheduled=False, clip=clip)
    for _ in range(9):
        const.step()
    diff = float((const.model.fc.weight.detach() - graphed.model.fc.weight.detach()).abs().max())
    print(f"clip={clip}: max |fc.weight(constant lr) - fc.weight(scheduled)| = {diff:.3e} (needs >= {100 * ATOL:.0e})")
    assert diff >= 100 * ATOL
    with pytest.raises(AssertionError):
        for p, q in zip(const.params(), eager.params()):
            torch.testing.assert_close(p, q, rtol=RTOL, atol=ATOL)


# ------------------------------------------------------------------ 4. Trainer
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
    opt = FusedSGD(model.parameters(), lr=0.1, momentum=0.9)
    if kw.get("lr_scheduler") == "instance":  # bound while the parameters are still on the CPU: the Trainer re-places it
        kw["lr_scheduler"] = cfg.ours("trainer_warmup_step", opt)
    t = Trainer(model, loader, opt, 0, loss_fn=mse_loss, verbose=False, **kw)
    return t, model, ref, X, Y


@pytest.mark.parametrize("how", ["callable", "instance"])
def test_trainer_lr_scheduler(pg, dev, how):
    make = (lambda o: cfg.ours("trainer_warmup_step", o)) if how == "callable" else "instance"
    t, model, ref, X, Y = _toy(dev, lr_scheduler=make)
    assert t.engine_name == "autograd"
    t.train(2)
    ropt = torch.optim.SGD(ref.parameters(), lr=0.1, momentum=0.9)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        rsched = cfg.torch_sched("trainer_warmup_step", ropt)
        for i in list(range(4)) * 2:
            ropt.zero_grad()
            torch.nn.functional.mse_loss(ref(X[16 * i:16 * i + 16]), Y[16 * i:16 * i + 16]).backward()
            ropt.step()
            rsched.step()
    for p, r in zip(model.parameters(), ref.parameters()):
        torch.testing.assert_close(p.detach(), r.detach(), rtol=RTOL, atol=ATOL)
    assert t.lr_scheduler.last_epoch == 8
    _assert_lr(t.lr_scheduler.get_last_lr(), [ropt.param_groups[0]["lr"]], (0.1,), "trainer")
    with pytest.raises(ValueError, match="lr_scheduler"):
        _toy(dev, lr_scheduler=make, engine="persistent")
    assert _toy(dev)[0].engine_name == "persistent"


# ------------------------------------------------------------------ 5. resume
@pytest.mark.parametrize("kind", ["sgd", "adamw"])
def test_resume_continues_the_trajectory(dev, tmp_path, kind):
    from pytorch_distributed_training_tutorials_amd.ops import FusedAdam, FusedSGD
    from pytorch_distributed_training_tutorials_amd.utils.checkpoint import load_checkpoint, save_checkpoint

    g = torch.Generator().manual_seed(5)
    x, y = torch.randn(32, 20, generator=g).to(dev), torch.randn(32, 1, generator=g).to(dev)

    def fresh():
        torch.manual_seed(6)
        m = torch.nn.Linear(20, 1).to(dev)
        o = (FusedSGD(m.parameters(), lr=0.1, momentum=0.9) if kind == "sgd" else
             FusedAdam(m.parameters(), lr=0.05, weight_decay=0.1, decoupled_weight_decay=True))
        return m, o, cfg.ours("loop_warmup_cosine", o)

    def run(m, o, s, n):
        for _ in range(n):
            o.zero_grad()
            torch.nn.functional.mse_loss(m(x), y).backward()
            o.step()
            s.step()

    whole = fresh()
    run(*whole, 10)
    first = fresh()
    run(*first, 5)
    path = str(tmp_path / "ck.pt")
    save_checkpoint(path, first[0], first[1], epoch=0, lr_scheduler=first[2])
    m, o, s = fresh()
    state = load_checkpoint(path, m, o, map_location=dev, lr_scheduler=s)
    assert state["lr_scheduler"]["t"] == 5 and int(s.counters[dev]) == 5
    assert s.lrs[dev].tolist() == first[2].lrs[dev].tolist() == s.get_last_lr()
    run(m, o, s, 5)
    for p, q in zip(m.parameters(), whole[0].parameters()):
        assert torch.equal(p, q)
    assert s.state_dict() == whole[2].state_dict()


# ------------------------------------------------------------------ 6. two devices
@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs 2 GPUs")
def test_one_group_on_two_devices(native):
    from pytorch_distributed_training_tutorials_amd.ops import FusedSGD

    devs = [torch.device("cuda", 0), torch.device("cuda", 1)]
    gen = torch.Generator().manual_seed(21)
    init = [torch.randn(n, generator=gen) for n in (4099, 257)]

    def make():
        ps = [v.clone().to(d).requires_grad_(True) for v, d in zip(init, devs)]
        return FusedSGD(ps, lr=0.1, momentum=0.9, weight_decay=1e-2), ps

    (oa, pa), (ob, pb) = make(), make()
    sched = cfg.ours("warmup6", oa)
    assert set(sched.lrs) == set(devs)
    for _ in range(7):
        lr = sched.lrs[devs[0]].tolist()
        for p, q in zip(pa, pb):
            g = torch.randn(p.shape, generator=gen)
            p.grad, q.grad = g.to(p.device), g.to(q.device)
        oa.step()
        sched.step()
        ob.param_groups[0]["lr"] = lr[0]
        ob.step()
    assert sched.lrs[devs[0]].tolist() == sched.lrs[devs[1]].tolist()
    assert [int(sched.counters[d]) for d in devs] == [7, 7]
    _assert_lr(sched.lrs[devs[1]].tolist(), cfg.torch_lrs("warmup6", 7, (0.1,))[7], (0.1,), "cuda:1")
    for p, q in zip(pa, pb):
        assert torch.equal(p.detach(), q.detach())
        assert torch.equal(oa.state[p]["momentum_buffer"], ob.state[q]["momentum_buffer"])
