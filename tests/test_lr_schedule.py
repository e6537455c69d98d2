"""Learning-rate schedules (ops/lr_scheduler.py) without a GPU: the host evaluator and the
CPU-parameter path against torch's own schedulers, state round trips, and the error paths."""
import copy
import warnings

import numpy as np
import pytest
import torch

from pytorch_distributed_training_tutorials_amd.ops import FusedAdam, FusedSGD
from pytorch_distributed_training_tutorials_amd.ops import lr_scheduler as L

from . import _lr_configs as cfg


def _two_groups(cls=FusedSGD, **kw):
    ps = [torch.zeros(3, requires_grad=True) for _ in cfg.BASES]
    return cls([{"params": [p], "lr": b} for p, b in zip(ps, cfg.BASES)], **kw), ps


def test_exported_from_ops():
    from pytorch_distributed_training_tutorials_amd import ops

    for name in ("ConstantLR", "LinearLR", "CosineAnnealingLR", "StepLR", "MultiStepLR", "ExponentialLR",
                 "PolynomialLR", "SequentialLR"):
        assert getattr(ops, name) is getattr(L, name)


@pytest.mark.parametrize("name", list(cfg.CONFIGS))
def test_host_evaluator_and_cpu_path_match_torch(name):
    """value_at(t) and the group["lr"] the CPU path writes: |lr - lr_torch| <= 1e-12 * base_lr over 40
    steps, and equal to torch after rounding to float32."""
    want = cfg.torch_lrs(name)
    opt, ps = _two_groups()
    sched = cfg.ours(name, opt)
    for t in range(cfg.STEPS + 1):
        stepped = [g["lr"] for g in opt.param_groups]
        for got in (sched.value_at(t), stepped):
            for g, (lr, ref) in enumerate(zip(got, want[t])):
                assert abs(lr - ref) <= cfg.FP64_SLACK * cfg.BASES[g], (name, t, g, lr, ref)
                assert np.float32(lr) == np.float32(ref), (name, t, g, lr, ref)
        assert sched.get_last_lr() == stepped and sched.last_epoch == t
        for p in ps:
            p.grad = torch.ones_like(p)
        opt.step()
        sched.step()


@pytest.mark.parametrize("name", ["warmup_cosine", "step"])
@pytest.mark.parametrize("kind", ["sgd", "adamw"])
def test_cpu_trajectory_matches_torch(name, kind):
    torch.manual_seed(0)
    a = torch.nn.Linear(20, 1)
    b = copy.deepcopy(a)
    x, y = torch.randn(32, 20), torch.randn(32, 1)
    if kind == "sgd":
        oa = FusedSGD(a.parameters(), lr=0.1, momentum=0.9)
        ob = torch.optim.SGD(b.parameters(), lr=0.1, momentum=0.9)
    else:
        oa = FusedAdam(a.parameters(), lr=0.1, weight_decay=0.1, decoupled_weight_decay=True)
        ob = torch.optim.AdamW(b.parameters(), lr=0.1, weight_decay=0.1)
    sa = cfg.ours(name, oa)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        sb = cfg.torch_sched(name, ob)
        for _ in range(12):
            for m, o, s in ((a, oa, sa), (b, ob, sb)):
                o.zero_grad()
                torch.nn.functional.mse_loss(m(x), y).backward()
                o.step()
                s.step()
    for p, q in zip(a.parameters(), b.parameters()):
        torch.testing.assert_close(p, q)
    assert not torch.equal(a.weight, torch.nn.Linear(20, 1).weight)


def _run(model, opt, sched, x, y, n):
    for _ in range(n):
        opt.zero_grad()
        torch.nn.functional.mse_loss(model(x), y).backward()
        opt.step()
        sched.step()


@pytest.mark.parametrize("through_file", [False, True])
def test_state_round_trip_continues_identically(tmp_path, through_file):
    from pytorch_distributed_training_tutorials_amd.utils.checkpoint import load_checkpoint, save_checkpoint

    def fresh():
        torch.manual_seed(1)
        m = torch.nn.Linear(20, 1)
        o = FusedSGD(m.parameters(), lr=0.1, momentum=0.9)
        return m, o, cfg.ours("warmup_cosine", o)

    g = torch.Generator().manual_seed(2)
    x, y = torch.randn(32, 20, generator=g), torch.randn(32, 1, generator=g)
    m0, o0, s0 = fresh()
    _run(m0, o0, s0, x, y, 14)
    m1, o1, s1 = fresh()
    _run(m1, o1, s1, x, y, 7)
    state = s1.state_dict()
    assert state["t"] == 7 and state["base_lrs"] == [0.1] and set(state) == {"t", "base_lrs", "program"}
    m2, o2, s2 = fresh()
    if through_file:
        path = str(tmp_path / "ck.pt")
        save_checkpoint(path, m1, o1, epoch=0, lr_scheduler=s1)
        saved = load_checkpoint(path, m2, o2, lr_scheduler=s2)
        assert saved["lr_scheduler"] == state
        save_checkpoint(path, m1, o1)  # a checkpoint without the key loads as before
        assert "lr_scheduler" not in load_checkpoint(path, m2, o2, lr_scheduler=s2)
    else:
        m2.load_state_dict(m1.state_dict())
        o2.load_state_dict(o1.state_dict())
        s2.load_state_dict(copy.deepcopy(state))
    assert s2.last_epoch == 7 and s2.get_last_lr() == s1.get_last_lr() == s0.value_at(7)
    _run(m2, o2, s2, x, y, 7)
    for p, q in zip(m2.parameters(), m0.parameters()):
        assert torch.equal(p, q)
    assert s2.state_dict() == s0.state_dict()


def test_optimizer_state_dict_keeps_torch_layout():
    opt, _ = _two_groups(momentum=0.9)
    cfg.ours("step", opt)
    groups = opt.state_dict()["param_groups"]
    assert all(isinstance(g["lr"], float) and g["initial_lr"] == b for g, b in zip(groups, cfg.BASES))


def test_errors():
    p = torch.zeros(2, requires_grad=True)
    with pytest.raises(TypeError, match="torch.optim.lr_scheduler"):
        L.StepLR(torch.optim.SGD([p], lr=0.1), 3)
    opt = FusedSGD([p], lr=0.1)
    with pytest.raises(ValueError, match="segments"):
        L.SequentialLR(opt, [L.ConstantLR(opt) for _ in range(5)], [2, 4, 6, 8])
    with pytest.raises(ValueError, match="milestones"):
        L.MultiStepLR(opt, list(range(17)))
    with pytest.raises(ValueError, match="ascending"):
        L.MultiStepLR(opt, [5, 3])
    with pytest.raises(ValueError, match="ascending"):
        L.SequentialLR(opt, [L.ConstantLR(opt), L.ConstantLR(opt), L.ConstantLR(opt)], [4, 4])
    with pytest.raises(ValueError, match="milestones"):
        L.SequentialLR(opt, [L.ConstantLR(opt), L.ConstantLR(opt)], [2, 4])
    with pytest.raises(ValueError):
        L.StepLR(opt, 0)
    many = FusedSGD([{"params": [torch.zeros(1, requires_grad=True)]} for _ in range(L.MAX_GROUPS + 1)], lr=0.1)
    with pytest.raises(ValueError, match="parameter groups"):
        L.StepLR(many, 3)
    L.MultiStepLR(opt, list(range(16)))  # the caps themselves are allowed
    L.SequentialLR(opt, [L.ConstantLR(opt) for _ in range(4)], [2, 4, 6])


def test_replaced_scheduler_no_longer_steps():
    opt = FusedSGD([torch.zeros(2, requires_grad=True)], lr=0.1)
    first = L.LinearLR(opt, 0.1, 1.0, 5)
    seq = L.SequentialLR(opt, [first, L.StepLR(opt, 3)], [5])
    with pytest.raises(RuntimeError):
        first.step()
    seq.step()
    assert seq.last_epoch == 1


def test_trainer_rejects_planned_engines():
    from pytorch_distributed_training_tutorials_amd.utils.trainer import Trainer

    model = torch.nn.Linear(20, 1)
    opt = FusedSGD(model.parameters(), lr=0.1)
    ds = torch.utils.data.TensorDataset(torch.randn(8, 20), torch.randn(8, 1))
    loader = torch.utils.data.DataLoader(ds, batch_size=4)
    for engine in ("persistent", "fused"):
        with pytest.raises(ValueError, match="lr_scheduler"):
            # the engine choice is refused before the communicator is used: a stand-in keeps this test
            # from creating the process-wide default one
            Trainer(model, loader, opt, 0, engine=engine, verbose=False, comm=object(),
                    lr_scheduler=lambda o: L.StepLR(o, 3))
