"""FusedLARS / FusedLAMB without a GPU: the CPU path against the float64 definition
(tests/_layerwise_ref.py), the parameter groups, checkpoints, and how the clipper, the schedulers
and the Trainer take the two classes. fp32 tolerance as tests/test_optim_semantics.py."""
import copy

import pytest
import torch

from pytorch_distributed_training_tutorials_amd.ops import (FusedAdam, FusedLAMB, FusedLARS, FusedSGD, GradClipper,
                                                            LinearLR, layerwise_param_groups)

from ._layerwise_ref import lamb_run, lars_run

RTOL, ATOL = 1e-5, 1e-6
# the geometry list of the GPU tests (tests/test_layerwise_optim_gpu.py)
SHAPES = [(1,), (3,), (4095,), (4096,), (4097,), (2 * 4096 + 5,), (64, 3, 7, 7), (17, 33)] + [(5,)] * 30
LARS_KW = dict(lr=0.2, momentum=0.9, weight_decay=1e-2, trust_coefficient=0.1)
LAMB_KW = dict(lr=0.05, weight_decay=1e-2)


def _case(seed, steps, shapes=SHAPES):
    gen = torch.Generator().manual_seed(seed)
    ps = [torch.randn(s, generator=gen) for s in shapes]
    grads = [[torch.randn(s, generator=gen) for s in shapes] for _ in range(steps)]
    return ps, grads


def _run(opt_cls, ps, grads, **kw):
    qs = [torch.nn.Parameter(p.clone()) for p in ps]
    opt = opt_cls(qs, **kw)
    for gs in grads:
        for q, g in zip(qs, gs):
            q.grad = g.clone()
        opt.step()
    return qs, opt


def _close(got, want):
    for q, r in zip(got, want):
        torch.testing.assert_close(q.detach().double(), r, rtol=RTOL, atol=ATOL)


@pytest.mark.parametrize("kw", [LARS_KW, dict(LARS_KW, nesterov=True), dict(LARS_KW, momentum=0.0, maximize=True),
                                dict(LARS_KW, dampening=0.5, weight_decay=0.0)])
def test_cpu_lars_matches_the_definition(kw):
    ps, grads = _case(1, 5)
    qs, opt = _run(FusedLARS, ps, grads, **kw)
    want, _, ratios = lars_run(ps, grads, [{}] * 5, **kw)
    _close(qs, want)
    got = opt.trust_ratios()
    for q, r in zip(qs, ratios):
        assert got[q][0] == pytest.approx(r, rel=1e-5)


@pytest.mark.parametrize("kw", [LAMB_KW, dict(LAMB_KW, bias_correction=False), dict(LAMB_KW, weight_decay=0.0),
                                dict(LAMB_KW, adapt=False), dict(LAMB_KW, maximize=True)])
def test_cpu_lamb_matches_the_definition(kw):
    ps, grads = _case(2, 5)
    qs, opt = _run(FusedLAMB, ps, grads, **kw)
    want, _, _, ratios = lamb_run(ps, grads, [{}] * 5, **kw)
    _close(qs, want)
    got = opt.trust_ratios()
    for q, r in zip(qs, ratios):
        assert got[q][0] == pytest.approx(r, rel=1e-5)
    if not kw.get("adapt", True):
        assert all(r == 1.0 for r in ratios)


def test_fp32_evaluation_of_the_definition_sits_well_inside_the_band():
    """The formulae evaluated in plain float32 torch, 5 steps on the geometry list, use a small part
    of the 1e-5 / 1e-6 band against float64: the band leaves room for another summation order and is
    no loosened one. Asserted at a tenth of the band."""
    for run, kw, seed in ((lars_run, LARS_KW, 1), (lamb_run, LAMB_KW, 2)):
        ps, grads = _case(seed, 5)
        want = run(ps, grads, [{}] * 5, **kw)[0]
        got = run(ps, grads, [{}] * 5, dtype=torch.float32, **kw)[0]
        worst = max(float(((g.double() - w).abs() / (ATOL + RTOL * w.abs())).max()) for g, w in zip(got, want))
        print(f"[measured] {run.__name__}: float32 evaluation uses {100 * worst:.2f} % of the band")
        assert worst < 0.1


class _Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.conv = torch.nn.Conv2d(3, 4, 3, bias=True)
        self.bn = torch.nn.BatchNorm2d(4)
        self.fc = torch.nn.Linear(4, 2)


def test_layerwise_param_groups():
    net = _Net()
    groups = layerwise_param_groups(net, 1e-4)
    assert [id(p) for p in groups[0]["params"]] == [id(net.conv.weight), id(net.fc.weight)]
    assert [id(p) for p in groups[1]["params"]] == [id(net.conv.bias), id(net.bn.weight), id(net.bn.bias),
                                                     id(net.fc.bias)]
    assert groups[0] == {"params": groups[0]["params"], "weight_decay": 1e-4}
    assert groups[1]["weight_decay"] == 0.0 and groups[1]["trust_coefficient"] == 0.0
    lamb = layerwise_param_groups(net, 1e-4, adapt=False)
    assert lamb[1]["adapt"] is False and "trust_coefficient" not in lamb[1]
    opt = FusedLARS(groups, lr=0.1, momentum=0.9)
    assert opt.param_groups[0]["trust_coefficient"] == 1e-3 and opt.param_groups[1]["trust_coefficient"] == 0.0
    opt = FusedLAMB(lamb, lr=0.1)
    assert opt.param_groups[0]["adapt"] is True and opt.param_groups[1]["adapt"] is False
    net.fc.bias.requires_grad_(False)
    assert sum(len(g["params"]) for g in layerwise_param_groups(net, 0.0)) == 5


def test_unadapted_cpu_group_is_fused_sgd():
    ps, grads = _case(3, 3, SHAPES[:8])
    kw = dict(lr=0.1, momentum=0.9, weight_decay=1e-2)
    a, _ = _run(FusedLARS, ps, grads, trust_coefficient=0.0, **kw)
    b, _ = _run(FusedSGD, ps, grads, **kw)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("parent,child,kw", [(FusedSGD, FusedLARS, dict(lr=0.1, momentum=0.9)),
                                             (FusedAdam, FusedLAMB, dict(lr=0.1))])
def test_state_dict_round_trips_with_the_parent_class(parent, child, kw):
    ps, grads = _case(4, 2, SHAPES[:8])
    extra = {"trust_coefficient": 0.02, "eps": 1e-8} if child is FusedLARS else {"bias_correction": True, "adapt": False}
    for src, dst in ((parent, child), (child, parent)):
        qs, opt = _run(src, ps, grads, **kw)
        sd = copy.deepcopy(opt.state_dict())
        rs = [torch.nn.Parameter(q.detach().clone()) for q in qs]
        new = dst(rs, **kw, **(extra if dst is child else {}))
        new.load_state_dict(sd)
        state_key = "momentum_buffer" if parent is FusedSGD else "exp_avg"
        for q, r in zip(qs, rs):
            assert torch.equal(new.state[r][state_key], opt.state[q][state_key])
        if dst is child:  # the parent's checkpoint has no layer-wise keys: the constructed values stay
            assert all(new.param_groups[0][k] == v for k, v in extra.items())
        if parent is FusedAdam:
            assert all(float(new.state_dict()["state"][i]["step"]) == 2.0 for i in range(len(rs)))
        for r, g in zip(rs, grads[0]):
            r.grad = g.clone()
        new.step()  # the loaded optimizer steps


def test_clipper_and_schedulers_accept_both_classes():
    for cls, kw in ((FusedLARS, dict(lr=0.5, momentum=0.9, trust_coefficient=0.1)), (FusedLAMB, dict(lr=0.5))):
        ps, grads = _case(5, 4, SHAPES[:8])
        qs = [torch.nn.Parameter(p.clone()) for p in ps]
        opt = cls(qs, **kw)
        sched = LinearLR(opt, start_factor=0.25, total_iters=3)
        clipper = GradClipper(qs, 0.5, optimizer=opt)
        lrs, coefs = [], []
        for gs in grads:
            for q, g in zip(qs, gs):
                q.grad = g.clone()
            lrs.append(opt.param_groups[0]["lr"])
            clipper()
            coefs.append(float(clipper.coef))
            opt.step()
            sched.step()
        assert lrs == pytest.approx([0.125, 0.25, 0.375, 0.5]) and all(c < 1 for c in coefs)
        run = lars_run if cls is FusedLARS else lamb_run
        want = run(ps, grads, [dict(lr=lr, gcoef=c) for lr, c in zip(lrs, coefs)], **{**kw})[0]
        _close(qs, want)


def test_trainer_takes_the_autograd_engine_and_refuses_a_forced_fused_one():
    from pytorch_distributed_training_tutorials_amd.utils.trainer import Trainer, _sgd_hparams

    model = torch.nn.Linear(20, 1)
    for opt in (FusedLARS(model.parameters(), lr=0.1, momentum=0.9), FusedLAMB(model.parameters(), lr=0.1)):
        assert _sgd_hparams(opt) is None
        t = Trainer.__new__(Trainer)  # engine choice only: no process group, no data
        t.optimizer, t.max_grad_norm, t.lr_scheduler = opt, None, None
        t.device, t.train_dataloader = torch.device("cpu"), None
        assert t._select_engine("auto", model) == "autograd"
        for engine in ("fused", "persistent"):
            with pytest.raises(ValueError, match="layer-wise"):
                t._select_engine(engine, model)


def test_constructor_validation():
    p = [torch.nn.Parameter(torch.zeros(3))]
    with pytest.raises(ValueError):
        FusedLARS(p, lr=0.1, trust_coefficient=-1e-3)
    with pytest.raises(ValueError):
        FusedLARS(p, lr=0.1, eps=-1e-8)
    with pytest.raises(ValueError):
        FusedLARS([{"params": p, "trust_coefficient": -1.0}], lr=0.1)
    with pytest.raises(ValueError):
        FusedLAMB(p, lr=0.1, eps=-1e-6)
    with pytest.raises(ValueError):
        FusedLARS(p, lr=-0.1)
