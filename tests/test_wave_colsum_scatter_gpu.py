"""Reduce-scattered column sums of the lean-plain hand-placed step (linear_wave_impl.h: hand_step_2x5_rs,
hand_sgd_bcast, hand_run_end).

The unchecked group body of the lean-plain kernels of Linear(17..20, 1) at B = 32 adds the six backward
column sums as a reduce-scatter over the 16 lanes of a DPP row (13 adds; each total ends in one bank of
one of two registers), and plain SGD reads each total from its lane with ``row_newbcast``. The gradient
the launch stores is formed from the two registers once, where a run of unchecked groups ends; a checked
group or the tail behind the run overwrites it.

The generic kernel (``PTDT_WAVE_GENERIC=1``, read when a plan is built) is the oracle: parameters,
gradient bucket, losses, optimizer step counter and cursor are compared bitwise after every launch of
one plan, and ``plan.kernel_variant`` is asserted in every case.

Launch lengths (groups are three steps): 3 and 6 end with a hand step, so ``G`` comes from the run-end
broadcast; 4 and 7 end in the tail; S + 1 and 3 S + 2 have a checked group behind a run. The features
are ``X[:, k] = (k + 1) * randn``: the six column totals of a feature group differ, so two values'
lanes or two broadcast lanes swapped show in ``P`` (the step size is 1e-4: the largest feature has
twenty times the unit scale, and mean-squared error diverges from about 3e-4). With ``mse`` the gradients are real
(``G.abs().sum() > 0``); soft-target cross-entropy of one class has a gradient that is identically
zero, so there the losses and the untouched parameters are what is compared.

A wait mismatch in this kernel shows as a hang: run this file alone first, under a time limit."""
import pytest
import torch

B = 32
SS = [8, 64]


def _launches(S):
    return [3, 6, 4, 7, S + 1, 3 * S + 2]


def _data(din, ns, dev):
    g = torch.Generator().manual_seed(23)
    X = torch.randn(ns, din, generator=g) * torch.arange(1, din + 1, dtype=torch.float32)
    Y = torch.rand(ns, 1, generator=g)
    return X.to(dev), Y.to(dev)


def _run(kind, din, bias, S, dev):
    """One plan, one launch per entry of ``_launches(S)``; the state after every launch."""
    from pytorch_distributed_training_tutorials_amd.data.device_sampler import DeviceDistributedSampler
    from pytorch_distributed_training_tutorials_amd.ops.fused_step import FusedMLPStep

    ns, launches = B * S, _launches(S)
    X, Y = _data(din, ns, dev)
    torch.manual_seed(11)
    eng = FusedMLPStep(torch.nn.Linear(din, 1, bias=bias).to(dev), loss=kind, lr=1e-4, momentum=0.0)
    sampler = DeviceDistributedSampler(ns, 1, 0, seed=5, device=dev)
    cursor = torch.zeros(2, dtype=torch.int32, device=dev)
    losses = torch.zeros(max(launches), device=dev)
    plan = eng.persistent_plan(X, Y, B, sampler, cursor, losses, variant="wave_f")
    assert plan.engine.startswith("wave:L0R2"), plan.engine
    snaps = []
    for n in launches:
        plan.launch(n)
        torch.cuda.synchronize()
        snaps.append({"P": eng.P.clone(), "G": eng.G.clone(), "losses": losses[:n].clone(), "cursor": cursor.tolist(),
                      "opt_step": int(eng.opt_step.item())})
    return plan.kernel_variant, snaps


@pytest.mark.gpu
@pytest.mark.parametrize("S", SS)
@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("din", [20, 17])
@pytest.mark.parametrize("kind", ["mse", "ce_soft"])
def test_scattered_sums_match_generic_bitwise(dev, monkeypatch, kind, din, bias, S):
    monkeypatch.delenv("PTDT_WAVE_GENERIC", raising=False)
    var, lean = _run(kind, din, bias, S, dev)
    assert var == "lean-plain"
    monkeypatch.setenv("PTDT_WAVE_GENERIC", "1")
    var, gen = _run(kind, din, bias, S, dev)
    assert var == "generic"
    total = 0
    for n, a, b in zip(_launches(S), lean, gen):
        total += n
        assert a["cursor"] == [total // S, total % S] == b["cursor"], n
        assert a["opt_step"] == total == b["opt_step"], n
        assert torch.isfinite(a["losses"]).all(), n
        if kind == "mse":
            assert a["G"].abs().sum().item() > 0, n  # a real gradient
        for key in ("P", "G", "losses"):
            assert torch.equal(a[key].view(torch.int32), b[key].view(torch.int32)), (key, n)
