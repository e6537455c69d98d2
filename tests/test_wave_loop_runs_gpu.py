"""Runs of unchecked groups in the wave engine's lean step loop (linear_wave_impl.h, wave_loop_schedule.h).

A lean kernel runs its unchecked three-step groups in runs under a down-counter (its own unrolled
body where the registers hold two, lean_two_bodies) and the groups around a list's end or the loss
ring's end in a checked body. tests/test_wave_step_loop_gpu.py stops at epochs of 7 steps, where no run
is longer than two groups; here the epochs are 8 to 13 and 64 steps (the benchmark's), so runs of two and
more groups occur, end at the list's end (S = 9), are cut by the steps left in the launch and by the
ring, and every residue of S against the unroll is met.

The generic kernel (``PTDT_WAVE_GENERIC=1``, read when a plan is built) keeps the per-step loop and is
the oracle: parameters, gradient bucket, momentum, losses and cursor are compared bitwise after every
launch of one plan. Every case asserts ``plan.kernel_variant``, so none passes by running generic.
B = 16 and 32 (R = 1, 2) take the two-body loop, B = 64 (R = 4) keeps one body under the per-group flag.

A barrier mismatch between the trainer and the helper waves shows as a hang: run
tests/test_wave_loop_runs.py first and this file under a time limit, and read wave_loop_schedule.h
before running it again."""
import os

import pytest
import torch

from pytorch_distributed_training_tutorials_amd.parallel.env import free_port
from pytorch_distributed_training_tutorials_amd.parallel.launcher import spawn

from . import _wave_runs_workers

SS = [8, 9, 10, 11, 13, 64]
# (loss, Din, Dout, B): R = B / 16 rows per lane
SHAPES = {
    "mse20x1_b16": ("mse", 20, 1, 16),
    "mse20x1_b32": ("mse", 20, 1, 32),
    "mse20x1_b64": ("mse", 20, 1, 64),       # one body (R = 4)
    "cei20x2_b32": ("ce_index", 20, 2, 32),  # every lane all rows (no scatter), no row image
}


def _launches(S):
    """1, 3, 6, 7; an epoch and one more; whole groups only, ending inside a run (cut by the steps left);
    several wraps; longer than the loss ring of 2 S + 3 slots (a run cut by the ring, not by the list)."""
    return [1, 3, 6, 7, S, S + 1, 3 * (S // 3), 3 * S + 2, 2 * (2 * S + 3) + 1]


def _data(kind, ns, din, dout, dev):
    g = torch.Generator().manual_seed(17)
    X = torch.randn(ns, din, generator=g)
    Y = torch.randint(0, dout, (ns,), generator=g) if kind == "ce_index" else torch.rand(ns, dout, generator=g)
    return X.to(dev), Y.to(dev)


def _run(kind, din, dout, B, ns, mom, launches, dev, engine):
    """One plan, one launch per entry of ``launches``; the state after every launch."""
    from pytorch_distributed_training_tutorials_amd.data.device_sampler import DeviceDistributedSampler
    from pytorch_distributed_training_tutorials_amd.ops.fused_step import FusedMLPStep

    X, Y = _data(kind, ns, din, dout, dev)
    torch.manual_seed(7)
    eng = FusedMLPStep(torch.nn.Linear(din, dout).to(dev), loss=kind, lr=0.05, momentum=mom)
    sampler = DeviceDistributedSampler(ns, 1, 0, seed=2, device=dev)
    cursor = torch.zeros(2, dtype=torch.int32, device=dev)
    losses = torch.zeros(max(launches), device=dev)
    plan = eng.persistent_plan(X, Y, B, sampler, cursor, losses, variant="wave_f")
    assert plan.engine.startswith(engine), plan.engine
    snaps = []
    for n in launches:
        plan.launch(n)
        torch.cuda.synchronize()
        snaps.append({"P": eng.P.clone(), "G": eng.G.clone(), "losses": losses[:n].clone(),
                      "cursor": cursor.tolist(), "mom": None if eng.mom is None else eng.mom.clone()})
    return plan.kernel_variant, snaps


def _lean_equals_generic(monkeypatch, kind, din, dout, B, S, mom, dev, engine):
    launches = _launches(S)
    args = (kind, din, dout, B, B * S, mom, launches, dev, engine)
    monkeypatch.delenv("PTDT_WAVE_GENERIC", raising=False)
    var, lean = _run(*args)
    assert var == ("lean-mom" if mom else "lean-plain")
    monkeypatch.setenv("PTDT_WAVE_GENERIC", "1")
    var, gen = _run(*args)
    assert var == "generic"
    total = 0
    for n, a, b in zip(launches, lean, gen):
        total += n
        assert a["cursor"] == [total // S, total % S] == b["cursor"], n
        assert torch.isfinite(a["losses"]).all() and a["G"].abs().sum().item() > 0  # a real gradient
        for key in ("P", "G", "losses") + (("mom",) if mom else ()):
            assert torch.equal(a[key].view(torch.int32), b[key].view(torch.int32)), (key, n)


@pytest.mark.gpu
@pytest.mark.parametrize("mom", [0.0, 0.9])
@pytest.mark.parametrize("S", SS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_runs_match_generic_bitwise(dev, monkeypatch, shape, S, mom):
    kind, din, dout, B = SHAPES[shape]
    _lean_equals_generic(monkeypatch, kind, din, dout, B, S, mom, dev, f"wave:L0R{B // 16}")


@pytest.mark.gpu
@pytest.mark.parametrize("mom", [0.0, 0.9])
def test_one_body_configuration_matches_generic_bitwise(dev, monkeypatch, mom):
    """Linear(64, 1) at B = 64: R = 4 with 16 features per lane, the configuration whose two-body kernel
    would need scratch memory; it keeps one group body under the per-group flag."""
    _lean_equals_generic(monkeypatch, "mse", 64, 1, 64, 9, mom, dev, "wave:L0R4K16")


@pytest.mark.gpu
def test_two_ranks_one_gpu_in_sync_and_equal_to_generic(tmp_path):
    """The all-reduce lean kernel (two bodies, its `failed` exit per group not taken) on two ranks that
    share one GPU: equal to the generic kernel on each rank, parameters and gradients equal across ranks."""
    world, S = 2, _wave_runs_workers.S
    spawn(_wave_runs_workers.lean_and_generic_two_ranks, args=(world, free_port(), str(tmp_path)), nprocs=world)
    res = [torch.load(os.path.join(tmp_path, f"r{r}.pt"), weights_only=True) for r in range(world)]
    total = sum(_wave_runs_workers.LAUNCHES)
    for r in res:
        assert r["lean_variant"] == "lean-plain" and r["generic_variant"] == "generic"
        assert r["lean_engine"].startswith("wave:L0R2") and r["generic_engine"].startswith("wave:L0R2")
        assert torch.equal(r["lean"].view(torch.int32), r["generic"].view(torch.int32))
        assert r["lean_cursor"].tolist() == r["generic_cursor"].tolist() == [total // S, total % S]
    n_state, k = 21 + 21, 0  # parameters and gradient bucket: identical on both ranks (the losses are per rank)
    for steps in _wave_runs_workers.LAUNCHES:
        assert torch.equal(res[0]["lean"][k:k + n_state], res[1]["lean"][k:k + n_state])
        k += n_state + steps
    assert torch.isfinite(res[0]["lean"]).all()
