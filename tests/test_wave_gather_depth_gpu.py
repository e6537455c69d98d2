"""Gather depth per kernel in the wave engine's lean step loop (wave_gather_depth in
csrc/kernels/wave_kernel_rules.h): the two-body lean kernels without the in-kernel all-reduce keep D
batches of row gathers in flight, every other kernel keeps kWavePrefetch = 3.

The scheme is tests/test_wave_step_loop_gpu.py's: the generic kernel (``PTDT_WAVE_GENERIC=1``, read
when a plan is built) keeps depth 3 and the per-step loop and is the oracle; parameters, gradient
bucket, momentum, losses and cursor are compared bitwise after every launch of one plan. Every case
asserts ``plan.kernel_variant``, so none passes by running generic. The dataset is B S rows.

A barrier mismatch between the trainer and the helper waves shows as a hang: run this file under a
time limit, and read wave_loop_schedule.h (tests/test_wave_gather_depth.py) before running it again."""
import pytest
import torch

D = 4  # wave_gather_depth of the deepened kernels
SS = list(range(1, D + 3))  # every residue against the D-step unroll, and S < D
# (loss, Din, Dout, B)
SHAPES = {
    "mse20x1_b32": ("mse", 20, 1, 32),          # hand-step kernel <2,5,1>
    "mse17x1_b32": ("mse", 17, 1, 32),          # the same kernel, a padded feature group
    "ce_soft20x1_b32": ("ce_soft", 20, 1, 32),  # the benchmark's kernel: zero gradient by construction, bits only
    "mse16x1_b32": ("mse", 16, 1, 32),          # <2,4,1>: deepened, the compiler's step in every body
    "mse20x1_b64": ("mse", 20, 1, 64),          # <4,5,1>: one group body, keeps depth 3 (the control)
}


def _launches(S):
    """Shorter than the depth, equal to it, every n % D, several wraps inside a launch, a wrap at a
    launch's end, and one launch longer than the loss ring (2 S + D slots)."""
    return list(range(1, D + 2)) + [S, S + 1, 3 * S + 2, 2 * (2 * S + D) + 1]


def _data(kind, ns, din, dout, dev):
    g = torch.Generator().manual_seed(11)
    X = torch.randn(ns, din, generator=g)
    Y = torch.rand(ns, dout, generator=g)
    return X.to(dev), Y.to(dev)


def _run(kind, din, dout, B, ns, mom, launches, dev):
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
    assert plan.engine.startswith(f"wave:L0R{B // 16}"), plan.engine
    snaps = []
    for n in launches:
        plan.launch(n)
        torch.cuda.synchronize()
        snaps.append({"P": eng.P.clone(), "G": eng.G.clone(), "losses": losses[:n].clone(),
                      "cursor": cursor.clone(), "mom": None if eng.mom is None else eng.mom.clone()})
    return plan.kernel_variant, snaps


@pytest.mark.gpu
@pytest.mark.parametrize("mom", [0.0, 0.9])
@pytest.mark.parametrize("S", SS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_gather_depth_matches_generic_bitwise(dev, monkeypatch, shape, S, mom):
    kind, din, dout, B = SHAPES[shape]
    launches = _launches(S)
    args = (kind, din, dout, B, B * S, mom, launches, dev)
    monkeypatch.delenv("PTDT_WAVE_GENERIC", raising=False)
    var, lean = _run(*args)
    assert var == ("lean-mom" if mom else "lean-plain")
    monkeypatch.setenv("PTDT_WAVE_GENERIC", "1")
    var, gen = _run(*args)
    assert var == "generic"
    total = 0
    for n, a, b in zip(launches, lean, gen):
        total += n
        assert a["cursor"].tolist() == [total // S, total % S] == b["cursor"].tolist()
        if kind == "mse":
            assert torch.isfinite(a["losses"]).all() and a["G"].abs().sum().item() > 0  # a real gradient
        for key in ("P", "G", "losses"):
            assert torch.equal(a[key].view(torch.int32), b[key].view(torch.int32)), (key, n)
        if mom:
            assert torch.equal(a["mom"].view(torch.int32), b["mom"].view(torch.int32)), ("mom", n)
