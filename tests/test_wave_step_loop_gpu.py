"""The lean step loop of the wave engine's layout F (linear_wave_impl.h): unchecked groups inside one
epoch list, checked groups around a wrap, one wait per batch, running list / loss-ring addresses, the
loss share scaled and masked in the helper waves.

The generic kernel (``PTDT_WAVE_GENERIC=1``, read when a plan is built) keeps the per-step loop and is
the oracle: parameters, gradient bucket, momentum, losses and cursor are compared bitwise after every
launch of one plan. Every case asserts ``plan.kernel_variant``, so none passes by running generic.

A barrier mismatch between the trainer and the helper waves shows as a hang: run this file under a
time limit, and read wave_loop_schedule.h (tests/test_wave_loop_schedule.py) before running it again."""
import pytest
import torch
import torch.nn.functional as F

SS = [1, 2, 3, 4, 5, 7]  # epoch lengths in steps: every residue against the 3-step unroll
# (loss, Din, Dout, B): R = B / 16 rows per lane; Dout == 1 with R > 1 is the reduce-scatter path
SHAPES = {
    "mse20x1_b16": ("mse", 20, 1, 16),
    "mse20x1_b32": ("mse", 20, 1, 32),
    "mse20x1_b64": ("mse", 20, 1, 64),
    "cei20x2_b32": ("ce_index", 20, 2, 32),  # every lane all rows (no scatter)
    "mse7x1_b32": ("mse", 7, 1, 32),         # a padded feature group
}


def _launches(S):
    """Shorter than the prefetch depth, equal to it, every n % 3, several wraps inside a launch, a wrap
    at a launch's end, and one launch longer than the loss ring (2 S + 3 slots)."""
    return [1, 2, 3, 4, S, S + 1, 3 * S + 2, 2 * (2 * S + 3) + 1]


def _data(kind, ns, din, dout, dev):
    g = torch.Generator().manual_seed(11)
    X = torch.randn(ns, din, generator=g)
    Y = torch.randint(0, dout, (ns,), generator=g) if kind == "ce_index" else torch.rand(ns, dout, generator=g)
    return X.to(dev), Y.to(dev)


def _run(kind, din, dout, B, ns, mom, launches, dev, data=None, seed=2):
    """One plan, one launch per entry of ``launches``; the state after every launch."""
    from pytorch_distributed_training_tutorials_amd.data.device_sampler import DeviceDistributedSampler
    from pytorch_distributed_training_tutorials_amd.ops.fused_step import FusedMLPStep

    X, Y = data if data is not None else _data(kind, ns, din, dout, dev)
    torch.manual_seed(7)
    eng = FusedMLPStep(torch.nn.Linear(din, dout).to(dev), loss=kind, lr=0.05, momentum=mom)
    sampler = DeviceDistributedSampler(ns, 1, 0, seed=seed, device=dev)
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


def _lean_and_generic(monkeypatch, *args, **kw):
    mom = args[5]
    monkeypatch.delenv("PTDT_WAVE_GENERIC", raising=False)
    var, lean = _run(*args, **kw)
    assert var == ("lean-mom" if mom else "lean-plain")
    monkeypatch.setenv("PTDT_WAVE_GENERIC", "1")
    var, gen = _run(*args, **kw)
    assert var == "generic"
    return lean, gen


@pytest.mark.gpu
@pytest.mark.parametrize("mom", [0.0, 0.9])
@pytest.mark.parametrize("S", SS)  # none dropped: the plan takes S = 1 and 2
@pytest.mark.parametrize("shape", list(SHAPES))
def test_step_loop_matches_generic_bitwise(dev, monkeypatch, shape, S, mom):
    kind, din, dout, B = SHAPES[shape]
    launches = _launches(S)
    lean, gen = _lean_and_generic(monkeypatch, kind, din, dout, B, B * S, mom, launches, dev)
    total = 0
    for n, a, b in zip(launches, lean, gen):
        total += n
        assert a["cursor"].tolist() == [total // S, total % S] == b["cursor"].tolist()
        assert torch.isfinite(a["losses"]).all() and a["G"].abs().sum().item() > 0  # a real gradient
        for key in ("P", "G", "losses"):
            assert torch.equal(a[key], b[key]), (key, n)
        if mom:
            assert torch.equal(a["mom"], b["mom"]), ("mom", n)


@pytest.mark.gpu
def test_non_finite_loss_row(dev, monkeypatch):
    """ce_soft, Linear(20, 1), B = 32, one row of X with an inf and a zero target, the other rows with
    nonzero targets: that row's loss, -0 * NaN, is NaN. ``losses`` must be the generic kernel's bits:
    finite before the row's batch, NaN in it, and NaN after it too, because that step's update makes
    the parameters NaN (so only the steps before the row's batch can be checked as finite).

    With R = 2 every batch row is computed in an owner DPP row q < 2 and again in q + 2, so the step's
    sum is NaN whether or not the helper waves zero the non-owner copy: this test pins the NaN
    propagation and the bits, it cannot tell a missing owner select. What guards the select and the
    scale that moved to the helper waves is the bitwise finite cases above, where a share counted
    twice or unscaled changes ``losses``."""
    from pytorch_distributed_training_tutorials_amd.data.device_sampler import reference_indices

    B, S, mom = 32, 3, 0.0
    ns = B * S
    order = torch.from_numpy(reference_indices(ns, 1, 0, 0, seed=2)).long()
    bad = int(order[B + 16 + 3])  # epoch 0, step 1, batch slot 19: row slot i = 3, rho = 1
    g = torch.Generator().manual_seed(5)
    X = torch.randn(ns, 20, generator=g)
    Y = torch.rand(ns, 1, generator=g) + 0.25
    Y[bad] = 0.0
    X[bad, 3] = float("inf")
    launches = [1, S + 1]  # step 0 alone (finite), then steps 1 .. S + 1 (the row's batch first)
    data = (X.to(dev), Y.to(dev))
    lean, gen = _lean_and_generic(monkeypatch, "ce_soft", 20, 1, B, ns, mom, launches, dev, data=data)
    for a, b in zip(lean, gen):
        assert torch.equal(a["losses"].view(torch.int32), b["losses"].view(torch.int32))  # NaN or not, the same bits
        assert torch.equal(a["P"].view(torch.int32), b["P"].view(torch.int32))
        assert a["cursor"].tolist() == b["cursor"].tolist()
    assert torch.isfinite(lean[0]["losses"]).all() and torch.isfinite(lean[0]["P"]).all()
    assert torch.isnan(lean[1]["losses"]).all()


@pytest.mark.gpu
def test_lean_mse_matches_torch(dev, monkeypatch):
    """A lean MSE run of n = 3 S + 2 steps at S = 4 against torch.nn.Linear + F.mse_loss +
    torch.optim.SGD (fp32) on the same index order; the tolerances of test_wave_variants_gpu.py."""
    from pytorch_distributed_training_tutorials_amd.data.device_sampler import reference_indices

    monkeypatch.delenv("PTDT_WAVE_GENERIC", raising=False)
    B, S, mom = 32, 4, 0.0
    ns, n_steps = B * S, 3 * S + 2
    var, snaps = _run("mse", 20, 1, B, ns, mom, [n_steps], dev)
    assert var == "lean-plain"
    X, Y = _data("mse", ns, 20, 1, torch.device("cpu"))
    torch.manual_seed(7)
    model = torch.nn.Linear(20, 1)
    opt = torch.optim.SGD(model.parameters(), lr=0.05, momentum=mom)
    ref_losses = []
    for step in range(n_steps):
        order = torch.from_numpy(reference_indices(ns, 1, 0, step // S, seed=2)).long()
        rows = order[(step % S) * B:(step % S + 1) * B]
        opt.zero_grad()
        loss = F.mse_loss(model(X[rows]), Y[rows])
        loss.backward()
        opt.step()
        ref_losses.append(loss.detach())
    ref = torch.cat([p.detach().reshape(-1) for p in model.parameters()])
    torch.testing.assert_close(snaps[0]["P"].cpu(), ref, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(snaps[0]["losses"].cpu(), torch.stack(ref_losses), rtol=1e-4, atol=1e-5)
