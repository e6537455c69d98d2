"""Plan-time kernel variants of the single-wave engine's layout F (linear_wave_impl.h).

A lean variant is today's kernel minus the code its plan can never run (other SGD kinds, the
no-ring loss path, short-batch masks, the stamps): the results must be the generic kernel's, bit
for bit. The generic kernel is forced with ``PTDT_WAVE_GENERIC=1`` (read when a plan is built)."""
import pytest
import torch
import torch.nn.functional as F

B = 32
LOSS_ID = {"ce_soft": 0, "ce_index": 1, "mse": 2}


def _data(kind, ns, dev):
    g = torch.Generator().manual_seed(11)
    X = torch.randn(ns, 20, generator=g)
    if kind == "mse":
        Y = torch.rand(ns, 1, generator=g)
    else:
        Y = torch.randint(0, 2, (ns,), generator=g)
    return X.to(dev), Y.to(dev)


def _engine(kind, mom, dev, **kw):
    from pytorch_distributed_training_tutorials_amd.ops.fused_step import FusedMLPStep

    torch.manual_seed(7)
    model = torch.nn.Linear(20, 1 if kind == "mse" else 2).to(dev)
    return FusedMLPStep(model, loss=kind, lr=0.05, momentum=mom, **kw)


def _run(kind, ns, mom, launches, dev, seed=2):
    """One plan, one launch per entry of ``launches``; the state after every launch."""
    from pytorch_distributed_training_tutorials_amd.data.device_sampler import DeviceDistributedSampler

    X, Y = _data(kind, ns, dev)
    eng = _engine(kind, mom, dev)
    sampler = DeviceDistributedSampler(ns, 1, 0, seed=seed, device=dev)
    cursor = torch.zeros(2, dtype=torch.int32, device=dev)
    losses = torch.zeros(max(launches), device=dev)
    plan = eng.persistent_plan(X, Y, B, sampler, cursor, losses)
    assert plan.engine.startswith("wave:L0")
    snaps = []
    for n in launches:
        plan.launch(n)
        torch.cuda.synchronize()
        snaps.append({"P": eng.P.clone(), "G": eng.G.clone(), "losses": losses[:n].clone(),
                      "cursor": cursor.clone(), "mom": None if eng.mom is None else eng.mom.clone()})
    return plan.kernel_variant, snaps, eng


@pytest.mark.gpu
@pytest.mark.parametrize("mom", [0.0, 0.9])
@pytest.mark.parametrize("ns", [64, 96])
@pytest.mark.parametrize("kind", ["mse", "ce_index"])
def test_lean_matches_generic_bitwise(dev, monkeypatch, kind, ns, mom):
    """Parameters, momentum, gradient bucket, losses and cursor after launches of 1, 5, S + 1 and
    3 S + 2 steps (epoch wraps inside and between launches): lean == generic, bitwise."""
    S = ns // B
    launches = [1, 5, S + 1, 3 * S + 2]
    monkeypatch.delenv("PTDT_WAVE_GENERIC", raising=False)
    var, lean, _ = _run(kind, ns, mom, launches, dev)
    assert var == ("lean-mom" if mom else "lean-plain")
    monkeypatch.setenv("PTDT_WAVE_GENERIC", "1")
    var, gen, _ = _run(kind, ns, mom, launches, dev)
    assert var == "generic"
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
def test_variant_selection(dev, monkeypatch):
    from pytorch_distributed_training_tutorials_amd.data.device_sampler import DeviceDistributedSampler
    from pytorch_distributed_training_tutorials_amd.models.toy import ddp_toy_model
    from pytorch_distributed_training_tutorials_amd.ops.fused_step import FusedMLPStep

    monkeypatch.delenv("PTDT_WAVE_GENERIC", raising=False)

    def variant(kind, ns, stamps=False, **kw):
        X, Y = _data(kind, ns, dev)
        eng = _engine(kind, kw.pop("mom", 0.0), dev, **kw)
        sampler = DeviceDistributedSampler(ns, 1, 0, seed=2, device=dev)
        st = torch.zeros(16, dtype=torch.int64, device=dev) if stamps else None
        plan = eng.persistent_plan(X, Y, B, sampler, torch.zeros(2, dtype=torch.int32, device=dev),
                                   torch.zeros(8, device=dev), stamps=st)
        assert plan.engine.startswith("wave:L0")
        return plan.kernel_variant

    assert variant("mse", 64) == "lean-plain"
    assert variant("mse", 64, mom=0.9) == "lean-mom"
    assert variant("mse", 80) == "generic"  # short last batch
    assert variant("mse", 64, weight_decay=1e-3) == "generic"
    assert variant("mse", 64, stamps=True) == "generic"
    # the flagship: Linear(20, 1), soft-target CE, plain SGD, 2048 samples in batches of 32
    g = torch.Generator().manual_seed(0)
    X, Y = torch.rand(2048, 20, generator=g).to(dev), torch.rand(2048, 1, generator=g).to(dev)
    eng = FusedMLPStep(ddp_toy_model().to(dev), loss="ce_soft", lr=1e-2)
    sampler = DeviceDistributedSampler(2048, 1, 0, seed=0, device=dev)
    plan = eng.persistent_plan(X, Y, B, sampler, torch.zeros(2, dtype=torch.int32, device=dev),
                               torch.zeros(8, device=dev))
    assert plan.engine == "wave:L0R2K5"  # the engine string does not name the variant
    assert plan.kernel_variant == "lean-plain"


def test_variant_query_strings(native, monkeypatch):
    """The same rules through the string-level query (no GPU needed)."""
    monkeypatch.delenv("PTDT_WAVE_GENERIC", raising=False)
    q = native.persistent_kernel_variant
    ce_soft, mse = LOSS_ID["ce_soft"], LOSS_ID["mse"]
    assert q(32, 20, 0, 1, ce_soft, 2048, 1) == "lean-plain"  # flagship
    assert q(32, 20, 0, 1, ce_soft, 2048, 1, momentum=0.9) == "lean-mom"
    assert q(32, 20, 0, 1, mse, 80, 1) == "generic"  # short last batch
    assert q(32, 20, 0, 1, mse, 64, 1, weight_decay=1e-3) == "generic"
    assert q(32, 20, 0, 1, mse, 64, 1, stamps=True) == "generic"
    assert q(24, 20, 0, 1, mse, 48, 1) == "generic"  # full batches, but not 16 rows per row slot group
    assert q(32, 20, 0, 1, ce_soft, 2048, 1, variant=3) == "generic"  # rows layout: no lean variants
    assert q(32, 20, 64, 10, 1, 2048, 1) == ""  # not the wave engine
    monkeypatch.setenv("PTDT_WAVE_GENERIC", "1")
    assert q(32, 20, 0, 1, ce_soft, 2048, 1) == "generic"


@pytest.mark.gpu
def test_lean_mse_matches_torch(dev, monkeypatch):
    """A lean MSE run against torch.nn.Linear + F.mse_loss + torch.optim.SGD (fp32) on the same
    index order; the tolerance of the wave-vs-native comparisons in test_xgmi_gpu.py."""
    from pytorch_distributed_training_tutorials_amd.data.device_sampler import reference_indices

    monkeypatch.delenv("PTDT_WAVE_GENERIC", raising=False)
    ns, mom, n_steps = 64, 0.9, 7
    var, snaps, eng = _run("mse", ns, mom, [n_steps], dev)
    assert var == "lean-mom"
    X, Y = _data("mse", ns, torch.device("cpu"))
    torch.manual_seed(7)
    model = torch.nn.Linear(20, 1)
    opt = torch.optim.SGD(model.parameters(), lr=0.05, momentum=mom)
    S, ref_losses = ns // B, []
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
