"""Packed plain SGD of the wave engine's lean-plain kernels (linear_wave_impl.h, layout F): per class the
values ``[W[c][0 .. KP-1], Wb[c]]`` are updated in pairs by one ``v_pk_fma_f32`` each, with the constant
pair ``{-lr, -lr}`` (``{-lr, -lr_b}`` where the bias is the second half); an odd last value stays scalar.

Each half of a packed FMA is the IEEE fma of the scalar update, so the generic kernel
(``PTDT_WAVE_GENERIC=1``, read when a plan is built) is the oracle and every comparison is bitwise
(int32 views: NaN payloads and the sign of zero count). The cases walk what decides the pairing:
every KP of the layout-F table (odd KP = 5 pairs the last weight with the bias, even KP leaves the bias
scalar), one and two classes, bias on and off (``lr_b = 0`` in the bias half), every rows-per-lane
count, and launch lengths 1, 2, 3, 4, 7, 11 over epochs of 2 steps (whole groups, both tails, wraps)."""
import pytest
import torch

LAUNCHES = [1, 2, 3, 4, 7, 11]
S = 2  # steps per epoch
# (loss, Din, Dout, B) -> layout F with KP = ceil(Din / 4) from {4, 5, 8, 10, 16}, R = B / 16
SHAPES = {
    "mse16x1_b32_k4": ("mse", 16, 1, 32),
    "mse20x1_b32_k5": ("mse", 20, 1, 32),
    "mse18x1_b16_k5pad": ("mse", 18, 1, 16),
    "mse32x1_b16_k8": ("mse", 32, 1, 16),
    "mse40x1_b32_k10": ("mse", 40, 1, 32),
    "mse64x1_b64_k16": ("mse", 64, 1, 64),
    "ces20x2_b32_k5": ("ce_soft", 20, 2, 32),
    "ces32x2_b16_k8": ("ce_soft", 32, 2, 16),
    "ces20x1_b32_k5": ("ce_soft", 20, 1, 32),  # the flagship: one class, the gradient is +0 or NaN
}


def _data(din, dout, ns, dev, scale=1.0):
    g = torch.Generator().manual_seed(23)
    X = torch.randn(ns, din, generator=g) * scale
    Y = (torch.rand(ns, dout, generator=g) + 0.125) * scale
    return X.to(dev), Y.to(dev)


def _run(kind, din, dout, B, bias, data, dev, zero_bias=False):
    from pytorch_distributed_training_tutorials_amd.data.device_sampler import DeviceDistributedSampler
    from pytorch_distributed_training_tutorials_amd.ops.fused_step import FusedMLPStep

    X, Y = data
    ns = X.shape[0]
    torch.manual_seed(3)
    model = torch.nn.Linear(din, dout, bias=bias).to(dev)
    if zero_bias:
        model.bias.data.zero_()
    eng = FusedMLPStep(model, loss=kind, lr=0.05)
    sampler = DeviceDistributedSampler(ns, 1, 0, seed=4, device=dev)
    cursor = torch.zeros(2, dtype=torch.int32, device=dev)
    losses = torch.zeros(max(LAUNCHES), device=dev)
    plan = eng.persistent_plan(X, Y, B, sampler, cursor, losses, variant="wave_f")
    assert plan.engine.startswith(f"wave:L0R{B // 16}K"), plan.engine
    snaps = []
    for n in LAUNCHES:
        plan.launch(n)
        torch.cuda.synchronize()
        snaps.append({"P": eng.P.clone(), "G": eng.G.clone(), "losses": losses[:n].clone(), "cursor": cursor.tolist()})
    return plan.kernel_variant, snaps


def _lean_and_generic(monkeypatch, *args):
    monkeypatch.delenv("PTDT_WAVE_GENERIC", raising=False)
    var, lean = _run(*args)
    assert var == "lean-plain"
    monkeypatch.setenv("PTDT_WAVE_GENERIC", "1")
    var, gen = _run(*args)
    assert var == "generic"
    return lean, gen


def _same_bits(lean, gen, keys=("P", "G", "losses")):
    for n, a, b in zip(LAUNCHES, lean, gen):
        assert a["cursor"] == b["cursor"]
        for key in keys:
            assert torch.equal(a[key].view(torch.int32), b[key].view(torch.int32)), (key, n)


@pytest.mark.gpu
@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_packed_sgd_matches_generic_bitwise(dev, monkeypatch, shape, bias):
    kind, din, dout, B = SHAPES[shape]
    data = _data(din, dout, B * S, dev)
    lean, gen = _lean_and_generic(monkeypatch, kind, din, dout, B, bias, data, dev)
    _same_bits(lean, gen)
    assert all(torch.isfinite(a["P"]).all() and torch.isfinite(a["losses"]).all() for a in lean)
    if not (kind == "ce_soft" and dout == 1):  # a real gradient moved the parameters at every launch
        assert all(a["G"].abs().sum().item() > 0 for a in lean)
        assert not torch.equal(lean[0]["P"], lean[-1]["P"])


@pytest.mark.gpu
def test_packed_sgd_subnormal_gradients(dev, monkeypatch):
    """MSE, Linear(20, 1) with a zero initial bias, inputs and targets scaled by 1e-20: dL/dz is about
    1e-21 and the weight gradients g * x about 1e-41, below the smallest normal float (1.18e-38). The
    packed halves must treat subnormal operands as the scalar fma does.

    Parameters and gradients only: the losses are subnormal too (about 1e-40), and there the lean
    kernels' loss report (raw shares scaled by the helper waves; not part of the update) differs from
    the generic kernel's in the last bit of some steps, with the scalar update as with the packed one."""
    B = 32
    data = _data(20, 1, B * S, dev, scale=1e-20)
    lean, gen = _lean_and_generic(monkeypatch, "mse", 20, 1, B, True, data, dev, True)
    _same_bits(lean, gen, ("P", "G"))
    G = lean[0]["G"]
    assert ((G != 0) & (G.abs() < 1.17549435e-38)).any(), G


@pytest.mark.gpu
def test_packed_sgd_non_finite_rows(dev, monkeypatch):
    """MSE, Linear(20, 1): one row of X holds a NaN, another an inf, in different feature groups.
    Gradients and parameters turn non-finite where the generic kernel's do, with its bits."""
    B = 32
    X, Y = _data(20, 1, B * S, dev)
    X[5, 2] = float("nan")
    X[40, 17] = float("inf")
    lean, gen = _lean_and_generic(monkeypatch, "mse", 20, 1, B, True, (X, Y), dev)
    _same_bits(lean, gen)
    assert not torch.isfinite(lean[-1]["P"]).all()
