"""The wave engine's row image on the GPU (csrc/kernels/wave_row_image.h): the pack kernel against an
image built with torch, and the lean kernels that gather from the image (layout F, one output, MSE and
soft-target CE) against the generic kernel, which reads X and Y (``PTDT_WAVE_GENERIC=1``, read when a
plan is built). Every comparison is bitwise (int32 views: NaN payloads and the sign of zero count):
parameters, gradient bucket, momentum, losses and cursor after every launch of one plan.

What the image changes in a step, and the case that walks it: the record gather with 16-byte loads
(Din 20: no padding; Din 18: zeros inside the last record; Din 8: an even KP, no 1.0 slot), the own
row's target chosen from the R loaded ones (B = 16, 32, 64: R = 1, 2, 4), the packed backward tail
{x[KP-1], 1} . {g, g} behind an odd KP (bias on and off; subnormal and non-finite values), launches
of 1, 2, 3, 4, 7, 11 steps over epochs of 3, 5, 6 and 10 steps (whole groups, the tails that gather nothing,
epoch wraps and the loss ring's wrap), and a dataset changed in place between two plans."""
import os

import pytest
import torch

from pytorch_distributed_training_tutorials_amd.parallel.env import free_port
from pytorch_distributed_training_tutorials_amd.parallel.launcher import spawn

from . import _wave_image_workers

LAUNCHES = [1, 2, 3, 4, 7, 11]
# (Din, B): R = B / 16 rows per lane, KP = 5 except Din 8 (KP 4)
SHAPES = {"d20_b32": (20, 32), "d18_b32": (18, 32), "d20_b16": (20, 16), "d20_b64": (20, 64), "d8_b32": (8, 32)}


def _torch_image(X, Y, din, kp):
    n = X.shape[0]
    rs = (kp + kp % 2 + 1 + 3) // 4 * 4
    xp = torch.zeros(n, 4 * kp, device=X.device)
    xp[:, :din] = X
    img = torch.zeros(n, 4, rs, device=X.device)
    img[:, :, :kp] = xp.view(n, 4, kp)
    if kp % 2:
        img[:, :, kp] = 1.0
    img[:, :, kp + kp % 2] = Y.reshape(n, 1)
    return img.view(n, 4 * rs)


@pytest.mark.gpu
@pytest.mark.parametrize("din,kp", [(17, 5), (18, 5), (20, 5), (8, 4), (30, 8), (40, 10), (64, 16)])
@pytest.mark.parametrize("n", [1, 33, 96])
def test_pack_kernel_matches_torch_image(dev, native, n, din, kp):
    g = torch.Generator().manual_seed(n * 100 + din)
    X = torch.randn(n, din, generator=g).to(dev)
    Y = torch.randn(n, 1, generator=g).to(dev)
    X[0, din - 1] = float("nan")  # bits, not values
    rs = native.wave_row_image_layout(din, kp)[0]
    ref = _torch_image(X, Y, din, kp)
    for Xs in (X, torch.cat([X, torch.full((n, 3), 7.0, device=dev)], dim=1)[:, :din]):  # contiguous, padded rows
        out = torch.full((n, 4 * rs), -5.0, device=dev)
        native.wave_pack_rows(Xs, Y, din, kp, out)
        torch.cuda.synchronize()
        assert torch.equal(out.view(torch.int32), ref.view(torch.int32))


def _data(din, ns, dev, scale=1.0):
    g = torch.Generator().manual_seed(31)
    X = torch.randn(ns, din, generator=g) * scale
    Y = (torch.rand(ns, 1, generator=g) + 0.125) * scale
    return X.to(dev), Y.to(dev)


def _run(kind, din, B, bias, mom, data, dev, zero_bias=False, launches=LAUNCHES, between=None):
    """One engine, one plan, one launch per entry of ``launches``; the state after every launch.
    ``between``: called with (X, Y) after the launches, followed by a second plan and the launches again."""
    from pytorch_distributed_training_tutorials_amd.data.device_sampler import DeviceDistributedSampler
    from pytorch_distributed_training_tutorials_amd.ops.fused_step import FusedMLPStep

    X, Y = data[0].clone(), data[1].clone()
    ns = X.shape[0]
    torch.manual_seed(3)
    model = torch.nn.Linear(din, 1, bias=bias).to(dev)
    if zero_bias:
        model.bias.data.zero_()
    eng = FusedMLPStep(model, loss=kind, lr=0.05, momentum=mom)
    sampler = DeviceDistributedSampler(ns, 1, 0, seed=4, device=dev)
    cursor = torch.zeros(2, dtype=torch.int32, device=dev)
    losses = torch.zeros(max(launches), device=dev)
    snaps, variants, image_bytes = [], [], []
    for rnd in range(2 if between is not None else 1):
        if rnd == 1:
            between(X, Y)
        plan = eng.persistent_plan(X, Y, B, sampler, cursor, losses, variant="wave_f")
        assert plan.engine.startswith(f"wave:L0R{B // 16}K"), plan.engine
        variants.append(plan.kernel_variant)
        image_bytes.append(plan.image_bytes)
        for n in launches:
            plan.launch(n)
            torch.cuda.synchronize()
            snaps.append({"P": eng.P.clone(), "G": eng.G.clone(), "losses": losses[:n].clone(),
                          "cursor": cursor.tolist(), "mom": None if eng.mom is None else eng.mom.clone()})
    return variants, image_bytes, snaps


def _lean_and_generic(monkeypatch, *args, **kw):
    mom = args[4]
    monkeypatch.delenv("PTDT_WAVE_GENERIC", raising=False)
    variants, image_bytes, lean = _run(*args, **kw)
    assert all(v == ("lean-mom" if mom else "lean-plain") for v in variants), variants
    ns, din = args[5][0].shape
    kp = 4 if din <= 16 else 5
    assert all(b == ns * 16 * ((kp + kp % 2 + 1 + 3) // 4 * 4) for b in image_bytes), image_bytes  # it read the image
    monkeypatch.setenv("PTDT_WAVE_GENERIC", "1")
    variants, image_bytes, gen = _run(*args, **kw)
    assert all(v == "generic" for v in variants) and not any(image_bytes)
    return lean, gen


def _same_bits(lean, gen, keys=("P", "G", "losses", "mom")):
    assert len(lean) == len(gen)
    for k, (a, b) in enumerate(zip(lean, gen)):
        assert a["cursor"] == b["cursor"]
        for key in keys:
            if a[key] is not None:
                assert torch.equal(a[key].view(torch.int32), b[key].view(torch.int32)), (key, k)


@pytest.mark.gpu
@pytest.mark.parametrize("rows", [0, 1])  # N = 96 and 160 rows (B = 64: 192 and 320)
@pytest.mark.parametrize("mom", [0.0, 0.9])
@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("kind", ["mse", "ce_soft"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_image_kernels_match_generic_bitwise(dev, monkeypatch, shape, kind, bias, mom, rows):
    """N = 96 and 160: epochs of 3 and 5 steps at B = 32, of 6 and 10 at B = 16. B = 64 takes N = 192
    and 320 (3 and 5 steps): a lean kernel takes whole batches only, and 96 or 160 rows are no whole
    number of 64-row batches."""
    din, B = SHAPES[shape]
    data = _data(din, (192, 320)[rows] if B == 64 else (96, 160)[rows], dev)
    lean, gen = _lean_and_generic(monkeypatch, kind, din, B, bias, mom, data, dev)
    _same_bits(lean, gen)
    assert all(torch.isfinite(a["P"]).all() and torch.isfinite(a["losses"]).all() for a in lean)
    if kind == "mse":  # one-class soft CE has a gradient of +0; MSE moves the parameters at every launch
        assert all(a["G"].abs().sum().item() > 0 for a in lean)
        assert not torch.equal(lean[0]["P"], lean[-1]["P"])


@pytest.mark.gpu
@pytest.mark.parametrize("scale,zero_bias", [(1e-30, False), (1e-20, True)])
def test_image_kernels_tiny_values(dev, monkeypatch, scale, zero_bias):
    """Inputs and targets scaled by 1e-30; and by 1e-20 with a zero initial bias, where dL/dz is about
    1e-21 and the weight gradients g * x about 1e-41: subnormal (below 1.18e-38), which the packed
    tail's {g * 1, fma(g, 1, s)} and the packed SGD must carry like the scalar forms.

    In the second case the losses themselves are subnormal (about 1e-40), and there the lean kernels'
    loss report -- raw shares scaled by the helper waves, which the row image does not touch -- differs
    from the generic kernel's in the last bit of some steps (measured: the same +-1 on the commit before
    the row image). That case therefore compares parameters and gradients, what the image feeds."""
    data = _data(20, 96, dev, scale=scale)
    lean, gen = _lean_and_generic(monkeypatch, "mse", 20, 32, True, 0.0, data, dev, zero_bias=zero_bias)
    _same_bits(lean, gen, ("P", "G") if zero_bias else ("P", "G", "losses"))
    if zero_bias:
        G = lean[0]["G"]
        assert ((G != 0) & (G.abs() < 1.17549435e-38)).any(), G


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["mse", "ce_soft"])
def test_image_kernels_non_finite_rows(dev, monkeypatch, kind):
    """A NaN and an inf in X, in different rows and feature groups: the image carries their bits, and
    the parameters turn non-finite where the generic kernel's do."""
    X, Y = _data(20, 96, dev)
    X[5, 2] = float("nan")
    X[40, 19] = float("inf")  # the last feature: the packed tail's pair
    lean, gen = _lean_and_generic(monkeypatch, kind, 20, 32, True, 0.0, (X, Y), dev)
    _same_bits(lean, gen)
    assert not torch.isfinite(lean[-1]["P"]).all()


@pytest.mark.gpu
def test_dataset_changed_in_place_gets_a_new_image(dev, monkeypatch):
    """A plan snapshots the dataset when it is created. After X and Y change in place, a new plan of the
    same engine must gather the new values: equal to the generic kernel, which reads X and Y."""
    def change(X, Y):
        X.mul_(-0.5)
        Y.add_(0.25)

    data = _data(20, 96, dev)
    lean, gen = _lean_and_generic(monkeypatch, "mse", 20, 32, True, 0.0, data, dev, launches=[4, 3], between=change)
    _same_bits(lean, gen)
    # and the change mattered: the same launches on the unchanged dataset end elsewhere
    monkeypatch.delenv("PTDT_WAVE_GENERIC", raising=False)
    _, _, same = _run("mse", 20, 32, True, 0.0, data, dev, launches=[4, 3], between=lambda X, Y: None)
    assert torch.equal(same[1]["P"], lean[1]["P"]) and not torch.equal(same[-1]["P"], lean[-1]["P"])


@pytest.mark.gpu
def test_image_above_the_cap_runs_the_generic_kernel(dev, monkeypatch):
    """``PTDT_WAVE_IMAGE_MAX_MB=0``: no image is packed, and the plan of a configuration whose lean kernels
    read nothing but an image takes the generic kernel on X and Y -- the results of a generic plan."""
    data = _data(20, 96, dev)
    monkeypatch.delenv("PTDT_WAVE_GENERIC", raising=False)
    monkeypatch.setenv("PTDT_WAVE_IMAGE_MAX_MB", "0")
    variants, image_bytes, capped = _run("mse", 20, 32, True, 0.0, data, dev)
    assert variants == ["generic"] and image_bytes == [0]
    monkeypatch.delenv("PTDT_WAVE_IMAGE_MAX_MB")
    monkeypatch.setenv("PTDT_WAVE_GENERIC", "1")
    variants, _, gen = _run("mse", 20, 32, True, 0.0, data, dev)
    assert variants == ["generic"]
    _same_bits(capped, gen)
    assert capped[-1]["G"].abs().sum().item() > 0


@pytest.mark.gpu
def test_two_ranks_one_gpu_in_sync_and_equal_to_generic(tmp_path):
    world = 2
    spawn(_wave_image_workers.lean_and_generic_two_ranks, args=(world, free_port(), str(tmp_path)), nprocs=world)
    res = [torch.load(os.path.join(tmp_path, f"r{r}.pt"), weights_only=True) for r in range(world)]
    for r in res:
        assert r["lean_variant"] == "lean-plain" and r["generic_variant"] == "generic"
        assert r["lean_image_bytes"] == 192 * 128 and r["generic_image_bytes"] == 0
        assert torch.equal(r["lean"].view(torch.int32), r["generic"].view(torch.int32))
        assert r["lean_cursor"].tolist() == r["generic_cursor"].tolist() == [11 // 3, 11 % 3]
    n_state = 21 + 21  # parameters and gradient bucket: identical on both ranks (the losses are per rank)
    for k, steps in ((0, 4), (42 + 4, 7)):
        assert torch.equal(res[0]["lean"][k:k + n_state], res[1]["lean"][k:k + n_state])
    assert torch.isfinite(res[0]["lean"]).all()
