"""The lean kernels' loss ring counted from the epoch list, and the hand-placed step in the checked
group of the four hand-step kernels (csrc/kernels/linear_wave_impl.h, wave_loop_schedule.h).

The scheme is tests/test_wave_gather_depth_gpu.py's, with its shapes: the generic kernel
(``PTDT_WAVE_GENERIC=1``, read when a plan is built) keeps the ring from the launch start and the
per-step loop and is the oracle; parameters, gradient bucket, momentum, losses and cursor are compared
bitwise after every launch of one plan, and ``plan.kernel_variant`` is asserted, so no case passes by
running generic twice. The dataset is B S rows. S = 1..6 holds the S < depth fallback (the ring from
the launch start) and the ring from the list; ``("mse", 16, 1, 32)`` is a kernel with the compiler's
step in every body that takes the new ring all the same. The launch lengths hold one longer than two
rings of 3 S slots. The split case runs the same steps as several ``launch_at`` calls from j0 != 0: a
first slot other than 0, a ring end inside a launch and a launch that begins in a checked group.

A barrier mismatch between the trainer and the helper waves shows as a hang: run this file under a
time limit, and read wave_loop_schedule.h (tests/test_wave_ring_origin.py) before running it again."""
import pytest
import torch

D = 4  # wave_gather_depth of the deepened kernels
SS = list(range(1, 7))
# (loss, Din, Dout, B)
SHAPES = {
    "mse20x1_b32": ("mse", 20, 1, 32),          # hand-step kernel <2,5,1>
    "mse17x1_b32": ("mse", 17, 1, 32),          # the same kernel, a padded feature group
    "ce_soft20x1_b32": ("ce_soft", 20, 1, 32),  # the benchmark's kernel: zero gradient by construction, bits only
    "mse16x1_b32": ("mse", 16, 1, 32),          # <2,4,1>: the compiler's step in every body, the new ring
    "mse20x1_b64": ("mse", 20, 1, 64),          # <4,5,1>: one group body, depth 3 (ring from the list at S >= 3)
}


def _launches(S):
    return list(range(1, D + 2)) + [S, S + 1, 3 * S + 2, 2 * (3 * S) + 1]


def _data(ns, din, dout, dev):
    g = torch.Generator().manual_seed(11)
    X = torch.randn(ns, din, generator=g)
    Y = torch.rand(ns, dout, generator=g)
    return X.to(dev), Y.to(dev)


def _run(kind, din, dout, B, ns, mom, launches, dev, pos0=None):
    """One plan, one launch per entry of ``launches``; the state after every launch. pos0: the launches
    are launch_at calls, the first from that position (the cursor is set to it first)."""
    from pytorch_distributed_training_tutorials_amd.data.device_sampler import DeviceDistributedSampler
    from pytorch_distributed_training_tutorials_amd.ops.fused_step import FusedMLPStep

    X, Y = _data(ns, din, dout, dev)
    torch.manual_seed(7)
    eng = FusedMLPStep(torch.nn.Linear(din, dout).to(dev), loss=kind, lr=0.05, momentum=mom)
    sampler = DeviceDistributedSampler(ns, 1, 0, seed=2, device=dev)
    S = ns // B
    pos = 0 if pos0 is None else pos0
    cursor = torch.tensor([pos // S, pos % S], dtype=torch.int32, device=dev)
    losses = torch.zeros(max(launches), device=dev)
    plan = eng.persistent_plan(X, Y, B, sampler, cursor, losses, variant="wave_f")
    assert plan.engine.startswith(f"wave:L0R{B // 16}"), plan.engine
    snaps = []
    for n in launches:
        if pos0 is None:
            plan.launch(n)
        else:
            plan.launch_at(n, pos)
        pos += n
        torch.cuda.synchronize()
        snaps.append({"P": eng.P.clone(), "G": eng.G.clone(), "losses": losses[:n].clone(),
                      "cursor": cursor.clone(), "mom": None if eng.mom is None else eng.mom.clone()})
    return plan.kernel_variant, snaps


def _compare(kind, S, mom, launches, lean, gen, pos=0):
    for n, a, b in zip(launches, lean, gen):
        pos += n
        assert a["cursor"].tolist() == [pos // S, pos % S] == b["cursor"].tolist()
        if kind == "mse":
            assert torch.isfinite(a["losses"]).all() and a["G"].abs().sum().item() > 0  # a real gradient
        for key in ("P", "G", "losses"):
            assert torch.equal(a[key].view(torch.int32), b[key].view(torch.int32)), (key, n)
        if mom:
            assert torch.equal(a["mom"].view(torch.int32), b["mom"].view(torch.int32)), ("mom", n)


@pytest.mark.gpu
@pytest.mark.parametrize("mom", [0.0, 0.9])
@pytest.mark.parametrize("S", SS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_checked_hand_step_and_list_ring_match_generic_bitwise(dev, monkeypatch, shape, S, mom):
    kind, din, dout, B = SHAPES[shape]
    launches = _launches(S)
    args = (kind, din, dout, B, B * S, mom, launches, dev)
    monkeypatch.delenv("PTDT_WAVE_GENERIC", raising=False)
    var, lean = _run(*args)
    assert var == ("lean-mom" if mom else "lean-plain")
    monkeypatch.setenv("PTDT_WAVE_GENERIC", "1")
    var, gen = _run(*args)
    assert var == "generic"
    _compare(kind, S, mom, launches, lean, gen)


@pytest.mark.gpu
@pytest.mark.parametrize("mom", [0.0, 0.9])
@pytest.mark.parametrize("shape", ["mse20x1_b32", "mse16x1_b32"])
def test_split_launches_from_inside_an_epoch(dev, monkeypatch, shape, mom):
    """S = 6, from position 9 (e0 = 1, j0 = 3): launch_at calls of 1 step (the next launch begins at
    j0 = 4, with its first list switch in the prologue's reads), 2 steps (then j0 = 0, and the group
    behind the prologue is a checked one), 29 steps (a ring end inside: 18 slots from slot j0 + 4),
    a whole ring and three steps."""
    kind, din, dout, B = SHAPES[shape]
    S, pos0, launches = 6, 9, [1, 2, 29, 18, 3]
    args = (kind, din, dout, B, B * S, mom, launches, dev, pos0)
    monkeypatch.delenv("PTDT_WAVE_GENERIC", raising=False)
    var, lean = _run(*args)
    assert var == ("lean-mom" if mom else "lean-plain")
    monkeypatch.setenv("PTDT_WAVE_GENERIC", "1")
    var, gen = _run(*args)
    assert var == "generic"
    _compare(kind, S, mom, launches, lean, gen, pos0)
