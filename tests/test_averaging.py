"""Weight averaging (ops/averaging.py) without a GPU: trajectories and state_dicts against
``torch.optim.swa_utils.AveragedModel``, the weights of the warm-up, wrappers, the Trainer, checkpoints,
``update_bn``, and the check that the per-step bound of tests/_averaging_ref.py is the reference's.

Models are float32 on the CPU unless a test says otherwise, so the eager ATen path is what runs."""
import copy

import numpy as np
import pytest
import torch
from torch.optim.swa_utils import AveragedModel as TorchAveragedModel
from torch.optim.swa_utils import get_ema_multi_avg_fn, update_bn

from pytorch_distributed_training_tutorials_amd.ops import AveragedModel

from . import _averaging_ref as R


def _small(seed=0):
    torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Linear(6, 5), torch.nn.BatchNorm1d(5), torch.nn.Linear(5, 3))


def _perturb(model, gen):
    """What a training step does to the model, as far as averaging can see: new parameters and buffers."""
    with torch.no_grad():
        for p in model.parameters():
            p.add_(0.1 * torch.randn(p.shape, generator=gen))
        for b in model.buffers():
            if b.is_floating_point():
                b.add_(0.05 * torch.rand(b.shape, generator=gen))
            else:
                b.add_(1)


def _assert_within_a_step(got, want, before, model) -> float:
    """Every tensor of ``got`` within BOUND * max(|a|, |p|) of ``want``: a the average before the update
    (``before``), p the model's tensor. Returns the largest share of the bound in use."""
    assert list(got) == list(want)
    worst = 0.0
    for k in got:
        if k == "n_averaged":
            assert torch.equal(got[k], want[k])
            continue
        src = model.state_dict()[k[len("module."):]]
        if not got[k].is_floating_point():  # integer buffers are copies of the model's, whatever use_buffers
            assert torch.equal(got[k], src), k  # says (torch averages them in integer arithmetic)
            continue
        bound = R.step_bound(before[k], src)
        err = (got[k].double() - want[k].double()).abs()
        assert bool((err <= bound).all()), (k, float(err.max()), float(bound.min()))
        worst = max(worst, float((err / bound.clamp_min(1e-300)).max()))
    return worst


def test_exported_from_ops():
    import pytorch_distributed_training_tutorials_amd.ops as ops
    from pytorch_distributed_training_tutorials_amd.ops.averaging import AveragedModel as A

    assert ops.AveragedModel is A


@pytest.mark.parametrize("use_buffers", [False, True])
@pytest.mark.parametrize("kind", ["swa", "ema"])
def test_trajectory_matches_torch(kind, use_buffers):
    """6 updates; after each, every tensor of the averaged module equals torch's within the per-step
    bound applied to the two float32 implementations (each is within it of the float64 step)."""
    model = _small()
    decay = None if kind == "swa" else R.DECAY
    ours = AveragedModel(model, decay=decay, use_buffers=use_buffers)
    theirs = TorchAveragedModel(model, use_buffers=use_buffers,
                                multi_avg_fn=None if kind == "swa" else get_ema_multi_avg_fn(R.DECAY))
    gen = torch.Generator().manual_seed(1)
    worst = 0.0
    for step in range(6):
        _perturb(model, gen)
        before = {k: v.clone() for k, v in theirs.state_dict().items()}
        ours.update_parameters(model)
        theirs.update_parameters(model)
        assert ours.last_weight() == R.ref_weight(step, decay)
        worst = max(worst, _assert_within_a_step(ours.state_dict(), theirs.state_dict(), before, model))
    print(f"{kind}, use_buffers={use_buffers}: worst |ours - torch| / bound over 6 updates = {worst:.3f}")
    assert int(ours.n_averaged) == int(theirs.n_averaged) == 6
    if not use_buffers:  # the buffers are the model's own
        for b, m in zip(ours.module.buffers(), model.buffers()):
            assert torch.equal(b, m)


def test_average_is_a_flat_fp32_buffer_with_the_sources_layout():
    model = torch.nn.Sequential(torch.nn.Conv2d(3, 4, 3), torch.nn.Linear(4, 2)).to(memory_format=torch.channels_last)
    avg = AveragedModel(model)
    ps = list(avg.module.parameters())
    store = {p.untyped_storage().data_ptr() for p in ps}
    assert len(store) == 1
    for p, q in zip(ps, model.parameters()):
        assert p.dtype == torch.float32 and p.shape == q.shape and p.stride() == q.stride()
        assert p.data_ptr() != q.data_ptr()
    assert not ps[0].is_contiguous() and ps[0].is_contiguous(memory_format=torch.channels_last)


@pytest.mark.parametrize("direction", ["ours_to_torch", "torch_to_ours"])
def test_state_dict_interchange_with_torch(direction):
    model = _small(2)
    gen = torch.Generator().manual_seed(3)
    fn = get_ema_multi_avg_fn(R.DECAY)
    a, b = AveragedModel(model, decay=R.DECAY), TorchAveragedModel(model, multi_avg_fn=fn)
    src, dst = (a, b) if direction == "ours_to_torch" else (b, a)
    for _ in range(3):
        _perturb(model, gen)
        src.update_parameters(model)
    sd = copy.deepcopy(src.state_dict())
    assert set(sd) == {"n_averaged"} | {"module." + k for k in model.state_dict()}
    dst.load_state_dict(sd)
    assert int(dst.n_averaged) == 3
    for k, v in dst.state_dict().items():
        assert torch.equal(v, sd[k]), k
    # and the loaded object goes on averaging from there, like the one that saved
    _perturb(model, gen)
    src.update_parameters(model)
    dst.update_parameters(model)
    _assert_within_a_step(dst.state_dict(), src.state_dict(), sd, model)
    assert int(dst.n_averaged) == int(src.n_averaged) == 4


def test_warmup_weights_equal_the_reference():
    model = torch.nn.Linear(2, 2)
    avg = AveragedModel(model, decay=R.DECAY, warmup=True)
    seen = []
    for n in range(13):
        avg.update_parameters(model)
        seen.append(avg.last_weight())
        assert int(avg.n_averaged) == n + 1
    assert seen == [R.ref_weight(n, R.DECAY, True) for n in range(13)]
    # the closed form, spelled out once more: 1, then 1 - (1 + n) / (10 + n) while that is below the decay
    assert seen[0] == 1.0 and seen[1] == float(np.float32(1.0 - 2.0 / 11.0)) and seen[12] == float(np.float32(1 - 13 / 22))
    assert R.ref_weight(10 ** 6, R.DECAY, True) == float(np.float32(1.0 - R.DECAY))
    swa = AveragedModel(model)
    for n in range(4):
        swa.update_parameters(model)
        assert swa.last_weight() == R.ref_weight(n) == float(np.float32(1.0 / (n + 1)))


def test_arguments_are_validated():
    model = torch.nn.Linear(2, 2)
    for bad in (0.0, 1.0, -0.1, 1.5):
        with pytest.raises(ValueError, match="decay"):
            AveragedModel(model, decay=bad)
    with pytest.raises(ValueError, match="warmup"):
        AveragedModel(model, warmup=True)
    with pytest.raises(ValueError, match="parameters and buffers"):
        AveragedModel(model).update_parameters(_small())


def test_bf16_model_keeps_an_fp32_average():
    """With decay 0.999 an average kept in bf16 stops moving; the fp32 master does not, and the module
    holds its rounding."""
    torch.manual_seed(4)
    model = torch.nn.Linear(8, 8).to(torch.bfloat16)
    with torch.no_grad():
        model.weight.fill_(1.0)  # a bf16 ulp of 2^-7 here; the steps below are 0.001 * 0.25
    avg = AveragedModel(model, decay=R.DECAY)
    avg.update_parameters(model)
    start = avg.module.weight.detach().clone()
    master = start.double()
    with torch.no_grad():
        model.weight.add_(0.25)
    w = R.ref_weight(1, R.DECAY)
    for _ in range(200):
        avg.update_parameters(model)
        master = master + w * (model.weight.detach().double() - master)
    assert avg.module.weight.dtype == torch.bfloat16
    assert not torch.equal(avg.module.weight, start)
    torch.testing.assert_close(avg.module.weight.double(), master, rtol=2.0 ** -8, atol=0)
    naive = start.clone()
    naive.lerp_(model.weight.detach(), 1 - R.DECAY)
    assert torch.equal(naive, start)  # the step is below a bf16 ulp: this is why the average is fp32


def test_ddp_wrapper_is_unwrapped(tmp_path):
    import torch.distributed as dist

    assert not dist.is_initialized()
    dist.init_process_group("gloo", init_method=f"file://{tmp_path / 'store'}", rank=0, world_size=1)
    try:
        model = _small(5)
        ddp = torch.nn.parallel.DistributedDataParallel(model)
        avg = AveragedModel(ddp, decay=0.9)
        assert type(avg.module) is type(model)
        assert set(avg.state_dict()) == {"n_averaged"} | {"module." + k for k in model.state_dict()}
        avg.update_parameters(ddp)
        for p, q in zip(avg.module.parameters(), model.parameters()):
            assert torch.equal(p, q)
    finally:
        dist.destroy_process_group()


def _toy_trainer(tmp_path=None, engine="auto", how="callable", **kw):
    from torch.utils.data import DataLoader, TensorDataset

    from pytorch_distributed_training_tutorials_amd.ops.loss import mse_loss
    from pytorch_distributed_training_tutorials_amd.ops.optim import FusedSGD
    from pytorch_distributed_training_tutorials_amd.utils.trainer import Trainer

    gen = torch.Generator().manual_seed(40)
    X, Y = torch.randn(64, 20, generator=gen), 3.0 * torch.randn(64, 1, generator=gen)
    torch.manual_seed(3)
    model = torch.nn.Linear(20, 1)
    loader = DataLoader(TensorDataset(X, Y), batch_size=16)
    make = (lambda m: AveragedModel(m, decay=0.9)) if how == "callable" else AveragedModel(model, decay=0.9)
    t = Trainer(model, loader, FusedSGD(model.parameters(), lr=0.05, momentum=0.9), loss_fn=mse_loss, engine=engine,
                verbose=False, averaged_model=make, **kw)
    return t, model


@pytest.mark.parametrize("how", ["callable", "instance"])
def test_trainer_updates_once_per_step(how):
    t, model = _toy_trainer(how=how)
    assert t.engine_name == "autograd"
    calls = []
    inner = t.averaged_model.update_parameters
    t.averaged_model.update_parameters = lambda m: (calls.append(1), inner(m))[1]
    t.train(2)
    assert len(calls) == 8 == int(t.averaged_model.n_averaged)
    assert t.averaged_model.last_weight() == R.ref_weight(7, 0.9)
    live = model.weight.detach()
    assert t.averaged_model.module.weight.device == live.device
    assert float((t.averaged_model.module.weight.detach() - live).abs().max()) > 1e-4  # an average, not a copy


def test_trainer_refuses_the_fused_engines():
    for engine in ("persistent", "fused"):
        with pytest.raises(ValueError, match="averaged_model"):
            # refused before the communicator is used (as tests/test_lr_schedule.py)
            _toy_trainer(engine=engine, comm=object())


def test_trainer_snapshot_round_trip(tmp_path):
    path = str(tmp_path / "snap.pt")
    t, _ = _toy_trainer(snapshot_path=path, save_every=1)
    t.train(1)
    saved = {k: v.detach().cpu().clone() for k, v in t.averaged_model.state_dict().items()}
    assert int(saved["n_averaged"]) == 4 and "averaged_model" in torch.load(path, weights_only=True)
    t2, _ = _toy_trainer(snapshot_path=path, save_every=1)
    assert t2.epochs_run == 1
    got = t2.averaged_model.state_dict()
    assert list(got) == list(saved)
    for k in saved:
        assert torch.equal(got[k].cpu(), saved[k]), k
    t2.train(2)
    assert int(t2.averaged_model.n_averaged) == 8


def test_checkpoint_round_trip(tmp_path):
    from pytorch_distributed_training_tutorials_amd.utils.checkpoint import load_checkpoint, save_checkpoint

    model = _small(6)
    gen = torch.Generator().manual_seed(7)
    avg = AveragedModel(model, use_buffers=True)
    for _ in range(3):
        _perturb(model, gen)
        avg.update_parameters(model)
    with_avg, without = str(tmp_path / "a.pt"), str(tmp_path / "b.pt")
    save_checkpoint(with_avg, model, epoch=2, averaged_model=avg)
    save_checkpoint(without, model, epoch=2)
    fresh = AveragedModel(_small(8), use_buffers=True)
    state = load_checkpoint(with_avg, _small(8), averaged_model=fresh)
    assert state["epoch"] == 2 and int(fresh.n_averaged) == 3
    for (k, v), w in zip(fresh.state_dict().items(), avg.state_dict().values()):
        assert torch.equal(v, w), k
    untouched = AveragedModel(_small(8), use_buffers=True)
    before = copy.deepcopy(untouched.state_dict())
    load_checkpoint(without, _small(8), averaged_model=untouched)  # a checkpoint written without one loads as before
    for k, v in untouched.state_dict().items():
        assert torch.equal(v, before[k]), k
    # both continue alike
    _perturb(model, gen)
    avg.update_parameters(model)
    fresh.update_parameters(model)
    for (k, v), w in zip(fresh.state_dict().items(), avg.state_dict().values()):
        assert torch.equal(v, w), k


def test_update_bn_runs_on_the_averaged_model():
    """torch's update_bn on an averaged copy of a model with the package's BatchNorm2d: the statistics are
    reset and re-estimated as the cumulative average (momentum=None) of the loader's batches."""
    from pytorch_distributed_training_tutorials_amd.ops.norm import BatchNorm2d

    torch.manual_seed(9)
    model = torch.nn.Sequential(torch.nn.Conv2d(3, 4, 3, padding=1), BatchNorm2d(4))
    avg = AveragedModel(model)
    avg.update_parameters(model)
    gen = torch.Generator().manual_seed(10)
    dev = next(avg.parameters()).device
    batches = [2.0 + torch.randn(8, 3, 6, 6, generator=gen) for _ in range(3)]
    update_bn([(b, None) for b in batches], avg, device=dev)
    bn = avg.module[1]
    assert int(bn.num_batches_tracked) == 3 and bn.momentum == 0.1
    with torch.no_grad():
        ys = [avg.module[0](b.to(dev)) for b in batches]
    mean = torch.stack([y.mean((0, 2, 3)) for y in ys]).mean(0)
    var = torch.stack([y.var((0, 2, 3), unbiased=True) for y in ys]).mean(0)
    torch.testing.assert_close(bn.running_mean, mean, rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(bn.running_var, var, rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("kind", ["swa", "ema", "ema_warmup"])
def test_float32_evaluation_stays_inside_the_bound(kind):
    """The bound is the reference's, not the kernel's: a float32 evaluation of fmaf(w, p - a, a) on
    the GPU tests' inputs (numpy float32; the product and sum are formed in float64 and rounded once,
    which is what a fused multiply-add does up to double rounding) stays inside it."""
    decay = None if kind == "swa" else R.DECAY
    avgs = [t.clone() for t in R.make_tensors(100)]
    worst = 0.0
    for step in range(5):
        w = R.ref_weight(step, decay, kind == "ema_warmup")
        srcs = R.make_tensors(101 + step)
        for i, (a, p) in enumerate(zip(avgs, srcs)):
            if w == 1.0:
                new = p.clone()
            else:
                a32, p32 = a.numpy().astype(np.float32), p.numpy().astype(np.float32)
                d = (p32 - a32).astype(np.float32)
                new = torch.from_numpy((np.float64(np.float32(w)) * d.astype(np.float64)
                                        + a32.astype(np.float64)).astype(np.float32))
            worst = max(worst, R.bound_share(new, a, p, w))
            avgs[i] = new.reshape(a.shape)
    print(f"{kind}: a float32 evaluation uses {100 * worst:.1f}% of the per-step bound")
    assert worst <= 1.0
