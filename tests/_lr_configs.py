"""The schedule configurations shared by tests/test_lr_schedule.py and tests/test_lr_schedule_gpu.py:
each builds the same schedule from ``ops.lr_scheduler`` and from ``torch.optim.lr_scheduler``.
torch's schedulers, stepped on a throw-away ``torch.optim.SGD``, are the reference."""
import functools

import torch
from torch.optim import lr_scheduler as T

BASES = (0.1, 0.003)  # two parameter groups
STEPS = 40
FP64_SLACK = 1e-12    # |closed form - torch| / base_lr: torch steps some schedules recursively in fp64


def _ours():
    from pytorch_distributed_training_tutorials_amd.ops import lr_scheduler as L

    return L


CONFIGS = {
    # runs past T_max on purpose: the cosine is periodic there, as torch's is
    "warmup_cosine": lambda M, o: M.SequentialLR(
        o, [M.LinearLR(o, start_factor=0.1, end_factor=1.0, total_iters=5), M.CosineAnnealingLR(o, T_max=30)], [5]),
    "step": lambda M, o: M.StepLR(o, 7, 0.1),
    "multistep": lambda M, o: M.MultiStepLR(o, [3, 3, 10, 25], 0.5),
    "exponential": lambda M, o: M.ExponentialLR(o, 0.9),
    "polynomial": lambda M, o: M.PolynomialLR(o, 33, power=2),
    "constant_polynomial": lambda M, o: M.SequentialLR(
        o, [M.ConstantLR(o, factor=0.25, total_iters=4), M.PolynomialLR(o, total_iters=20, power=1)], [6]),
}

# schedules of single tests (not part of the six value configurations)
EXTRA = {
    # the captured DDP loop: linear warm-up 0.1 -> 1 over 4 steps, then cosine with T_max = 6
    "loop_warmup_cosine": lambda M, o: M.SequentialLR(
        o, [M.LinearLR(o, start_factor=0.1, end_factor=1.0, total_iters=4), M.CosineAnnealingLR(o, T_max=6)], [4]),
    # the Trainer: warm-up over 3 steps, then halved every 2 steps
    "trainer_warmup_step": lambda M, o: M.SequentialLR(
        o, [M.LinearLR(o, start_factor=0.1, end_factor=1.0, total_iters=3), M.StepLR(o, 2, 0.5)], [3]),
    # the twin-optimizer comparisons: linear warm-up 0.1 -> 1 over the 6 steps they take
    "warmup6": lambda M, o: M.LinearLR(o, start_factor=0.1, end_factor=1.0, total_iters=6),
}
_ALL = {**CONFIGS, **EXTRA}


def ours(name, optimizer):
    return _ALL[name](_ours(), optimizer)


def torch_sched(name, optimizer):
    return _ALL[name](T, optimizer)


@functools.lru_cache(maxsize=None)
def torch_lrs(name, steps=STEPS, bases=BASES):
    """``[[lr of group g at t] for t in 0..steps]`` from torch's own scheduler (fp64 Python floats).
    Computed once per configuration; the rows are tuples, so no test can change them."""
    import warnings

    opt = torch.optim.SGD([{"params": [torch.zeros(1, requires_grad=True)], "lr": b} for b in bases], lr=1.0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # SequentialLR warns about its own use of the epoch argument
        sched = torch_sched(name, opt)
        rows = [tuple(g["lr"] for g in opt.param_groups)]
        for _ in range(steps):
            opt.step()
            sched.step()
            rows.append(tuple(g["lr"] for g in opt.param_groups))
    return tuple(rows)
