"""Cost of a device learning rate on the ResNet-50 parameter set: ``FusedSGD.step()`` with the rate
as a host float against the same step reading it from a bound ``ops.lr_scheduler`` buffer, with and
without the ``scheduler.step()`` launch behind it, and that launch alone.

The parameters are the 161 tensors / 25,557,032 elements of ResNet-50 with their gradients laid out
as the DDP wrapper's bucket views at world 1 (the layout of ``benchmarks/gradclip_bench.py``), updated
by ``FusedSGD(momentum=0.9, weight_decay=1e-4, bf16_shadow=True)`` as in ``benchmarks/resnet_ddp.py``.
Every variant is timed with device events around the whole call; the variants alternate inside each
of the ``--reps`` rounds and the medians are reported. The eager calls include the host's launch
work; the ``*_graph`` variants replay the same calls from a captured hipGraph, which is how they run
inside ``GraphedStep``.

  python benchmarks/lr_schedule_bench.py [--reps 50] [--warmup 5]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def bench(dev, reps, warmup):
    from gradclip_bench import _bucket_grads, _graphed, _time

    from pytorch_distributed_training_tutorials_amd.ops import lr_scheduler as S
    from pytorch_distributed_training_tutorials_amd.ops.optim import FusedSGD

    ddp, params = _bucket_grads(dev, torch.float32)
    gen = torch.Generator(device=dev).manual_seed(1)
    for p in params:
        p.grad.copy_(torch.randn(p.grad.shape, generator=gen, device=dev))
    kw = dict(lr=1e-4, momentum=0.9, weight_decay=1e-4, bf16_shadow=True)
    host = FusedSGD(params, **kw)
    devlr = FusedSGD(params, **kw)
    sched = S.SequentialLR(devlr, [S.LinearLR(devlr, start_factor=0.1, end_factor=1.0, total_iters=5),
                                   S.CosineAnnealingLR(devlr, T_max=1000)], [5])

    def update_and_schedule():
        devlr.step()
        sched.step()

    variants = {"update_host_lr": host.step, "update_device_lr": devlr.step,
                "update_device_lr_and_schedule": update_and_schedule, "schedule_step": sched.step}
    for fn in list(variants.values()):  # state allocation happens in the first calls, before any capture
        fn()
    for k in list(variants):
        variants[k + "_graph"] = _graphed(variants[k], dev)
    times = {k: [] for k in variants}
    nothing = lambda: None  # noqa: E731  (nothing to restore: the update does not write the gradients)
    for fn in variants.values():
        _time(fn, nothing, 0, warmup)
    for _ in range(reps):
        for k, fn in variants.items():
            times[k] += _time(fn, nothing, 1, 0)
    med = {k: statistics.median(v) for k, v in times.items()}
    return {
        "tensors": len(params), "numel": sum(p.numel() for p in params), "reps": reps,
        "median_us": {k: round(v, 1) for k, v in med.items()},
        "min_us": {k: round(min(v), 1) for k, v in times.items()},
        "max_us": {k: round(max(v), 1) for k, v in times.items()},
        "device_lr_minus_host_lr_graph_us": round(med["update_device_lr_graph"] - med["update_host_lr_graph"], 1),
        "schedule_in_step_graph_us": round(med["update_device_lr_and_schedule_graph"] - med["update_host_lr_graph"], 1),
        "scheduler_steps": sched.last_epoch, "last_lr": sched.get_last_lr(),
    }


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("lr_schedule_bench.py measures on the GPU; none is available")
    from pytorch_distributed_training_tutorials_amd.parallel import env

    env.init_process_group("nccl")
    dev = env.device()
    print(json.dumps({"bench": "lr_schedule", **bench(dev, a.reps, a.warmup)}), flush=True)
    env.destroy_process_group()


if __name__ == "__main__":
    main()
