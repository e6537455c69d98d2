"""Gradient-norm clipping on the ResNet-50 gradient set: ops.clip.GradClipper (in place and fused
mode) against torch.nn.utils.clip_grad_norm_(foreach=True) in the same process.

The gradients are the 161 tensors / 25,557,032 elements of ResNet-50, laid out as the DDP wrapper's
bucket views at world 1 (float32), and the same layout in bfloat16 buffers. Every repetition starts
from the same standard-normal gradients (restored outside the timed window; max_norm 1.0 clips) and
is timed with device events around the whole call; the three variants alternate inside each of the
``--reps`` rounds and the medians are reported. ``native_fused`` is the norm-only cost (partials +
finalise, the coefficient goes to the optimizer). The eager calls include the host's launch work;
the ``*_graph`` variants replay the same calls from a captured hipGraph, which is how they run inside
``GraphedStep``, and the norm pass's read rate is its bytes over the ``native_fused_graph`` time.

  python benchmarks/gradclip_bench.py [--reps 50] [--warmup 5]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK_TBS = 8.0       # MI355X HBM3E spec peak
HBM_MEASURED_TBS = 6.29  # float4 copy, measured (79 % of spec)


def _bucket_grads(dev, dtype):
    """ResNet-50 parameters whose .grad are back-to-back views of per-bucket flat buffers, in the
    layout of the DDP wrapper's buckets."""
    from pytorch_distributed_training_tutorials_amd.models.resnet import resnet50
    from pytorch_distributed_training_tutorials_amd.parallel import comm as comm_mod
    from pytorch_distributed_training_tutorials_amd.parallel.ddp import DistributedDataParallel

    torch.manual_seed(0)
    model = resnet50(num_classes=1000).to(dev).to(memory_format=torch.channels_last)
    ddp = DistributedDataParallel(model, device_ids=[dev.index], comm=comm_mod.get_default(dev))
    params = list(model.parameters())
    for bucket in ddp.bucket_params():
        views = [ddp.reducer.grad_view(i) for i in bucket]
        if dtype == torch.float32:
            for i, v in zip(bucket, views):
                params[i].grad = v
        else:  # the same order and offsets in a bf16 buffer
            order = sorted(range(len(bucket)), key=lambda k: views[k].data_ptr())
            flat = torch.empty(sum(v.numel() for v in views), dtype=dtype, device=dev)
            off = 0
            for k in order:
                p = params[bucket[k]]
                p.data = p.data.to(dtype)
                p.grad = flat[off:off + p.numel()].as_strided(p.shape, p.stride())
                off += p.numel()
    return ddp, params


def _time(fn, restore, reps, warmup):
    times = []
    for r in range(warmup + reps):
        restore()
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        torch.cuda.synchronize()
        if r >= warmup:
            times.append(t0.elapsed_time(t1) * 1e3)  # us
    return times


def _graphed(fn, dev):
    """``fn`` captured into a hipGraph after one eager call on the capture stream; returns the replay."""
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        fn()
    torch.cuda.current_stream(dev).wait_stream(s)
    torch.cuda.synchronize(dev)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        fn()
    torch.cuda.synchronize(dev)
    return g.replay


def bench(dev, dtype, reps, warmup, max_norm):
    from pytorch_distributed_training_tutorials_amd.ops.clip import GradClipper
    from pytorch_distributed_training_tutorials_amd.ops.optim import FusedSGD

    ddp, params = _bucket_grads(dev, dtype)
    grads = [p.grad for p in params]
    numel = sum(g.numel() for g in grads)
    gen = torch.Generator(device=dev).manual_seed(1)
    master = [torch.randn(g.shape, generator=gen, device=dev, dtype=torch.float32).to(dtype) for g in grads]

    def restore():
        torch._foreach_copy_(grads, master)

    inplace = GradClipper(params, max_norm)
    fused = GradClipper(params, max_norm, optimizer=FusedSGD(params, lr=0.1))
    variants = {
        "native_inplace": inplace,
        "native_fused": fused,
        "torch_foreach": lambda: torch.nn.utils.clip_grad_norm_(params, max_norm, foreach=True),
    }
    restore()
    variants["native_inplace_graph"] = _graphed(inplace, dev)
    variants["native_fused_graph"] = _graphed(fused, dev)
    times = {k: [] for k in variants}
    for k, fn in variants.items():  # warm every variant first
        _time(fn, restore, 0, warmup)
    for _ in range(reps):  # then alternate them
        for k, fn in variants.items():
            times[k] += _time(fn, restore, 1, 0)
    restore()
    ref = float(torch.nn.utils.clip_grad_norm_(params, max_norm, foreach=True))
    restore()
    got = float(inplace())
    med = {k: statistics.median(v) for k, v in times.items()}
    nbytes = numel * grads[0].element_size()
    return {
        "dtype": str(dtype).replace("torch.", ""), "tensors": len(grads), "numel": numel, "spans": inplace.num_spans,
        "max_norm": max_norm, "reps": reps,
        "median_us": {k: round(v, 1) for k, v in med.items()},
        "min_us": {k: round(min(v), 1) for k, v in times.items()},
        "max_us": {k: round(max(v), 1) for k, v in times.items()},
        "norm_pass_bytes": nbytes, "norm_pass_GBs": round(nbytes / med["native_fused_graph"] / 1e3, 1),
        "hbm_peak_TBs": HBM_PEAK_TBS, "hbm_measured_copy_TBs": HBM_MEASURED_TBS,
        "total_norm": got, "total_norm_torch": ref,
    }


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--max_norm", type=float, default=1.0)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("gradclip_bench.py measures on the GPU; none is available")
    from pytorch_distributed_training_tutorials_amd.parallel import env

    env.init_process_group("nccl")
    dev = env.device()
    out = [bench(dev, dt, a.reps, a.warmup, a.max_norm) for dt in (torch.float32, torch.bfloat16)]
    print(json.dumps({"bench": "gradclip", "results": out}), flush=True)
    env.destroy_process_group()


if __name__ == "__main__":
    main()
