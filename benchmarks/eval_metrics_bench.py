#!/usr/bin/env python3
"""Cost of one evaluation-meter update against the torch composition it replaces.

``ops.ClassificationMeter(topk=(1, 5)).update(logits, target)`` (csrc/kernels/eval_metrics.hip: one
pass over the logits + one accumulate launch, no host read) at ``[256, 1000]`` and ``[1024, 1000]``
bf16 and at ``[64, 32000]`` fp32, against

    loss_sum = F.cross_entropy(logits, target, reduction="sum")
    top = logits.topk(5).indices.eq(target[:, None])
    top1, top5 = top[:, 0].sum(), top.sum()

(no ``.item()``, and no accumulation into running totals, which the meter does do) in the same
process. Every timing is a host clock around ``--steps`` updates ending in a device synchronise; the
two variants alternate inside each of ``--rounds`` rounds, after ``--warmup`` updates of each at
every shape, and the median and the minimum round are reported. The native update is also replayed as a captured graph.
Logits are randn-scale random data, the same tensors for both variants.

  python benchmarks/eval_metrics_bench.py --steps 500 --rounds 9

Prints one JSON line: microseconds per update per shape and variant, the ratio native / torch, the
achieved GB/s of the native update under the byte model "every logit read once" (B C elsize), and,
after one update, each variant's loss-sum error against float64 and both variants' top-k counts.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = ((256, 1000, "bf16"), (1024, 1000, "bf16"), (64, 32000, "fp32"))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=500, help="updates per timed window")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("eval_metrics_bench needs a GPU: a CPU timing says nothing about the kernels")

    from pytorch_distributed_training_tutorials_amd.ops import ClassificationMeter

    dev = torch.device("cuda", 0)

    def window(fn):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(a.steps):
            fn()
        torch.cuda.synchronize(dev)
        return 1e6 * (time.perf_counter() - t0) / a.steps

    out = {}
    for B, C, dt in SHAPES:
        dtype = torch.bfloat16 if dt == "bf16" else torch.float32
        gen = torch.Generator(device=dev).manual_seed(B + C)
        z = torch.randn(B, C, device=dev, generator=gen).to(dtype)
        y = torch.randint(0, C, (B,), device=dev, generator=gen)
        meter = ClassificationMeter(topk=(1, 5), device=dev)
        acc = {}  # the composition's results of the last update

        def native_update():
            meter.update(z, y)

        def torch_update():
            acc["loss"] = F.cross_entropy(z, y, reduction="sum")
            top = z.topk(5).indices.eq(y[:, None])
            acc["top1"] = top[:, 0].sum()
            acc["top5"] = top.sum()

        # one update each: the variants count the same rows (torch.topk breaks ties its own way: the top-5
        # counts may differ by the tied rows, top-1 only when the maximum is tied with the target)
        native_update()
        torch_update()
        torch.cuda.synchronize(dev)
        ref = F.cross_entropy(z.double(), y, reduction="sum").item()
        agree = {"native_loss_rel_err": abs(meter.loss_sum.item() - ref) / ref,
                 "torch_loss_rel_err": abs(acc["loss"].item() - ref) / ref,
                 "top1": (int(meter.counters[5]), int(acc["top1"])), "top5": (int(meter.counters[6]), int(acc["top5"]))}

        fns = {"native": native_update, "torch": torch_update}
        for fn in fns.values():
            for _ in range(a.warmup):
                fn()
        times = {k: [] for k in fns}
        for _ in range(a.rounds):
            for k, fn in fns.items():
                times[k].append(window(fn))

        graph = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream(dev)
        torch.cuda.synchronize(dev)
        with torch.cuda.graph(graph, stream=side):
            native_update()
        for _ in range(a.warmup):
            graph.replay()
        times["native_graph"] = []
        for _ in range(a.rounds):
            times["native_graph"].append(window(graph.replay))

        med = {k: statistics.median(v) for k, v in times.items()}
        nbytes = B * C * z.element_size()
        out[f"{B}x{C}_{dt}"] = {
            "us_median": {k: round(v, 2) for k, v in med.items()},
            "us_min": {k: round(min(v), 2) for k, v in times.items()},
            "relative_spread": {k: round((max(v) - min(v)) / med[k], 3) for k, v in times.items()},
            "native_over_torch": round(med["native"] / med["torch"], 3),
            "native_graph_over_torch": round(med["native_graph"] / med["torch"], 3),
            "native_GBps": round(nbytes / (1e3 * med["native"]), 1),
            "native_graph_GBps": round(nbytes / (1e3 * med["native_graph"]), 1),
            "logit_bytes": nbytes, "agreement_after_one_update": agree,
        }
    print(json.dumps({"metric": "evaluation-meter update (loss sum + top-1 / top-5 counts)", "unit": "us/update",
                      "steps": a.steps, "rounds": a.rounds, "warmup": a.warmup, "shapes": out}), flush=True)


if __name__ == "__main__":
    main()
