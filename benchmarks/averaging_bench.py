#!/usr/bin/env python3
"""Cost of one weight-averaging update over ResNet-50's parameters and buffers.

``ops.AveragedModel.update_parameters`` (EMA, ``use_buffers=False``: 161 fp32 parameters averaged,
106 fp32 buffers and 53 int64 counters copied) on models.resnet.resnet50, with and without the bf16
shadow, and with the sources in one flat span (``FlatParameters``: one launch for the parameters),
against ``torch.optim.swa_utils.AveragedModel(multi_avg_fn=get_ema_multi_avg_fn(d))`` in the same
process. Every timing is a host clock around ``--steps`` updates ending in a device synchronise; the
variants alternate inside each of ``--rounds`` rounds and the median round is reported. The native
variants are also replayed as one captured graph each (torch's update reads ``n_averaged`` on the
host and cannot be captured).

  python benchmarks/averaging_bench.py --steps 200 --rounds 7

Prints one JSON line: microseconds per update, the ratio to torch's, and the achieved GB/s under
the byte model: 12 bytes per averaged fp32 element (read p, read a, write a), 2 more with the
shadow, 8 per copied fp32 buffer element.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DECAY = 0.999


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200, help="updates per timed window")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("averaging_bench needs a GPU: a CPU timing says nothing about the kernels")

    from torch.optim.swa_utils import AveragedModel as TorchAveragedModel
    from torch.optim.swa_utils import get_ema_multi_avg_fn

    from pytorch_distributed_training_tutorials_amd.models.resnet import resnet50
    from pytorch_distributed_training_tutorials_amd.ops import AveragedModel, FlatParameters

    dev = torch.device("cuda", 0)

    def fresh(flat=False):
        torch.manual_seed(0)
        model = resnet50(num_classes=1000).to(dev).to(memory_format=torch.channels_last)
        if flat:
            FlatParameters(list(model.parameters()))
        return model

    models = {k: fresh(flat=k == "native_flat") for k in ("native", "native_shadow", "native_flat", "torch")}
    avgs = {
        "native": AveragedModel(models["native"], decay=DECAY),
        "native_shadow": AveragedModel(models["native_shadow"], decay=DECAY, bf16_shadow=True),
        "native_flat": AveragedModel(models["native_flat"], decay=DECAY),
        "torch": TorchAveragedModel(models["torch"], multi_avg_fn=get_ema_multi_avg_fn(DECAY)),
    }
    fns = {k: (lambda k=k: avgs[k].update_parameters(models[k])) for k in avgs}
    params = sum(p.numel() for p in models["native"].parameters())
    bufs = sum(b.numel() for b in models["native"].buffers() if b.is_floating_point())
    nbytes = {k: (14 if k == "native_shadow" else 12) * params + 8 * bufs for k in avgs}

    def window(fn):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(a.steps):
            fn()
        torch.cuda.synchronize(dev)
        return 1e6 * (time.perf_counter() - t0) / a.steps

    for m in models.values():  # the sources move away from the averages, as in training: the same move for all
        gen = torch.Generator(device=dev).manual_seed(1)
        with torch.no_grad():
            for p in m.parameters():
                p.add_(1e-2 * torch.randn(p.shape, device=dev, generator=gen))
    for fn in fns.values():  # the first update copies; later ones average
        for _ in range(a.warmup):
            fn()
    eager = {k: [] for k in fns}
    for _ in range(a.rounds):
        for k, fn in fns.items():
            eager[k].append(window(fn))

    graphs = {}
    side = torch.cuda.Stream(dev)
    for k, fn in fns.items():
        if k == "torch":
            continue
        g = torch.cuda.CUDAGraph()
        torch.cuda.synchronize(dev)
        with torch.cuda.graph(g, stream=side):
            fn()
        graphs[k] = g
    for g in graphs.values():
        for _ in range(a.warmup):
            g.replay()
    graphed = {k: [] for k in graphs}
    for _ in range(a.rounds):
        for k, g in graphs.items():
            graphed[k].append(window(g.replay))

    med = lambda d: {k: round(statistics.median(v), 2) for k, v in d.items()}  # noqa: E731
    e, g = med(eager), med(graphed)
    rounds = {**{f"eager_{k}": v for k, v in eager.items()}, **{f"graph_{k}": v for k, v in graphed.items()}}
    spread = {k: round((max(v) - min(v)) / statistics.median(v), 3) for k, v in rounds.items()}
    same = all(torch.equal(x, y)
               for x, y in zip(avgs["native"].module.parameters(), avgs["native_flat"].module.parameters()))
    print(json.dumps({
        "metric": "weight-averaging update over the ResNet-50 parameters and buffers", "unit": "us/update",
        "decay": DECAY, "param_tensors": sum(1 for _ in models["native"].parameters()), "param_elements": params,
        "float_buffer_elements": bufs, "steps": a.steps, "rounds": a.rounds, "eager_us": e, "graph_us": g,
        "ratio_to_torch_eager": {**{f"eager_{k}": round(v / e["torch"], 3) for k, v in e.items() if k != "torch"},
                                 **{f"graph_{k}": round(v / e["torch"], 3) for k, v in g.items()}},
        "bytes_per_update": nbytes,
        "eager_GBps": {k: round(nbytes[k] / (1e3 * v), 1) for k, v in e.items()},
        "graph_GBps": {k: round(nbytes[k] / (1e3 * v), 1) for k, v in g.items()},
        "relative_spread": spread, "updates": {k: int(v.n_averaged) for k, v in avgs.items()},
        "last_weight": avgs["native"].last_weight(), "flat_matches_multi": same,
    }), flush=True)


if __name__ == "__main__":
    main()
