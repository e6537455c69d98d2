#!/usr/bin/env python3
"""ResNet-50's three stride-2 1x1 downsample convolutions + BatchNorm at batch 128 (NHWC bf16): the native
gathered-row kernels (csrc/kernels/conv1x1_s2.hip, PTDT_CONVBN_S2=1) against the composed path (knob 0):

  forward kernel   conv1x1_s2_bn_stats                      vs  MIOpen's strided conv2d
  forward pair     conv1x1_s2_bn_stats + bn_fwd_apply       vs  MIOpen's conv2d + bn_fwd_train
  backward         bn_bwd_reduce + conv1x1_s2_bwd           vs  bn_bwd + aten.convolution_backward (MIOpen)

``torch.backends.cudnn.benchmark`` is on, as in benchmarks/resnet_ddp.py: MIOpen picks its solvers by exhaustive
find during the warm call. Warm, device events, the arms of a row alternated in one process: median of --rounds
(min .. max), us. A verdict compares the arms' whole ranges: wins / loses only where they do not overlap.

``--step`` adds the whole-step A/B: benchmarks/resnet_ddp.py with PTDT_CONVBN_S2=0 vs 1 on top of the caller's
environment, alternated child processes. ``--out`` writes the markdown record (profiles/conv1x1_s2.md).

    python benchmarks/conv1x1_s2_probe.py [--batch 128] [--rounds 5] [--step 2] [--resources FILE] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(56, 256, 512), (28, 512, 1024), (14, 1024, 2048)]  # (H = W, Cin, Cout): layer2, layer3, layer4
ARMS = ("fwd_native", "fwd_miopen", "fwdpair_native", "fwdpair_composed", "bwd_native", "bwd_composed")


def timed(fn, iters=20):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    torch.cuda.synchronize()
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1e3  # us


def shapes_table(batch, rounds):
    from pytorch_distributed_training_tutorials_amd._ext import native

    C = native()
    torch.backends.cudnn.benchmark = True  # MIOpen exhaustive find: the composed arms as the workload runs them
    dev = torch.device("cuda", 0)
    cl = dict(memory_format=torch.channels_last)
    rows = []
    for hw, cin, cout in SHAPES:
        ho = (hw + 1) // 2
        M = batch * ho * ho
        x = torch.randn(batch, cin, hw, hw, device=dev).to(torch.bfloat16).contiguous(**cl)
        w4 = (torch.randn(cout, cin, 1, 1, device=dev) * cin ** -0.5).to(torch.bfloat16)
        w2 = w4.reshape(cout, cin)
        gy = torch.randn(batch, cout, ho, ho, device=dev).to(torch.bfloat16).contiguous(**cl)
        gamma, beta = torch.rand(cout, device=dev) + 0.5, torch.randn(cout, device=dev) * 0.1
        tickets = torch.zeros(C.conv1x1_s2_num_tickets(M, cin, cout), dtype=torch.int32, device=dev)

        def fwd_native():
            return C.conv1x1_s2_bn_stats(x, w2, gamma, beta, None, None, None, 0.1, 1e-5, tickets)

        def fwd_miopen():
            return torch.nn.functional.conv2d(x, w4, stride=2)

        def fwdpair_native():
            y, st = fwd_native()
            return C.bn_fwd_apply(y, st, None, False, False)[0]

        def fwdpair_composed():
            return C.bn_fwd_train(fwd_miopen(), gamma, beta, None, None, None, None, False, 0.1, 1e-5, None, False)[0]

        y, stats = fwd_native()
        ym = fwd_miopen().contiguous(**cl)
        ey = float((y.float() - ym.float()).abs().max() / ym.float().abs().max())

        def bwd_native():
            g, _, _, coef = C.bn_bwd_reduce(gy, y, gamma, stats, False, True, None, None, None, None, None)
            return C.conv1x1_s2_bwd(g, y, x, w2, coef)

        def bwd_composed():
            dy, _, _, _ = C.bn_bwd(gy, y, None, gamma, stats, False, False, True)
            dx, dw, _ = torch.ops.aten.convolution_backward(dy, x, w4, None, [2, 2], [0, 0], [1, 1], False, [0, 0], 1,
                                                            [True, True, False])
            return dx, dw

        (dxn, dwn), (dxc, dwc) = bwd_native(), bwd_composed()
        ex = float((dxn.float() - dxc.float()).abs().max() / dxc.float().abs().max())
        ew = float((dwn.float() - dwc.reshape(cout, cin).float()).abs().max() / dwc.float().abs().max())
        arms = dict(zip(ARMS, (fwd_native, fwd_miopen, fwdpair_native, fwdpair_composed, bwd_native, bwd_composed)))
        t = {k: [] for k in ARMS}
        for _ in range(rounds):
            for k, fn in arms.items():
                t[k].append(timed(fn))
        rec = {"HW": hw, "K": cin, "N": cout, "M_out": M, "y_rel_diff": round(ey, 5), "dx_rel_diff": round(ex, 5),
               "dw_rel_diff": round(ew, 5),
               **{k: [round(statistics.median(v), 1), round(min(v), 1), round(max(v), 1)] for k, v in t.items()}}
        print(json.dumps(rec), flush=True)
        rows.append(rec)
    return rows


def step_ab(runs, steps):
    """ms/step and final loss of the flagship benchmark per PTDT_CONVBN_S2 value; child processes alternated."""
    out = {"0": [], "1": []}
    for _ in range(runs):
        for mode in out:
            p = subprocess.run([sys.executable, os.path.join(ROOT, "benchmarks", "resnet_ddp.py"), "--steps",
                                str(steps), "--warmup", "10"], env=dict(os.environ, PTDT_CONVBN_S2=mode),
                               stdout=subprocess.PIPE, text=True, timeout=420)
            if p.returncode != 0:
                raise RuntimeError(f"resnet_ddp.py failed with PTDT_CONVBN_S2={mode} (exit {p.returncode})")
            rec = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
            out[mode].append((rec["ms_per_step"], rec["final_loss"]))
            print(json.dumps({"PTDT_CONVBN_S2": mode, "ms_per_step": rec["ms_per_step"],
                              "final_loss": rec["final_loss"]}), flush=True)
    return out


def _cell(v):
    return f"{v[0]} ({v[1]} .. {v[2]})"


def _verdict(a, b):
    """a against b, each (median, min, max)."""
    return "wins" if a[2] < b[1] else "loses" if a[1] > b[2] else "ties"


def markdown(rows, ab, batch, resources):
    knobs = " ".join(f"{k}={v}" for k, v in sorted(os.environ.items()) if k.startswith("PTDT_")) or "none set"
    ln = ["# Native stride-2 1x1 conv + BN kernels (PTDT_CONVBN_S2)", "",
          f"Batch {batch}, NHWC bf16, BN without ReLU or residual (the downsample branch); median of alternated rounds "
          "(min .. max), us, device events. `native`: csrc/kernels/conv1x1_s2.hip (+ bn_fwd_apply / bn_bwd_reduce); "
          "the other arm: MIOpen with exhaustive find (+ bn_fwd_train / bn_bwd), the knob-0 path. The verdict is the "
          "native arm's: wins / loses only where the two ranges do not overlap. Relative differences are max-abs "
          "over the other arm's max-abs.", "",
          "| Cin -> Cout | H = W | M' | fwd kernel native | MIOpen | | fwd pair native | composed | | backward native "
          "| composed | | y diff | dX diff | dW diff |",
          "|---|---:|---:|---:|---:|---|---:|---:|---|---:|---:|---|---:|---:|---:|"]
    for r in rows:
        cells = []
        for a, b in zip(ARMS[::2], ARMS[1::2]):
            cells += [_cell(r[a]), _cell(r[b]), _verdict(r[a], r[b])]
        ln.append(f"| {r['K']} -> {r['N']} | {r['HW']} | {r['M_out']} | " + " | ".join(cells) +
                  f" | {r['y_rel_diff']} | {r['dx_rel_diff']} | {r['dw_rel_diff']} |")
    tot = {k: sum(r[k][0] for r in rows) for k in ARMS}
    ln += ["", "Sum over the three shapes (medians): forward pair native {fwdpair_native:.0f} us, composed "
           "{fwdpair_composed:.0f} us; backward native {bwd_native:.0f} us, composed {bwd_composed:.0f} us."
           .format(**tot), ""]
    if ab:
        ln += ["## Whole step: benchmarks/resnet_ddp.py, 1 GPU, PTDT_CONVBN_S2=0 (the parent commit's path) vs 1 "
               f"(alternated runs; other knobs: {knobs})", "",
               "| PTDT_CONVBN_S2 | ms/step per run | median (min .. max) | final loss per run |", "|---|---|---|---|"]
        for mode, v in ab.items():
            ms = [t[0] for t in v]
            ln.append(f"| {mode} | {', '.join(f'{t:.3f}' for t in ms)} | {statistics.median(ms):.3f} "
                      f"({min(ms):.3f} .. {max(ms):.3f}) | {', '.join(f'{t[1]:.4f}' for t in v)} |")
        m0, m1 = ([t[0] for t in ab[k]] for k in ("0", "1"))
        verdict = ("wins: faster outside the two arms' ranges" if max(m1) < min(m0) else
                   "loses: slower outside the two arms' ranges" if min(m1) > max(m0) else
                   "ties: the two arms' ranges overlap")
        ln += ["", f"The whole step with the knob on {verdict}.", ""]
    if resources:
        ln += ["## Compiler resource report (-Rpass-analysis=kernel-resource-usage)", "",
               "Planned residency: 2 workgroups (8 waves) per CU for every kernel (64 KiB of LDS each); the register "
               "counts below allow that, and nothing spills.", "", "```", resources.rstrip(), "```", ""]
    return "\n".join(ln)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--step", type=int, default=0, metavar="RUNS", help="whole-step A/B runs per value (0: none)")
    ap.add_argument("--step_steps", type=int, default=40, help="timed steps of each whole-step run")
    ap.add_argument("--resources", default=None, help="text file with the compiler's resource report to include")
    ap.add_argument("--out", default=None, help="write the markdown tables here")
    a = ap.parse_args()
    if torch.cuda.device_count() < 1:  # a count only: no context here while the children below run
        raise SystemExit("conv1x1_s2_probe: needs a GPU")
    ab = step_ab(a.step, a.step_steps) if a.step > 0 else None
    rows = shapes_table(a.batch, a.rounds)
    res = open(a.resources).read() if a.resources else None
    md = markdown(rows, ab, a.batch, res)
    print(md)
    if a.out:
        with open(a.out, "w") as f:
            f.write(md + "\n")


if __name__ == "__main__":
    main()
