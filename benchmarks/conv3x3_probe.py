#!/usr/bin/env python3
"""``conv2 -> bn2 -> ReLU`` for ResNet-50's four stride-1 3x3 shapes at batch 128 (NHWC bf16): the native implicit
GEMM with the BN statistics in its epilogue (csrc/kernels/conv3x3_bn.hip, PTDT_CONV3X3) against MIOpen.

  pair    fused     conv3x3_bn_stats + bn_fwd_apply
          composed  conv2d (MIOpen, cudnn.benchmark = True) + bn_fwd_train (statistics + apply)
  kernel  native    conv3x3_bn_stats alone            (achieved FLOP/s from 2 M 9 Cin Cout)
          miopen    conv2d alone

Warm, device events, the arms alternated in one process (median of --rounds, min .. max). ``--step`` adds the
whole-step A/B: benchmarks/resnet_ddp.py with PTDT_CONV3X3=0 vs auto, alternated child processes, each under its
own time limit. ``--resources FILE`` appends the compiler's resource report
(-Rpass-analysis=kernel-resource-usage output of csrc/kernels/conv3x3_bn.hip). ``--out`` writes the markdown
record (profiles/conv3x3_bn.md).

    python benchmarks/conv3x3_probe.py [--batch 128] [--rounds 5] [--step 3] [--resources FILE] [--out FILE]
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

# (H = W, Cin = Cout, convolutions per step)
SHAPES = [(56, 64, 3), (28, 128, 3), (14, 256, 5), (7, 512, 2)]
ARMS = ("pair_fused", "pair_composed", "kernel_native", "kernel_miopen")


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
    torch.backends.cudnn.benchmark = True  # MIOpen exhaustive find, as benchmarks/resnet_ddp.py runs it
    dev = torch.device("cuda", 0)
    cl = dict(memory_format=torch.channels_last)
    rows = []
    for hw, ch, cnt in SHAPES:
        M = batch * hw * hw
        x = torch.randn(batch, ch, hw, hw, device=dev).to(torch.bfloat16).contiguous(**cl)
        w = (torch.randn(ch, ch, 3, 3, device=dev) * (9 * ch) ** -0.5).to(torch.bfloat16).contiguous(**cl)
        tk = torch.zeros(C.conv3x3_bn_num_tickets(M, ch, ch), dtype=torch.int32, device=dev)

        def native_():
            return C.conv3x3_bn_stats(x, w, None, None, None, None, None, 0.1, 1e-5, tk)

        def miopen():
            return torch.nn.functional.conv2d(x, w, padding=1)

        def fused():
            y, st = native_()
            return C.bn_fwd_apply(y, st, None, True, False)

        def composed():
            return C.bn_fwd_train(miopen(), None, None, None, None, None, None, True, 0.1, 1e-5, None, False)

        yn, ym = native_()[0].float(), miopen().float()
        arms = dict(zip(ARMS, (fused, composed, native_, miopen)))
        t = {k: [] for k in arms}
        for _ in range(rounds):
            for k, fn in arms.items():
                t[k].append(timed(fn))
        rec = {"C": ch, "HW": hw, "M": M, "per_step": cnt,
               "y_rel_diff": round(float((yn - ym).abs().max() / ym.abs().max()), 5)}
        for k, v in t.items():
            rec[k] = [round(statistics.median(v), 1), round(min(v), 1), round(max(v), 1)]
        rec["native_TFLOPs"] = round(2.0 * M * 9 * ch * ch / rec["kernel_native"][0] / 1e6, 1)
        rec["miopen_TFLOPs"] = round(2.0 * M * 9 * ch * ch / rec["kernel_miopen"][0] / 1e6, 1)
        print(json.dumps(rec), flush=True)
        rows.append(rec)
    return rows


def step_ab(runs, steps):
    """ms/step of the flagship benchmark per PTDT_CONV3X3 value and the shapes auto kept on the native kernel;
    child processes alternated."""
    out = {"0": [], "auto": []}
    picked = {}
    for _ in range(runs):
        for mode in out:
            p = subprocess.run([sys.executable, os.path.join(ROOT, "benchmarks", "resnet_ddp.py"), "--steps",
                                str(steps), "--warmup", "10"], env=dict(os.environ, PTDT_CONV3X3=mode),
                               stdout=subprocess.PIPE, text=True, timeout=420)
            if p.returncode != 0:
                raise RuntimeError(f"resnet_ddp.py failed with PTDT_CONV3X3={mode} (exit {p.returncode})")
            rec = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
            out[mode].append((rec["ms_per_step"], rec["final_loss"]))
            if mode == "auto":
                picked = rec.get("kernel_choices", {}).get("conv3x3bn", picked)
            print(json.dumps({"PTDT_CONV3X3": mode, "ms_per_step": rec["ms_per_step"],
                              "final_loss": rec["final_loss"]}), flush=True)
    return out, picked


def _cell(v):
    return f"{v[0]} ({v[1]} .. {v[2]})"


def _verdict(a, b):
    """a against b, each (median, min, max): outside the measured spread or a tie."""
    return "wins" if a[2] < b[1] else "loses" if a[1] > b[2] else "ties"


def markdown(rows, ab, batch, resources):
    ln = ["# Native 3x3 conv + BN statistics (PTDT_CONV3X3)", "",
          f"Batch {batch}, NHWC bf16, stride 1, padding 1; median of alternated rounds (min .. max), us, device "
          "events. `fused`: conv3x3_bn_stats + bn_fwd_apply; `composed`: MIOpen conv2d + bn_fwd_train. The verdict "
          "compares the arms' whole ranges: wins / loses only where they do not overlap.", "",
          "| Cin = Cout | H = W | M | per step | fused | composed | pair | native kernel | MIOpen conv | kernel | "
          "native TFLOP/s | MIOpen TFLOP/s | Y diff |", "|---|---:|---:|---:|---:|---:|---|---:|---:|---|---:|---:|---:|"]
    for r in rows:
        ln.append(f"| {r['C']} | {r['HW']} | {r['M']} | {r['per_step']} | {_cell(r['pair_fused'])} | "
                  f"{_cell(r['pair_composed'])} | {_verdict(r['pair_fused'], r['pair_composed'])} | "
                  f"{_cell(r['kernel_native'])} | {_cell(r['kernel_miopen'])} | "
                  f"{_verdict(r['kernel_native'], r['kernel_miopen'])} | {r['native_TFLOPs']} | {r['miopen_TFLOPs']} | "
                  f"{r['y_rel_diff']} |")
    tot = {k: sum(r["per_step"] * r[k][0] for r in rows) for k in ARMS}
    ln += ["", "Sum over a step's 13 stride-1 3x3 convolutions (medians): fused pair {pair_fused:.0f} us, composed "
           "pair {pair_composed:.0f} us; native kernel {kernel_native:.0f} us, MIOpen {kernel_miopen:.0f} us."
           .format(**tot), ""]
    if ab:
        out, picked = ab
        ln += ["## Whole step: benchmarks/resnet_ddp.py, 1 GPU, PTDT_CONV3X3=0 (the parent commit's path) vs auto "
               "(alternated runs)", "", "| PTDT_CONV3X3 | ms/step per run | median | spread | final loss per run |",
               "|---|---|---:|---:|---|"]
        for mode, v in out.items():
            ms = [t[0] for t in v]
            ln.append(f"| {mode} | {', '.join(f'{t:.3f}' for t in ms)} | {statistics.median(ms):.3f} | "
                      f"{max(ms) - min(ms):.3f} | {', '.join(f'{t[1]:.4f}' for t in v)} |")
        m0, m1 = ([t[0] for t in out[k]] for k in ("0", "auto"))
        verdict = ("improves outside the spread" if max(m1) < min(m0) else
                   "is slower outside the spread" if min(m1) > max(m0) else "does not change outside the spread")
        ln += ["", f"The whole step {verdict} of the two arms. `auto`'s choices in its last run (N,H,W,Cin,Cout): " +
               (", ".join(f"{k} {v}" for k, v in sorted(picked.items())) or "none recorded") + ".", ""]
    if resources:
        ln += ["## Compiler resource report (-Rpass-analysis=kernel-resource-usage)", "",
               "Planned residency: 2 workgroups (8 waves) per CU for the 128-wide tile (64 KiB of LDS each), 3 for "
               "the 64-wide (48 KiB); the register counts below allow at least that, and nothing spills.", "", "```",
               resources.rstrip(), "```", ""]
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
        raise SystemExit("conv3x3_probe: needs a GPU")
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
