#!/usr/bin/env python3
"""Backward of ``ReLU(BN(conv1x1(x)))`` for ResNet-50's layer2-4 stride-1 1x1 convolutions, the eight
(Cin, Cout) the streaming fused backward has no instance for, at batch 128 (NHWC bf16):

  tiled   bn_bwd_reduce (g, coefficients) + conv1x1_bwd_tiled (csrc/kernels/conv1x1_bwd_tiled.hip:
          dY formed inside the data- and weight-gradient kernels, fixed-order merge)
  parent  bn_bwd (reduce + apply, writes dY) + aten.convolution_backward (MIOpen): PTDT_CONVBN_BWD=1

``torch.backends.cudnn.benchmark`` is on, as in benchmarks/resnet_ddp.py: MIOpen picks its backward
solvers by exhaustive find (during the warm call), which is what the parent path runs in the workload.

Warm, device events, the two alternated in one process (median of --rounds). Bytes are what each
path has to move, from the shapes: activations [M, C] bf16, dY written and re-read twice by the parent,
g and y read by each of the tiled path's two products, its fp32 partials written and merged.

``--step`` adds the whole-step A/B: benchmarks/resnet_ddp.py with PTDT_CONVBN_BWD=1 vs all, alternated
child processes. ``--out`` writes the markdown record (profiles/conv1x1_bwd_tiled.md).

    python benchmarks/conv1x1_bwd_probe.py [--batch 128] [--rounds 5] [--step 3] [--out FILE]
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

# (H=W, Cin, Cout, count per step): benchmarks/conv1x1_probe.py's table without the streaming instances
SHAPES = [(28, 128, 512, 4), (28, 512, 128, 3), (28, 512, 256, 1), (14, 256, 1024, 6), (14, 1024, 256, 5),
          (14, 1024, 512, 1), (7, 512, 2048, 3), (7, 2048, 512, 2)]


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


def traffic(M, K, N, splits):
    """Bytes each path needs (bf16 activations; no cache reuse counted)."""
    act_n, act_k, wt = 2 * M * N, 2 * M * K, 2 * N * K
    reduce_pass = 2 * act_n  # dy and y in
    tiled = (reduce_pass + act_n) + (2 * act_n + wt + act_k) + (2 * act_n + act_k + 4 * N * K * splits) + (
        4 * N * K * splits + wt)
    parent = (reduce_pass + 3 * act_n) + (act_n + wt + act_k) + (act_n + act_k + wt)
    return tiled, parent


def shapes_table(batch, rounds):
    from pytorch_distributed_training_tutorials_amd._ext import native

    C = native()
    torch.backends.cudnn.benchmark = True  # MIOpen exhaustive find: the parent arm as the workload runs it
    dev = torch.device("cuda", 0)
    rows = []
    for hw, cin, cout, cnt in SHAPES:
        M = batch * hw * hw
        cl = dict(memory_format=torch.channels_last)
        x4 = torch.randn(batch, cin, hw, hw, device=dev).to(torch.bfloat16).contiguous(**cl)
        w4 = (torch.randn(cout, cin, 1, 1, device=dev) * cin ** -0.5).to(torch.bfloat16)
        y4 = torch.nn.functional.conv2d(x4, w4).contiguous(**cl)
        dy4 = torch.randn(batch, cout, hw, hw, device=dev).to(torch.bfloat16).contiguous(**cl)
        gamma = torch.rand(cout, device=dev) + 0.5
        beta = torch.randn(cout, device=dev) * 0.1
        _, stats, _ = C.bn_fwd_train(y4, gamma, beta, None, None, None, None, True, 0.1, 1e-5)
        x2 = x4.permute(0, 2, 3, 1).reshape(M, cin)
        y2 = y4.permute(0, 2, 3, 1).reshape(M, cout)
        w2 = w4.reshape(cout, cin)

        def tiled():
            g, _, _, coef = C.bn_bwd_reduce(dy4, y4, gamma, stats, True, True, None, None, None, None, None)
            return C.conv1x1_bwd_tiled(g.permute(0, 2, 3, 1).reshape(M, cout), y2, x2, w2, coef)

        def parent():
            dy, _, _, _ = C.bn_bwd(dy4, y4, None, gamma, stats, True, False, True)
            dx, dw, _ = torch.ops.aten.convolution_backward(dy, x4, w4, None, [1, 1], [0, 0], [1, 1], False, [0, 0],
                                                            1, [True, True, False])
            return dx, dw

        (dxt, dwt), (dxp, dwp) = tiled(), parent()
        dxp2 = dxp.permute(0, 2, 3, 1).reshape(M, cin).float()
        ex = float((dxt.float() - dxp2).abs().max() / dxp2.abs().max())
        ew = float((dwt.float() - dwp.reshape(cout, cin).float()).abs().max() / dwp.float().abs().max())
        tt, tp = [], []
        for _ in range(rounds):
            tt.append(timed(tiled))
            tp.append(timed(parent))
        bt, bp = traffic(M, cin, cout, C.conv1x1_bwd_tiled_splits(M, cin, cout))
        rec = {"K": cin, "N": cout, "M": M, "per_step": cnt, "tiled_us": round(statistics.median(tt), 1),
               "parent_us": round(statistics.median(tp), 1), "tiled_us_spread": [round(min(tt), 1), round(max(tt), 1)],
               "parent_us_spread": [round(min(tp), 1), round(max(tp), 1)], "tiled_MB": round(bt / 1e6, 1),
               "parent_MB": round(bp / 1e6, 1), "dx_rel_diff": round(ex, 5), "dw_rel_diff": round(ew, 5)}
        print(json.dumps(rec), flush=True)
        rows.append(rec)
    return rows


def step_ab(runs, steps):
    """ms/step of the flagship benchmark per PTDT_CONVBN_BWD value, child processes alternated."""
    out = {"1": [], "all": []}
    for _ in range(runs):
        for mode in out:
            env = dict(os.environ, PTDT_CONVBN_BWD=mode)
            p = subprocess.run([sys.executable, os.path.join(ROOT, "benchmarks", "resnet_ddp.py"), "--steps",
                                str(steps), "--warmup", "10"], env=env, stdout=subprocess.PIPE, text=True, timeout=600)
            if p.returncode != 0:
                raise RuntimeError(f"resnet_ddp.py failed with PTDT_CONVBN_BWD={mode} (exit {p.returncode})")
            rec = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
            out[mode].append(rec["ms_per_step"])
            print(json.dumps({"PTDT_CONVBN_BWD": mode, "ms_per_step": rec["ms_per_step"]}), flush=True)
    return out


def markdown(rows, ab, batch):
    ln = ["## Per shape: linked backward (bn_bwd_reduce + conv1x1_bwd_tiled) vs the parent path (bn_bwd + "
          "convolution_backward)", "",
          f"Batch {batch}, NHWC bf16, ReLU BN without residual; median of alternated rounds (min .. max), us. MB: the "
          "bytes each path needs from the shapes (tiled: with its fp32 partials, written and merged). Relative "
          "differences are max-abs over the parent's max-abs.", "",
          "| (K, N) | M | per step | tiled us | parent us | tiled / parent | tiled MB | parent MB | dX diff | dW diff |",
          "|---|---:|---:|---:|---:|---:|---:|---:|---:|---:|"]
    tot_t = tot_p = 0.0
    for r in rows:
        tot_t += r["per_step"] * r["tiled_us"]
        tot_p += r["per_step"] * r["parent_us"]
        ln.append(f"| ({r['K']}, {r['N']}) | {r['M']} | {r['per_step']} | {r['tiled_us']} ({r['tiled_us_spread'][0]} .. "
                  f"{r['tiled_us_spread'][1]}) | {r['parent_us']} ({r['parent_us_spread'][0]} .. "
                  f"{r['parent_us_spread'][1]}) | {r['tiled_us'] / r['parent_us']:.2f} | {r['tiled_MB']} | "
                  f"{r['parent_MB']} | {r['dx_rel_diff']} | {r['dw_rel_diff']} |")
    ln += ["", f"Sum over a step's 25 convolutions: tiled {tot_t:.0f} us, parent {tot_p:.0f} us.", ""]
    lose = [f"{r['K']}x{r['N']}" for r in rows if r["tiled_us"] > r["parent_us"]]
    ln += ["Shapes where tiled loses: " + (", ".join(lose) + f" (`PTDT_CONVBN_BWD_SKIP={','.join(lose)}`)."
                                           if lose else "none."), ""]
    if ab:
        ln += ["## Whole step: benchmarks/resnet_ddp.py, 1 GPU, PTDT_CONVBN_BWD=1 vs all (alternated runs)", "",
               "| PTDT_CONVBN_BWD | ms/step per run | median | spread |", "|---|---|---:|---:|"]
        for mode, v in ab.items():
            ln.append(f"| {mode} | {', '.join(f'{t:.3f}' for t in v)} | {statistics.median(v):.3f} | "
                      f"{max(v) - min(v):.3f} |")
        ln.append("")
    return "\n".join(ln)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--step", type=int, default=0, metavar="RUNS", help="whole-step A/B runs per value (0: none)")
    ap.add_argument("--step_steps", type=int, default=40, help="timed steps of each whole-step run")
    ap.add_argument("--out", default=None, help="write the markdown tables here")
    a = ap.parse_args()
    if torch.cuda.device_count() < 1:  # a count only: no context here while the children below run
        raise SystemExit("conv1x1_bwd_probe: needs a GPU")
    ab = step_ab(a.step, a.step_steps) if a.step > 0 else None
    rows = shapes_table(a.batch, a.rounds)
    md = markdown(rows, ab, a.batch)
    print(md)
    if a.out:
        with open(a.out, "w") as f:
            f.write(md + "\n")


if __name__ == "__main__":
    main()
