#!/usr/bin/env python3
"""``conv2 -> bn2 -> ReLU -> conv3 -> bn3`` from conv2's output on, for ResNet-50's four conv3 shapes at batch
128 (NHWC bf16): the input BatchNorm applied inside the 1x1 convolution (PTDT_CONVBN_PRE=1) against the paths
it replaces.

  forward   pre     bn_fwd_stats + conv1x1_pre_bn_stats (csrc/kernels/conv1x1_pre.hip)
            fused   bn_fwd_train (statistics + apply, writes a) + conv1x1_bn_stats (streaming / tiled GEMM)
            miopen  bn_fwd_train + conv2d (MIOpen) + bn_fwd_train's statistics pass of the output
  backward  pre     conv1x1_bwd_tiled(pre=) + bn_bwd of bn2
            parent  the linked backward the shape has at PTDT_CONVBN_BWD=all (streaming conv1x1_bwd for
                    64 -> 256, else conv1x1_bwd_tiled) on the saved a + bn_bwd of bn2
  (bn3's apply and reduce passes are the same on every path and are left out.)

Warm, device events, the arms alternated in one process (median of --rounds, min .. max). ``--step`` adds the
whole-step A/B: benchmarks/resnet_ddp.py at PTDT_CONVBN_BWD=all with PTDT_CONVBN_PRE=0 vs 1, alternated child
processes, ms/step and peak allocated memory. ``--resources FILE`` appends the compiler's resource report
(-Rpass-analysis=kernel-resource-usage output of the new and touched units). ``--out`` writes the markdown
record (profiles/conv1x1_pre.md).

    python benchmarks/conv1x1_pre_probe.py [--batch 128] [--rounds 5] [--step 3] [--resources FILE] [--out FILE]
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

# (H = W, width = Cin, Cout, Bottlenecks per step)
SHAPES = [(56, 64, 256, 3), (28, 128, 512, 4), (14, 256, 1024, 6), (7, 512, 2048, 3)]


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
    from pytorch_distributed_training_tutorials_amd.ops import convbn

    C = native()
    torch.backends.cudnn.benchmark = True  # MIOpen exhaustive find, as benchmarks/resnet_ddp.py runs it
    dev = torch.device("cuda", 0)
    rows = []
    for hw, cin, cout, cnt in SHAPES:
        M = batch * hw * hw
        cl = dict(memory_format=torch.channels_last)
        x4 = torch.randn(batch, cin, hw, hw, device=dev).to(torch.bfloat16).contiguous(**cl)  # conv2's output
        w4 = (torch.randn(cout, cin, 1, 1, device=dev) * cin ** -0.5).to(torch.bfloat16)
        w2 = w4.reshape(cout, cin)
        g2w, g2b = torch.rand(cin, device=dev) + 0.5, torch.randn(cin, device=dev) * 0.1
        x2 = x4.permute(0, 2, 3, 1).reshape(M, cin)
        tile = convbn._tile(M, cout, cin)
        tk_pre = torch.zeros(C.conv1x1_pre_num_tickets(M, cin, cout), dtype=torch.int32, device=dev)
        tk_old = torch.zeros(C.conv1x1_bn_num_tickets(M, cout, tile, cin), dtype=torch.int32, device=dev)

        def f_pre():
            st = C.bn_fwd_stats(x4, g2w, g2b, None, None, None, 0.1, 1e-5)
            return C.conv1x1_pre_bn_stats(x2, st, w2, None, None, None, None, None, 0.1, 1e-5, tk_pre)

        def f_fused():
            a4, _, _ = C.bn_fwd_train(x4, g2w, g2b, None, None, None, None, True, 0.1, 1e-5)
            return C.conv1x1_bn_stats(a4.permute(0, 2, 3, 1).reshape(M, cin), w2, None, None, None, None, None, 0.1,
                                      1e-5, tk_old, tile)

        def f_miopen():
            a4, _, _ = C.bn_fwd_train(x4, g2w, g2b, None, None, None, None, True, 0.1, 1e-5)
            y4 = torch.nn.functional.conv2d(a4, w4).contiguous(**cl)
            return y4, C.bn_fwd_stats(y4, None, None, None, None, None, 0.1, 1e-5)

        (yp, sp), (yf, _) = f_pre(), f_fused()
        ey = float((yp.float() - yf.float()).abs().max() / yf.float().abs().max())

        # backward operands: bn3's masked gradient g and coefficients, as its reduce pass leaves them
        a4, pst, _ = C.bn_fwd_train(x4, g2w, g2b, None, None, None, None, True, 0.1, 1e-5)
        a2 = a4.permute(0, 2, 3, 1).reshape(M, cin)
        g2 = torch.randn(M, cout, device=dev).to(torch.bfloat16)
        coef = (torch.randn(3, cout, device=dev) * torch.tensor([[1.0], [0.3], [0.1]], device=dev)).contiguous()
        old_bwd = C.conv1x1_bwd if C.conv1x1_bwd_supported(cin, cout) else C.conv1x1_bwd_tiled

        def b_pre():
            da, dw = C.conv1x1_bwd_tiled(g2, yp, x2, w2, coef, pst[2:4])
            return C.bn_bwd(da.view(batch, hw, hw, cin).permute(0, 3, 1, 2), x4, None, g2w, pst, True, False, True), dw

        def b_parent():
            da, dw = old_bwd(g2, yp, a2, w2, coef)
            return C.bn_bwd(da.view(batch, hw, hw, cin).permute(0, 3, 1, 2), x4, None, g2w, pst, True, False, True), dw

        (_, dwp), (_, dwo) = b_pre(), b_parent()
        ew = float((dwp.float() - dwo.float()).abs().max() / dwo.float().abs().max())
        arms = {"fwd_pre": f_pre, "fwd_fused": f_fused, "fwd_miopen": f_miopen, "bwd_pre": b_pre, "bwd_parent": b_parent}
        t = {k: [] for k in arms}
        for _ in range(rounds):
            for k, fn in arms.items():
                t[k].append(timed(fn))
        rec = {"K": cin, "N": cout, "M": M, "per_step": cnt, "fused_engine": "stream" if tile == 0 else f"tile{tile}",
               "parent_bwd": "stream" if old_bwd is C.conv1x1_bwd else "tiled",
               "saved_MB": round(2 * M * cin / 1e6, 1), "y_rel_diff": round(ey, 5), "dw_rel_diff": round(ew, 5)}
        for k, v in t.items():
            rec[k] = [round(statistics.median(v), 1), round(min(v), 1), round(max(v), 1)]
        print(json.dumps(rec), flush=True)
        rows.append(rec)
    return rows


def step_ab(runs, steps):
    """ms/step and peak allocated MB of the flagship benchmark per PTDT_CONVBN_PRE value, child processes
    alternated, both at PTDT_CONVBN_BWD=all."""
    out = {"0": [], "1": []}
    for _ in range(runs):
        for mode in out:
            env = dict(os.environ, PTDT_CONVBN_BWD="all", PTDT_CONVBN_PRE=mode)
            p = subprocess.run([sys.executable, os.path.join(ROOT, "benchmarks", "resnet_ddp.py"), "--steps",
                                str(steps), "--warmup", "10"], env=env, stdout=subprocess.PIPE, text=True, timeout=600)
            if p.returncode != 0:
                raise RuntimeError(f"resnet_ddp.py failed with PTDT_CONVBN_PRE={mode} (exit {p.returncode})")
            rec = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
            out[mode].append((rec["ms_per_step"], rec["peak_mem_MB"], rec["final_loss"]))
            print(json.dumps({"PTDT_CONVBN_PRE": mode, "ms_per_step": rec["ms_per_step"],
                              "peak_mem_MB": rec["peak_mem_MB"], "final_loss": rec["final_loss"]}), flush=True)
    return out


def _cell(v):
    return f"{v[0]} ({v[1]} .. {v[2]})"


def markdown(rows, ab, batch, resources):
    ln = ["# Input BN + ReLU inside the 1x1 conv + BN-statistics kernels (PTDT_CONVBN_PRE)", "",
          f"Batch {batch}, NHWC bf16; median of alternated rounds (min .. max), us, device events. bn3's apply and "
          "reduce passes are common to every arm and not timed. `saved MB`: the activation a = ReLU(bn2(y2)) the "
          "knob neither writes nor keeps for the backward, from the shape.", "",
          "Not built: a streaming instance of the prologue for layer1's 64 -> 256 (a `PRE` flag of "
          "`conv1x1_bn_stream_kernel`). Every shape below, 64 -> 256 included, runs the tiled kernel of "
          "`conv1x1_pre.hip`, against the streaming kernels where the parent has them. `bn_fwd_stats` is "
          "`bn_forward_train` with no output tensor, the statistics-only form `BnFwdArgs` already had (`y == nullptr`), "
          "so no new flag was added.", "",
          "## Forward: bn_fwd_stats + conv1x1_pre_bn_stats vs bn_fwd_train + the existing forwards", "",
          "| (K, N) | M | per step | pre | fused (engine) | MIOpen + stats pass | pre / best other | Y diff |",
          "|---|---:|---:|---:|---:|---:|---:|---:|"]
    lose = []
    for r in rows:
        best = min(r["fwd_fused"][0], r["fwd_miopen"][0])
        ln.append(f"| ({r['K']}, {r['N']}) | {r['M']} | {r['per_step']} | {_cell(r['fwd_pre'])} | "
                  f"{_cell(r['fwd_fused'])} ({r['fused_engine']}) | {_cell(r['fwd_miopen'])} | "
                  f"{r['fwd_pre'][0] / best:.2f} | {r['y_rel_diff']} |")
    ln += ["", "## Backward: conv1x1_bwd_tiled(pre=) + bn2's bn_bwd vs the parent's linked backward + bn_bwd", "",
           "| (K, N) | pre | parent (kernel) | pre / parent | dW diff | saved MB |", "|---|---:|---:|---:|---:|---:|"]
    for r in rows:
        ln.append(f"| ({r['K']}, {r['N']}) | {_cell(r['bwd_pre'])} | {_cell(r['bwd_parent'])} ({r['parent_bwd']}) | "
                  f"{r['bwd_pre'][0] / r['bwd_parent'][0]:.2f} | {r['dw_rel_diff']} | {r['saved_MB']} |")
        # loses outside the arms' spread: pre's fastest round is slower than the other path's slowest
        other = min((r["fwd_fused"], r["fwd_miopen"]), key=lambda v: v[0])
        if r["fwd_pre"][1] + r["bwd_pre"][1] > other[2] + r["bwd_parent"][2]:
            lose.append(f"{r['K']}x{r['N']}")
    tot = {k: sum(r["per_step"] * r[k][0] for r in rows) for k in ("fwd_pre", "fwd_fused", "fwd_miopen", "bwd_pre",
                                                                  "bwd_parent")}
    ln += ["", "Sum over a step's 16 Bottlenecks (medians): forward pre {fwd_pre:.0f} us, fused {fwd_fused:.0f} us, "
           "MIOpen {fwd_miopen:.0f} us; backward pre {bwd_pre:.0f} us, parent {bwd_parent:.0f} us.".format(**tot), "",
           "Shapes where forward + backward lose outside the arms' spread: " +
           (", ".join(lose) + f" (suggested `PTDT_CONVBN_PRE_SKIP={','.join(lose)}`)." if lose else "none."), ""]
    if ab:
        ln += ["## Whole step: benchmarks/resnet_ddp.py, 1 GPU, PTDT_CONVBN_BWD=all, PTDT_CONVBN_PRE=0 vs 1 "
               "(alternated runs)", "",
               "| PTDT_CONVBN_PRE | ms/step per run | median | spread | peak allocated MB | final loss per run |",
               "|---|---|---:|---:|---:|---|"]
        for mode, v in ab.items():
            ms = [t[0] for t in v]
            ln.append(f"| {mode} | {', '.join(f'{t:.3f}' for t in ms)} | {statistics.median(ms):.3f} | "
                      f"{max(ms) - min(ms):.3f} | {statistics.median(t[1] for t in v):.1f} | "
                      f"{', '.join(f'{t[2]:.4f}' for t in v)} |")
        m0, m1 = ([t[0] for t in ab[k]] for k in ("0", "1"))
        verdict = ("improves outside the spread" if max(m1) < min(m0) else
                   "is slower outside the spread" if min(m1) > max(m0) else "does not change outside the spread")
        ln += ["", f"The whole step {verdict} of the two arms.", ""]
    if resources:
        ln += ["## Compiler resource report (-Rpass-analysis=kernel-resource-usage)", "", "```", resources.rstrip(),
               "```", ""]
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
        raise SystemExit("conv1x1_pre_probe: needs a GPU")
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
