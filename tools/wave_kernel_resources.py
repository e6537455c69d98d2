#!/usr/bin/env python3
"""Registers, scratch and code size of every linear_wave_f_kernel instantiation in device assembly files
(hipcc --offload-arch=gfx950 --cuda-device-only -S -fno-slp-vectorize csrc/kernels/linear_wave_*.hip).

    python3 tools/wave_kernel_resources.py DIR              one line per kernel
    python3 tools/wave_kernel_resources.py BASE_DIR DIR     lean kernels of both, and those whose scratch grew

Used to decide which lean configurations keep one group body (lean_two_bodies in
csrc/kernels/linear_wave_impl.h; profiles/wave_loop_runs.md). Needs no GPU."""
from __future__ import annotations

import glob
import os
import re
import sys

LOSS = {0: "ce_soft", 1: "ce_index", 2: "mse"}
VAR = {0: "generic", 1: "lean-plain", 2: "lean-mom"}
NAME = re.compile(r"linear_wave_f_kernelILi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)ELb([01])ELi(\d+)EE")


def read(directory):
    """{(R, KP, DOUT, loss, ar, variant): {vgpr (the unified count, AGPRs included), agpr, scratch, sgpr_spill, code}}"""
    out = {}
    for path in sorted(glob.glob(os.path.join(directory, "*.s"))):
        cur, code = None, {}
        sym = None
        for line in open(path, errors="replace"):
            m = re.match(r"^(_Z\w+):", line)
            if m:
                sym = m.group(1)
            m = re.match(r"^; codeLenInByte = (\d+)", line)
            if m and sym:
                code[sym] = int(m.group(1))
            t = line.strip()
            if t.startswith("- .agpr_count:"):
                cur = {"agpr": int(t.split()[-1])}
            elif cur is not None and t.startswith("."):
                k, _, v = t.partition(":")
                v = v.strip()
                if k == ".name":
                    cur["name"] = v
                elif k in (".private_segment_fixed_size", ".vgpr_count", ".sgpr_spill_count", ".vgpr_spill_count"):
                    cur[k] = int(v)
                if k == ".wavefront_size":  # last key of a kernel's block
                    m = NAME.search(cur.get("name", ""))
                    if m:
                        r, kp, do, loss, ar, var = (int(x) for x in m.groups())
                        out[(r, kp, do, LOSS[loss], bool(ar), VAR[var])] = {
                            "vgpr": cur[".vgpr_count"], "agpr": cur["agpr"], "scratch": cur[".private_segment_fixed_size"],
                            "sgpr_spill": cur[".sgpr_spill_count"], "code": code.get(cur["name"], 0)}
                    cur = None
    return out


def label(k):
    r, kp, do, loss, ar, var = k
    return f"<{r},{kp},{do},{loss},{'AR' if ar else '--'},{var}>"


def main(argv):
    if len(argv) == 1:
        for k, v in sorted(read(argv[0]).items()):
            print(f"{label(k):40s} regs {v['vgpr']:3d} (agpr {v['agpr']:3d}) scratch {v['scratch']:5d} sgpr-spill {v['sgpr_spill']:3d} code {v['code']:6d}")
        return 0
    base, new = read(argv[0]), read(argv[1])
    grew = []
    for k in sorted(new):
        if k[5] == "generic" or k not in base:
            continue
        b, n = base[k], new[k]
        mark = ""
        if n["scratch"] > b["scratch"]:
            mark = "  <-- scratch grew"
            grew.append(k)
        print(f"{label(k):40s} regs {b['vgpr']:3d} -> {n['vgpr']:3d} (agpr {b['agpr']:3d} -> {n['agpr']:3d})  scratch {b['scratch']:5d} -> {n['scratch']:5d}  "
              f"code {b['code']:6d} -> {n['code']:6d}{mark}")
    print(f"{len(grew)} lean kernels gained scratch")
    for k in grew:
        print("  " + label(k))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
