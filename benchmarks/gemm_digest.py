#!/usr/bin/env python3
"""SHA-256 digests of what the LDS-DMA GEMMs compute, for build-to-build comparisons.

Runs ``gemm_big_`` (every schedule of the 256 tile, the 128 tile; f32 and bf16 output; plain and with
bias + ReLU + alpha + beta) and ``int8_mm`` (shapes that reach the tiled, the 256-tile ping-pong and the
direct kernel) of the extension directly, on inputs drawn from a seeded CPU generator (so two builds
see the same bytes), and prints one JSON line with the digest of every output. Two builds that
compute the same bits print the same ``digests``; load another build with ``PTDT_EXT_PATH``:

    python benchmarks/gemm_digest.py --tag new
    PTDT_EXT_PATH=/path/to/other/_C.so python benchmarks/gemm_digest.py --tag parent

Split-K is left out: its slices meet in fp32 atomics in arrival order, which differs run to run.
``benchmarks/nhwc_digest.py`` covers the conv1x1 + BatchNorm kernels that share the tile code.
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DEV = torch.device("cuda", 0)
OUT: dict[str, str] = {}

GEMM_SHAPES = [(256, 256, 64), (300, 200, 128), (1, 257, 64), (1000, 17, 192), (512, 768, 1024)]
INT8_SHAPES = [(70, 50, 128), (130, 260, 384), (5, 130, 48), (3845, 4090, 384)]


def digest(name, t):
    OUT[name] = hashlib.sha256(t.detach().cpu().contiguous().reshape(-1).view(torch.uint8).numpy().tobytes()).hexdigest()[:32]


def gen_for(name):
    return torch.Generator().manual_seed(int.from_bytes(hashlib.sha256(name.encode()).digest()[:4], "little"))


def gemm_big(C_, M, N, K):
    g = gen_for(f"gemm_{M}x{N}x{K}")
    A = (torch.rand(M, K, generator=g) * 2 - 1).to(torch.bfloat16).to(DEV)
    Bt = (torch.rand(N, K, generator=g) * 2 - 1).to(torch.bfloat16).to(DEV)
    bias, c0 = torch.randn(N, generator=g).to(DEV), torch.randn(M, N, generator=g)
    for tile, scheds in ((256, range(7)), (128, (0, 1))):
        for sched in scheds:
            for dt in (torch.float32, torch.bfloat16):
                name = f"gemm_{M}x{N}x{K}/tile{tile}/sched{sched}/{str(dt)[6:]}"
                C = torch.empty(M, N, device=DEV, dtype=dt)
                C_.gemm_big_(A, Bt, C, sched=sched, tile=tile)
                digest(name + "/plain", C)
                C1 = c0.to(dt).to(DEV)
                C_.gemm_big_(A, Bt, C1, bias, True, 0.5, 2.0, sched, tile=tile)
                digest(name + "/bias_relu_alpha_beta", C1)


def int8_mm(C_, M, N, K):
    g = gen_for(f"int8_{M}x{N}x{K}")
    A = torch.randint(-127, 128, (M, K), generator=g, dtype=torch.int8).to(DEV)
    B = torch.randint(-127, 128, (N, K), generator=g, dtype=torch.int8).to(DEV)
    sa, sb = (torch.rand(M, generator=g) * 0.01).to(DEV), (torch.rand(N, generator=g) * 0.01).to(DEV)
    add, bias = torch.randn(M, N, generator=g).to(DEV), torch.randn(N, generator=g).to(DEV)
    ones_m, ones_n = torch.ones(M, device=DEV), torch.ones(N, device=DEV)
    digest(f"int8_{M}x{N}x{K}/exact", C_.int8_mm(A, ones_m, B, ones_n))
    for out in ("float32", "bfloat16", "float16"):
        digest(f"int8_{M}x{N}x{K}/epilogue_{out}", C_.int8_mm(A, sa, B, sb, add, bias.to(getattr(torch, out)), out))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--tag", default=None, help="free-form label of the build, copied into the JSON line")
    a = ap.parse_args()
    from pytorch_distributed_training_tutorials_amd._ext import native

    C_ = native()
    for shape in GEMM_SHAPES:
        gemm_big(C_, *shape)
    for shape in INT8_SHAPES:
        int8_mm(C_, *shape)
    torch.cuda.synchronize()
    ext = "PTDT_EXT_PATH" if os.environ.get("PTDT_EXT_PATH") else "in-tree"
    print(json.dumps({"tag": a.tag, "ext": ext, "n": len(OUT), "digests": dict(sorted(OUT.items()))}), flush=True)


if __name__ == "__main__":
    main()
