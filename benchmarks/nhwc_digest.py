#!/usr/bin/env python3
"""SHA-256 digests of what the NHWC statistics kernels compute, for build-to-build comparisons.

Runs the BatchNorm (local and cross-rank), conv1x1+BN statistics, max-pool and eval-apply calls of
the extension directly, on inputs drawn from a seeded CPU generator (so two builds see the same
bytes), and prints one JSON line with the digest of every output tensor and of every buffer updated
in place (running statistics, num_batches_tracked, tickets). Two builds that compute the same bits
print the same ``digests``; load another build with ``PTDT_EXT_PATH``:

    python benchmarks/nhwc_digest.py --tag new
    PTDT_EXT_PATH=/path/to/other/_C.so python benchmarks/nhwc_digest.py --tag parent

The wide channel tile (PTDT_BN_TC=32) is read once per process, so that section runs in a child.
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import subprocess
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DEV = torch.device("cuda", 0)
OUT: dict[str, str] = {}


def digest(name, t):
    if t is None:
        return
    c = t.detach().cpu()
    if c.dim() == 4:  # channels_last: hash the bytes in memory order
        c = c.permute(0, 2, 3, 1)
    OUT[name] = hashlib.sha256(c.contiguous().reshape(-1).view(torch.uint8).numpy().tobytes()).hexdigest()[:32]


def gen_for(name):
    return torch.Generator().manual_seed(int.from_bytes(hashlib.sha256(name.encode()).digest()[:4], "little"))


def randn(g, shape, dtype=torch.float32, scale=1.0, shift=0.0):
    return (torch.randn(shape, generator=g) * scale + shift).to(dtype).to(DEV)


def bn_params(g, C):
    w, b = randn(g, (C,), scale=0.5, shift=1.0), randn(g, (C,), scale=0.3)
    rm, rv = randn(g, (C,), scale=0.1), randn(g, (C,), scale=0.1).abs() + 0.5
    return w, b, rm, rv, torch.zeros((), dtype=torch.long, device=DEV)


def bn_local(C_, name, dtype, M, C):
    """bn_fwd_train + bn_bwd: (residual, relu, want_mask / y for the backward's mask, dy2)."""
    g = gen_for(name)
    x, dy = randn(g, (M, C), dtype, 1.5, 0.7), randn(g, (M, C), dtype)
    res, dy2 = randn(g, (M, C), dtype), randn(g, (M, C), dtype)
    tickets = torch.zeros(64, dtype=torch.int32, device=DEV)
    for tag, use_res, relu, want_mask, use_y, use_dy2 in (
            ("lin", False, False, False, False, False), ("relu_x", False, True, False, False, False),
            ("relu_y", False, True, False, True, False), ("res_mask_dy2", True, True, True, False, True),
            ("res_y", True, True, False, True, False), ("res_lin_dy2", True, False, False, False, True)):
        w, b, rm, rv, nbt = bn_params(gen_for(name + tag), C)
        y, stats, mask = C_.bn_fwd_train(x, w, b, rm, rv, nbt, res if use_res else None, relu, 0.1, 1e-5, tickets,
                                         want_mask)
        dx, dw, db, dres = C_.bn_bwd(dy, x, y if use_y else None, w, stats, relu, use_res, True, tickets, None, None,
                                     dy2 if use_dy2 else None, mask if want_mask else None)
        for k, t in (("y", y), ("stats", stats), ("mask", mask if want_mask else None), ("rm", rm), ("rv", rv),
                     ("nbt", nbt), ("tickets", tickets), ("dx", dx), ("dw", dw), ("db", db),
                     ("dres", dres if use_res else None)):
            digest(f"{name}/{tag}/{k}", t)


def bn_sync(C_, name, M, C):
    g = gen_for(name)
    x, dy, dy2 = randn(g, (M, C), torch.bfloat16, 1.5, 0.7), randn(g, (M, C), torch.bfloat16), randn(g, (M, C), torch.bfloat16)
    w, b, rm, rv, nbt = bn_params(g, C)
    tickets = torch.zeros(64, dtype=torch.int32, device=DEV)
    rec = torch.zeros(2 * C + 1, dtype=torch.float64, device=DEV)
    C_.bn_sync_stats(x, rec, tickets)
    other = torch.cat([torch.randn(C, generator=g, dtype=torch.float64) * 0.2 + 0.7,
                       torch.rand(C, generator=g, dtype=torch.float64) * 2000.0 + 1500.0,
                       torch.tensor([1000.0], dtype=torch.float64)]).to(DEV)
    recs = torch.stack([rec, torch.zeros_like(rec), other])  # the middle rank has no rows
    stats, count = C_.bn_sync_merge(recs, w, b, rm, rv, nbt, 0.1, 1e-5)
    gg, dw, db, sums = C_.bn_sync_bwd_reduce(dy, x, w, stats, True, True, tickets, None, None, dy2, None)
    coef = C_.bn_sync_coef(sums * 2.0, count, w, stats)  # "all-reduced" over two equal ranks
    dx = C_.bn_bwd_apply_g(gg, x, coef)
    for k, t in (("rec", rec), ("stats", stats), ("count", count), ("rm", rm), ("rv", rv), ("nbt", nbt),
                 ("tickets", tickets), ("g", gg), ("dw", dw), ("db", db), ("sums", sums), ("coef", coef), ("dx", dx)):
        digest(f"{name}/{k}", t)


def convbn(C_, name, M, K, N, tile):
    g = gen_for(name)
    x, wt = randn(g, (M, K), torch.bfloat16), randn(g, (N, K), torch.bfloat16, 0.1)
    w, b, rm, rv, nbt = bn_params(g, N)
    tickets = torch.zeros(C_.conv1x1_bn_num_tickets(M, N, tile, K), dtype=torch.int32, device=DEV)
    for launch in (1, 2):  # the second launch runs on re-armed tickets and the updated running mean
        y, stats = C_.conv1x1_bn_stats(x, wt, w, b, rm, rv, nbt, 0.1, 1e-5, tickets, tile)
        for k, t in (("y", y), ("stats", stats), ("rm", rm), ("rv", rv), ("nbt", nbt), ("tickets", tickets)):
            digest(f"{name}/launch{launch}/{k}", t)


def pool(C_, name, dtype):
    g = gen_for(name)
    x = randn(g, (2, 16, 9, 9), dtype).contiguous(memory_format=torch.channels_last)
    x[0, :, 0:2, 0:2] = float("-inf")  # output (0, 0)'s window holds -inf only
    x[1, 3, 4, 4] = float("nan")
    gy = randn(g, (2, 16, 5, 5), dtype).contiguous(memory_format=torch.channels_last)
    scale, shift = randn(g, (16,), scale=0.5, shift=1.0), randn(g, (16,), scale=0.3)
    for tag, sc, sf, relu in (("plain", None, None, False), ("affine", scale, shift, False),
                              ("affine_relu", scale, shift, True)):
        y, arg = C_.maxpool2d_fwd(x, [3, 3], [2, 2], [1, 1], sc, sf, relu)
        gx = C_.maxpool2d_bwd(gy, arg, [2, 16, 9, 9], [3, 3], [2, 2], [1, 1])
        for k, t in (("y", y), ("arg", arg), ("gx", gx)):
            digest(f"{name}/{tag}/{k}", t)


def apply_eval(C_, name, M, C):
    g = gen_for(name)
    x, res = randn(g, (M, C), torch.bfloat16, 1.5, 0.7), randn(g, (M, C), torch.bfloat16)
    digest(f"{name}/y", C_.bn_apply(x, res, randn(g, (C,), scale=0.5, shift=1.0), randn(g, (C,), scale=0.3), True))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--tag", default=None, help="free-form label of the build, copied into the JSON line")
    ap.add_argument("--section", default="all", choices=["all", "wide"], help="wide: the PTDT_BN_TC=32 child")
    a = ap.parse_args()
    if a.section == "all":  # the wide-tile section first, in a process of its own
        child = subprocess.run([sys.executable, os.path.abspath(__file__), "--section", "wide"],
                               env=dict(os.environ, PTDT_BN_TC="32"), stdout=subprocess.PIPE, text=True, check=True)
        OUT.update(json.loads(child.stdout.strip().splitlines()[-1])["digests"])
    from pytorch_distributed_training_tutorials_amd._ext import native

    C_ = native()
    if a.section == "wide":
        bn_local(C_, "bn_bf16_4096x256_tc32", torch.bfloat16, 4096, 256)
    else:
        bn_local(C_, "bn_bf16_4096x128", torch.bfloat16, 4096, 128)
        bn_local(C_, "bn_f32_3001x20", torch.float32, 3001, 20)
        bn_sync(C_, "syncbn_bf16_4096x128", 4096, 128)
        for tile in (128, 256):
            convbn(C_, f"convbn_tile{tile}_643x64x136", 643, 64, 136, tile)
        convbn(C_, "convbn_stream_25088x64x256", 25088, 64, 256, 0)
        convbn(C_, "convbn_stream_25088x256x64", 25088, 256, 64, 0)
        pool(C_, "pool_bf16", torch.bfloat16)
        pool(C_, "pool_f32", torch.float32)
        apply_eval(C_, "bn_apply_bf16_4096x128", 4096, 128)
    torch.cuda.synchronize()
    ext = "PTDT_EXT_PATH" if os.environ.get("PTDT_EXT_PATH") else "in-tree"
    print(json.dumps({"tag": a.tag, "ext": ext, "n": len(OUT), "digests": dict(sorted(OUT.items()))}), flush=True)


if __name__ == "__main__":
    main()
