"""Arithmetic of the LDS operand tiles (csrc/kernels/lds_tile.h).

The LDS-DMA GEMMs (gemm_big.hip, int8_mm.hip, conv1x1_bn.hip) stage their operand tiles, swizzle them
over the banks and read their fragments back with the same few functions; conv1x1_bn.hip and
conv1x1_bwd.hip share the channel map of their paired MFMA tiles. That part holds no device code, so
it is checked here on the host, exhaustively for the row sizes and tile shapes the kernels
instantiate, in a program of its own built with AddressSanitizer and UBSan
(tools/lds_tile_check.cpp: the properties are listed there)."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_swizzle_staging_and_channel_maps_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or "g++"  # the sanitizer runtimes linked in: nothing to preload, no link-order rule
    exe = tmp_path / "lds_tile_check"
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-static-libasan", "-static-libubsan", "-I" + os.path.join(ROOT, "csrc"),
           os.path.join(ROOT, "tools", "lds_tile_check.cpp"), "-o", str(exe)]
    b = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert b.returncode == 0, b.stdout  # a missing compiler or runtime fails the test
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    assert "checks ok" in r.stdout
