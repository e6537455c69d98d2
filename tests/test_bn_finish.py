"""Per-channel finalise of the BatchNorm statistics (csrc/kernels/bn_finish.h).

Every producer of the [4, C] statistics (the local and cross-rank BatchNorm reductions, the tiled and
the streaming conv1x1+BN kernels) forms mean / invstd / scale / shift and the running buffers with
the same two functions. They hold no device code, so they are checked here on the host, against long
double, in a program of its own built with AddressSanitizer and UBSan (tools/bn_finish_check.cpp:
the input grid and the bound are described there)."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_finalise_matches_long_double_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or "g++"  # the sanitizer runtimes linked in: nothing to preload, no link-order rule
    exe = tmp_path / "bn_finish_check"
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-static-libasan", "-static-libubsan", "-I" + os.path.join(ROOT, "csrc"),
           os.path.join(ROOT, "tools", "bn_finish_check.cpp"), "-o", str(exe)]
    b = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert b.returncode == 0, b.stdout  # a missing compiler or runtime fails the test
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    assert "checks ok" in r.stdout
