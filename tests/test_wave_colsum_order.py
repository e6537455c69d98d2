"""Operand order of the wave engine's two column-sum trees (tools/wave_colsum_order_check.cpp).

The lean-plain hand-placed step adds its six column sums as a reduce-scatter and reads each total from
one lane; every other kernel keeps the all-reduce in which each lane ends with every total. The host
model runs both lane by lane, instruction by instruction: for finite rows the total has the
all-reduce's bits in every lane, and so it has with one NaN leaf per column or sixteen equal ones, for
either rule of which operand's NaN an add returns. Run by hand it checks 10^6 rows and prints which
leaf's NaN each tree returns when all sixteen differ."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_model_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or "g++"  # the sanitizer runtimes linked in: nothing to preload
    exe = tmp_path / "wave_colsum_order_check"
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-static-libasan", "-static-libubsan", os.path.join(ROOT, "tools", "wave_colsum_order_check.cpp"),
           "-o", str(exe)]
    b = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert b.returncode == 0, b.stdout  # a missing compiler or runtime fails the test
    r = subprocess.run([str(exe), "50000"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    assert "finite: 50000 rows" in r.stdout and "the same bits in every lane, both rules" in r.stdout
    # the leaf each total's lane (kHsBcast) returns when all sixteen NaNs differ: src0 first, src1 first
    assert "leaf 15 5 11 3 15 5" in r.stdout and "leaf 0 10 4 12 0 10" in r.stdout
