"""Run length of the wave engine's lean step loop (csrc/kernels/wave_loop_schedule.h).

The lean kernels run unchecked groups of three steps in runs: ``WaveLoopSchedule::run()`` is the number
of consecutive groups, from the current state, for which ``fits()`` holds (a closed form of what is
left of the epoch list, of the loss ring and of the launch), and ``advance(r)`` moves the state by a
whole run. Both are compared here with repeated ``fits()`` / ``advance()``: written out in Python from
every state of small shapes, and in the extension at every group boundary of every launch of the
shapes the kernels meet. A run that is a group too long reads past a list's end or skips an epoch
barrier, which hangs the GPU, so this runs on the host, before anything is launched."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEPTHS = (2, 3, 4)


def _repeat(S, B, depth, ring, ij, rslot, left):
    """(run, ij, lofs, rslot) by fits() and advance(), one group at a time."""
    lofs, run = ij * B, 0
    while run < left and S - ij >= depth and ring - rslot > depth:  # fits()
        ij, lofs, rslot, run = ij + depth, lofs + depth * B, rslot + depth, run + 1  # advance()
    return run, ij, lofs, rslot


@pytest.mark.parametrize("depth", DEPTHS)
def test_run_length_from_every_state(native, depth):
    """Every state (ij <= S, rslot < ring, groups left) of S = 1..9, reachable or not."""
    B = 32
    for S in range(1, 10):
        ring = 2 * S + depth
        for ij in range(S + 1):
            for rslot in range(ring):
                for left in range(ring // depth + 3):
                    got = tuple(native.wave_loop_run_length(S, B, depth, ring, ij, rslot, left))
                    assert got == _repeat(S, B, depth, ring, ij, rslot, left), (S, ij, rslot, left)


def test_flagship_epoch_runs(native):
    """S = 64, depth 3, ring 131: a run from the list's start is 21 groups, cut to the groups left; at
    ij = 63 or with rslot = 128 no group fits."""
    assert tuple(native.wave_loop_run_length(64, 32, 3, 131, 0, 0, 1000)) == (21, 63, 63 * 32, 63)
    assert tuple(native.wave_loop_run_length(64, 32, 3, 131, 0, 0, 5)) == (5, 15, 15 * 32, 15)
    assert tuple(native.wave_loop_run_length(64, 32, 3, 131, 63, 3, 1000))[0] == 0
    assert tuple(native.wave_loop_run_length(64, 32, 3, 131, 2, 128, 1000))[0] == 0
    assert tuple(native.wave_loop_run_length(64, 32, 3, 131, 2, 127, 1000))[0] == 1  # slots 127..129 and 130 to spare
    assert tuple(native.wave_loop_run_length(64, 32, 3, 131, 2, 100, 1000))[0] == 10  # cut by the ring, not the list


@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("S0", range(1, 71, 10))
def test_runs_in_every_launch(native, S0, depth):
    """S 1..70, every j0, ring = 2 S + depth, n 0..3 ring: in front of every group of every launch, run()
    and advance(run()) against repeated fits() / advance() (wave_loop_check_runs)."""
    for S in range(S0, S0 + 10):
        ring = 2 * S + depth
        launches, boundaries, bad = native.wave_loop_check_runs(S, 32, depth, 3 * ring)
        assert bad is None, (S, depth, bad)
        assert launches == S * (3 * ring + 1)
        assert boundaries == S * sum(n // depth for n in range(3 * ring + 1))  # every group of every launch


def test_standalone_program_under_sanitizers(tmp_path):
    """The same ranges in a host program of its own, built with AddressSanitizer and UBSan, with the
    reads and slots of the launches enumerated into exactly sized arrays."""
    cxx = shutil.which("g++") or "g++"  # the sanitizer runtimes linked in: nothing to preload
    exe = tmp_path / "wave_loop_runs_check"
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-static-libasan", "-static-libubsan", "-I" + os.path.join(ROOT, "csrc"),
           os.path.join(ROOT, "tools", "wave_loop_runs_check.cpp"), "-o", str(exe)]
    b = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert b.returncode == 0, b.stdout  # a missing compiler or runtime fails the test
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    assert "enumerated ok" in r.stdout
