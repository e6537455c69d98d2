"""Loop control of the wave engine's lean step loop (csrc/kernels/wave_loop_schedule.h).

The lean kernels run a launch in groups of three steps: unchecked while a group's reads stay inside
one epoch list and its slots inside the loss ring, checked otherwise. The schedule they run is compared here, exhaustively over small shapes, with the
per-step rule of the generic kernel's ``read_index`` written out in Python: wrap when ``++ij == S``,
a barrier in front of the first read of a new epoch while ``barriers < T``. A barrier too few or too
many against the helper waves hangs the GPU, so this runs on the host, before anything is launched."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEPTH = 3  # kWavePrefetch: batches in flight


def _stride(ns, B):  # wave_list_stride
    return ((((ns + B - 1) // B) * B + 64 + 3) // 4) * 4


def _rule(S, B, e0, j0, n, depth):
    """(offsets, barrier flags, T) of the 1 + depth + (n - n % depth) reads, one step at a time."""
    estride = _stride(S * B, B)
    T = int((j0 + n - 1) / S)  # C division: truncates
    ie, ij, barriers, bar_due = e0, j0, 0, False
    lofs = (ie & 1) * estride + ij * B
    ofs, bar = [], []
    for _ in range(1 + depth + n - n % depth):
        bar.append(int(bar_due))
        if bar_due:
            barriers += 1
            bar_due = False
        ofs.append(lofs)
        lofs += B
        ij += 1
        if ij == S:
            ij, ie = 0, ie + 1
            lofs = (ie & 1) * estride
            bar_due = barriers < T
    return ofs, bar, T


@pytest.mark.parametrize("S", range(1, 9))
def test_schedule_matches_per_step_rule(native, S):
    B = 32
    for j0 in range(S):
        for e0 in (0, 1):
            for n in range(41):
                ofs, bar, slots, barriers, estride = native.wave_loop_schedule(S, B, e0, j0, n, DEPTH)
                ref_ofs, ref_bar, T = _rule(S, B, e0, j0, n, DEPTH)
                case = (S, j0, e0, n)
                assert estride == _stride(S * B, B), case
                assert list(ofs) == ref_ofs, case
                assert list(bar) == ref_bar, case
                assert barriers == sum(ref_bar) == max(T, 0), case  # exactly T (n == 0, S == 1: T == -1, none)
                # every read inside one padded list, with the up to 64 row slots a read touches
                assert all(0 <= o < 2 * estride and o % estride + 64 <= estride for o in ofs), case
                assert list(slots) == [k % (2 * S + DEPTH) for k in range(n)], case  # loss ring slot of every step


def test_other_batch_sizes_and_depths(native):
    for B in (16, 64):
        for depth in (2, 3, 4):
            for S in (1, 2, 5):
                for j0 in range(S):
                    for n in range(0, 41, 3 if depth == 3 else 1):
                        ofs, bar, slots, barriers, _ = native.wave_loop_schedule(S, B, 0, j0, n, depth)
                        ref_ofs, ref_bar, T = _rule(S, B, 0, j0, n, depth)
                        assert (list(ofs), list(bar), barriers) == (ref_ofs, ref_bar, max(T, 0)), (B, depth, S, j0, n)
                        assert list(slots) == [k % (2 * S + depth) for k in range(n)]


def test_standalone_program_under_sanitizers(tmp_path):
    """The same ranges in a host program of its own, built with AddressSanitizer and UBSan (exactly
    sized output arrays: a read or a step too many is reported)."""
    cxx = shutil.which("g++") or "g++"  # the sanitizer runtimes linked in: nothing to preload, no link-order rule
    exe = tmp_path / "wave_loop_schedule_check"
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-static-libasan", "-static-libubsan", "-I" + os.path.join(ROOT, "csrc"),
           os.path.join(ROOT, "tools", "wave_loop_schedule_check.cpp"), "-o", str(exe)]
    b = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert b.returncode == 0, b.stdout  # a missing compiler or runtime fails the test
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    assert "cases ok" in r.stdout
