"""The row image of the wave engine's layout F (csrc/kernels/wave_row_image.h): a dataset row as four
records, one per feature group q, of ``RS = round_up(KP + (KP odd) + 1, 4)`` floats -- the group's KP
features (0 past Din), 1.0 if KP is odd, the row's target, zeros. The header is the one the pack kernel
and the lean kernels compile; here its binding is compared with the layout written out in NumPy, and a
stand-alone program (tools/wave_row_image_check.cpp) packs images on the host under sanitizers."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KPS = [4, 5, 8, 10, 16]  # every KP of layout F's table for one-output models
ONE, Y, ZERO = -1, -2, -3


def _reference(din, kp):
    """(RS, source[q][s]) from the definition."""
    used = kp + (kp % 2) + 1
    rs = (used + 3) // 4 * 4
    src = np.full((4, rs), ZERO, dtype=np.int64)
    for q in range(4):
        for s in range(kp):
            if q * kp + s < din:
                src[q, s] = q * kp + s
        if kp % 2:
            src[q, kp] = ONE
        src[q, kp + kp % 2] = Y
    return rs, src


@pytest.mark.parametrize("kp", KPS)
def test_layout_matches_definition(native, kp):
    for din in range(1, 25):
        if 4 * kp < din:
            continue
        rs, row_bytes, one_slot, y_slot, src = native.wave_row_image_layout(din, kp)
        ref_rs, ref_src = _reference(din, kp)
        assert (rs, row_bytes) == (ref_rs, 16 * ref_rs), (din, kp)
        assert one_slot == (kp if kp % 2 else -1) and y_slot == kp + kp % 2, (din, kp)
        assert np.array_equal(np.asarray(src), ref_src), (din, kp)
        # every feature exactly once, one target per record, 1.0 only behind an odd KP
        flat = ref_src.reshape(-1)
        assert sorted(flat[flat >= 0].tolist()) == list(range(din))
        assert (flat == Y).sum() == 4 and (flat == ONE).sum() == (4 if kp % 2 else 0)
        for row in (0, 1, 95):
            for q in range(4):
                assert native.wave_row_image_offset(row, q, kp) == row * 16 * ref_rs + q * 4 * ref_rs


def test_flagship_record_is_32_bytes(native):
    rs, row_bytes, one_slot, y_slot, _ = native.wave_row_image_layout(20, 5)
    assert (rs, row_bytes, one_slot, y_slot) == (8, 128, 5, 6)


def test_limits(native):
    assert native.wave_row_image_fits((1 << 24) - 1, 20, 5)      # 2^31 - 128 bytes
    assert not native.wave_row_image_fits(1 << 24, 20, 5)        # row index past 24 bits
    assert native.wave_row_image_fits((1 << 31) // 320, 64, 16)
    assert not native.wave_row_image_fits((1 << 31) // 320 + 1, 64, 16)  # 2^31 bytes or more
    assert not native.wave_row_image_fits(8, 21, 5)              # 4 KP does not cover Din


def test_standalone_program_under_sanitizers(tmp_path):
    """Images packed on the host from exactly sized heap arrays, built with AddressSanitizer and UBSan:
    a read past Din, past the last row or a write past the image is reported."""
    cxx = shutil.which("g++") or "g++"  # the sanitizer runtimes linked in: nothing to preload, no link-order rule
    exe = tmp_path / "wave_row_image_check"
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-static-libasan", "-static-libubsan", "-I" + os.path.join(ROOT, "csrc"),
           os.path.join(ROOT, "tools", "wave_row_image_check.cpp"), "-o", str(exe)]
    b = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert b.returncode == 0, b.stdout  # a missing compiler or runtime fails the test
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    assert "cases ok" in r.stdout
