"""Loop control of the wave engine's lean step loop at the gather depth D of the deepened kernels
(wave_gather_depth in csrc/kernels/wave_kernel_rules.h; csrc/kernels/wave_loop_schedule.h is generic
in the depth). The assertions are those of tests/test_wave_loop_schedule.py and
tests/test_wave_loop_runs.py at depth 3: the schedule against the per-step rule of the generic
kernel's ``read_index``, exhaustively over small shapes, and run() / advance(run()) against repeated
fits() / advance(). A barrier too few or too many against the helper waves hangs the GPU, so this runs
on the host, before anything is launched."""
import pytest

D = 4  # wave_gather_depth of the deepened kernels


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
        for n in range(41):
            ofs, bar, slots, barriers, estride = native.wave_loop_schedule(S, B, 0, j0, n, D)
            ref_ofs, ref_bar, T = _rule(S, B, 0, j0, n, D)
            case = (S, j0, n)
            assert estride == _stride(S * B, B), case
            assert list(ofs) == ref_ofs, case
            assert list(bar) == ref_bar, case
            assert barriers == sum(ref_bar) == max(T, 0), case  # exactly T (n == 0, S == 1: T == -1, none)
            # every read inside one padded list, with the up to 64 row slots a read touches
            assert all(0 <= o < 2 * estride and o % estride + 64 <= estride for o in ofs), case
            assert list(slots) == [k % (2 * S + D) for k in range(n)], case  # loss ring slot of every step


@pytest.mark.parametrize("S0", range(1, 71, 10))
def test_runs_in_every_launch(native, S0):
    """S 1..70, every j0, ring = 2 S + D, n 0..3 ring: in front of every group of every launch, run()
    and advance(run()) against repeated fits() / advance() (wave_loop_check_runs)."""
    for S in range(S0, S0 + 10):
        ring = 2 * S + D
        launches, boundaries, bad = native.wave_loop_check_runs(S, 32, D, 3 * ring)
        assert bad is None, (S, bad)
        assert launches == S * (3 * ring + 1)
        assert boundaries == S * sum(n // D for n in range(3 * ring + 1))  # every group of every launch
