"""The loss ring counted from the epoch list (csrc/kernels/wave_loop_schedule.h: wave_ring_from_list,
wave_ring_slots, wave_ring_first_slot), on the host through ``wave_loop_schedule``,
``wave_loop_check_runs`` and ``wave_loop_run_length``.

A lean launch from (e0, j0) over epochs of S steps at gather depth D stores step k's loss shares in
slot (j0 + k + D) % (3 S) where S >= D, and in slot k % (2 S + D) otherwise (and wherever the LDS does
not hold 3 S slots). The read behind step k is position j0 + k + D + 1, so under the first rule the
ring ends exactly where a list ends. Checked here, before anything is launched:

- no slot is stored again before the helper waves' reduction bound has passed its previous step: the
  helpers reduce the steps before (e0 + i) S - D behind epoch barrier i and are done with them at
  barrier i + 1 at the latest, and they never read a step that is not stored;
- where S >= D a run of unchecked groups ends only where the list or the launch ends;
- with the default ring and start slot both bindings return what they returned before."""
import pytest

B = 32
DEPTHS = (3, 4)


def _ring(S, D):
    """(slots, first slot of a launch from j0 = 0) by the kernel's rule, the LDS holding either ring."""
    return (3 * S, D) if S >= D else (2 * S + D, 0)


def _first_slot(S, D, j0):
    ring, s0 = _ring(S, D)
    return j0 + s0 if S >= D else 0


def _launch_lengths(ring, D):
    # 0, shorter than a group, every n % D next to one ring, and three rings
    return [0, 1, D + 1, ring + 1, ring + 2, 3 * ring]


def _check_reuse(S, D, j0, n, ring, slot0, flags, slots):
    case = (S, D, j0, n)
    assert list(slots) == [(slot0 + k) % ring for k in range(n)], case
    # barrier i stands in front of the i-th flagged read; read r follows step r - D - 1 (the first
    # 1 + D reads are the prologue's): `done` steps are stored when the barrier is taken
    done = [max(0, r - D) for r, f in enumerate(flags) if f]
    bound = [max(0, min((i + 1) * S - D, j0 + n) - j0) for i in range(len(done))]  # e0 = 0: pos0 = j0
    for i, (d, b) in enumerate(zip(done, bound)):
        assert b <= d, (case, "helpers would read an unwritten step", i)
    taken = 0
    for k in range(ring, n):  # step k stores into the slot of step k - ring
        while taken < len(done) and done[taken] <= k:
            taken += 1
        # behind barrier `taken` the helpers may still be at work on bound[taken - 1]; bound[taken - 2] is done
        reduced = bound[taken - 2] if taken >= 2 else 0
        assert k - ring < reduced, (case, "slot stored again before it was reduced", k)


@pytest.mark.parametrize("D", DEPTHS)
@pytest.mark.parametrize("S0", range(1, 71, 10))
def test_no_slot_is_stored_again_before_it_is_reduced(native, S0, D):
    for S in range(S0, S0 + 10):
        ring, _ = _ring(S, D)
        for j0 in range(S):
            slot0 = _first_slot(S, D, j0)
            for n in _launch_lengths(ring, D):
                _, flags, slots, barriers, _ = native.wave_loop_schedule(S, B, 0, j0, n, D, ring, slot0)
                assert barriers == sum(flags)
                _check_reuse(S, D, j0, n, ring, slot0, flags, slots)


@pytest.mark.parametrize("D", DEPTHS)
def test_parent_ring_passes_the_same_check(native, D):
    """The ring from the launch start (every S, the S < D fallback included) under the same check."""
    for S in range(1, 20):
        ring = 2 * S + D
        for j0 in range(S):
            for n in _launch_lengths(ring, D):
                _, flags, slots, _, _ = native.wave_loop_schedule(S, B, 0, j0, n, D)
                _check_reuse(S, D, j0, n, ring, 0, flags, slots)


@pytest.mark.parametrize("D", DEPTHS)
@pytest.mark.parametrize("S0", range(1, 71, 10))
def test_runs_end_only_at_list_or_launch_end(native, S0, D):
    """Every launch walked group by group as wave_loop_run does: run() in front of every group is the
    smaller of the whole groups left in the list and in the launch, never the ring's. The run lengths and
    advance() themselves are checked against fits() by wave_loop_check_runs."""
    for S in range(S0, S0 + 10):
        ring, s0 = _ring(S, D)
        launches, boundaries, bad = native.wave_loop_check_runs(S, B, D, 3 * ring, ring, s0, 1 if S >= D else 0)
        assert bad is None, (S, D, bad)
        assert launches == S * (3 * ring + 1)
        assert boundaries == S * sum(n // D for n in range(3 * ring + 1))
        if S < D:
            continue
        for j0 in range(S):
            n = 3 * ring
            left = n // D
            ij = (j0 + D) % S + 1  # after the prologue's 1 + D reads
            rslot = _first_slot(S, D, j0)
            ring_ends = 0
            while left > 0:
                r, ij2, _, rslot2 = native.wave_loop_run_length(S, B, D, ring, ij, rslot, left)
                assert r == min((S - ij) // D, left), (S, D, j0, ij, rslot, left)
                ij, rslot, left = ij2, rslot2, left - r
                if left > 0:  # the checked group behind the run
                    switched = False
                    for _ in range(D):
                        if ij == S:
                            ij, switched = 0, True
                        ij += 1
                        rslot += 1
                        if rslot == ring:
                            assert ij == 1, (S, D, j0, "the ring ends where the list does not")
                            rslot = 0
                            ring_ends += 1
                    assert switched, (S, D, j0, "a checked group without a list end")
                    left -= 1
            assert ring_ends >= 2, (S, D, j0)


@pytest.mark.parametrize("D", DEPTHS)
def test_default_ring_and_start_slot_are_the_parents(native, D):
    for S in (1, 2, 3, 4, 5, 7, 16, 64, 70):
        ring = 2 * S + D
        for j0 in sorted({0, S // 2, S - 1}):
            for n in (0, 1, D, ring - 1, ring, 2 * ring + 1):
                plain = native.wave_loop_schedule(S, B, 0, j0, n, D)
                assert plain == native.wave_loop_schedule(S, B, 0, j0, n, D, 0, 0)
                assert plain == native.wave_loop_schedule(S, B, 0, j0, n, D, ring, 0)
                assert list(plain[2]) == [k % ring for k in range(n)]
        plain = native.wave_loop_check_runs(S, B, D, 2 * ring)
        assert plain[2] is None
        assert plain == native.wave_loop_check_runs(S, B, D, 2 * ring, 0, 0, 0)
        assert plain == native.wave_loop_check_runs(S, B, D, 2 * ring, ring, 0, 0)
