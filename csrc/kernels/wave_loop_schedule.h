// Loop control of the wave engine's lean step loop (linear_wave_impl.h, layout F), as plain host /
// device arithmetic: no device intrinsics, so the same code runs in the kernel, in the Python binding
// (tests/test_wave_loop_schedule.py) and in a sanitizer-built host program (tools/wave_loop_schedule_check.cpp).
//
// The trainer wave reads one batch of list entries per *read*: read r belongs to position
// (e0, j0) + r. A launch of n steps makes 1 + depth + (n - n % depth) reads (depth = batches in
// flight): one ahead of the first gather, `depth` with the prologue's gathers, one with every step of
// the unrolled part. The per-step rule (the generic kernel's read_index) wraps after the read whose
// ++ij reaches S and takes a barrier in front of the first read of a new epoch while fewer than
// T = (j0 + n - 1) / S barriers were taken.
//
// The lean loop runs whole groups of `depth` steps in one unrolled body. A group whose reads stay
// inside the current epoch list and whose steps stay inside the loss ring runs unchecked: its reads
// only advance a running address, with no wrap test and no barrier test. Any other group runs
// with a checked read after every step (list switch, barrier) and a checked ring slot.
// Unchecked groups come in runs: run() is the number of them from the current state, a closed form
// of what is left of the list, of the ring and of the launch, so the loop looks at the state once per
// run and counts the run's groups down; advance(r) then moves the state by the whole run.
// The n % depth steps after the last group make no read; their ring slots are checked.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PTDT_HD __host__ __device__
#else
#define PTDT_HD
#endif

namespace ptdt {

struct WaveLoopSchedule {
  int S;         // steps (batches) per epoch
  int B;         // list entries per batch
  int estride;   // entries between the two epoch lists (wave_list_stride)
  int T;         // epoch barriers of this launch
  int depth;     // batches in flight: steps per unrolled group
  int ring;      // loss ring slots
  int ij;        // reads made in the current list; == S: the next read switches lists first
  int par;       // which of the two lists (epoch & 1)
  int lofs;      // entry offset of the next read
  int barriers;  // barriers taken
  int rslot;     // loss ring slot of the next step (< ring between steps)

  PTDT_HD void init(int S_, int B_, int estride_, int e0, int j0, int n, int depth_, int ring_) {
    S = S_;
    B = B_;
    estride = estride_;
    T = (j0 + n - 1) / S_;
    depth = depth_;
    ring = ring_;
    ij = j0;
    par = e0 & 1;
    lofs = par * estride_ + j0 * B_;
    barriers = 0;
    rslot = 0;
  }
  // The launch's first read, at the start position itself (j0 < S): no list switch, no barrier.
  PTDT_HD int first() {
    const int o = lofs;
    lofs += B;
    ++ij;
    return o;
  }
  // Checked read: the entry offset to read at. *switched: the read is the first of the other list
  // (otherwise it follows the previous read: a running address stays valid); *barrier: a barrier comes
  // first (the new epoch's list is ready behind it, the old one free).
  PTDT_HD int next(bool* barrier, bool* switched) {
    *barrier = false;
    *switched = false;
    if (ij == S) {
      ij = 0;
      par ^= 1;
      lofs = par * estride;
      *switched = true;
      if (barriers < T) {
        *barrier = true;
        ++barriers;
      }
    }
    const int o = lofs;
    lofs += B;
    ++ij;
    return o;
  }
  // A checked step has used ring slot rslot: true if the next step starts the ring again.
  PTDT_HD bool slot_done() {
    if (++rslot == ring) {
      rslot = 0;
      return true;
    }
    return false;
  }
  // The next group needs no check: its `depth` reads stay in the current list, and its slots and the
  // one after them in the ring (rslot < ring holds between groups).
  PTDT_HD bool fits() const { return S - ij >= depth && ring - rslot > depth; }
  // After an unchecked group: its reads were at lofs, lofs + B, ... and its slots rslot, rslot + 1, ...
  PTDT_HD void advance() { advance(1); }
  // After r unchecked groups in a row.
  PTDT_HD void advance(int r) {
    ij += r * depth;
    lofs += r * depth * B;
    rslot += r * depth;
  }
  // Run length: how many of the next `groups_left` groups run unchecked in a row, that is for how
  // many g = 0, 1, ... fits() holds after advance(g). Group g fits iff S - ij - g depth >= depth and
  // ring - rslot - g depth > depth, so the run is the smallest of (S - ij) / depth (whole groups left
  // in the list), (ring - rslot - 1) / depth (whole groups in the ring with a slot to spare) and
  // groups_left. Both numerators are >= 0 between groups (ij <= S, rslot < ring).
  PTDT_HD int run(int groups_left) const {
    const int in_list = (S - ij) / depth, in_ring = (ring - rslot - 1) / depth;
    const int r = in_list < in_ring ? in_list : in_ring;
    return r < groups_left ? r : groups_left;
  }
};

// The loop itself, after the prologue's 1 + depth reads (first(), then `depth` checked ones). Its
// control is the run length: the state is looked at when a run starts, not per group.
// unchecked(): one group of depth steps inside a run, each followed by a read. It takes no schedule
//   state: the reads and ring slots follow the caller's running addresses (step k of the run's group
//   g reads at lofs + (g depth + k) B and uses slot rslot + g depth + k, for lofs and rslot as they
//   were when the run started). The only control of a run is a down-counter; s.advance(groups run)
//   follows it once.
// checked(s): one group with s.next() and s.slot_done() after every step; one follows every run (a
//   run of no group included) unless the launch's groups are used up.
// tail(s, left): the last left < depth steps, no reads, s.slot_done() after each; returns the steps done.
// unchecked and checked return false to end the launch after the group. Returns the steps done.
template <class Unchecked, class Checked, class Tail>
PTDT_HD inline int wave_loop_run(WaveLoopSchedule& s, int n, Unchecked&& unchecked, Checked&& checked, Tail&& tail) {
  const int ngroups = n / s.depth;
  int left = ngroups;
  bool go = true;
  while (left > 0 && go) {
    const int r = s.run(left);
    int k = r;
    while (k > 0 && go) {
      go = unchecked();
      --k;
    }
    s.advance(r - k);
    left -= r - k;
    // A run is maximal: it ends at the launch's last group or where the next group does not fit.
    // The checked group follows the run on one path (not as the other arm of an if / else on r): with
    // the two bodies as siblings the compiler kept their registers apart and copied every live value,
    // the batches in flight behind a full wait included, at both ends of every run.
    if (left > 0 && go) {
      go = checked(s);
      --left;
    }
  }
  int done = (ngroups - left) * s.depth;
  if (go && done < n) done += tail(s, n - done);
  return done;
}

// The loop with one group body under a per-group flag, as the lean kernels ran it before the run
// length: group(s, checked) is one group of depth steps; unchecked it ends with s.advance(). Kept for
// the lean configurations whose registers do not hold two unrolled bodies (lean_two_bodies in
// linear_wave_impl.h). Same sequence of groups as wave_loop_run: a group is checked iff !s.fits().
template <class Group, class Tail>
PTDT_HD inline int wave_loop_run_flagged(WaveLoopSchedule& s, int n, Group&& group, Tail&& tail) {
  const int nfull = n - n % s.depth;
  int done = 0;
  bool go = true;
  while (done < nfull && go) {
    go = group(s, !s.fits());
    done += s.depth;
  }
  if (go && done < n) done += tail(s, n - done);
  return done;
}

// Host enumeration of a launch's reads (entry offset, barrier in front) and ring slots through the
// same functions, the way the kernel uses them: a running read offset and a running ring slot that
// only a checked read / slot resets, so a run length or an advance(r) that leaves the schedule's
// state behind the running addresses shows in what is returned. Returns the number of reads, or -1
// if a capacity is too small.
inline int wave_loop_enumerate(int S, int B, int estride, int e0, int j0, int n, int depth, int ring, int* ofs,
                               unsigned char* bar, int cap_reads, int* slots, int cap_slots, int* barriers_out) {
  WaveLoopSchedule s;
  s.init(S, B, estride, e0, j0, n, depth, ring);
  int nr = 0, nsl = 0;
  int lp = 0, rp = 0;  // running entry offset of the next read, running ring slot of the next step
  auto read = [&](bool b) {
    if (nr < cap_reads) {
      ofs[nr] = lp;
      bar[nr] = b ? 1 : 0;
    }
    ++nr;
    lp += B;
  };
  auto use_slot = [&]() {
    if (nsl < cap_slots) slots[nsl] = rp;
    ++nsl;
    ++rp;
  };
  auto checked = [&](WaveLoopSchedule& c) {
    bool b, sw;
    const int o = c.next(&b, &sw);
    if (sw) lp = o;
    read(b);
  };
  lp = s.first();
  read(false);
  for (int u = 0; u < depth; ++u) checked(s);
  wave_loop_run(
      s, n,
      [&]() {
        for (int k = 0; k < depth; ++k) {
          use_slot();
          read(false);
        }
        return true;
      },
      [&](WaveLoopSchedule& c) {
        for (int k = 0; k < c.depth; ++k) {
          use_slot();
          checked(c);
          if (c.slot_done()) rp = 0;
        }
        return true;
      },
      [&](WaveLoopSchedule& c, int left) {
        for (int k = 0; k < left; ++k) {
          use_slot();
          if (c.slot_done()) rp = 0;
        }
        return left;
      });
  *barriers_out = s.barriers;
  return (nr <= cap_reads && nsl <= cap_slots) ? nr : -1;
}

// Host check of run() and advance(r) over one launch, against the per-group rule: the launch is
// walked one group at a time (fits() ? advance() : `depth` checked reads and slots), and in front of
// every group run(groups left) must be the number of times fits() / advance() can be repeated from
// there, and advance(that many) must leave the state those repeats leave. Returns the number of
// group boundaries checked, or -1 - (index of the first one that differs).
inline long wave_loop_check_runs(int S, int B, int estride, int e0, int j0, int n, int depth, int ring) {
  WaveLoopSchedule s;
  s.init(S, B, estride, e0, j0, n, depth, ring);
  bool b, sw;
  s.first();
  for (int u = 0; u < depth; ++u) s.next(&b, &sw);
  long checked = 0;
  for (int left = n / depth; left > 0; --left) {
    WaveLoopSchedule rep = s, adv = s;
    int ref = 0;
    while (ref < left && rep.fits()) {
      rep.advance();
      ++ref;
    }
    adv.advance(ref);
    if (s.run(left) != ref || adv.ij != rep.ij || adv.par != rep.par || adv.lofs != rep.lofs ||
        adv.barriers != rep.barriers || adv.rslot != rep.rslot)
      return -1 - checked;
    ++checked;
    if (s.fits()) {
      s.advance();
    } else {
      for (int k = 0; k < depth; ++k) {
        s.next(&b, &sw);
        s.slot_done();
      }
    }
  }
  return checked;
}

}  // namespace ptdt
