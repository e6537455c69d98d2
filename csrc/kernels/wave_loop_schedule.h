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
// only advance a running address, with no wrap test and no barrier test. Any other group runs the
// same body with a checked read after every step (list switch, barrier) and a checked ring slot.
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
  PTDT_HD void advance() {
    ij += depth;
    lofs += depth * B;
    rslot += depth;
  }
};

// The loop itself, after the prologue's 1 + depth reads (first(), then `depth` checked ones).
// group(s, checked): one group of depth steps, each followed by a read. Unchecked: step k reads at
//   s.lofs + k * B and uses ring slot s.rslot + k (running addresses in the kernel), then
//   s.advance(). Checked: every step is followed by s.next() and s.slot_done().
// tail(s, left): the last left < depth steps, no reads, s.slot_done() after each; returns the steps done.
// group returns false to end the launch after it. Returns the steps done.
template <class Group, class Tail>
PTDT_HD inline int wave_loop_run(WaveLoopSchedule& s, int n, Group&& group, Tail&& tail) {
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
// same functions. Returns the number of reads, or -1 if a capacity is too small.
inline int wave_loop_enumerate(int S, int B, int estride, int e0, int j0, int n, int depth, int ring, int* ofs,
                               unsigned char* bar, int cap_reads, int* slots, int cap_slots, int* barriers_out) {
  WaveLoopSchedule s;
  s.init(S, B, estride, e0, j0, n, depth, ring);
  int nr = 0, nsl = 0;
  auto read = [&](int o, bool b) {
    if (nr < cap_reads) {
      ofs[nr] = o;
      bar[nr] = b ? 1 : 0;
    }
    ++nr;
  };
  auto use_slot = [&](int sl) {
    if (nsl < cap_slots) slots[nsl] = sl;
    ++nsl;
  };
  auto checked = [&](WaveLoopSchedule& c) {
    bool b, sw;
    const int o = c.next(&b, &sw);
    read(o, b);
  };
  read(s.first(), false);
  for (int u = 0; u < depth; ++u) checked(s);
  wave_loop_run(
      s, n,
      [&](WaveLoopSchedule& c, bool chk) {
        for (int k = 0; k < c.depth; ++k) {
          if (chk) {
            use_slot(c.rslot);
            checked(c);
            c.slot_done();
          } else {
            use_slot(c.rslot + k);
            read(c.lofs + k * c.B, false);
          }
        }
        if (!chk) c.advance();
        return true;
      },
      [&](WaveLoopSchedule& c, int left) {
        for (int k = 0; k < left; ++k) {
          use_slot(c.rslot);
          c.slot_done();
        }
        return left;
      });
  *barriers_out = s.barriers;
  return (nr <= cap_reads && nsl <= cap_slots) ? nr : -1;
}

}  // namespace ptdt
