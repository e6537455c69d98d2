// Stand-alone host check of the lean wave loop's run length (csrc/kernels/wave_loop_schedule.h):
// WaveLoopSchedule::run() and advance(r) against repeated fits() / advance(), at every group
// boundary of every launch, and the launch's reads and ring slots through wave_loop_enumerate with
// exactly sized output arrays. Meant to be built with sanitizers and run on a CPU
// (tests/test_wave_loop_runs.py does):
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Icsrc \
//       tools/wave_loop_runs_check.cpp -o wave_loop_runs_check && ./wave_loop_runs_check
//
// Ranges: S in 1..70, j0 in 0..S-1, depth 2, 3, 4, ring = 2 S + depth, n in 0..3 ring (B = 32).
// The enumeration runs for a thinned set of these (every launch length for S <= 12 and S == 64, else
// the lengths around a multiple of the epoch and of the ring), its arrays sized exactly: a run that
// is a group too long makes a read or a step too many, a heap overflow the sanitizer reports.
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

#include "kernels/wave_loop_schedule.h"

namespace {

int list_stride(int num_samples, int B) { return (((num_samples + B - 1) / B) * B + 64 + 3) & ~3; }  // wave_list_stride

int fail(const char* what, int S, int j0, int n, int depth, long k) {
  std::fprintf(stderr, "FAIL %s: S=%d j0=%d n=%d depth=%d at %ld\n", what, S, j0, n, depth, k);
  return 1;
}

// reads and slots of one launch: offsets by the per-step rule, slots k % ring
int enumerate(int S, int B, int estride, int j0, int n, int depth, int ring) {
  const int reads = 1 + depth + n - n % depth;
  int* ofs = (int*)std::malloc(sizeof(int) * reads);
  unsigned char* bar = (unsigned char*)std::malloc(reads);
  int* slots = (int*)std::malloc(sizeof(int) * (n > 0 ? n : 1));
  int barriers = -1;
  const int nr = ptdt::wave_loop_enumerate(S, B, estride, 0, j0, n, depth, ring, ofs, bar, reads, slots, n, &barriers);
  int rc = nr != reads ? fail("number of reads", S, j0, n, depth, nr) : 0;
  int ij = j0, par = 0, lofs = j0 * B;
  for (int r = 0; !rc && r < reads; ++r) {
    if (ofs[r] != lofs) rc = fail("offset", S, j0, n, depth, r);
    lofs += B;
    if (++ij == S) {
      ij = 0;
      par ^= 1;
      lofs = par * estride;
    }
  }
  for (int k = 0; !rc && k < n; ++k)
    if (slots[k] != k % ring) rc = fail("ring slot", S, j0, n, depth, k);
  std::free(ofs);
  std::free(bar);
  std::free(slots);
  return rc;
}

}  // namespace

int main() {
  const int B = 32;
  long launches = 0, boundaries = 0, enumerated = 0;
  for (int depth : {3, 2, 4})
    for (int S = 1; S <= 70; ++S) {
      const int estride = list_stride(S * B, B), ring = 2 * S + depth;
      for (int j0 = 0; j0 < S; ++j0)
        for (int n = 0; n <= 3 * ring; ++n) {
          const long c = ptdt::wave_loop_check_runs(S, B, estride, 0, j0, n, depth, ring);
          if (c < 0) return fail("run length / advance(r)", S, j0, n, depth, -1 - c);
          ++launches;
          boundaries += c;
          const bool near = n % S <= depth || n % S >= S - depth || n % ring <= depth || n % ring >= ring - depth;
          if (S <= 12 || S == 64 ? true : near) {
            if (enumerate(S, B, estride, j0, n, depth, ring)) return 1;
            ++enumerated;
          }
        }
    }
  std::printf("wave loop runs: %ld launches, %ld group boundaries, %ld enumerated ok\n", launches, boundaries, enumerated);
  return 0;
}
