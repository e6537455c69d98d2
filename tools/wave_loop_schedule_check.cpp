// Stand-alone host check of the lean wave loop's control (csrc/kernels/wave_loop_schedule.h) against
// the per-step rule of the generic kernel's read_index, written out below. Meant to be built with
// sanitizers and run on a CPU (tests/test_wave_loop_schedule.py does):
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Icsrc \
//       tools/wave_loop_schedule_check.cpp -o wave_loop_schedule_check && ./wave_loop_schedule_check
//
// Ranges: S in 1..8, j0 in 0..S-1, n in 0..40, both list parities, B = 16 / 32 / 64, depth 3 (and 2, 4).
// The output arrays are sized exactly (reads = 1 + depth + n - n % depth, slots = n), so a schedule
// that makes one read or one step too many is a heap overflow the sanitizer reports.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "kernels/wave_loop_schedule.h"

namespace {

int list_stride(int num_samples, int B) { return (((num_samples + B - 1) / B) * B + 64 + 3) & ~3; }  // wave_list_stride

int fail(const char* what, int S, int B, int e0, int j0, int n, int depth, int k) {
  std::fprintf(stderr, "FAIL %s: S=%d B=%d e0=%d j0=%d n=%d depth=%d at %d\n", what, S, B, e0, j0, n, depth, k);
  return 1;
}

int check(int S, int B, int e0, int j0, int n, int depth) {
  const int estride = list_stride(S * B, B), ring = 2 * S + depth;
  const int T = (j0 + n - 1) / S, reads = 1 + depth + n - n % depth;
  // the per-step rule
  std::vector<int> ofs_ref(reads);
  std::vector<unsigned char> bar_ref(reads);
  {
    int ie = e0, ij = j0, barriers = 0, lofs = (ie & 1) * estride + ij * B;
    bool bar_due = false;
    for (int r = 0; r < reads; ++r) {
      bar_ref[r] = bar_due ? 1 : 0;
      if (bar_due) {
        ++barriers;
        bar_due = false;
      }
      ofs_ref[r] = lofs;
      lofs += B;
      if (++ij == S) {
        ij = 0;
        ++ie;
        lofs = (ie & 1) * estride;
        bar_due = barriers < T;
      }
    }
    // (n == 0 at j0 == 0 gives T == -1 for S == 1: no barrier, like T == 0)
    if (barriers != (T > 0 ? T : 0)) return fail("rule: barriers != T", S, B, e0, j0, n, depth, barriers);
  }
  int* ofs = (int*)std::malloc(sizeof(int) * reads);  // exact sizes: see the header comment
  unsigned char* bar = (unsigned char*)std::malloc(reads);
  int* slots = (int*)std::malloc(sizeof(int) * (n > 0 ? n : 1));
  int barriers = -1;
  const int nr = ptdt::wave_loop_enumerate(S, B, estride, e0, j0, n, depth, ring, ofs, bar, reads, slots, n, &barriers);
  int rc = 0;
  if (nr != reads) rc = fail("number of reads", S, B, e0, j0, n, depth, nr);
  if (!rc && barriers != (T > 0 ? T : 0)) rc = fail("barriers != T", S, B, e0, j0, n, depth, barriers);
  for (int r = 0; !rc && r < reads; ++r) {
    if (ofs[r] != ofs_ref[r]) rc = fail("offset", S, B, e0, j0, n, depth, r);
    else if (bar[r] != bar_ref[r]) rc = fail("barrier position", S, B, e0, j0, n, depth, r);
    const int rel = ofs[r] % estride;  // inside one padded list, with the 64 row slots a read may touch
    if (!rc && (ofs[r] < 0 || ofs[r] >= 2 * estride || rel + 64 > estride)) rc = fail("offset range", S, B, e0, j0, n, depth, r);
  }
  for (int k = 0; !rc && k < n; ++k)
    if (slots[k] != k % ring) rc = fail("ring slot", S, B, e0, j0, n, depth, k);
  std::free(ofs);
  std::free(bar);
  std::free(slots);
  return rc;
}

}  // namespace

int main() {
  long cases = 0;
  for (int depth : {3, 2, 4})
    for (int B : {16, 32, 64})
      for (int S = 1; S <= 8; ++S)
        for (int j0 = 0; j0 < S; ++j0)
          for (int e0 = 0; e0 < 2; ++e0)
            for (int n = 0; n <= 40; ++n) {
              if (check(S, B, e0, j0, n, depth)) return 1;
              ++cases;
            }
  std::printf("wave loop schedule: %ld cases ok\n", cases);
  return 0;
}
