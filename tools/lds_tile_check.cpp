// Stand-alone host check of the LDS tile arithmetic (csrc/kernels/lds_tile.h): the bank swizzle, the
// staging loop's chunk map against the fragment read's offset, and the channel map of the paired
// MFMA tiles. Meant to be built with sanitizers and run on a CPU (tests/test_lds_tile.py does):
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Icsrc \
//       tools/lds_tile_check.cpp -o lds_tile_check && ./lds_tile_check
//
// For rows of 128, 256 and 512 bytes:
//   (a) swz is an involution on the chunks of every row;
//   (b) for every chunk, the 16 rows from any multiple of 16 land in 16 distinct 16-byte slots of the
//       256-byte bank row -- the conflict-free claim of the header;
//   (c) for every (ROWS, ROW_BYTES, THREADS) the kernels instantiate: the image written by the staging
//       loop (round i, thread t -> linear chunk i * THREADS + t <- source chunk staged_chunk: stage_rows,
//       and the loops the streaming and the 8-phase kernel keep on the same map) read back at
//       tile_off(row, chunk) returns every source chunk exactly once. The image is a heap array of
//       exactly the tile's chunks, so an offset past it is an overflow the sanitizer reports;
//   (d) pair_channel maps the 2 x 16 rows of a tile pair onto the 32 channels of the pair, one to one.
#include <cstdio>
#include <cstdlib>

#include "kernels/lds_tile.h"

namespace {

long failures = 0, checks = 0;

void expect(bool ok, const char* what, int row_bytes, int a, int b) {
  ++checks;
  if (ok) return;
  ++failures;
  std::fprintf(stderr, "FAIL %s: row bytes %d at (%d, %d)\n", what, row_bytes, a, b);
}

template <int RB>
void check_swizzle() {
  constexpr int CPR = RB / 16;
  for (int r = 0; r < 1024; ++r)
    for (int c = 0; c < CPR; ++c) {
      const int s = ptdt::swz<RB>(r, c);
      expect(s >= 0 && s < CPR, "slot in the row", RB, r, c);
      expect(ptdt::swz<RB>(r, s) == c, "involution", RB, r, c);
      expect(ptdt::tile_off<RB>(r, c) == r * RB + s * 16, "tile_off", RB, r, c);
    }
  for (int r0 = 0; r0 < 1024; r0 += 16)
    for (int c = 0; c < CPR; ++c) {
      unsigned seen = 0;  // 16-byte slots of the 256-byte bank row
      for (int r = r0; r < r0 + 16; ++r) seen |= 1u << (ptdt::tile_off<RB>(r, c) % 256 / 16);
      expect(seen == 0xffffu, "16 rows on 16 distinct slots", RB, r0, c);
    }
}

template <int ROWS, int RB, int THREADS>
void check_stage() {
  constexpr int CPR = RB / 16, CHUNKS = ROWS * CPR;
  int* image = (int*)std::malloc(sizeof(int) * CHUNKS);  // source chunk id held by each 16 B of the LDS image
  for (int p = 0; p < CHUNKS; ++p) image[p] = -1;
  for (int i = 0; i < ptdt::stage_rounds<ROWS, RB, THREADS>(); ++i)
    for (int t = 0; t < THREADS; ++t) {
      const int p = i * THREADS + t;
      const ptdt::TileChunk s = ptdt::staged_chunk<RB>(p);
      expect(s.r >= 0 && s.r < ROWS && s.c >= 0 && s.c < CPR, "staged chunk in the tile", RB, ROWS, p);
      expect(image[p] == -1, "image chunk written once", RB, ROWS, p);
      image[p] = s.r * CPR + s.c;
    }
  int* times = (int*)std::calloc(CHUNKS, sizeof(int));
  for (int r = 0; r < ROWS; ++r)
    for (int c = 0; c < CPR; ++c) {
      const int off = ptdt::tile_off<RB>(r, c);
      expect(off % 16 == 0, "aligned offset", RB, r, c);
      const int got = image[off / 16];
      expect(got == r * CPR + c, "read returns the staged chunk", RB, r, c);
      if (got >= 0 && got < CHUNKS) ++times[got];
    }
  for (int id = 0; id < CHUNKS; ++id) expect(times[id] == 1, "every source chunk exactly once", RB, ROWS, id);
  std::free(times);
  std::free(image);
}

void check_pair_channel() {
  for (int p = 0; p < 8; ++p) {
    unsigned seen = 0;
    for (int h = 0; h < 2; ++h)
      for (int i = 0; i < 16; ++i) {
        const int ch = ptdt::pair_channel(2 * p + h, i);
        expect(ch >= 32 * p && ch < 32 * p + 32, "channel in the pair", 0, 2 * p + h, i);
        seen |= 1u << (ch & 31);
        // lane group q = i / 4 holds 8 consecutive channels over its two tiles
        expect(ch == 32 * p + 8 * (i / 4) + 4 * h + i % 4, "8 consecutive channels per lane group", 0, 2 * p + h, i);
      }
    expect(seen == 0xffffffffu, "bijection on the pair's 32 channels", 0, p, 0);
  }
}

}  // namespace

int main() {
  check_swizzle<128>();
  check_swizzle<256>();
  check_swizzle<512>();
  // gemm_big.hip (bf16, BK = 64) and int8_mm.hip (BKB = 128): 128-byte rows
  check_stage<256, 128, 512>();  // 256x256 tiles, 8 waves
  check_stage<128, 128, 256>();  // 128x128 tiles, 4 waves
  check_stage<128, 128, 512>();  // the piece ring's pieces, the 8-phase quarters; conv1x1_bn K = 64, 8 waves
  // conv1x1_bn.hip: 16 rows per wave, 4 or 8 waves, K = 64, 128, 256
  check_stage<64, 128, 256>();
  check_stage<64, 256, 256>();
  check_stage<128, 256, 512>();
  check_stage<64, 512, 256>();
  check_stage<128, 512, 512>();
  check_pair_channel();
  if (failures) {
    std::fprintf(stderr, "lds tile: %ld of %ld checks failed\n", failures, checks);
    return 1;
  }
  std::printf("lds tile: %ld checks ok\n", checks);
  return 0;
}
