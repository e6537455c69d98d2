// Stand-alone host model of the two column-sum trees of the wave engine's hand-placed step
// (csrc/kernels/linear_wave_impl.h): the all-reduce of row16_sum_n<6> / hand_step_2x5 (24 DPP adds,
// every lane of a 16-lane row ends with every total) and the reduce-scatter of hand_step_2x5_rs (13
// adds, each total in one bank, read back from lane kHsBcast[k] by row_newbcast). Every add is modelled
// as the instruction is written: src0 is the DPP operand (the other lane's value), src1 the lane's own.
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       tools/wave_colsum_order_check.cpp -o wave_colsum_order_check && ./wave_colsum_order_check [rows]
//
// 1. Finite rows: for `rows` (default 10^6) random rows of six values the broadcast total of the scattered tree has the
//    bits of the all-reduce in each of the 16 lanes (the pairs of every stage are the same and a finite
//    add commutes). Exit status 1 otherwise.
// 2. NaN rows: an add of two NaNs returns one of them, and which one depends on the operand order. The
//    report lists, for each value and for both rules (src0's NaN first, src1's NaN first), the leaf whose
//    NaN each lane of the all-reduce ends with when all sixteen leaves are different NaNs, and the leaf
//    the scattered tree hands to the row. The all-reduce gives sixteen lanes sixteen different answers
//    (lane i: leaf i + 1 or leaf i); the scattered tree gives the row one. They agree where at most one
//    leaf of a column is a NaN, or all NaN leaves have the same bits.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>

namespace {

constexpr int kHsBcast[6] = {0, 10, 4, 12, 0, 10};  // linear_wave_impl.h

uint32_t bits(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  return u;
}
float from_bits(uint32_t u) {
  float f;
  std::memcpy(&f, &u, 4);
  return f;
}
bool is_nan(float f) { return f != f; }

int g_rule = 0;  // 0: the first NaN operand (src0, then src1) comes out quieted; 1: src1, then src0
float add(float src0, float src1) {
  const float a = g_rule == 0 ? src0 : src1, b = g_rule == 0 ? src1 : src0;
  if (is_nan(a)) return from_bits(bits(a) | 0x00400000u);
  if (is_nan(b)) return from_bits(bits(b) | 0x00400000u);
  return src0 + src1;
}

using Row = float[16];

// v_add_f32_dpp dst, src, src CTRL bank_mask: lane i of an enabled bank gets add(src[from(i)], src[i])
template <class From>
void dpp_add(Row& dst, const Row& src, From from, unsigned bank_mask) {
  Row out;
  for (int i = 0; i < 16; ++i) out[i] = dst[i];
  for (int i = 0; i < 16; ++i) {
    const int j = from(i);
    if (!((bank_mask >> (i >> 2)) & 1u) || j < 0 || j > 15) continue;
    out[i] = add(src[j], src[i]);
  }
  for (int i = 0; i < 16; ++i) dst[i] = out[i];
}
auto ror(int n) {
  return [n](int i) { return (i - n) & 15; };
}
auto shl(int n) {
  return [n](int i) { return i + n; };
}
auto shr(int n) {
  return [n](int i) { return i - n; };
}
auto qxor(int n) {
  return [n](int i) { return i ^ n; };
}

// row16_sum_n: v += ror(v) for 8, 4, 2, 1, all lanes
void all_reduce(Row (&v)[6]) {
  for (int n : {8, 4, 2, 1})
    for (int k = 0; k < 6; ++k) dpp_add(v[k], v[k], ror(n), 0xf);
}

// hand_step_2x5_rs; returns the six totals as the row reads them (lane kHsBcast[k] of gx / gy)
void reduce_scatter(Row (&v)[6], float (&total)[6]) {
  for (int p = 0; p < 3; ++p) {  // stage 1: AB, CD, EF in v[0], v[2], v[4]
    dpp_add(v[2 * p], v[2 * p], ror(8), 0x3);
    dpp_add(v[2 * p], v[2 * p + 1], ror(8), 0xc);
  }
  dpp_add(v[0], v[0], shl(4), 0x5);  // stage 2: gx = v[0], gy = v[4]
  dpp_add(v[0], v[2], shr(4), 0xa);
  dpp_add(v[4], v[4], shl(4), 0x5);
  for (int n : {2, 1}) {  // stages 3, 4
    dpp_add(v[0], v[0], qxor(n), 0xf);
    dpp_add(v[4], v[4], qxor(n), 0xf);
  }
  for (int k = 0; k < 6; ++k) total[k] = v[k < 4 ? 0 : 4][kHsBcast[k]];
}

int check_finite(int rows) {
  std::mt19937 rng(12345);
  std::normal_distribution<float> nd(0.f, 1.f);
  std::uniform_int_distribution<int> ex(-20, 20);
  for (int it = 0; it < rows; ++it) {
    Row a[6], b[6];
    for (int k = 0; k < 6; ++k)
      for (int i = 0; i < 16; ++i) a[k][i] = b[k][i] = std::ldexp(nd(rng), (it & 1) ? ex(rng) : 0);
    float total[6];
    all_reduce(a);
    reduce_scatter(b, total);
    for (int k = 0; k < 6; ++k)
      for (int i = 0; i < 16; ++i)
        if (bits(a[k][i]) != bits(total[k])) {
          std::fprintf(stderr, "FAIL finite: row %d value %d lane %d: all-reduce %08x, scattered %08x\n", it, k, i,
                       bits(a[k][i]), bits(total[k]));
          return 1;
        }
  }
  std::printf("finite: %d rows x 6 values x 16 lanes, the scattered total has the all-reduce's bits\n", rows);
  return 0;
}

// all sixteen leaves different NaNs (payload = leaf + 1): the payload that comes out names the leaf
void report_nan() {
  for (g_rule = 0; g_rule < 2; ++g_rule) {
    Row a[6], b[6];
    for (int k = 0; k < 6; ++k)
      for (int i = 0; i < 16; ++i) a[k][i] = b[k][i] = from_bits(0x7FC00000u | (uint32_t)(i + 1));
    float total[6];
    all_reduce(a);
    reduce_scatter(b, total);
    std::printf("rule %s: all-reduce lane i ends with leaf", g_rule == 0 ? "src0 first" : "src1 first");
    for (int i = 0; i < 16; ++i) std::printf(" %d", (int)(bits(a[0][i]) & 0xffff) - 1);
    std::printf("\n  scattered tree, value k read from lane kHsBcast[k]: leaf");
    for (int k = 0; k < 6; ++k) std::printf(" %d", (int)(bits(total[k]) & 0xffff) - 1);
    std::printf("\n");
  }
  g_rule = 0;
}

// one NaN leaf among finite ones, and sixteen NaN leaves of the same bits: both trees agree in every lane
int check_single_nan() {
  for (g_rule = 0; g_rule < 2; ++g_rule)
    for (int pattern = 0; pattern < 2; ++pattern)
      for (int leaf = 0; leaf < 16; ++leaf) {
        Row a[6], b[6];
        for (int k = 0; k < 6; ++k)
          for (int i = 0; i < 16; ++i)
            a[k][i] = b[k][i] = pattern == 0 ? (i == leaf ? from_bits(0xFFC00000u | (uint32_t)(k + 1)) : 0.25f * (float)(i + k))
                                             : from_bits(0x7FC00000u | (uint32_t)(leaf + 1));
        float total[6];
        all_reduce(a);
        reduce_scatter(b, total);
        for (int k = 0; k < 6; ++k)
          for (int i = 0; i < 16; ++i)
            if (bits(a[k][i]) != bits(total[k])) {
              std::fprintf(stderr, "FAIL nan pattern %d leaf %d value %d lane %d\n", pattern, leaf, k, i);
              return 1;
            }
      }
  g_rule = 0;
  std::printf("one NaN leaf per column, or sixteen equal NaN leaves: the same bits in every lane, both rules\n");
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (check_finite(argc > 1 ? std::atoi(argv[1]) : 1000000)) return 1;
  if (check_single_nan()) return 1;
  report_nan();
  return 0;
}
