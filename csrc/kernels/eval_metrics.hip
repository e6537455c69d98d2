// Evaluation metrics (gfx950): per-row cross-entropy and the rank of the target among the logits
// in one pass, and the fixed-order accumulation of both into a device-resident meter.
//
//   rows       : z_y is loaded first (one broadcast load), then every logit of the row is read
//                once. A thread keeps a running maximum m, the rescaled sum s of exp(z - m) (online
//                softmax), the count of z_c > z_y and the count of z_c == z_y with c < y. The rank
//                #greater + #equal-before is the target's position in a stable descending sort, so
//                "rank < k" is top-k correctness for every k at once. row_loss = m + log(s) - z_y.
//   accumulate : one workgroup adds the rows' results to int64 counters and a float64 loss sum.
//
// Geometry, from C alone: rows of C <= kWaveRowMaxC (2048) take one wave each, four rows per
// 256-thread workgroup (at most 32 (fp32) or 16 (bf16) 16-byte groups per lane); longer rows take
// one 1024-thread workgroup each, so that a [64, 32000] batch still has every load of a row in
// flight after a few rounds. A thread owns the same 16-byte groups of the row (group g belongs to
// thread g mod NT, folded in ascending g) whether it reaches them with one 16-byte load (row
// pointer 16-byte aligned and C a multiple of the group) or element by element, and the partial
// states are merged lane-butterfly then wave 0..n-1: a row's results are a function of its contents
// and C, never of B, of the row's position or of its alignment. No atomics, no memsets, no host
// reads, no allocation: every launch is hipGraph-capturable.
//
// -inf: while a running maximum is still -inf its sum holds only exp(-inf) = 0 terms (or a NaN), so
// the rescale factor is taken as 1 and exponents are formed against 0 instead of against -inf; rows
// with masked (-inf) classes give the exact finite result, all--inf rows give lse = -inf. NaNs never
// raise the maximum (fmaxf) or count as greater, and reach the loss through the sum.
#include "common.h"
#include "kernels.h"
#include "vec16.h"

namespace ptdt {
namespace {

constexpr int kWaveRowMaxC = 2048;            // longest row scanned by one wave
constexpr int kRowBlock = 256;                // wave-per-row kernel
constexpr int kRowsPerBlock = kRowBlock / 64;
constexpr int kBigBlock = 1024;               // workgroup-per-row kernel
constexpr int kUnroll = 4;                    // 16-byte loads issued before the first is used
constexpr int kAccBlock = 256;
static_assert(kRowsPerBlock == kEvalRowsPerBlock, "kernels.h states the rows per workgroup");
static_assert(kWaveRowMaxC == kEvalWaveRowMaxC, "kernels.h states the geometry threshold");

struct RowState {
  float m;  // maximum of the non-NaN logits seen
  float s;  // sum of exp(z - m) over the logits seen (against 0 while m is -inf)
  int gt;   // logits greater than the target's
  int eq;   // logits equal to the target's at a smaller class index
};

// the V logits of group [c0, c0 + V) into the state; positions past the row hold -inf
template <int V>
__device__ __forceinline__ void fold_group(RowState& st, const float* f, int c0, float zy, int y) {
  float cm = -INFINITY;
#pragma unroll
  for (int e = 0; e < V; ++e) cm = fmaxf(cm, f[e]);
  if (cm > st.m) {
    st.s *= st.m == -INFINITY ? 1.f : expf(st.m - cm);
    st.m = cm;
  }
  const float ms = st.m == -INFINITY ? 0.f : st.m;
#pragma unroll
  for (int e = 0; e < V; ++e) {
    st.s += expf(f[e] - ms);
    st.gt += f[e] > zy ? 1 : 0;
    st.eq += (f[e] == zy && c0 + e < y) ? 1 : 0;
  }
}

__device__ __forceinline__ RowState merge(const RowState& a, const RowState& b) {
#pragma clang fp contract(off)
  RowState r;
  r.m = fmaxf(a.m, b.m);
  const float fa = a.m == -INFINITY ? 1.f : expf(a.m - r.m);
  const float fb = b.m == -INFINITY ? 1.f : expf(b.m - r.m);
  r.s = a.s * fa + b.s * fb;
  r.gt = a.gt + b.gt;
  r.eq = a.eq + b.eq;
  return r;
}

__device__ __forceinline__ RowState wave_merge(RowState st) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    RowState o;
    o.m = __shfl_xor(st.m, off);
    o.s = __shfl_xor(st.s, off);
    o.gt = __shfl_xor(st.gt, off);
    o.eq = __shfl_xor(st.eq, off);
    st = merge(st, o);
  }
  return st;
}

// thread t of NT scans its groups of one row
template <typename T, int NT, bool VEC>
__device__ __forceinline__ RowState scan_row(const T* __restrict__ z, int C, int t, float zy, int y) {
  constexpr int V = Vec16<T>::N;
  const int G = (C + V - 1) / V;
  RowState st{-INFINITY, 0.f, 0, 0};
  if constexpr (VEC) {
    const u32x4* zv = reinterpret_cast<const u32x4*>(z);
    for (int g = t; g < G; g += NT * kUnroll) {
      u32x4 w[kUnroll];
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) w[u] = zv[min(g + u * NT, G - 1)];  // always a group of this row
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        const int gu = g + u * NT;
        if (gu < G) {
          float f[V];
          Vec16<T>::unpack(w[u], f);
          fold_group<V>(st, f, gu * V, zy, y);
        }
      }
    }
  } else {
    for (int g = t; g < G; g += NT) {
      float f[V];
#pragma unroll
      for (int e = 0; e < V; ++e) {
        const int c = g * V + e;
        const float v = Cvt<T>::load(z, min(c, C - 1));  // always a load: the group's V loads issue together
        f[e] = c < C ? v : -INFINITY;
      }
      fold_group<V>(st, f, g * V, zy, y);
    }
  }
  return st;
}

// Row b by the NT threads of a wave (NT == 64) or of the workgroup. False: the row has no scan
// (ignored or bad target, already written); uniform over the NT threads.
template <typename T, int NT>
__device__ __forceinline__ bool row_partial(const T* __restrict__ logits, int64_t ld,
                                            const int64_t* __restrict__ target, int b, int C, int64_t ignore_index,
                                            int t, float* __restrict__ row_loss, int32_t* __restrict__ rank,
                                            RowState& st, float& zy) {
  const int64_t y = target[b];
  if (y == ignore_index || y < 0 || y >= C) {  // z + y is never formed
    if (t == 0) {
      row_loss[b] = 0.f;
      rank[b] = y == ignore_index ? -1 : -2;
    }
    return false;
  }
  const T* z = logits + (int64_t)b * ld;
  zy = Cvt<T>::load(z, y);
  const bool vec = (reinterpret_cast<uintptr_t>(z) & 15) == 0 && C % Vec16<T>::N == 0;
  st = vec ? scan_row<T, NT, true>(z, C, t, zy, (int)y) : scan_row<T, NT, false>(z, C, t, zy, (int)y);
  st = wave_merge(st);
  return true;
}

__device__ __forceinline__ void row_store(const RowState& st, float zy, int b, int C, float* __restrict__ row_loss,
                                          int32_t* __restrict__ rank) {
  const float lse = st.m + logf(st.s);
  row_loss[b] = lse - zy;
  rank[b] = zy != zy ? C : st.gt + st.eq;
}

template <typename T>
__global__ void __launch_bounds__(kRowBlock) eval_rows_wave_kernel(const T* __restrict__ logits, int64_t ld,
                                                                   const int64_t* __restrict__ target, int B, int C,
                                                                   int64_t ignore_index, float* __restrict__ row_loss,
                                                                   int32_t* __restrict__ rank) {
  const int b = blockIdx.x * kRowsPerBlock + (threadIdx.x >> 6);
  if (b >= B) return;  // wave-uniform
  const int lane = threadIdx.x & 63;
  RowState st;
  float zy;
  if (!row_partial<T, 64>(logits, ld, target, b, C, ignore_index, lane, row_loss, rank, st, zy)) return;
  if (lane == 0) row_store(st, zy, b, C, row_loss, rank);
}

template <typename T>
__global__ void __launch_bounds__(kBigBlock) eval_rows_block_kernel(const T* __restrict__ logits, int64_t ld,
                                                                    const int64_t* __restrict__ target, int B, int C,
                                                                    int64_t ignore_index, float* __restrict__ row_loss,
                                                                    int32_t* __restrict__ rank) {
  __shared__ RowState parts[kBigBlock / 64];
  const int b = blockIdx.x;
  RowState st;
  float zy;
  if (!row_partial<T, kBigBlock>(logits, ld, target, b, C, ignore_index, threadIdx.x, row_loss, rank, st, zy))
    return;  // block-uniform
  if ((threadIdx.x & 63) == 0) parts[threadIdx.x >> 6] = st;
  __syncthreads();
  if (threadIdx.x == 0) {
    st = parts[0];
    for (int w = 1; w < kBigBlock / 64; ++w) st = merge(st, parts[w]);
    row_store(st, zy, b, C, row_loss, rank);
  }
}

// counters: rows, valid, ignored, bad_target, nonfinite, correct[k_0 .. k_{n-1}]
__global__ void __launch_bounds__(kAccBlock) eval_accumulate_kernel(const float* __restrict__ row_loss,
                                                                    const int32_t* __restrict__ rank, int B,
                                                                    EvalTopK ks, int64_t* __restrict__ counters,
                                                                    double* __restrict__ loss_sum) {
  constexpr int kCnt = 4 + kEvalMaxK;  // valid, ignored, bad_target, nonfinite, correct[]
  constexpr int kWaves = kAccBlock / 64;
  __shared__ int scnt[kWaves][kCnt];
  __shared__ double ssum[kWaves];
  int cnt[kCnt];
#pragma unroll
  for (int i = 0; i < kCnt; ++i) cnt[i] = 0;
  double sum = 0.0;
  for (int b = threadIdx.x; b < B; b += kAccBlock) {
    const int r = rank[b];
    const float l = row_loss[b];
    const bool valid = r >= 0;
    const bool finite = fabsf(l) < INFINITY;  // false for NaN
    cnt[0] += valid ? 1 : 0;
    cnt[1] += r == -1 ? 1 : 0;
    cnt[2] += r == -2 ? 1 : 0;
    cnt[3] += (valid && !finite) ? 1 : 0;
    if (valid && finite) sum += (double)l;
#pragma unroll
    for (int i = 0; i < kEvalMaxK; ++i) cnt[4 + i] += (i < ks.n && valid && r < ks.k[i]) ? 1 : 0;
  }
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
#pragma unroll
    for (int i = 0; i < kCnt; ++i) cnt[i] += __shfl_xor(cnt[i], off);
    sum += __shfl_xor(sum, off);
  }
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < kCnt; ++i) scnt[wid][i] = cnt[i];
    ssum[wid] = sum;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kWaves; ++w) sum += ssum[w];
    *loss_sum += sum;
    counters[0] += B;
    for (int i = 0; i < 4 + ks.n; ++i) {
      int64_t c = 0;
      for (int w = 0; w < kWaves; ++w) c += scnt[w][i];
      counters[1 + i] += c;
    }
  }
}

}  // namespace

hipError_t eval_rows(const void* logits, int dtype, int64_t ld, const int64_t* target, int B, int C,
                     int64_t ignore_index, float* row_loss, int32_t* rank, hipStream_t s) {
  if (logits == nullptr || target == nullptr || row_loss == nullptr || rank == nullptr) return hipErrorInvalidValue;
  if ((dtype != kF32 && dtype != kBF16) || B < 1 || C < 1 || (B > 1 && ld < C)) return hipErrorInvalidValue;
  const bool wave = C <= kWaveRowMaxC;
  const dim3 grid(wave ? (unsigned)((B + kRowsPerBlock - 1) / kRowsPerBlock) : (unsigned)B);
  const dim3 block(wave ? kRowBlock : kBigBlock);
  if (dtype == kF32) {
    const float* z = static_cast<const float*>(logits);
    if (wave)
      hipLaunchKernelGGL(eval_rows_wave_kernel<float>, grid, block, 0, s, z, ld, target, B, C, ignore_index, row_loss,
                         rank);
    else
      hipLaunchKernelGGL(eval_rows_block_kernel<float>, grid, block, 0, s, z, ld, target, B, C, ignore_index,
                         row_loss, rank);
  } else {
    const uint16_t* z = static_cast<const uint16_t*>(logits);
    if (wave)
      hipLaunchKernelGGL(eval_rows_wave_kernel<uint16_t>, grid, block, 0, s, z, ld, target, B, C, ignore_index,
                         row_loss, rank);
    else
      hipLaunchKernelGGL(eval_rows_block_kernel<uint16_t>, grid, block, 0, s, z, ld, target, B, C, ignore_index,
                         row_loss, rank);
  }
  return hipGetLastError();
}

hipError_t eval_accumulate(const float* row_loss, const int32_t* rank, int B, const EvalTopK& ks, int64_t* counters,
                           double* loss_sum, hipStream_t s) {
  if (row_loss == nullptr || rank == nullptr || counters == nullptr || loss_sum == nullptr || B < 1 || ks.n < 0 ||
      ks.n > kEvalMaxK)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(eval_accumulate_kernel, dim3(1), dim3(kAccBlock), 0, s, row_loss, rank, B, ks, counters,
                     loss_sum);
  return hipGetLastError();
}

}  // namespace ptdt
