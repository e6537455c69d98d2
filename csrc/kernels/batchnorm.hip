// Training-mode BatchNorm over channels-last activations with the ResNet
// epilogues fused: y = ReLU?(BN(x) + residual?), and its backward.
//
// Why (profiles/r1_resnet_window.md): in the ResNet-50 DDP step (bf16,
// channels_last, B=128) MIOpen's BatchNorm kernels plus the separate ReLU
// (clamp), residual add, ReLU-backward (threshold) and MIOpen's SubTensorOp
// passes take ~12 ms of a ~27 ms step -- all of it HBM-bound elementwise and
// reduction traffic over 11.1 M activations per image. Fusing the epilogues
// drops whole read/write passes; the reductions are written for the NHWC
// layout, where one activation row is C contiguous channels.
//
// Layout: x is [M, C] with unit channel stride (NHWC channels_last, M = N*H*W,
// or a plain [M, C] batch), bf16 or f32; weight/bias/statistics f32.
//
// Each pass loads 16 B per lane (8 bf16 / 4 f32 channels). A reduction launch is
// grid (row blocks, channel tiles): threads of a block cover TC channel vectors
// x RPI rows and walk the block's row range; partial sums are combined in LDS,
// written per row block, and the LAST row block of each channel tile to finish
// (atomic ticket; sc1 partial stores/loads, see handoff.h) reduces the partials
// in fixed order (deterministic), computes the per-channel coefficients and
// re-arms its ticket. So a BN forward is 2 launches (stats, apply) and a
// backward 2 launches (reduce, apply).
//
// Forward statistics use shifted sums (x - K, K = the channel's median of rows 0, M/2, M-1), so
// E[(x-K)^2] - E[x-K]^2 does not cancel catastrophically for |mean| >> std;
// the final combine runs in double. Running stats: torch's momentum update
// with the unbiased variance, num_batches_tracked incremented in-kernel.
//
// Backward (dy' = dy * [y > 0] with ReLU):
//   dbeta = sum dy',  dgamma = invstd * sum dy' (x - mean)
//   dx    = k dy' - k s2 (x - mean) - k s1,   k = gamma invstd,
//           s1 = dbeta / M, s2 = invstd^2 sum dy'(x - mean) / M
// i.e. dx = A dy' + B x + C per channel; with a residual branch d(residual) = dy'.
// An optional second addend dy2 (the residual gradient of the NEXT block, handed
// over by ops/norm.py's residual link) is summed into dy on the fly, replacing a
// separate add kernel (two reads + a write) by one extra read in each pass.
// The ReLU mask comes from the forward output y, or -- for BNs without a residual
// -- is recomputed from x with the forward's own fmaf(x, scale, shift), sparing
// one of the three reads in both backward passes.
#include <type_traits>

#include "bn_finish.h"
#include "common.h"
#include "handoff.h"
#include "kernels.h"
#include "vec16.h"

namespace ptdt {
namespace {

constexpr int kThreads = 256;   // apply kernels
constexpr int kRed = 512;       // reduction kernels
constexpr int kRedBlocks = 384; // ~1.5 reduction blocks per CU
constexpr int kMaxGx = 256;     // row blocks per channel tile (bounds the last block's combine)

// channel vectors per block row of a reduction (a tile of TC*V channels): 32 (whole 512-B rows
// of a C = 256 bf16 tensor per 32 lanes) for tall tensors, where the wider tile measured up to
// 13 % faster, 8 below (more row blocks to fill the chip; profiles/r3_bn_sweep.md).
// PTDT_BN_TC forces one width.
constexpr int64_t kWideRows = 262144;
int forced_tc() {
  static const int v = [] {
    const int t = env_int("PTDT_BN_TC", 0);
    return (t == 4 || t == 8 || t == 16 || t == 32 || t == 64) ? t : 0;
  }();
  return v;
}
int max_tc(int64_t M) {
  const int f = forced_tc();
  return f ? f : (M >= kWideRows ? 32 : 8);
}
int min_tc() {  // the narrowest tile any M may get: sizes the ticket array
  const int f = forced_tc();
  return f ? f : 8;
}
// vectors per thread in flight in the elementwise passes (PTDT_BN_AU: 1, 2, 4)
int apply_unroll() {
  static const int v = [] {
    const int u = env_int("PTDT_BN_AU", 1);
    return (u == 1 || u == 2 || u == 4) ? u : 1;
  }();
  return v;
}
// cap on elementwise workgroups (grid-stride beyond it); PTDT_BN_APPLY_BLOCKS, 0 = uncapped
int apply_block_cap() {
  static const int v = env_int("PTDT_BN_APPLY_BLOCKS", 4096);
  return v;
}

// Row order of the reduction passes (PTDT_BN_INTERLEAVE=0: one contiguous slab per row block).
int interleave_rows() {
  static const int v = env_int("PTDT_BN_INTERLEAVE", 1) != 0;
  return v;
}

// reduction geometry knobs (profiles/r3_bn_sweep.md): minimum rows per thread (PTDT_BN_RPT) and the
// cap on reduction workgroups (PTDT_BN_RED_BLOCKS; the grid is at most cap / channel tiles row blocks)
int red_rows_per_thread() {
  static const int v = [] {
    const int r = env_int("PTDT_BN_RPT", 16);
    return r >= 1 && r <= 256 ? r : 16;
  }();
  return v;
}
int red_block_cap() {
  static const int v = [] {
    const int c = env_int("PTDT_BN_RED_BLOCKS", kRedBlocks);
    return c >= 64 && c <= 4096 ? c : kRedBlocks;
  }();
  return v;
}

struct Geom {
  int TC, RPI;       // channel vectors per row, rows per block iteration
  int gx, gy;        // row blocks, channel tiles
  int64_t rows_per_block;
};

template <typename T>
Geom geom(int64_t M, int C) {
  constexpr int V = Vec16<T>::N;
  Geom g;
  const int cv = C / V, mt = max_tc(M);
  g.TC = cv < mt ? cv : mt;
  g.RPI = kRed / g.TC;
  g.gy = (cv + g.TC - 1) / g.TC;
  const int rpt = red_rows_per_thread();
  int64_t want = (M + (int64_t)g.RPI * rpt - 1) / ((int64_t)g.RPI * rpt);  // >= rpt rows per thread
  int64_t cap = red_block_cap() / g.gy;
  if (cap > kMaxGx) cap = kMaxGx;
  if (cap < 1) cap = 1;
  g.gx = (int)(want < 1 ? 1 : (want > cap ? cap : want));
  g.rows_per_block = (M + g.gx - 1) / g.gx;
  g.gx = (int)((M + g.rows_per_block - 1) / g.rows_per_block);
  return g;
}

// Block-level combine of per-thread V-vectors over the RPI rows sharing a channel
// vector; returns (in threads t < TC*V) the block's sum for channel c0 + t.
template <int V, int NS>
__device__ __forceinline__ void block_rows_sum(float (&acc)[NS][V], float* sh, int TC, int RPI, float (&out)[NS]) {
  const int tid = threadIdx.x;
  const int width = TC * V;
  const int rr = tid / TC, tc = tid % TC;
  if (rr < RPI) {
#pragma unroll
    for (int s = 0; s < NS; ++s)
#pragma unroll
      for (int v = 0; v < V; ++v) sh[(s * RPI + rr) * width + tc * V + v] = acc[s][v];
  }
  __syncthreads();
  if (tid < width) {
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      // in double: a serial float sum of up to 512 row sums was the largest error of the whole
      // reduction (several ulp of the variance, measured against float64)
      double a = 0.0;
      for (int r = 0; r < RPI; ++r) a += (double)sh[(s * RPI + r) * width + tid];
      out[s] = (float)a;
    }
  }
}

// Last block of a channel tile: sum the gx row-block partials (two [gx][C] slabs) of the tile's
// `width` channels with ALL threads. Thread (part, quad) adds rows part, part + P, ... of 4
// consecutive channels (P = kRed / (width / 4) parts), kCombineRows rows x 2 slabs of two 8-B
// (agent-scope atomic) loads per 4 channels in flight per thread, so the whole combine is
// ceil(gx / (P kCombineRows)) round trips -- one for
// every ResNet-50 shape. (Round 4's form, one channel per thread and 4 rows in flight, took up to
// 32 dependent round trips on the wide layer-1 tiles: gx = 256 row blocks, 256 channels.) The P
// part-sums are then added in part order through LDS (deterministic). Result in threads t < width.
constexpr int kCombineRows = 4;
// 2 slabs x P x width doubles. P x width = 4 kRed for every tile width (P = 4 kRed / width), so this
// is the size every combine needs, not a worst case (ADVICE r5 asked to size it per launch). It does
// not cost occupancy: a CU holds 4 of these 512-thread blocks by waves (32), 128 KiB of LDS.
constexpr size_t kCombineLds = (size_t)2 * kRed * 4 * sizeof(double);
__device__ __forceinline__ void combine_partials(const float* ws, int gx, int C, int cbase, int width, float* sh,
                                                 double& s0, double& s1, bool fence) {
  const int nq = width >> 2;
  const int P = kRed / nq;
  const int t = threadIdx.x, qd = t % nq, part = t / nq;
  const int c = cbase + 4 * qd;
  double a0[4] = {0.0, 0.0, 0.0, 0.0}, a1[4] = {0.0, 0.0, 0.0, 0.0};
  if (part < P && c < C) {
    const float* w0 = ws + c;
    const float* w1 = ws + (int64_t)gx * C + c;
    for (int b = part; b < gx; b += kCombineRows * P) {
      float u[kCombineRows][4], v[kCombineRows][4];
#pragma unroll
      for (int k = 0; k < kCombineRows; ++k) {
        const int r = b + k * P;
        if (r < gx) {
          ld2_sc1(w0 + (int64_t)r * C, u[k][0], u[k][1], fence);
          ld2_sc1(w0 + (int64_t)r * C + 2, u[k][2], u[k][3], fence);
          ld2_sc1(w1 + (int64_t)r * C, v[k][0], v[k][1], fence);
          ld2_sc1(w1 + (int64_t)r * C + 2, v[k][2], v[k][3], fence);
        } else {
#pragma unroll
          for (int i = 0; i < 4; ++i) u[k][i] = v[k][i] = 0.f;
        }
      }
#pragma unroll
      for (int k = 0; k < kCombineRows; ++k)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          a0[i] += (double)u[k][i];
          a1[i] += (double)v[k][i];
        }
    }
  }
  __syncthreads();  // the reduction slots in sh are free again
  double* d = reinterpret_cast<double*>(sh);
  if (part < P) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      d[part * width + 4 * qd + i] = a0[i];
      d[(P + part) * width + 4 * qd + i] = a1[i];
    }
  }
  __syncthreads();
  s0 = s1 = 0.0;
  if (t < width) {
    for (int q = 0; q < P; ++q) {
      s0 += d[q * width + t];
      s1 += d[(P + q) * width + t];
    }
  }
}

// Cross-rank statistics (SyncBatchNorm, ops/norm.py). SYNC / RAW instances of the two reduction
// kernels stop before the local row count finalises anything: the last block writes this rank's
// float64 record instead, the ranks exchange the records, and bn_sync_merge_kernel /
// bn_sync_coef_kernel finish with the global count. The parameter blocks extend the local ones, so
// the sweeps, the partial hand-off and the combine are the same code.
struct BnSyncParams : BnParams {
  double* rec;  // [2 C + 1]: local mean[C], M2[C] = sum (x - local mean)^2, row count
};
struct BnSyncBwdParams : BnBwdParams {
  double* sums;  // [2, C]: local sum g, sum g (x - mean) about the GLOBAL mean
};

// Pivot K of the shifted sums: per channel the median of rows 0, M/2 and M-1, so one outlying row
// (row 0 of a padded or sorted batch) cannot put K far from the mean and bring the cancellation in
// E[(x-K)^2] - E[x-K]^2 back. Every block and the last block's combine form the same K.
__device__ __forceinline__ float median3(float a, float b, float c) {
  return fmaxf(fminf(a, b), fminf(fmaxf(a, b), c));
}
template <typename T>
__device__ __forceinline__ float pivot_of(const T* x, int64_t M, int C, int c) {
  return median3(Cvt<T>::load(x, c), Cvt<T>::load(x, (M / 2) * C + c), Cvt<T>::load(x, (M - 1) * C + c));
}

template <typename T, bool SYNC = false>
__global__ void __launch_bounds__(kRed) bn_stats_kernel(const T* __restrict__ x, int64_t M, int C, int TC, int RPI,
                                                        int64_t rows_per_block, int il, float* ws, int* tickets,
                                                        std::conditional_t<SYNC, BnSyncParams, BnParams> p) {
  constexpr int V = Vec16<T>::N;
  constexpr int U = 8;  // rows in flight per thread
  extern __shared__ float sh[];  // 2 x RPI x TC*V reduction slots, then the last-block flag
  int* flag = reinterpret_cast<int*>(sh + 2 * kRed * V);
  const int tid = threadIdx.x, rr = tid / TC, tc = tid % TC;
  const int c0 = (blockIdx.y * TC + tc) * V;  // this thread's channels c0..c0+V
  const bool active = rr < RPI && c0 < C;
  // il bit 1: sweep the rows last to first (pass_dirs())
  const bool rev = (il & 2) != 0;
  il &= 1;
  auto row = [&](int64_t r) { return rev ? M - 1 - r : r; };
  // il: rows interleaved across the row blocks in RPI-row chunks (block b: chunks b, b + gx, ...),
  // so the grid sweeps the tensor front to back together, as the elementwise passes do; else each
  // block owns one contiguous slab of rows_per_block rows (gx separate streams)
  const int64_t rs = il ? (int64_t)gridDim.x * RPI : RPI;
  const int64_t rb = il ? (int64_t)blockIdx.x * RPI : (int64_t)blockIdx.x * rows_per_block;
  const int64_t re = il ? M : min(M, rb + rows_per_block);
  float acc[2][V];
#pragma unroll
  for (int v = 0; v < V; ++v) acc[0][v] = acc[1][v] = 0.f;
  if (active) {
    float K[V], K1[V], K2[V];  // pivot (same for every block): pivot_of(), a vector at a time
    Vec16<T>::load(x + c0, K);
    Vec16<T>::load(x + (M / 2) * C + c0, K1);
    Vec16<T>::load(x + (M - 1) * C + c0, K2);
#pragma unroll
    for (int v = 0; v < V; ++v) K[v] = median3(K[v], K1[v], K2[v]);
    int64_t r = rb + rr;
    for (; r + (U - 1) * rs < re; r += U * rs) {  // U independent 16-B loads in flight
      float a[U][V];
#pragma unroll
      for (int u = 0; u < U; ++u) Vec16<T>::load(x + row(r + u * rs) * C + c0, a[u]);
      // each batch of U rows is summed on its own and then added: a running float sum of every
      // row stagnates on bf16 data (the addends sit on a coarse grid and tie after tie rounds to
      // even, i.e. down), which biased the variance low by up to 2e-6 of itself on tall tensors
      float b[2][V];
#pragma unroll
      for (int v = 0; v < V; ++v) b[0][v] = b[1][v] = 0.f;
#pragma unroll
      for (int u = 0; u < U; ++u)
#pragma unroll
        for (int v = 0; v < V; ++v) {
          const float d = a[u][v] - K[v];
          b[0][v] += d;
          b[1][v] = fmaf(d, d, b[1][v]);
        }
#pragma unroll
      for (int v = 0; v < V; ++v) {
        acc[0][v] += b[0][v];
        acc[1][v] += b[1][v];
      }
    }
    for (; r < re; r += rs) {
      float a[V];
      Vec16<T>::load(x + row(r) * C + c0, a);
#pragma unroll
      for (int v = 0; v < V; ++v) {
        const float d = a[v] - K[v];
        acc[0][v] += d;
        acc[1][v] = fmaf(d, d, acc[1][v]);
      }
    }
  }
  float part[2];
  block_rows_sum<V, 2>(acc, sh, TC, RPI, part);
  const int width = TC * V;
  const int c = blockIdx.y * width + tid;
  const int gx = (int)gridDim.x;  // row blocks: the ticket's count
  if (tid < width && c < C) {
    st_sc1(ws + (int64_t)blockIdx.x * C + c, part[0], (p.fence_handoff != 0));
    st_sc1(ws + ((int64_t)gx + blockIdx.x) * C + c, part[1], (p.fence_handoff != 0));
  }
  if (!last_arrival(tickets + blockIdx.y, gx, flag, (p.fence_handoff != 0))) return;
  double s, q;
  combine_partials(ws, gx, C, blockIdx.y * width, width, sh, s, q, (p.fence_handoff != 0));
  if constexpr (SYNC) {  // this rank's record; invstd and the running statistics wait for the merge
    if (tid < width && c < C) {
      double m2 = q - s * s / (double)M;
      if (m2 < 0.0) m2 = 0.0;
      p.rec[c] = (double)pivot_of<T>(x, M, C, c) + s / (double)M;
      p.rec[C + c] = m2;
    }
    if (tid == 0 && blockIdx.y == 0) p.rec[2 * C] = (double)M;
    return;
  }
  if (tid < width && c < C) {
    const double Kc = (double)pivot_of<T>(x, M, C, c);
    const double ms = s / (double)M;
    double var = q / (double)M - ms * ms;
    if (var < 0.0) var = 0.0;
    bn_finish_channel(p, c, Kc + ms, var, M > 1 ? var * (double)M / (double)(M - 1) : var);
  }
  if (tid == 0 && blockIdx.y == 0 && p.num_batches_tracked) *p.num_batches_tracked += 1;
}

// Merge of the W gathered records ([W, 2 C + 1], rank-major) into the [4, C] statistics the apply
// and backward passes consume; one thread per channel, Chan's pairwise update in rank order, in
// double. Every rank merges the same bytes in the same order: statistics and running buffers come
// out bitwise identical across ranks. `count` receives the global row count N (the backward's
// coefficient pass reads it there: no host round trip). A rank with no rows is skipped.
__global__ void __launch_bounds__(kThreads) bn_sync_merge_kernel(const double* __restrict__ rec, int W, int C,
                                                                 BnParams p, double* __restrict__ count) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const int64_t slot = 2 * (int64_t)C + 1;
  double n = 0.0, mean = 0.0, m2 = 0.0;
  for (int r = 0; r < W; ++r) {
    const double* rr = rec + r * slot;
    const double nb = rr[2 * C];
    if (!(nb > 0.0)) continue;
    const double mb = rr[c], m2b = rr[C + c];
    if (n == 0.0) {
      n = nb;
      mean = mb;
      m2 = m2b;
    } else {
      const double na = n, d = mb - mean;
      n = na + nb;
      mean = mean + d * nb / n;
      m2 = m2 + m2b + d * d * na * nb / n;
    }
  }
  const double var = n > 0.0 ? m2 / n : 0.0;
  bn_finish_channel(p, c, mean, var, n > 1.0 ? m2 / (n - 1.0) : var);
  if (c == 0) {
    *count = n;
    if (p.num_batches_tracked) *p.num_batches_tracked += 1;
  }
}

// dx = A g + B x + C coefficients from the all-reduced sums ([2, C]: sum g, sum g (x - mean)) and
// the global row count: bn_bwd_reduce_kernel's formulas with M replaced by N
__global__ void __launch_bounds__(kThreads) bn_sync_coef_kernel(const double* __restrict__ sums,
                                                                const double* __restrict__ count, int C,
                                                                BnBwdParams p) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  bn_bwd_coef_channel(p, c, sums[c], sums[C + c], *count);
}

// MASKOUT: also write the ReLU mask, one byte per V-vector (bit v: y > 0), for a backward that
// then reads 1/16 (bf16) of a tensor instead of y
// Elementwise passes: each thread keeps AU vectors (stride apart) in flight per iteration.
template <typename T, bool RELU, bool RES, bool MASKOUT = false, int AU = 1>
__global__ void __launch_bounds__(kThreads) bn_apply_kernel(const T* __restrict__ x, const T* __restrict__ res,
                                                            T* __restrict__ y, const float* __restrict__ scale,
                                                            const float* __restrict__ shift, int64_t nvec, int C,
                                                            int rev, uint8_t* __restrict__ mask) {
  constexpr int V = Vec16<T>::N;
  extern __shared__ float sh[];  // scale[C], shift[C]
  for (int c = threadIdx.x; c < C; c += blockDim.x) {
    sh[c] = scale[c];
    sh[C + c] = shift[c];
  }
  __syncthreads();
  const int cv = C / V;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  auto vid = [&](int64_t i) { return rev ? nvec - 1 - i : i; };  // rev: last vector first
  for (int64_t i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i0 < nvec; i0 += AU * stride) {
    float a[AU][V], rv[AU][V];
#pragma unroll
    for (int u = 0; u < AU; ++u) {
      const int64_t i = vid(i0 + u * stride);
      if (i0 + u * stride < nvec) {
        Vec16<T>::load(x + i * V, a[u]);
        if constexpr (RES) Vec16<T>::load(res + i * V, rv[u]);
      }
    }
#pragma unroll
    for (int u = 0; u < AU; ++u) {
      if (i0 + u * stride >= nvec) break;
      const int64_t i = vid(i0 + u * stride);
      const int c0 = (int)(i % cv) * V;
      unsigned bits = 0;
#pragma unroll
      for (int v = 0; v < V; ++v) {
        float o = fmaf(a[u][v], sh[c0 + v], sh[C + c0 + v]);
        if constexpr (RES) o += rv[u][v];
        if constexpr (RELU) o = fmaxf(o, 0.f);
        if constexpr (MASKOUT) bits |= (o > 0.f ? 1u : 0u) << v;
        a[u][v] = o;
      }
      Vec16<T>::store(y + i * V, a[u]);
      if constexpr (MASKOUT) mask[i] = (uint8_t)bits;
    }
  }
}

// MASK: 0 no ReLU, 1 ReLU mask from the forward output y, 2 ReLU mask recomputed
// from x (y > 0 <=> fmaf(x, scale, shift) > 0 bit-exactly, as the forward applied
// it): BNs without a residual skip reading y in both backward passes.
// MASK 3: the forward's bit mask (one byte per V-vector); `y` carries the bit as 0 / 1.
template <int MASK, int V>
__device__ __forceinline__ float masked_dy(float g, float x, float y, float sc, float sf) {
  if constexpr (MASK == 1 || MASK == 3) return y > 0.f ? g : 0.f;
  if constexpr (MASK == 2) return fmaf(x, sc, sf) > 0.f ? g : 0.f;
  return g;
}

// GOUT: the masked gradient g = mask (dy + dy2), rounded to T, is also written (to gout): it IS
// the residual gradient, and the apply pass then reads g and x only (bn_bwd_apply_g_kernel)
// instead of dy, dy2, x and the mask. The sums use the rounded g, so both passes agree.
// RAW (cross-rank statistics): mean / invstd are the global ones; the last block writes the local
// sums as float64 (for the all-reduce) and the LOCAL parameter gradients, and no coefficients.
template <typename T, int MASK, bool ADD2, bool GOUT = false, bool RAW = false>
__global__ void __launch_bounds__(kRed) bn_bwd_reduce_kernel(const T* __restrict__ dy, const T* __restrict__ dy2,
                                                             const T* __restrict__ x,
                                                             const T* __restrict__ y, const uint8_t* __restrict__ mk,
                                                             T* __restrict__ gout, int64_t M, int C, int TC,
                                                             int RPI, int64_t rows_per_block, int il, float* ws,
                                                             int* tickets,
                                                             std::conditional_t<RAW, BnSyncBwdParams, BnBwdParams> p) {
  constexpr int V = Vec16<T>::N;
  constexpr int U = 4;  // rows in flight per thread (x 2-3 loads each)
  extern __shared__ float sh[];
  int* flag = reinterpret_cast<int*>(sh + 2 * kRed * V);
  const int tid = threadIdx.x, rr = tid / TC, tc = tid % TC;
  const int c0 = (blockIdx.y * TC + tc) * V;
  const bool active = rr < RPI && c0 < C;
  const bool rev = (il & 2) != 0;
  il &= 1;
  auto row = [&](int64_t r) { return rev ? M - 1 - r : r; };
  const int64_t rs = il ? (int64_t)gridDim.x * RPI : RPI;  // row order: as in bn_stats_kernel
  const int64_t rb = il ? (int64_t)blockIdx.x * RPI : (int64_t)blockIdx.x * rows_per_block;
  const int64_t re = il ? M : min(M, rb + rows_per_block);
  float acc[2][V];
#pragma unroll
  for (int v = 0; v < V; ++v) acc[0][v] = acc[1][v] = 0.f;
  if (active) {
    float mu[V], sc[V], sf[V];
#pragma unroll
    for (int v = 0; v < V; ++v) {
      mu[v] = p.mean[c0 + v];
      sc[v] = MASK == 2 ? p.scale[c0 + v] : 0.f;
      sf[v] = MASK == 2 ? p.shift[c0 + v] : 0.f;
    }
    int64_t r = rb + rr;
    const int cv = C / V;
    // ReLU mask operand o[v] (0 / 1 bits for MASK 3, y for MASK 1)
    auto load_mask = [&](int64_t row, int64_t off, float (&o)[V]) {
      if constexpr (MASK == 1) {
        Vec16<T>::load(y + off, o);
      } else if constexpr (MASK == 3) {
        const unsigned b = mk[row * cv + c0 / V];
#pragma unroll
        for (int v = 0; v < V; ++v) o[v] = (float)((b >> v) & 1u);
      }
    };
    auto finish = [&](float (&g)[V], const float (&a)[V], const float (&o)[V], int64_t off) {
#pragma unroll
      for (int v = 0; v < V; ++v) {
        float gg = masked_dy<MASK, V>(g[v], a[v], (MASK == 1 || MASK == 3) ? o[v] : 0.f, sc[v], sf[v]);
        if constexpr (GOUT) gg = round_to<T>(gg);
        g[v] = gg;
        acc[0][v] += gg;
        acc[1][v] = fmaf(gg, a[v] - mu[v], acc[1][v]);
      }
      if constexpr (GOUT) Vec16<T>::store(gout + off, g);
    };
    for (; r + (U - 1) * rs < re; r += U * rs) {
      float g[U][V], a[U][V], o[U][V], g2[ADD2 ? U : 1][V];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int64_t off = row(r + u * rs) * C + c0;
        Vec16<T>::load(dy + off, g[u]);
        if constexpr (ADD2) Vec16<T>::load(dy2 + off, g2[u]);
        Vec16<T>::load(x + off, a[u]);
        load_mask(row(r + u * rs), off, o[u]);
      }
      if constexpr (ADD2) {
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
          for (int v = 0; v < V; ++v) g[u][v] += g2[u][v];
      }
#pragma unroll
      for (int u = 0; u < U; ++u) finish(g[u], a[u], o[u], row(r + u * rs) * C + c0);
    }
    for (; r < re; r += rs) {
      float g[V], a[V], o[V];
      const int64_t off = row(r) * C + c0;
      Vec16<T>::load(dy + off, g);
      if constexpr (ADD2) {
        float g2[V];
        Vec16<T>::load(dy2 + off, g2);
#pragma unroll
        for (int v = 0; v < V; ++v) g[v] += g2[v];
      }
      Vec16<T>::load(x + off, a);
      load_mask(row(r), off, o);
      finish(g, a, o, off);
    }
  }
  float part[2];
  block_rows_sum<V, 2>(acc, sh, TC, RPI, part);
  const int width = TC * V;
  const int c = blockIdx.y * width + tid;
  const int gx = (int)gridDim.x;  // row blocks: the ticket's count
  if (tid < width && c < C) {
    st_sc1(ws + (int64_t)blockIdx.x * C + c, part[0], (p.fence_handoff != 0));
    st_sc1(ws + ((int64_t)gx + blockIdx.x) * C + c, part[1], (p.fence_handoff != 0));
  }
  if (!last_arrival(tickets + blockIdx.y, gx, flag, (p.fence_handoff != 0))) return;
  double sdy, sdx;
  combine_partials(ws, gx, C, blockIdx.y * width, width, sh, sdy, sdx, (p.fence_handoff != 0));
  if constexpr (RAW) {  // this rank's sums for the all-reduce; the coefficients wait for bn_sync_coef_kernel
    if (tid < width && c < C) {
      p.sums[c] = sdy;
      p.sums[C + c] = sdx;
    }
  }
  if (tid < width && c < C) bn_bwd_finish_channel(p, c, sdy, sdx, (double)M, !RAW);
}

// dx = A g + B x + C from the reduce pass's materialised g (GOUT): 2 reads + 1 write
template <typename T, int AU = 1>
__global__ void __launch_bounds__(kThreads) bn_bwd_apply_g_kernel(const T* __restrict__ g, const T* __restrict__ x,
                                                                  T* __restrict__ dx, BnBwdParams p, int64_t nvec,
                                                                  int C, int rev) {
  constexpr int V = Vec16<T>::N;
  extern __shared__ float sh[];  // A[C], B[C], C[C]
  for (int c = threadIdx.x; c < C; c += blockDim.x) {
    sh[c] = p.coef_a[c];
    sh[C + c] = p.coef_b[c];
    sh[2 * C + c] = p.coef_c[c];
  }
  __syncthreads();
  const int cv = C / V;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  auto vid = [&](int64_t i) { return rev ? nvec - 1 - i : i; };  // rev: last vector first
  for (int64_t i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i0 < nvec; i0 += AU * stride) {
    float gg[AU][V], a[AU][V];
#pragma unroll
    for (int u = 0; u < AU; ++u) {
      const int64_t i = vid(i0 + u * stride);
      if (i0 + u * stride < nvec) {
        Vec16<T>::load(g + i * V, gg[u]);
        Vec16<T>::load(x + i * V, a[u]);
      }
    }
#pragma unroll
    for (int u = 0; u < AU; ++u) {
      if (i0 + u * stride >= nvec) break;
      const int64_t i = vid(i0 + u * stride);
      const int c0 = (int)(i % cv) * V;
#pragma unroll
      for (int v = 0; v < V; ++v)
        a[u][v] = fmaf(sh[c0 + v], gg[u][v], fmaf(sh[C + c0 + v], a[u][v], sh[2 * C + c0 + v]));
      Vec16<T>::store(dx + i * V, a[u]);
    }
  }
}

template <typename T, int MASK, bool RES, bool ADD2, int AU = 1>
__global__ void __launch_bounds__(kThreads) bn_bwd_apply_kernel(const T* __restrict__ dy, const T* __restrict__ dy2,
                                                                const T* __restrict__ x,
                                                                const T* __restrict__ y, T* __restrict__ dx,
                                                                T* __restrict__ dres, BnBwdParams p, int64_t nvec,
                                                                int C, int rev) {
  constexpr int V = Vec16<T>::N;
  extern __shared__ float sh[];  // A[C], B[C], C[C] (+ scale[C], shift[C] for MASK 2)
  for (int c = threadIdx.x; c < C; c += blockDim.x) {
    sh[c] = p.coef_a[c];
    sh[C + c] = p.coef_b[c];
    sh[2 * C + c] = p.coef_c[c];
    if constexpr (MASK == 2) {
      sh[3 * C + c] = p.scale[c];
      sh[4 * C + c] = p.shift[c];
    }
  }
  __syncthreads();
  const int cv = C / V;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  auto vid = [&](int64_t i) { return rev ? nvec - 1 - i : i; };  // rev: last vector first
  for (int64_t i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i0 < nvec; i0 += AU * stride) {
    float g[AU][V], a[AU][V], o[AU][V], g2[ADD2 ? AU : 1][V];
#pragma unroll
    for (int u = 0; u < AU; ++u) {
      const int64_t i = vid(i0 + u * stride);
      if (i0 + u * stride < nvec) {
        Vec16<T>::load(dy + i * V, g[u]);
        if constexpr (ADD2) Vec16<T>::load(dy2 + i * V, g2[u]);
        Vec16<T>::load(x + i * V, a[u]);
        if constexpr (MASK == 1) Vec16<T>::load(y + i * V, o[u]);
      }
    }
#pragma unroll
    for (int u = 0; u < AU; ++u) {
      if (i0 + u * stride >= nvec) break;
      const int64_t i = vid(i0 + u * stride);
      const int c0 = (int)(i % cv) * V;
#pragma unroll
      for (int v = 0; v < V; ++v) {
        float gv = g[u][v];
        if constexpr (ADD2) gv += g2[u][v];
        gv = masked_dy<MASK, V>(gv, a[u][v], MASK == 1 ? o[u][v] : 0.f, MASK == 2 ? sh[3 * C + c0 + v] : 0.f,
                                MASK == 2 ? sh[4 * C + c0 + v] : 0.f);
        g[u][v] = gv;
        a[u][v] = fmaf(sh[c0 + v], gv, fmaf(sh[C + c0 + v], a[u][v], sh[2 * C + c0 + v]));
      }
      Vec16<T>::store(dx + i * V, a[u]);
      if constexpr (RES) Vec16<T>::store(dres + i * V, g[u]);
    }
  }
}

// LDS of a reduction launch: the row-sum slots (2 x kRed x V floats, then the last-block flag)
// and the combine's part sums (kCombineLds) share one array
template <typename T>
size_t red_lds() {
  const size_t rows = (size_t)2 * kRed * Vec16<T>::N * sizeof(float) + 16;
  return rows > kCombineLds ? rows : kCombineLds;
}

int apply_grid(int64_t nvec) {
  const int au = apply_unroll(), cap = apply_block_cap();
  int64_t per = (int64_t)kThreads * (cap > 0 ? 4 : au);  // >= 4 vectors per thread when capped
  int64_t b = (nvec + per - 1) / per;
  if (cap > 0 && b > cap) b = cap;
  return (int)(b < 1 ? 1 : b);
}

// Sweep direction of each pass (PTDT_BN_DIR bits: 1 stats, 2 forward apply, 4 backward reduce,
// 8 backward apply; set = last row first). Consecutive passes over one tensor in opposite
// directions re-read the most recently touched lines first, which the 256 MiB Infinity Cache
// still holds (MI355X_MICROARCH.md "Infinity Cache").
int pass_dirs() {
  static const int v = env_int("PTDT_BN_DIR", 0);
  return v;
}
int dir(int bit) { return (pass_dirs() & bit) ? 1 : 0; }

// Dynamic LDS of the elementwise passes: their per-channel tables (2, 3 or 5 floats per channel).
// Above 64 KiB a kernel has to be opted in to its size; a workgroup can hold 160 KiB at the most, and
// the widest table (5 floats: bn_bwd_apply_kernel<MASK 2>) then bounds the channel count the native
// path takes (bn_max_channels(); the bindings and ops/norm.py send wider tensors to the composite).
constexpr size_t kLdsOptIn = 64 * 1024, kLdsMax = 160 * 1024;
template <typename K, typename... A>
hipError_t launch_lds(K kernel, dim3 grid, dim3 blk, size_t lds, hipStream_t s, A... args) {
  if (lds > kLdsMax) return hipErrorInvalidValue;
  if (lds > kLdsOptIn)
    PTDT_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(kernel, grid, blk, lds, s, args...);
  return hipGetLastError();
}

// runtime AU -> template
template <typename F>
hipError_t with_au(F&& f) {
  switch (apply_unroll()) {
    case 2: return f(std::integral_constant<int, 2>{});
    case 4: return f(std::integral_constant<int, 4>{});
    default: return f(std::integral_constant<int, 1>{});
  }
}

template <typename T>
hipError_t fwd_impl(const BnFwdArgs& a, hipStream_t s) {
  constexpr int V = Vec16<T>::N;
  if (a.C % V != 0) return hipErrorInvalidValue;
  const Geom g = geom<T>(a.M, a.C);
  const size_t sh_red = red_lds<T>();
  if (!a.stats_ready) {
    hipLaunchKernelGGL(bn_stats_kernel<T>, dim3(g.gx, g.gy), dim3(kRed), sh_red, s, static_cast<const T*>(a.x),
                       a.M, a.C, g.TC, g.RPI, g.rows_per_block, interleave_rows() | (dir(1) << 1), a.workspace,
                       a.tickets, a.p);
    PTDT_HIP_CHECK(hipGetLastError());
  }
  if (a.y == nullptr) return hipSuccess;  // statistics only (the apply runs in the consumer, e.g. a pool)
  const int64_t nvec = a.M * a.C / V;
  const size_t sh_ap = (size_t)2 * a.C * sizeof(float);
  const T* x = static_cast<const T*>(a.x);
  const T* r = static_cast<const T*>(a.residual);
  T* y = static_cast<T*>(a.y);
  const dim3 grid(apply_grid(nvec)), blk(kThreads);
  const float *sc = a.p.scale, *sf = a.p.shift;
  uint8_t* mo = a.mask_out;
  const int C = a.C;
  return with_au([&](auto au) {
    constexpr int AU = decltype(au)::value;
    if (a.relu) {
      if (r && mo) return launch_lds(bn_apply_kernel<T, true, true, true, AU>, grid, blk, sh_ap, s, x, r, y, sc, sf, nvec, C, dir(2), mo);
      else if (r) return launch_lds(bn_apply_kernel<T, true, true, false, AU>, grid, blk, sh_ap, s, x, r, y, sc, sf, nvec, C, dir(2), nullptr);
      else return launch_lds(bn_apply_kernel<T, true, false, false, AU>, grid, blk, sh_ap, s, x, r, y, sc, sf, nvec, C, dir(2), nullptr);
    } else {
      if (r) return launch_lds(bn_apply_kernel<T, false, true, false, AU>, grid, blk, sh_ap, s, x, r, y, sc, sf, nvec, C, dir(2), nullptr);
      else return launch_lds(bn_apply_kernel<T, false, false, false, AU>, grid, blk, sh_ap, s, x, r, y, sc, sf, nvec, C, dir(2), nullptr);
    }
  });
}

template <typename T>
hipError_t apply_impl(const void* x, const void* res, void* y, const float* scale, const float* shift, int64_t M,
                      int C, int relu, hipStream_t s) {
  constexpr int V = Vec16<T>::N;
  if (C % V != 0) return hipErrorInvalidValue;
  const int64_t nvec = M * C / V;
  const size_t sh_ap = (size_t)2 * C * sizeof(float);
  const T* xx = static_cast<const T*>(x);
  const T* r = static_cast<const T*>(res);
  T* yy = static_cast<T*>(y);
  const dim3 grid(apply_grid(nvec)), blk(kThreads);
  return with_au([&](auto au) {
    constexpr int AU = decltype(au)::value;
    if (relu) {
      if (r) return launch_lds(bn_apply_kernel<T, true, true, false, AU>, grid, blk, sh_ap, s, xx, r, yy, scale, shift, nvec, C, 0, nullptr);
      else return launch_lds(bn_apply_kernel<T, true, false, false, AU>, grid, blk, sh_ap, s, xx, r, yy, scale, shift, nvec, C, 0, nullptr);
    } else {
      if (r) return launch_lds(bn_apply_kernel<T, false, true, false, AU>, grid, blk, sh_ap, s, xx, r, yy, scale, shift, nvec, C, 0, nullptr);
      else return launch_lds(bn_apply_kernel<T, false, false, false, AU>, grid, blk, sh_ap, s, xx, r, yy, scale, shift, nvec, C, 0, nullptr);
    }
  });
}

template <typename T, int MASK, bool ADD2>
hipError_t bwd_launch(const BnBwdArgs& a, const Geom& g, hipStream_t s) {
  constexpr int V = Vec16<T>::N;
  const size_t sh_red = red_lds<T>();
  const T* dy = static_cast<const T*>(a.dy);
  const T* dy2 = static_cast<const T*>(a.dy2);
  const T* x = static_cast<const T*>(a.x);
  const T* y = static_cast<const T*>(a.y);
  const int64_t nvec = a.M * a.C / V;
  T* dx = static_cast<T*>(a.dx);
  T* dr = static_cast<T*>(a.dres);
  const dim3 grid(apply_grid(nvec)), blk(kThreads);
  if (a.reduce_only) {  // g materialised for a consumer that applies the coefficients itself
    if (!dr) return hipErrorInvalidValue;
    hipLaunchKernelGGL((bn_bwd_reduce_kernel<T, MASK, ADD2, true>), dim3(g.gx, g.gy), dim3(kRed), sh_red, s, dy, dy2,
                       x, y, a.mask, dr, a.M, a.C, g.TC, g.RPI, g.rows_per_block, interleave_rows() | (dir(4) << 1),
                       a.workspace, a.tickets, a.p);
    return hipGetLastError();
  }
  if (dr) {  // the residual gradient is wanted: the reduce pass writes g there, the apply reads g and x
    hipLaunchKernelGGL((bn_bwd_reduce_kernel<T, MASK, ADD2, true>), dim3(g.gx, g.gy), dim3(kRed), sh_red, s, dy, dy2,
                       x, y, a.mask, dr, a.M, a.C, g.TC, g.RPI, g.rows_per_block, interleave_rows() | (dir(4) << 1), a.workspace,
                       a.tickets, a.p);
    PTDT_HIP_CHECK(hipGetLastError());
    return with_au([&](auto au) {
      return launch_lds(bn_bwd_apply_g_kernel<T, decltype(au)::value>, grid, blk, (size_t)3 * a.C * sizeof(float), s,
                        static_cast<const T*>(dr), x, dx, a.p, nvec, a.C, dir(8));
    });
  }
  hipLaunchKernelGGL((bn_bwd_reduce_kernel<T, MASK, ADD2>), dim3(g.gx, g.gy), dim3(kRed), sh_red, s, dy, dy2, x, y,
                     a.mask, nullptr, a.M, a.C, g.TC, g.RPI, g.rows_per_block, interleave_rows() | (dir(4) << 1), a.workspace,
                     a.tickets, a.p);
  PTDT_HIP_CHECK(hipGetLastError());
  if constexpr (MASK == 3) {
    return hipErrorInvalidValue;  // bit masks come with a residual (RES): the g path above
  } else {
    const size_t sh_ap = (size_t)(MASK == 2 ? 5 : 3) * a.C * sizeof(float);
    return with_au([&](auto au) {
      return launch_lds(bn_bwd_apply_kernel<T, MASK, false, ADD2, decltype(au)::value>, grid, blk, sh_ap, s, dy, dy2,
                        x, y, dx, dr, a.p, nvec, a.C, dir(8));
    });
  }
}

template <typename T, int MASK>
hipError_t bwd_launch2(const BnBwdArgs& a, const Geom& g, hipStream_t s) {
  return a.dy2 != nullptr ? bwd_launch<T, MASK, true>(a, g, s) : bwd_launch<T, MASK, false>(a, g, s);
}

template <typename T>
hipError_t bwd_impl(const BnBwdArgs& a, hipStream_t s) {
  constexpr int V = Vec16<T>::N;
  if (a.C % V != 0) return hipErrorInvalidValue;
  const Geom g = geom<T>(a.M, a.C);
  if (!a.relu) return bwd_launch2<T, 0>(a, g, s);
  if (a.mask != nullptr) {
    if (a.dres == nullptr) return hipErrorInvalidValue;
    return bwd_launch2<T, 3>(a, g, s);
  }
  if (a.y != nullptr) return bwd_launch2<T, 1>(a, g, s);
  if (a.p.scale == nullptr || a.p.shift == nullptr) return hipErrorInvalidValue;
  return bwd_launch2<T, 2>(a, g, s);
}

// ---- cross-rank statistics (SyncBatchNorm): launches of the SYNC / RAW instances
template <typename T>
hipError_t sync_stats_impl(const void* x, int64_t M, int C, float* ws, int* tickets, double* rec, int fence,
                           hipStream_t s) {
  if (C % Vec16<T>::N != 0) return hipErrorInvalidValue;
  const Geom g = geom<T>(M, C);
  BnSyncParams p{};
  p.rec = rec;
  p.fence_handoff = fence;
  hipLaunchKernelGGL((bn_stats_kernel<T, true>), dim3(g.gx, g.gy), dim3(kRed), red_lds<T>(), s,
                     static_cast<const T*>(x), M, C, g.TC, g.RPI, g.rows_per_block,
                     interleave_rows() | (dir(1) << 1), ws, tickets, p);
  return hipGetLastError();
}

template <typename T, int MASK, bool ADD2>
hipError_t sync_reduce_launch(const BnBwdArgs& a, double* sums, hipStream_t s) {
  const Geom g = geom<T>(a.M, a.C);
  BnSyncBwdParams p{};
  static_cast<BnBwdParams&>(p) = a.p;
  p.sums = sums;
  hipLaunchKernelGGL((bn_bwd_reduce_kernel<T, MASK, ADD2, true, true>), dim3(g.gx, g.gy), dim3(kRed), red_lds<T>(), s,
                     static_cast<const T*>(a.dy), static_cast<const T*>(a.dy2), static_cast<const T*>(a.x),
                     static_cast<const T*>(nullptr), a.mask, static_cast<T*>(a.dres), a.M, a.C, g.TC, g.RPI,
                     g.rows_per_block, interleave_rows() | (dir(4) << 1), a.workspace, a.tickets, p);
  return hipGetLastError();
}

template <typename T>
hipError_t sync_reduce_impl(const BnBwdArgs& a, double* sums, hipStream_t s) {
  if (a.C % Vec16<T>::N != 0 || a.dres == nullptr) return hipErrorInvalidValue;
  const bool add2 = a.dy2 != nullptr;
  if (!a.relu) return add2 ? sync_reduce_launch<T, 0, true>(a, sums, s) : sync_reduce_launch<T, 0, false>(a, sums, s);
  if (a.mask != nullptr)
    return add2 ? sync_reduce_launch<T, 3, true>(a, sums, s) : sync_reduce_launch<T, 3, false>(a, sums, s);
  if (a.p.scale == nullptr || a.p.shift == nullptr) return hipErrorInvalidValue;
  return add2 ? sync_reduce_launch<T, 2, true>(a, sums, s) : sync_reduce_launch<T, 2, false>(a, sums, s);
}

template <typename T>
hipError_t apply_g_impl(const void* g, const void* x, void* dx, const float* coef, int64_t M, int C, hipStream_t s) {
  constexpr int V = Vec16<T>::N;
  if (C % V != 0) return hipErrorInvalidValue;
  const int64_t nvec = M * C / V;
  BnBwdParams p{};
  p.coef_a = const_cast<float*>(coef);
  p.coef_b = const_cast<float*>(coef) + C;
  p.coef_c = const_cast<float*>(coef) + 2 * C;
  const dim3 grid(apply_grid(nvec)), blk(kThreads);
  return with_au([&](auto au) {
    return launch_lds(bn_bwd_apply_g_kernel<T, decltype(au)::value>, grid, blk, (size_t)3 * C * sizeof(float), s,
                      static_cast<const T*>(g), static_cast<const T*>(x), static_cast<T*>(dx), p, nvec, C, dir(8));
  });
}

}  // namespace

int64_t bn_workspace_floats(int64_t M, int C, int dtype) {
  const Geom g = dtype == kF32 ? geom<float>(M, C) : geom<uint16_t>(M, C);
  return (int64_t)2 * g.gx * C;
}
// the reduction grid of an [M, C] tensor as the launches take it: out = TC, RPI, gx, gy (tests)
void bn_geometry(int64_t M, int C, int dtype, int out[4]) {
  const Geom g = dtype == kF32 ? geom<float>(M, C) : geom<uint16_t>(M, C);
  out[0] = g.TC, out[1] = g.RPI, out[2] = g.gx, out[3] = g.gy;
}
// widest C of the native path: bn_bwd_apply_kernel<MASK 2> stages 5 floats per channel in LDS
int bn_max_channels() { return (int)(kLdsMax / (5 * sizeof(float))); }
int bn_num_tickets(int C, int dtype) {
  const int V = dtype == kF32 ? 4 : 8;
  const int cv = C / V, mt = min_tc();
  const int TC = cv < mt ? cv : mt;
  return (cv + TC - 1) / TC;
}

// PTDT_BN_FENCE=1: the fence-based partial hand-off, for same-box A/B measurements only
int fence_handoff() {
  static const int v = env_int("PTDT_BN_FENCE", 0) != 0;
  return v;
}

hipError_t bn_forward_train(const BnFwdArgs& a0, hipStream_t s) {
  if (a0.M <= 0 || a0.C <= 0 || a0.C > bn_max_channels()) return hipErrorInvalidValue;
  BnFwdArgs a = a0;
  a.p.fence_handoff = fence_handoff();
  return a.dtype == kF32 ? fwd_impl<float>(a, s) : fwd_impl<uint16_t>(a, s);
}

hipError_t bn_apply(const void* x, const void* residual, void* y, int dtype, const float* scale, const float* shift,
                    int64_t M, int C, int relu, hipStream_t s) {
  if (M <= 0 || C <= 0 || C > bn_max_channels()) return hipErrorInvalidValue;
  return dtype == kF32 ? apply_impl<float>(x, residual, y, scale, shift, M, C, relu, s)
                       : apply_impl<uint16_t>(x, residual, y, scale, shift, M, C, relu, s);
}

hipError_t bn_backward(const BnBwdArgs& a0, hipStream_t s) {
  if (a0.M <= 0 || a0.C <= 0 || a0.C > bn_max_channels()) return hipErrorInvalidValue;
  BnBwdArgs a = a0;
  a.p.fence_handoff = fence_handoff();
  return a.dtype == kF32 ? bwd_impl<float>(a, s) : bwd_impl<uint16_t>(a, s);
}

hipError_t bn_sync_stats(const void* x, int dtype, int64_t M, int C, float* workspace, int* tickets, double* rec,
                         hipStream_t s) {
  if (M <= 0 || C <= 0 || C > bn_max_channels()) return hipErrorInvalidValue;
  return dtype == kF32 ? sync_stats_impl<float>(x, M, C, workspace, tickets, rec, fence_handoff(), s)
                       : sync_stats_impl<uint16_t>(x, M, C, workspace, tickets, rec, fence_handoff(), s);
}

hipError_t bn_sync_merge(const double* rec, int W, int C, const BnParams& p, double* count, hipStream_t s) {
  if (W <= 0 || C <= 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(bn_sync_merge_kernel, dim3((C + kThreads - 1) / kThreads), dim3(kThreads), 0, s, rec, W, C, p,
                     count);
  return hipGetLastError();
}

hipError_t bn_sync_backward_reduce(const BnBwdArgs& a0, double* sums, hipStream_t s) {
  if (a0.M <= 0 || a0.C <= 0 || a0.C > bn_max_channels()) return hipErrorInvalidValue;
  BnBwdArgs a = a0;
  a.p.fence_handoff = fence_handoff();
  return a.dtype == kF32 ? sync_reduce_impl<float>(a, sums, s) : sync_reduce_impl<uint16_t>(a, sums, s);
}

hipError_t bn_sync_coef(const double* sums, const double* count, int C, const BnBwdParams& p, hipStream_t s) {
  if (C <= 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(bn_sync_coef_kernel, dim3((C + kThreads - 1) / kThreads), dim3(kThreads), 0, s, sums, count, C,
                     p);
  return hipGetLastError();
}

hipError_t bn_backward_apply_g(const void* g, const void* x, void* dx, int dtype, const float* coef, int64_t M, int C,
                               hipStream_t s) {
  if (M <= 0 || C <= 0 || C > bn_max_channels()) return hipErrorInvalidValue;
  return dtype == kF32 ? apply_g_impl<float>(g, x, dx, coef, M, C, s) : apply_g_impl<uint16_t>(g, x, dx, coef, M, C, s);
}

}  // namespace ptdt
