// Stride-2 1x1 convolution over an NHWC bf16 activation with the batch statistics of its own output in the
// epilogue, and its backward linked to the BatchNorm's (ops/convbn.py, PTDT_CONVBN_S2=1): the downsample
// branches of ResNet-50's layer2-4 (256 -> 512 at 56^2, 512 -> 1024 at 28^2, 1024 -> 2048 at 14^2).
//
// The convolution is the stride-1 GEMM with the activation's rows gathered: output row m' = (n Ho + ho) Wo + wo
// reads the input pixel row (n H + 2 ho) W + 2 wo, K contiguous bf16 values, Ho = (H + 1) / 2, Wo = (W + 1) / 2.
//
//   Y[M', N]  = Xs . W[N, K]^T                                  fp32 MFMA accumulate, bf16 out
//   stats[4, N] (mean, invstd, scale, shift) of the stored bf16 Y, running statistics updated
//   dY[m', n] = fma(A[n], g[m', n], fma(B[n], y[m', n], C[n]))  rounded to bf16, never stored; 0 for m' >= M'
//   dX[n, 2 ho, 2 wo, :] = (dY . W)[m', :], every other pixel of dX = +0
//   dW[N, K]  = dY^T . Xs                                       fixed-order merge, bf16 out
//
// K % 64 == 0, N % 64 == 0, 64 <= K, N <= 4096, H, W >= 1, input pixel rows < 2^31. Three kernels, each 4 waves
// as 2 x 2 of 64 x 64 (v_mfma_f32_16x16x32_bf16), 2 workgroups per CU, two LDS buffers per operand image and one
// barrier per reduction step:
// * forward: conv1x1_pre.hip's tile and epilogue (W rows permuted by pair_channel: 16-B Y stores; centred
//   per-wave partials; ticketed fixed-order merge in double; bn_finish_channel). No operand is transformed, so
//   BOTH images go by LDS-DMA; a thread decodes its four gathered rows once, before the K loop.
// * data gradient: conv1x1_bwd_tiled.hip's loop over N. The lane that holds 8 input channels of row m' owns the
//   pixels (2 ho .. 2 ho + 1, 2 wo .. 2 wo + 1) that lie inside the image: it stores its result to the first and
//   16 B of zeros to the others. Every pixel (h, w) has the one owner (h / 2, w / 2), so dX is written exactly
//   once and completely: no memset, no atomics.
// * weight gradient: conv1x1_bwd_tiled.hip's split-M kernel with the X image LDS-DMA'd from gathered rows (a
//   thread's DMA rows are the rows of its dY chunks: one decode serves both), then conv1x1_bwd_merge.
// Rows m' >= M' read row M' - 1: computed, neither stored nor counted (times dY = 0 in the weight gradient).
#include "bn_finish.h"
#include "bn_merge.h"
#include "common.h"
#include "conv_bwd_tile.h"
#include "handoff.h"
#include "kernels.h"
#include "lds_tile.h"

namespace ptdt {
namespace {

constexpr int kThreads = 256;
constexpr int kTM = 128, kTN = 128;  // forward output tile; dX block rows / channels; dW tile
constexpr int kTK = 64;              // reduction step: K slice (forward), N slice (dX), row block (dW)
constexpr int kWaveRows = 64;        // rows of one statistics partial
constexpr int kImg = 128 * kTK * 2;  // one operand image: [128][64] or [64][128] bf16
constexpr int kLds = 4 * kImg;       // two buffers of two images: 64 KiB
static_assert(3 * kThreads * 8 + 16 <= kLds, "merge scratch");

// floor(n / d) for 0 <= n < 2^31 by one 32 x 32 -> 64 multiply: mul = ceil(2^shift / d), shift = 31 + ceil(log2 d)
// (Granlund & Montgomery 1994, theorem 4.2 with N = 31)
struct FastDiv {
  uint32_t mul;
  int shift;
};
__device__ __forceinline__ int fdiv(int n, FastDiv d) { return (int)(((uint64_t)(uint32_t)n * d.mul) >> d.shift); }

struct S2Geom {
  int H, W, Ho, Wo;
  FastDiv dWo, dHo;
};
struct S2Pix {
  int n, ho, wo;
};
__device__ __forceinline__ S2Pix s2_pixel(const S2Geom& g, int m) {
  const int t = fdiv(m, g.dWo), n = fdiv(t, g.dHo);
  return {n, t - n * g.Ho, m - t * g.Wo};
}
// input pixel row of output row m
__device__ __forceinline__ int s2_in_row(const S2Geom& g, int m) {
  const S2Pix p = s2_pixel(g, m);
  return (p.n * g.H + 2 * p.ho) * g.W + 2 * p.wo;
}
// v[q] without a dynamic register index
__device__ __forceinline__ int pick4(const int (&v)[4], int q) {
  return q == 0 ? v[0] : q == 1 ? v[1] : q == 2 ? v[2] : v[3];
}

// ---- forward: block = (row tile bm) * tn + (channel tile bn)
__global__ void __launch_bounds__(kThreads, 2) conv1x1_s2_bn_kernel(const uint16_t* __restrict__ X,
                                                                    const uint16_t* __restrict__ W,
                                                                    uint16_t* __restrict__ Y, S2Geom geo, int M, int K,
                                                                    int N, int tm, int tn, GemmBnEpi e) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  uint8_t* const ab = smem;             // 2 x [128 m][64 k], rows of 128 B
  uint8_t* const wb = smem + 2 * kImg;  // 2 x [128 n (MFMA row order)][64 k]
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fr = lane & 15, fq = lane >> 4;
  const int wn = w >> 1, wm = w & 1;
  const int bn = (int)(blockIdx.x % tn), bm = (int)(blockIdx.x / tn);
  const int n0 = bn * kTN;
  const int64_t m0 = (int64_t)bm * kTM;

  // this thread's DMA rows of the x image: tile rows (tid >> 3) + 32 i
  int xr[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int64_t m = m0 + (tid >> 3) + 32 * i;
    xr[i] = s2_in_row(geo, m < M ? (int)m : M - 1);
  }
  // W image row r = (wave half r >> 6, tile (r >> 4) & 3, MFMA row r & 15) <-> channel
  auto stage = [&](int t, int buf) {
    stage_rows<128, 2 * kTK, kThreads>(X, K, kTK * t, ab + buf * kImg, w, lane,
                                       [&](int r) { return pick4(xr, r >> 5); });
    stage_rows<128, 2 * kTK, kThreads>(W, K, kTK * t, wb + buf * kImg, w, lane, [&](int r) {
      const int ch = n0 + 64 * (r >> 6) + pair_channel((r >> 4) & 3, r & 15);
      return ch < N ? ch : N - 1;
    });
  };

  f32x4_t acc[4][4];  // [channel tile j][row tile i]
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[j][i] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  const int nt = K / kTK;
  stage(0, 0);
  for (int t = 0; t < nt; ++t) {
    const int cur = t & 1;
    const uint8_t* const at = ab + cur * kImg;
    const uint8_t* const wt = wb + cur * kImg;
    vm_wait<0>();     // this wave's part of slice t landed
    __syncthreads();  // slice t complete; every wave is past its reads of slice t - 1 (the other buffers)
    if (t + 1 < nt) stage(t + 1, cur ^ 1);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int ks = 0; ks < kTK / 32; ++ks) {
      bf16x8_t a[4], b[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) a[j] = read_frag<bf16x8_t, 2 * kTK>(wt, 64 * wn + 16 * j + fr, 4 * ks + fq);
#pragma unroll
      for (int i = 0; i < 4; ++i) b[i] = read_frag<bf16x8_t, 2 * kTK>(at, 64 * wm + 16 * i + fr, 4 * ks + fq);
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[j][i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[j], b[i], acc[j][i], 0, 0, 0);
    }
  }

  // lane (fr, fq) of tiles (2p, 2p + 1), row tile i: row 16 i + fr, channels 32 p + 8 fq .. + 7. The
  // accumulators keep the stored (rounded) values for the statistics.
  bool rowok[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int64_t m = m0 + 64 * wm + 16 * i + fr;
    rowok[i] = m < M;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      const int n = n0 + 64 * wn + 32 * p + 8 * fq;
      u32x4_t pk;
#pragma unroll
      for (int h = 0; h < 4; ++h) {
        f32x4_t& v = acc[2 * p + (h >> 1)][i];
        pk[h] = pack_bf16x2(v[(2 * h) & 3], v[(2 * h + 1) & 3]);
        v[(2 * h) & 3] = __uint_as_float(pk[h] << 16);
        v[(2 * h + 1) & 3] = __uint_as_float(pk[h] & 0xffff0000u);
      }
      if (rowok[i] && n < N) *reinterpret_cast<u32x4_t*>(Y + m * N + n) = pk;
    }
  }

  // 1. wave partials: rows m0 + 64 wm .. + 63 (nvalid of them inside M), this lane's 16 channels summed over
  // its four rows and the 16 lanes of its DPP row
  const int P = 2 * tm;  // partials per channel
  float* const wsS = e.ws;
  float* const wsQ = e.ws + (int64_t)P * N;
  const int64_t left = (int64_t)M - (m0 + kWaveRows * wm);
  const int nvalid = left < 0 ? 0 : (left < kWaveRows ? (int)left : kWaveRows);
  const float inv_n = nvalid > 0 ? 1.f / (float)nvalid : 0.f;
  const int part = 2 * bm + wm;
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float s = 0.f;
#pragma unroll
      for (int i = 0; i < 4; ++i) s += rowok[i] ? acc[j][i][r] : 0.f;
      s = group_sum<16>(s);
      const float mu = s * inv_n;
      float q = 0.f;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float d = rowok[i] ? acc[j][i][r] - mu : 0.f;
        q = fmaf(d, d, q);
      }
      q = group_sum<16>(q);
      const int c = n0 + 64 * wn + pair_channel(j, 4 * fq + r);
      if (fr == 0 && c < N) {
        st_sc1(wsS + (int64_t)part * N + c, s);
        st_sc1(wsQ + (int64_t)part * N + c, q);
      }
    }

  // 2. group merge by the group's last row tile (its first barrier also ends every wave's fragment reads: the
  // LDS is scratch from here on)
  double* const sh = reinterpret_cast<double*>(smem);
  int* const flag = reinterpret_cast<int*>(smem + 3 * kThreads * sizeof(double));
  const int G = e.group, ng = (tm + G - 1) / G;
  const int gi = bm / G;
  const int g_first = gi * G, g_count = min(G, tm - g_first);
  if (!last_arrival(e.tickets + gi * tn + bn, g_count, flag)) return;
  double n, S, Q;
  auto rows_in = [&](int64_t first, int64_t span) {
    const int64_t l = (int64_t)M - first;
    return (int)(l < 0 ? 0 : (l < span ? l : span));
  };
  merge_range<kThreads, kTN>(wsS, wsQ, N, n0, 2 * g_first, 2 * (g_first + g_count),
                             [&](int p) { return rows_in((int64_t)p * kWaveRows, kWaveRows); }, sh, n, S, Q);
  float* const gS = e.ws + (int64_t)2 * P * N;
  float* const gQ = gS + (int64_t)ng * N;
  const int c = n0 + tid;
  if (tid < kTN && c < N) {
    st_sc1(gS + (int64_t)gi * N + c, (float)S);
    st_sc1(gQ + (int64_t)gi * N + c, (float)Q);
  }

  // 3. channel-tile merge by the last group, final coefficients
  if (!last_arrival(e.tickets + ng * tn + bn, ng, flag)) return;
  const int64_t grows = (int64_t)G * kTM;
  merge_range<kThreads, kTN>(gS, gQ, N, n0, 0, ng, [&](int p) { return rows_in(p * grows, grows); }, sh, n, S, Q);
  if (tid < kTN && c < N) {
    const double Md = (double)M;
    const double var = Q / Md > 0.0 ? Q / Md : 0.0;
    bn_finish_channel(e.p, c, S / Md, var, M > 1 ? var * Md / (Md - 1.0) : var);
  }
  if (tid == 0 && bn == 0 && e.p.num_batches_tracked) *e.p.num_batches_tracked += 1;
}

// ---- data gradient: rows m0 .. + 127 of dY . W, channels k0 .. + 127, scattered to dX[Nb, H, W, K];
// block = (row tile) * ktn + (k tile)
__global__ void __launch_bounds__(kThreads, 2) conv1x1_s2_dx_kernel(
    const uint16_t* __restrict__ G, const uint16_t* __restrict__ Y, const uint16_t* __restrict__ W,
    const float* __restrict__ coef, uint16_t* __restrict__ dX, S2Geom geo, int M, int K, int N, int ktn) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  uint8_t* const dyb = smem;             // 2 x [128 m][64 n], rows of 128 B
  uint8_t* const wb = smem + 2 * kImg;   // 2 x [64 n][128 k], rows of 256 B
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fr = lane & 15, fq = lane >> 4, tq = fr >> 2, tp = fr & 3;
  const int wm = w >> 1, wk = w & 1;
  const int k0 = (int)(blockIdx.x % ktn) * kTN;
  const int64_t m0 = (int64_t)(blockIdx.x / ktn) * kTM;

  // this thread's dY chunks: rows (tid >> 3) + 32 i, channels 8 cc .. + 7 of every slice
  const int cc = tid & 7, r0 = tid >> 3;
  int64_t roff[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int64_t m = m0 + r0 + 32 * i;
    roff[i] = (m < M ? m : (int64_t)M - 1) * N + 8 * cc;  // edge rows are computed and never stored
  }
  u32x4_t gv[4], yv[4];
  Coef8 ck;
  auto load = [&](int t) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      gv[i] = *reinterpret_cast<const u32x4_t*>(G + roff[i] + kTK * t);
      yv[i] = *reinterpret_cast<const u32x4_t*>(Y + roff[i] + kTK * t);
    }
    ck = load_coef(coef, N, kTK * t + 8 * cc);
  };
  auto stage = [&](int t, uint8_t* img) {
    stage_image<kThreads>(W, K, k0, K - 8, img, w, lane, [&](int r) { return kTK * t + r; });
  };

  f32x4_t acc[4][4];  // [channel tile j][row tile i]
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[j][i] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  const int nt = N / kTK;
  load(0);
  stage(0, wb);
  for (int t = 0; t < nt; ++t) {
    const int cur = t & 1;
    uint8_t* const dyt = dyb + cur * kImg;
    const uint8_t* const wt = wb + cur * kImg;
#pragma unroll
    for (int i = 0; i < 4; ++i)
      *reinterpret_cast<u32x4_t*>(dyt + tile_off<128>(r0 + 32 * i, cc)) = dy_chunk(gv[i], yv[i], ck, true);
    vm_wait<0>();     // this wave's part of W slice t landed
    __syncthreads();  // slice t complete; every wave is past its reads of slice t - 1 (the other buffers)
    if (t + 1 < nt) {
      load(t + 1);
      stage(t + 1, wb + (cur ^ 1) * kImg);
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int ks = 0; ks < kTK / 32; ++ks) {
      const int rb = 32 * ks + 8 * fq + tq;
      bf16x8_t a[4], b[4];
      // W^T tile j, row i <-> channel 64 wk + pair_channel(j, i) (conv1x1_bwd_tiled.hip)
#pragma unroll
      for (int j = 0; j < 4; ++j) a[j] = read_tr(wt, rb, 8 * wk + 4 * (j >> 1) + tp, j & 1);
#pragma unroll
      for (int i = 0; i < 4; ++i) b[i] = read_frag<bf16x8_t, 128>(dyt, 64 * wm + 16 * i + fr, 4 * ks + fq);
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[j][i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[j], b[i], acc[j][i], 0, 0, 0);
    }
  }

  // lane (fr, fq) of tiles (2p, 2p + 1), row tile i: row 16 i + fr, channels 32 p + 8 fq .. + 7, to pixel
  // (2 ho, 2 wo); zeros to the pixels right of, below and diagonal to it that the image has
  const int64_t rowK = (int64_t)geo.W * K;
  const u32x4_t zero = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int64_t m = m0 + 64 * wm + 16 * i + fr;
    if (m >= M) continue;
    const S2Pix px = s2_pixel(geo, (int)m);
    const bool right = 2 * px.wo + 1 < geo.W, below = 2 * px.ho + 1 < geo.H;
    uint16_t* const base = dX + (((int64_t)px.n * geo.H + 2 * px.ho) * geo.W + 2 * px.wo) * K;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      const int k = k0 + 64 * wk + 32 * p + 8 * fq;
      if (k >= K) continue;
      u32x4_t pk;
#pragma unroll
      for (int h = 0; h < 4; ++h) {
        const f32x4_t& v = acc[2 * p + (h >> 1)][i];
        const f32x2_t f = {v[(2 * h) & 3], v[(2 * h + 1) & 3]};
        pk[h] = __builtin_bit_cast(uint32_t, __builtin_convertvector(f, bf16x2_t));
      }
      *reinterpret_cast<u32x4_t*>(base + k) = pk;
      if (right) *reinterpret_cast<u32x4_t*>(base + K + k) = zero;
      if (below) *reinterpret_cast<u32x4_t*>(base + rowK + k) = zero;
      if (right && below) *reinterpret_cast<u32x4_t*>(base + rowK + K + k) = zero;
    }
  }
}

// ---- weight gradient: partial of dW[n0 .. +127][k0 .. +127] over the row blocks of split s,
// block = s * tiles + (n tile) * ktn + (k tile)
__global__ void __launch_bounds__(kThreads, 2) conv1x1_s2_dw_kernel(
    const uint16_t* __restrict__ G, const uint16_t* __restrict__ Y, const uint16_t* __restrict__ X,
    const float* __restrict__ coef, float* __restrict__ ws, S2Geom geo, int M, int K, int N, int ktn, int tiles,
    int S) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  uint8_t* const dyb = smem;            // 2 x [64 m][128 n]
  uint8_t* const xb = smem + 2 * kImg;  // 2 x [64 m][128 k]
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fr = lane & 15, fq = lane >> 4, tq = fr >> 2, tp = fr & 3;
  const int wn = w >> 1, wk = w & 1;
  const int tile = (int)(blockIdx.x % tiles), s = (int)(blockIdx.x / tiles);
  const int n0 = (tile / ktn) * kTN, k0 = (tile % ktn) * kTN;
  const int nblk = (int)(((int64_t)M + kTK - 1) / kTK);
  const int b0 = (int)((int64_t)s * nblk / S), b1 = (int)((int64_t)(s + 1) * nblk / S);

  // this thread's dY chunks: rows (tid >> 4) + 16 i of a block, channels nc .. nc + 7 of the tile; the same
  // rows are its DMA rows of the X image (xr: their gathered input pixel rows)
  const int cc = tid & 15, r0 = tid >> 4;
  const int nc = n0 + 8 * cc < N ? n0 + 8 * cc : N - 8;  // a tile past N: valid columns, nothing stored
  const Coef8 ck = load_coef(coef, N, nc);
  u32x4_t gv[4], yv[4];
  bool valid[4];
  int xr[4];
  auto load = [&](int b) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int64_t m = (int64_t)b * kTK + r0 + 16 * i;
      valid[i] = m < M;
      const int mc = valid[i] ? (int)m : M - 1;  // X row M - 1 times dY = 0
      const int64_t off = (int64_t)mc * N + nc;
      gv[i] = *reinterpret_cast<const u32x4_t*>(G + off);
      yv[i] = *reinterpret_cast<const u32x4_t*>(Y + off);
      xr[i] = s2_in_row(geo, mc);
    }
  };
  auto stage = [&](uint8_t* img) {
    stage_image<kThreads>(X, K, k0, K - 8, img, w, lane, [&](int r) { return pick4(xr, r >> 4); });
  };

  f32x4_t acc[4][4];  // [n tile a][k tile t]
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[a][t] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  if (b0 < b1) {
    load(b0);
    stage(xb);
  }
  for (int b = b0; b < b1; ++b) {
    const int cur = (b - b0) & 1;
    uint8_t* const dyt = dyb + cur * kImg;
    const uint8_t* const xt = xb + cur * kImg;
#pragma unroll
    for (int i = 0; i < 4; ++i)
      *reinterpret_cast<u32x4_t*>(dyt + tile_off<256>(r0 + 16 * i, cc)) = dy_chunk(gv[i], yv[i], ck, valid[i]);
    vm_wait<0>();     // this wave's part of X block b landed
    __syncthreads();  // block b complete; every wave is past its reads of block b - 1 (the other buffers)
    if (b + 1 < b1) {
      load(b + 1);
      stage(xb + (cur ^ 1) * kImg);
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int ks = 0; ks < kTK / 32; ++ks) {
      const int rb = 32 * ks + 8 * fq + tq;
      bf16x8_t af[4], bfv[4];
      // lane group tp addresses columns 16 t + 4 tp .. + 3: half (tp & 1) of chunk 2 t + (tp >> 1)
#pragma unroll
      for (int a = 0; a < 4; ++a) af[a] = read_tr(dyt, rb, 8 * wn + 2 * a + (tp >> 1), tp & 1);
#pragma unroll
      for (int t = 0; t < 4; ++t) bfv[t] = read_tr(xt, rb, 8 * wk + 2 * t + (tp >> 1), tp & 1);
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int t = 0; t < 4; ++t)
          acc[a][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[a], bfv[t], acc[a][t], 0, 0, 0);
    }
  }

  // lane (fr, fq) of tile (a, t): dW[n = 16 a + 4 fq + r][k = 16 t + fr]; an empty range stores zeros
  float* const wp = ws + (int64_t)s * N * K;
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int n = n0 + 64 * wn + 16 * a + 4 * fq + r, k = k0 + 64 * wk + 16 * t + fr;
        if (n < N && k < K) wp[(int64_t)n * K + k] = acc[a][t][r];
      }
}

int ceil_div(int64_t a, int b) { return (int)((a + b - 1) / b); }

// row tiles per merge group: ceil(sqrt(tm)), so group merges and the final merge read alike
int s2_group(int tm) {
  int G = 1;
  while ((int64_t)G * G < tm) ++G;
  return G;
}

FastDiv fast_div(int d) {
  int l = 0;
  while (((int64_t)1 << l) < d) ++l;
  const uint64_t p = (uint64_t)1 << (31 + l);
  return {(uint32_t)((p + (uint64_t)d - 1) / (uint64_t)d), 31 + l};
}

// false: the shape is outside the kernels' range
bool s2_geometry(int Nb, int H, int W, S2Geom& g, int& M) {
  if (Nb < 1 || H < 1 || W < 1 || (int64_t)Nb * H * W >= ((int64_t)1 << 31)) return false;
  g.H = H, g.W = W, g.Ho = (H + 1) / 2, g.Wo = (W + 1) / 2;
  g.dWo = fast_div(g.Wo), g.dHo = fast_div(g.Ho);
  M = Nb * g.Ho * g.Wo;
  return true;
}

template <class Kern>
hipError_t allow_lds(Kern* kern) {
  return hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, kLds);
}

}  // namespace

bool conv1x1_s2_supported(int K, int N) { return conv1x1_bwd_tiled_supported(K, N); }

int64_t conv1x1_s2_ws_floats(int Mout, int K, int N) {
  if (Mout <= 0 || !conv1x1_s2_supported(K, N)) return 0;
  const int tm = ceil_div(Mout, kTM);
  return (int64_t)2 * N * ((int64_t)2 * tm + ceil_div(tm, s2_group(tm)));
}

int64_t conv1x1_s2_num_tickets(int Mout, int K, int N) {
  if (Mout <= 0 || !conv1x1_s2_supported(K, N)) return 0;
  const int tm = ceil_div(Mout, kTM);
  return (int64_t)(ceil_div(tm, s2_group(tm)) + 1) * ceil_div(N, kTN);
}

int conv1x1_s2_bwd_splits(int Mout, int K, int N) { return conv1x1_bwd_tiled_splits(Mout, K, N); }

int64_t conv1x1_s2_bwd_ws_floats(int Mout, int K, int N) { return (int64_t)conv1x1_s2_bwd_splits(Mout, K, N) * N * K; }

hipError_t conv1x1_s2_bn_stats(const void* x, const void* w, void* y, int Nb, int H, int W, int K, int N, GemmBnEpi e,
                               hipStream_t s) {
  S2Geom g;
  int M;
  if (!s2_geometry(Nb, H, W, g, M) || !conv1x1_s2_supported(K, N) || e.ws == nullptr || e.tickets == nullptr ||
      e.p.mean == nullptr || e.p.invstd == nullptr || e.p.scale == nullptr || e.p.shift == nullptr)
    return hipErrorInvalidValue;
  if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(w) | reinterpret_cast<uintptr_t>(y)) & 15)
    return hipErrorInvalidValue;
  static bool attr = false;
  if (!attr) {
    PTDT_HIP_CHECK(allow_lds(&conv1x1_s2_bn_kernel));
    attr = true;
  }
  const int tm = ceil_div(M, kTM), tn = ceil_div(N, kTN);  // <= 2^24 row tiles x <= 32 channel tiles
  e.group = s2_group(tm);
  hipLaunchKernelGGL(conv1x1_s2_bn_kernel, dim3((unsigned)((int64_t)tm * tn)), dim3(kThreads), kLds, s,
                     static_cast<const uint16_t*>(x), static_cast<const uint16_t*>(w), static_cast<uint16_t*>(y), g, M,
                     K, N, tm, tn, e);
  return hipGetLastError();
}

hipError_t conv1x1_s2_bwd(const void* g, const void* y, const void* x, const void* w, const float* coef, void* dx,
                          void* dw, float* ws, int Nb, int H, int W, int K, int N, hipStream_t s) {
  S2Geom geo;
  int M;
  if (!s2_geometry(Nb, H, W, geo, M) || ws == nullptr || !conv1x1_s2_supported(K, N)) return hipErrorInvalidValue;
  if ((reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(x) |
       reinterpret_cast<uintptr_t>(w) | reinterpret_cast<uintptr_t>(dx) | reinterpret_cast<uintptr_t>(dw) |
       reinterpret_cast<uintptr_t>(ws) | reinterpret_cast<uintptr_t>(coef)) & 15)
    return hipErrorInvalidValue;
  static bool attr = false;
  if (!attr) {
    PTDT_HIP_CHECK(allow_lds(&conv1x1_s2_dx_kernel));
    PTDT_HIP_CHECK(allow_lds(&conv1x1_s2_dw_kernel));
    attr = true;
  }
  const int ktn = ceil_div(K, kTN), tiles = ceil_div(N, kTN) * ktn;
  const int S = conv1x1_s2_bwd_splits(M, K, N);
  const int64_t mt = ceil_div(M, kTM);  // <= 2^24 row tiles x <= 32 k tiles
  hipLaunchKernelGGL(conv1x1_s2_dx_kernel, dim3((unsigned)(mt * ktn)), dim3(kThreads), kLds, s,
                     static_cast<const uint16_t*>(g), static_cast<const uint16_t*>(y),
                     static_cast<const uint16_t*>(w), coef, static_cast<uint16_t*>(dx), geo, M, K, N, ktn);
  PTDT_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(conv1x1_s2_dw_kernel, dim3((unsigned)(S * tiles)), dim3(kThreads), kLds, s,
                     static_cast<const uint16_t*>(g), static_cast<const uint16_t*>(y),
                     static_cast<const uint16_t*>(x), coef, ws, geo, M, K, N, ktn, tiles, S);
  PTDT_HIP_CHECK(hipGetLastError());
  return conv1x1_bwd_merge(ws, S, N * K / 4, dw, s);
}

}  // namespace ptdt
