// Backward of ``BN(conv1x1(X))`` for any K % 64 == 0, N % 64 == 0 up to 4096 (ops/convbn.py,
// PTDT_CONVBN_BWD=all): the shapes the streaming kernel (conv1x1_bwd.hip: W^T and N*K/256 accumulators
// per lane resident) cannot hold. Same operands, results and rounding points:
//
//   dY[m, n] = fma(A[n], g[m, n], fma(B[n], y[m, n], C[n]))   rounded to bf16, never stored; 0 for m >= M
//   dX[M, K] = dY . W                                          fp32 accumulate, bf16 out
//   dW[N, K] = dY^T . X                                        fp32 accumulate, fixed-order merge, bf16 out
//              (pre given: dY^T . a, a = bf16(max(fmaf(X, scale, shift), 0)) recomputed, conv1x1_pre.hip)
//
// Two tiled MFMA kernels (v_mfma_f32_16x16x32_bf16, 4 waves as 2 x 2 of 64 x 64, 2 workgroups per CU),
// each forming dY in its operand path, then conv1x1_bwd.hip's merge kernel:
//
// * data gradient (reduction over N in slices of 64): a workgroup owns a 128 x 128 block of dX. Each
//   thread loads four 16-B chunks of g and y of the NEXT slice (and the 8 channels' coefficients) before
//   the MFMAs of the current one, applies the coefficients and writes bf16 chunks to a swizzled
//   [128 m][64 n] tile -- the MFMA B operand, one ds_read_b128 per fragment. The W slice [64 n][128 k] is
//   LDS-DMA'd as it stands; W^T is the A operand, read with ds_read_b64_tr_b16, columns picked by
//   pair_channel so a lane ends up with 8 consecutive input channels of one row: 16-B dX stores.
// * weight gradient (reduction over M): a workgroup owns a 128 x 128 tile of dW and one of S contiguous
//   ranges of 64-row blocks. Per block a dY image [64 m][128 n] (register path, this thread's 8 channels'
//   coefficients held for the whole launch) and an X image [64 m][128 k] (LDS-DMA); both operands are
//   column slices of row-major images, read with the transposing LDS read. The accumulators stay in
//   registers over the range and go to ws[split][N][K] with plain stores; S depends on (M, K, N) only.
//
// Both loops run over two buffers of each image with one barrier per step: step t's images are written /
// DMA'd before the barrier, step t+1's global loads and DMA are issued right after it. A channel tile
// that sticks out of K or N (K or N an odd multiple of 64) reads clamped, valid columns and stores
// nothing for them.
#include "common.h"
#include "conv_bwd_tile.h"
#include "kernels.h"
#include "lds_tile.h"

namespace ptdt {
namespace {

constexpr int kThreads = 256;
constexpr int kTM = 128;            // rows of a dX block
constexpr int kTC = 128;            // channels of a tile (K of dX; N and K of dW)
constexpr int kTS = 64;             // reduction step: channels n of a slice (dX), rows of a block (dW)
constexpr int kImg = 64 * 256;      // one image: [64][128] or [128][64] bf16
constexpr int kLds = 4 * kImg;      // two buffers of two images: 64 KiB
constexpr int kTargetWgs = 384;     // weight-gradient grid: 1.5 workgroups per CU of a 256-CU part
constexpr int kMinBlocks = 4;       // row blocks per split at least (amortises the 64-KiB partial)
constexpr int64_t kWsFloats = 8 << 20;  // workspace cap (32 MiB) unless one partial alone is larger

// The fragment of the recomputed operand a = bf16(max(fmaf(x, scale, shift), 0)) (conv1x1_pre.hip) from a
// read_tr fragment of x: one channel (this lane's scale / shift) over 8 rows.
__device__ __forceinline__ bf16x8_t pre_frag(bf16x8_t xf, float sc, float sf) {
  const u32x4_t xv = __builtin_bit_cast(u32x4_t, xf);
  u32x4_t pk;
#pragma unroll
  for (int h = 0; h < 4; ++h)
    pk[h] = pack_bf16x2(fmaxf(fmaf(__uint_as_float(xv[h] << 16), sc, sf), 0.f),
                        fmaxf(fmaf(__uint_as_float(xv[h] & 0xffff0000u), sc, sf), 0.f));
  return __builtin_bit_cast(bf16x8_t, pk);
}

// ---- data gradient: dX[m0 .. +127][k0 .. +127], block = (row tile) * ktn + (k tile)
__global__ void __launch_bounds__(kThreads, 2) conv1x1_bwd_tiled_dx_kernel(
    const uint16_t* __restrict__ G, const uint16_t* __restrict__ Y, const uint16_t* __restrict__ W,
    const float* __restrict__ coef, uint16_t* __restrict__ dX, int M, int K, int N, int ktn) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  uint8_t* const dyb = smem;             // 2 x [128 m][64 n], rows of 128 B
  uint8_t* const wb = smem + 2 * kImg;   // 2 x [64 n][128 k], rows of 256 B
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fr = lane & 15, fq = lane >> 4, tq = fr >> 2, tp = fr & 3;
  const int wm = w >> 1, wk = w & 1;
  const int k0 = (int)(blockIdx.x % ktn) * kTC;
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
      gv[i] = *reinterpret_cast<const u32x4_t*>(G + roff[i] + kTS * t);
      yv[i] = *reinterpret_cast<const u32x4_t*>(Y + roff[i] + kTS * t);
    }
    ck = load_coef(coef, N, kTS * t + 8 * cc);
  };
  auto stage = [&](int t, uint8_t* img) {
    stage_image<kThreads>(W, K, k0, K - 8, img, w, lane, [&](int r) { return kTS * t + r; });
  };

  f32x4_t acc[4][4];  // [channel tile j][row tile i]
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[j][i] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  const int nt = N / kTS;
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
    for (int ks = 0; ks < kTS / 32; ++ks) {
      const int rb = 32 * ks + 8 * fq + tq;
      bf16x8_t a[4], b[4];
      // W^T tile j, row i <-> channel 64 wk + pair_channel(j, i): lane group tp addresses channels
      // 32 (j >> 1) + 8 tp + 4 (j & 1) .. + 3, half (j & 1) of chunk 8 wk + 4 (j >> 1) + tp
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

  // lane (fr, fq) of tiles (2p, 2p + 1), row tile i: row 16 i + fr, channels 32 p + 8 fq .. + 7
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int64_t m = m0 + 64 * wm + 16 * i + fr;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      const int k = k0 + 64 * wk + 32 * p + 8 * fq;
      u32x4_t pk;
#pragma unroll
      for (int h = 0; h < 4; ++h) {
        const f32x4_t& v = acc[2 * p + (h >> 1)][i];
        const f32x2_t f = {v[(2 * h) & 3], v[(2 * h + 1) & 3]};
        pk[h] = __builtin_bit_cast(uint32_t, __builtin_convertvector(f, bf16x2_t));
      }
      if (m < M && k < K) *reinterpret_cast<u32x4_t*>(dX + m * K + k) = pk;
    }
  }
}

// ---- weight gradient: partial of dW[n0 .. +127][k0 .. +127] over the row blocks of split s,
// block = s * tiles + (n tile) * ktn + (k tile). PRE: X is the input of a BatchNorm + ReLU (pre = its
// scale[K], shift[K]) and the product takes a = bf16(max(fmaf(x, scale, shift), 0)), formed on the X
// fragments: a lane's fragment of k tile t is channel 16 t + fr over 8 rows, so its 4 + 4 coefficients
// serve the whole launch.
template <bool PRE>
__global__ void __launch_bounds__(kThreads, 2) conv1x1_bwd_tiled_dw_kernel(
    const uint16_t* __restrict__ G, const uint16_t* __restrict__ Y, const uint16_t* __restrict__ X,
    const float* __restrict__ coef, const float* __restrict__ pre, float* __restrict__ ws, int M, int K, int N,
    int ktn, int tiles, int S) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  uint8_t* const dyb = smem;            // 2 x [64 m][128 n]
  uint8_t* const xb = smem + 2 * kImg;  // 2 x [64 m][128 k]
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fr = lane & 15, fq = lane >> 4, tq = fr >> 2, tp = fr & 3;
  const int wn = w >> 1, wk = w & 1;
  const int tile = (int)(blockIdx.x % tiles), s = (int)(blockIdx.x / tiles);
  const int n0 = (tile / ktn) * kTC, k0 = (tile % ktn) * kTC;
  const int nblk = (int)(((int64_t)M + kTS - 1) / kTS);
  const int b0 = (int)((int64_t)s * nblk / S), b1 = (int)((int64_t)(s + 1) * nblk / S);

  // this thread's dY chunks: rows (tid >> 4) + 16 i of a block, channels nc .. nc + 7 of the tile
  const int cc = tid & 15, r0 = tid >> 4;
  const int nc = n0 + 8 * cc < N ? n0 + 8 * cc : N - 8;  // a tile past N: valid columns, nothing stored
  const Coef8 ck = load_coef(coef, N, nc);
  u32x4_t gv[4], yv[4];
  bool valid[4];
  auto load = [&](int b) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int64_t m = (int64_t)b * kTS + r0 + 16 * i;
      valid[i] = m < M;
      const int64_t off = (valid[i] ? m : (int64_t)M - 1) * N + nc;
      gv[i] = *reinterpret_cast<const u32x4_t*>(G + off);
      yv[i] = *reinterpret_cast<const u32x4_t*>(Y + off);
    }
  };
  auto stage = [&](int b, uint8_t* img) {
    stage_image<kThreads>(X, K, k0, K - 8, img, w, lane, [&](int r) {
      const int64_t m = (int64_t)b * kTS + r;
      return m < M ? m : (int64_t)M - 1;  // times dY = 0
    });
  };

  float psc[4], psf[4];
  if constexpr (PRE) {
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int k = k0 + 64 * wk + 16 * t + fr;
      psc[t] = pre[k < K ? k : K - 1];  // a tile past K: valid coefficients, nothing stored
      psf[t] = pre[K + (k < K ? k : K - 1)];
    }
  }

  f32x4_t acc[4][4];  // [n tile a][k tile t]
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[a][t] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  if (b0 < b1) {
    load(b0);
    stage(b0, xb);
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
      stage(b + 1, xb + (cur ^ 1) * kImg);
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int ks = 0; ks < kTS / 32; ++ks) {
      const int rb = 32 * ks + 8 * fq + tq;
      bf16x8_t af[4], bfv[4];
      // lane group tp addresses columns 16 t + 4 tp .. + 3: half (tp & 1) of chunk 2 t + (tp >> 1)
#pragma unroll
      for (int a = 0; a < 4; ++a) af[a] = read_tr(dyt, rb, 8 * wn + 2 * a + (tp >> 1), tp & 1);
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        bfv[t] = read_tr(xt, rb, 8 * wk + 2 * t + (tp >> 1), tp & 1);
        if constexpr (PRE) bfv[t] = pre_frag(bfv[t], psc[t], psf[t]);
      }
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

int ceil_div(int a, int b) { return (a + b - 1) / b; }

template <bool PRE>
hipError_t launch_dw(const void* g, const void* y, const void* x, const float* coef, const float* pre, float* ws, int M,
                     int K, int N, int ktn, int tiles, int S, hipStream_t s) {
  static bool attr = false;
  if (!attr) {
    PTDT_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&conv1x1_bwd_tiled_dw_kernel<PRE>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, kLds));
    attr = true;
  }
  hipLaunchKernelGGL(conv1x1_bwd_tiled_dw_kernel<PRE>, dim3((unsigned)(S * tiles)), dim3(kThreads), kLds, s,
                     static_cast<const uint16_t*>(g), static_cast<const uint16_t*>(y),
                     static_cast<const uint16_t*>(x), coef, pre, ws, M, K, N, ktn, tiles, S);
  return hipGetLastError();
}

}  // namespace

bool conv1x1_bwd_tiled_supported(int K, int N) {
  return K >= 64 && N >= 64 && K <= 4096 && N <= 4096 && K % 64 == 0 && N % 64 == 0;
}

int conv1x1_bwd_tiled_splits(int M, int K, int N) {
  if (M <= 0 || !conv1x1_bwd_tiled_supported(K, N)) return 0;
  const int64_t nblk = ((int64_t)M + kTS - 1) / kTS;
  int64_t S = kTargetWgs / (ceil_div(N, kTC) * ceil_div(K, kTC));
  if (S > nblk / kMinBlocks) S = nblk / kMinBlocks;
  if (S > kWsFloats / ((int64_t)N * K)) S = kWsFloats / ((int64_t)N * K);
  return S < 1 ? 1 : (int)S;
}

int64_t conv1x1_bwd_tiled_ws_floats(int M, int K, int N) {
  return (int64_t)conv1x1_bwd_tiled_splits(M, K, N) * N * K;
}

hipError_t conv1x1_bwd_tiled(const void* g, const void* y, const void* x, const void* w, const float* coef,
                             const float* pre, void* dx, void* dw, float* ws, int M, int K, int N, hipStream_t s) {
  if (M <= 0 || ws == nullptr || !conv1x1_bwd_tiled_supported(K, N)) return hipErrorInvalidValue;
  if ((reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(x) |
       reinterpret_cast<uintptr_t>(w) | reinterpret_cast<uintptr_t>(dx) | reinterpret_cast<uintptr_t>(dw) |
       reinterpret_cast<uintptr_t>(ws) | reinterpret_cast<uintptr_t>(coef) | reinterpret_cast<uintptr_t>(pre)) & 15)
    return hipErrorInvalidValue;
  static bool attr = false;
  if (!attr) {
    PTDT_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&conv1x1_bwd_tiled_dx_kernel),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, kLds));
    attr = true;
  }
  const int ktn = ceil_div(K, kTC), tiles = ceil_div(N, kTC) * ktn;
  const int S = conv1x1_bwd_tiled_splits(M, K, N);
  const int64_t mt = ((int64_t)M + kTM - 1) / kTM;  // <= 2^24 row tiles x <= 32 k tiles
  hipLaunchKernelGGL(conv1x1_bwd_tiled_dx_kernel, dim3((unsigned)(mt * ktn)), dim3(kThreads), kLds, s,
                     static_cast<const uint16_t*>(g), static_cast<const uint16_t*>(y),
                     static_cast<const uint16_t*>(w), coef, static_cast<uint16_t*>(dx), M, K, N, ktn);
  PTDT_HIP_CHECK(hipGetLastError());
  PTDT_HIP_CHECK(pre ? launch_dw<true>(g, y, x, coef, pre, ws, M, K, N, ktn, tiles, S, s)
                     : launch_dw<false>(g, y, x, coef, pre, ws, M, K, N, ktn, tiles, S, s));
  return conv1x1_bwd_merge(ws, S, N * K / 4, dw, s);
}

}  // namespace ptdt
