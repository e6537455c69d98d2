// 1x1 convolution whose input is a training BatchNorm + ReLU that is never stored, with the batch statistics
// of its own output in the epilogue (ops/convbn.py, PTDT_CONVBN_PRE=1): ResNet-50's conv2 -> bn2 -> ReLU ->
// conv3 -> bn3 without bn2's apply pass and without the activation it writes.
//
//   a[m, k] = bf16(max(fmaf(x[m, k], scale[k], shift[k]), 0))    bn_apply_kernel's rounding point; never stored
//   Y[M, N] = a . W[N, K]^T                                       fp32 MFMA accumulate, bf16 out
//   stats[4, N] (mean, invstd, scale, shift) of the stored bf16 Y, running statistics updated
//
// K % 64 == 0, N % 64 == 0, 64 <= K, N <= 4096, 1 <= M < 2^31 (conv1x1_bwd_tiled_supported).
//
// A workgroup (4 waves as 2 x 2 of 64 x 64, v_mfma_f32_16x16x32_bf16, 2 workgroups per CU) owns a 128 x 128
// tile of Y and steps K in slices of 64 over two LDS buffers of each operand, one barrier per slice:
// * x goes through registers: a thread loads its four 16-B chunks of slice t + 1 and their 8 channels' scale /
//   shift before the MFMAs of slice t, transforms them and writes bf16 chunks to a swizzled [128 m][64 k]
//   image, the MFMA B operand;
// * W goes by LDS-DMA. Its rows are permuted by pair_channel on the way in and W is the A operand, so a lane
//   ends up with 8 consecutive output channels of one row: Y leaves in 16-B stores, no LDS epilogue;
// * statistics as gemm_bn_stats (gemm_big.hip): centred partials per wave (64 rows x 64 channels, over the
//   stored bf16 values), merged in a fixed order in double by the last workgroup of each group of row tiles and
//   then by the last group of the column tile (bn_merge.h, tickets re-armed to zero), bn_finish_channel.
// Rows m >= M read row M - 1: computed, neither stored nor counted. A channel tile that sticks out of N (N an
// odd multiple of 64) reads valid weight rows and stores nothing for them.
#include "bn_finish.h"
#include "bn_merge.h"
#include "common.h"
#include "handoff.h"
#include "kernels.h"
#include "lds_tile.h"

namespace ptdt {
namespace {

typedef __attribute__((ext_vector_type(4))) unsigned u32x4_t;

constexpr int kThreads = 256;
constexpr int kTM = 128, kTN = 128;  // output tile
constexpr int kTK = 64;              // K slice
constexpr int kWaveRows = 64;        // rows of one statistics partial
constexpr int kImg = 128 * kTK * 2;  // one operand image: [128][64] bf16
constexpr int kLds = 4 * kImg;       // two buffers of two images: 64 KiB
static_assert(3 * kThreads * 8 + 16 <= kLds, "merge scratch");

struct Pre8 {
  f32x4_t sc[2], sf[2];
};
// scale / shift of channels k .. k + 7 (k % 8 == 0)
__device__ __forceinline__ Pre8 load_pre(const float* __restrict__ scale, const float* __restrict__ shift, int k) {
  Pre8 p;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    p.sc[h] = *reinterpret_cast<const f32x4_t*>(scale + k + 4 * h);
    p.sf[h] = *reinterpret_cast<const f32x4_t*>(shift + k + 4 * h);
  }
  return p;
}
// 8 channels of a from a 16-B chunk of x
__device__ __forceinline__ u32x4_t pre_chunk(u32x4_t xv, const Pre8& p) {
  float a[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const float x = bf16_to_f32((uint16_t)(xv[e >> 1] >> (16 * (e & 1))));
    a[e] = fmaxf(fmaf(x, p.sc[e >> 2][e & 3], p.sf[e >> 2][e & 3]), 0.f);
  }
  u32x4_t pk;
#pragma unroll
  for (int h = 0; h < 4; ++h) pk[h] = pack_bf16x2(a[2 * h], a[2 * h + 1]);
  return pk;
}

// block = (row tile bm) * tn + (channel tile bn)
__global__ void __launch_bounds__(kThreads, 2) conv1x1_pre_kernel(const uint16_t* __restrict__ X,
                                                                  const float* __restrict__ scale,
                                                                  const float* __restrict__ shift,
                                                                  const uint16_t* __restrict__ W,
                                                                  uint16_t* __restrict__ Y, int M, int K, int N,
                                                                  int tm, int tn, GemmBnEpi e) {
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

  // this thread's x chunks: rows (tid >> 3) + 32 i, channels 8 cc .. + 7 of every slice
  const int cc = tid & 7, r0 = tid >> 3;
  int64_t roff[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int64_t m = m0 + r0 + 32 * i;
    roff[i] = (m < M ? m : (int64_t)M - 1) * K + 8 * cc;
  }
  u32x4_t xv[4];
  Pre8 pk8;
  auto load = [&](int t) {
#pragma unroll
    for (int i = 0; i < 4; ++i) xv[i] = *reinterpret_cast<const u32x4_t*>(X + roff[i] + kTK * t);
    pk8 = load_pre(scale, shift, kTK * t + 8 * cc);
  };
  // image row r = (wave half r >> 6, tile (r >> 4) & 3, MFMA row r & 15) <-> channel
  auto stage = [&](int t, uint8_t* img) {
    stage_rows<128, 2 * kTK, kThreads>(W, K, kTK * t, img, w, lane, [&](int r) {
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
  load(0);
  stage(0, wb);
  for (int t = 0; t < nt; ++t) {
    const int cur = t & 1;
    uint8_t* const at = ab + cur * kImg;
    const uint8_t* const wt = wb + cur * kImg;
#pragma unroll
    for (int i = 0; i < 4; ++i)
      *reinterpret_cast<u32x4_t*>(at + tile_off<2 * kTK>(r0 + 32 * i, cc)) = pre_chunk(xv[i], pk8);
    vm_wait<0>();     // this wave's part of W slice t landed
    __syncthreads();  // slice t complete; every wave is past its reads of slice t - 1 (the other buffers)
    if (t + 1 < nt) {
      load(t + 1);
      stage(t + 1, wb + (cur ^ 1) * kImg);
    }
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

int ceil_div(int64_t a, int b) { return (int)((a + b - 1) / b); }

// row tiles per merge group: ceil(sqrt(tm)), so group merges and the final merge read alike
int pre_group(int tm) {
  int G = 1;
  while ((int64_t)G * G < tm) ++G;
  return G;
}

}  // namespace

bool conv1x1_pre_supported(int K, int N) { return conv1x1_bwd_tiled_supported(K, N); }

int64_t conv1x1_pre_ws_floats(int M, int K, int N) {
  if (M <= 0 || !conv1x1_pre_supported(K, N)) return 0;
  const int tm = ceil_div(M, kTM);
  return (int64_t)2 * N * ((int64_t)2 * tm + ceil_div(tm, pre_group(tm)));
}

int64_t conv1x1_pre_num_tickets(int M, int K, int N) {
  if (M <= 0 || !conv1x1_pre_supported(K, N)) return 0;
  const int tm = ceil_div(M, kTM);
  return (int64_t)(ceil_div(tm, pre_group(tm)) + 1) * ceil_div(N, kTN);
}

hipError_t conv1x1_pre_bn_stats(const void* x, const float* scale, const float* shift, const void* w, void* y, int M,
                                int K, int N, GemmBnEpi e, hipStream_t s) {
  if (M <= 0 || !conv1x1_pre_supported(K, N) || e.ws == nullptr || e.tickets == nullptr || e.p.mean == nullptr ||
      e.p.invstd == nullptr || e.p.scale == nullptr || e.p.shift == nullptr)
    return hipErrorInvalidValue;
  if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(w) | reinterpret_cast<uintptr_t>(y) |
       reinterpret_cast<uintptr_t>(scale) | reinterpret_cast<uintptr_t>(shift)) & 15)
    return hipErrorInvalidValue;
  static bool attr = false;
  if (!attr) {
    PTDT_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&conv1x1_pre_kernel),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, kLds));
    attr = true;
  }
  const int tm = ceil_div(M, kTM), tn = ceil_div(N, kTN);  // <= 2^24 row tiles x <= 32 channel tiles
  e.group = pre_group(tm);
  hipLaunchKernelGGL(conv1x1_pre_kernel, dim3((unsigned)((int64_t)tm * tn)), dim3(kThreads), kLds, s,
                     static_cast<const uint16_t*>(x), scale, shift, static_cast<const uint16_t*>(w),
                     static_cast<uint16_t*>(y), M, K, N, tm, tn, e);
  return hipGetLastError();
}

}  // namespace ptdt
