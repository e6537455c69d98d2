// 3x3 convolution (stride 1, padding 1) over an NHWC bf16 activation as an implicit GEMM, with the training
// BatchNorm's batch statistics of its own output in the epilogue (ops/convbn.py, PTDT_CONV3X3): ResNet-50's
// conv2 -> bn2 without bn2's statistics pass, and without MIOpen.
//
//   Y[n, h, w, :] = sum over (kh, kw) of X[n, h + kh - 1, w + kw - 1, :] . W[:, kh, kw, :]^T
//   X [N, H, W, Cin], W [Cout, 3, 3, Cin], Y [N, H, W, Cout] bf16; fp32 MFMA accumulate
//   stats[4, Cout] (mean, invstd, scale, shift) of the stored bf16 Y, running statistics updated
//
// Cin % 64 == 0, Cout % 64 == 0, 64 <= Cin, Cout <= 1024, 1 <= M = N H W < 2^31, any H, W >= 1.
//
// The GEMM is Y[M, Cout] = A[M, 9 Cin] . W[Cout, 9 Cin]^T where row m of A is the 3x3 neighbourhood of pixel m,
// tap-major; A is never stored. K is walked as 9 taps x Cin / 64 slices of 64, so a slice lies inside one tap.
// A workgroup (4 waves, v_mfma_f32_16x16x32_bf16) owns a 128-row tile of Y, TN = 128 or 64 channels wide, over
// two LDS buffers of each operand, one barrier per slice:
// * TN = 128: waves as 2 x 2 of 64 rows x 64 channels, 64 KiB of LDS, 2 workgroups per CU;
//   TN = 64: waves as 4 x 1 of 32 rows x 64 channels, 48 KiB, 3 per CU: for Cout = 64 (no idle MFMA half)
//   and for shapes whose 128-wide tiles would leave CUs empty (7^2 x 128 rows at 512 channels: 196 tiles);
// * the activation goes through registers, as conv1x1_pre.hip moves x: a thread owns four tile rows (pixels)
//   and one 16-B chunk position. It decodes each pixel's (h, w) once into a 9-bit mask of the taps that lie
//   inside the image; per slice the source is the pixel's own offset plus a wave-uniform tap offset, and a tap
//   outside the image is a zero chunk. The chunks of slice t + 1 are loaded before the MFMAs of slice t and
//   written to the swizzled [128 m][64 k] image after them. Chosen over LDS-DMA with a zero block as the
//   source of outside taps: it needs no such block (no allocation, nothing to keep valid under graph
//   capture), costs no more LDS traffic, and leaves the register stage where an input BatchNorm + ReLU can
//   be applied later;
// * W [Cout][9 Cin] is K-contiguous and goes by LDS-DMA, rows permuted by pair_channel and W the MFMA A
//   operand, so a lane ends up with 8 consecutive output channels of one pixel: Y leaves in 16-B stores;
// * statistics as conv1x1_pre.hip: centred partials per wave over the stored (rounded) values, merged in a
//   fixed order in double by the last workgroup of each group of row tiles and then by the last group of the
//   channel tile (bn_merge.h, tickets re-armed to zero), bn_finish_channel.
// Rows m >= M are computed from pixel M - 1, neither stored nor counted. A channel tile that sticks out of Cout
// reads valid weight rows and stores nothing for them.
//
// Backward: the BN's native backward, then MIOpen's convolution_backward; or, with PTDT_CONV3X3_BWD=1,
// conv3x3_bwd.hip, which takes this kernel's raw Y (the BN applies later) and the BN's reduce-pass coefficients
// and forms dY = A g + B y + C on the same kind of register stage, with the same tap masks.
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
constexpr int kTM = 128;             // rows (pixels) of a tile
constexpr int kTK = 64;              // K slice
constexpr int kImgA = kTM * kTK * 2;  // activation image: [128][64] bf16

template <int TN>
struct Geo {
  static_assert(TN == 64 || TN == 128, "channel tile");
  static constexpr int kWN = TN / 64;        // waves across channels
  static constexpr int kWM = 4 / kWN;        // waves across rows
  static constexpr int kWR = kTM / kWM;      // rows of a wave = rows of one statistics partial
  static constexpr int kRI = kWR / 16;       // MFMA row tiles of a wave
  static constexpr int kImgW = TN * kTK * 2;  // weight image: [TN][64] bf16
  static constexpr int kLds = 2 * (kImgA + kImgW);
  static constexpr int kOcc = TN == 128 ? 2 : 3;  // workgroups per CU the LDS allows
  static_assert(3 * kThreads * 8 + 16 <= kLds, "merge scratch");
};

// block = (row tile bm) * tn + (channel tile bn)
template <int TN>
__global__ void __launch_bounds__(kThreads, Geo<TN>::kOcc)
    conv3x3_bn_kernel(const uint16_t* __restrict__ X, const uint16_t* __restrict__ W, uint16_t* __restrict__ Y, int M,
                      int H, int Wd, int Cin, int N, int tm, int tn, GemmBnEpi e) {
  using G = Geo<TN>;
  constexpr int kWR = G::kWR, kRI = G::kRI;
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  uint8_t* const ab = smem;              // 2 x [128 m][64 k], rows of 128 B
  uint8_t* const wb = smem + 2 * kImgA;  // 2 x [TN n (MFMA row order)][64 k]
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fr = lane & 15, fq = lane >> 4;
  const int wn = w / G::kWM, wm = w % G::kWM;
  const int bn = (int)(blockIdx.x % tn), bm = (int)(blockIdx.x / tn);
  const int n0 = bn * TN;
  const int64_t m0 = (int64_t)bm * kTM;
  const int K = 9 * Cin;

  // this thread's activation chunks: pixels m0 + (tid >> 3) + 32 i, channels 8 cc .. + 7 of every slice.
  // roff: the pixel's own element offset; ok bit (3 kh + kw): that tap's source pixel is inside the image
  const int cc = tid & 7, r0 = tid >> 3;
  int64_t roff[4];
  unsigned ok[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    int64_t m = m0 + r0 + 32 * i;
    m = m < M ? m : (int64_t)M - 1;
    const int pw = (int)(m % Wd), ph = (int)((m / Wd) % H);
    unsigned bits = 0;
#pragma unroll
    for (int kh = 0; kh < 3; ++kh)
#pragma unroll
      for (int kw = 0; kw < 3; ++kw) {
        const int sh = ph + kh - 1, sw = pw + kw - 1;
        if (sh >= 0 && sh < H && sw >= 0 && sw < Wd) bits |= 1u << (3 * kh + kw);
      }
    ok[i] = bits;
    roff[i] = m * Cin + 8 * cc;
  }
  const int spt = Cin / kTK;  // slices per tap
  u32x4_t xv[4];
  int ltap = 0, lsl = 0;  // tap and slice within it of the next load
  auto load = [&]() {
    const int64_t d = ((int64_t)(ltap / 3 - 1) * Wd + (ltap % 3 - 1)) * Cin + kTK * lsl;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      xv[i] = u32x4_t{0u, 0u, 0u, 0u};
      if ((ok[i] >> ltap) & 1u) xv[i] = *reinterpret_cast<const u32x4_t*>(X + (roff[i] + d));
    }
    if (++lsl == spt) lsl = 0, ++ltap;
  };
  // image row r = (wave r >> 6, tile (r >> 4) & 3, MFMA row r & 15) <-> channel
  auto stage = [&](int t, uint8_t* img) {
    stage_rows<TN, 2 * kTK, kThreads>(W, K, kTK * t, img, w, lane, [&](int r) {
      const int ch = n0 + 64 * (r >> 6) + pair_channel((r >> 4) & 3, r & 15);
      return ch < N ? ch : N - 1;
    });
  };

  f32x4_t acc[4][kRI];  // [channel tile j][row tile i]
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int i = 0; i < kRI; ++i) acc[j][i] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  const int nt = 9 * spt;
  load();
  stage(0, wb);
  for (int t = 0; t < nt; ++t) {
    const int cur = t & 1;
    uint8_t* const at = ab + cur * kImgA;
    const uint8_t* const wt = wb + cur * G::kImgW;
#pragma unroll
    for (int i = 0; i < 4; ++i) *reinterpret_cast<u32x4_t*>(at + tile_off<2 * kTK>(r0 + 32 * i, cc)) = xv[i];
    vm_wait<0>();     // this wave's part of W slice t landed
    __syncthreads();  // slice t complete; every wave is past its reads of slice t - 1 (the other buffers)
    if (t + 1 < nt) {
      load();
      stage(t + 1, wb + (cur ^ 1) * G::kImgW);
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int ks = 0; ks < kTK / 32; ++ks) {
      bf16x8_t a[4], b[kRI];
#pragma unroll
      for (int j = 0; j < 4; ++j) a[j] = read_frag<bf16x8_t, 2 * kTK>(wt, 64 * wn + 16 * j + fr, 4 * ks + fq);
#pragma unroll
      for (int i = 0; i < kRI; ++i) b[i] = read_frag<bf16x8_t, 2 * kTK>(at, kWR * wm + 16 * i + fr, 4 * ks + fq);
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int i = 0; i < kRI; ++i)
          acc[j][i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[j], b[i], acc[j][i], 0, 0, 0);
    }
  }

  // lane (fr, fq) of tiles (2p, 2p + 1), row tile i: row 16 i + fr, channels 32 p + 8 fq .. + 7. The
  // accumulators keep the stored (rounded) values for the statistics.
  bool rowok[kRI];
#pragma unroll
  for (int i = 0; i < kRI; ++i) {
    const int64_t m = m0 + kWR * wm + 16 * i + fr;
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

  // 1. wave partials: rows m0 + kWR wm .. + kWR - 1 (nvalid of them inside M), this lane's 16 channels summed
  // over its row tiles and the 16 lanes of its DPP row
  const int P = G::kWM * tm;  // partials per channel
  float* const wsS = e.ws;
  float* const wsQ = e.ws + (int64_t)P * N;
  const int64_t left = (int64_t)M - (m0 + kWR * wm);
  const int nvalid = left < 0 ? 0 : (left < kWR ? (int)left : kWR);
  const float inv_n = nvalid > 0 ? 1.f / (float)nvalid : 0.f;
  const int part = G::kWM * bm + wm;
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float s = 0.f;
#pragma unroll
      for (int i = 0; i < kRI; ++i) s += rowok[i] ? acc[j][i][r] : 0.f;
      s = group_sum<16>(s);
      const float mu = s * inv_n;
      float q = 0.f;
#pragma unroll
      for (int i = 0; i < kRI; ++i) {
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
  const int Gr = e.group, ng = (tm + Gr - 1) / Gr;
  const int gi = bm / Gr;
  const int g_first = gi * Gr, g_count = min(Gr, tm - g_first);
  if (!last_arrival(e.tickets + gi * tn + bn, g_count, flag)) return;
  double n, S, Q;
  auto rows_in = [&](int64_t first, int64_t span) {
    const int64_t l = (int64_t)M - first;
    return (int)(l < 0 ? 0 : (l < span ? l : span));
  };
  merge_range<kThreads, TN>(wsS, wsQ, N, n0, G::kWM * g_first, G::kWM * (g_first + g_count),
                            [&](int p) { return rows_in((int64_t)p * kWR, kWR); }, sh, n, S, Q);
  float* const gS = e.ws + (int64_t)2 * P * N;
  float* const gQ = gS + (int64_t)ng * N;
  const int c = n0 + tid;
  if (tid < TN && c < N) {
    st_sc1(gS + (int64_t)gi * N + c, (float)S);
    st_sc1(gQ + (int64_t)gi * N + c, (float)Q);
  }

  // 3. channel-tile merge by the last group, final coefficients
  if (!last_arrival(e.tickets + ng * tn + bn, ng, flag)) return;
  const int64_t grows = (int64_t)Gr * kTM;
  merge_range<kThreads, TN>(gS, gQ, N, n0, 0, ng, [&](int p) { return rows_in(p * grows, grows); }, sh, n, S, Q);
  if (tid < TN && c < N) {
    const double Md = (double)M;
    const double var = Q / Md > 0.0 ? Q / Md : 0.0;
    bn_finish_channel(e.p, c, S / Md, var, M > 1 ? var * Md / (Md - 1.0) : var);
  }
  if (tid == 0 && bn == 0 && e.p.num_batches_tracked) *e.p.num_batches_tracked += 1;
}

int ceil_div(int64_t a, int b) { return (int)((a + b - 1) / b); }

// row tiles per merge group: ceil(sqrt(tm)), so group merges and the final merge read alike
int merge_group(int tm) {
  int G = 1;
  while ((int64_t)G * G < tm) ++G;
  return G;
}

// The MI355X's CU count, as a constant: the geometry below also sizes the workspace and the tickets, so it must
// be a function of the shape alone, the same on every device and rank.
constexpr int kChipCUs = 256;

// The channel tile of a shape: 64 where 128 would idle half the MFMAs (Cout = 64) or leave fewer tiles than
// the chip has CUs; `tile` 64 / 128 forces one (tests, probes). The one place the geometry is chosen: the
// sizing functions and the launch all come through here.
int tile_n(int M, int N, int tile) {
  if (tile == 64 || tile == 128) return tile;
  return (N == 64 || (int64_t)ceil_div(M, kTM) * ceil_div(N, 128) < kChipCUs) ? 64 : 128;
}

template <int TN>
hipError_t launch(const void* x, const void* w, void* y, int M, int H, int Wd, int Cin, int N, GemmBnEpi e,
                  hipStream_t s) {
  static bool attr = false;
  if (!attr) {
    PTDT_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&conv3x3_bn_kernel<TN>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, Geo<TN>::kLds));
    attr = true;
  }
  const int tm = ceil_div(M, kTM), tn = ceil_div(N, TN);  // <= 2^24 row tiles x <= 16 channel tiles
  e.group = merge_group(tm);
  hipLaunchKernelGGL(conv3x3_bn_kernel<TN>, dim3((unsigned)((int64_t)tm * tn)), dim3(kThreads), Geo<TN>::kLds, s,
                     static_cast<const uint16_t*>(x), static_cast<const uint16_t*>(w), static_cast<uint16_t*>(y), M,
                     H, Wd, Cin, N, tm, tn, e);
  return hipGetLastError();
}

}  // namespace

bool conv3x3_bn_supported(int Cin, int Cout) {
  return Cin >= 64 && Cout >= 64 && Cin <= 1024 && Cout <= 1024 && Cin % 64 == 0 && Cout % 64 == 0;
}

int64_t conv3x3_bn_ws_floats(int M, int Cin, int Cout, int tile) {
  if (M <= 0 || !conv3x3_bn_supported(Cin, Cout)) return 0;
  const int tm = ceil_div(M, kTM);
  const int wm = tile_n(M, Cout, tile) == 128 ? Geo<128>::kWM : Geo<64>::kWM;
  return (int64_t)2 * Cout * ((int64_t)wm * tm + ceil_div(tm, merge_group(tm)));
}

int64_t conv3x3_bn_num_tickets(int M, int Cin, int Cout, int tile) {
  if (M <= 0 || !conv3x3_bn_supported(Cin, Cout)) return 0;
  const int tm = ceil_div(M, kTM);
  return (int64_t)(ceil_div(tm, merge_group(tm)) + 1) * ceil_div(Cout, tile_n(M, Cout, tile));
}

hipError_t conv3x3_bn_stats(const void* x, const void* w, void* y, int N, int H, int W, int Cin, int Cout,
                            GemmBnEpi e, hipStream_t s, int tile) {
  if (N <= 0 || H <= 0 || W <= 0 || (int64_t)N * H * W >= (1LL << 31) || !conv3x3_bn_supported(Cin, Cout) ||
      (tile != 0 && tile != 64 && tile != 128) || e.ws == nullptr || e.tickets == nullptr || e.p.mean == nullptr ||
      e.p.invstd == nullptr || e.p.scale == nullptr || e.p.shift == nullptr)
    return hipErrorInvalidValue;
  if (x == nullptr || w == nullptr || y == nullptr ||
      ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(w) | reinterpret_cast<uintptr_t>(y)) & 15))
    return hipErrorInvalidValue;
  const int M = N * H * W;
  return tile_n(M, Cout, tile) == 128 ? launch<128>(x, w, y, M, H, W, Cin, Cout, e, s)
                                      : launch<64>(x, w, y, M, H, W, Cin, Cout, e, s);
}

}  // namespace ptdt
