// Backward of ``BN(conv3x3(X))``, stride 1, padding 1, NHWC bf16 (ops/convbn.py, PTDT_CONV3X3_BWD): the
// 3x3 counterpart of conv1x1_bwd_tiled.hip, with its operands, rounding points and split / merge scheme.
// With M = N H W pixels:
//
//   dY[m, co]        = fma(A[co], g[m, co], fma(B[co], y[m, co], C[co]))   rounded to bf16, never stored
//   dX[n, h, w, ci]  = sum over (kh, kw, co) of dY[n, h - kh + 1, w - kw + 1, co] . W[co, kh, kw, ci]
//   dW[co, kh, kw, ci] = sum over (n, h, w) of dY[n, h, w, co] . X[n, h + kh - 1, w + kw - 1, ci]
//
// fp32 MFMA accumulate (v_mfma_f32_16x16x32_bf16), bf16 out; a pixel outside the image contributes exactly
// zero: in dX that is a zero dY chunk (not C), in dW a zero X chunk. Cin % 64 == 0, Cout % 64 == 0,
// 64 <= Cin, Cout <= 1024, 1 <= M < 2^31, any H, W >= 1. Three launches:
//
// * data gradient: the implicit GEMM dX[M, Cin] = D[M, 9 Cout] . Wt walked as 9 taps x Cout / 64 slices; it
//   is conv1x1_bwd_tiled.hip's data-gradient kernel (128 pixels x 128 input channels per workgroup, 4 waves
//   as 2 x 2, two LDS buffers per operand, one barrier per slice, W^T read with ds_read_b64_tr_b16 so dX
//   leaves in 16-B stores) with two changes. The source pixel of a thread's g / y chunks is its tile pixel
//   plus the wave-uniform offset of the FLIPPED tap ((1 - kh) W + (1 - kw) pixels), masked by bit 8 - tap of
//   the 9-bit inside-image mask that conv3x3_bn.hip decodes once per pixel; and the weight slice is rows
//   co .. co + 63 of W [Cout][9 Cin] at column tap Cin + ci0, LDS-DMA'd as it stands.
// * weight gradient: per tap a [Cout, Cin] GEMM reduced over pixels, in blocks of 64 pixels. A workgroup
//   owns a TC x TC tile of (co, ci), NT taps of it, and one of S contiguous ranges of blocks (S a function
//   of the shape alone). Per block it forms ONE dY image [64 m][TC co] (coefficients applied in registers)
//   and NT X images [64 m][TC ci], one per tap, each from the pixel shifted by that tap and written as
//   zeros where the tap leaves the image: the mask is per (pixel, tap), so it lives on the register path of
//   the operand that differs between taps, and the dY image is shared by the NT taps. Both are row-major
//   images read with the transposing LDS read; the block's (h, w) decode costs two integer divisions per
//   chunk row. Accumulators stay in registers over the range and go to ws[split][Cout][9 Cin] with plain
//   stores. Two instances:
//     TC = 128, NT = 1 (tap = grid dimension): 64 accumulators per lane; a second tap would be 128.
//     TC = 64, NT = 3 (one kernel row kh; kh = grid dimension): 48 accumulators per lane, every MFMA of a
//       64 x 64 shape does useful work, and dY is formed 3 times per pixel instead of 9. All nine taps
//       (144 accumulators) would need ten images per buffer, 160 KiB of LDS for two buffers.
//   Both use 64 KiB of LDS (two buffers of 1 + NT images), 2 workgroups per CU. TC = 64 is taken where a
//   channel count is 64; `tile` 64 / 128 forces one (tests, probes).
// * conv1x1_bwd.hip's merge kernel sums the S partials in fixed order (K = 9 Cin): no atomics, two launches
//   are bit-identical.
//
// A channel tile that sticks out of Cin or Cout reads clamped, valid columns and stores nothing for them.
// In the data gradient rows m >= M are computed from pixel M - 1 and never stored; in the weight gradient
// they are zero chunks of both operands.
#include "common.h"
#include "conv_bwd_tile.h"
#include "kernels.h"
#include "lds_tile.h"

namespace ptdt {
namespace {

constexpr int kThreads = 256;
constexpr int kTM = 128;            // pixels of a dX block
constexpr int kTC = 128;            // input channels of a dX block
constexpr int kTS = 64;             // reduction step: output channels of a slice (dX), pixels of a block (dW)
constexpr int kImg = 64 * 256;      // one dX-kernel image: [64][128] or [128][64] bf16
constexpr int kLds = 4 * kImg;      // 64 KiB, both kernels
constexpr int kTargetWgs = 512;     // weight-gradient grid: 2 workgroups per CU of a 256-CU part
constexpr int kMinBlocks = 4;       // pixel blocks per split at least (amortises the partial's stores)
constexpr int64_t kWsFloats = 8 << 20;  // workspace cap (32 MiB) unless one partial alone is larger

// bit (3 kh + kw): pixel (ph + kh - 1, pw + kw - 1) lies inside the H x Wd image
__device__ __forceinline__ unsigned tap_mask(int ph, int pw, int H, int Wd) {
  unsigned bits = 0;
#pragma unroll
  for (int kh = 0; kh < 3; ++kh)
#pragma unroll
    for (int kw = 0; kw < 3; ++kw) {
      const int sh = ph + kh - 1, sw = pw + kw - 1;
      if (sh >= 0 && sh < H && sw >= 0 && sw < Wd) bits |= 1u << (3 * kh + kw);
    }
  return bits;
}

// ---- data gradient: dX[m0 .. +127][k0 .. +127], block = (pixel tile) * ktn + (ci tile); N = Cout
__global__ void __launch_bounds__(kThreads, 2) conv3x3_bwd_dx_kernel(
    const uint16_t* __restrict__ G, const uint16_t* __restrict__ Y, const uint16_t* __restrict__ W,
    const float* __restrict__ coef, uint16_t* __restrict__ dX, int M, int H, int Wd, int Cin, int N, int ktn) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  uint8_t* const dyb = smem;             // 2 x [128 m][64 co], rows of 128 B
  uint8_t* const wb = smem + 2 * kImg;   // 2 x [64 co][128 ci], rows of 256 B
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fr = lane & 15, fq = lane >> 4, tq = fr >> 2, tp = fr & 3;
  const int wm = w >> 1, wk = w & 1;
  const int k0 = (int)(blockIdx.x % ktn) * kTC;
  const int64_t m0 = (int64_t)(blockIdx.x / ktn) * kTM;
  const int64_t K = 9 * (int64_t)Cin;

  // this thread's dY chunks: pixels m0 + (tid >> 3) + 32 i, channels 8 cc .. + 7 of every slice. roff: the
  // pixel's own element offset in g / y; ok: its inside-image mask (edge rows: pixel M - 1, never stored)
  const int cc = tid & 7, r0 = tid >> 3;
  int64_t roff[4];
  unsigned ok[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    int64_t m = m0 + r0 + 32 * i;
    m = m < M ? m : (int64_t)M - 1;
    ok[i] = tap_mask((int)((m / Wd) % H), (int)(m % Wd), H, Wd);
    roff[i] = m * N + 8 * cc;
  }
  const int spt = N / kTS;  // slices per tap
  u32x4_t gv[4], yv[4];
  bool vl[4];
  Coef8 ck;
  int ltap = 0, lsl = 0;  // tap and slice within it of the next issue
  // slice (ltap, lsl): its W image by DMA into img, its g / y chunks and coefficients into registers. Tap
  // (kh, kw) takes dY from pixel (h - kh + 1, w - kw + 1): the forward's tap 8 - tap of this pixel.
  auto issue = [&](uint8_t* img) {
    const int c0 = ltap * Cin + k0, n0 = kTS * lsl;
    stage_image<kThreads>(W, K, c0, ltap * Cin + Cin - 8, img, w, lane, [&](int r) { return n0 + r; });
    const int64_t d = ((int64_t)(1 - ltap / 3) * Wd + (1 - ltap % 3)) * N + n0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      vl[i] = (ok[i] >> (8 - ltap)) & 1u;
      gv[i] = yv[i] = u32x4_t{0u, 0u, 0u, 0u};
      if (vl[i]) {
        gv[i] = *reinterpret_cast<const u32x4_t*>(G + (roff[i] + d));
        yv[i] = *reinterpret_cast<const u32x4_t*>(Y + (roff[i] + d));
      }
    }
    ck = load_coef(coef, N, n0 + 8 * cc);
    if (++lsl == spt) lsl = 0, ++ltap;
  };

  f32x4_t acc[4][4];  // [channel tile j][row tile i]
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[j][i] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  const int nt = 9 * spt;
  issue(wb);
  for (int t = 0; t < nt; ++t) {
    const int cur = t & 1;
    uint8_t* const dyt = dyb + cur * kImg;
    const uint8_t* const wt = wb + cur * kImg;
#pragma unroll
    for (int i = 0; i < 4; ++i)
      *reinterpret_cast<u32x4_t*>(dyt + tile_off<128>(r0 + 32 * i, cc)) = dy_chunk(gv[i], yv[i], ck, vl[i]);
    vm_wait<0>();     // this wave's part of W slice t landed
    __syncthreads();  // slice t complete; every wave is past its reads of slice t - 1 (the other buffers)
    if (t + 1 < nt) issue(wb + (cur ^ 1) * kImg);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int ks = 0; ks < kTS / 32; ++ks) {
      const int rb = 32 * ks + 8 * fq + tq;
      bf16x8_t a[4], b[4];
      // W^T tile j, row i <-> channel 64 wk + pair_channel(j, i), as conv1x1_bwd_tiled.hip
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

  // lane (fr, fq) of tiles (2p, 2p + 1), row tile i: pixel 16 i + fr, channels 32 p + 8 fq .. + 7
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
      if (m < M && k < Cin) *reinterpret_cast<u32x4_t*>(dX + m * Cin + k) = pk;
    }
  }
}

// ---- weight gradient: partial of dW[co0 .. +TC-1][taps tap0 .. +NT-1][ci0 .. +TC-1] over the pixel blocks
// of split s; block = (s * tiles + (co tile) * ktn + (ci tile)) * (9 / NT) + (tap group)
template <int TC, int NT>
struct DwGeo {
  static_assert((TC == 128 && NT == 1) || (TC == 64 && NT == 3), "instances");
  static constexpr int kRB = 2 * TC;               // bytes of an image row
  static constexpr int kImgB = kTS * kRB;          // one image [64 m][TC]
  static constexpr int kBuf = (1 + NT) * kImgB;    // dY + NT X images
  static constexpr int kCPR = TC / 8;              // 16-B chunks per row
  static constexpr int kRS = kThreads / kCPR;      // rows one pass of the workgroup covers
  static constexpr int kCH = kTS / kRS;            // chunks per thread and image
  static constexpr int kFT = TC / 32;              // 16-wide MFMA tiles of a wave, each way
  static constexpr int kNG = 9 / NT;               // tap groups
  static_assert(2 * kBuf == kLds, "64 KiB");
};

template <int TC, int NT>
__global__ void __launch_bounds__(kThreads, 2) conv3x3_bwd_dw_kernel(
    const uint16_t* __restrict__ G, const uint16_t* __restrict__ Y, const uint16_t* __restrict__ X,
    const float* __restrict__ coef, float* __restrict__ ws, int M, int H, int Wd, int Cin, int N, int ktn, int tiles,
    int S) {
  using D = DwGeo<TC, NT>;
  constexpr int RB = D::kRB, CH = D::kCH, RS = D::kRS, FT = D::kFT;
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fr = lane & 15, fq = lane >> 4, tq = fr >> 2, tp = fr & 3;
  const int wn = w >> 1, wk = w & 1;
  const int tg = (int)(blockIdx.x % D::kNG);
  const int tile = (int)((blockIdx.x / D::kNG) % tiles), s = (int)(blockIdx.x / D::kNG / tiles);
  const int co0 = (tile / ktn) * TC, ci0 = (tile % ktn) * TC;
  const int tap0 = tg * NT;
  const int nblk = (int)(((int64_t)M + kTS - 1) / kTS);
  const int b0 = (int)((int64_t)s * nblk / S), b1 = (int)((int64_t)(s + 1) * nblk / S);

  // this thread's chunks: pixels (tid / kCPR) + RS i of a block; channels nc .. + 7 of dY, kc .. + 7 of X
  // (a tile past Cout or Cin: valid columns, nothing stored)
  const int cc = tid % D::kCPR, r0 = tid / D::kCPR;
  const int nc = co0 + 8 * cc < N ? co0 + 8 * cc : N - 8;
  const int kc = ci0 + 8 * cc < Cin ? ci0 + 8 * cc : Cin - 8;
  const Coef8 ck = load_coef(coef, N, nc);
  u32x4_t gv[CH], yv[CH], xv[NT][CH];
  bool vl[CH];
  auto load = [&](int b) {
#pragma unroll
    for (int i = 0; i < CH; ++i) {
      const int64_t m = (int64_t)b * kTS + r0 + RS * i;
      vl[i] = m < M;
      gv[i] = yv[i] = u32x4_t{0u, 0u, 0u, 0u};
      int ph = 0, pw = 0;
      if (vl[i]) {
        const unsigned um = (unsigned)m, q = um / (unsigned)Wd;
        pw = (int)(um - q * (unsigned)Wd);
        ph = (int)(q % (unsigned)H);
        gv[i] = *reinterpret_cast<const u32x4_t*>(G + (m * N + nc));
        yv[i] = *reinterpret_cast<const u32x4_t*>(Y + (m * N + nc));
      }
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        const int dh = (tap0 + j) / 3 - 1, dw = (tap0 + j) % 3 - 1;
        const int sh = ph + dh, sw = pw + dw;
        xv[j][i] = u32x4_t{0u, 0u, 0u, 0u};
        if (vl[i] && sh >= 0 && sh < H && sw >= 0 && sw < Wd)
          xv[j][i] = *reinterpret_cast<const u32x4_t*>(X + ((m + (int64_t)dh * Wd + dw) * Cin + kc));
      }
    }
  };

  f32x4_t acc[NT][FT][FT];  // [tap j][co tile a][ci tile t]
#pragma unroll
  for (int j = 0; j < NT; ++j)
#pragma unroll
    for (int a = 0; a < FT; ++a)
#pragma unroll
      for (int t = 0; t < FT; ++t) acc[j][a][t] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  if (b0 < b1) load(b0);
  for (int b = b0; b < b1; ++b) {
    uint8_t* const dyt = smem + ((b - b0) & 1) * D::kBuf;  // then the NT X images
#pragma unroll
    for (int i = 0; i < CH; ++i) {
      const int off = tile_off<RB>(r0 + RS * i, cc);
      *reinterpret_cast<u32x4_t*>(dyt + off) = dy_chunk(gv[i], yv[i], ck, vl[i]);
#pragma unroll
      for (int j = 0; j < NT; ++j) *reinterpret_cast<u32x4_t*>(dyt + (1 + j) * D::kImgB + off) = xv[j][i];
    }
    __syncthreads();  // block b complete; every wave is past its reads of block b - 1 (the other buffer)
    if (b + 1 < b1) load(b + 1);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int ks = 0; ks < kTS / 32; ++ks) {
      // opaque per step: the 4 FT swizzled fragment addresses are recomputed here (a few VALU next to 2 FT^2 NT
      // MFMAs), not kept in as many registers for the whole loop, which spilled the TC = 128 instance
      int rq = 8 * fq + tq;
      asm volatile("" : "+v"(rq));
      const int rb = 32 * ks + rq;
      bf16x8_t af[FT];
      // lane group tp addresses columns 16 t + 4 tp .. + 3 of the wave's TC / 2: half (tp & 1) of chunk
      // 2 t + (tp >> 1). One X fragment at a time: FT + 1 fragments live, not 2 FT
#pragma unroll
      for (int a = 0; a < FT; ++a) af[a] = read_tr<RB>(dyt, rb, TC / 16 * wn + 2 * a + (tp >> 1), tp & 1);
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        const uint8_t* const xt = dyt + (1 + j) * D::kImgB;
#pragma unroll
        for (int t = 0; t < FT; ++t) {
          const bf16x8_t bfv = read_tr<RB>(xt, rb, TC / 16 * wk + 2 * t + (tp >> 1), tp & 1);
#pragma unroll
          for (int a = 0; a < FT; ++a)
            acc[j][a][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[a], bfv, acc[j][a][t], 0, 0, 0);
        }
      }
    }
  }

  // lane (fr, fq) of tile (a, t): dW[co = 16 a + 4 fq + r][tap][ci = 16 t + fr]; an empty range stores zeros
  const int64_t K = 9 * (int64_t)Cin;
  float* const wp = ws + (int64_t)s * N * K;
#pragma unroll
  for (int j = 0; j < NT; ++j)
#pragma unroll
    for (int a = 0; a < FT; ++a)
#pragma unroll
      for (int t = 0; t < FT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int co = co0 + TC / 2 * wn + 16 * a + 4 * fq + r, ci = ci0 + TC / 2 * wk + 16 * t + fr;
          if (co < N && ci < Cin) wp[co * K + (tap0 + j) * Cin + ci] = acc[j][a][t][r];
        }
}

int ceil_div(int64_t a, int b) { return (int)((a + b - 1) / b); }

// The weight-gradient instance of a shape: the one place it is chosen (sizing and launch come through here)
int tile_c(int Cin, int Cout, int tile) {
  if (tile == 64 || tile == 128) return tile;
  return (Cin == 64 || Cout == 64) ? 64 : 128;
}

template <int TC, int NT>
hipError_t launch_dw(const void* g, const void* y, const void* x, const float* coef, float* ws, int M, int H, int Wd,
                     int Cin, int Cout, int S, hipStream_t s) {
  using D = DwGeo<TC, NT>;
  static bool attr = false;
  if (!attr) {
    PTDT_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&conv3x3_bwd_dw_kernel<TC, NT>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, kLds));
    attr = true;
  }
  const int ktn = ceil_div(Cin, TC), tiles = ceil_div(Cout, TC) * ktn;
  hipLaunchKernelGGL((conv3x3_bwd_dw_kernel<TC, NT>), dim3((unsigned)(S * tiles * D::kNG)), dim3(kThreads), kLds, s,
                     static_cast<const uint16_t*>(g), static_cast<const uint16_t*>(y),
                     static_cast<const uint16_t*>(x), coef, ws, M, H, Wd, Cin, Cout, ktn, tiles, S);
  return hipGetLastError();
}

}  // namespace

bool conv3x3_bwd_supported(int Cin, int Cout) {
  return Cin >= 64 && Cout >= 64 && Cin <= 1024 && Cout <= 1024 && Cin % 64 == 0 && Cout % 64 == 0;
}

int conv3x3_bwd_splits(int M, int Cin, int Cout, int tile) {
  if (M <= 0 || !conv3x3_bwd_supported(Cin, Cout)) return 0;
  const int TC = tile_c(Cin, Cout, tile);
  const int64_t nblk = ((int64_t)M + kTS - 1) / kTS, nk = (int64_t)Cout * 9 * Cin;
  int64_t S = kTargetWgs / (ceil_div(Cout, TC) * ceil_div(Cin, TC) * (TC == 128 ? 9 : 3));
  if (S > nblk / kMinBlocks) S = nblk / kMinBlocks;
  if (S > kWsFloats / nk) S = kWsFloats / nk;
  return S < 1 ? 1 : (int)S;
}

int64_t conv3x3_bwd_ws_floats(int M, int Cin, int Cout, int tile) {
  return (int64_t)conv3x3_bwd_splits(M, Cin, Cout, tile) * Cout * 9 * Cin;
}

hipError_t conv3x3_bwd(const void* g, const void* y, const void* x, const void* w, const float* coef, void* dx,
                       void* dw, float* ws, int N, int H, int W, int Cin, int Cout, hipStream_t s, int tile) {
  if (N <= 0 || H <= 0 || W <= 0 || (int64_t)N * H * W >= (1LL << 31) || !conv3x3_bwd_supported(Cin, Cout) ||
      (tile != 0 && tile != 64 && tile != 128))
    return hipErrorInvalidValue;
  if (g == nullptr || y == nullptr || x == nullptr || w == nullptr || coef == nullptr || dx == nullptr ||
      dw == nullptr || ws == nullptr)
    return hipErrorInvalidValue;
  if ((reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(x) |
       reinterpret_cast<uintptr_t>(w) | reinterpret_cast<uintptr_t>(dx) | reinterpret_cast<uintptr_t>(dw) |
       reinterpret_cast<uintptr_t>(ws) | reinterpret_cast<uintptr_t>(coef)) & 15)
    return hipErrorInvalidValue;
  static bool attr = false;
  if (!attr) {
    PTDT_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&conv3x3_bwd_dx_kernel),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, kLds));
    attr = true;
  }
  const int M = N * H * W;
  const int ktn = ceil_div(Cin, kTC);
  const int64_t mt = ((int64_t)M + kTM - 1) / kTM;  // <= 2^24 pixel tiles x <= 8 channel tiles
  hipLaunchKernelGGL(conv3x3_bwd_dx_kernel, dim3((unsigned)(mt * ktn)), dim3(kThreads), kLds, s,
                     static_cast<const uint16_t*>(g), static_cast<const uint16_t*>(y),
                     static_cast<const uint16_t*>(w), coef, static_cast<uint16_t*>(dx), M, H, W, Cin, Cout, ktn);
  PTDT_HIP_CHECK(hipGetLastError());
  const int S = conv3x3_bwd_splits(M, Cin, Cout, tile);
  PTDT_HIP_CHECK(tile_c(Cin, Cout, tile) == 128 ? (launch_dw<128, 1>(g, y, x, coef, ws, M, H, W, Cin, Cout, S, s))
                                                : (launch_dw<64, 3>(g, y, x, coef, ws, M, H, W, Cin, Cout, S, s)));
  return conv1x1_bwd_merge(ws, S, Cout * 9 * Cin / 4, dw, s);
}

}  // namespace ptdt
