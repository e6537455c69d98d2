// Microbenchmark: issue cost (8 independent chains) and dependent latency (1 chain) of
// the wave-level instructions the single-wave engine (csrc/kernels/linear_wave_impl.h)
// is built from, in shader-clock cycles (s_memtime) on one wave of gfx950.
// Build: hipcc --offload-arch=gfx950 -O3 tools/microbench_isa.hip -o tools/bin/microbench_isa
#include <hip/hip_runtime.h>

#include <cstdio>

#define CK(x)                                                                          \
  do {                                                                                 \
    hipError_t e = (x);                                                                \
    if (e != hipSuccess) {                                                             \
      std::printf("HIP error %s at %s:%d\n", hipGetErrorString(e), __FILE__, __LINE__); \
      return 1;                                                                        \
    }                                                                                  \
  } while (0)

enum Op { kFma, kDppRor8, kDppXor1, kSwap16, kSwap32, kPkFma, kDsRoundTrip, kSwizzle, kBpermute, kExp,
          kPkFmaSgpr, kPkMul, kDppPkFma, kCndmaskSgpr, kNumOps };
static const char* kNames[] = {"v_fma_f32", "v_add_f32_dpp row_ror:8", "v_add_f32_dpp quad_perm xor1",
                               "v_permlane16_swap+add", "v_permlane32_swap+add", "v_pk_fma_f32",
                               "ds_write+ds_read", "ds_swizzle(swap16)+add", "ds_bpermute+add", "v_exp_f32",
                               "v_pk_fma_f32 s[n:n+1] operand", "v_pk_mul_f32", "2 v_add_f32_dpp -> v_pk_fma_f32",
                               "v_cndmask_b32 sgpr mask"};
// The packed rows (v_pk_*) count VALUES like every other row: one packed instruction is two values, so
// its cost per instruction is twice the printed figure. "2 v_add_f32_dpp -> v_pk_fma_f32" is the wave
// engine's packed SGD on the outputs of its DPP column sums: per value one DPP add and half a packed FMA
// with an SGPR-pair multiplier (the {-lr, -lr} constants).

template <int OP>
__device__ __forceinline__ float apply(float v, float* lds, int lane) {
  if constexpr (OP == kFma) {
    return fmaf(v, 1.0001f, 0.5f);
  } else if constexpr (OP == kDppRor8) {
    return v + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x128, 0xF, 0xF, false));
  } else if constexpr (OP == kDppXor1) {
    return v + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xF, 0xF, false));
  } else if constexpr (OP == kSwap16) {
    auto p = __builtin_amdgcn_permlane16_swap(__float_as_int(v), __float_as_int(v), false, false);
    return __int_as_float(p[0]) + __int_as_float(p[1]);
  } else if constexpr (OP == kSwap32) {
    auto p = __builtin_amdgcn_permlane32_swap(__float_as_int(v), __float_as_int(v), false, false);
    return __int_as_float(p[0]) + __int_as_float(p[1]);
  } else if constexpr (OP == kDsRoundTrip) {
    lds[lane] = v;
    __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0)
    return lds[lane ^ 1] + 1.f;
  } else if constexpr (OP == kSwizzle) {
    // swizzle pattern: xor 16 over 32 lanes (bitmask mode: and 0x1f, xor 0x10)
    const int s = __builtin_amdgcn_ds_swizzle(__float_as_int(v), (0x10 << 10) | 0x1f);
    return v + __int_as_float(s);
  } else if constexpr (OP == kBpermute) {
    return v + __int_as_float(__builtin_amdgcn_ds_bpermute(((lane ^ 16) << 2), __float_as_int(v)));
  } else if constexpr (OP == kCndmaskSgpr) {
    // lane-constant condition: the compare is hoisted, the loop keeps one v_cndmask_b32 with its mask in SGPRs
    return (lane & 16) ? v : (float)lane;
  } else {
    return __expf(v) * 0.5f;
  }
}

template <int OP, int CH>
__global__ void __launch_bounds__(64) k_op(float* out, long long* cyc, int iters, float s0, float s1) {
  __shared__ float lds[64 * 8];
  const int lane = threadIdx.x;
  float v[CH];
#pragma unroll
  for (int c = 0; c < CH; ++c) v[c] = lane * 1e-3f + c;
  typedef float f2g __attribute__((ext_vector_type(2)));
  f2g gp = {1.f + lane * 1e-6f, 1.f - lane * 1e-6f};  // a VGPR pair that stays put
  asm volatile("" : "+v"(gp));
  const long long t0 = __builtin_amdgcn_s_memtime();
  for (int it = 0; it < iters; ++it) {
#pragma unroll
    for (int u = 0; u < 16; ++u) {  // 16 x CH ops per loop trip: loop overhead amortised
    if constexpr (OP == kPkFma || OP == kPkFmaSgpr || OP == kPkMul || OP == kDppPkFma) {
#pragma unroll
      for (int c = 0; c + 1 < CH || c == 0; c += 2) {
        typedef float f2 __attribute__((ext_vector_type(2)));
        f2 a = {v[c], CH > 1 ? v[c + 1] : v[c]};
        const f2 m = {1.0001f, 1.0001f}, b = {0.5f, 0.5f};
        const f2 sp = {s0, s1};  // kernel arguments: an SGPR pair
        if constexpr (OP == kPkFma) {
          a = __builtin_elementwise_fma(a, m, b);
        } else if constexpr (OP == kPkFmaSgpr) {
          a = __builtin_elementwise_fma(sp, gp, a);
        } else if constexpr (OP == kPkMul) {
          a = a * gp;
        } else {
          const f2 t = {a.x + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(a.x), 0x121, 0xF, 0xF, false)),
                        a.y + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(a.y), 0x121, 0xF, 0xF, false))};
          a = __builtin_elementwise_fma(sp, t, a);
        }
        v[c] = a.x;
        if (CH > 1) v[c + 1] = a.y;
      }
    } else {
#pragma unroll
      for (int c = 0; c < CH; ++c) v[c] = apply<OP>(v[c], lds + 64 * c, lane);
    }
#pragma unroll
    for (int c = 0; c < CH; ++c) asm volatile("" : "+v"(v[c]));
    }
  }
  float s = 0.f;
#pragma unroll
  for (int c = 0; c < CH; ++c) s += v[c];
  const long long t1 = __builtin_amdgcn_s_memtime();
  out[lane] = s;
  if (lane == 0) cyc[0] = t1 - t0;
}

// One step's gather of the wave engine (R = 2, KP = 5), three batches in flight as in its step loop:
// MODE 0 today's five loads per batch (x4, x1, x4, x1 of two 80-byte rows and the target's x1), MODE 1
// the row image's four 16-byte loads (two 32-byte records). Every loaded value is consumed one wait per
// batch; offsets change from batch to batch inside a 64 KiB table (L1 / L2 hits). Cycles per batch.
template <int MODE>
__global__ void __launch_bounds__(64) k_gather(const float* tab, float* out, long long* cyc, int iters) {
  typedef float f4 __attribute__((ext_vector_type(4)));
  const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(tab), (short)0, 65536, 0x00020000);
  const uint32_t lane = threadIdx.x;
  f4 a[3][4];  // MODE 0 uses a[u][0..1] and b[u][0..2], MODE 1 a[u][0..3]
  float b[3][3];
  auto issue = [&](int u, uint32_t o) {
    if constexpr (MODE == 0) {
      a[u][0] = __builtin_bit_cast(f4, __builtin_amdgcn_raw_buffer_load_b128(r, o, 0, 0));
      b[u][0] = __int_as_float(__builtin_amdgcn_raw_buffer_load_b32(r, o + 16, 0, 0));
      a[u][1] = __builtin_bit_cast(f4, __builtin_amdgcn_raw_buffer_load_b128(r, o + 2560, 0, 0));
      b[u][1] = __int_as_float(__builtin_amdgcn_raw_buffer_load_b32(r, o + 2576, 0, 0));
      b[u][2] = __int_as_float(__builtin_amdgcn_raw_buffer_load_b32(r, (o >> 3) + 40960, 0, 0));
    } else {
      a[u][0] = __builtin_bit_cast(f4, __builtin_amdgcn_raw_buffer_load_b128(r, o, 0, 0));
      a[u][2] = __builtin_bit_cast(f4, __builtin_amdgcn_raw_buffer_load_b128(r, o + 16, 0, 0));
      a[u][1] = __builtin_bit_cast(f4, __builtin_amdgcn_raw_buffer_load_b128(r, o + 2560, 0, 0));
      a[u][3] = __builtin_bit_cast(f4, __builtin_amdgcn_raw_buffer_load_b128(r, o + 2576, 0, 0));
    }
  };
  float acc = 0.f;
  uint32_t o = lane * 32u;
  const long long t0 = __builtin_amdgcn_s_memtime();
#pragma unroll
  for (int u = 0; u < 3; ++u) issue(u, o + 4096u * u);
  for (int it = 0; it < iters; ++it) {
#pragma unroll
    for (int u = 0; u < 3; ++u) {
      if constexpr (MODE == 1) {  // the record's fifth feature, 1.0f and target (3 of the second vector's 4 floats)
        b[u][0] = a[u][2].x + a[u][2].y;
        b[u][1] = a[u][3].x + a[u][3].y;
        b[u][2] = a[u][2].z + a[u][3].z;
      }
      acc += (a[u][0].x + a[u][0].y) + (a[u][0].z + a[u][0].w) + (a[u][1].x + a[u][1].y) + (a[u][1].z + a[u][1].w) +
             b[u][0] + b[u][1] + b[u][2];
      asm volatile("" : "+v"(acc));
      o = (o + 12288u) & 0x7fffu;
      issue(u, o + (lane & 3u) * 16u);
    }
  }
  const long long t1 = __builtin_amdgcn_s_memtime();
  out[lane] = acc + a[0][0].x + a[1][0].x + a[2][0].x;
  if (lane == 0) cyc[0] = t1 - t0;
}

// L2-hit latency: dependent loads through a 64-entry table
__global__ void __launch_bounds__(64) k_chase(const int* tab, int* out, long long* cyc, int iters) {
  int i = threadIdx.x;
  const long long t0 = __builtin_amdgcn_s_memtime();
  for (int t = 0; t < iters; ++t) i = tab[i];
  const long long t1 = __builtin_amdgcn_s_memtime();
  out[threadIdx.x] = i;
  if (threadIdx.x == 0) cyc[0] = t1 - t0;
}

// dependent system-scope (L2-bypassing) loads, as the all-reduce polls issue them
__global__ void __launch_bounds__(64) k_chase_sys(int* tab, int* out, long long* cyc, int iters) {
  int i = threadIdx.x;
  const long long t0 = __builtin_amdgcn_s_memtime();
  for (int t = 0; t < iters; ++t) i = __hip_atomic_load(tab + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  const long long t1 = __builtin_amdgcn_s_memtime();
  out[threadIdx.x] = i;
  if (threadIdx.x == 0) cyc[0] = t1 - t0;
}

// store a new value, spin until a system-scope load returns it
__global__ void __launch_bounds__(64) k_store_visible(int* buf, long long* cyc, int iters) {
  const long long t0 = __builtin_amdgcn_s_memtime();
  for (int t = 1; t <= iters; ++t) {
    __hip_atomic_store(buf + threadIdx.x, t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    int spins = 0;
    while (__hip_atomic_load(buf + threadIdx.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != t && ++spins < 100000) {
    }
  }
  const long long t1 = __builtin_amdgcn_s_memtime();
  if (threadIdx.x == 0) cyc[0] = t1 - t0;
}

template <int OP>
int run_op(float* out, long long* dcyc) {
  const int iters = 1024;
  long long c1 = 0, c8 = 0;
  for (int rep = 0; rep < 2; ++rep) {  // second run: warm I-cache
    hipLaunchKernelGGL((k_op<OP, 1>), dim3(1), dim3(64), 0, 0, out, dcyc, iters, -1e-3f, -2e-3f);
    CK(hipMemcpy(&c1, dcyc, 8, hipMemcpyDeviceToHost));
    hipLaunchKernelGGL((k_op<OP, 8>), dim3(1), dim3(64), 0, 0, out, dcyc, iters, -1e-3f, -2e-3f);
    CK(hipMemcpy(&c8, dcyc, 8, hipMemcpyDeviceToHost));
  }
  std::printf("%-32s latency %6.2f  issue %6.2f cycles\n", kNames[OP], (double)c1 / (16.0 * iters),
              (double)c8 / (8.0 * 16.0 * iters));
  return 0;
}

int main() {
  float* out;
  long long* dcyc;
  int *tab, *iout;
  CK(hipMalloc(&out, 64 * sizeof(float)));
  CK(hipMalloc(&dcyc, sizeof(long long)));
  CK(hipMalloc(&tab, 64 * sizeof(int)));
  CK(hipMalloc(&iout, 64 * sizeof(int)));
  int h[64];
  for (int i = 0; i < 64; ++i) h[i] = (i * 17 + 5) & 63;
  CK(hipMemcpy(tab, h, sizeof(h), hipMemcpyHostToDevice));
  if (run_op<kFma>(out, dcyc) || run_op<kDppRor8>(out, dcyc) || run_op<kDppXor1>(out, dcyc) ||
      run_op<kSwap16>(out, dcyc) || run_op<kSwap32>(out, dcyc) || run_op<kPkFma>(out, dcyc) ||
      run_op<kDsRoundTrip>(out, dcyc) || run_op<kSwizzle>(out, dcyc) || run_op<kBpermute>(out, dcyc) ||
      run_op<kExp>(out, dcyc) || run_op<kPkFmaSgpr>(out, dcyc) || run_op<kPkMul>(out, dcyc) ||
      run_op<kDppPkFma>(out, dcyc) || run_op<kCndmaskSgpr>(out, dcyc))
    return 1;
  long long c = 0;
  for (int rep = 0; rep < 2; ++rep) {
    hipLaunchKernelGGL(k_chase, dim3(1), dim3(64), 0, 0, tab, iout, dcyc, 2048);
    CK(hipMemcpy(&c, dcyc, 8, hipMemcpyDeviceToHost));
  }
  std::printf("%-32s latency %6.2f cycles\n", "global_load (L1 hit, 256 B table)", (double)c / 2048);
  // 1 MiB table, 4 KiB stride walk: misses L1 (32 KiB), hits L2 (4 MiB per XCD) after the first lap
  const int n = 1 << 18;
  int* big;
  CK(hipMalloc(&big, n * sizeof(int)));
  int* hb = new int[n];
  for (int i = 0; i < n; ++i) hb[i] = (i + 1024 + 64 * ((i >> 10) & 7)) % n;
  CK(hipMemcpy(big, hb, n * sizeof(int), hipMemcpyHostToDevice));
  delete[] hb;
  for (int rep = 0; rep < 3; ++rep) {
    hipLaunchKernelGGL(k_chase, dim3(1), dim3(64), 0, 0, big, iout, dcyc, 4096);
    CK(hipMemcpy(&c, dcyc, 8, hipMemcpyDeviceToHost));
  }
  std::printf("%-32s latency %6.2f cycles\n", "global_load (L2 hit, 1 MiB walk)", (double)c / 4096);
  for (int rep = 0; rep < 2; ++rep) {  // one step's gather: five loads (x4 x1 x4 x1 x1) against four x4
    hipLaunchKernelGGL(k_gather<0>, dim3(1), dim3(64), 0, 0, (const float*)big, out, dcyc, 1024);
    CK(hipMemcpy(&c, dcyc, 8, hipMemcpyDeviceToHost));
  }
  std::printf("%-32s per batch %6.2f cycles\n", "gather x4 x1 x4 x1 x1 (3 in flight)", (double)c / (3.0 * 1024));
  for (int rep = 0; rep < 2; ++rep) {
    hipLaunchKernelGGL(k_gather<1>, dim3(1), dim3(64), 0, 0, (const float*)big, out, dcyc, 1024);
    CK(hipMemcpy(&c, dcyc, 8, hipMemcpyDeviceToHost));
  }
  std::printf("%-32s per batch %6.2f cycles\n", "gather x4 x4 x4 x4 (3 in flight)", (double)c / (3.0 * 1024));
  // polling memory of the one-shot all-reduce: uncached and fine-grained allocations
  // (64-entry table, so a cacheable allocation would hit L1)
  for (int kind = 0; kind < 2; ++kind) {
    int* t2;
    CK(hipExtMallocWithFlags((void**)&t2, 64 * sizeof(int),
                             kind == 0 ? hipDeviceMallocUncached : hipDeviceMallocFinegrained));
    CK(hipMemcpy(t2, h, sizeof(h), hipMemcpyHostToDevice));
    for (int rep = 0; rep < 2; ++rep) {
      hipLaunchKernelGGL(k_chase_sys, dim3(1), dim3(64), 0, 0, t2, iout, dcyc, 1024);
      CK(hipMemcpy(&c, dcyc, 8, hipMemcpyDeviceToHost));
    }
    std::printf("%-32s latency %6.2f cycles\n", kind == 0 ? "system-scope load, uncached mem" : "system-scope load, fine-grained",
                (double)c / 1024);
    CK(hipFree(t2));
  }
  {  // store -> visible to a system-scope load of the same wave (write round trip on uncached memory)
    int* t3;
    CK(hipExtMallocWithFlags((void**)&t3, 64 * sizeof(int), hipDeviceMallocUncached));
    CK(hipMemset(t3, 0, 64 * sizeof(int)));
    for (int rep = 0; rep < 2; ++rep) {
      hipLaunchKernelGGL(k_store_visible, dim3(1), dim3(64), 0, 0, t3, dcyc, 1024);
      CK(hipMemcpy(&c, dcyc, 8, hipMemcpyDeviceToHost));
    }
    std::printf("%-32s latency %6.2f cycles\n", "store->load seen, uncached mem", (double)c / 1024);
    CK(hipFree(t3));
  }
  CK(hipDeviceSynchronize());
  return 0;
}
