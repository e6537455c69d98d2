// Fixed-order merge of centred BatchNorm partials (n rows, S = sum, Q = sum of squares about the partial's own
// mean) by the last workgroup of a ticket (handoff.h): the merge of the GEMMs that compute a BN's statistics in
// their epilogue (gemm_big.hip gemm_bn_stats_kernel, conv1x1_pre.hip).
#pragma once

#include "handoff.h"

namespace ptdt {

// (n, S, Q) <- (n, S, Q) merged with (np, Sp, Qp): S = sum, Q = sum of squares about the mean
__device__ __forceinline__ void chan_merge(double& n, double& S, double& Q, double np, double Sp, double Qp) {
  if (np <= 0.0) return;
  if (n <= 0.0) {
    n = np, S = Sp, Q = Qp;
    return;
  }
  const double d = Sp / np - S / n;
  Q += Qp + d * d * n * np / (n + np);
  S += Sp;
  n += np;
}

// Merge partials [p0, p1) (row counts from rows_of(p)) of the BN columns n0 .. n0 + BN - 1 of a workgroup of NT
// threads; the NT/BN thread groups take interleaved partials and are merged in group order through LDS
// (sh: 3 NT doubles). Result (n, S, Q) valid in threads t < BN.
template <int NT, int BN, class RowsOf>
__device__ __forceinline__ void merge_range(const float* wsS, const float* wsQ, int N, int n0, int p0, int p1,
                                            RowsOf rows_of, double* sh, double& n, double& S, double& Q) {
  constexpr int PARTS = NT / BN;
  const int tid = threadIdx.x, col = tid % BN, part = tid / BN;
  const int c = n0 + col;
  n = S = Q = 0.0;
  if (c < N) {
    for (int p = p0 + part; p < p1; p += PARTS)
      chan_merge(n, S, Q, (double)rows_of(p), (double)ld_sc1(wsS + (int64_t)p * N + c),
                 (double)ld_sc1(wsQ + (int64_t)p * N + c));
  }
  __syncthreads();  // LDS scratch free
  if (part > 0) {
    sh[(part * 3 + 0) * BN + col] = n;
    sh[(part * 3 + 1) * BN + col] = S;
    sh[(part * 3 + 2) * BN + col] = Q;
  }
  __syncthreads();
  if (part == 0) {
#pragma unroll
    for (int q = 1; q < PARTS; ++q)
      chan_merge(n, S, Q, sh[(q * 3 + 0) * BN + col], sh[(q * 3 + 1) * BN + col], sh[(q * 3 + 2) * BN + col]);
  }
}

}  // namespace ptdt
