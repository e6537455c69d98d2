// (tensor, chunk) block mapping of the multi-tensor launches (optim.hip, layerwise.hip,
// gradclip.hip, averaging.hip): the list's tensors are cut into kChunk-element chunks, one
// block per chunk, and a block finds its tensor by a prefix search over the chunk counts in
// the kernel arguments. launch_chunks is the host side: one block per chunk of the list.
#pragma once

#include <stdint.h>

#include <hip/hip_runtime.h>

namespace ptdt {

constexpr int kChunk = 4096;  // elements per block in multi-tensor launches

__device__ __forceinline__ void locate_chunk(const int64_t* numel, int n, int blk, int& t,
                                             int64_t& start) {
  int acc = 0;
  for (t = 0; t < n; ++t) {
    const int c = (int)((numel[t] + kChunk - 1) / kChunk);
    if (blk < acc + c) break;
    acc += c;
  }
  start = (int64_t)(blk - acc) * kChunk;
}

template <typename L>
int chunk_blocks(const L& l) {
  int b = 0;
  for (int i = 0; i < l.n; ++i) b += (int)((l.numel[i] + kChunk - 1) / kChunk);
  return b;
}

// kernel<<<chunk_blocks(l), block, 0, s>>>(l, args...); an empty list launches nothing
template <typename K, typename L, typename... A>
hipError_t launch_chunks(K kernel, int block, const L& l, hipStream_t s, A... args) {
  const int nb = chunk_blocks(l);
  if (nb == 0) return hipSuccess;
  hipLaunchKernelGGL(kernel, dim3(nb), dim3(block), 0, s, l, args...);
  return hipGetLastError();
}

}  // namespace ptdt
