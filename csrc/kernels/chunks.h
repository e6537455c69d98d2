// (tensor, chunk) block mapping of the multi-tensor launches (optim.hip, gradclip.hip):
// the list's tensors are cut into kChunk-element chunks, one block per chunk, and a
// block finds its tensor by a prefix search over the chunk counts in the kernel arguments.
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

}  // namespace ptdt
