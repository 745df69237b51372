// The ascending bitonic network over one integer key per element, shared by the kernels that sort in LDS with it
// (colbert_candidates.hip: int32 sorted-view positions; rank_metrics.hip: 64-bit (score key, arrival index) pairs).
#pragma once
#include <stdint.h>

namespace mm {

// Ascending bitonic network over key[0, n) (n a power of two), all threads of the workgroup.
template <class K>
__device__ __forceinline__ void bitonic_asc(K* key, int n, int tid, int nt) {
  for (int size = 2; size <= n; size <<= 1) {
    for (int strd = size >> 1; strd > 0; strd >>= 1) {
      __syncthreads();
      for (int idx = tid; idx < (n >> 1); idx += nt) {
        const int lo = 2 * idx - (idx & (strd - 1));
        const int hi = lo + strd;
        const bool asc = (lo & size) == 0;
        const K a = key[lo], b = key[hi];
        if ((a > b) == asc) { key[lo] = b; key[hi] = a; }
      }
    }
  }
  __syncthreads();
}

}  // namespace mm
