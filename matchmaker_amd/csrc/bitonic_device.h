// What the kernels that sort and select share: the order-preserving integer keys of a float score, the padded power of two
// of a sort, and the bitonic networks: ascending over one integer key per element in LDS (colbert_candidates.hip: int32
// sorted-view positions; rank_metrics.hip and distinct_hits.hip: 64-bit pairs; ivf_device.h: 64-bit (score key, row) pairs),
// descending over one key and the merge pass (graph_search.hip).  dot_topk.hip keeps its own networks over (float score,
// int index) pairs.  Every network is called by all threads of the workgroup, under a uniform condition.
// No kernel is defined here.  The keys and pow2_ge are plain C++17 without a HIP compiler
// (tests/test_device_primitives_cpu.py compiles them on their own).
#pragma once
#include <stdint.h>

#include "launch_geometry.h"

namespace mm {

// The order-preserving key of a float's bits, larger float <=> larger unsigned key, and its inverse; DESC: the complement of
// that key (the two directions are one function each, so that the compiler folds the complement into the key's own select).
template <bool DESC>
MM_HD uint32_t order_key(uint32_t u) {
  const uint32_t k = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return DESC ? ~k : k;
}
template <bool DESC>
MM_HD uint32_t order_unkey(uint32_t k) {
  const uint32_t o = DESC ? ~k : k;
  return (o & 0x80000000u) ? (o & 0x7fffffffu) : ~o;
}

// ascending key = ascending float (-0 below +0); asc_unkey returns the bits exactly
MM_HD uint32_t asc_key(float f) { return order_key<false>(__builtin_bit_cast(uint32_t, f)); }
MM_HD float asc_unkey(uint32_t o) { return __builtin_bit_cast(float, order_unkey<false>(o)); }

// ASCENDING key = DESCENDING score, and -0 counts as +0: the order in which a top-k is written.
MM_HD uint32_t desc_key(float s) { return order_key<true>(__builtin_bit_cast(uint32_t, s + 0.0f)); }
MM_HD float desc_unkey(uint32_t k) { return __builtin_bit_cast(float, order_unkey<true>(k)); }
// ... with every NaN on the one key behind -inf's (the rankings and the list losses)
MM_HD uint32_t desc_key_nan_last(float s) { return s != s ? 0xffffffffu : desc_key(s); }

// the smallest power of two >= v that is >= from (itself a power of two); the result has to fit I
template <class I>
MM_HD I pow2_ge(I v, I from = 1) {
  I p = from;
  while (p < v) p <<= 1;
  return p;
}

#ifdef __HIPCC__
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

// Descending bitonic network over key[0, n) (n a power of two).  The barrier FOLLOWS every pass: the caller's own barrier
// has made key[] visible.
template <class K>
__device__ __forceinline__ void bitonic_desc(K* key, int n, int tid, int nt) {
  for (int size = 2; size <= n; size <<= 1)
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int i = tid; i < n; i += nt) {
        const int j = i ^ stride;
        if (j > i) {
          const K x = key[i], y = key[j];
          const bool down = (i & size) == 0;
          if ((x < y) == down) { key[i] = y; key[j] = x; }
        }
      }
      __syncthreads();
    }
}

// The merge pass: key[0, n) bitonic (visible to the workgroup) -> ascending.
template <class K>
__device__ __forceinline__ void bitonic_merge_asc(K* key, int n, int tid, int nt) {
  for (int stride = n >> 1; stride > 0; stride >>= 1) {
    for (int t = tid; t < (n >> 1); t += nt) {
      const int i = ((t & ~(stride - 1)) << 1) | (t & (stride - 1)), j = i | stride;
      const K x = key[i], y = key[j];
      if (x > y) { key[i] = y; key[j] = x; }
    }
    __syncthreads();
  }
}
#endif

}  // namespace mm
