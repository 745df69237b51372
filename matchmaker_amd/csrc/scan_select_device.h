// What the retrieval kernels that count, compact and select share: the workgroup and wavefront prefix sums, the IVF radix
// selection and the clamped range of a list (ivf_device.h, kmeans.hip, store_writer.hip, colbert_candidates.hip,
// distinct_hits.hip).  Device-only; no kernel is defined here.
//
// Protocol.
//   * Barriers.  block_incl_scan_lds, block_excl_scan, block_offset_from_waves and ivf_radix_kth contain __syncthreads():
//     every thread of the workgroup calls them, under a condition that is uniform over the workgroup, with uniform `n` and
//     `want`.  wave_incl_scan has no barrier, but its 64 lanes call it together.  Each of the barrier functions ends with a
//     barrier or leaves its LDS words read-only until the caller's next one, so two calls may follow each other on the same
//     scratch.
//   * LDS.  block_incl_scan_lds / block_excl_scan: T sh[1024], a workgroup of exactly 1,024 threads.  block_offset_from_waves:
//     one T per wavefront.  ivf_radix_kth: int hist[256] and sh[4] (it owns sh[0..2]: the bin, the count below it, the bin's
//     count; the caller keeps its own counters elsewhere).  dot_topk.hip's selection has its own hand-off block misc[8]:
//     [0] / [1] the key bounds, [3] / [4] the bin and the count above it, [2] and [5] its kernels' counters.
#pragma once
#include <stdint.h>

namespace mm {

// List l of a partition given by its bounds lb[nlist + 1] over n rows, clamped so that a malformed bound never leaves [0, n].
__device__ __forceinline__ void list_range(const int64_t* lb, int64_t n, int l, int64_t* b, int64_t* len) {
  int64_t lo = lb[l], hi = lb[l + 1];
  lo = lo < 0 ? 0 : (lo > n ? n : lo);
  hi = hi < lo ? lo : (hi > n ? n : hi);
  *b = lo;
  *len = hi - lo;
}

// ---- prefix sums ----------------------------------------------------------------------------------------------------------

// Inclusive scan over the lanes of a wavefront (int, uint32_t, int64_t).
template <typename T>
__device__ __forceinline__ T wave_incl_scan(T v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const T t = __shfl_up(v, o, 64);
    if (lane >= o) v += t;
  }
  return v;
}

// (inclusive value of wave_incl_scan, the thread's own value) -> the thread's exclusive offset in the workgroup; *total = the
// workgroup's sum.  wtot[nwaves]: LDS, not read by the caller before its next barrier.
template <typename T>
__device__ __forceinline__ T block_offset_from_waves(T incl, T own, T* wtot, int lane, int wave, int nwaves, T* total) {
  if (lane == 63) wtot[wave] = incl;
  __syncthreads();
  T off = incl - own, tot = 0;
  for (int w = 0; w < nwaves; ++w) {
    const T t = wtot[w];
    if (w < wave) off += t;
    tot += t;
  }
  *total = tot;
  return off;
}

// Hillis-Steele step of ONE workgroup of 1024 threads: sh[tid] holds the thread's value (written by the thread itself) and
// becomes the inclusive sum over the threads up to tid, visible to the whole workgroup.
template <typename T>
__device__ __forceinline__ void block_incl_scan_lds(T* sh /* [1024] */, int tid) {
  __syncthreads();
  for (int o = 1; o < 1024; o <<= 1) {
    const T t = tid >= o ? sh[tid - o] : (T)0;
    __syncthreads();
    sh[tid] += t;
    __syncthreads();
  }
}

// exclusive scan of f(i), i < n, by ONE workgroup of 1024 threads; out[n] = the total
template <typename T, typename F, typename O>
__device__ void block_excl_scan(F f, O out, int n, T* sh /* [1024] */) {
  const int tid = threadIdx.x;
  T carry = 0;
  for (int i0 = 0; i0 < n; i0 += 1024) {
    const int i = i0 + tid;
    const T v = i < n ? f(i) : (T)0;
    sh[tid] = v;
    block_incl_scan_lds(sh, tid);
    if (i < n) out(i, carry + sh[tid] - v);
    const T tot = sh[1023];
    __syncthreads();
    carry += tot;
  }
  if (tid == 0) out(n, carry);
}

// ---- radix selection ------------------------------------------------------------------------------------------------------
// Two forms exist: this one (the k-th SMALLEST key under a predicate, with the counts below and at it: ivf_select_kernel) and
// dot_topk.hip's radix_mth_largest (the m-th largest, bytes shared by all keys skipped, the bin found by wavefront 0); putting
// both on one function made the flat top-k intermittently wrong for a reason that was not found.

// The `want`-th smallest key (want >= 1) among the elements i < n with ok(i), by ONE workgroup: 4 passes of 8 bits.
// Returns the key; *below = elements with a smaller key, *ties = elements with that key.
template <typename OK, typename KEY>
__device__ uint32_t ivf_radix_kth(int n, int want, OK ok, KEY key, int* hist /* [256] */, int* sh /* [4] */, int* below, int* ties) {
  const int tid = threadIdx.x, nt = blockDim.x;
  uint32_t prefix = 0, mask = 0;
  int remaining = want, less = 0, eq = 0;
  for (int shift = 24; shift >= 0; shift -= 8) {
    for (int i = tid; i < 256; i += nt) hist[i] = 0;
    __syncthreads();
    for (int i = tid; i < n; i += nt) {
      if (!ok(i)) continue;
      const uint32_t kx = key(i);
      if ((kx & mask) == prefix) atomicAdd(hist + ((kx >> shift) & 255u), 1);
    }
    __syncthreads();
    if (tid == 0) {
      int cum = 0, b = 0;
      for (; b < 255; ++b) {
        if (cum + hist[b] >= remaining) break;
        cum += hist[b];
      }
      sh[0] = b; sh[1] = cum; sh[2] = hist[b];
    }
    __syncthreads();
    const int b = sh[0];
    remaining -= sh[1];
    less += sh[1];
    eq = sh[2];
    prefix |= (uint32_t)b << shift;
    mask |= 255u << shift;
    __syncthreads();
  }
  *below = less;
  *ties = eq;
  return prefix;
}

}  // namespace mm
