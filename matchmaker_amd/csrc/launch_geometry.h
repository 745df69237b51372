// Host arithmetic of the launches: which pairs a wavefront scores, and the workspace cursor of the entry points, which both
// measures and carves the layout of the retrieval operators' workspaces.
// Nothing from HIP is included: any C++17 compiler takes this header on its own (tests/test_launch_geometry_cpu.py does).
#pragma once
#include <stddef.h>
#include <stdint.h>

// Small functions that the kernels use and a plain C++17 compiler can also take (the sort keys of bitonic_device.h, the bf16
// rounding of elem_device.h): inlined into host and device code under a HIP compiler, ordinary inline functions without one.
#ifdef __HIPCC__
#define MM_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define MM_HD inline
#endif

namespace mm {

constexpr int kCUs = 256;  // MI355X

// n pairs over at most max_waves wavefronts: wavefront i scores pairs [i * pairs_per_wave, (i + 1) * pairs_per_wave),
// grid = the wavefronts that have one.  n <= 0: an empty grid.
struct WaveSplit {
  int64_t pairs_per_wave, grid;
};
inline WaveSplit wave_split(int64_t n, int64_t max_waves) {
  if (n <= 0) return {1, 0};
  int64_t waves = max_waves < 1 ? 1 : max_waves;
  if (waves > n) waves = n;
  const int64_t per = (n + waves - 1) / waves;
  return {per, (n + per - 1) / per};
}

// All-pairs MaxSim, XCD-aware: the Bq queries in groups of q_per_group, the Bd documents in 8 * t slices; workgroup
// (xcd, slice, lane) of the 8 * t * gw streams document slice xcd * t + slice for the query groups lane, lane + gw, ...
// `target` = workgroups per XCD.  items32: a workgroup numbers its (query group, document) items with 32 bits (the tiled
// kernel); otherwise only the documents are (the shared-ring kernel).  grid == 0: that index range is too large.
struct AllPairsMap {
  int gw, t;
  int64_t grid;
};
inline AllPairsMap all_pairs_map(int64_t Bq, int64_t Bd, int q_per_group, int64_t target, bool items32) {
  const int64_t G = (Bq + q_per_group - 1) / q_per_group;
  const int64_t gw = G < target ? G : target;               // query-group lanes per (XCD, slice)
  int64_t T = target / gw;                                  // document slices per XCD
  const int64_t max_t = (Bd + 7) / 8;                       // >= 1 document per slice
  if (T > max_t) T = max_t;
  if (T < 1) T = 1;
  const int64_t items = items32 ? ((G + gw - 1) / gw) * ((Bd + 8 * T - 1) / (8 * T) + 1) : Bd;
  return {(int)gw, (int)T, items >= (1LL << 31) ? 0 : 8 * T * gw};
}

// the tiled kernel (maxsim_allpairs_tiled_kernel): nqt queries per wavefront, one wavefront per SIMD
inline AllPairsMap all_pairs_tiled(int64_t Bq, int64_t Bd, int nqt) {
  return all_pairs_map(Bq, Bd, nqt, (int64_t)kCUs * 4 / 8, true);
}
// the shared-ring kernel (maxsim_allpairs_wg_kernel): 4 x nqt queries per workgroup, two workgroups per CU
inline AllPairsMap all_pairs_ring(int64_t Bq, int64_t Bd, int nqt) {
  return all_pairs_map(Bq, Bd, 4 * nqt, (int64_t)kCUs * 2 / 8, false);
}

// the row widths the LDS-DMA streaming kernels (MaxSim: 16-bit, pair, fp8) are instantiated for, NSL = E / 128
inline bool stream_width(int E) { return E == 128 || E == 256 || E == 384 || E == 512 || E == 768; }
// ... and those of kernel pooling's K-sliced stream (TK, TKL), NS = E / 100
inline bool kp_stream_width(int E) { return E == 100 || E == 200 || E == 300; }

// Workspace blocks start on 256-byte boundaries.
inline size_t a256(size_t b) { return (b + 255) & ~(size_t)255; }

// What is left of a call's workspace; a null workspace has no bytes.  take<T>(count) reserves the next block of the layout,
// a256(count * sizeof(T)) bytes, and counts it in `used`.  A cursor without a base measures: every take returns null and
// `used` ends as the size of the layout, so an operator states its layout ONCE, in a function that its size query runs on a
// measuring cursor and its entry point (after comparing `used` of that run with the bytes it was given) on the workspace.
struct WsCursor {
  char* p;
  size_t left;
  size_t used = 0;
  WsCursor() : p(nullptr), left(0) {}
  WsCursor(void* workspace, size_t bytes) : p((char*)workspace), left(workspace ? bytes : 0) {}
  template <class T>
  T* take(size_t count) {
    const size_t b = a256(count * sizeof(T));
    used += b;
    if (!p) return nullptr;      // no pointer is formed from a null base
    T* block = (T*)p;
    p += b;
    left = left > b ? left - b : 0;
    return block;
  }
};

}  // namespace mm
