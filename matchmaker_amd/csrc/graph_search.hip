// Beam search over a fixed-degree neighbour graph (dense retrieval, faiss_index_type: hnsw) for MI355X (gfx950 / CDNA4).
//
// Replaces, for one GPU's shard, the search of the reference's CPU HNSW index (matchmaker/retrieval/faiss_indices.py
// FaissHNSWIndexer; faiss itself is a third-party dependency absent from the reference tree).  The graph is ONE level,
// built exactly from the shard's k-NN lists (matchmaker_amd/retrieval.py GraphIPIndexer); this file is the search.
//
// Semantics per query (restated in tests/graph_reference.py):
//   start    the candidate list L = the query's entry rows (-1 and duplicates ignored), scored; they form the visited set;
//            L keeps the best ef, score descending, lower row first on equal scores
//   iterate  at most max_iters times: the `width` best entries of L not yet expanded are marked expanded (none: stop);
//            every neighbour of theirs that is not -1 and not visited is marked visited and scored; the new pairs are
//            merged into L, L is cut to ef
//   output   the first k entries of L, (-inf, -1) padded; stats = (iterations run, rows scored)
// The visited set stores full row numbers (open addressing, linear probing, one compare-and-swap per insert): it is
// exact, so the result depends only on the set semantics, not on the order in which lanes insert.
//
// One workgroup of 256 threads per query (a workgroup walks queries blockIdx.x, + gridDim.x, ...).  In LDS: L (keys of
// 64 bits: order-preserving score key, row, expanded bit — ascending key = output order), the compacted list of an
// iteration's new rows, and the visited table when the host found that it fits; otherwise the table is the workgroup's
// slice of the workspace, cleared by the workgroup itself before every query.  New rows are scored by 16-lane groups
// with 16-byte loads (E = 128: one load per lane, E = 768: six), two rows per group = eight rows per wavefront in
// flight, fp32 accumulation, cross-lane reduction; the query's chunks stay in registers for the whole call.  The merge
// is a bitonic sort of the new pairs (descending) and a bitonic merge with L.  No MFMA, plain vector stores only.
#include "mm_internal.h"
#include "elem_device.h"
#include "bitonic_device.h"

namespace mm {

constexpr int kGsThreads = 256;
constexpr int kGsMaxEf = 2048;
constexpr int kGsMaxWidth = 8;
constexpr int kGsMaxM = 128;
constexpr int kGsMaxIters = 1 << 16;
constexpr int kGsLdsSlots = 16384;      // visited table in LDS: at most 64 KiB of int32 rows
constexpr int kGsMaxGrid = 1024;        // workgroups of a call = slices of the workspace
constexpr unsigned long long kGsEmpty = ~0ull;

struct GsArgs {
  const void* q;            // [nq, E]
  const void* v;            // [n, E]
  const int32_t* nbr;       // [n, M]
  const int32_t* entry;     // [nq, n_entry]
  int64_t n;
  int nq, M, n_entry, ef, width, max_iters, k;
  int lcap;                 // slots of L (power of two >= ef and >= ccap)
  int ccap;                 // slots of the new-pair list (power of two >= max(width M, n_entry))
  int slots;                // slots of the visited table (power of two)
  int lds_table;            // 1: the table lives in LDS
  int32_t* gtable;          // [gridDim.x, slots] when lds_table == 0
  float* out_s;             // [nq, k]
  int64_t* out_r;           // [nq, k]
  int32_t* stats;           // [nq, 2] or null
};

template <int DT>
__device__ __forceinline__ float gs_dot8(short8 a, short8 b, float acc);
template <>
__device__ __forceinline__ float gs_dot8<MM_F16>(short8 a, short8 b, float acc) {
  const f16x8 x = __builtin_bit_cast(f16x8, a), y = __builtin_bit_cast(f16x8, b);
#pragma unroll
  for (int i = 0; i < 8; ++i) acc = __builtin_fmaf((float)x[i], (float)y[i], acc);
  return acc;
}
template <>
__device__ __forceinline__ float gs_dot8<MM_BF16>(short8 a, short8 b, float acc) {
#pragma unroll
  for (int i = 0; i < 8; ++i)
    acc = __builtin_fmaf(bits_to_f32<MM_BF16>((uint16_t)a[i]), bits_to_f32<MM_BF16>((uint16_t)b[i]), acc);
  return acc;
}

// true when `row` was not in the set before (and is now)
__device__ __forceinline__ bool gs_visit(int32_t* tab, int mask, int32_t row) {
  uint32_t h = (uint32_t)row * 2654435761u;
  h ^= h >> 16;
  for (;;) {
    h &= (uint32_t)mask;
    const int32_t old = atomicCAS(tab + h, -1, row);
    if (old == -1) return true;
    if (old == row) return false;
    ++h;
  }
}

// Scores nk[0 .. C) (each slot holds a row number) against the query and leaves the slot's key there.
template <int DT, int NSL>
__device__ __forceinline__ void gs_score(const GsArgs& a, const short8 (&qv)[NSL], unsigned long long* nk, int C) {
  const int gid = threadIdx.x >> 4, gl = threadIdx.x & 15;
  const char* vb = (const char*)a.v;
  for (int base = 0; base < C; base += 32) {
    const int i0 = base + gid, i1 = base + 16 + gid;
    const int64_t r0 = i0 < C ? (int64_t)nk[i0] : 0, r1 = i1 < C ? (int64_t)nk[i1] : 0;   // row 0 exists: loaded, not used
    const char* p0 = vb + r0 * (NSL * 256) + gl * 16;
    const char* p1 = vb + r1 * (NSL * 256) + gl * 16;
    short8 x0[NSL], x1[NSL];
#pragma unroll
    for (int s = 0; s < NSL; ++s) x0[s] = *(const short8*)(p0 + s * 256);
#pragma unroll
    for (int s = 0; s < NSL; ++s) x1[s] = *(const short8*)(p1 + s * 256);
    float s0 = 0.0f, s1 = 0.0f;
#pragma unroll
    for (int s = 0; s < NSL; ++s) {
      s0 = gs_dot8<DT>(x0[s], qv[s], s0);
      s1 = gs_dot8<DT>(x1[s], qv[s], s1);
    }
#pragma unroll
    for (int o = 8; o >= 1; o >>= 1) {
      s0 += __shfl_xor(s0, o, 64);
      s1 += __shfl_xor(s1, o, 64);
    }
    if (gl == 0) {
      if (i0 < C) nk[i0] = ((unsigned long long)desc_key(s0) << 32) | ((unsigned long long)r0 << 1);
      if (i1 < C) nk[i1] = ((unsigned long long)desc_key(s1) << 32) | ((unsigned long long)r1 << 1);
    }
  }
}

// nk[0 .. C) unsorted keys -> merged into the ascending list L [lcap], which is then cut to ef.
__device__ __forceinline__ void gs_merge(const GsArgs& a, unsigned long long* L, unsigned long long* nk, int C) {
  const int tid = threadIdx.x;
  const int c2 = pow2_ge(C);
  for (int i = C + tid; i < c2; i += kGsThreads) nk[i] = kGsEmpty;
  __syncthreads();
  bitonic_desc(nk, c2, tid, kGsThreads);
  // L ascending, (padding, nk) descending: the element-wise minimum is bitonic and holds the lcap smallest keys
  const int off = a.lcap - c2;
  for (int j = tid; j < c2; j += kGsThreads) {
    const unsigned long long x = L[off + j], y = nk[j];
    if (y < x) L[off + j] = y;
  }
  __syncthreads();
  bitonic_merge_asc(L, a.lcap, tid, kGsThreads);
  for (int i = a.ef + tid; i < a.lcap; i += kGsThreads) L[i] = kGsEmpty;
  __syncthreads();
}

template <int DT, int NSL>
__global__ void __launch_bounds__(kGsThreads) graph_search_kernel(const GsArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  unsigned long long* L = (unsigned long long*)smem;     // [lcap]
  unsigned long long* nk = L + a.lcap;                   // [ccap]
  int32_t* sel = (int32_t*)(nk + a.ccap);                // [8] rows expanded in this iteration
  int32_t* sh = sel + kGsMaxWidth;                       // [8]: 0 = new rows, 1 = expanded entries
  int32_t* ltab = sh + 8;                                // [slots] when lds_table
  const int tid = threadIdx.x, lane = tid & 63, gl = tid & 15;
  int32_t* tab = a.lds_table ? ltab : a.gtable + (int64_t)blockIdx.x * a.slots;
  const int mask = a.slots - 1;

  for (int q = blockIdx.x; q < a.nq; q += gridDim.x) {
    short8 qv[NSL];
#pragma unroll
    for (int s = 0; s < NSL; ++s) qv[s] = *(const short8*)((const char*)a.q + (int64_t)q * (NSL * 256) + s * 256 + gl * 16);
    if (a.lds_table) {
      for (int i = tid; i < a.slots; i += kGsThreads) ltab[i] = -1;
    } else {
      for (int i = tid; i < a.slots; i += kGsThreads) tab[i] = -1;
      __threadfence();
    }
    for (int i = tid; i < a.lcap; i += kGsThreads) L[i] = kGsEmpty;
    if (tid == 0) sh[0] = 0;
    __syncthreads();

    // ---- start: the entry rows
    for (int i = tid; i < a.n_entry; i += kGsThreads) {
      const int32_t r = a.entry[(int64_t)q * a.n_entry + i];
      if (r >= 0 && r < a.n && (a.lds_table ? gs_visit(ltab, mask, r) : gs_visit(tab, mask, r))) nk[atomicAdd(sh, 1)] = (unsigned long long)r;
    }
    __syncthreads();
    int C = sh[0];
    int scored = C, iters = 0;
    int len = C < a.ef ? C : a.ef;
    gs_score<DT, NSL>(a, qv, nk, C);
    __syncthreads();
    gs_merge(a, L, nk, C);

    // ---- iterate
    for (int it = 0; it < a.max_iters; ++it) {
      if (tid < 64) {
        int found = 0;
        for (int base = 0; base < len && found < a.width; base += 64) {
          const int i = base + lane;
          const unsigned long long key = i < len ? L[i] : kGsEmpty;
          const bool un = key != kGsEmpty && !(key & 1ull);
          const unsigned long long m = __ballot(un);
          const int mine = found + __popcll(m & ((1ull << lane) - 1ull));
          if (un && mine < a.width) {
            sel[mine] = (int32_t)((uint32_t)key >> 1);
            L[i] = key | 1ull;
          }
          found += __popcll(m);
        }
        if (lane == 0) {
          sh[1] = found < a.width ? found : a.width;
          sh[0] = 0;
        }
      }
      __syncthreads();
      const int nsel = sh[1];
      if (nsel == 0) break;
      ++iters;
      for (int idx = tid; idx < nsel * a.M; idx += kGsThreads) {
        const int e = idx / a.M, j = idx - e * a.M;
        const int32_t r = a.nbr[(int64_t)sel[e] * a.M + j];
        if (r >= 0 && r < a.n && (a.lds_table ? gs_visit(ltab, mask, r) : gs_visit(tab, mask, r))) nk[atomicAdd(sh, 1)] = (unsigned long long)r;
      }
      __syncthreads();
      C = sh[0];
      if (C == 0) {                   // uniform
        __syncthreads();              // every wavefront has read sh[0] before wavefront 0 resets it for the next iteration
        continue;
      }
      scored += C;
      len = len + C < a.ef ? len + C : a.ef;
      gs_score<DT, NSL>(a, qv, nk, C);
      __syncthreads();
      gs_merge(a, L, nk, C);
    }

    // ---- output
    for (int i = tid; i < a.k; i += kGsThreads) {
      const unsigned long long e = L[i];
      const bool ok = e != kGsEmpty;
      a.out_s[(int64_t)q * a.k + i] = ok ? desc_unkey((uint32_t)(e >> 32)) : neg_inf();
      a.out_r[(int64_t)q * a.k + i] = ok ? (int64_t)((uint32_t)e >> 1) : -1;
    }
    if (a.stats && tid == 0) {
      a.stats[2 * (int64_t)q] = iters;
      a.stats[2 * (int64_t)q + 1] = scored;
    }
    __syncthreads();
  }
}

// the largest visited table the envelope allows is 2^28 slots: its size fits an int
static_assert(2 * ((int64_t)kGsMaxEf + (int64_t)kGsMaxIters * kGsMaxWidth * kGsMaxM) <= (1LL << 28), "visited table slots");

struct GsGeom {
  int lcap, ccap, slots, lds_table, grid;
  size_t lds;
};

// the arguments are inside the envelope
static GsGeom gs_geom(int64_t n, int nq, int M, int ef, int width, int n_entry, int max_iters) {
  GsGeom g;
  const int wm = width * M;
  g.ccap = (int)pow2_ge<int64_t>(wm > n_entry ? wm : n_entry);
  const int ef2 = (int)pow2_ge<int64_t>(ef);
  g.lcap = ef2 > g.ccap ? ef2 : g.ccap;
  // rows a query can visit: the placement goes by the bound of the call's parameters alone, the size of a slice in the
  // workspace also knows that no more than n distinct rows exist
  const int64_t bound = (int64_t)n_entry + (int64_t)max_iters * wm;
  g.lds_table = 2 * bound <= kGsLdsSlots;
  const int64_t need = g.lds_table ? bound : (bound < n ? bound : n);
  g.slots = (int)pow2_ge<int64_t>(2 * (need > 32 ? need : 32));     // <= 2^28, see above
  g.grid = nq < kGsMaxGrid ? nq : kGsMaxGrid;
  g.lds = (size_t)g.lcap * 8 + (size_t)g.ccap * 8 + (kGsMaxWidth + 8) * 4 + (g.lds_table ? (size_t)g.slots * 4 : 0);
  return g;
}

static int gs_envelope(int64_t n, int nq, int E, int dtype, int M, int n_entry, int ef, int width, int max_iters, int k) {
  if (n <= 0 || nq <= 0) return set_error(MM_EINVAL, "graph_search: non-positive shape");
  if (dtype != MM_F16 && dtype != MM_BF16) return set_error(MM_EUNSUPPORTED, "graph_search: float16 / bfloat16 vectors only");
  if (E < 128 || E > 768 || E % 128) return set_error(MM_EUNSUPPORTED, "graph_search: E=%d is not one of 128, 256, ..., 768 (pad the vectors)", E);
  if (ef < 1 || ef > kGsMaxEf) return set_error(MM_EUNSUPPORTED, "graph_search: ef=%d outside 1 .. %d", ef, kGsMaxEf);
  if (k < 1 || k > ef) return set_error(MM_EUNSUPPORTED, "graph_search: k=%d outside 1 .. ef=%d", k, ef);
  if (width < 1 || width > kGsMaxWidth) return set_error(MM_EUNSUPPORTED, "graph_search: width=%d outside 1 .. %d", width, kGsMaxWidth);
  if (n_entry < 1 || n_entry > ef) return set_error(MM_EUNSUPPORTED, "graph_search: n_entry=%d outside 1 .. ef=%d", n_entry, ef);
  if (M < 2 || M > kGsMaxM || (M & 1)) return set_error(MM_EUNSUPPORTED, "graph_search: M=%d is not an even number in 2 .. %d", M, kGsMaxM);
  if (max_iters < 1 || max_iters > kGsMaxIters) return set_error(MM_EUNSUPPORTED, "graph_search: max_iters=%d outside 1 .. %d", max_iters, kGsMaxIters);
  if (n >= (1LL << 31)) return set_error(MM_EUNSUPPORTED, "graph_search: more than 2^31-1 vectors");
  return MM_OK;
}

template <int DT>
static const void* gs_kernel(int E) {
  switch (E) {
    case 128: return (const void*)graph_search_kernel<DT, 1>;
    case 256: return (const void*)graph_search_kernel<DT, 2>;
    case 384: return (const void*)graph_search_kernel<DT, 3>;
    case 512: return (const void*)graph_search_kernel<DT, 4>;
    case 640: return (const void*)graph_search_kernel<DT, 5>;
    default: return (const void*)graph_search_kernel<DT, 6>;
  }
}

}  // namespace mm

using namespace mm;

extern "C" size_t mm_graph_search_workspace_bytes(int64_t n, int nq, int M, int ef, int width, int n_entry, int max_iters) {
  if (gs_envelope(n, nq, 128, MM_F16, M, n_entry, ef, width, max_iters, 1) != MM_OK) return 0;
  const GsGeom g = gs_geom(n, nq, M, ef, width, n_entry, max_iters);
  return g.lds_table ? 256 : (size_t)g.grid * g.slots * 4;
}

extern "C" int mm_graph_search_fwd(const void* queries, const void* vectors, const int32_t* neighbors, const int32_t* entry_rows,
                                   int64_t n, int nq, int E, int dtype, int M, int n_entry, int ef, int width, int max_iters,
                                   int k, float* out_scores, int64_t* out_rows, int32_t* stats, void* workspace,
                                   size_t workspace_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!queries || !vectors || !neighbors || !entry_rows || !out_scores || !out_rows) return set_error(MM_EINVAL, "graph_search: null pointer");
  if (int e = gs_envelope(n, nq, E, dtype, M, n_entry, ef, width, max_iters, k)) return e;
  if (((uintptr_t)queries | (uintptr_t)vectors) & 15) return set_error(MM_EINVAL, "graph_search: 16-byte alignment required");
  const size_t need = mm_graph_search_workspace_bytes(n, nq, M, ef, width, n_entry, max_iters);
  if (!workspace || workspace_bytes < need) return set_error(MM_EWORKSPACE, "graph_search: workspace needs %zu bytes", need);

  const GsGeom g = gs_geom(n, nq, M, ef, width, n_entry, max_iters);
  GsArgs a{};
  a.q = queries; a.v = vectors; a.nbr = neighbors; a.entry = entry_rows;
  a.n = n; a.nq = nq; a.M = M; a.n_entry = n_entry; a.ef = ef; a.width = width; a.max_iters = max_iters; a.k = k;
  a.lcap = g.lcap; a.ccap = g.ccap; a.slots = g.slots; a.lds_table = g.lds_table;
  a.gtable = (int32_t*)workspace;
  a.out_s = out_scores; a.out_r = out_rows; a.stats = stats;

  const void* kern = nullptr;
  with_dtype16(dtype, [&](auto dt) { kern = gs_kernel<MM_V(dt)>(E); return MM_OK; });
  if (g.lds > 64 * 1024) (void)hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)g.lds);
  void* params[] = {(void*)&a};
  if (hipLaunchKernel(kern, dim3(g.grid), dim3(kGsThreads), params, g.lds, stream) != hipSuccess) {
    (void)hipGetLastError();
    return set_error(MM_ELAUNCH, "graph_search_kernel: launch failed");
  }
  return check_launch("graph_search_kernel");
}
