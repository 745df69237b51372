// ColBERT retrieval, candidate generation: the token rows a token search returned -> per query the set of documents that
// own at least one of them, ascending by document index, with their row ranges (the input of mm_maxsim_ragged_fwd).
//
// Replaces the step between the token search and the aggregate of the reference's ColBERT retrieval branch
// (matchmaker/dense_retrieval.py:391-412: `current_ids` is meant to be the set of documents of the hits, scored one by one
// through colbert.py:100-112).
//
// One workgroup per query (grid-stride over the queries).  The owner of a hit is found by a binary search over the begin
// rows of the documents, sorted by (begin, end) on the host.  Everything a workgroup sorts is ONE int32 per hit in LDS
// (64 KB at the H = 16,384 limit, so two workgroups share a CU and the wavefronts of one cover the search latency of the
// other):
//   1. keys = position j of the owning document in the sorted view (sentinel for a dropped hit); ascending bitonic sort;
//      first occurrences flagged, prefix-summed and compacted -> the c distinct j, kept in the workspace as well;
//   2. keys = doc_of_sorted[j] (the index in seq_ids order); sorted again over the next power of two of c -> cand_doc;
//   3. the lane that holds distinct document i finds its output slot by a binary search of its index in the sorted keys
//      (the indices are distinct, so the slots are) and writes the document's range there.
// Every output element is written once, by one lane; no atomics, nothing read back: graph-capturable, bit-reproducible.
#include "mm_internal.h"
#include "bitonic_device.h"
#include "scan_select_device.h"

namespace mm {

constexpr int kCandMaxH = 16384;          // hits per query: 64 KB of int32 keys
constexpr int kCandMaxGrid = kCUs;        // workgroups of a launch (and workspace slots); further queries by grid stride
constexpr int kCandThreads = 1024;
constexpr int kCandPer = kCandMaxH / kCandThreads;   // keys per lane in the compaction, at most
constexpr int32_t kCandNone = 0x7fffffff;            // sorts behind every document

struct CandArgs {
  const int64_t* hit;
  const int64_t* dbeg;
  const int64_t* dend;
  const int32_t* doc_of;
  int64_t n_docs, T;
  int64_t top;          // largest power of two <= n_docs: first step of the ownership search
  int nq, H, n2, C_cap;
  int32_t* cand_doc;
  int64_t* cand_begin;
  int64_t* cand_end;
  int32_t* cand_count;
  int32_t* ws;          // [gridDim.x, n2] the distinct sorted-view positions of the query a workgroup works on
};

// Owner of `row`: the last j with dbeg[j] <= row owns it when row < dend[j] (zero-length documents sort in front of a
// document that shares their begin, so they never own a row).  Fixed step count and no data-dependent branch: the U
// searches of a lane run side by side and their loads overlap.  Every load index is below n_docs whatever `row` is.
template <int U>
__device__ __forceinline__ void owners(const CandArgs& a, const int64_t (&row)[U], int32_t (&key)[U]) {
  uint32_t pos[U];                                        // n_docs < 2^31: pos + step fits
  bool ok[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    pos[u] = 0;
    ok[u] = row[u] >= 0 && row[u] < a.T;
  }
  const uint32_t n = (uint32_t)a.n_docs;
  for (uint32_t s = (uint32_t)a.top; s > 0; s >>= 1) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const uint32_t np = pos[u] + s;
      const bool can = ok[u] && np <= n;
      const int64_t b = a.dbeg[can ? np - 1 : 0];          // unconditional: no branch between the U loads of a step
      if (can && b <= row[u]) pos[u] = np;
    }
  }
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const bool in = ok[u] && pos[u] > 0;
    const int64_t e = a.dend[in ? pos[u] - 1 : 0];
    key[u] = (in && row[u] < e) ? (int32_t)(pos[u] - 1) : kCandNone;
  }
}

// 8 wavefronts per SIMD = two 1,024-thread workgroups per CU: at most 64 VGPRs
__global__ void __launch_bounds__(kCandThreads, 8) colbert_candidates_kernel(CandArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  int32_t* key = (int32_t*)smem;          // [n2]
  int32_t* wtot = key + a.n2;             // [16] flagged keys per wavefront
  const int tid = threadIdx.x, nt = blockDim.x;
  const int lane = tid & (kWave - 1), wave = tid / kWave, nwaves = nt / kWave;
  int32_t* ws = a.ws + (int64_t)blockIdx.x * a.n2;
  const int per = a.n2 > nt ? a.n2 / nt : 1;     // contiguous keys per lane in the compaction (n2 and nt are powers of two)

  for (int q = blockIdx.x; q < a.nq; q += gridDim.x) {
    const int64_t* hit = a.hit + (int64_t)q * a.H;
    // ---- 1. owners of the hits, four searches per lane at a time
    for (int base = tid; base < a.n2; base += 4 * nt) {
      int64_t row[4];
      int32_t k4[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int h = base + u * nt;
        row[u] = h < a.H ? hit[h] : -1;
      }
      owners<4>(a, row, k4);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int h = base + u * nt;
        if (h < a.n2) key[h] = k4[u];
      }
    }
    bitonic_asc(key, a.n2, tid, nt);

    // ---- first occurrences -> exclusive prefix sum -> compaction in place
    const int first = tid * per;
    int32_t mine[kCandPer];
    unsigned flags = 0;                                    // bit i: key first + i is a first occurrence
    if (first < a.n2) {
      int32_t prev = first > 0 ? key[first - 1] : -1;      // positions are >= 0: the first key is always a first occurrence
#pragma unroll
      for (int i = 0; i < kCandPer; ++i) {
        if (i < per) {
          const int32_t v = key[first + i];
          mine[i] = v;
          if (v != kCandNone && v != prev) flags |= 1u << i;
          prev = v;
        }
      }
    }
    const int n_mine = __popc(flags);
    int c;                                                 // (the helper's barrier also: every lane has read its keys)
    int off = block_offset_from_waves(wave_incl_scan(n_mine, lane), n_mine, wtot, lane, wave, nwaves, &c);
#pragma unroll
    for (int i = 0; i < kCandPer; ++i)
      if (flags >> i & 1u) key[off++] = mine[i];
    __syncthreads();

    // ---- 2. the c distinct documents by their index in seq_ids order
    const int c2 = pow2_ge(c);
    for (int i = tid; i < c2; i += nt) {
      int32_t d = kCandNone;
      if (i < c) {
        const int32_t j = key[i];
        ws[i] = j;                                         // read back below by this same lane
        d = a.doc_of[j];
      }
      key[i] = d;
    }
    bitonic_asc(key, c2, tid, nt);

    // ---- 3. outputs
    int32_t* o_doc = a.cand_doc + (int64_t)q * a.C_cap;
    int64_t* o_beg = a.cand_begin + (int64_t)q * a.C_cap;
    int64_t* o_end = a.cand_end + (int64_t)q * a.C_cap;
    for (int i = tid; i < a.C_cap; i += nt) {
      o_doc[i] = i < c ? key[i] : -1;
      if (i >= c) { o_beg[i] = 0; o_end[i] = 0; }
    }
    for (int i = tid; i < c; i += nt) {
      const int32_t j = ws[i];
      const int32_t d = a.doc_of[j];
      int lo = 0, hi = c;                                  // first slot whose key is >= d: below c, because d is a key
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (key[mid] < d) lo = mid + 1; else hi = mid;
      }
      if (lo >= c) lo = c - 1;                             // never taken for keys that hold d; keeps the store in bounds anyway
      o_beg[lo] = a.dbeg[j];
      o_end[lo] = a.dend[j];
    }
    if (tid == 0) a.cand_count[q] = c;
    __syncthreads();                                       // the keys are reused by the next query
  }
}

}  // namespace mm

using namespace mm;

extern "C" size_t mm_colbert_candidates_workspace_bytes(int nq, int H) {
  if (nq <= 0 || H < 1 || H > kCandMaxH) return 0;
  const int grid = nq < kCandMaxGrid ? nq : kCandMaxGrid;
  return (size_t)grid * pow2_ge(H) * sizeof(int32_t);
}

extern "C" int mm_colbert_candidates(const int64_t* hit_rows, const int64_t* doc_begin_sorted, const int64_t* doc_end_sorted,
                                     const int32_t* doc_of_sorted, int64_t n_docs, int64_t T, int nq, int H, int C_cap,
                                     int32_t* cand_doc, int64_t* cand_begin, int64_t* cand_end, int32_t* cand_count,
                                     void* workspace, size_t workspace_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!hit_rows || !doc_begin_sorted || !doc_end_sorted || !doc_of_sorted || !cand_doc || !cand_begin || !cand_end || !cand_count)
    return set_error(MM_EINVAL, "colbert_candidates: null pointer");
  if (nq < 0) return set_error(MM_EINVAL, "colbert_candidates: nq=%d", nq);
  if (H < 1 || H > kCandMaxH)
    return set_error(MM_EUNSUPPORTED, "colbert_candidates: H=%d hits per query outside 1 .. %d", H, kCandMaxH);
  if (n_docs < 1 || n_docs >= (1LL << 31) || T < 0)
    return set_error(MM_EUNSUPPORTED, "colbert_candidates: n_docs=%lld outside 1 .. 2^31-1 (or T=%lld negative)", (long long)n_docs,
                     (long long)T);
  if (C_cap < (H < n_docs ? H : (int)n_docs))
    return set_error(MM_EUNSUPPORTED, "colbert_candidates: C_cap=%d is below min(H, n_docs)=%d", C_cap, H < n_docs ? H : (int)n_docs);
  if (nq == 0) return MM_OK;
  const size_t need = mm_colbert_candidates_workspace_bytes(nq, H);
  if (!workspace || workspace_bytes < need) return set_error(MM_EWORKSPACE, "colbert_candidates: workspace needs %zu bytes", need);

  CandArgs a{};
  a.hit = hit_rows; a.dbeg = doc_begin_sorted; a.dend = doc_end_sorted; a.doc_of = doc_of_sorted;
  a.n_docs = n_docs; a.T = T; a.nq = nq; a.H = H; a.C_cap = C_cap;
  a.n2 = pow2_ge(H);
  a.top = 1;
  while (a.top * 2 <= n_docs) a.top *= 2;
  a.cand_doc = cand_doc; a.cand_begin = cand_begin; a.cand_end = cand_end; a.cand_count = cand_count;
  a.ws = (int32_t*)workspace;
  // a lane per key up to 1,024 (every key's search in flight at once), whole wavefronts
  const int threads = a.n2 < kWave ? kWave : (a.n2 < kCandThreads ? a.n2 : kCandThreads);
  const int grid = nq < kCandMaxGrid ? nq : kCandMaxGrid;
  const size_t lds = (size_t)a.n2 * 4 + 16 * 4;
  if (lds > 64 * 1024)
    (void)hipFuncSetAttribute((const void*)colbert_candidates_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL(colbert_candidates_kernel, dim3(grid), dim3(threads), lds, stream, a);
  return check_launch("colbert_candidates_kernel");
}
