// MaxP retrieval: passage hits -> distinct documents (matchmaker/dense_retrieval.py:414-429: the host loop that walks a
// query's hit list with a Python set and keeps the first hit of every id until top_n documents are found).
//
//   mm_distinct_hits_fwd   one workgroup per query.  The list's (id, position) keys go to LDS for the next power of two >= K
//                          and are sorted ascending by the shared bitonic network (bitonic_device.h).  An id is compared as
//                          an UNSIGNED 64-bit number, so its sign bit is the valid bit: every id < 0 (a dropped hit) and
//                          every padding slot sorts behind every valid id, INT64_MAX included, and no id value is reserved.
//                          A sorted element whose predecessor has another id is that id's lowest position = its first
//                          occurrence in list order; it sets a flag byte indexed by POSITION.  Every thread then owns a
//                          contiguous stretch of positions: a workgroup prefix sum over the stretches' (first occurrences,
//                          valid hits) counts, packed 16 + 16 bits, gives every first occurrence its rank, and those with
//                          rank < top_n are stored.  Scores are payload: read as 32-bit words where they are stored, never
//                          compared.
// No atomics, no workspace, no read-back, vector stores only, every output element stored exactly once: graph-capturable,
// and two calls give the same bits.
#include "mm_internal.h"
#include "bitonic_device.h"
#include "scan_select_device.h"

namespace mm {

constexpr int kDistinctMaxHits = MM_DISTINCT_MAX_HITS;      // 8192 x 16 bytes = 128 KiB of LDS keys
constexpr uint32_t kNegInfBits = 0xff800000u;

struct alignas(16) HitKey {
  uint64_t id;       // the id's bits; >= 2^63: dropped or padding
  uint64_t pos;      // position in the list (distinct, so the order is total)
  __device__ __forceinline__ bool operator>(const HitKey& o) const { return id > o.id || (id == o.id && pos > o.pos); }
};

// LDS of one workgroup: keys [n2], wave sums [16], flags [K]
inline size_t distinct_lds_bytes(int K, int n2) { return (size_t)n2 * sizeof(HitKey) + 16 * 4 + (size_t)((K + 15) & ~15); }

__global__ void __launch_bounds__(1024) distinct_hits_kernel(const uint32_t* hit_scores, const int64_t* hit_ids, int K, int n2,
                                                             int top_n, uint32_t* out_scores, int64_t* out_ids, int32_t* out_pos,
                                                             int32_t* n_distinct, int32_t* n_valid) {
  extern __shared__ __align__(16) unsigned char distinct_lds[];
  HitKey* key = (HitKey*)distinct_lds;               // [n2]
  uint32_t* wave_sum = (uint32_t*)(key + n2);        // [16]
  uint8_t* flag = (uint8_t*)(wave_sum + 16);         // [K]: bit 1 = valid hit, bit 0 = first occurrence of its id
  const int tid = threadIdx.x, nt = blockDim.x, lane = tid & 63, wave = tid >> 6;
  const int64_t q = blockIdx.x;
  const int64_t* ids = hit_ids + q * K;
  for (int i = tid; i < n2; i += nt) {
    const int64_t id = i < K ? ids[i] : -1;
    key[i] = HitKey{(uint64_t)id, (uint64_t)i};
    if (i < K) flag[i] = id >= 0 ? 2 : 0;
  }
  bitonic_asc(key, n2, tid, nt);
  for (int i = tid; i < n2; i += nt) {
    const HitKey k = key[i];
    if ((int64_t)k.id >= 0 && (i == 0 || key[i - 1].id != k.id)) flag[k.pos] = 3;      // k.pos < K: a valid key is a list entry
  }
  __syncthreads();
  // positions [p0, p1) are this thread's; counts packed as (valid << 16) | first occurrences, each <= 8192
  const int per = (K + nt - 1) / nt;
  const int p0 = tid * per < K ? tid * per : K, p1 = p0 + per < K ? p0 + per : K;
  uint32_t mine = 0;
  for (int p = p0; p < p1; ++p) {
    const uint32_t f = flag[p];
    mine += (f & 1u) + ((f >> 1) << 16);
  }
  uint32_t total;
  const uint32_t excl = block_offset_from_waves(wave_incl_scan(mine, lane), mine, wave_sum, lane, wave, nt >> 6, &total);
  const int distinct = (int)(total & 0xffffu), valid = (int)(total >> 16);
  int rank = (int)(excl & 0xffffu);
  const int64_t o = q * top_n;
  for (int p = p0; p < p1 && rank < top_n; ++p) {
    if (flag[p] & 1u) {
      out_scores[o + rank] = hit_scores[q * K + p];
      out_ids[o + rank] = ids[p];
      out_pos[o + rank] = p;
      ++rank;
    }
  }
  for (int r = (distinct < top_n ? distinct : top_n) + tid; r < top_n; r += nt) {
    out_scores[o + r] = kNegInfBits;
    out_ids[o + r] = -1;
    out_pos[o + r] = -1;
  }
  if (tid == 0) {
    n_distinct[q] = distinct;
    n_valid[q] = valid;
  }
}

}  // namespace mm

using namespace mm;

extern "C" int mm_distinct_hits_fwd(const float* hit_scores, const int64_t* hit_ids, int nq, int K, int top_n, float* out_scores,
                                    int64_t* out_ids, int32_t* out_pos, int32_t* n_distinct, int32_t* n_valid, void* stream_) {
  if (nq < 0) return set_error(MM_EINVAL, "distinct_hits: negative query count");
  if (K < 1 || K > kDistinctMaxHits)
    return set_error(MM_EUNSUPPORTED, "distinct_hits: K=%d outside 1 .. %d hits per query", K, kDistinctMaxHits);
  if (top_n < 1 || top_n > K) return set_error(MM_EUNSUPPORTED, "distinct_hits: top_n=%d outside 1 .. K=%d", top_n, K);
  if (nq == 0) return MM_OK;
  if (!hit_scores || !hit_ids || !out_scores || !out_ids || !out_pos || !n_distinct || !n_valid)
    return set_error(MM_EINVAL, "distinct_hits: null pointer");
  const int n2 = pow2_ge(K);
  const int nt = n2 / 2 > 1024 ? 1024 : (n2 / 2 < 64 ? 64 : n2 / 2);      // a multiple of 64: the scan's wavefronts are whole
  const size_t lds = distinct_lds_bytes(K, n2);
  if (lds > 64 * 1024) {
    const hipError_t e = hipFuncSetAttribute((const void*)distinct_hits_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess)
      return set_error(MM_ELAUNCH, "distinct_hits: %d bytes of dynamic LDS refused: %s", (int)lds, hipGetErrorString(e));
  }
  hipLaunchKernelGGL(distinct_hits_kernel, dim3((unsigned)nq), dim3(nt), lds, (hipStream_t)stream_, (const uint32_t*)hit_scores,
                     hit_ids, K, n2, top_n, (uint32_t*)out_scores, out_ids, out_pos, n_distinct, n_valid);
  return check_launch("distinct_hits_kernel");
}
