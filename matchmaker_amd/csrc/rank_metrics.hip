// Ranking and IR metrics on the device: scores in arrival order -> per-query rank order -> the per-query quantities
// the reference's metric dicts are made of (matchmaker/utils/core_metrics.py:22-511).
//
//   mm_segment_rank_fwd        segmented STABLE descending sort (core_metrics.py:507, Python's sorted(reverse=True)):
//                              a 64-bit key per row = (order-preserving score key << 32) | arrival index, sorted ascending.
//                              Segments of <= 64 rows: one wavefront each, four per workgroup, every lane counts the keys
//                              below its own (keys are distinct, so the count is the rank); no LDS, no barrier.
//                              Longer segments: one workgroup each, the shared bitonic network (bitonic_device.h) over the
//                              next power of two of the segment's own length in LDS.
//   mm_rank_metrics_fwd        one wavefront per query walks its rows in rank order, 64 per step: ballots + lane prefix
//                              counts renumber the rows that pass the candidate threshold; the float64 terms of the judged
//                              rows (few) are added lane by lane in rank order into wave-uniform sums.
//   mm_rank_metrics_depth_fwd  every candidate threshold t = 1..hi at once: the query's (cand_pos, grade) pairs are staged in
//                              LDS in rank order and ONE LANE PER THRESHOLD walks them, counting the admitted rows (the merged
//                              rank) and adding its terms in rank order.  All lanes read the same LDS word in the same step
//                              (a broadcast) and the branch on "this row is judged" is wave-uniform.  Nothing of size
//                              [hi, hi] exists (core_metrics.py:40, 88-92 builds it).
// No atomics, no workspace, no read-back, vector stores only: graph-capturable, and two calls give the same bits.
#include "mm_internal.h"
#include "elem_device.h"
#include "bitonic_device.h"

namespace mm {

constexpr int kRankMaxLen = MM_RANK_MAX_LEN;      // 8192 rows x 8 bytes = 64 KiB of LDS keys
constexpr int kRankMaxCut = MM_RANK_MAX_CUTOFFS;
constexpr int32_t kNoGrade = INT32_MIN;           // MM_RANK_NOT_JUDGED
constexpr uint64_t kPadKey = ~0ull;               // sorts behind every row (a row's low word is < kRankMaxLen)

// ascending key = descending score, -0 == +0, every NaN on the one key behind -inf's; equal scores in arrival order
__device__ __forceinline__ uint64_t rank_key(float s, int i) { return ((uint64_t)desc_key_nan_last(s) << 32) | (uint32_t)i; }

// rows [beg, beg + len) of segment s, clamped into [0, n) whatever seg_begin holds
__device__ __forceinline__ void seg_range(const int64_t* sb, int s, int64_t n, int64_t* beg, int64_t* len) {
  int64_t b = sb[s], e = sb[s + 1];
  b = b < 0 ? 0 : (b > n ? n : b);
  e = e < b ? b : (e > n ? n : e);
  *beg = b;
  *len = e - b;
}

template <int DT>
__global__ void __launch_bounds__(256) seg_rank_wave_kernel(const void* scores, const int64_t* sb, int64_t n, int nq, int cap,
                                                            int32_t* order) {
  const int lane = threadIdx.x & 63;
  const int s = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (s >= nq) return;
  int64_t beg, len;
  seg_range(sb, s, n, &beg, &len);
  if (len > 64) {
    if (len > cap)      // longer than the caller's bound: arrival order (the workgroup kernel leaves it alone)
      for (int64_t i = lane; i < len; i += 64) order[beg + i] = (int32_t)(beg + i);
    return;
  }
  const bool in = lane < len;
  const uint64_t mine = in ? rank_key(load_elem<DT>(scores, beg + (in ? lane : 0)), lane) : kPadKey;
  int rank = 0;
  for (int j = 0; j < (int)len; ++j) {
    const uint32_t hi = __shfl((int)(mine >> 32), j, 64), lo = __shfl((int)(uint32_t)mine, j, 64);
    rank += ((((uint64_t)hi << 32) | lo) < mine) ? 1 : 0;
  }
  if (in) order[beg + rank] = (int32_t)(beg + lane);
}

template <int DT>
__global__ void seg_rank_block_kernel(const void* scores, const int64_t* sb, int64_t n, int cap, int32_t* order) {
  extern __shared__ uint64_t rank_keys[];
  const int tid = threadIdx.x, nt = blockDim.x;
  int64_t beg, len64;
  seg_range(sb, blockIdx.x, n, &beg, &len64);
  if (len64 <= 64 || len64 > cap) return;      // the wavefront kernel's (uniform over the workgroup: no barrier is skipped)
  const int len = (int)len64;
  const int n2 = pow2_ge(len, 128);             // <= the LDS of the launch: len <= cap <= its power of two
  for (int i = tid; i < n2; i += nt) rank_keys[i] = i < len ? rank_key(load_elem<DT>(scores, beg + i), i) : kPadKey;
  bitonic_asc(rank_keys, n2, tid, nt);
  for (int i = tid; i < len; i += nt) order[beg + i] = (int32_t)(beg + (int64_t)(uint32_t)rank_keys[i]);
}

// ---- metrics ------------------------------------------------------------------------------------------------------------
struct RmArgs {
  const int32_t* order;
  const int64_t* sb;
  const int32_t* grade;
  const int32_t* cpos;
  int64_t n;
  int nq, threshold, hi, tblocks;
  double binp;
  int nR, nN, map_cut;
  int rcut[kRankMaxCut], ncut[kRankMaxCut];
  const int32_t* bnr;
  const double* idcg;
  const double* lg;
  int32_t* first_rank;
  int32_t* hits;
  double* ap;
  double* ndcg;
};

__global__ void __launch_bounds__(256) rank_metrics_kernel(const RmArgs a) {
  const int lane = threadIdx.x & 63;
  const int q = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (q >= a.nq) return;
  int64_t beg, len;
  seg_range(a.sb, q, a.n, &beg, &len);
  const uint64_t below = (1ull << lane) - 1;
  int base = 0, kbase = 0, first = 0;
  bool any_judged = false, any_rel = false;
  int hits[kRankMaxCut];
  double dcg[kRankMaxCut], aps = 0.0;
#pragma unroll
  for (int c = 0; c < kRankMaxCut; ++c) { hits[c] = 0; dcg[c] = 0.0; }
  for (int64_t r0 = 0; r0 < len; r0 += 64) {
    const bool in = r0 + lane < len;
    const int row = in ? a.order[beg + r0 + lane] : -1;
    const bool ok = row >= 0 && row < a.n;
    const int g = ok ? a.grade[row] : kNoGrade;
    const bool keep = ok && (a.cpos == nullptr || a.cpos[row] <= a.threshold);
    const bool judged = g != kNoGrade;
    const bool rel = judged && (double)g >= a.binp;
    const uint64_t km = __ballot(keep);
    const int rank = base + __popcll(km & below) + 1;      // merged_ranks, core_metrics.py:252-254 (used where keep)
    base += __popcll(km);
    any_judged |= __ballot(judged) != 0;
    any_rel |= __ballot(rel) != 0;
    const bool rs = rel && keep;
    const uint64_t bm = __ballot(rs);
    const int k = kbase + __popcll(bm & below) + 1;
    if (first == 0 && bm != 0) first = __shfl(rank, __ffsll((long long)bm) - 1, 64);
    kbase += __popcll(bm);
#pragma unroll
    for (int c = 0; c < kRankMaxCut; ++c)
      if (c < a.nR) hits[c] += __popcll(__ballot(rs && rank <= a.rcut[c]));
    // the float64 sums, in rank order (the order of the sweep kernel's walk, so the two give the same bits): every judged
    // surviving row's terms are added from its lane, lowest lane first; the accumulators are wave-uniform
    const bool js = judged && keep;
    const double ap_t = rs && rank <= a.map_cut ? (double)k / (double)rank : 0.0;
    double dcg_t[kRankMaxCut];
#pragma unroll
    for (int c = 0; c < kRankMaxCut; ++c) dcg_t[c] = c < a.nN && js && rank <= a.ncut[c] ? (double)g / a.lg[rank] : 0.0;
    for (uint64_t jm = __ballot(js); jm != 0; jm &= jm - 1) {
      const int l = __ffsll((long long)jm) - 1;
      aps += __shfl(ap_t, l, 64);
#pragma unroll
      for (int c = 0; c < kRankMaxCut; ++c)
        if (c < a.nN) dcg[c] += __shfl(dcg_t[c], l, 64);
    }
  }
  if (lane != 0) return;
  a.first_rank[q] = first;
  a.ap[q] = any_rel ? aps / (double)a.bnr[q] : 0.0;
#pragma unroll
  for (int c = 0; c < kRankMaxCut; ++c) {
    if (c < a.nR) a.hits[(int64_t)q * a.nR + c] = hits[c];
    if (c < a.nN) a.ndcg[(int64_t)q * a.nN + c] = any_judged ? dcg[c] / a.idcg[(int64_t)q * a.nN + c] : 0.0;   // 0 / 0 = NaN as in the reference
  }
}

__global__ void __launch_bounds__(256) rank_metrics_depth_kernel(const RmArgs a) {
  extern __shared__ int32_t depth_rows[];
  int32_t* cp = depth_rows;            // [hi] cand_pos in rank order
  int32_t* gr = depth_rows + a.hi;     // [hi] grade in rank order
  const int tid = threadIdx.x;
  const int q = blockIdx.x / a.tblocks;
  const int t = (blockIdx.x - q * a.tblocks) * 256 + tid + 1;
  int64_t beg, len64;
  seg_range(a.sb, q, a.n, &beg, &len64);
  const int len = len64 > a.hi ? a.hi : (int)len64;      // (the Python layer refuses a longer segment, as the reference does)
  for (int i = tid; i < len; i += 256) {
    const int row = a.order[beg + i];
    const bool ok = row >= 0 && row < a.n;
    cp[i] = ok ? a.cpos[row] : INT32_MAX;
    gr[i] = ok ? a.grade[row] : kNoGrade;
  }
  __syncthreads();
  if (t > a.hi) return;
  int cnt = 0, k = 0, first = 0;
  bool any_judged = false, any_rel = false;
  int hits[kRankMaxCut];
  double dcg[kRankMaxCut], aps = 0.0;
#pragma unroll
  for (int c = 0; c < kRankMaxCut; ++c) { hits[c] = 0; dcg[c] = 0.0; }
  for (int p = 0; p < len; ++p) {
    const bool adm = cp[p] <= t;
    cnt += adm ? 1 : 0;                 // the merged rank of row p at threshold t, where admitted
    const int g = gr[p];
    if (g == kNoGrade) continue;        // wave-uniform
    any_judged = true;
    const bool rel = (double)g >= a.binp;
    any_rel |= rel;
    if (!adm) continue;
    if (rel) {
      ++k;
      if (first == 0) first = cnt;
      if (cnt <= a.map_cut) aps += (double)k / (double)cnt;
#pragma unroll
      for (int c = 0; c < kRankMaxCut; ++c)
        if (c < a.nR && cnt <= a.rcut[c]) ++hits[c];
    }
#pragma unroll
    for (int c = 0; c < kRankMaxCut; ++c)
      if (c < a.nN && cnt <= a.ncut[c]) dcg[c] += (double)g / a.lg[cnt];
  }
  const int64_t o = (int64_t)q * a.hi + (t - 1);
  a.first_rank[o] = first;
  a.ap[o] = any_rel ? aps / (double)a.bnr[q] : 0.0;
#pragma unroll
  for (int c = 0; c < kRankMaxCut; ++c) {
    if (c < a.nR) a.hits[o * a.nR + c] = hits[c];
    if (c < a.nN) a.ndcg[o * a.nN + c] = any_judged ? dcg[c] / a.idcg[(int64_t)q * a.nN + c] : 0.0;
  }
}

// The argument checks the two metric entries share; fills `a`.  Nothing is launched before they pass.
static int rm_check(const char* what, RmArgs& a, const int32_t* order, const int64_t* seg_begin, const int32_t* grade,
                    const int32_t* cand_pos, int64_t n_rows, int nq, double binp, const int32_t* mrr_cutoffs, int n_mrr,
                    const int32_t* ndcg_cutoffs, int n_ndcg, int map_cutoff, const int32_t* bnr, const double* idcg,
                    const double* log2_table, int n_log2, int32_t* first_rank, int32_t* hits, double* ap, double* ndcg) {
  if (nq < 0 || n_rows < 0) return set_error(MM_EINVAL, "%s: negative query or row count", what);
  if (n_rows >= (1LL << 31)) return set_error(MM_EUNSUPPORTED, "%s: more than 2^31-1 rows in one call", what);
  if (n_mrr < 0 || n_mrr > kRankMaxCut || n_ndcg < 0 || n_ndcg > kRankMaxCut)
    return set_error(MM_EUNSUPPORTED, "%s: %d MRR / %d nDCG cutoffs outside 0 .. %d", what, n_mrr, n_ndcg, kRankMaxCut);
  if ((n_mrr > 0 && !mrr_cutoffs) || (n_ndcg > 0 && !ndcg_cutoffs)) return set_error(MM_EINVAL, "%s: null cutoff list", what);
  if (map_cutoff < 1) return set_error(MM_EINVAL, "%s: map_cutoff=%d below 1", what, map_cutoff);
  for (int c = 0; c < n_mrr; ++c)
    if (mrr_cutoffs[c] < 1) return set_error(MM_EINVAL, "%s: MRR cutoff %d below 1", what, mrr_cutoffs[c]);
  for (int c = 0; c < n_ndcg; ++c) {
    if (ndcg_cutoffs[c] < 1) return set_error(MM_EINVAL, "%s: nDCG cutoff %d below 1", what, ndcg_cutoffs[c]);
    if (ndcg_cutoffs[c] >= n_log2)
      return set_error(MM_EINVAL, "%s: log2_table has %d entries, nDCG cutoff %d needs %d", what, n_log2, ndcg_cutoffs[c],
                       ndcg_cutoffs[c] + 1);
  }
  if (nq > 0 && (!seg_begin || !bnr || !first_rank || !ap || (n_mrr > 0 && !hits) || (n_ndcg > 0 && (!idcg || !ndcg || !log2_table))))
    return set_error(MM_EINVAL, "%s: null pointer", what);
  if (n_rows > 0 && nq > 0 && (!order || !grade)) return set_error(MM_EINVAL, "%s: null pointer", what);
  a.order = order; a.sb = seg_begin; a.grade = grade; a.cpos = cand_pos; a.n = n_rows; a.nq = nq; a.binp = binp;
  a.nR = n_mrr; a.nN = n_ndcg; a.map_cut = map_cutoff;
  for (int c = 0; c < kRankMaxCut; ++c) {
    a.rcut[c] = c < n_mrr ? mrr_cutoffs[c] : 0;
    a.ncut[c] = c < n_ndcg ? ndcg_cutoffs[c] : 0;
  }
  a.bnr = bnr; a.idcg = idcg; a.lg = log2_table; a.first_rank = first_rank; a.hits = hits; a.ap = ap; a.ndcg = ndcg;
  return MM_OK;
}

}  // namespace mm

using namespace mm;

extern "C" int mm_segment_rank_fwd(const void* scores, int dtype, const int64_t* seg_begin, int64_t n_rows, int nq, int max_len,
                                   int32_t* order, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (nq < 0 || n_rows < 0 || max_len < 0) return set_error(MM_EINVAL, "segment_rank: negative count");
  if (dtype != MM_F32 && dtype != MM_F16 && dtype != MM_BF16) return set_error(MM_EUNSUPPORTED, "segment_rank: unknown dtype %d", dtype);
  if (max_len > kRankMaxLen)
    return set_error(MM_EUNSUPPORTED, "segment_rank: max_len=%d above the native limit of %d rows per segment", max_len, kRankMaxLen);
  if (n_rows >= (1LL << 31)) return set_error(MM_EUNSUPPORTED, "segment_rank: more than 2^31-1 rows in one call");
  if (nq == 0 || n_rows == 0) return MM_OK;
  if (!scores || !seg_begin || !order) return set_error(MM_EINVAL, "segment_rank: null pointer");
  return with_dtype(dtype, [&](auto dt) {
    hipLaunchKernelGGL(seg_rank_wave_kernel<MM_V(dt)>, dim3((unsigned)((nq + 3) / 4)), dim3(256), 0, stream, scores, seg_begin,
                       n_rows, nq, max_len, order);
    if (max_len > 64) {
      const int n2 = pow2_ge(max_len, 128);
      const int nt = n2 / 2 > 1024 ? 1024 : n2 / 2;      // one comparator per thread per pass up to 2,048 rows
      hipLaunchKernelGGL(seg_rank_block_kernel<MM_V(dt)>, dim3((unsigned)nq), dim3(nt), (size_t)n2 * 8, stream, scores, seg_begin,
                         n_rows, max_len, order);
    }
    return check_launch("segment_rank");
  });
}

extern "C" int mm_rank_metrics_fwd(const int32_t* order, const int64_t* seg_begin, const int32_t* grade, const int32_t* cand_pos,
                                   int64_t n_rows, int nq, int threshold, double binarization_point, const int32_t* mrr_cutoffs,
                                   int n_mrr, const int32_t* ndcg_cutoffs, int n_ndcg, int map_cutoff,
                                   const int32_t* binary_num_relevant, const double* idcg, const double* log2_table, int n_log2,
                                   int32_t* first_rank, int32_t* hits, double* ap, double* ndcg, void* stream_) {
  RmArgs a{};
  const int rc = rm_check("rank_metrics", a, order, seg_begin, grade, cand_pos, n_rows, nq, binarization_point, mrr_cutoffs, n_mrr,
                          ndcg_cutoffs, n_ndcg, map_cutoff, binary_num_relevant, idcg, log2_table, n_log2, first_rank, hits, ap,
                          ndcg);
  if (rc != MM_OK) return rc;
  if (nq == 0) return MM_OK;
  a.threshold = threshold;
  hipLaunchKernelGGL(rank_metrics_kernel, dim3((unsigned)((nq + 3) / 4)), dim3(256), 0, (hipStream_t)stream_, a);
  return check_launch("rank_metrics");
}

extern "C" int mm_rank_metrics_depth_fwd(const int32_t* order, const int64_t* seg_begin, const int32_t* grade,
                                         const int32_t* cand_pos, int64_t n_rows, int nq, int hi, double binarization_point,
                                         const int32_t* mrr_cutoffs, int n_mrr, const int32_t* ndcg_cutoffs, int n_ndcg,
                                         int map_cutoff, const int32_t* binary_num_relevant, const double* idcg,
                                         const double* log2_table, int n_log2, int32_t* first_rank, int32_t* hits, double* ap,
                                         double* ndcg, void* stream_) {
  RmArgs a{};
  const int rc = rm_check("rank_metrics_depth", a, order, seg_begin, grade, cand_pos, n_rows, nq, binarization_point, mrr_cutoffs,
                          n_mrr, ndcg_cutoffs, n_ndcg, map_cutoff, binary_num_relevant, idcg, log2_table, n_log2, first_rank, hits,
                          ap, ndcg);
  if (rc != MM_OK) return rc;
  if (hi < 1) return set_error(MM_EINVAL, "rank_metrics_depth: hi=%d below 1", hi);
  if (hi > kRankMaxLen)
    return set_error(MM_EUNSUPPORTED, "rank_metrics_depth: hi=%d above the native limit of %d thresholds", hi, kRankMaxLen);
  if (n_rows > 0 && nq > 0 && !cand_pos) return set_error(MM_EINVAL, "rank_metrics_depth: cand_pos is needed");
  if (nq == 0) return MM_OK;
  a.hi = hi;
  a.tblocks = (hi + 255) / 256;
  if ((int64_t)nq * a.tblocks >= (1LL << 31)) return set_error(MM_EUNSUPPORTED, "rank_metrics_depth: nq * ceil(hi / 256) >= 2^31");
  hipLaunchKernelGGL(rank_metrics_depth_kernel, dim3((unsigned)(nq * a.tblocks)), dim3(256), (size_t)hi * 8, (hipStream_t)stream_, a);
  return check_launch("rank_metrics_depth");
}
