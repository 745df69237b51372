// Shared scaffolding of the list-major scans (ivf_scan.hip: 16-bit rows; ah_scan.hip: 4-bit codes; ivf_scan_fp8.hip: e4m3fn
// codes + row scales): the ragged candidate
// rows, the 32-row task table, the rounds, the counting sort of the (query, list) pairs by list and the exact radix
// selection (its scans and ivf_radix_kth are scan_select_device.h's).  A scan supplies its score kernel (one wavefront per
// 32-row block of a list, which writes every candidate score of the round) and runs through ivf_run: the two row scans
// instantiate ivf_score_kernel below over their row source, ah_scan.hip has its own.  Kernels have internal linkage: every
// translation unit that includes this header gets its own copy of the small ones.
#pragma once
#include "mm_internal.h"
#include "elem_device.h"
#include "bitonic_device.h"
#include "fp8_device.h"
#include "scan_select_device.h"

namespace mm {
namespace ivf_dev {

constexpr int kIvfMaxK = 4096;
constexpr int kIvfMaxProbe = 4096;
constexpr int64_t kIvfCapFloor = 1LL << 28;   // floats

struct IvfGeom {
  int64_t cap;      // floats in the candidate buffer
  int64_t S;        // round width in candidates (a round holds the queries whose prefix falls into [r S, (r + 1) S))
  int rounds;
  int64_t max_tasks;  // bound on the 32-row blocks over all lists
};

inline IvfGeom ivf_geom(int64_t n, int nlist, int nq) {
  IvfGeom g;
  const int64_t worst = (int64_t)nq * n;
  const int64_t cap_max = kIvfCapFloor > 2 * n ? kIvfCapFloor : 2 * n;
  if (worst <= cap_max) {
    g.cap = worst > 0 ? worst : 1;
    g.S = g.cap + 1;
    g.rounds = 1;
  } else {
    g.cap = cap_max;
    g.S = cap_max - n + 1;
    g.rounds = (int)((worst + g.S - 1) / g.S);
  }
  g.max_tasks = n / 32 + nlist + 1;
  return g;
}

struct IvfArgs {
  const void* q;            // [nq, E]
  const void* v;            // [n, E] rows (ivf_scan) / [n, E / 4] codes (ah_scan) / [n, E] e4m3fn codes (ivf_scan_fp8)
  const int64_t* lb;        // [nlist + 1]
  const int32_t* probes;    // [nq, nprobe]
  const void* codebook;     // ah_scan: [E / 2, 16, 2], the dtype of q
  const float* probe_scores;  // ah_scan: [nq, nprobe] added to every score of the pair's list
  const float* scales;      // ivf_scan_fp8: [n] power-of-two row scales, multiplied into the finished dot product
  int64_t n;
  int nlist, nq, nprobe, k;
  int64_t S;
  // once per call
  int32_t* seg_off;         // [nq, nprobe] offset of the pair's list inside the query's ragged row
  int32_t* total;           // [nq] candidates of the query
  int64_t* prefix;          // [nq + 1] exclusive prefix of `total`: a row starts at prefix[q] - prefix[first query of its round]
  int32_t* qbeg;            // [rounds + 1] first query of every round
  int32_t* tstart;          // [nlist + 1] first task (32-row block) of every list
  int32_t* blk_list;        // [max_tasks] list of every task
  // per round
  int32_t* cnt;             // [nlist] pairs of the round per list     } zeroed together before every round
  int32_t* fill;            // [nlist] fill level of the counting sort }
  int32_t* start;           // [nlist + 1]
  int32_t* pairs;           // [nq * nprobe] pair ids (q * nprobe + j) grouped by list
  float* cand;              // [cap]
  float* out_s;             // [nq, k]
  int64_t* out_r;           // [nq, k]
};

// one wavefront per query
static __global__ void __launch_bounds__(256) ivf_rows_kernel(const IvfArgs a) {
  const int lane = threadIdx.x & 63;
  const int q = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (q >= a.nq) return;
  int64_t carry = 0;
  for (int j0 = 0; j0 < a.nprobe; j0 += 64) {
    const int j = j0 + lane;
    int len = 0;
    if (j < a.nprobe) {
      const int l = a.probes[(int64_t)q * a.nprobe + j];
      if (l >= 0 && l < a.nlist) {
        int64_t b, ln;
        list_range(a.lb, a.n, l, &b, &ln);
        len = (int)ln;
      }
    }
    // a row never holds more than n_vectors candidates: lists named twice (an error) are dropped, not written past the buffer
    int64_t incl = wave_incl_scan<int64_t>(len, lane);
    if (carry + incl > a.n) len = 0;
    incl = wave_incl_scan<int64_t>(len, lane);
    if (j < a.nprobe) a.seg_off[(int64_t)q * a.nprobe + j] = (int32_t)(carry + incl - len);
    carry += __shfl((long long)incl, 63, 64);
  }
  if (lane == 0) a.total[q] = (int32_t)carry;
}

static __global__ void __launch_bounds__(1024) ivf_tasks_kernel(const IvfArgs a) {
  __shared__ int sh[1024];
  block_excl_scan<int>(
      [&](int l) {
        int64_t b, len;
        list_range(a.lb, a.n, l, &b, &len);
        return (int)((len + 31) >> 5);
      },
      [&](int l, int v) { a.tstart[l] = v; }, a.nlist, sh);
  __syncthreads();
  __threadfence_block();
  for (int l = threadIdx.x; l < a.nlist; l += 1024) {
    const int t0 = a.tstart[l], t1 = a.tstart[l + 1];
    for (int t = t0; t < t1; ++t) a.blk_list[t] = l;
  }
}

static __global__ void __launch_bounds__(1024) ivf_chunks_kernel(const IvfArgs a, int rounds) {
  __shared__ int64_t sh[1024];
  for (int r = threadIdx.x; r <= rounds; r += 1024) a.qbeg[r] = r == 0 ? 0 : a.nq;
  block_excl_scan<int64_t>([&](int q) { return (int64_t)a.total[q]; }, [&](int q, int64_t v) { a.prefix[q] = v; }, a.nq, sh);
  __syncthreads();
  __threadfence_block();
  // a row holds at most n_vectors < S candidates: the round number grows by at most one from a query to the next
  for (int q = threadIdx.x + 1; q < a.nq; q += 1024) {
    const int64_t r0 = a.prefix[q - 1] / a.S, r1 = a.prefix[q] / a.S;
    if (r1 != r0 && r1 < rounds) a.qbeg[r1] = q;
  }
}

// counting sort of the round's probe pairs by list: FILL = false counts, FILL = true places
template <bool FILL>
static __global__ void __launch_bounds__(256) ivf_group_kernel(const IvfArgs a, int round) {
  const int qa = a.qbeg[round], qb = a.qbeg[round + 1];
  const int64_t p1 = (int64_t)qb * a.nprobe;
  for (int64_t p = (int64_t)qa * a.nprobe + (int64_t)blockIdx.x * 256 + threadIdx.x; p < p1; p += (int64_t)gridDim.x * 256) {
    const int q = (int)(p / a.nprobe), j = (int)(p - (int64_t)q * a.nprobe);
    const int l = a.probes[p];
    if (l < 0 || l >= a.nlist) continue;
    const int end = j + 1 < a.nprobe ? a.seg_off[p + 1] : a.total[q];
    if (end == a.seg_off[p]) continue;   // empty (or dropped) list
    if (FILL) a.pairs[a.start[l] + atomicAdd(a.fill + l, 1)] = (int32_t)p;
    else atomicAdd(a.cnt + l, 1);
  }
}

static __global__ void __launch_bounds__(1024) ivf_lscan_kernel(const IvfArgs a, int round) {
  __shared__ int sh[1024];
  if (a.qbeg[round] >= a.qbeg[round + 1]) return;
  block_excl_scan<int>([&](int l) { return a.cnt[l]; }, [&](int l, int v) { a.start[l] = v; }, a.nlist, sh);
}

static __global__ void __launch_bounds__(1024) ivf_select_kernel(const IvfArgs a, int round, int k2) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  unsigned long long* sel = (unsigned long long*)smem;    // [k2] (key << 32 | row), ascending = the output order
  int* hist = (int*)(sel + k2);                            // [256]
  int* sh = hist + 256;                                    // [4]
  int* nsel = sh + 4;                                      // [1]
  const int tid = threadIdx.x;
  const int qa = a.qbeg[round];
  const int q = qa + blockIdx.x;
  if (q >= a.qbeg[round + 1]) return;
  const int C = a.total[q], k = a.k;
  const float* row = a.cand + (a.prefix[q] - a.prefix[qa]);
  const int32_t* so = a.seg_off + (int64_t)q * a.nprobe;
  const int32_t* pr = a.probes + (int64_t)q * a.nprobe;
  // position in the ragged row -> row of `vectors`: the last probe whose offset is <= pos has the position in its list
  auto vrow = [&](int pos) -> uint32_t {
    int lo = 0, hi = a.nprobe;   // first j with so[j] > pos
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (so[mid] <= pos) lo = mid + 1; else hi = mid;
    }
    const int j = lo - 1;
    int64_t b, len;
    list_range(a.lb, a.n, pr[j], &b, &len);
    return (uint32_t)(b + (pos - so[j]));
  };
  for (int i = tid; i < k2; i += 1024) sel[i] = ~0ull;
  if (tid == 0) *nsel = 0;
  __syncthreads();
  const int kk = C < k ? C : k;
  if (C <= k) {
    for (int i = tid; i < C; i += 1024) sel[i] = ((unsigned long long)desc_key(row[i]) << 32) | vrow(i);
  } else {
    int below, ties;
    const uint32_t T = ivf_radix_kth(C, k, [&](int) { return true; }, [&](int i) { return desc_key(row[i]); }, hist, sh, &below, &ties);
    uint32_t Trow = 0xffffffffu;
    if (below + ties > k) {   // more candidates tie with the k-th score than fit: the lower rows win
      int b2, t2;
      Trow = ivf_radix_kth(C, k - below, [&](int i) { return desc_key(row[i]) == T; }, vrow, hist, sh, &b2, &t2);
    }
    for (int i = tid; i < C; i += 1024) {
      const uint32_t kx = desc_key(row[i]);
      if (kx > T) continue;
      const uint32_t vr = vrow(i);
      if (kx == T && vr > Trow) continue;
      const int slot = atomicAdd(nsel, 1);
      if (slot < k) sel[slot] = ((unsigned long long)kx << 32) | vr;   // (slot >= k: only with a list probed twice)
    }
  }
  bitonic_asc(sel, k2, tid, 1024);      // (its first barrier orders the selection's writes before the sort)
  for (int i = tid; i < k; i += 1024) {
    const unsigned long long e = sel[i];
    const bool okv = i < kk && e != ~0ull;
    a.out_s[(int64_t)q * k + i] = okv ? desc_unkey((uint32_t)(e >> 32)) : neg_inf();
    a.out_r[(int64_t)q * k + i] = okv ? (int64_t)(uint32_t)e : -1;
  }
}

// ---- the score kernel of the row scans (ivf_scan.hip, ivf_scan_fp8.hip) -----------------------------------------------------
// A row-source policy turns the lane's part of row `trow` into the KS MFMA A fragments (lane (r, h): elements 16 s + 8 h .. + 7
// of k-step s) and names the factor of the finished dot product.

// 16-bit rows [n, E]: the fragment is the load.
struct IvfRows16 {
  static constexpr bool kScaled = false;
  template <int DT, int KS>
  static __device__ __forceinline__ void load(const IvfArgs& a, int64_t trow, int h, short8 (&af)[KS], float (&)[16]) {
    const char* arow = (const char*)a.v + trow * (KS * 32) + h * 16;
#pragma unroll
    for (int s = 0; s < KS; ++s) af[s] = *(const short8*)(arow + s * 32);
  }
};

// e4m3fn codes [n, E] + row scales [n]: 8 bytes per lane and k-step, converted once to the query's type (cvt8 at scale 1.0:
// exact); lane r (h = 0) fetches the scale of row r, and 16 cross-lane reads hand every lane the scales of its 16 accumulator
// rows (register i = row (i & 3) + 8 (i >> 2) + 4 h) — once per block.
struct IvfRowsFp8 {
  static constexpr bool kScaled = true;
  template <int DT, int KS>
  static __device__ __forceinline__ void load(const IvfArgs& a, int64_t trow, int h, short8 (&af)[KS], float (&sc)[16]) {
    const uint8_t* arow = (const uint8_t*)a.v + trow * (KS * 16) + h * 8;
#pragma unroll
    for (int s = 0; s < KS; ++s) af[s] = cvt8<DT>(*(const u32x2*)(arow + s * 16));
    const float mine = h == 0 ? a.scales[trow] : 0.0f;
#pragma unroll
    for (int i = 0; i < 16; ++i) sc[i] = __shfl(mine, rowof(i) + 4 * h, 64);
  }
};

// One wavefront per task = 32-row block of a list.  A = the block's rows (ROWS::load), B = 32 of the queries that probe the
// list (lane (r, h): query r, same elements); D: lane's column = its query, register i = row (i & 3) + 8 (i >> 2) + 4 h.
// A lane past the end of a partial last block reads the block's LAST row and never stores.
template <int DT, int NSL, class ROWS>
__global__ void __launch_bounds__(256) ivf_score_kernel(const IvfArgs a, int round) {
  constexpr int QB = NSL * 256;   // bytes per query
  constexpr int KS = NSL * 8;     // k-steps of 16
  const int qa = a.qbeg[round];
  if (qa >= a.qbeg[round + 1]) return;
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r = lane & 31, h = lane >> 5;
  const int64_t t = (int64_t)blockIdx.x * 4 + w;
  if (t >= a.tstart[a.nlist]) return;
  const int l = a.blk_list[t];
  const int nqs = a.cnt[l];
  if (nqs == 0) return;
  int64_t lb, len;
  list_range(a.lb, a.n, l, &lb, &len);
  const int row0 = (int)(t - a.tstart[l]) * 32;
  const int rows = (int)(len - row0 < 32 ? len - row0 : 32);   // >= 1 by construction of the task table
  if (rows <= 0) return;
  const int64_t base0 = a.prefix[qa];

  short8 af[KS];
  float sc[16];
  ROWS::template load<DT, KS>(a, lb + row0 + (r < rows ? r : rows - 1), h, af, sc);   // never past the list
  const int32_t* pl = a.pairs + a.start[l];
  for (int t0 = 0; t0 < nqs; t0 += 32) {
    const int qi = t0 + r < nqs ? t0 + r : nqs - 1;
    const int64_t p = pl[qi];
    const int q = (int)(p / a.nprobe);
    const char* qrow = (const char*)a.q + (int64_t)q * QB + h * 16;
    f32x16 acc0 = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, acc1 = acc0;
#pragma unroll
    for (int s = 0; s < KS; s += 2) {
      acc0 = Mfma32x16<DT>::run(af[s], *(const short8*)(qrow + s * 32), acc0);
      acc1 = Mfma32x16<DT>::run(af[s + 1], *(const short8*)(qrow + (s + 1) * 32), acc1);
    }
    if (t0 + r < nqs) {
      float* dst = a.cand + (a.prefix[q] - base0) + a.seg_off[p] + row0;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int row = rowof(i) + 4 * h;
        if (row < rows) dst[row] = ROWS::kScaled ? (acc0[i] + acc1[i]) * sc[i] : acc0[i] + acc1[i];
      }
    }
  }
}

// The workspace of a scan, stated once: block by block in the order of IvfArgs.  On a measuring cursor this leaves the size in
// ws.used (ivf_workspace_bytes), on a call's workspace it sets the pointers of `a` (ivf_run).
inline void ivf_layout(IvfArgs& a, const IvfGeom& g, WsCursor& ws) {
  const size_t pairs = (size_t)a.nq * a.nprobe, nq = (size_t)a.nq, nlist = (size_t)a.nlist;
  a.seg_off = ws.take<int32_t>(pairs);
  a.pairs = ws.take<int32_t>(pairs);
  a.total = ws.take<int32_t>(nq);
  a.prefix = ws.take<int64_t>(nq + 1);
  a.qbeg = ws.take<int32_t>((size_t)g.rounds + 1);
  a.tstart = ws.take<int32_t>(nlist + 1);
  a.start = ws.take<int32_t>(nlist + 1);
  a.blk_list = ws.take<int32_t>((size_t)g.max_tasks);
  a.cnt = ws.take<int32_t>(2 * nlist);      // cnt | fill in ONE block: a round zeroes both with one memset
  a.fill = a.cnt ? a.cnt + nlist : nullptr;
  a.cand = ws.take<float>((size_t)g.cap);
}

inline size_t ivf_workspace_bytes(int64_t n_vectors, int nlist, int nq, int nprobe) {
  if (n_vectors < 0 || nlist <= 0 || nq <= 0 || nprobe <= 0) return 0;
  IvfArgs a{};
  a.n = n_vectors; a.nlist = nlist; a.nq = nq; a.nprobe = nprobe;
  WsCursor measure;
  ivf_layout(a, ivf_geom(n_vectors, nlist, nq), measure);
  return measure.used;
}

// The checks both scans share (`what` names the caller), before any launch.
inline int ivf_check(const char* what, int64_t n_vectors, int nlist, int nq, int nprobe, int E, int dtype, int k) {
  if (n_vectors < 0 || nlist <= 0 || nq <= 0 || nprobe <= 0 || k <= 0) return set_error(MM_EINVAL, "%s: non-positive shape", what);
  if (dtype != MM_F16 && dtype != MM_BF16) return set_error(MM_EUNSUPPORTED, "%s: float16 / bfloat16 vectors only", what);
  if (k > kIvfMaxK || nprobe > kIvfMaxProbe)
    return set_error(MM_EUNSUPPORTED, "%s: k=%d / nprobe=%d exceed %d / %d", what, k, nprobe, kIvfMaxK, kIvfMaxProbe);
  if (n_vectors >= (1LL << 31) || (int64_t)nq * nprobe >= (1LL << 31))
    return set_error(MM_EUNSUPPORTED, "%s: more than 2^31-1 vectors or (query, probe) pairs in one call", what);
  if (!stream_width(E))
    return set_error(MM_EUNSUPPORTED, "%s: E=%d is not one of 128, 256, 384, 512, 768 (pad the vectors)", what, E);
  return MM_OK;
}

// Carves the workspace (which the caller has compared with ivf_workspace_bytes), enqueues the preparation and every round.
// `a` arrives with the inputs, the shape and the outputs set; score(a, round, g) enqueues the caller's score kernel for one
// round and returns MM_OK or an error.
template <typename Score>
int ivf_run(IvfArgs a, WsCursor ws, hipStream_t stream, const char* what, Score score) {
  const IvfGeom g = ivf_geom(a.n, a.nlist, a.nq);
  const size_t pairs = (size_t)a.nq * a.nprobe;
  const int nlist = a.nlist, nq = a.nq, k = a.k;
  a.S = g.S;
  ivf_layout(a, g, ws);

  hipLaunchKernelGGL(ivf_rows_kernel, dim3((nq + 3) / 4), dim3(256), 0, stream, a);
  hipLaunchKernelGGL(ivf_tasks_kernel, dim3(1), dim3(1024), 0, stream, a);
  hipLaunchKernelGGL(ivf_chunks_kernel, dim3(1), dim3(1024), 0, stream, a, g.rounds);
  if (int e = check_launch(what)) return e;

  const int k2 = pow2_ge(k);
  const size_t lds_sel = (size_t)k2 * 8 + 256 * 4 + 32;
  const unsigned grid_pairs = (unsigned)((pairs + 255) / 256 < 4096 ? (pairs + 255) / 256 : 4096);
  for (int r = 0; r < g.rounds; ++r) {
    if (hipMemsetAsync(a.cnt, 0, (size_t)nlist * 8, stream) != hipSuccess) return set_error(MM_ELAUNCH, "%s: memset failed", what);
    hipLaunchKernelGGL(ivf_group_kernel<false>, dim3(grid_pairs), dim3(256), 0, stream, a, r);
    hipLaunchKernelGGL(ivf_lscan_kernel, dim3(1), dim3(1024), 0, stream, a, r);
    hipLaunchKernelGGL(ivf_group_kernel<true>, dim3(grid_pairs), dim3(256), 0, stream, a, r);
    if (int e = check_launch(what)) return e;
    if (int e = score(a, r, g)) return e;
    hipLaunchKernelGGL(ivf_select_kernel, dim3(nq), dim3(1024), lds_sel, stream, a, r, k2);
    if (int e = check_launch("ivf_select_kernel")) return e;
  }
  return MM_OK;
}

}  // namespace ivf_dev
}  // namespace mm
