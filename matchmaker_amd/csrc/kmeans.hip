// k-means building blocks (IVF training, query clustering) for MI355X (gfx950 / CDNA4).
//
// Replaces, for one GPU, the arithmetic of the reference's dynamic IVF index (matchmaker/retrieval/faiss_indices.py:323-352
// FaissDynamicIndexer.prepare = faiss k-means over the query vectors, :401-428 search_single = the quantizer's nearest
// centroid) and of the per-query assignment loop of matchmaker/distillation/query_clusterer.py:218-221.  Both are
// maximum-inner-product assignment against a centroid table; the centroid update is a sum of rows per list.
//
// Everything is enqueued on the caller's stream; no host read-back, no allocation, no atomics: the calls are graph-capturable
// and their results are pure functions of their inputs.
//
//   mm_kmeans_assign
//     kmeans_assign_kernel   one workgroup (4 wavefronts) per 128 rows of x.  A wavefront loads its 32 rows ONCE as MFMA B
//                            fragments (registers: E/16 short8 per lane) and keeps them for the whole call.  The centroid table
//                            is walked in blocks of 32 rows: the workgroup stages a block in LDS (double buffered, rows padded
//                            by 16 bytes so that the 128-bit fragment reads are conflict free), every wavefront reads it as A
//                            fragments and runs one v_mfma_f32_32x32x16 chain of E/16 steps.  Centroids on M, rows of x on N: a
//                            lane owns ONE row of x and gets 16 of the block's scores in its accumulator registers, in
//                            ascending centroid order, so the running (max, arg) lives in two registers per lane and a strict
//                            `>` keeps the lowest centroid on equal scores.  The two lanes of a row (centroid rows 8 g + 0..3
//                            and 8 g + 4..7) are combined at the end on (score descending, centroid ascending).  8 bytes per
//                            row are written; no score matrix exists anywhere.
//   mm_kmeans_segment_sum
//     kms_tasks_kernel       one workgroup: list l has ceil(len / 512) chunks; exclusive scan of the chunk counts (tstart)
//     kms_partial_kernel     one workgroup per chunk: thread (rl, cg) sums the 8 columns 8 cg .. 8 cg + 7 of the chunk's rows
//                            rl, rl + RL, .. in that order (RL = 256 / (E / 8) row lanes), the RL partial rows are added in
//                            ascending rl through LDS.  A list of ONE chunk is written straight to `sums`, the chunks of a
//                            longer list go to the workspace.
//     kms_combine_kernel     one workgroup per list: zeros for an empty list, the chunks of a long list added in ascending order
#include "mm_internal.h"
#include "elem_device.h"
#include "scan_select_device.h"

namespace mm {

constexpr int kKmMaxLists = 65536;
constexpr int kKmSplit = 512;     // rows per chunk of the segment sum
constexpr int kKmTile = 128;      // rows of x per workgroup of the assignment (4 wavefronts x 32)
constexpr int kKmBlock = 32;      // centroids per LDS block

// A = the centroid block from LDS (lane (r, h): centroid c0 + r, elements 16 s + 8 h .. + 7 of k-step s), B = the wavefront's 32
// rows of x (lane (r, h): row r, same elements); D: lane's column = its row of x, register i = centroid c0 + rowof(i) + 4 h.
template <int DT, int NSL>
__global__ void __launch_bounds__(256) kmeans_assign_kernel(const void* __restrict__ x, const void* __restrict__ cent, int64_t n,
                                                            int nlist, int32_t* __restrict__ out_list,
                                                            float* __restrict__ out_score) {
  constexpr int RB = NSL * 256;        // bytes per row
  constexpr int KS = NSL * 8;          // k-steps of 16
  constexpr int LROW = RB + 16;        // LDS row pitch
  constexpr int CPR = RB / 16;         // 16-byte pieces per row
  constexpr int NST = 2 * NSL;         // pieces per thread and block (32 CPR / 256)
  extern __shared__ __attribute__((aligned(16))) char smem[];   // [2][32][LROW]
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int64_t row = (int64_t)blockIdx.x * kKmTile + w * 32 + r;

  short8 bf[KS];
  {
    const char* xrow = (const char*)x + (row < n ? row : n - 1) * RB + h * 16;   // n >= 1: never past the last row
#pragma unroll
    for (int s = 0; s < KS; ++s) bf[s] = *(const short8*)(xrow + s * 32);
  }

  short8 st[NST];
  auto fetch = [&](int c0) {
#pragma unroll
    for (int j = 0; j < NST; ++j) {
      const int p = tid + 256 * j;
      const int cr = p / CPR, cc = p - cr * CPR;
      const int c = c0 + cr < nlist ? c0 + cr : nlist - 1;   // the last block repeats the last centroid
      st[j] = *(const short8*)((const char*)cent + (int64_t)c * RB + cc * 16);
    }
  };
  auto stash = [&](int buf) {
#pragma unroll
    for (int j = 0; j < NST; ++j) {
      const int p = tid + 256 * j;
      const int cr = p / CPR, cc = p - cr * CPR;
      *(short8*)(smem + buf * (kKmBlock * LROW) + cr * LROW + cc * 16) = st[j];
    }
  };

  float best = neg_inf();
  int arg = 0;
  const int nb = (nlist + kKmBlock - 1) / kKmBlock;
  fetch(0);
  stash(0);
  __syncthreads();
  for (int b = 0; b < nb; ++b) {
    const int c0 = b * kKmBlock;
    if (b + 1 < nb) fetch(c0 + kKmBlock);
    const char* arow = smem + (b & 1) * (kKmBlock * LROW) + r * LROW + h * 16;
    f32x16 acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int s = 0; s < KS; ++s) acc = Mfma32x16<DT>::run(*(const short8*)(arow + s * 32), bf[s], acc);
    if (c0 + kKmBlock <= nlist) {
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int c = c0 + rowof(i) + 4 * h;
        if (acc[i] > best) { best = acc[i]; arg = c; }
      }
    } else {
      // the repeated last centroid keeps its own number: a copy can tie with it but never replace a lower centroid
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        int c = c0 + rowof(i) + 4 * h;
        c = c < nlist ? c : nlist - 1;
        if (acc[i] > best) { best = acc[i]; arg = c; }
      }
    }
    if (b + 1 < nb) stash((b + 1) & 1);
    __syncthreads();
  }
  const float ob = __shfl_xor(best, 32, 64);
  const int oa = __shfl_xor(arg, 32, 64);
  if (ob > best || (ob == best && oa < arg)) { best = ob; arg = oa; }
  if (h == 0 && row < n) {
    out_list[row] = arg;
    out_score[row] = best;
  }
}

// ---- segment sums ---------------------------------------------------------------------------------------------------------

struct KmsArgs {
  const void* x;            // [n, E]
  const int64_t* order;     // [n]
  const int64_t* lb;        // [nlist + 1]
  int64_t n;
  int nlist, E;
  int64_t max_tasks;        // chunks the workspace holds
  int32_t* tstart;          // [nlist + 1] first chunk of every list
  float* partial;           // [max_tasks, E]
  float* sums;              // [nlist, E]
};

__global__ void __launch_bounds__(1024) kms_tasks_kernel(const KmsArgs a) {
  __shared__ int sh[1024];
  block_excl_scan<int>(
      [&](int l) {
        int64_t b, len;
        list_range(a.lb, a.n, l, &b, &len);
        return (int)((len + kKmSplit - 1) / kKmSplit);
      },
      [&](int l, int v) { a.tstart[l] = v; }, a.nlist, sh);
}

template <int DT>
__global__ void __launch_bounds__(256) kms_partial_kernel(const KmsArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];   // [RL][E] float
  float* red = (float*)smem;
  const int64_t t = blockIdx.x;
  const int total = a.tstart[a.nlist];
  if (t >= total) return;
  int lo = 0, hi = a.nlist;                 // the last list whose first chunk is <= t (empty lists share a start: skipped)
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (a.tstart[mid] <= t) lo = mid; else hi = mid;
  }
  const int l = lo;
  int64_t lbeg, len;
  list_range(a.lb, a.n, l, &lbeg, &len);
  const int nch = a.tstart[l + 1] - a.tstart[l];
  const int c = (int)(t - a.tstart[l]);
  const int64_t p0 = lbeg + (int64_t)c * kKmSplit;
  const int rows = (int)(len - (int64_t)c * kKmSplit < kKmSplit ? len - (int64_t)c * kKmSplit : kKmSplit);
  const int E = a.E, CG = E >> 3, RL = 256 / CG;
  const int tid = threadIdx.x;
  const int rl = tid / CG, cg = tid - rl * CG;
  if (rl < RL) {
    float s[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const char* xb = (const char*)a.x + cg * 16;
    const int64_t rbytes = (int64_t)E * 2;
    int j = rl;
    for (; j + 3 * RL < rows; j += 4 * RL) {      // four rows in flight, added in row order
      short8 v[4];
      bool ok[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int64_t rr = a.order[p0 + j + u * RL];
        ok[u] = rr >= 0 && rr < a.n;
        v[u] = *(const short8*)(xb + (ok[u] ? rr : 0) * rbytes);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (ok[u]) {
#pragma unroll
          for (int e = 0; e < 8; ++e) s[e] += bits_to_f32<DT>((uint16_t)v[u][e]);
        }
    }
    for (; j < rows; j += RL) {
      const int64_t rr = a.order[p0 + j];
      if (rr >= 0 && rr < a.n) {
        const short8 v = *(const short8*)(xb + rr * rbytes);
#pragma unroll
        for (int e = 0; e < 8; ++e) s[e] += bits_to_f32<DT>((uint16_t)v[e]);
      }
    }
    float* dst = red + rl * E + cg * 8;
    *(f32x4*)dst = f32x4{s[0], s[1], s[2], s[3]};
    *(f32x4*)(dst + 4) = f32x4{s[4], s[5], s[6], s[7]};
  }
  __syncthreads();
  float* out = nch == 1 ? a.sums + (int64_t)l * E : (t < a.max_tasks ? a.partial + t * E : nullptr);
  if (!out) return;
  for (int col = tid; col < E; col += 256) {
    float v = red[col];
    for (int q = 1; q < RL; ++q) v += red[q * E + col];
    out[col] = v;
  }
}

__global__ void __launch_bounds__(256) kms_combine_kernel(const KmsArgs a) {
  const int l = blockIdx.x;
  const int64_t t0 = a.tstart[l];
  int nch = a.tstart[l + 1] - a.tstart[l];
  if (nch == 1) return;                                   // written by its only chunk
  if (t0 + nch > a.max_tasks) nch = t0 < a.max_tasks ? (int)(a.max_tasks - t0) : 0;   // (only with a list_begin that is not one)
  for (int col = threadIdx.x; col < a.E; col += 256) {
    float v = 0.0f;
    for (int c = 0; c < nch; ++c) v += a.partial[(t0 + c) * a.E + col];
    a.sums[(int64_t)l * a.E + col] = v;
  }
}

// The workspace of the segment sum, stated once: the size query runs it on a measuring cursor, the entry point on its workspace.
static void kms_layout(KmsArgs& a, WsCursor& ws) {
  a.max_tasks = a.n / kKmSplit + a.nlist;
  a.tstart = ws.take<int32_t>((size_t)a.nlist + 1);
  a.partial = ws.take<float>((size_t)a.max_tasks * a.E);
}

}  // namespace mm

using namespace mm;

extern "C" int mm_kmeans_assign(const void* x, const void* centroids, int64_t n, int nlist, int E, int dtype, int32_t* out_list,
                                float* out_score, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!centroids || ((!x || !out_list || !out_score) && n > 0)) return set_error(MM_EINVAL, "kmeans_assign: null pointer");
  if (n < 0) return set_error(MM_EINVAL, "kmeans_assign: negative row count");
  if (dtype != MM_F16 && dtype != MM_BF16) return set_error(MM_EUNSUPPORTED, "kmeans_assign: float16 / bfloat16 vectors only");
  if (nlist < 1 || nlist > kKmMaxLists) return set_error(MM_EUNSUPPORTED, "kmeans_assign: nlist=%d outside 1 .. %d", nlist, kKmMaxLists);
  if (n >= (1LL << 31)) return set_error(MM_EUNSUPPORTED, "kmeans_assign: more than 2^31-1 rows in one call");
  if (!stream_width(E)) return set_error(MM_EUNSUPPORTED, "kmeans_assign: E=%d is not one of 128, 256, 384, 512, 768 (pad the vectors)", E);
  if (((uintptr_t)x | (uintptr_t)centroids) & 15) return set_error(MM_EINVAL, "kmeans_assign: 16-byte alignment required");
  if (n == 0) return MM_OK;
  const unsigned grid = (unsigned)((n + kKmTile - 1) / kKmTile);
  const size_t lds = (size_t)2 * kKmBlock * (E * 2 + 16);
  return with_dtype16(dtype, [&](auto dt) {
    return with_nsl(E, [&](auto nsl) {
      const auto kernel = kmeans_assign_kernel<MM_V(dt), MM_V(nsl)>;
      if constexpr (MM_V(nsl) == 6) {     // 99,328 bytes of LDS: above the 64 KiB a kernel gets without asking
        const hipError_t attr = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (attr != hipSuccess) return set_error(MM_ELAUNCH, "kmeans_assign: %zu bytes of LDS refused: %s", lds, hipGetErrorString(attr));
      }
      hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), lds, stream, x, centroids, n, nlist, out_list, out_score);
      return check_launch("kmeans_assign_kernel");
    });
  });
}

extern "C" size_t mm_kmeans_segment_sum_workspace_bytes(int64_t n, int nlist, int E) {
  if (n < 0 || nlist <= 0 || E <= 0) return 0;
  KmsArgs a{};
  a.n = n; a.nlist = nlist; a.E = E;
  WsCursor measure;
  kms_layout(a, measure);
  return measure.used;
}

extern "C" int mm_kmeans_segment_sum(const void* x, const int64_t* order, const int64_t* list_begin, int64_t n, int nlist, int E,
                                     int dtype, float* sums, void* workspace, size_t workspace_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!list_begin || !sums || ((!x || !order) && n > 0)) return set_error(MM_EINVAL, "kmeans_segment_sum: null pointer");
  if (n < 0) return set_error(MM_EINVAL, "kmeans_segment_sum: negative row count");
  if (dtype != MM_F16 && dtype != MM_BF16) return set_error(MM_EUNSUPPORTED, "kmeans_segment_sum: float16 / bfloat16 vectors only");
  if (nlist < 1 || nlist > kKmMaxLists)
    return set_error(MM_EUNSUPPORTED, "kmeans_segment_sum: nlist=%d outside 1 .. %d", nlist, kKmMaxLists);
  if (n >= (1LL << 31)) return set_error(MM_EUNSUPPORTED, "kmeans_segment_sum: more than 2^31-1 rows in one call");
  if (!stream_width(E))
    return set_error(MM_EUNSUPPORTED, "kmeans_segment_sum: E=%d is not one of 128, 256, 384, 512, 768 (pad the vectors)", E);
  if (((uintptr_t)x | (uintptr_t)sums) & 15) return set_error(MM_EINVAL, "kmeans_segment_sum: 16-byte alignment required");
  const size_t need = mm_kmeans_segment_sum_workspace_bytes(n, nlist, E);
  if (!workspace || workspace_bytes < need) return set_error(MM_EWORKSPACE, "kmeans_segment_sum: workspace needs %zu bytes", need);

  KmsArgs a{};
  a.x = x; a.order = order; a.lb = list_begin; a.n = n; a.nlist = nlist; a.E = E; a.sums = sums;
  WsCursor ws(workspace, workspace_bytes);
  kms_layout(a, ws);
  hipLaunchKernelGGL(kms_tasks_kernel, dim3(1), dim3(1024), 0, stream, a);
  if (n > 0) {
    const int RL = 256 / (E >> 3);
    const size_t lds = (size_t)RL * E * 4;
    with_dtype16(dtype, [&](auto dt) {
      hipLaunchKernelGGL(kms_partial_kernel<MM_V(dt)>, dim3((unsigned)a.max_tasks), dim3(256), lds, stream, a);
      return MM_OK;
    });
  }
  hipLaunchKernelGGL(kms_combine_kernel, dim3(nlist), dim3(256), 0, stream, a);
  return check_launch("kmeans_segment_sum");
}
