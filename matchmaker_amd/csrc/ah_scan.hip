// Quantized list scan and exact re-score (dense retrieval, faiss_index_type: scann) for MI355X (gfx950 / CDNA4).
//
// Replaces, for one GPU's shard, the two scoring stages of the reference's ScaNN index (matchmaker/retrieval/
// scann_index.py:24-47: a tree of leaves, `score_ah(2, ...)` = 4-bit codes of 2-dimensional blocks, `reorder(top_n)` = the
// exact re-score of the best candidates; ScaNN itself is a third-party CPU library absent from the reference tree).
// Semantics restated here:
//
//   mm_ah_scan_fwd   score(q, i) = probe_scores[q, j] + <q, decode(codes[i])> for every row i of the lists the query probes
//                    (j = the probe that names i's list, decode = the concatenation of the row's codewords, products of
//                    16-bit values accumulated in fp32); the EXACT top-k of those scores, descending, lower row first.
//   mm_gather_dot    out[q, j] = <q, vectors[rows[q, j]]>, fp32-accumulated; -inf for a row of -1.
//
// The scan is ivf_scan.hip's with another score kernel: the ragged candidate rows, the rounds, the grouping of the
// (query, list) pairs by list and the radix selection are ivf_device.h's.
//
//   ah_score_kernel  LIST-MAJOR, one wavefront per 32-row block of a list.  The workgroup first copies the codebook into
//                    LDS as one dword (two 16-bit values) per (block, codeword): 32 E bytes, 24 KB at E 768.  A wavefront
//                    then DECODES its 32 rows once into the v_mfma_f32_32x32x16 A fragments that ivf_score_kernel loads
//                    from memory — lane (r, h) of k-step s holds elements 16 s + 8 h .. + 7 of row r = the codewords of
//                    blocks 8 s + 4 h .. + 3 = two bytes of codes and four dword look-ups — and multiplies them against
//                    every query that probes the list, exactly as ivf_score_kernel does.  Workgroups walk the task table
//                    with a grid stride, so the codebook is copied once per workgroup, not once per block.
//                    LDS layout: the 16 codewords of a block are 16 consecutive dwords = 16 distinct banks, so the 32 lanes
//                    of a half-wave (one block, 32 codes) never conflict: equal codes are one address.  The two half-waves
//                    read blocks 4 apart = 64 dwords apart = the same banks modulo 32; the table is stored with bit 4 of
//                    the dword index flipped for blocks with (block & 4), which puts half h = 1 on the other 16 banks.
//   gather_dot_kernel  16 lanes per (query, row) pair, 16 pairs per workgroup pass, four passes whose loads are issued
//                    together; the query's fragment stays in registers.
#include "ivf_device.h"

namespace mm {
using namespace ivf_dev;

template <int DT, int NSL>
__global__ void __launch_bounds__(256) ah_score_kernel(const IvfArgs a, int round) {
  constexpr int KS = NSL * 8;      // k-steps of 16
  constexpr int CB = NSL * 32;     // bytes of codes per row
  constexpr int RB = NSL * 256;    // bytes per query row
  constexpr int NT = NSL * 1024;   // dwords of the codebook: E / 2 blocks x 16 codewords
  extern __shared__ __attribute__((aligned(16))) uint32_t tab[];
  const int qa = a.qbeg[round];
  if (qa >= a.qbeg[round + 1]) return;   // uniform over the grid
  {
    const uint32_t* cb = (const uint32_t*)a.codebook;
    for (int i = threadIdx.x; i < NT; i += 256) tab[i ^ (((i >> 6) & 1) << 4)] = cb[i];   // i = block * 16 + code
  }
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r = lane & 31, h = lane >> 5;
  // byte offset of codeword 0 of block 8 s + 4 h + j inside k-step s's 128 dwords, with the swizzle applied
  int boff[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) boff[j] = (h * 64 + ((j ^ h) & 1) * 16 + (j & 2) * 16) * 4;
  const int ntask = a.tstart[a.nlist];
  const int64_t base0 = a.prefix[qa];
  for (int t = blockIdx.x * 4 + w; t < ntask; t += gridDim.x * 4) {
    const int l = a.blk_list[t];
    const int nqs = a.cnt[l];
    if (nqs == 0) continue;
    int64_t lb, len;
    list_range(a.lb, a.n, l, &lb, &len);
    const int row0 = (t - a.tstart[l]) * 32;
    const int rows = (int)(len - row0 < 32 ? len - row0 : 32);   // >= 1 by construction of the task table
    if (rows <= 0) continue;

    short8 af[KS];
    {
      const uint4* crow = (const uint4*)((const char*)a.v + (lb + row0 + (r < rows ? r : rows - 1)) * CB);   // never past the list
#pragma unroll
      for (int g = 0; g < KS / 4; ++g) {
        const uint4 cw = crow[g];
        const uint32_t wd[4] = {cw.x, cw.y, cw.z, cw.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int s = g * 4 + j;
          const uint32_t hw = wd[j] >> (16 * h);   // bytes 4 s + 2 h, 4 s + 2 h + 1: low nibble = the even block
          const char* ts = (const char*)(tab + s * 128);
          uint4 d;
          d.x = *(const uint32_t*)(ts + boff[0] + ((hw & 15u) << 2));
          d.y = *(const uint32_t*)(ts + boff[1] + (((hw >> 4) & 15u) << 2));
          d.z = *(const uint32_t*)(ts + boff[2] + (((hw >> 8) & 15u) << 2));
          d.w = *(const uint32_t*)(ts + boff[3] + (((hw >> 12) & 15u) << 2));
          af[s] = __builtin_bit_cast(short8, d);
        }
      }
    }
    const int32_t* pl = a.pairs + a.start[l];
    for (int t0 = 0; t0 < nqs; t0 += 32) {
      const int qi = t0 + r < nqs ? t0 + r : nqs - 1;
      const int64_t p = pl[qi];
      const int q = (int)(p / a.nprobe);
      const char* qrow = (const char*)a.q + (int64_t)q * RB + h * 16;
      f32x16 acc0 = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, acc1 = acc0;
#pragma unroll
      for (int s = 0; s < KS; s += 2) {
        acc0 = Mfma32x16<DT>::run(af[s], *(const short8*)(qrow + s * 32), acc0);
        acc1 = Mfma32x16<DT>::run(af[s + 1], *(const short8*)(qrow + (s + 1) * 32), acc1);
      }
      if (t0 + r < nqs) {
        const float ps = a.probe_scores[p];
        float* dst = a.cand + (a.prefix[q] - base0) + a.seg_off[p] + row0;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int row = rowof(i) + 4 * h;
          if (row < rows) dst[row] = ps + (acc0[i] + acc1[i]);
        }
      }
    }
  }
}

// Workgroup = 64 (query, row) pairs of ONE query: 16 lanes per pair, 16 pairs at a time, four passes.
template <int DT, int NSL>
__global__ void __launch_bounds__(256) gather_dot_kernel(const void* queries, const void* vectors, const int64_t* rows, float* out,
                                                         int64_t n, int R, int wg_per_q) {
  constexpr int RB = NSL * 256;   // bytes per row = NSL * 16 chunks of 16 bytes: NSL chunks per lane
  const int q = blockIdx.x / wg_per_q;
  const int j0 = (blockIdx.x - q * wg_per_q) * 64 + (threadIdx.x >> 4) * 4;
  const int c = threadIdx.x & 15;
  short8 qf[NSL];
#pragma unroll
  for (int i = 0; i < NSL; ++i) qf[i] = *(const short8*)((const char*)queries + (int64_t)q * RB + (c + 16 * i) * 16);
  short8 x[4][NSL];
  bool ok[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int j = j0 + u;
    const int64_t row = j < R ? rows[(int64_t)q * R + j] : -1;
    ok[u] = row >= 0 && row < n;
    const char* src = (const char*)vectors + (ok[u] ? row : 0) * RB;
#pragma unroll
    for (int i = 0; i < NSL; ++i) x[u][i] = ok[u] ? *(const short8*)(src + (c + 16 * i) * 16) : short8{0, 0, 0, 0, 0, 0, 0, 0};
  }
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    float acc = 0.0f;
#pragma unroll
    for (int i = 0; i < NSL; ++i)
#pragma unroll
      for (int e = 0; e < 8; ++e) acc = fmaf(bits_to_f32<DT>((uint16_t)x[u][i][e]), bits_to_f32<DT>((uint16_t)qf[i][e]), acc);
#pragma unroll
    for (int m = 8; m >= 1; m >>= 1) acc += __shfl_xor(acc, m, 16);
    if (c == 0 && j0 + u < R) out[(int64_t)q * R + j0 + u] = ok[u] ? acc : neg_inf();
  }
}

}  // namespace mm

using namespace mm;

extern "C" size_t mm_ah_scan_workspace_bytes(int64_t n_vectors, int nlist, int nq, int nprobe, int k) {
  (void)k;
  return ivf_workspace_bytes(n_vectors, nlist, nq, nprobe);
}

extern "C" int mm_ah_scan_fwd(const void* queries, const uint8_t* codes, const void* codebook, const int64_t* list_begin,
                              const int32_t* probes, const float* probe_scores, int64_t n_vectors, int nlist, int nq, int nprobe,
                              int E, int dtype, int k, float* out_scores, int64_t* out_rows, void* workspace,
                              size_t workspace_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!queries || !codebook || !list_begin || !probes || !probe_scores || !out_scores || !out_rows || (!codes && n_vectors > 0))
    return set_error(MM_EINVAL, "ah_scan: null pointer");
  if (int e = ivf_check("ah_scan", n_vectors, nlist, nq, nprobe, E, dtype, k)) return e;
  if (((uintptr_t)queries | (uintptr_t)codes) & 15) return set_error(MM_EINVAL, "ah_scan: 16-byte alignment required");
  if ((uintptr_t)codebook & 3) return set_error(MM_EINVAL, "ah_scan: the codebook must be 4-byte aligned");
  const size_t need = mm_ah_scan_workspace_bytes(n_vectors, nlist, nq, nprobe, k);
  if (!workspace || workspace_bytes < need) return set_error(MM_EWORKSPACE, "ah_scan: workspace needs %zu bytes", need);

  IvfArgs a{};
  a.q = queries; a.v = codes; a.codebook = codebook; a.probe_scores = probe_scores; a.lb = list_begin; a.probes = probes;
  a.n = n_vectors; a.nlist = nlist; a.nq = nq; a.nprobe = nprobe; a.k = k;
  a.out_s = out_scores; a.out_r = out_rows;
  return ivf_run(a, WsCursor(workspace, workspace_bytes), stream, "ah_scan", [&](const IvfArgs& b, int r, const IvfGeom& g) {
    // two workgroups per CU stay resident (192 VGPRs of A fragments at E 768); they walk the task table with a grid stride
    const int64_t wgs = (g.max_tasks + 3) / 4;
    const unsigned grid = (unsigned)(wgs < 4 * kCUs ? wgs : 4 * kCUs);
    return with_dtype16(dtype, [&](auto dt) {
      return with_nsl(E, [&](auto nsl) {
        hipLaunchKernelGGL((ah_score_kernel<MM_V(dt), MM_V(nsl)>), dim3(grid), dim3(256), (size_t)E * 32, stream, b, r);
        return check_launch("ah_score_kernel");
      });
    });
  });
}

extern "C" int mm_gather_dot(const void* queries, const void* vectors, const int64_t* rows, int64_t n_vectors, int nq, int R,
                             int E, int dtype, float* out, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!queries || !rows || !out || (!vectors && n_vectors > 0)) return set_error(MM_EINVAL, "gather_dot: null pointer");
  if (n_vectors < 0 || nq <= 0 || R <= 0) return set_error(MM_EINVAL, "gather_dot: non-positive shape");
  if (dtype != MM_F16 && dtype != MM_BF16) return set_error(MM_EUNSUPPORTED, "gather_dot: float16 / bfloat16 vectors only");
  if (!stream_width(E))
    return set_error(MM_EUNSUPPORTED, "gather_dot: E=%d is not one of 128, 256, 384, 512, 768 (pad the vectors)", E);
  if ((int64_t)nq * ((R + 63) / 64) >= (1LL << 31)) return set_error(MM_EUNSUPPORTED, "gather_dot: more than 2^31-1 workgroups");
  if (((uintptr_t)queries | (uintptr_t)vectors) & 15) return set_error(MM_EINVAL, "gather_dot: 16-byte alignment required");
  const int wpq = (R + 63) / 64;
  return with_dtype16(dtype, [&](auto dt) {
    return with_nsl(E, [&](auto nsl) {
      hipLaunchKernelGGL((gather_dot_kernel<MM_V(dt), MM_V(nsl)>), dim3((unsigned)((int64_t)nq * wpq)), dim3(256), 0, stream, queries,
                         vectors, rows, out, n_vectors, R, wpq);
      return check_launch("gather_dot_kernel");
    });
  });
}
