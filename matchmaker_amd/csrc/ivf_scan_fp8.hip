// IVF list scan over an fp8 token store (codes + row scales) for MI355X (gfx950 / CDNA4).
//
// The fp8 twin of ivf_scan.hip: the same reference lines (the list scan of FaissIVFIndexer.search,
// matchmaker/retrieval/faiss_indices.py:106-145), the same semantics (for every query the EXACT k best scores over the union
// of the lists named in its probe row, descending, lower row first on equal scores), with the lists held as the fp8 token
// store holds its rows: codes [n, E] OCP e4m3fn bytes + scales [n] float32 powers of two (mm_fp8_quantize_rows), list by list.
//
//   score(q, t) = scales[t] * sum_k queries[q, k] * deq(codes[t, k])
//
// The preparation, the rounds, the grouping and the selection are ivf_device.h's, shared with ivf_scan.hip and ah_scan.hip;
// so is the score kernel, one template with ivf_scan.hip's, here over the fp8 row source (IvfRowsFp8):
//
//   ivf_score_kernel       one wavefront per 32-row block of a list.  The block's codes are read ONCE (8 bytes per lane and
//                          k-step: 128 NSL bytes per row, half of the 16-bit scan's), converted ONCE to the query's 16-bit
//                          type (cvt8 at scale 1.0: exact) into the MFMA A fragments and multiplied against every query that
//                          probes the list, 32 queries per v_mfma_f32_32x32x16 chain.  Every product is exact and the sum is
//                          fp32.  A lane's 16 accumulators are 16 different rows, so the 32 row scales are fetched once per
//                          block, one lane per row, and handed to the lanes that need them by 16 cross-lane reads — once per
//                          block, not once per query tile.  The scale multiplies the FINISHED dot product (a power of two:
//                          exact) before the score is stored.  No LDS, no atomics: two calls give the same bits.
//
// Bounds: a lane past the end of a partial last block reads the block's LAST row (codes and scale alike) and never stores;
// no load uses a row index >= n_rows.
#include "fp8_device.h"
#include "ivf_device.h"

using namespace mm;
using namespace mm::ivf_dev;

extern "C" size_t mm_ivf_scan_fp8_workspace_bytes(int64_t n_rows, int nlist, int nq, int nprobe, int k) {
  (void)k;
  return ivf_workspace_bytes(n_rows, nlist, nq, nprobe);
}

extern "C" int mm_ivf_scan_fp8_fwd(const void* queries, const uint8_t* codes, const float* scales, const int64_t* list_begin,
                                   const int32_t* probes, int64_t n_rows, int nlist, int nq, int nprobe, int E, int q_dtype,
                                   int k, float* out_scores, int64_t* out_rows, void* workspace, size_t workspace_bytes,
                                   void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!queries || !list_begin || !probes || !out_scores || !out_rows || ((!codes || !scales) && n_rows > 0))
    return set_error(MM_EINVAL, "ivf_scan_fp8: null pointer");
  if (q_dtype == MM_F32)
    return set_error(MM_EUNSUPPORTED, "ivf_scan_fp8: the query is fp16 or bf16 (an fp32 query has no exact 16-bit MFMA operand)");
  if (int e = ivf_check("ivf_scan_fp8", n_rows, nlist, nq, nprobe, E, q_dtype, k)) return e;
  if ((((uintptr_t)queries | (uintptr_t)codes) & 15) || ((uintptr_t)scales & 3))
    return set_error(MM_EINVAL, "ivf_scan_fp8: queries / codes must be 16-byte aligned, scales 4-byte aligned");
  const size_t need = mm_ivf_scan_fp8_workspace_bytes(n_rows, nlist, nq, nprobe, k);
  if (!workspace || workspace_bytes < need) return set_error(MM_EWORKSPACE, "ivf_scan_fp8: workspace needs %zu bytes", need);

  IvfArgs a{};
  a.q = queries; a.v = codes; a.scales = scales; a.lb = list_begin; a.probes = probes;
  a.n = n_rows; a.nlist = nlist; a.nq = nq; a.nprobe = nprobe; a.k = k;
  a.out_s = out_scores; a.out_r = out_rows;
  return ivf_run(a, WsCursor(workspace, workspace_bytes), stream, "ivf_scan_fp8", [&](const IvfArgs& b, int r, const IvfGeom& g) {
    const unsigned grid_score = (unsigned)((g.max_tasks + 3) / 4);
    return with_dtype16(q_dtype, [&](auto dt) {
      return with_nsl(E, [&](auto nsl) {
        hipLaunchKernelGGL((ivf_score_kernel<MM_V(dt), MM_V(nsl), IvfRowsFp8>), dim3(grid_score), dim3(256), 0, stream, b, r);
        return check_launch("ivf_fp8_score_kernel");
      });
    });
  });
}
