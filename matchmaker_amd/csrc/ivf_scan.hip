// IVF list scan (dense retrieval, faiss_index_type: ivf) for MI355X (gfx950 / CDNA4).
//
// Replaces, for one GPU's shard, the list scan of the reference's GPU IVF index (matchmaker/retrieval/faiss_indices.py:106-145
// FaissIVFIndexer = IndexIVFFlat-style inverted lists searched with nprobe lists per query; faiss itself is a third-party
// dependency absent from the reference tree).  Semantics restated here: for every query the EXACT k largest inner products
// over the union of the lists named in its probe row, descending, lower row first on equal scores.
//
// Everything is enqueued on the caller's stream; no host read-back, no allocation: the call is graph-capturable.
//
//   once per call
//     ivf_rows_kernel    one wavefront per query: the prefix sum of its probed list lengths (seg_off) and their total —
//                        a query's candidate scores live in a RAGGED row, list after list in probe order
//     ivf_tasks_kernel   one workgroup: the 32-row blocks of every list, numbered list after list (tstart, blk_list)
//     ivf_chunks_kernel  one workgroup: prefix sum of the row totals over the queries -> the ROUND each query is scored in
//                        (round = prefix / S) and its row's offset in the candidate buffer.  S = CAP - n_vectors + 1, so the
//                        rows of one round always fit the CAP floats of the buffer.  The number of rounds R the host
//                        enqueues is the worst case ceil(nq n_vectors / S); rounds without queries return at once.
//   per round
//     ivf_group_kernel   (COUNT, then FILL) counting sort of the round's (query, list) probe pairs by list
//     ivf_lscan_kernel   one workgroup: exclusive scan of the per-list pair counts
//     ivf_score_kernel   LIST-MAJOR scoring.  One wavefront per 32-row block of a list: the block's rows are loaded ONCE as
//                        MFMA A fragments (registers: 8 x E/128 short8 per lane) and multiplied against every query that
//                        probes the list, 32 queries (B fragments, straight from global memory / L2) per
//                        v_mfma_f32_32x32x16 chain.  Rows on M, queries on N: a lane owns one query and writes that
//                        query's 16 scores into its ragged row.  No LDS.
//     ivf_select_kernel  one workgroup per query: exact radix select (4 x 8 bits of the order-preserving key) of the k-th
//                        score, a second radix select over the ROW numbers of the candidates that tie with it (lower row
//                        first), then a bitonic sort of the k survivors by (score descending, row ascending).
//
// The preparation, the grouping and the selection are ivf_device.h's, shared with ah_scan.hip; so is the score kernel, one
// template with ivf_scan_fp8.hip's, here over the 16-bit row source (IvfRows16).
//
// Workspace bound: CAP = min(nq n_vectors, max(2^28, 2 n_vectors)) floats of candidate scores (<= 1 GiB below 2^27
// vectors) + 12 bytes per (query, probe) pair + 20 bytes per query + 12 bytes per list + 4 bytes per 32-row block.
#include "ivf_device.h"

using namespace mm;
using namespace mm::ivf_dev;

extern "C" size_t mm_ivf_scan_workspace_bytes(int64_t n_vectors, int nlist, int nq, int nprobe, int k) {
  (void)k;
  return ivf_workspace_bytes(n_vectors, nlist, nq, nprobe);
}

extern "C" int mm_ivf_scan_fwd(const void* queries, const void* vectors, const int64_t* list_begin, const int32_t* probes,
                               int64_t n_vectors, int nlist, int nq, int nprobe, int E, int dtype, int k, float* out_scores,
                               int64_t* out_rows, void* workspace, size_t workspace_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!queries || !list_begin || !probes || !out_scores || !out_rows || (!vectors && n_vectors > 0))
    return set_error(MM_EINVAL, "ivf_scan: null pointer");
  if (int e = ivf_check("ivf_scan", n_vectors, nlist, nq, nprobe, E, dtype, k)) return e;
  if (((uintptr_t)queries | (uintptr_t)vectors) & 15) return set_error(MM_EINVAL, "ivf_scan: 16-byte alignment required");
  const size_t need = mm_ivf_scan_workspace_bytes(n_vectors, nlist, nq, nprobe, k);
  if (!workspace || workspace_bytes < need) return set_error(MM_EWORKSPACE, "ivf_scan: workspace needs %zu bytes", need);

  IvfArgs a{};
  a.q = queries; a.v = vectors; a.lb = list_begin; a.probes = probes;
  a.n = n_vectors; a.nlist = nlist; a.nq = nq; a.nprobe = nprobe; a.k = k;
  a.out_s = out_scores; a.out_r = out_rows;
  return ivf_run(a, WsCursor(workspace, workspace_bytes), stream, "ivf_scan", [&](const IvfArgs& b, int r, const IvfGeom& g) {
    const unsigned grid_score = (unsigned)((g.max_tasks + 3) / 4);
    return with_dtype16(dtype, [&](auto dt) {
      return with_nsl(E, [&](auto nsl) {
        hipLaunchKernelGGL((ivf_score_kernel<MM_V(dt), MM_V(nsl), IvfRows16>), dim3(grid_score), dim3(256), 0, stream, b, r);
        return check_launch("ivf_score_kernel");
      });
    });
  });
}
