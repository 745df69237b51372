// PACRR (matchmaker/models/pacrr.py:68-113): cosine match matrix -> n-gram convolutions + channel max -> per-row k-max
// pooling, fused.  Forward: ONE launch per call, one workgroup (four wavefronts) per pair; the match matrix lives only in
// LDS, as a ring of 64 document columns (two 32-column blocks: the block being pooled and the next one, whose first n - 1
// columns are the convolutions' right halo).  Backward: ONE launch, one workgroup per pair (see pacrr_bwd_kernel).
//
// The phases live in pacrr_device.h, shared with co_pacrr.hip (all of them) and matchpyramid.hip (the cosine).
// Arithmetic:
//   cosine   <q_i, d_j> * 1/(|q_i| + 1e-13) * 1/(|d_j| + 1e-13); the dot on v_mfma_f32_32x32x2_f32 (exact fp32: a k-ordered
//            fma chain), the four wavefronts split E and their partial tiles are summed in fixed order (deterministic);
//   conv     an im2col product [C x n^2] x [n^2 x 32 positions] on the same fp32 MFMA, the accumulator initialised with the
//            bias; the channel max is taken on the accumulators (lowest channel on ties, MaxPool3d's rule);
//   top-k    per (query row, path) a sorted list of k (value, column | channel << 16) in LDS, updated by whole-wave
//            insertions; ties keep the lower column first.
#include "pacrr_device.h"

namespace mm {

namespace {

using namespace pacrr_dev;

struct PacrrArgs {
  const float* q;
  const float* d;
  const float* w;   // packed conv weights: width n = 2 .. N, [C, n, n] each
  const float* b;   // packed biases: [N - 1, C]
  float* out;       // [n_pairs, Q, k N]
  int32_t* idx;     // optional [n_pairs, Q, k N]: column | channel << 16
  int64_t n_pairs, ppq;
  int Q, D, E, C, N, k;
};

__global__ void __launch_bounds__(256, 4) pacrr_fwd_kernel(PacrrArgs a) {
  extern __shared__ float lds[];
  const int Q = a.Q, D = a.D, E = a.E, C = a.C, N = a.N, k = a.k;
  const FwdLds L(Q, C, N, k);
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r32 = lane & 31;
  const int64_t pair = blockIdx.x;
  const float* q = a.q + (pair / a.ppq) * (int64_t)Q * E;
  const float* d = a.d + pair * (int64_t)D * E;
  const int nb = (D + 31) / 32, S = tap_off(N + 1);
  float* rq = lds + L.rq;
  float* rd = lds + L.rd;
  float* dn = lds + L.dn;
  float* wt = lds + L.wt;
  float* bs = lds + L.bs;
  float* ring = lds + L.ring;
  float* part = lds + L.part;
  float* tv = lds + L.tv;
  int* ti = (int*)(lds + L.ti);

  // prologue: weights, biases, zero halo rows of the ring, query norms (one wavefront per row)
  for (int i = tid; i < C * S; i += 256) wt[i] = a.w[i];
  for (int i = tid; i < C * (N - 1); i += 256) bs[i] = a.b[i];
  for (int i = tid; i < (Q + kPNmax) * kRing; i += 256) ring[i] = 0.0f;
  query_rnorms(q, Q, E, rq, w, lane);
  __syncthreads();

  for (int s = 0; s <= nb; ++s) {
    // ---- cosine block s -> ring half (s & 1); s == nb: the zero columns past the document (ConstantPad2d)
    const int j0 = 32 * s, rb = (s & 1) * 32;
    if (s < nb) cosine_block_partials(q, d, Q, D, E, j0, part, dn, w, lane);
    __syncthreads();
    if (s < nb) {
      cosine_block_finish(Q, part, dn, rq, rd, tid, [&](int i, int j, float v) { ring[i * kRing + rb + j] = v; });
    } else {
      for (int c = tid; c < Q * 32; c += 256) ring[(c >> 5) * kRing + rb + (c & 31)] = 0.0f;
    }
    __syncthreads();
    if (s == 0) continue;

    // ---- block s - 1: every path, every query row (rows are wavefront-owned: no barrier between paths)
    const int c0 = 32 * (s - 1), cb = ((s - 1) & 1) * 32;
    const int col = c0 + r32;
    const bool ok = col < D;
    const int cnt0 = (c0 < k ? c0 : k);
    for (int p = 0; p < N; ++p) {
      for (int r = w; r < Q; r += 4) {
        float v;
        int id;
        if (p == 0) {
          v = ring[r * kRing + ((cb + r32) & 63)];
          id = col;
        } else {
          const ConvMax m = conv_channel_max(wt, bs, ring, r, cb, p + 1, C, lane);
          v = m.v;
          id = col | (m.ch << 16);
        }
        const int base = (r * N + p) * k;
        float lv = lane < cnt0 ? tv[base + lane] : neg_inf();
        int li = lane < cnt0 ? ti[base + lane] : 0;
        int cnt = cnt0;
        topk_insert(lv, li, cnt, v, id, ok, k, lane);
        if (lane < cnt) {
          tv[base + lane] = lv;
          ti[base + lane] = li;
        }
      }
    }
    __syncthreads();
  }

  // per_query_results [Q, k N] in path order 0, 2, .., N (pacrr.py:97)
  float* o = a.out + pair * (int64_t)Q * N * k;
  for (int c = tid; c < Q * N * k; c += 256) o[c] = tv[c];
  if (a.idx) {
    int32_t* oi = a.idx + pair * (int64_t)Q * N * k;
    for (int c = tid; c < Q * N * k; c += 256) oi[c] = ti[c];
  }
}

// ---------------------------------------------------------------------------------------------------------------- backward
// One workgroup per pair: the family's backward through the value slots (pacrr_device.h, P0-P4) with K = k, grad_out as is.
__global__ void __launch_bounds__(256) pacrr_bwd_kernel(BwdArgs a) {
  extern __shared__ float lds[];
  const float* go = a.go + (int64_t)blockIdx.x * a.Q * a.N * a.k;
  bwd_value_slots(a, a.k, lds, [&](int i) { return go[i]; });
}

}  // namespace
}  // namespace mm

using namespace mm;

extern "C" size_t mm_pacrr_workspace_bytes(int64_t n_pairs, int Q, int D, int C, int N, int k) {
  (void)D;
  (void)C;
  if (n_pairs <= 0 || Q <= 0 || k <= 0 || N < 2) return 0;
  return (size_t)n_pairs * (size_t)Q * (size_t)k * (size_t)tap_off(N + 1) * sizeof(float);
}

extern "C" int mm_pacrr_fwd(const float* q, const float* d, const float* conv_w, const float* conv_b, float* out,
                            int32_t* saved_idx, int64_t n_pairs, int64_t pairs_per_query, int Q, int D, int E, int C, int N,
                            int k, void* workspace, size_t workspace_bytes, void* stream) {
  (void)workspace;
  (void)workspace_bytes;
  const char* what = "mm_pacrr_fwd";
  if (!q || !d || !out || (N >= 2 && (!conv_w || !conv_b)))
    return set_error(MM_EINVAL, "mm_pacrr_fwd: null q / d / out, or null conv_w / conv_b with N >= 2");
  int rc = check_pairs(n_pairs, pairs_per_query, what);
  if (rc == MM_OK) rc = check_shape(Q, D, E, C, N, k, kPKmax, what);
  if (rc != MM_OK || n_pairs == 0) return rc;
  PacrrArgs a{q, d, conv_w, conv_b, out, saved_idx, n_pairs, pairs_per_query, Q, D, E, C, N, k};
  return launch_per_pair(pacrr_fwd_kernel, a, FwdLds(Q, C, N, k).total, stream, what);
}

extern "C" int mm_pacrr_bwd(const float* q, const float* d, const float* conv_w, const int32_t* saved_idx,
                            const float* grad_out, float* grad_q, float* grad_d, float* grad_w, float* grad_b,
                            int64_t n_pairs, int64_t pairs_per_query, int Q, int D, int E, int C, int N, int k,
                            void* workspace, size_t workspace_bytes, void* stream) {
  const char* what = "mm_pacrr_bwd";
  if (!q || !d || !saved_idx || !grad_out || !grad_q || !grad_d || (N >= 2 && (!conv_w || !grad_w || !grad_b)))
    return set_error(MM_EINVAL, "mm_pacrr_bwd: null pointer argument");
  int rc = check_pairs(n_pairs, pairs_per_query, what);
  if (rc == MM_OK) rc = check_shape(Q, D, E, C, N, k, kPKmax, what);
  if (rc != MM_OK || n_pairs == 0) return rc;
  if ((rc = check_grid(n_pairs, what)) != MM_OK) return rc;   // reported before a workspace that is too small
  const size_t need = mm_pacrr_workspace_bytes(n_pairs, Q, D, C, N, k);
  if (need && (!workspace || workspace_bytes < need))
    return set_error(MM_EWORKSPACE, "mm_pacrr_bwd: workspace of %zu bytes, needs %zu", workspace_bytes, need);
  BwdArgs a{q, d, conv_w, saved_idx, grad_out, grad_q, grad_d, grad_w, grad_b, (float*)workspace, n_pairs,
            pairs_per_query, Q, D, E, C, N, k};
  return launch_per_pair(pacrr_bwd_kernel, a, BwdLds(Q, D, C, N, k).total, stream, what);
}
