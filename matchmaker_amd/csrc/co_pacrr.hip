// CO-PACRR (matchmaker/models/co_pacrr.py:79-158): PACRR's cosine match matrix -> n-gram convolutions + channel max ->
// per-row k-max pipeline, with four nested document views and a context similarity gathered at every selected column.
// Forward: ONE launch per call, one workgroup (four wavefronts) per pair, PACRR's structure (csrc/pacrr.hip) on the same
// phase functions (pacrr_device.h): the match matrix lives in an LDS ring of 64 document columns.  Backward: ONE launch, one
// workgroup per pair: the family's value-slot backward, then the context slots.
//
// Additions to PACRR's forward:
//   context  ctx[j] = cosine(mean_i q_i, (1/6) sum_{t = j .. j+5, t < D} d_t) for every column j below min(v_3, D), computed
//            before the stream (one wavefront per column, lanes over E) and kept in LDS;
//   views    the view sizes v_0 <= .. <= v_3 are nested prefixes of the stream: the block holding min(v_i, D) inserts its
//            columns below it, copies the running list (values and ctx[col]) to view i's output slots, then inserts the rest.
//            No column at or past min(v_3, D) is inserted; the stream goes on to the next block for the conv halo.
// Ties (values and therefore contexts): descending, lower column first, lowest channel — PACRR's rule.
#include "pacrr_device.h"

namespace mm {

namespace {

using namespace pacrr_dev;

constexpr int kCoKmax = 8;   // 4 views x k <= 32 list lanes in the backward

struct CoArgs {
  const float* q;
  const float* d;
  const float* w;   // packed conv weights: width n = 2 .. N, [C, n, n] each
  const float* b;   // packed biases: [N - 1, C]
  float* out;       // [n_pairs, Q, N, 8k]: per path 4k values (views 0..3), then their 4k contexts
  int32_t* idx;     // optional [n_pairs, Q, N, 4k]: column | channel << 16 of every value slot
  int64_t n_pairs, ppq;
  int Q, D, E, C, N, k;
  int v0, v1, v2, v3;
};

// PACRR's forward layout plus the context similarities; the query context aliases `part` (free until the first cosine block)
struct CoFwdLds : FwdLds {
  int ctx;
  __host__ __device__ CoFwdLds(int Q, int D, int C, int N, int k) : FwdLds(Q, C, N, k) {
    ctx = total;
    total += D;
  }
};

__global__ void __launch_bounds__(256, 4) co_pacrr_fwd_kernel(CoArgs a) {
  extern __shared__ float lds[];
  const int Q = a.Q, D = a.D, E = a.E, C = a.C, N = a.N, k = a.k;
  const CoFwdLds L(Q, D, C, N, k);
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r32 = lane & 31;
  const int64_t pair = blockIdx.x;
  const float* q = a.q + (pair / a.ppq) * (int64_t)Q * E;
  const float* d = a.d + pair * (int64_t)D * E;
  const int nb = (D + 31) / 32, S = tap_off(N + 1);
  const int Dv = min(a.v3, D);                 // columns that enter a list
  const int nbp = (Dv + 31) / 32;        // blocks that are pooled
  float* rq = lds + L.rq;
  float* rd = lds + L.rd;
  float* dn = lds + L.dn;
  float* wt = lds + L.wt;
  float* bs = lds + L.bs;
  float* ring = lds + L.ring;
  float* part = lds + L.part;
  float* tv = lds + L.tv;
  int* ti = (int*)(lds + L.ti);
  float* ctx = lds + L.ctx;
  float* qc = part;

  // prologue: weights, biases, zero halo rows of the ring, query norms (one wavefront per row), query context (:98)
  for (int i = tid; i < C * S; i += 256) wt[i] = a.w[i];
  for (int i = tid; i < C * (N - 1); i += 256) bs[i] = a.b[i];
  for (int i = tid; i < (Q + kPNmax) * kRing; i += 256) ring[i] = 0.0f;
  query_rnorms(q, Q, E, rq, w, lane);
  for (int e = tid; e < E; e += 256) {
    float s = 0.0f;
    for (int i = 0; i < Q; ++i) s += q[(int64_t)i * E + e];
    qc[e] = s / (float)Q;
  }
  __syncthreads();

  // ---- context similarities ctx[j], j < Dv (:99-101): one wavefront per column, four elements per lane
  {
    float qq = 0.0f;
    for (int e = 4 * lane; e < E; e += 256) {
      qq += qc[e] * qc[e] + qc[e + 1] * qc[e + 1] + qc[e + 2] * qc[e + 2] + qc[e + 3] * qc[e + 3];
    }
    const float rqc = 1.0f / (sqrtf(wave_sum(qq)) + kTiny);
    for (int j = w; j < Dv; j += 4) {
      const int t1 = min(j + 6, D);
      float p1 = 0.0f, p2 = 0.0f;
      for (int e = 4 * lane; e < E; e += 256) {
        f32x4 s = *(const f32x4*)(d + (int64_t)j * E + e);
        for (int t = j + 1; t < t1; ++t) s += *(const f32x4*)(d + (int64_t)t * E + e);
        const f32x4 x = s / 6.0f;
        p1 += x[0] * qc[e] + x[1] * qc[e + 1] + x[2] * qc[e + 2] + x[3] * qc[e + 3];
        p2 += x[0] * x[0] + x[1] * x[1] + x[2] * x[2] + x[3] * x[3];
      }
      p1 = wave_sum(p1);
      p2 = wave_sum(p2);
      if (lane == 0) ctx[j] = (p1 * rqc) * (1.0f / (sqrtf(p2) + kTiny));
    }
  }
  __syncthreads();   // qc (in `part`) is dead from here on

  float* o = a.out + pair * (int64_t)Q * N * 8 * k;
  int32_t* oi = a.idx ? a.idx + pair * (int64_t)Q * N * 4 * k : nullptr;
  for (int s = 0; s <= nbp; ++s) {
    // ---- cosine block s -> ring half (s & 1); s >= nb: the zero columns past the document (ConstantPad2d)
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
        // views whose last column lies in this block: insert up to it, snapshot, go on (bnd[i] >= k: the list is full)
        int lo = c0;
#pragma unroll 1
        for (int i = 0; i < 4; ++i) {
          const int bi = min(i == 0 ? a.v0 : i == 1 ? a.v1 : i == 2 ? a.v2 : a.v3, D);
          if (bi > c0 && bi <= c0 + 32) {
            topk_insert(lv, li, cnt, v, id, col >= lo && col < bi, k, lane);
            lo = bi;
            if (lane < k) {
              float* ov = o + ((int64_t)r * N + p) * 8 * k;
              ov[i * k + lane] = lv;
              ov[4 * k + i * k + lane] = ctx[li & 0xffff];
              if (oi) oi[((int64_t)r * N + p) * 4 * k + i * k + lane] = li;
            }
          }
        }
        topk_insert(lv, li, cnt, v, id, col >= lo && col < Dv, k, lane);
        if (lane < cnt) {
          tv[base + lane] = lv;
          ti[base + lane] = li;
        }
      }
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------------------------------------------- backward
struct CoBwdArgs : BwdArgs {   // idx [n_pairs, Q, N, 4k], go [n_pairs, Q, N, 8k], wincos [n_pairs, Q 4k S]; k is the model's
  float* gdctx;         // workspace [n_pairs, D, E]: d(loss)/d(dctx_j) / 6
  float* gqh;           // workspace [n_pairs, 4, E]: per-wavefront partials of d(loss)/d(qctx-hat)
};

// One workgroup per pair.  P0-P4 are the family's backward (pacrr_device.h, bwd_value_slots) over the K = 4k VALUE slots of
// every (row, path) — the first 4k of the path's 8k gradients: a column chosen by several views appears in several slots and
// every slot adds its own term.  P5 adds the CONTEXT slots:
//   P5a  gctx[j] = sum of the context-slot gradients whose slot selected column j (fixed slot order)
//   P5b  per column j with gctx[j] != 0 (wavefront-owned, lanes over E): dctx_j recomputed, the cosine Jacobian of
//        (qctx, dctx_j) -> d(loss)/d(dctx_j) / 6 into the workspace, d(loss)/d(qctx-hat) accumulated per wavefront
//   P5c  grad_q rows += d(loss)/d(qctx) / Q; grad_d row t += the workspace rows j = t - 5 .. t in ascending order
__global__ void __launch_bounds__(256) co_pacrr_bwd_kernel(CoBwdArgs a) {
  extern __shared__ float lds[];
  const int Q = a.Q, D = a.D, E = a.E, N = a.N, k = 4 * a.k, NK = N * k;
  const BwdLds L(Q, D, a.C, N, k);
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int64_t pair = blockIdx.x;
  const float* q = a.q + (pair / a.ppq) * (int64_t)Q * E;
  const float* d = a.d + pair * (int64_t)D * E;
  const float* go = a.go + pair * (int64_t)Q * N * 2 * k;
  float* rd = lds + L.rd;
  float* eg = lds + L.eg;
  const int* ei = (const int*)(lds + L.ei);
  float* gq = a.gq + pair * (int64_t)Q * E;
  float* gd = a.gd + pair * (int64_t)D * E;
  const int ME = (E + 63) / 64;

  bwd_value_slots(a, k, lds, [&](int i) { return go[(i / k) * 2 * k + i % k]; });

  // ---- P5a: eg <- the context-slot gradients (eg / rd are free after P3)
  __syncthreads();
  float* gctx = rd;
  for (int i = tid; i < Q * NK; i += 256) eg[i] = go[(i / k) * 2 * k + k + i % k];
  __syncthreads();
  for (int j = tid; j < D; j += 256) {
    float g = 0.0f;
    for (int e = 0; e < Q * NK; ++e) {
      if ((ei[e] & 0xffff) == j) g += eg[e];
    }
    gctx[j] = g;
  }
  __syncthreads();

  // ---- P5b
  float* W = a.gdctx + pair * (int64_t)D * E;
  float qc[kMaxEPerLane], acc[kMaxEPerLane];
  float qq = 0.0f;
#pragma unroll
  for (int m = 0; m < kMaxEPerLane; ++m) {
    const int e = lane + 64 * m;
    float s = 0.0f;
    if (m < ME && e < E) {
      for (int i = 0; i < Q; ++i) s += q[(int64_t)i * E + e];
    }
    qc[m] = s / (float)Q;
    qq += qc[m] * qc[m];
    acc[m] = 0.0f;
  }
  const float nqc = sqrtf(wave_sum(qq)), rqc = 1.0f / (nqc + kTiny);
  for (int j = w; j < D; j += 4) {
    const float g = gctx[j];
    if (g == 0.0f) continue;
    const int t1 = min(j + 6, D);
    float x[kMaxEPerLane];
    float p2 = 0.0f, dq = 0.0f;
#pragma unroll
    for (int m = 0; m < kMaxEPerLane; ++m) {
      const int e = lane + 64 * m;
      float s = 0.0f;
      if (m < ME && e < E) {
        for (int t = j; t < t1; ++t) s += d[(int64_t)t * E + e];
      }
      x[m] = s / 6.0f;
      p2 += x[m] * x[m];
      dq += x[m] * (qc[m] * rqc);
    }
    p2 = wave_sum(p2);
    dq = wave_sum(dq);
    const float nx = sqrtf(p2), rx = 1.0f / (nx + kTiny);
    const float f = nx > 0.0f ? g * dq * rx * rx / nx : 0.0f;
#pragma unroll
    for (int m = 0; m < kMaxEPerLane; ++m) {
      const int e = lane + 64 * m;
      if (m < ME && e < E) W[(int64_t)j * E + e] = (g * (qc[m] * rqc) * rx - x[m] * f) / 6.0f;
      acc[m] += g * rx * x[m];
    }
  }
  float* P = a.gqh + pair * 4 * (int64_t)E;
#pragma unroll
  for (int m = 0; m < kMaxEPerLane; ++m) {
    const int e = lane + 64 * m;
    if (m < ME && e < E) P[w * E + e] = acc[m];
  }
  __syncthreads();

  // ---- P5c
  float dot = 0.0f;
#pragma unroll
  for (int m = 0; m < kMaxEPerLane; ++m) {
    const int e = lane + 64 * m;
    acc[m] = (m < ME && e < E) ? ((P[e] + P[E + e]) + P[2 * E + e]) + P[3 * E + e] : 0.0f;
    dot += acc[m] * qc[m];
  }
  dot = wave_sum(dot);
  const float fq = nqc > 0.0f ? dot * rqc * rqc / nqc : 0.0f;
#pragma unroll
  for (int m = 0; m < kMaxEPerLane; ++m) acc[m] = (acc[m] * rqc - qc[m] * fq) / (float)Q;   // d/dq_i of mean_i q_i
  for (int i = w; i < Q; i += 4) {
#pragma unroll
    for (int m = 0; m < kMaxEPerLane; ++m) {
      const int e = lane + 64 * m;
      if (m < ME && e < E) gq[(int64_t)i * E + e] += acc[m];
    }
  }
  for (int t = w; t < D; t += 4) {
    const int j0 = max(t - 5, 0);
    bool any = false;
    for (int j = j0; j <= t; ++j) any |= gctx[j] != 0.0f;
    if (!any) continue;
#pragma unroll
    for (int m = 0; m < kMaxEPerLane; ++m) {
      const int e = lane + 64 * m;
      if (m < ME && e < E) {
        float s = gd[(int64_t)t * E + e];
        for (int j = j0; j <= t; ++j) {
          if (gctx[j] != 0.0f) s += W[(int64_t)j * E + e];
        }
        gd[(int64_t)t * E + e] = s;
      }
    }
  }
}

// The family's checks with the views' own in their places: ascending before the shape, view 0 against k after it.
int check_call(int64_t n_pairs, int64_t ppq, int Q, int D, int E, int C, int N, int k, const int* v, const char* what) {
  int rc = check_pairs(n_pairs, ppq, what);
  if (rc == MM_OK && (v[0] > v[1] || v[1] > v[2] || v[2] > v[3]))
    rc = set_error(MM_EINVAL, "%s: views %d / %d / %d / %d are not ascending", what, v[0], v[1], v[2], v[3]);
  if (rc == MM_OK) rc = check_shape(Q, D, E, C, N, k, kCoKmax, what);
  if (rc == MM_OK && v[0] < k)   // torch.topk of a view narrower than k raises in the reference (co_pacrr.py:115, :140)
    rc = set_error(MM_EUNSUPPORTED, "%s: view 0 holds %d < k = %d columns", what, v[0], k);
  return rc;
}

}  // namespace
}  // namespace mm

using namespace mm;

extern "C" size_t mm_co_pacrr_workspace_bytes(int64_t n_pairs, int Q, int D, int E, int C, int N, int k) {
  (void)C;
  if (n_pairs <= 0 || Q <= 0 || D <= 0 || E <= 0 || k <= 0 || N <= 0) return 0;
  const size_t win = N >= 2 ? (size_t)Q * 4 * (size_t)k * (size_t)tap_off(N + 1) : 0;
  return (size_t)n_pairs * (win + (size_t)D * E + 4 * (size_t)E) * sizeof(float);
}

extern "C" int mm_co_pacrr_fwd(const float* q, const float* d, const float* conv_w, const float* conv_b, float* out,
                               int32_t* saved_idx, int64_t n_pairs, int64_t pairs_per_query, int Q, int D, int E, int C,
                               int N, int k, int view0, int view1, int view2, int view3, void* workspace,
                               size_t workspace_bytes, void* stream) {
  (void)workspace;
  (void)workspace_bytes;
  const char* what = "mm_co_pacrr_fwd";
  if (!q || !d || !out || (N >= 2 && (!conv_w || !conv_b)))
    return set_error(MM_EINVAL, "mm_co_pacrr_fwd: null q / d / out, or null conv_w / conv_b with N >= 2");
  const int v[4] = {view0, view1, view2, view3};
  const int rc = check_call(n_pairs, pairs_per_query, Q, D, E, C, N, k, v, what);
  if (rc != MM_OK || n_pairs == 0) return rc;
  CoArgs a{q, d, conv_w, conv_b, out, saved_idx, n_pairs, pairs_per_query, Q, D, E, C, N, k, view0, view1, view2, view3};
  return launch_per_pair(co_pacrr_fwd_kernel, a, CoFwdLds(Q, D, C, N, k).total, stream, what);
}

extern "C" int mm_co_pacrr_bwd(const float* q, const float* d, const float* conv_w, const int32_t* saved_idx,
                               const float* grad_out, float* grad_q, float* grad_d, float* grad_w, float* grad_b,
                               int64_t n_pairs, int64_t pairs_per_query, int Q, int D, int E, int C, int N, int k,
                               int view0, int view1, int view2, int view3, void* workspace, size_t workspace_bytes,
                               void* stream) {
  const char* what = "mm_co_pacrr_bwd";
  if (!q || !d || !saved_idx || !grad_out || !grad_q || !grad_d || (N >= 2 && (!conv_w || !grad_w || !grad_b)))
    return set_error(MM_EINVAL, "mm_co_pacrr_bwd: null pointer argument");
  const int v[4] = {view0, view1, view2, view3};
  int rc = check_call(n_pairs, pairs_per_query, Q, D, E, C, N, k, v, what);
  if (rc != MM_OK || n_pairs == 0) return rc;
  if ((rc = check_grid(n_pairs, what)) != MM_OK) return rc;   // reported before a workspace that is too small
  const size_t need = mm_co_pacrr_workspace_bytes(n_pairs, Q, D, E, C, N, k);
  if (!workspace || workspace_bytes < need)
    return set_error(MM_EWORKSPACE, "mm_co_pacrr_bwd: workspace of %zu bytes, needs %zu", workspace_bytes, need);
  float* ws = (float*)workspace;
  const size_t win = N >= 2 ? (size_t)n_pairs * Q * 4 * (size_t)k * (size_t)tap_off(N + 1) : 0;
  CoBwdArgs a{{q, d, conv_w, saved_idx, grad_out, grad_q, grad_d, grad_w, grad_b, ws, n_pairs, pairs_per_query, Q, D, E, C, N, k},
              ws + win, ws + win + (size_t)n_pairs * D * E};
  return launch_per_pair(co_pacrr_bwd_kernel, a, BwdLds(Q, D, C, N, 4 * k).total, stream, what);
}
