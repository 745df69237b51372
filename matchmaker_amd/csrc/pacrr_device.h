// Shared by the PACRR family (pacrr.hip, co_pacrr.hip; matchpyramid.hip takes the cosine phases): limits, the packed
// conv-weight layout, the LDS layouts, the fp32 MFMA, and ONE copy of every phase the family has in common —
//   query_rnorms / cosine_block_partials / cosine_block_finish   the cosine match matrix, 32 document columns at a time
//   conv_channel_max                                             one n-gram convolution + channel max for one query row
//   topk_insert                                                  the whole-wave sorted top-k insertion
//   bwd_value_slots                                              the backward through the selected VALUE slots (P0-P4)
// and the host side the entry points repeat (check_pairs, check_shape, launch_per_pair).  These are the numerically delicate
// parts (fixed summation orders, tie rules): the models' bit-equality tests hold because there is one copy.
#pragma once
#include "mm_internal.h"

namespace mm {
namespace pacrr_dev {

constexpr int kPQmax = 64, kPDmax = 2048, kPEmax = 1024, kPCmax = 64, kPNmax = 5, kPKmax = 32;
constexpr int kPB = 3;           // chunks of 8 elements whose loads a wavefront issues together (cosine phase)
constexpr int kRing = 65;         // ring row stride in floats (64 columns + 1: rows land on distinct banks)
constexpr int kMaxEPerLane = kPEmax / 64;   // backward: elements of a row held by one lane

// sum of m^2 for m = 2 .. n - 1: offset of width n's taps in the packed weights (per channel), in units of C floats
__host__ __device__ __forceinline__ int tap_off(int n) { return (n - 1) * n * (2 * n - 1) / 6 - 1; }

__device__ __forceinline__ f32x16 mfma32(float a, float b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}

// ------------------------------------------------------------------------------------------------------------------ cosine
// 1 / (|x_i| + tiny) of the rows of x [R, E] -> rn (and |x_i| -> nrm, for the backward's Jacobians): one wavefront per row.
__device__ __forceinline__ void query_rnorms(const float* x, int R, int E, float* rn, int w, int lane,
                                             float* nrm = nullptr) {
  for (int i = w; i < R; i += 4) {
    float s = 0.0f;
    for (int e = lane; e < E; e += 64) s += x[(int64_t)i * E + e] * x[(int64_t)i * E + e];
    s = wave_sum(s);
    if (lane == 0) {
      if (nrm) nrm[i] = sqrtf(s);
      rn[i] = 1.0f / (sqrtf(s) + kTiny);
    }
  }
}

// <q_i, d_j> for the 32 document columns at j0 on the fp32 32x32x2 MFMA (exact fp32: a k-ordered fma chain).  The four
// wavefronts split E; wavefront w leaves its partial tile(s) in part[(w nrt + rt) 32 x 33] and its halves' sums of d_j^2 in
// dn[(2 w + h) 32 + j].  The caller's barrier comes between this and cosine_block_finish.
// NRT = row tiles of 32 query rows, a compile-time count: the accumulators are indexed by constants only and stay two
// 16-register tiles (indexed by a run-time nrt they reach the register allocator as one 32-float value, which costs copies
// and, in a kernel without a launch bound to hold it back, occupancy).
template <int NRT>
__device__ __forceinline__ void cosine_block_partials_nrt(const float* q, const float* d, int Q, int D, int E, int j0,
                                                          float* part, float* dn, int w, int lane) {
  const int r32 = lane & 31, h = lane >> 5, nch = (E + 7) / 8;
  f32x16 acc[NRT];
#pragma unroll
  for (int rt = 0; rt < NRT; ++rt) acc[rt] = f32x16{};
  float dsq = 0.0f;
  const bool drow = j0 + r32 < D;
  const float* dp = d + (int64_t)(j0 + r32) * E;
  // kPB chunks of 8 per batch: every load of a batch is issued before its first MFMA (one memory latency per batch,
  // not per chunk: the rows are 4 x 16 B per lane, far apart, and nothing else hides their latency)
  for (int m0 = w; m0 < nch; m0 += 4 * kPB) {
    f32x4 dv[kPB], qv[NRT][kPB];
#pragma unroll
    for (int u = 0; u < kPB; ++u) {
      const int k0 = 8 * (m0 + 4 * u) + 4 * h;
      const bool kin = m0 + 4 * u < nch && k0 < E;
      dv[u] = load4_or0(dp + k0, drow && kin);
#pragma unroll
      for (int rt = 0; rt < NRT; ++rt) {
        const int qi = rt * 32 + r32;
        qv[rt][u] = load4_or0(q + (int64_t)qi * E + k0, qi < Q && kin);
      }
    }
#pragma unroll
    for (int u = 0; u < kPB; ++u) {
      dsq += dv[u][0] * dv[u][0] + dv[u][1] * dv[u][1] + dv[u][2] * dv[u][2] + dv[u][3] * dv[u][3];
#pragma unroll
      for (int rt = 0; rt < NRT; ++rt) {
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[rt] = mfma32(qv[rt][u][e], dv[u][e], acc[rt]);
      }
    }
  }
#pragma unroll
  for (int rt = 0; rt < NRT; ++rt) {
    float* pp = part + (w * NRT + rt) * 32 * 33;
#pragma unroll
    for (int g = 0; g < 16; ++g) pp[((g & 3) + 8 * (g >> 2) + 4 * h) * 33 + r32] = acc[rt][g];
  }
  dn[(w * 2 + h) * 32 + r32] = dsq;
}

__device__ __forceinline__ void cosine_block_partials(const float* q, const float* d, int Q, int D, int E, int j0,
                                                      float* part, float* dn, int w, int lane) {
  if (Q > 32) cosine_block_partials_nrt<2>(q, d, Q, D, E, j0, part, dn, w, lane);
  else cosine_block_partials_nrt<1>(q, d, Q, D, E, j0, part, dn, w, lane);
}

// The block's document norms -> rd (fixed order over the eight halves), ONE barrier, then store(i, j, cosine) for every query
// row i and block column j: the four partial tiles summed in wavefront order, (v * rq[i]) * rd[j].
template <class Store>
__device__ __forceinline__ void cosine_block_finish(int Q, const float* part, const float* dn, const float* rq, float* rd,
                                                    int tid, Store store) {
  const int nrt = (Q + 31) / 32;
  if (tid < 32) {
    float t = 0.0f;
    for (int u = 0; u < 8; ++u) t += dn[u * 32 + tid];
    rd[tid] = 1.0f / (sqrtf(t) + kTiny);
  }
  __syncthreads();
  for (int c = tid; c < Q * 32; c += 256) {
    const int i = c >> 5, j = c & 31, rt = i >> 5, ii = i & 31;
    float v = part[(0 * nrt + rt) * 32 * 33 + ii * 33 + j];
    v += part[(1 * nrt + rt) * 32 * 33 + ii * 33 + j];
    v += part[(2 * nrt + rt) * 32 * 33 + ii * 33 + j];
    v += part[(3 * nrt + rt) * 32 * 33 + ii * 33 + j];
    store(i, j, (v * rq[i]) * rd[j]);
  }
}

// --------------------------------------------------------------------------------------------------------- conv + top-k
// LDS layout of the forward (floats)
struct FwdLds {
  int rq, rd, dn, wt, bs, ring, part, tv, ti, total;
  __host__ __device__ FwdLds(int Q, int C, int N, int k) {
    const int nrt = (Q + 31) / 32;
    int o = 0;
    rq = o; o += kPQmax;
    rd = o; o += 32;
    dn = o; o += 4 * 2 * 32;
    wt = o; o += C * tap_off(N + 1);
    bs = o; o += C * (N - 1);
    ring = o; o += (Q + kPNmax) * kRing;
    part = o; o += 4 * nrt * 32 * 33;     // >= 4224 >= kPEmax
    tv = o; o += Q * N * k;
    ti = o; o += Q * N * k;
    total = o;
  }
};

struct ConvMax {
  float v;
  int ch;
};

// Width-n convolution of query row r at the 32 ring columns from cb (lane & 31 = column), every channel: an im2col product
// [C x n^2] x [n^2 x 32] on the fp32 MFMA, the accumulator initialised with the bias, then the channel max on the accumulators
// (lowest channel on ties, MaxPool3d's rule).  Both lane halves return the column's maximum and its channel.
__device__ __forceinline__ ConvMax conv_channel_max(const float* wt, const float* bs, const float* ring, int r, int cb, int n,
                                                    int C, int lane) {
  const int r32 = lane & 31, h = lane >> 5, nn = n * n;
  const float* wp = wt + C * tap_off(n);
  const float* bp = bs + C * (n - 2);
  float best = neg_inf();
  int bch = 0;
  for (int ct = 0; ct * 32 < C; ++ct) {
    f32x16 acc;
#pragma unroll
    for (int g = 0; g < 16; ++g) {
      const int ch = ct * 32 + (g & 3) + 8 * (g >> 2) + 4 * h;
      acc[g] = ch < C ? bp[ch] : neg_inf();
    }
    const int cha = ct * 32 + r32;
    for (int st = 0; st < (nn + 1) / 2; ++st) {
      const int t = 2 * st + h;
      const bool tin = t < nn;
      const int ta = tin ? t / n : 0, tb = tin ? t - ta * n : 0;
      const float av = (tin && cha < C) ? wp[cha * nn + t] : 0.0f;
      const float bv = tin ? ring[(r + ta) * kRing + ((cb + r32 + tb) & 63)] : 0.0f;
      acc = mfma32(av, bv, acc);
    }
#pragma unroll
    for (int g = 0; g < 16; ++g) {
      const int ch = ct * 32 + (g & 3) + 8 * (g >> 2) + 4 * h;
      if (acc[g] > best) {
        best = acc[g];
        bch = ch;
      }
    }
  }
  // the other lane half holds channels + 4 of the same column
  const float ob = __shfl_xor(best, 32, 64);
  const int oc = __shfl_xor(bch, 32, 64);
  if (ob > best || (ob == best && oc < bch)) {
    best = ob;
    bch = oc;
  }
  return {best, bch};
}

// Whole-wave insertion of up to 32 new values (lanes 0..31: v / id of column c0 + lane, `ok` = the column exists) into the
// sorted list held by lanes 0..k-1 (lv / li, cnt entries).  A value enters when the list is not full or when it is STRICTLY
// greater than the k-th: with the columns visited in ascending order, equal values keep the lower column first.
__device__ __forceinline__ void topk_insert(float& lv, int& li, int& cnt, float v, int id, bool ok, int k, int lane) {
  float thr = __shfl(lv, k - 1, 64);
  unsigned long long cand = __ballot(lane < 32 && ok && v == v && (cnt < k || v > thr));
  while (cand) {
    const int c = __builtin_ctzll(cand);
    cand &= cand - 1;
    const float vc = __shfl(v, c, 64);
    const int ic = __shfl(id, c, 64);
    if (cnt == k && !(vc > thr)) continue;
    const int pos = __popcll(__ballot(lane < cnt && lv >= vc));
    const float pv = __shfl(lv, lane > 0 ? lane - 1 : 0, 64);
    const int pi = __shfl(li, lane > 0 ? lane - 1 : 0, 64);
    if (lane == pos) {
      lv = vc;
      li = ic;
    } else if (lane > pos && lane <= cnt && lane < k) {
      lv = pv;
      li = pi;
    }
    cnt = cnt < k ? cnt + 1 : k;
    thr = __shfl(lv, k - 1, 64);
  }
}

// ---------------------------------------------------------------------------------------------------------------- backward
struct BwdArgs {
  const float* q;
  const float* d;
  const float* w;
  const int32_t* idx;   // [n_pairs, Q, N, K]: column | channel << 16 of every value slot
  const float* go;      // the model's grad_out (PACRR [n_pairs, Q, N, K]; CO-PACRR [n_pairs, Q, N, 2K])
  float* gq;            // [n_pairs, Q, E]
  float* gd;            // [n_pairs, D, E]
  float* gw;            // [n_pairs, C S]
  float* gb;            // [n_pairs, (N - 1) C]
  float* wincos;        // workspace [n_pairs, Q K S]
  int64_t n_pairs, ppq;
  int Q, D, E, C, N, k;
};

// LDS layout of the backward (floats), K list slots per (row, path)
struct BwdLds {
  int rq, nq, rd, nd, wt, eg, ei, G, gwl, gbl, total;
  __host__ __device__ BwdLds(int Q, int D, int C, int N, int K) {
    const int S = tap_off(N + 1);
    int o = 0;
    rq = o; o += kPQmax;
    nq = o; o += kPQmax;
    rd = o; o += D;
    nd = o; o += D;
    wt = o; o += C * S;
    eg = o; o += Q * N * K;
    ei = o; o += Q * N * K;
    G = o; o += Q * 33;
    gwl = o; o += C * S;
    gbl = o; o += C * (N - 1);
    total = o;
  }
};

// The backward through the K value slots of every (row, path) of the workgroup's pair; go_at(i) is the gradient of slot
// i = (row N + path) K + slot.  A column held by several slots gets every slot's term.
//   P0  norms of the query rows and of every document row, the weights, the pair's saved entries and their gradients -> LDS
//   P1  the cosine at every tap of every selected conv window (one dot each, recomputed from q / d) -> workspace
//   P2  grad_w / grad_b of the pair: thread (path, tap) owns column `tap` of that width's weight gradient, thread `path` its
//       bias gradient; each walks the entries in a fixed order (no atomics)
//   P3  per 32-column document block: the sparse dcos block gathered into LDS (each cell sums its contributions in a fixed
//       order), grad_d of the block's rows through the normalisation Jacobian, grad_q-hat accumulated in grad_q
//   P4  grad_q through the query's normalisation Jacobian
// The rows of P3 / P4 are wavefront-owned with one lane per 64th element: the thread that accumulates a grad_q element is the
// one that finishes it.  Ends without a barrier: LDS (rq, nq, rd, nd, ei) is intact, eg and G are free after one.
template <class GradOutAt>
__device__ __forceinline__ void bwd_value_slots(const BwdArgs& a, int K, float* lds, GradOutAt go_at) {
  const int Q = a.Q, D = a.D, E = a.E, C = a.C, N = a.N;
  const int S = tap_off(N + 1), NK = N * K;
  const BwdLds L(Q, D, C, N, K);
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int64_t pair = blockIdx.x;
  const float* q = a.q + (pair / a.ppq) * (int64_t)Q * E;
  const float* d = a.d + pair * (int64_t)D * E;
  float* rq = lds + L.rq;
  float* nqv = lds + L.nq;
  float* rd = lds + L.rd;
  float* ndv = lds + L.nd;
  float* wt = lds + L.wt;
  float* eg = lds + L.eg;
  int* ei = (int*)(lds + L.ei);
  float* G = lds + L.G;
  float* gwl = lds + L.gwl;
  float* gbl = lds + L.gbl;
  float* wc = a.wincos + pair * (int64_t)Q * K * S;
  const int ME = (E + 63) / 64;

  // ---- P0
  for (int i = tid; i < C * S; i += 256) {
    wt[i] = a.w[i];
    gwl[i] = 0.0f;
  }
  for (int i = tid; i < C * (N - 1); i += 256) gbl[i] = 0.0f;
  for (int i = tid; i < Q * NK; i += 256) {
    eg[i] = go_at(i);
    ei[i] = a.idx[pair * (int64_t)Q * NK + i];
  }
  query_rnorms(q, Q, E, rq, w, lane, nqv);
  query_rnorms(d, D, E, rd, w, lane, ndv);   // the same loop over the document rows
  __syncthreads();

  // ---- P1: wincos[r][K soff(n) + i n^2 + t] for every conv entry (r, width n, slot i) and tap t
  const int per_row = K * S;
  for (int it = w; it < Q * per_row; it += 4) {
    const int r = it / per_row;
    int rem = it - r * per_row;
    int n = 2;
    while (n < N && rem >= K * tap_off(n + 1)) ++n;
    rem -= K * tap_off(n);
    const int nn = n * n, i = rem / nn, t = rem - i * nn;
    const int id = ei[r * NK + (n - 1) * K + i];
    const int col = id & 0xffff, ra = r + t / n, cb = col + t % n;
    float v = 0.0f;
    if (ra < Q && cb < D) {          // past the matrix: ConstantPad2d's zeros
      float s = 0.0f;
      for (int e = lane; e < E; e += 64) s += q[(int64_t)ra * E + e] * d[(int64_t)cb * E + e];
      v = (wave_sum(s) * rq[ra]) * rd[cb];
    }
    if (lane == 0) wc[it] = v;
  }
  __syncthreads();

  // ---- P2
  if (tid < S) {
    int n = 2;
    while (n < N && tid >= tap_off(n + 1)) ++n;
    const int nn = n * n, t = tid - tap_off(n);
    float* gwn = gwl + C * tap_off(n);
    for (int r = 0; r < Q; ++r) {
      for (int i = 0; i < K; ++i) {
        const int e = r * NK + (n - 1) * K + i;
        const int ch = min(ei[e] >> 16, C - 1);     // (a foreign index array must not write outside the LDS rows)
        gwn[ch * nn + t] += eg[e] * wc[r * per_row + K * tap_off(n) + i * nn + t];
      }
    }
  } else if (tid >= 64 && tid < 64 + N - 1) {
    const int p = tid - 64 + 1;
    for (int r = 0; r < Q; ++r) {
      for (int i = 0; i < K; ++i) {
        const int e = r * NK + p * K + i;
        gbl[(p - 1) * C + min(ei[e] >> 16, C - 1)] += eg[e];
      }
    }
  }
  __syncthreads();
  for (int i = tid; i < C * S; i += 256) a.gw[pair * (int64_t)C * S + i] = gwl[i];
  for (int i = tid; i < C * (N - 1); i += 256) a.gb[pair * (int64_t)C * (N - 1) + i] = gbl[i];

  // ---- P3
  float* gq = a.gq + pair * (int64_t)Q * E;
  float* gd = a.gd + pair * (int64_t)D * E;
  for (int c0 = 0; c0 < D; c0 += 32) {
    for (int c = tid; c < Q * 32; c += 256) {
      const int i = c >> 5, col = c0 + (c & 31);
      float g = 0.0f;
      if (col < D) {
        for (int s = 0; s < K; ++s) {
          if (ei[i * NK + s] == col) g += eg[i * NK + s];
        }
        for (int n = 2; n <= N; ++n) {
          const int nn = n * n;
          const float* wn = wt + C * tap_off(n);
          for (int ra = 0; ra < n && ra <= i; ++ra) {
            const int r = i - ra;
            for (int s = 0; s < K; ++s) {
              const int e = r * NK + (n - 1) * K + s;
              const int id = ei[e];
              const int b = col - (id & 0xffff);
              if (b >= 0 && b < n) g += eg[e] * wn[min(id >> 16, C - 1) * nn + ra * n + b];
            }
          }
        }
      }
      G[i * 33 + (c & 31)] = g;
    }
    __syncthreads();
    // grad_d of the block's rows: ghat = sum_i G[i][j] qhat_i, then d/dx of x / (|x| + tiny)
    for (int jj = w; jj < 32 && c0 + jj < D; jj += 4) {
      const int col = c0 + jj;
      float acc[kMaxEPerLane];
#pragma unroll
      for (int m = 0; m < kMaxEPerLane; ++m) acc[m] = 0.0f;
      for (int i = 0; i < Q; ++i) {
        const float g = G[i * 33 + jj];
        if (g == 0.0f) continue;
        const float gs = g * rq[i];
#pragma unroll
        for (int m = 0; m < kMaxEPerLane; ++m) {
          const int e = lane + 64 * m;
          if (m < ME && e < E) acc[m] += gs * q[(int64_t)i * E + e];
        }
      }
      float dot = 0.0f;
#pragma unroll
      for (int m = 0; m < kMaxEPerLane; ++m) {
        const int e = lane + 64 * m;
        if (m < ME && e < E) dot += acc[m] * d[(int64_t)col * E + e];
      }
      dot = wave_sum(dot);
      const float nrm = ndv[col], r1 = rd[col];
      const float f = nrm > 0.0f ? dot * r1 * r1 / nrm : 0.0f;
#pragma unroll
      for (int m = 0; m < kMaxEPerLane; ++m) {
        const int e = lane + 64 * m;
        if (m < ME && e < E) gd[(int64_t)col * E + e] = acc[m] * r1 - d[(int64_t)col * E + e] * f;
      }
    }
    // grad_q-hat += sum_j G[i][j] dhat_j
    for (int i = w; i < Q; i += 4) {
      float acc[kMaxEPerLane];
#pragma unroll
      for (int m = 0; m < kMaxEPerLane; ++m) {
        const int e = lane + 64 * m;
        acc[m] = (c0 > 0 && m < ME && e < E) ? gq[(int64_t)i * E + e] : 0.0f;
      }
      for (int jj = 0; jj < 32 && c0 + jj < D; ++jj) {
        const float g = G[i * 33 + jj];
        if (g == 0.0f) continue;
        const float gs = g * rd[c0 + jj];
#pragma unroll
        for (int m = 0; m < kMaxEPerLane; ++m) {
          const int e = lane + 64 * m;
          if (m < ME && e < E) acc[m] += gs * d[(int64_t)(c0 + jj) * E + e];
        }
      }
#pragma unroll
      for (int m = 0; m < kMaxEPerLane; ++m) {
        const int e = lane + 64 * m;
        if (m < ME && e < E) gq[(int64_t)i * E + e] = acc[m];
      }
    }
    __syncthreads();
  }
  // rows of the document past the last block do not exist (D is covered); grad_d rows with no entry were written as zeros

  // ---- P4
  for (int i = w; i < Q; i += 4) {
    float acc[kMaxEPerLane];
    float dot = 0.0f;
#pragma unroll
    for (int m = 0; m < kMaxEPerLane; ++m) {
      const int e = lane + 64 * m;
      acc[m] = (m < ME && e < E) ? gq[(int64_t)i * E + e] : 0.0f;
      if (m < ME && e < E) dot += acc[m] * q[(int64_t)i * E + e];
    }
    dot = wave_sum(dot);
    const float nrm = nqv[i], r1 = rq[i];
    const float f = nrm > 0.0f ? dot * r1 * r1 / nrm : 0.0f;
#pragma unroll
    for (int m = 0; m < kMaxEPerLane; ++m) {
      const int e = lane + 64 * m;
      if (m < ME && e < E) gq[(int64_t)i * E + e] = acc[m] * r1 - q[(int64_t)i * E + e] * f;
    }
  }
}

// --------------------------------------------------------------------------------------------------------------- host side
inline int check_pairs(int64_t n_pairs, int64_t ppq, const char* what) {
  if (n_pairs < 0 || ppq < 1) return set_error(MM_EINVAL, "%s: n_pairs = %lld, pairs_per_query = %lld", what, (long long)n_pairs, (long long)ppq);
  return MM_OK;
}

inline int check_shape(int Q, int D, int E, int C, int N, int k, int kmax, const char* what) {
  if (Q < 1 || Q > kPQmax || k < 1 || k > kmax || D < k || D > kPDmax || E < 4 || E > kPEmax || E % 4 || C < 1 ||
      C > kPCmax || N < 1 || N > kPNmax)
    return set_error(MM_EUNSUPPORTED,
                     "%s: Q = %d, D = %d, E = %d, C = %d, N = %d, k = %d outside 1 <= Q <= 64, k <= D <= 2048, 4 <= E <= 1024 "
                     "(a multiple of 4), 1 <= C <= 64, 1 <= N <= 5, 1 <= k <= %d",
                     what, Q, D, E, C, N, k, kmax);
  return MM_OK;
}

inline int check_grid(int64_t n_pairs, const char* what) {
  if (n_pairs > 0x7fffffff) return set_error(MM_EUNSUPPORTED, "%s: %lld pairs in one call", what, (long long)n_pairs);
  return MM_OK;
}

// One workgroup of 256 threads per pair with lds_floats of dynamic LDS (the grid holds n_pairs as an unsigned int).
template <class Args>
int launch_per_pair(void (*kernel)(Args), const Args& a, int lds_floats, void* stream, const char* what) {
  const int rc = check_grid(a.n_pairs, what);
  if (rc != MM_OK) return rc;
  (void)hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds_floats * (int)sizeof(float));
  hipLaunchKernelGGL(kernel, dim3((unsigned)a.n_pairs), dim3(256), (size_t)lds_floats * sizeof(float), (hipStream_t)stream, a);
  return check_launch(what);
}

}  // namespace pacrr_dev
}  // namespace mm
