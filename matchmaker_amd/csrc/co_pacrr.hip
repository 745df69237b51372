// CO-PACRR (matchmaker/models/co_pacrr.py:79-158): PACRR's cosine match matrix -> n-gram convolutions + channel max ->
// per-row k-max pipeline, with four nested document views and a context similarity gathered at every selected column.
// Forward: ONE launch per call, one workgroup (four wavefronts) per pair, PACRR's structure (csrc/pacrr.hip): the match
// matrix lives in an LDS ring of 64 document columns.  Backward: ONE launch, one workgroup per pair.
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

// LDS layout of the forward (floats); the query context aliases `part` (free until the first cosine block)
struct CoFwdLds {
  int rq, rd, dn, wt, bs, ring, part, tv, ti, ctx, total;
  __host__ __device__ CoFwdLds(int Q, int D, int C, int N, int k) {
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
    ctx = o; o += D;
    total = o;
  }
};

__global__ void __launch_bounds__(256, 4) co_pacrr_fwd_kernel(CoArgs a) {
  extern __shared__ float lds[];
  const int Q = a.Q, D = a.D, E = a.E, C = a.C, N = a.N, k = a.k;
  const CoFwdLds L(Q, D, C, N, k);
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r32 = lane & 31, h = lane >> 5;
  const int64_t pair = blockIdx.x;
  const float* q = a.q + (pair / a.ppq) * (int64_t)Q * E;
  const float* d = a.d + pair * (int64_t)D * E;
  const int nrt = (Q + 31) / 32, nch = (E + 7) / 8, nb = (D + 31) / 32, S = tap_off(N + 1);
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
  for (int i = w; i < Q; i += 4) {
    float s = 0.0f;
    for (int e = lane; e < E; e += 64) s += q[(int64_t)i * E + e] * q[(int64_t)i * E + e];
    s = wave_sum(s);
    if (lane == 0) rq[i] = 1.0f / (sqrtf(s) + kTiny);
  }
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
    if (s < nb) {
      f32x16 acc[2];
      acc[0] = f32x16{};
      acc[1] = f32x16{};
      float dsq = 0.0f;
      const bool drow = j0 + r32 < D;
      const float* dp = d + (int64_t)(j0 + r32) * E;
      for (int m0 = w; m0 < nch; m0 += 4 * kPB) {
        f32x4 dv[kPB], qv[2][kPB];
#pragma unroll
        for (int u = 0; u < kPB; ++u) {
          const int k0 = 8 * (m0 + 4 * u) + 4 * h;
          const bool kin = m0 + 4 * u < nch && k0 < E;
          dv[u] = load4_or0(dp + k0, drow && kin);
#pragma unroll
          for (int rt = 0; rt < 2; ++rt) {
            const int qi = rt * 32 + r32;
            qv[rt][u] = load4_or0(q + (int64_t)qi * E + k0, rt < nrt && qi < Q && kin);
          }
        }
#pragma unroll
        for (int u = 0; u < kPB; ++u) {
          dsq += dv[u][0] * dv[u][0] + dv[u][1] * dv[u][1] + dv[u][2] * dv[u][2] + dv[u][3] * dv[u][3];
#pragma unroll
          for (int rt = 0; rt < 2; ++rt) {
            if (rt >= nrt) break;
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[rt] = mfma32(qv[rt][u][e], dv[u][e], acc[rt]);
          }
        }
      }
#pragma unroll
      for (int rt = 0; rt < 2; ++rt) {
        if (rt >= nrt) break;
        float* pp = part + (w * nrt + rt) * 32 * 33;
#pragma unroll
        for (int g = 0; g < 16; ++g) pp[((g & 3) + 8 * (g >> 2) + 4 * h) * 33 + r32] = acc[rt][g];
      }
      dn[(w * 2 + h) * 32 + r32] = dsq;
    }
    __syncthreads();
    if (s < nb) {
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
        ring[i * kRing + rb + j] = (v * rq[i]) * rd[j];
      }
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
      const int n = p + 1, nn = n * n;
      for (int r = w; r < Q; r += 4) {
        float v;
        int id;
        if (p == 0) {
          v = ring[r * kRing + ((cb + r32) & 63)];
          id = col;
        } else {
          const float* wp = wt + C * tap_off(n);
          const float* bp = bs + C * (p - 1);
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
          v = best;
          id = col | (bch << 16);
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
struct CoBwdArgs {
  const float* q;
  const float* d;
  const float* w;
  const int32_t* idx;   // [n_pairs, Q, N, 4k]
  const float* go;      // [n_pairs, Q, N, 8k]
  float* gq;            // [n_pairs, Q, E]
  float* gd;            // [n_pairs, D, E]
  float* gw;            // [n_pairs, C S]
  float* gb;            // [n_pairs, (N - 1) C]
  float* wincos;        // workspace [n_pairs, Q 4k S]
  float* gdctx;         // workspace [n_pairs, D, E]: d(loss)/d(dctx_j) / 6
  float* gqh;           // workspace [n_pairs, 4, E]: per-wavefront partials of d(loss)/d(qctx-hat)
  int64_t n_pairs, ppq;
  int Q, D, E, C, N, k;
};

// PACRR's backward layout with K = 4k list slots per (row, path)
struct CoBwdLds {
  int rq, nq, rd, nd, wt, eg, ei, G, gwl, gbl, total;
  __host__ __device__ CoBwdLds(int Q, int D, int C, int N, int K) {
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

constexpr int kMaxEPerLane = kPEmax / 64;

// One workgroup per pair.  P0-P4 are PACRR's backward (pacrr_bwd_kernel) over the 4k VALUE slots of every (row, path): a
// column chosen by several views appears in several slots and every slot adds its own term.  P5 adds the CONTEXT slots:
//   P5a  gctx[j] = sum of the context-slot gradients whose slot selected column j (fixed slot order)
//   P5b  per column j with gctx[j] != 0 (wavefront-owned, lanes over E): dctx_j recomputed, the cosine Jacobian of
//        (qctx, dctx_j) -> d(loss)/d(dctx_j) / 6 into the workspace, d(loss)/d(qctx-hat) accumulated per wavefront
//   P5c  grad_q rows += d(loss)/d(qctx) / Q; grad_d row t += the workspace rows j = t - 5 .. t in ascending order
__global__ void __launch_bounds__(256) co_pacrr_bwd_kernel(CoBwdArgs a) {
  extern __shared__ float lds[];
  const int Q = a.Q, D = a.D, E = a.E, C = a.C, N = a.N, k = 4 * a.k;
  const int S = tap_off(N + 1), NK = N * k;
  const CoBwdLds L(Q, D, C, N, k);
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int64_t pair = blockIdx.x;
  const float* q = a.q + (pair / a.ppq) * (int64_t)Q * E;
  const float* d = a.d + pair * (int64_t)D * E;
  const float* go = a.go + pair * (int64_t)Q * N * 2 * k;
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
  float* wc = a.wincos + pair * (int64_t)Q * k * S;
  const int ME = (E + 63) / 64;

  // ---- P0 (value-slot gradients: the first 4k of every path's 8k)
  for (int i = tid; i < C * S; i += 256) {
    wt[i] = a.w[i];
    gwl[i] = 0.0f;
  }
  for (int i = tid; i < C * (N - 1); i += 256) gbl[i] = 0.0f;
  for (int i = tid; i < Q * NK; i += 256) {
    eg[i] = go[(i / k) * 2 * k + i % k];
    ei[i] = a.idx[pair * (int64_t)Q * NK + i];
  }
  for (int i = w; i < Q; i += 4) {
    float s = 0.0f;
    for (int e = lane; e < E; e += 64) s += q[(int64_t)i * E + e] * q[(int64_t)i * E + e];
    s = wave_sum(s);
    if (lane == 0) {
      nqv[i] = sqrtf(s);
      rq[i] = 1.0f / (sqrtf(s) + kTiny);
    }
  }
  for (int j = w; j < D; j += 4) {
    float s = 0.0f;
    for (int e = lane; e < E; e += 64) s += d[(int64_t)j * E + e] * d[(int64_t)j * E + e];
    s = wave_sum(s);
    if (lane == 0) {
      ndv[j] = sqrtf(s);
      rd[j] = 1.0f / (sqrtf(s) + kTiny);
    }
  }
  __syncthreads();

  // ---- P1: wincos[r][k soff(n) + i n^2 + t] for every conv entry (r, width n, slot i) and tap t
  const int per_row = k * S;
  for (int it = w; it < Q * per_row; it += 4) {
    const int r = it / per_row;
    int rem = it - r * per_row;
    int n = 2;
    while (n < N && rem >= k * tap_off(n + 1)) ++n;
    rem -= k * tap_off(n);
    const int nn = n * n, i = rem / nn, t = rem - i * nn;
    const int id = ei[r * NK + (n - 1) * k + i];
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
      for (int i = 0; i < k; ++i) {
        const int e = r * NK + (n - 1) * k + i;
        const int ch = min(ei[e] >> 16, C - 1);     // (a foreign index array must not write outside the LDS rows)
        gwn[ch * nn + t] += eg[e] * wc[r * per_row + k * tap_off(n) + i * nn + t];
      }
    }
  } else if (tid >= 64 && tid < 64 + N - 1) {
    const int p = tid - 64 + 1;
    for (int r = 0; r < Q; ++r) {
      for (int i = 0; i < k; ++i) {
        const int e = r * NK + p * k + i;
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
        for (int s = 0; s < k; ++s) {
          if (ei[i * NK + s] == col) g += eg[i * NK + s];
        }
        for (int n = 2; n <= N; ++n) {
          const int nn = n * n;
          const float* wn = wt + C * tap_off(n);
          for (int ra = 0; ra < n && ra <= i; ++ra) {
            const int r = i - ra;
            for (int s = 0; s < k; ++s) {
              const int e = r * NK + (n - 1) * k + s;
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

int check_shape(int64_t n_pairs, int64_t ppq, int Q, int D, int E, int C, int N, int k, const int* v, const char* what) {
  if (n_pairs < 0 || ppq < 1) return set_error(MM_EINVAL, "%s: n_pairs = %lld, pairs_per_query = %lld", what, (long long)n_pairs, (long long)ppq);
  if (v[0] > v[1] || v[1] > v[2] || v[2] > v[3])
    return set_error(MM_EINVAL, "%s: views %d / %d / %d / %d are not ascending", what, v[0], v[1], v[2], v[3]);
  if (Q < 1 || Q > kPQmax || k < 1 || k > kCoKmax || D < k || D > kPDmax || E < 4 || E > kPEmax || E % 4 || C < 1 ||
      C > kPCmax || N < 1 || N > kPNmax)
    return set_error(MM_EUNSUPPORTED,
                     "%s: Q = %d, D = %d, E = %d, C = %d, N = %d, k = %d outside 1 <= Q <= 64, k <= D <= 2048, 4 <= E <= 1024 "
                     "(a multiple of 4), 1 <= C <= 64, 1 <= N <= 5, 1 <= k <= 8",
                     what, Q, D, E, C, N, k);
  if (v[0] < k)   // torch.topk of a view narrower than k raises in the reference (co_pacrr.py:115, :140)
    return set_error(MM_EUNSUPPORTED, "%s: view 0 holds %d < k = %d columns", what, v[0], k);
  return MM_OK;
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
  if (!q || !d || !out || (N >= 2 && (!conv_w || !conv_b)))
    return set_error(MM_EINVAL, "mm_co_pacrr_fwd: null q / d / out, or null conv_w / conv_b with N >= 2");
  const int v[4] = {view0, view1, view2, view3};
  int rc = check_shape(n_pairs, pairs_per_query, Q, D, E, C, N, k, v, "mm_co_pacrr_fwd");
  if (rc != MM_OK) return rc;
  if (n_pairs == 0) return MM_OK;
  if (n_pairs > 0x7fffffff) return set_error(MM_EUNSUPPORTED, "mm_co_pacrr_fwd: %lld pairs in one call", (long long)n_pairs);
  const CoFwdLds L(Q, D, C, N, k);
  CoArgs a{q, d, conv_w, conv_b, out, saved_idx, n_pairs, pairs_per_query, Q, D, E, C, N, k, view0, view1, view2, view3};
  (void)hipFuncSetAttribute((const void*)co_pacrr_fwd_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, L.total * (int)sizeof(float));
  hipLaunchKernelGGL(co_pacrr_fwd_kernel, dim3((unsigned)n_pairs), dim3(256), (size_t)L.total * sizeof(float),
                     (hipStream_t)stream, a);
  return check_launch("mm_co_pacrr_fwd");
}

extern "C" int mm_co_pacrr_bwd(const float* q, const float* d, const float* conv_w, const int32_t* saved_idx,
                               const float* grad_out, float* grad_q, float* grad_d, float* grad_w, float* grad_b,
                               int64_t n_pairs, int64_t pairs_per_query, int Q, int D, int E, int C, int N, int k,
                               int view0, int view1, int view2, int view3, void* workspace, size_t workspace_bytes,
                               void* stream) {
  if (!q || !d || !saved_idx || !grad_out || !grad_q || !grad_d || (N >= 2 && (!conv_w || !grad_w || !grad_b)))
    return set_error(MM_EINVAL, "mm_co_pacrr_bwd: null pointer argument");
  const int v[4] = {view0, view1, view2, view3};
  int rc = check_shape(n_pairs, pairs_per_query, Q, D, E, C, N, k, v, "mm_co_pacrr_bwd");
  if (rc != MM_OK) return rc;
  if (n_pairs == 0) return MM_OK;
  if (n_pairs > 0x7fffffff) return set_error(MM_EUNSUPPORTED, "mm_co_pacrr_bwd: %lld pairs in one call", (long long)n_pairs);
  const size_t need = mm_co_pacrr_workspace_bytes(n_pairs, Q, D, E, C, N, k);
  if (!workspace || workspace_bytes < need)
    return set_error(MM_EWORKSPACE, "mm_co_pacrr_bwd: workspace of %zu bytes, needs %zu", workspace_bytes, need);
  const CoBwdLds L(Q, D, C, N, 4 * k);
  float* ws = (float*)workspace;
  const size_t win = N >= 2 ? (size_t)n_pairs * Q * 4 * (size_t)k * (size_t)tap_off(N + 1) : 0;
  CoBwdArgs a{q, d, conv_w, saved_idx, grad_out, grad_q, grad_d, grad_w, grad_b, ws, ws + win,
              ws + win + (size_t)n_pairs * D * E, n_pairs, pairs_per_query, Q, D, E, C, N, k};
  (void)hipFuncSetAttribute((const void*)co_pacrr_bwd_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, L.total * (int)sizeof(float));
  hipLaunchKernelGGL(co_pacrr_bwd_kernel, dim3((unsigned)n_pairs), dim3(256), (size_t)L.total * sizeof(float),
                     (hipStream_t)stream, a);
  return check_launch("mm_co_pacrr_bwd");
}
