// PACRR (matchmaker/models/pacrr.py:68-113): cosine match matrix -> n-gram convolutions + channel max -> per-row k-max
// pooling, fused.  Forward: ONE launch per call, one workgroup (four wavefronts) per pair; the match matrix lives only in
// LDS, as a ring of 64 document columns (two 32-column blocks: the block being pooled and the next one, whose first n - 1
// columns are the convolutions' right halo).  Backward: ONE launch, one workgroup per pair (see pacrr_bwd_kernel).
//
// Arithmetic:
//   cosine   <q_i, d_j> * 1/(|q_i| + 1e-13) * 1/(|d_j| + 1e-13); the dot on v_mfma_f32_32x32x2_f32 (exact fp32: a k-ordered
//            fma chain), the four wavefronts split E and their partial tiles are summed in fixed order (deterministic);
//   conv     an im2col product [C x n^2] x [n^2 x 32 positions] on the same fp32 MFMA, the accumulator initialised with the
//            bias; the channel max is taken on the accumulators (lowest channel on ties, MaxPool3d's rule);
//   top-k    per (query row, path) a sorted list of k (value, column | channel << 16) in LDS, updated by whole-wave
//            insertions; ties keep the lower column first.
#include "mm_internal.h"

namespace mm {

namespace {

constexpr int kPQmax = 64, kPDmax = 2048, kPEmax = 1024, kPCmax = 64, kPNmax = 5, kPKmax = 32;
constexpr float kTiny = 1e-13f;   // allennlp's cosine (mm_native.h, kernel pooling)
constexpr int kPB = 3;           // chunks of 8 elements whose loads a wavefront issues together (cosine phase)
constexpr int kRing = 65;         // ring row stride in floats (64 columns + 1: rows land on distinct banks)

// sum of m^2 for m = 2 .. n - 1: offset of width n's taps in the packed weights (per channel), in units of C floats
__host__ __device__ __forceinline__ int tap_off(int n) { return (n - 1) * n * (2 * n - 1) / 6 - 1; }

__device__ __forceinline__ f32x16 mfma32(float a, float b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}

__device__ __forceinline__ f32x4 load4_or0(const float* p, bool ok) {
  return ok ? *(const f32x4*)p : f32x4{0.0f, 0.0f, 0.0f, 0.0f};
}

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
    part = o; o += 4 * nrt * 32 * 33;
    tv = o; o += Q * N * k;
    ti = o; o += Q * N * k;
    total = o;
  }
};

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

__global__ void __launch_bounds__(256, 4) pacrr_fwd_kernel(PacrrArgs a) {
  extern __shared__ float lds[];
  const int Q = a.Q, D = a.D, E = a.E, C = a.C, N = a.N, k = a.k;
  const FwdLds L(Q, C, N, k);
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r32 = lane & 31, h = lane >> 5;
  const int64_t pair = blockIdx.x;
  const float* q = a.q + (pair / a.ppq) * (int64_t)Q * E;
  const float* d = a.d + pair * (int64_t)D * E;
  const int nrt = (Q + 31) / 32, nch = (E + 7) / 8, nb = (D + 31) / 32, S = tap_off(N + 1);
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
  for (int i = w; i < Q; i += 4) {
    float s = 0.0f;
    for (int e = lane; e < E; e += 64) s += q[(int64_t)i * E + e] * q[(int64_t)i * E + e];
    s = wave_sum(s);
    if (lane == 0) rq[i] = 1.0f / (sqrtf(s) + kTiny);
  }
  __syncthreads();

  for (int s = 0; s <= nb; ++s) {
    // ---- cosine block s -> ring half (s & 1); s == nb: the zero columns past the document (ConstantPad2d)
    const int j0 = 32 * s, rb = (s & 1) * 32;
    if (s < nb) {
      f32x16 acc[2];
      acc[0] = f32x16{};
      acc[1] = f32x16{};
      float dsq = 0.0f;
      const bool drow = j0 + r32 < D;
      const float* dp = d + (int64_t)(j0 + r32) * E;
      // kPB chunks of 8 per batch: every load of a batch is issued before its first MFMA (one memory latency per batch,
      // not per chunk: the rows are 4 x 16 B per lane, far apart, and nothing else hides their latency)
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
    const bool ok = col < D;
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
struct BwdArgs {
  const float* q;
  const float* d;
  const float* w;
  const int32_t* idx;
  const float* go;   // [n_pairs, Q, k N]
  float* gq;         // [n_pairs, Q, E]
  float* gd;         // [n_pairs, D, E]
  float* gw;         // [n_pairs, C S]
  float* gb;         // [n_pairs, (N - 1) C]
  float* wincos;     // workspace [n_pairs, Q k S]
  int64_t n_pairs, ppq;
  int Q, D, E, C, N, k;
};

struct BwdLds {
  int rq, nq, rd, nd, wt, eg, ei, G, gwl, gbl, total;
  __host__ __device__ BwdLds(int Q, int D, int C, int N, int k) {
    const int S = tap_off(N + 1);
    int o = 0;
    rq = o; o += kPQmax;
    nq = o; o += kPQmax;
    rd = o; o += D;
    nd = o; o += D;
    wt = o; o += C * S;
    eg = o; o += Q * N * k;
    ei = o; o += Q * N * k;
    G = o; o += Q * 33;
    gwl = o; o += C * S;
    gbl = o; o += C * (N - 1);
    total = o;
  }
};

constexpr int kMaxEPerLane = kPEmax / 64;

// One workgroup per pair:
//   P0  norms of the query rows and of every document row, the weights, the pair's saved entries and their gradients -> LDS
//   P1  the cosine at every tap of every selected conv window (one dot each, recomputed from q / d) -> workspace
//   P2  grad_w / grad_b of the pair: thread (path, tap) owns column `tap` of that width's weight gradient, thread `path` its
//       bias gradient; each walks the entries in a fixed order (no atomics)
//   P3  per 32-column document block: the sparse dcos block gathered into LDS (each cell sums its contributions in a fixed
//       order), grad_d of the block's rows through the normalisation Jacobian, grad_q-hat accumulated in grad_q
//   P4  grad_q through the query's normalisation Jacobian
// The rows of P3 / P4 are wavefront-owned with one lane per 64th element: the thread that accumulates a grad_q element is the
// one that finishes it.
__global__ void __launch_bounds__(256) pacrr_bwd_kernel(BwdArgs a) {
  extern __shared__ float lds[];
  const int Q = a.Q, D = a.D, E = a.E, C = a.C, N = a.N, k = a.k;
  const int S = tap_off(N + 1), NK = N * k;
  const BwdLds L(Q, D, C, N, k);
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
  float* wc = a.wincos + pair * (int64_t)Q * k * S;
  const int ME = (E + 63) / 64;

  // ---- P0
  for (int i = tid; i < C * S; i += 256) {
    wt[i] = a.w[i];
    gwl[i] = 0.0f;
  }
  for (int i = tid; i < C * (N - 1); i += 256) gbl[i] = 0.0f;
  for (int i = tid; i < Q * NK; i += 256) {
    eg[i] = a.go[pair * (int64_t)Q * NK + i];
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

int check_shape(int64_t n_pairs, int64_t ppq, int Q, int D, int E, int C, int N, int k, const char* what) {
  if (n_pairs < 0 || ppq < 1) return set_error(MM_EINVAL, "%s: n_pairs = %lld, pairs_per_query = %lld", what, (long long)n_pairs, (long long)ppq);
  if (Q < 1 || Q > kPQmax || k < 1 || k > kPKmax || D < k || D > kPDmax || E < 4 || E > kPEmax || E % 4 || C < 1 ||
      C > kPCmax || N < 1 || N > kPNmax)
    return set_error(MM_EUNSUPPORTED,
                     "%s: Q = %d, D = %d, E = %d, C = %d, N = %d, k = %d outside 1 <= Q <= 64, k <= D <= 2048, 4 <= E <= 1024 "
                     "(a multiple of 4), 1 <= C <= 64, 1 <= N <= 5, 1 <= k <= 32",
                     what, Q, D, E, C, N, k);
  return MM_OK;
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
  if (!q || !d || !out || (N >= 2 && (!conv_w || !conv_b)))
    return set_error(MM_EINVAL, "mm_pacrr_fwd: null q / d / out, or null conv_w / conv_b with N >= 2");
  int rc = check_shape(n_pairs, pairs_per_query, Q, D, E, C, N, k, "mm_pacrr_fwd");
  if (rc != MM_OK) return rc;
  if (n_pairs == 0) return MM_OK;
  if (n_pairs > 0x7fffffff) return set_error(MM_EUNSUPPORTED, "mm_pacrr_fwd: %lld pairs in one call", (long long)n_pairs);
  const FwdLds L(Q, C, N, k);
  PacrrArgs a{q, d, conv_w, conv_b, out, saved_idx, n_pairs, pairs_per_query, Q, D, E, C, N, k};
  (void)hipFuncSetAttribute((const void*)pacrr_fwd_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, L.total * (int)sizeof(float));
  hipLaunchKernelGGL(pacrr_fwd_kernel, dim3((unsigned)n_pairs), dim3(256), (size_t)L.total * sizeof(float),
                     (hipStream_t)stream, a);
  return check_launch("mm_pacrr_fwd");
}

extern "C" int mm_pacrr_bwd(const float* q, const float* d, const float* conv_w, const int32_t* saved_idx,
                            const float* grad_out, float* grad_q, float* grad_d, float* grad_w, float* grad_b,
                            int64_t n_pairs, int64_t pairs_per_query, int Q, int D, int E, int C, int N, int k,
                            void* workspace, size_t workspace_bytes, void* stream) {
  if (!q || !d || !saved_idx || !grad_out || !grad_q || !grad_d || (N >= 2 && (!conv_w || !grad_w || !grad_b)))
    return set_error(MM_EINVAL, "mm_pacrr_bwd: null pointer argument");
  int rc = check_shape(n_pairs, pairs_per_query, Q, D, E, C, N, k, "mm_pacrr_bwd");
  if (rc != MM_OK) return rc;
  if (n_pairs == 0) return MM_OK;
  if (n_pairs > 0x7fffffff) return set_error(MM_EUNSUPPORTED, "mm_pacrr_bwd: %lld pairs in one call", (long long)n_pairs);
  const size_t need = mm_pacrr_workspace_bytes(n_pairs, Q, D, C, N, k);
  if (need && (!workspace || workspace_bytes < need))
    return set_error(MM_EWORKSPACE, "mm_pacrr_bwd: workspace of %zu bytes, needs %zu", workspace_bytes, need);
  const BwdLds L(Q, D, C, N, k);
  BwdArgs a{q, d, conv_w, saved_idx, grad_out, grad_q, grad_d, grad_w, grad_b, (float*)workspace, n_pairs,
            pairs_per_query, Q, D, E, C, N, k};
  (void)hipFuncSetAttribute((const void*)pacrr_bwd_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, L.total * (int)sizeof(float));
  hipLaunchKernelGGL(pacrr_bwd_kernel, dim3((unsigned)n_pairs), dim3(256), (size_t)L.total * sizeof(float),
                     (hipStream_t)stream, a);
  return check_launch("mm_pacrr_bwd");
}
