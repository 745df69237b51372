// ONE copy of the phases the two exact-f32 tiled backward kernels have in common: kernel_pool_bwd_tiled_kernel (kernel_pool_bwd.hip,
// TK pooling) and tkl_bwd_tiled_kernel (tkl_bwd.hip, TKL).  Both keep a normalised query tile QH [Q][ES] and one 32-row block of raw
// document rows DB [32][ES] in LDS and run three small products per block on the matrix pipe in exact float32
// (v_mfma_f32_32x32x2_f32) with NW = NTHR / 64 wavefronts:
//   * cosines C = DB QH^T: K = E split between the wavefronts, the partial 32 x 32 tiles meet in LDS in a fixed order
//     (cosine_partials, partial_sum);
//   * grad_d block [32 rows x E] = G Qh: wavefront w owns the 32-column tiles w, w + NW of E, K = the query tokens
//     (grad_d_operand, grad_d_tile);
//   * grad_q [Q x E] += (G / (|d| + tiny)) DB: the same column tiles, K = the block's 32 rows, accumulated in registers across the
//     blocks (grad_q_accumulate) and finished once (grad_q_store_tile).
// What differs stays in the kernels: where a row comes from (their fetch()), everything between the cosines and G, how a grad_d tile
// is stored, and TKL's extra term of grad_q (the `fin` argument of grad_q_store_tile).
// Everything the matrix pipe is fed with is read unconditionally (clamped addresses, zeros selected afterwards): a conditional LDS
// read in front of an MFMA becomes a branch, a wait and an exposed latency per step.
// Free functions only; LDS tiles and lane coordinates (ln = lane & 31, lh = (lane >> 5) & 1 of the MFMA layout, wv = wavefront) are
// plain arguments.
#pragma once
#include "mm_internal.h"

namespace mm {
namespace bwd_tiled {

// Row stride of the [row][E] tiles in floats: an ODD number of 16-byte units, so that the sixteen lanes of a ds_read_b128
// phase that read one column chunk of sixteen consecutive rows (the A / B operands of the cosine MFMAs) cover all 64 banks.
// (E + 4 alone is even for E = 300: 304 floats = 48 banks apart, rows r and r + 4 on the same banks, 8-way conflicts.)
__host__ __device__ inline int row_stride(int E) { return ((E >> 2) & 1) ? E + 8 : E + 4; }

__device__ __forceinline__ float dot4(const f32x4& a, const f32x4& b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2] + a[3] * b[3]; }

// BWD_KEEP16(v): the sixteen values are computed HERE.  Without it the compiler sinks each value's LDS reads and arithmetic
// into the lane-conditional block of the store that uses it: per store two dependent LDS round trips behind a branch.  (One
// statement for all sixteen: a volatile asm per value orders them and serialises the reads just the same — both measured, 35 %
// and 17 % of the kernel.)
#define BWD_KEEP16(v)                                                                                                         \
  asm volatile("" : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]), "+v"(v[4]), "+v"(v[5]), "+v"(v[6]), "+v"(v[7]), "+v"(v[8]), \
               "+v"(v[9]), "+v"(v[10]), "+v"(v[11]), "+v"(v[12]), "+v"(v[13]), "+v"(v[14]), "+v"(v[15]))

// Phase clocks (tools/build_variant.sh phases kernel_pool_bwd -DMM_KP_BWD_PHASE_TIMES=1, ... phases tkl_bwd -DMM_TKL_BWD_PHASE_TIMES=1;
// tools/bench_kp_bwd_phases.py, tools/bench_tkl_bwd_phases.py): thread 0 of a workgroup sums s_memtime deltas per phase into the
// kernel's `ph` and the first workgroup overwrites the head of a parameter-gradient row with them.
#ifndef MM_KP_BWD_PHASE_TIMES
#define MM_KP_BWD_PHASE_TIMES 0
#endif
#ifndef MM_TKL_BWD_PHASE_TIMES
#define MM_TKL_BWD_PHASE_TIMES 0
#endif
#if MM_KP_BWD_PHASE_TIMES || MM_TKL_BWD_PHASE_TIMES
#define BWD_PH(k) do { const long long t_ = clock64(); ph[k] += (float)(t_ - t_last); t_last = t_; } while (0)
#else
#define BWD_PH(k) do { } while (0)
#endif

// ---------------------------------------------------------------------------------------------------------------- rows and norms
// raw query rows [Q][E] -> QH [Q][ES], 16 bytes per thread and step
template <int NTHR>
__device__ __forceinline__ void load_query_rows(float* QH, const float* qb, int Q, int NC, int E, int ES, int tid) {
  for (int idx = tid; idx < Q * NC; idx += NTHR) {
    const int i = idx / NC, c = idx - i * NC;
    *(f32x4*)(QH + i * ES + 4 * c) = *(const f32x4*)(qb + (int64_t)i * E + 4 * c);
  }
}

// sum over the sixteen lanes that share a row (sub = lane & 15); every one of them gets the total
__device__ __forceinline__ float sum16(float v) {
#pragma unroll
  for (int o = 1; o < 16; o <<= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// sum of squares of an LDS row of nc 16-byte chunks, sixteen threads per row: lane `sub` takes the chunks sub, sub + 16, ...
// (nc = 0 for a row that does not exist: whole wavefronts reach the shuffles)
__device__ __forceinline__ float row_sumsq16(const float* row, int nc, int sub) {
  float ss = 0.0f;
  for (int c = sub; c < nc; c += 16) {
    const f32x4 v = *(const f32x4*)(row + 4 * c);
    ss += dot4(v, v);
  }
  return sum16(ss);
}

// the row times r, in place, by the same sixteen threads
__device__ __forceinline__ void scale_row16(float* row, int nc, int sub, float r) {
  for (int c = sub; c < nc; c += 16) {
    f32x4* p = (f32x4*)(row + 4 * c);
    *p = *p * r;
  }
}

// ---------------------------------------------------------------------------------------------------------------------- staging
// A block of rows travels global -> registers -> LDS in two steps: the kernel's fetch() issues every load of a thread's share at
// once (kLB <= 8 chunks of 16 bytes = ceil(32 (E / 4) / NTHR)) and is called one block AHEAD, right after the barrier that opens the
// current block's arithmetic; stage_commit() stores them to DB once that arithmetic has read the current block.  With one
// workgroup per CU nothing else hides the load latency: issued at the point of use (round 4's first version) it was half of the
// kernels' time.  A thread's chunks are the same (row, column) in every block: frow = 32 marks a chunk it does not have.
template <int kLB, int NTHR>
__device__ __forceinline__ void stage_plan(int tid, int NC, int (&frow)[kLB], int (&fcol)[kLB]) {
#pragma unroll
  for (int u = 0; u < kLB; ++u) {
    const int idx = tid + u * NTHR;
    frow[u] = 32;
    fcol[u] = 0;
    if (idx < 32 * NC) {
      frow[u] = idx / NC;
      fcol[u] = 4 * (idx - frow[u] * NC);
    }
  }
}

template <int kLB>
__device__ __forceinline__ void stage_commit(float* DB, int ES, const int (&frow)[kLB], const int (&fcol)[kLB], const f32x4 (&nxt)[kLB]) {
#pragma unroll
  for (int u = 0; u < kLB; ++u)
    if (frow[u] < 32) *(f32x4*)(DB + frow[u] * ES + fcol[u]) = nxt[u];
}

// ---------------------------------------------------------------------------------------------------------------------- cosines
// This wavefront's K slice of the 32 x 32 tile DB QH^T (wavefront w takes the 32-byte chunk pairs w, w + NW, ...: A = document
// rows, B = query tokens, both read as 16 bytes per lane and four MFMA steps), left in PS [NW / 2][32 rows][32 tokens]: wavefronts
// w and w + NW / 2 share a slot, the upper one stores, the lower one adds behind the barrier INSIDE.  The caller follows with a
// barrier and partial_sum().
template <int NW>
__device__ __forceinline__ void cosine_partials(const float* DB, const float* QH, float* PS, int Q, int NC, int ES, int wv, int ln, int lh) {
  constexpr int NS = NW / 2;
  f32x16 acc = {0};
  const float* arow = DB + ln * ES;
  const float* brow = QH + (ln < Q ? ln : Q - 1) * ES;
  for (int p = wv; 2 * p < NC; p += NW) {
    const int cc = 2 * p + lh;
    const int cl = cc < NC ? cc : NC - 1;            // (odd NC: the last pair's upper half multiplies zeros)
    f32x4 av = *(const f32x4*)(arow + 4 * cl);
    const f32x4 bv = *(const f32x4*)(brow + 4 * cl);
    if (cc >= NC) av = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[j], bv[j], acc, 0, 0, 0);
  }
  float* ps = PS + (wv % NS) * 1024 + 4 * lh * 32 + ln;
  if (wv >= NS) {
#pragma unroll
    for (int i = 0; i < 16; ++i) ps[rowof(i) * 32] = acc[i];
  }
  __syncthreads();
  if (wv < NS) {
#pragma unroll
    for (int i = 0; i < 16; ++i) ps[rowof(i) * 32] += acc[i];
  }
}

// element idx = 32 row + token of the tile: the NS slots summed in slot order (un-normalised: the caller multiplies by 1 / (|d| + tiny))
template <int NS>
__device__ __forceinline__ float partial_sum(const float* PS, int idx) {
  float v = PS[idx];
#pragma unroll
  for (int w = 1; w < NS; ++w) v += PS[w * 1024 + idx];
  return v;
}

// ----------------------------------------------------------------------------------------------------------------------- grad_d
// A operand of the grad_d product: ga[st] = G[row lq][token 2 st + hq] out of the [32][QS] tile (K = tokens, two per step; zero
// past Q), shared by the wavefront's column tiles
__device__ __forceinline__ void grad_d_operand(float (&ga)[16], const float* G, int Q, int QS, int lq, int hq) {
#pragma unroll
  for (int st = 0; st < 16; ++st) {
    const int i = 2 * st + hq;
    ga[st] = G[lq * QS + (i < QS ? i : QS - 1)];
    if (i >= Q) ga[st] = 0.0f;
  }
}

// one 32-row x 32-column tile of G Qh: B = Qh[token][column] (qcol = QH + the lane's column: consecutive lanes read consecutive
// floats), KQ = ceil(Q / 2) MFMA steps in pairs
__device__ __forceinline__ f32x16 grad_d_tile(const float (&ga)[16], const float* qcol, int Q, int KQ, int ES, int hq) {
  float bq[16];
#pragma unroll
  for (int st = 0; st < 16; ++st) {
    const int i = 2 * st + hq;
    bq[st] = qcol[(i < Q ? i : Q - 1) * ES];       // (multiplied by ga = 0 past Q)
  }
  f32x16 acc = {0};
#pragma unroll
  for (int g2 = 0; g2 < 8; ++g2) {
    if (2 * g2 < KQ) {                             // wave-uniform
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ga[2 * g2], bq[2 * g2], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ga[2 * g2 + 1], bq[2 * g2 + 1], acc, 0, 0, 0);
    }
  }
  return acc;
}

// ----------------------------------------------------------------------------------------------------------------------- grad_q
// accq[t] += (G / (|d| + tiny)) DB on this wavefront's column tiles: A[token][row] = GI[token][row] rd[row] out of the [QS][32]
// tile (K = the block's 32 rows), B = the raw document block, sixteen MFMAs per tile
template <int NW, int TPW>
__device__ __forceinline__ void grad_q_accumulate(f32x16 (&accq)[TPW], const float* GI, const float* rd, const float* DB, int Q, int E,
                                                  int ES, int NT, int wv, int lq, int hq) {
  float gi[16];
  const int tk = lq < Q ? lq : Q - 1;
#pragma unroll
  for (int st = 0; st < 16; ++st) {
    const int i = 2 * st + hq;
    gi[st] = GI[tk * 32 + i] * rd[i];
    if (lq >= Q) gi[st] = 0.0f;
  }
#pragma unroll
  for (int t = 0; t < TPW; ++t) {
    const int nt = wv + NW * t;
    if (nt >= NT) break;                             // wave-uniform
    const int col = 32 * nt + lq;
    const float* dcol = DB + (col < E ? col : 0);
    float bd[16];
#pragma unroll
    for (int st = 0; st < 16; ++st) bd[st] = dcol[(2 * st + hq) * ES];
#pragma unroll
    for (int st = 0; st < 16; ++st) accq[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(gi[st], bd[st], accq[t], 0, 0, 0);
  }
}

// column `col` (< E) of grad_q out of one finished accumulator tile: fin((acc - qh self) rq, token) with self = sum_j G c of the
// token (0 for a zero vector, as torch.norm's backward defines it; QH holds q_i / |q_i| to 1e-13); gq is the pair's [Q][E]
template <class Fin>
__device__ __forceinline__ void grad_q_store_tile(const f32x16& acc, const float* QH, const float* nq, const float* sq, const float* rq,
                                                  float* gq, int Q, int E, int ES, int col, int lh, Fin fin) {
  float ov[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int tok = rowof(i) + 4 * lh, tc = tok < Q ? tok : Q - 1;
    const float self = nq[tc] > 0.0f ? sq[tc] : 0.0f;
    ov[i] = fin((acc[i] - QH[tc * ES + col] * self) * rq[tc], tc);
  }
  BWD_KEEP16(ov);
#pragma unroll
  for (int i = 0; i < 16; ++i)
    if (rowof(i) + 4 * lh < Q) gq[(uint32_t)((rowof(i) + 4 * lh) * E + col)] = ov[i];
}

}  // namespace bwd_tiled
}  // namespace mm
