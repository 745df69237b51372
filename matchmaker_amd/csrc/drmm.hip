// DRMM (matchmaker/models/drmm.py:66-91): cosine match matrix -> per query token a histogram of the cosines over the
// document (torch.histc(row, bins, -1, 1)) -> log1p -> FeedForward(bins -> bins -> 1, tanh) -> gated sum.  ONE launch per
// call; the match matrix never leaves the registers, and with the fused head nothing of size Q x bins leaves the chip.
//
//   cos[i,j]  = (<q_i, d_j> * 1/(|q_i| + 1e-13)) * 1/(|d_j| + 1e-13)   the dot on v_mfma_f32_32x32x2_f32 (exact fp32: a
//               k-ordered fma chain — bin decisions are discontinuous, so no split-bf16 here)
//   bin       = min(int((cos + 1) / 2 * bins), bins - 1) in fp32, dropped when cos < -1 or cos > 1 (histc's rule; `clamp`
//               = 1 clamps the cosine into [-1, 1] first: a deliberate deviation, off by default)
//   head      = sum_i gate[i] * tanh(w2 . tanh(W1 log1p(h_i) + b1) + b2)
//
// Layout: one wavefront per workgroup, document tokens on the MFMA M axis, so lane (r, h) owns query token r and 16 of a
// block's 32 document rows: the counters are LANE-LOCAL.  Per block a lane adds 1 << 4 bin into two
// 64-bit words of sixteen 4-bit fields (8 cosines each: no field overflows), folds them into 8-bit fields that live for 8
// blocks, and unpacks those into sixteen 32-bit counters.  No LDS or global atomics: results are bit-deterministic.
//
// drmm_stream_kernel<NS> (E == 100 NS, Q <= 32): the document stream of kernel_pool_stream_kernel (kernel_pool.hip) —
//   HBM -> LDS by LDS-DMA in slices of 32 rows x 25 16-B chunks, a ring of three slices, the query tile in VGPRs.
// drmm_generic_kernel<NRT> (any E % 4 == 0 up to 1024, Q <= 32 NRT <= 64): direct fragment loads.
// Both skip the blocks past a pair's d_len and add the skipped columns to bin bins / 2 (the bin of a zero cosine).
#include "mm_internal.h"
#include "kp_device.h"

namespace mm {

namespace {

constexpr int kDQmax = 64, kDEmax = 1024, kDDmax = 65535, kDBmax = 16;

struct DrmmArgs {
  const float* q;
  const float* d;
  const int32_t* d_len;   // optional [n_pairs]: rows at or past it count as zero rows (never loaded past the block)
  float* hist;            // optional [n_pairs, Q, bins]
  float* score;           // optional [n_pairs]
  const float* gate;      // [n_pairs / ppq or n_pairs, Q]
  const float* W1;
  const float* b1;
  const float* w2;
  const float* b2;
  int64_t n_pairs, ppq, pairs_per_wave;
  int Q, D, E, bins;
  int gate_per_pair, clamp;
};

// ---- lane-local counters ------------------------------------------------------------------------------------------------
struct Bins {
  uint32_t ev[2], od[2];   // 8-bit fields: bins 0, 2, .. 14 / 1, 3, .. 15 (at most 16 per block: flushed every 8 blocks)
  int cnt[kDBmax];
  int pend;
  __device__ __forceinline__ void clear() {
    ev[0] = ev[1] = od[0] = od[1] = 0u;
    pend = 0;
#pragma unroll
    for (int k = 0; k < kDBmax; ++k) cnt[k] = 0;
  }
  __device__ __forceinline__ void flush() {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      cnt[2 * j] += (int)((ev[j >> 2] >> (8 * (j & 3))) & 0xffu);
      cnt[2 * j + 1] += (int)((od[j >> 2] >> (8 * (j & 3))) & 0xffu);
    }
    ev[0] = ev[1] = od[0] = od[1] = 0u;
    pend = 0;
  }
};

// One 32 x 32 tile: acc[i] of lane (r, h) is <d_row, q_r> for document row rowof(i) + 4 h of the block.  valid: bit per
// document row of the block (rows past the pair's length are not counted here).  hb = bins / 2 (exact in fp32):
// (c + 1) / 2 * bins == (c + 1) * hb bit for bit, because the division by two is exact.
__device__ __forceinline__ void bin_tile(Bins& B, const f32x16& acc, const float (&rdr)[16], float rq, uint32_t valid, int h,
                                         float hb, int bmax, bool clamp) {
  uint64_t nib[2] = {0ull, 0ull};
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    float c = (acc[i] * rq) * rdr[i];
    if (clamp) c = __builtin_amdgcn_fmed3f(c, -1.0f, 1.0f);
    const bool in = ((valid >> (rowof(i) + 4 * h)) & 1u) && c >= -1.0f && c <= 1.0f;
    const float t = __fmul_rn(__fadd_rn(c, 1.0f), hb);
    int b = (int)t;
    b = b < 0 ? 0 : (b > bmax ? bmax : b);
    nib[i >> 3] += (uint64_t)(in ? 1u : 0u) << (4 * b);
  }
  constexpr uint32_t M = 0x0f0f0f0fu;
#pragma unroll
  for (int w = 0; w < 2; ++w) {
    const uint32_t a = (uint32_t)(nib[0] >> (32 * w)), b = (uint32_t)(nib[1] >> (32 * w));
    B.ev[w] += (a & M) + (b & M);
    B.od[w] += ((a >> 4) & M) + ((b >> 4) & M);
  }
  if (++B.pend == 8) B.flush();
}

// W1 [nb, nb] | b1 [nb] | w2 [nb] | b2: nb^2 + 2 nb + 1 floats of LDS, staged only when a score is asked for
__host__ __device__ __forceinline__ int head_floats(int nb) { return nb * nb + 2 * nb + 1; }

__device__ __forceinline__ void stage_head(const DrmmArgs& a, float* hl, int lane) {
  if (!a.score) return;
  const int nb = a.bins;
  for (int i = lane; i < nb * nb; i += 64) hl[i] = a.W1[i];
  if (lane < nb) {
    hl[nb * nb + lane] = a.b1[lane];
    hl[nb * nb + nb + lane] = a.w2[lane];
  }
  if (lane == 0) hl[nb * nb + 2 * nb] = a.b2[0];
}

// End of a pair: the two lane halves meet, the skipped tail goes to the bin of a zero cosine, then hist and / or the head.
// row = the lane's query token (lanes of the upper half and tokens >= Q write nothing).
__device__ __forceinline__ float finish_rows(const DrmmArgs& a, int64_t pair, Bins& B, int row, int lane, int skipped,
                                             const float* hl) {
  if (B.pend) B.flush();
  const int nb = a.bins, mid = nb >> 1;
  float x[kDBmax];
#pragma unroll
  for (int k = 0; k < kDBmax; ++k) {
    int c = B.cnt[k] + __shfl_xor(B.cnt[k], 32, 64);
    if (k == mid) c += skipped;
    x[k] = (float)c;
  }
  const bool own = lane < 32 && row < a.Q;
  if (a.hist && own) {
    float* o = a.hist + (pair * a.Q + row) * (int64_t)nb;
#pragma unroll
    for (int k = 0; k < kDBmax; ++k)
      if (k < nb) o[k] = x[k];
  }
  float s = 0.0f;
  if (a.score) {
#pragma unroll
    for (int k = 0; k < kDBmax; ++k) x[k] = k < nb ? log1pf(x[k]) : 0.0f;
    float o = hl[nb * nb + 2 * nb];
    for (int j = 0; j < nb; ++j) {
      float t = hl[nb * nb + j];
#pragma unroll
      for (int k = 0; k < kDBmax; ++k)
        if (k < nb) t = fmaf(hl[j * nb + k], x[k], t);
      o = fmaf(hl[nb * nb + nb + j], tanhf(t), o);
    }
    const int64_t g = a.gate_per_pair ? pair : pair / a.ppq;
    if (own) s = a.gate[g * a.Q + row] * tanhf(o);
  }
  return s;
}

__device__ __forceinline__ int pair_len(const DrmmArgs& a, int64_t p) {
  int len = a.d_len ? (int)sload_u32(a.d_len, p) : a.D;
  return len < 0 ? 0 : (len > a.D ? a.D : len);
}

__device__ __forceinline__ void load_rdr(const float* rdbuf, int h, float (&rdr)[16]) {
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const f32x4 v = *(const f32x4*)(rdbuf + 8 * g + 4 * h);
    rdr[4 * g + 0] = v[0]; rdr[4 * g + 1] = v[1]; rdr[4 * g + 2] = v[2]; rdr[4 * g + 3] = v[3];
  }
}

// ---- the LDS-DMA document stream (the slice geometry of kernel_pool.hip's streaming kernels) -----------------------------
constexpr int kNbuf = 3;

template <int NS>
__global__ void __launch_bounds__(64) drmm_stream_kernel(const DrmmArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x;
  const int r = lane & 31, h = lane >> 5;
  const int64_t p0 = (int64_t)blockIdx.x * a.pairs_per_wave;
  const int64_t p1 = (p0 + a.pairs_per_wave < a.n_pairs) ? p0 + a.pairs_per_wave : a.n_pairs;
  if (p0 >= p1) return;
  constexpr int E = 100 * NS;
  constexpr int RB = E * 4;  // row bytes
  const int D = a.D, Q = a.Q;
  const int nblk_tot = (D + 31) >> 5;
  const int rows_last = D - 32 * (nblk_tot - 1);
  const uint32_t lds0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)smem;
  float* rdbuf = (float*)(smem + kNbuf * kSliceBytes);  // 32 floats: 1/(|d|+tiny) of the block's rows
  float* hl = rdbuf + 32;
  stage_head(a, hl, lane);

  // LDS-DMA source offsets: slot s = 64n + lane of the slice image [32 rows][25 chunks]
  uint32_t voff[kSliceInstr];
#pragma unroll
  for (int n = 0; n < kSliceInstr; ++n) {
    int s = 64 * n + lane;
    if (s > 32 * kSC - 1) s = 32 * kSC - 1;  // the last half instruction re-reads the final chunk
    const int row = s / kSC, c = s - row * kSC;
    voff[n] = (uint32_t)(row * RB + c * 16);
  }
  const uint32_t vmax_tail = (uint32_t)((rows_last - 1) * RB + (kSC - 1) * 16);
  const uint32_t a_off = (uint32_t)(r * (kSC * 16) + h * 16);  // this lane's A-fragment base inside a slice

  const char* dbase = (const char*)a.d;
  // producer cursor over (pair, block, slice)
  int64_t pp = p0;
  int pt = 0, ps = 0, pn = 0;
  while (pp < p1 && (pn = (pair_len(a, pp) + 31) >> 5) == 0) ++pp;
  int pbuf = 0, cbuf = 0, inflight = 0;
  auto top_up = [&]() {
    while (pp < p1 && inflight < kNbuf) {
      const char* g = dbase + (pp * D + (int64_t)pt * 32) * RB + ps * (kSC * 16);
      issue_slice<true>(g, voff, vmax_tail, pt == nblk_tot - 1 && rows_last != 32, lds0 + (uint32_t)pbuf * kSliceBytes);
      pbuf = (pbuf + 1 == kNbuf) ? 0 : pbuf + 1;
      ++inflight;
      if (++ps == NS) {
        ps = 0;
        if (++pt == pn) {
          pt = 0;
          ++pp;
          while (pp < p1 && (pn = (pair_len(a, pp) + 31) >> 5) == 0) ++pp;
        }
      }
    }
  };
  top_up();

  f32x4 qf[NS][kPairSteps];
  float rq = 0.0f;
  int64_t cur_q = -1;
  const float hb = 0.5f * (float)a.bins;
  const int bmax = a.bins - 1;
  const bool clamp = a.clamp != 0;

  for (int64_t pair = p0; pair < p1; ++pair) {
    const int64_t qi = pair / a.ppq;
    if (qi != cur_q) {
      cur_q = qi;
      const int qr = r < Q ? r : Q - 1;
      const char* qrow = (const char*)a.q + (qi * Q + qr) * RB + h * 16;
      float ss = 0.0f;
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        const char* base = qrow + s * (kSC * 16);
#pragma unroll
        for (int p = 0; p < kPairSteps; ++p) {
          // chunk pair p of the slice: lane half h takes chunk 2p + h; chunk 25 does not exist
          const bool ok = !(p == kPairSteps - 1 && h);
          qf[s][p] = ok ? *(const f32x4*)(base + p * 32) : f32x4{0, 0, 0, 0};
#pragma unroll
          for (int j = 0; j < 4; ++j) ss += qf[s][p][j] * qf[s][p][j];
        }
      }
      ss += __shfl_xor(ss, 32, 64);
      rq = 1.0f / (sqrtf(ss) + kTiny);
    }
    const int len = pair_len(a, pair);
    const int nb = (len + 31) >> 5;
    Bins B;
    B.clear();

    for (int t = 0; t < nb; ++t) {
      f32x16 acc = {0};
      f32x2 ss2 = {0.0f, 0.0f};
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        top_up();
        wait_slices<kNbuf - 1>(inflight - 1);
        const char* buf = smem + cbuf * kSliceBytes + a_off;
#pragma unroll
        for (int p = 0; p < kPairSteps; ++p) {
          f32x4 av = *(const f32x4*)(buf + p * 32);
          if (p == kPairSteps - 1 && h) av = f32x4{0, 0, 0, 0};
#pragma unroll
          for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[j], qf[s][p][j], acc, 0, 0, 0);
          const f32x2 lo = {av[0], av[1]}, hi = {av[2], av[3]};
          ss2 += lo * lo;
          ss2 += hi * hi;
        }
        cbuf = (cbuf + 1 == kNbuf) ? 0 : cbuf + 1;
        --inflight;
      }
      // document-token norms: lane (r,h) summed the even/odd chunks of row r
      float ss = ss2[0] + ss2[1];
      ss += __shfl_xor(ss, 32, 64);
      if (h == 0) rdbuf[r] = 1.0f / (sqrtf(ss) + kTiny);
      float rdr[16];
      load_rdr(rdbuf, h, rdr);
      const int rem = len - 32 * t;
      const uint32_t valid = rem >= 32 ? 0xffffffffu : ((1u << rem) - 1u);
      bin_tile(B, acc, rdr, rq, valid, h, hb, bmax, clamp);
    }
    float s = finish_rows(a, pair, B, r, lane, D - len, hl);
    if (a.score) {
      s = wave_sum(s);
      if (lane == 0) a.score[pair] = s;
    }
  }
}

// ---- any shape within the limits: direct fragment loads ---------------------------------------------------------------
template <int NRT>
__global__ void __launch_bounds__(64) drmm_generic_kernel(const DrmmArgs a) {
  __shared__ __attribute__((aligned(16))) float lds[32 + kDBmax * kDBmax + 2 * kDBmax + 4];
  const int lane = threadIdx.x;
  const int r = lane & 31, h = lane >> 5;
  const int64_t p0 = (int64_t)blockIdx.x * a.pairs_per_wave;
  const int64_t p1 = (p0 + a.pairs_per_wave < a.n_pairs) ? p0 + a.pairs_per_wave : a.n_pairs;
  if (p0 >= p1) return;
  const int D = a.D, Q = a.Q, E = a.E;
  const int nch = (E + 7) >> 3;
  float* rdbuf = lds;
  float* hl = lds + 32;
  stage_head(a, hl, lane);
  const float hb = 0.5f * (float)a.bins;
  const int bmax = a.bins - 1;
  const bool clamp = a.clamp != 0;

  float rq[NRT];
  const float* qp[NRT];
  int64_t cur_q = -1;
  for (int64_t pair = p0; pair < p1; ++pair) {
    const int64_t qi = pair / a.ppq;
    if (qi != cur_q) {
      cur_q = qi;
#pragma unroll
      for (int rt = 0; rt < NRT; ++rt) {
        const int row = rt * 32 + r;
        qp[rt] = a.q + (qi * Q + (row < Q ? row : Q - 1)) * (int64_t)E;
        float ss = 0.0f;
        for (int m = 0; m < nch; ++m) {
          const int k0 = 8 * m + 4 * h;
          ss += sumsq4(load4_or0(qp[rt] + k0, k0 < E));
        }
        ss += __shfl_xor(ss, 32, 64);
        rq[rt] = 1.0f / (sqrtf(ss) + kTiny);
      }
    }
    const int len = pair_len(a, pair);
    const int nb = (len + 31) >> 5;
    Bins B[NRT];
#pragma unroll
    for (int rt = 0; rt < NRT; ++rt) B[rt].clear();

    for (int t = 0; t < nb; ++t) {
      const int drow = 32 * t + r < D ? 32 * t + r : D - 1;   // rows past the document: a copy of the last one, never counted
      const float* dp = a.d + (pair * D + drow) * (int64_t)E;
      f32x16 acc[NRT];
#pragma unroll
      for (int rt = 0; rt < NRT; ++rt) acc[rt] = f32x16{};
      float ss = 0.0f;
      for (int m = 0; m < nch; ++m) {
        const int k0 = 8 * m + 4 * h;
        const bool kin = k0 < E;
        const f32x4 dv = load4_or0(dp + k0, kin);
        ss += sumsq4(dv);
#pragma unroll
        for (int rt = 0; rt < NRT; ++rt) {
          const f32x4 qv = load4_or0(qp[rt] + k0, kin);
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[rt] = __builtin_amdgcn_mfma_f32_32x32x2f32(dv[j], qv[j], acc[rt], 0, 0, 0);
        }
      }
      ss += __shfl_xor(ss, 32, 64);
      if (h == 0) rdbuf[r] = 1.0f / (sqrtf(ss) + kTiny);
      float rdr[16];
      load_rdr(rdbuf, h, rdr);
      const int rem = len - 32 * t;
      const uint32_t valid = rem >= 32 ? 0xffffffffu : ((1u << rem) - 1u);
#pragma unroll
      for (int rt = 0; rt < NRT; ++rt) bin_tile(B[rt], acc[rt], rdr, rq[rt], valid, h, hb, bmax, clamp);
    }
    float s = 0.0f;
#pragma unroll
    for (int rt = 0; rt < NRT; ++rt) s += finish_rows(a, pair, B[rt], rt * 32 + r, lane, D - len, hl);
    if (a.score) {
      s = wave_sum(s);
      if (lane == 0) a.score[pair] = s;
    }
  }
}

template <typename Kern>
int launch(Kern kern, DrmmArgs a, int lds, hipStream_t stream, const char* what) {
  const unsigned waves = split_pairs(a, (int64_t)kCUs * 4);   // one wavefront per SIMD: the fp32 MFMA pipe is the co-limiter (as kernel pooling)
  hipLaunchKernelGGL(kern, dim3(waves), dim3(64), (size_t)lds, stream, a);
  return check_launch(what);
}

}  // namespace
}  // namespace mm

using namespace mm;

extern "C" size_t mm_drmm_workspace_bytes(int64_t n_pairs, int Q, int D, int E, int bins) {
  (void)n_pairs; (void)Q; (void)D; (void)E; (void)bins;
  return 0;   // the counters live in registers
}

extern "C" int mm_drmm_fwd(const float* q, const float* d, const int32_t* d_len, float* hist, float* score, const float* gate,
                           int gate_per_pair, const float* W1, const float* b1, const float* w2, const float* b2,
                           int64_t n_pairs, int64_t pairs_per_query, int Q, int D, int E, int bins, int clamp,
                           void* workspace, size_t workspace_bytes, void* stream) {
  (void)workspace;
  (void)workspace_bytes;
  if (!q || !d || (!hist && !score)) return set_error(MM_EINVAL, "mm_drmm_fwd: null q / d, or neither hist nor score");
  if (score && (!gate || !W1 || !b1 || !w2 || !b2))
    return set_error(MM_EINVAL, "mm_drmm_fwd: score needs gate, W1, b1, w2 and b2");
  if (n_pairs < 0 || pairs_per_query < 1 || (gate_per_pair != 0 && gate_per_pair != 1) || (clamp != 0 && clamp != 1))
    return set_error(MM_EINVAL, "mm_drmm_fwd: n_pairs = %lld, pairs_per_query = %lld, gate_per_pair = %d, clamp = %d",
                     (long long)n_pairs, (long long)pairs_per_query, gate_per_pair, clamp);
  if (Q < 1 || Q > kDQmax || D < 1 || D > kDDmax || E < 4 || E > kDEmax || E % 4 || bins < 1 || bins > kDBmax)
    return set_error(MM_EUNSUPPORTED,
                     "mm_drmm_fwd: Q = %d, D = %d, E = %d, bins = %d outside 1 <= Q <= 64, 1 <= D <= 65535, 4 <= E <= 1024 "
                     "(a multiple of 4), 1 <= bins <= 16",
                     Q, D, E, bins);
  if (n_pairs == 0) return MM_OK;
  DrmmArgs a{q, d, d_len, hist, score, gate, W1, b1, w2, b2, n_pairs, pairs_per_query, 1, Q, D, E, bins, gate_per_pair, clamp};
  hipStream_t s = (hipStream_t)stream;
  if (Q <= 32 && (E == 100 || E == 200 || E == 300)) {
    // the ring + 128 B leave 896 B of a quarter of the CU's 160 KB: the head of up to 13 bins fits beside them, so four
    // workgroups still share a CU (14 .. 16 bins with a fused score: three)
    const int lds = kNbuf * kSliceBytes + (32 + (score ? head_floats(bins) : 0)) * (int)sizeof(float);
    if (E == 100) return launch(drmm_stream_kernel<1>, a, lds, s, "drmm_stream_kernel");
    if (E == 200) return launch(drmm_stream_kernel<2>, a, lds, s, "drmm_stream_kernel");
    return launch(drmm_stream_kernel<3>, a, lds, s, "drmm_stream_kernel");
  }
  if (Q <= 32) return launch(drmm_generic_kernel<1>, a, 0, s, "drmm_generic_kernel");
  return launch(drmm_generic_kernel<2>, a, 0, s, "drmm_generic_kernel");
}
