// fp8 ColBERT token store for MI355X (gfx950 / CDNA4): row quantiser and ragged MaxSim over the quantised rows.
//
// Store format (include/mm_native.h): codes [T, E] uint8 = OCP e4m3fn bytes, scales [T] float32 = one power
// of two per token row; a row's values are deq(code_k) * scale, an exact product.
//
//   out[p] = sum_{i<Q, qmask}  max_{t in [begin_p, end_p)} ( scales[t] * sum_k q[i,k] * deq(codes[t,k]) )
//
// Three kernels:
//   * fp8_quantize_rows_kernel — one 16-lane group per row: row maximum (4 shuffles), scale, v_cvt_pk_fp8_f32.
//   * maxsim_fp8_stream_kernel — the structure of maxsim_stream_body<.., RAG = true> (maxsim.hip) with a document side of one
//     byte per element: an 8 KiB ring slot holds 64 token rows x 128 codes, an A fragment is an 8-byte LDS read converted in
//     registers to the query's 16-bit type (v_cvt_scalef32_pk_{bf16,f16}_fp8, scale 1.0: every e4m3 value is exact in both)
//     and fed to the same v_mfma_f32_32x32x16_{bf16,f16}.  The 64 row scales of a block ride in the slot's 256-byte tail
//     and multiply the finished fp32 dot products before the running maximum.
//   * maxsim_fp8_plain_kernel — any E % 16 == 0, any Q: one wavefront per pair, direct loads.  A correctness path.
#include "mm_internal.h"
#include "maxsim_device.h"
#include "fp8_device.h"

namespace mm {

struct Fp8Args {
  const void* q;
  const uint8_t* codes;
  const float* scales;
  PackedMask qm;
  float* out;
  int64_t n_pairs;
  int64_t ppq;
  int64_t pairs_per_wave;
  const int64_t* begin;
  const int64_t* end;
  int Q, E;
  int rnd;
};

// ---------------------------------------------------------------------------------------------
// Quantiser.  One 16-lane group per row (four rows per wavefront, 16 per workgroup); the per-row code is fp8_quantize_row
// (fp8_device.h), which the store writer's scatter kernel runs as well.
// No atomics, every output byte written once, no dependence on launch geometry: two calls give the same bits.
// ---------------------------------------------------------------------------------------------
template <int DT>
__global__ void __launch_bounds__(256) fp8_quantize_rows_kernel(const void* x, int64_t n_rows, int E, uint8_t* codes, float* scales) {
  const int l = threadIdx.x & 15;
  const int64_t row = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
  if (row >= n_rows) return;                       // (a whole 16-lane group leaves; the shuffles stay inside a group)
  constexpr int ES = DT == MM_F32 ? 4 : 2;
  fp8_quantize_row<DT>((const char*)x + row * (int64_t)E * ES, E, l, codes + row * (int64_t)E, scales + row);
}

// ---------------------------------------------------------------------------------------------
// Streaming MaxSim over the quantised store (the ring slot and its LDS-DMA: fp8_device.h).
// ---------------------------------------------------------------------------------------------

// NSL = E / 128 slices per ROWS-token block (one ring slot each; the accumulators run across the slices); NQT = query
// tiles of 32 tokens held as MFMA B fragments (Q <= 32 * NQT).
template <int DT, int NSL, int NQT, int ROWS>
__global__ void __launch_bounds__(64) maxsim_fp8_stream_kernel(const Fp8Args a) {
  using S = Fp8Slot<ROWS>;
  constexpr int NBUF = S::kNbuf;
  constexpr int MT = ROWS / 32;  // 32-row MFMA tiles per block
  constexpr int RB = NSL * 128;  // bytes per token row
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x;
  const int r = lane & 31, h = lane >> 5;
  const int64_t p0 = (int64_t)blockIdx.x * a.pairs_per_wave;
  const int64_t p1 = (p0 + a.pairs_per_wave < a.n_pairs) ? p0 + a.pairs_per_wave : a.n_pairs;
  if (p0 >= p1) return;
  const int64_t ppq = a.ppq;
  const int Q = a.Q;
  const uint32_t lds0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)smem;

  // per-lane source offsets of the code instructions of a slot
  uint32_t voff[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int row = 8 * k + (lane >> 3);
    const int c = (lane & 7) ^ ((row >> 1) & 7);
    voff[k] = (uint32_t)(row * RB + c * 16);
  }
  // per-lane LDS offsets of the 8 A-fragment reads of a 32-row tile (the second tile is 4 KiB further; 32 rows do not
  // change (R >> 1) & 7): half h of chunk kk of row r lives at slot kk ^ ((r >> 1) & 7)
  uint32_t lo[8];
#pragma unroll
  for (int kk = 0; kk < 8; ++kk) lo[kk] = (uint32_t)(r * 128 + ((kk ^ ((r >> 1) & 7)) << 4) + 8 * h);

  auto doc_len = [&](int64_t p) -> int {
    const int64_t l = sload_i64(a.end, p) - sload_i64(a.begin, p);
    return l < 0 ? 0 : (l > 0x7fffffc0LL ? 0x7fffffc0 : (int)l);
  };

  // ---- producer cursor: next (pair, block, slice) to put in flight ---------------------------
  int64_t pp = p0;
  int pt = 0, pn = 0, psl = 0, plen = 0;
  while (pp < p1 && (pn = ((plen = doc_len(pp)) + ROWS - 1) / ROWS) == 0) ++pp;   // empty documents stream nothing
  int pbuf = 0, cbuf = 0, inflight = 0;

  auto top_up = [&]() {
    while (pp < p1 && inflight < NBUF) {
      const int64_t row0 = sload_i64(a.begin, pp) + (int64_t)pt * ROWS;
      const uint8_t* g = a.codes + row0 * RB + psl * 128;
      const float* gs = a.scales + row0;
      const uint32_t dst = lds0 + (uint32_t)pbuf * S::kBytes;
      // rows past this document's end are redirected to its last row (codes and scale alike): the last document never
      // reads past `codes` / `scales`
      const int rl = plen - ROWS * pt;  // rows of this block that exist (>= 1)
      if (rl < ROWS) {
        uint32_t vt[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const int over = 8 * k + (lane >> 3) - (rl - 1);
          vt[k] = voff[k] - (uint32_t)((over > 0 ? over : 0) * RB);
        }
        issue_slot<ROWS>(g, vt, gs, (uint32_t)((lane < rl ? lane : rl - 1) * 4), dst);
      } else {
        issue_slot<ROWS>(g, voff, gs, (uint32_t)((lane < ROWS ? lane : ROWS - 1) * 4), dst);
      }
      pbuf = (pbuf + 1 == NBUF) ? 0 : pbuf + 1;
      ++inflight;
      if (NSL > 1 && ++psl < NSL) continue;
      psl = 0;
      if (++pt >= pn) {
        pt = 0;
        ++pp;
        while (pp < p1 && (pn = ((plen = doc_len(pp)) + ROWS - 1) / ROWS) == 0) ++pp;
      }
    }
  };
  top_up();

  // ---- query tile(s) as MFMA B fragments (16-bit, exactly as the 16-bit kernel holds them) -----
  short8 qf[NQT][NSL][8];
  bool qvalid[NQT];
#pragma unroll
  for (int n = 0; n < NQT; ++n) qvalid[n] = false;
  int64_t cur_q = -1;
  int64_t qi = p0 / ppq;
  int64_t q_left = ppq - (p0 - qi * ppq);  // pairs left on this query
  const int qwords = (Q + 31) >> 5;

  for (int64_t pair = p0; pair < p1; ++pair) {
    if (q_left == 0) {
      ++qi;
      q_left = ppq;
    }
    --q_left;
    if (qi != cur_q) {
      cur_q = qi;
      const int qlen = a.qm.len ? (int)sload_u32(a.qm.len, qi) : Q;
#pragma unroll
      for (int n = 0; n < NQT; ++n) {
        const int qt = 32 * n + r;
        const int qr = qt < Q ? qt : Q - 1;
        const char* qrow = (const char*)a.q + (qi * Q + qr) * (int64_t)(2 * RB);
#pragma unroll
        for (int sl = 0; sl < NSL; ++sl) {
          // two tiles at dim >= 512 exceed the 256 VGPRs: the second tile lives in AGPRs (maxsim.hip)
          if (NQT == 2 && NSL >= 4 && n == 1) load_q_frags_agpr(qrow + sl * 256 + h * 16, qf[n][sl]);
          else load_q_frags(qrow + sl * 256 + h * 16, qf[n][sl]);
        }
        qvalid[n] = qt < Q && qt < qlen;
        if (a.qm.bits && n < qwords) qvalid[n] = qvalid[n] && ((sload_u32(a.qm.bits, qi * qwords + n) >> r) & 1u);
      }
    }
    const int len = doc_len(pair);
    const int nb = (len + ROWS - 1) / ROWS;
    // every stored row is a real token; an empty document scores like a fully padded one
    const float fill = len == 0 ? -1000.0f : neg_inf();
    float m1[NQT];
#pragma unroll
    for (int n = 0; n < NQT; ++n) m1[n] = fill;

    for (int t = 0; t < nb; ++t) {
      const int rem = len - ROWS * t;
      const bool two = MT == 2 && rem > 32;          // wave-uniform: the block's second 32 rows hold a token
      f32x16 acc[NQT][MT];
#pragma unroll
      for (int n = 0; n < NQT; ++n)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) acc[n][mt] = f32x16{0};
      const char* sbuf = smem;
#pragma unroll
      for (int sl = 0; sl < NSL; ++sl) {
        top_up();
        wait_slot<S::kVm>(inflight - 1);
        const char* buf = smem + cbuf * S::kBytes;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
          if (mt == 1 && !two) break;
#pragma unroll
          for (int kk = 0; kk < 8; ++kk) {
            const short8 av = cvt8<DT>(*(const u32x2*)(buf + mt * 4096 + lo[kk]));
#pragma unroll
            for (int n = 0; n < NQT; ++n) acc[n][mt] = Mfma32x16<DT>::run(av, qf[n][sl][kk], acc[n][mt]);
          }
        }
        sbuf = buf + S::kCodes;           // every slice carries the block's scales; the last one is read below
        cbuf = (cbuf + 1 == NBUF) ? 0 : cbuf + 1;
        --inflight;
      }
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        if (mt == 1 && !two) break;
        const int rm = rem - 32 * mt;
        const uint32_t ex = rm >= 32 ? 0xffffffffu : ((1u << rm) - 1u);
        // accumulator register i of lane half h is row (i & 3) + 8 (i >> 2) + 4 h of its 32-row tile: four 16-byte reads
        // (one address per lane half: broadcast) fetch its 16 scales.  The slot is not refilled before the next top_up().
        f32x4 sc[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) sc[g] = *(const f32x4*)(sbuf + (32 * mt + 8 * g + 4 * h) * 4);
#pragma unroll
        for (int n = 0; n < NQT; ++n) {
          f32x16 s;
#pragma unroll
          for (int i = 0; i < 16; ++i) s[i] = acc[n][mt][i] * sc[i >> 2][i & 3];   // exact: a power of two
          block_max1(m1[n], s, ex, ex, fill, h);
        }
      }
    }
    float s = 0.0f;
#pragma unroll
    for (int n = 0; n < NQT; ++n) s += finish_pair1<DT>(m1[n], qvalid[n], h, a.rnd);  // tiles in index order: deterministic
    if (lane == 0) a.out[pair] = finish_sum<DT>(s, a.rnd);
  }
}

// ---------------------------------------------------------------------------------------------
// Plain path: any E % 16 == 0, any Q.  One wavefront per pair, fragment-shaped direct loads (8 bytes of codes and
// 16 bytes of query per lane and K step), query tiles of 32 tokens looped in order.  Not tuned.
// ---------------------------------------------------------------------------------------------
template <int DT>
__global__ void __launch_bounds__(64) maxsim_fp8_plain_kernel(const Fp8Args a) {
  const int lane = threadIdx.x;
  const int r = lane & 31, h = lane >> 5;
  const int64_t pair = blockIdx.x;
  if (pair >= a.n_pairs) return;
  const int Q = a.Q, E = a.E;
  const int64_t qi = pair / a.ppq;
  const int64_t drow0 = a.begin[pair];
  const int64_t l = a.end[pair] - drow0;
  const int len = l < 0 ? 0 : (l > 0x7fffffc0LL ? 0x7fffffc0 : (int)l);
  const int nb = (len + 31) >> 5;
  const int qwords = (Q + 31) >> 5;
  const float fill = len == 0 ? -1000.0f : neg_inf();
  const int qlen = a.qm.len ? a.qm.len[qi] : Q;
  const uint8_t* dbase = a.codes + drow0 * E;
  const char* qbase = (const char*)a.q + qi * Q * (int64_t)E * 2;
  const int nch = E >> 4;

  float total = 0.0f;
  for (int n = 0; n < qwords; ++n) {
    const int qtok = 32 * n + r;
    const int qr = qtok < Q ? qtok : Q - 1;
    bool qvalid = qtok < Q && qtok < qlen;
    if (a.qm.bits) qvalid = qvalid && ((a.qm.bits[qi * qwords + n] >> r) & 1u);
    const char* qrow = qbase + (int64_t)qr * E * 2;
    float m = fill;
    for (int t = 0; t < nb; ++t) {
      const int drow = 32 * t + r;
      const uint8_t* dr = dbase + (int64_t)(drow < len ? drow : len - 1) * E;
      f32x16 acc = {0};
      for (int c = 0; c < nch; ++c) {
        const short8 av = cvt8<DT>(*(const u32x2*)(dr + c * 16 + 8 * h));
        const short8 bv = *(const short8*)(qrow + c * 32 + 16 * h);
        acc = Mfma32x16<DT>::run(av, bv, acc);
      }
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int row = 32 * t + rowof(i) + 4 * h;
        acc[i] *= a.scales[drow0 + (row < len ? row : len - 1)];
      }
      const int rem = len - 32 * t;
      const uint32_t ex = rem >= 32 ? 0xffffffffu : ((1u << rem) - 1u);
      block_max1(m, acc, ex, ex, fill, h);
    }
    total += finish_pair1<DT>(m, qvalid, h, a.rnd);
  }
  if (lane == 0) a.out[pair] = finish_sum<DT>(total, a.rnd);
}

// ---------------------------------------------------------------------------------------------
template <int DT, int NSL>
static int launch_fp8_stream(const Fp8Args& a0, hipStream_t stream) {
  Fp8Args a = a0;
  constexpr int lds = Fp8Slot<64>::kNbuf * Fp8Slot<64>::kBytes;   // (the 32-row ring is 4 x 4.25 KiB: no larger)
  static_assert(Fp8Slot<32>::kNbuf * Fp8Slot<32>::kBytes <= lds + 512, "ring sizes");
  int wpc = env().maxsim_wpc > 0 ? env().maxsim_wpc : 4;
  if (wpc > 8) wpc = 8;
  const unsigned waves = split_pairs(a, (int64_t)kCUs * wpc);
  if (a.Q > 32) {
    constexpr int ROWS = NSL >= 6 ? 32 : 64;
    hipLaunchKernelGGL((maxsim_fp8_stream_kernel<DT, NSL, 2, ROWS>), dim3(waves), dim3(64),
                       Fp8Slot<ROWS>::kNbuf * Fp8Slot<ROWS>::kBytes, stream, a);
  } else {
    hipLaunchKernelGGL((maxsim_fp8_stream_kernel<DT, NSL, 1, 64>), dim3(waves), dim3(64), lds, stream, a);
  }
  return check_launch("maxsim_fp8_stream_kernel");
}

template <int DT>
static int launch_fp8(const Fp8Args& a, bool stream_ok, hipStream_t stream) {
  if (stream_ok) return with_nsl(a.E, [&](auto nsl) { return launch_fp8_stream<DT, MM_V(nsl)>(a, stream); });
  if (a.n_pairs > 0x7fffffffLL) return set_error(MM_EUNSUPPORTED, "maxsim_ragged_fp8: more than 2^31-1 pairs in one plain launch");
  hipLaunchKernelGGL(maxsim_fp8_plain_kernel<DT>, dim3((unsigned)a.n_pairs), dim3(64), 0, stream, a);
  return check_launch("maxsim_fp8_plain_kernel");
}

}  // namespace mm

using namespace mm;

extern "C" int mm_fp8_quantize_rows(const void* x, int64_t n_rows, int E, int dtype, uint8_t* codes, float* scales,
                                    void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (n_rows < 0 || E <= 0) return set_error(MM_EINVAL, "fp8_quantize_rows: bad shape");
  if (dtype != MM_F32 && dtype != MM_F16 && dtype != MM_BF16) return set_error(MM_EINVAL, "fp8_quantize_rows: bad dtype %d", dtype);
  if (E % 16) return set_error(MM_EUNSUPPORTED, "fp8_quantize_rows: E=%d is not a multiple of 16", E);
  if (n_rows == 0) return MM_OK;
  if (!x || !codes || !scales) return set_error(MM_EINVAL, "fp8_quantize_rows: null tensor pointer");
  if ((((uintptr_t)x | (uintptr_t)codes) & 15) || ((uintptr_t)scales & 3))
    return set_error(MM_EINVAL, "fp8_quantize_rows: x / codes must be 16-byte aligned, scales 4-byte aligned");
  const int64_t blocks = (n_rows + 15) / 16;
  if (blocks > 0x7fffffffLL) return set_error(MM_EUNSUPPORTED, "fp8_quantize_rows: more than 2^35 - 16 rows in one launch");
  const dim3 grid((unsigned)blocks), block(256);
  if (dtype == MM_F32) hipLaunchKernelGGL(fp8_quantize_rows_kernel<MM_F32>, grid, block, 0, stream, x, n_rows, E, codes, scales);
  else if (dtype == MM_F16) hipLaunchKernelGGL(fp8_quantize_rows_kernel<MM_F16>, grid, block, 0, stream, x, n_rows, E, codes, scales);
  else hipLaunchKernelGGL(fp8_quantize_rows_kernel<MM_BF16>, grid, block, 0, stream, x, n_rows, E, codes, scales);
  return check_launch("fp8_quantize_rows_kernel");
}

extern "C" size_t mm_maxsim_ragged_fp8_workspace_bytes(int64_t n_pairs, int64_t pairs_per_query, int Q, int q_mask_kind) {
  if (pairs_per_query <= 0) pairs_per_query = 1;
  return packed_mask_bytes(q_mask_kind, (n_pairs + pairs_per_query - 1) / pairs_per_query, Q);
}

extern "C" int mm_maxsim_ragged_fp8_fwd(const void* q, const uint8_t* codes, const float* scales, const int64_t* doc_begin,
                                        const int64_t* doc_end, const void* q_mask, int q_mask_kind, float* out,
                                        int64_t n_pairs, int64_t pairs_per_query, int Q, int E, int q_dtype, int flags,
                                        void* workspace, size_t workspace_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!q || !codes || !scales || !out) return set_error(MM_EINVAL, "maxsim_ragged_fp8: null tensor pointer");
  if (n_pairs < 0 || Q <= 0 || E <= 0) return set_error(MM_EINVAL, "maxsim_ragged_fp8: non-positive shape");
  if (q_dtype == MM_F32)
    return set_error(MM_EUNSUPPORTED, "maxsim_ragged_fp8: the query is fp16 or bf16 (an fp32 query has no exact 16-bit MFMA operand)");
  if (q_dtype != MM_F16 && q_dtype != MM_BF16) return set_error(MM_EINVAL, "maxsim_ragged_fp8: bad dtype %d", q_dtype);
  if (E % 16) return set_error(MM_EUNSUPPORTED, "maxsim_ragged_fp8: E=%d is not a multiple of 16", E);
  if ((((uintptr_t)q | (uintptr_t)codes) & 15) || ((uintptr_t)scales & 3))
    return set_error(MM_EINVAL, "maxsim_ragged_fp8: q / codes must be 16-byte aligned, scales 4-byte aligned");
  if (flags & ~(MM_SIM_ROUND | MM_SUM_ROUND)) return set_error(MM_EINVAL, "maxsim_ragged_fp8: unknown flags 0x%x", flags);
  if (!doc_begin || !doc_end) return set_error(MM_EINVAL, "maxsim_ragged_fp8: null document range pointer");
  if (pairs_per_query <= 0) return set_error(MM_EINVAL, "maxsim_ragged_fp8: pairs_per_query must be >= 1");
  if (n_pairs == 0) return MM_OK;
  const int64_t nq = (n_pairs + pairs_per_query - 1) / pairs_per_query;
  Fp8Args a{};
  a.q = q; a.codes = codes; a.scales = scales; a.out = out; a.n_pairs = n_pairs; a.ppq = pairs_per_query;
  a.begin = doc_begin; a.end = doc_end; a.Q = Q; a.E = E; a.rnd = flags;
  WsCursor ws(workspace, workspace_bytes);
  if (int e = resolve_mask(q_mask, q_mask_kind, nq, Q, ws, stream, &a.qm)) return e;
  const bool stream_ok = !env().maxsim_generic && Q <= 64 && stream_width(E);
  return with_dtype16(q_dtype, [&](auto dt) { return launch_fp8<MM_V(dt)>(a, stream_ok, stream); });
}
