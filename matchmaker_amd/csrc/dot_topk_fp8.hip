// Brute-force inner-product top-k over an fp8 token store for MI355X (gfx950 / CDNA4): mm_dot_topk_fwd (dot_topk.hip; the
// flat index of matchmaker/retrieval/faiss_indices.py:22-36, called from matchmaker/dense_retrieval.py:391) with the corpus
// given as codes [n_rows, E] uint8 (OCP e4m3fn) + scales [n_rows] float32, the format of mm_fp8_quantize_rows:
//
//   score[q, t] = scales[t] * sum_k queries[q, k] * deq(codes[t, k])
//
// The query is fp16 / bf16 and is NOT quantised: the codes are converted to its type in registers (cvt8, exact), multiplied
// on v_mfma_f32_32x32x16_{f16,bf16} (exact products, fp32 sum) and the power-of-two scale multiplies the finished fp32 dot
// product (exact) before the threshold test and before anything is filed.
//
// The three phases, the workspace, the threshold rule, the tie rule and status are dot_topk.hip's (the host helpers of
// mm_internal.h: one copy); only the streaming kernel between them is this file's:
//
// dot_fp8_stream_kernel: ONE wavefront per workgroup.  It keeps 32 * NQT queries as MFMA B fragments for its whole life
// (documents on the M axis, queries on N: a lane owns one query per tile and the threshold test is a lane-local compare)
// and streams its slice of the rows through a wavefront-PRIVATE LDS-DMA ring of four slots of 32 rows x one 128-code slice
// (4 KiB) plus the rows' scales as one more global_load_lds_dword — the document side of maxsim_fp8_stream_kernel
// (fp8_device.h): source-side chunk swizzle, ds_read_b64 + four converts per A fragment, the 16 scales a lane needs from
// broadcast LDS reads.  Work map: the 32-row blocks are split 8 ways by XCD (blockIdx % 8); inside an XCD the workgroups are
// (query group, sub-slice), so the wavefronts of one XCD sweep the same rows for different query groups at about the same
// time and re-read them from that XCD's L2.
// Where this leaves dot_stream_kernel's plan (four wavefronts sharing one ring, a barrier per block): at one byte per
// element a wavefront's private ring moves half the bytes of the 16-bit one, no barrier couples the wavefronts, and where
// the registers allow two wavefronts per SIMD (one query tile up to dim 512, two tiles at dim 128) they hide each other's
// LDS and filing latency, which the one-wavefront-per-SIMD kernel has to do by hand.  The price is paid where only one
// wavefront fits and in the L2 re-reads of 64-query groups (what was and was not measured).
// Survivors are staged in LDS (positions from the ballot of the compare, fill level in a scalar register) and flushed with
// one returning atomic per entry when the area runs full, as dot_stream_kernel's flush_wave does.
#include "mm_internal.h"
#include "maxsim_device.h"
#include "fp8_device.h"

namespace mm {

enum { DOTF_SAMPLE = 0, DOTF_FILTER = 1 };
constexpr int kFp8Stage = 128;   // staged survivors per wavefront (score, row, query: 12 bytes each)

struct DotFp8Args {
  const void* q;        // [nq, E] fp16 / bf16
  const uint8_t* codes; // [n_rows, E]
  const float* scales;  // [n_rows]
  int64_t ndocs;        // rows visited by this launch: row(i) = i * stride, i < ndocs
  int64_t stride;       // 1 = every row, > 1 = strided sample
  int nq, G, T;         // query groups of 32 * NQT, sub-slices per XCD (grid = 8 * G * T)
  // SAMPLE
  float* all_out;       // [nq, ld_all] scores of the visited rows
  int64_t ld_all;
  // FILTER
  const float* tau;     // [nq]
  int32_t* count;       // [nq] survivors (may exceed cap: overflow)
  float* cand_score;    // [nq, cap]
  int32_t* cand_idx;    // [nq, cap] row of the store
  int cap;
};

// NSL = E / 128 slices per 32-row block (one ring slot each; the accumulators run across the slices in slice order, K steps
// in order: SAMPLE and FILTER give the same bits for one (query, row) pair); NQT = query tiles of 32.
template <int DT, int NSL, int NQT, int MODE>
__global__ void __launch_bounds__(64) dot_fp8_stream_kernel(const DotFp8Args a) {
  using S = Fp8Slot<32>;
  constexpr int NBUF = S::kNbuf;
  constexpr int RB = NSL * 128;  // bytes per row of codes
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x;
  const int r = lane & 31, h = lane >> 5;
  const uint32_t lds0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)smem;

  // ---- work map ---------------------------------------------------------------------------------
  const int xcd = blockIdx.x & 7;
  const int j = blockIdx.x >> 3;
  const int g = j % a.G, t = j / a.G;
  const int64_t nblk = (a.ndocs + 31) >> 5;
  const int64_t x_lo = nblk * xcd / 8, x_hi = nblk * (xcd + 1) / 8;
  const int64_t b_lo = x_lo + (x_hi - x_lo) * t / a.T, b_hi = x_lo + (x_hi - x_lo) * (t + 1) / a.T;
  if (b_lo >= b_hi) return;
  const int q0 = g * (32 * NQT);

  // survivor staging (FILTER): three arrays behind the ring
  float* st_s = (float*)(smem + NBUF * S::kBytes);
  int* st_d = (int*)(st_s + kFp8Stage);
  int* st_q = st_d + kFp8Stage;
  int scnt = 0;  // wave-uniform fill level
  auto flush_wave = [&]() {
    for (int i = lane; i < scnt; i += 64) {
      const int qq = st_q[i];
      if (qq >= a.nq) continue;   // (a query past the end has tau = +inf: only an infinite score gets here)
      const int slot = atomicAdd(a.count + qq, 1);
      if ((unsigned)slot < (unsigned)a.cap) {
        a.cand_score[(int64_t)qq * a.cap + slot] = st_s[i];
        a.cand_idx[(int64_t)qq * a.cap + slot] = st_d[i];
      }
    }
    scnt = 0;
  };

  // ---- LDS-DMA: per-lane source offsets of the four code instructions of a slot and of its scale instruction ------
  const int64_t rowstep = a.stride * RB;   // bytes between consecutive visited rows (the host keeps 31 * rowstep below 2^32)
  uint32_t voff[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int row = 8 * (k & 3) + (lane >> 3);
    const int c = (lane & 7) ^ ((row >> 1) & 7);
    voff[k] = (uint32_t)(row * rowstep) + (uint32_t)(c * 16);
  }
  const uint32_t soff = (uint32_t)((lane < 32 ? lane : 31) * a.stride * 4);
  // per-lane LDS offsets of the 8 A-fragment reads: half h of chunk kk of row r lives at slot kk ^ ((r >> 1) & 7)
  uint32_t lo[8];
#pragma unroll
  for (int kk = 0; kk < 8; ++kk) lo[kk] = (uint32_t)(r * 128 + ((kk ^ ((r >> 1) & 7)) << 4) + 8 * h);

  // ---- producer cursor: next (block, slice) to put in flight -------------------------------------
  int64_t pb = b_lo;
  int psl = 0, pbuf = 0, cbuf = 0, inflight = 0;
  auto top_up = [&]() {
    while (pb < b_hi && inflight < NBUF) {
      const int64_t row0 = pb * 32 * a.stride;
      const uint8_t* gb = a.codes + row0 * RB + psl * 128;
      const float* gs = a.scales + row0;
      const uint32_t dst = lds0 + (uint32_t)pbuf * S::kBytes;
      // rows past the end of the store's last block are redirected to the last visited row (codes and scale alike): no load
      // uses a row index >= n_rows; they are never filed (the epilogue's `rem`)
      const int64_t left = a.ndocs - pb * 32;   // visited rows of this block that exist (>= 1)
      if (left < 32) {
        const int rl = (int)left;
        uint32_t vt[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          int row = 8 * (k & 3) + (lane >> 3);
          if (row >= rl) row = rl - 1;
          // (the swizzle follows the LDS row the chunk lands in, not the row it is read from)
          vt[k] = (uint32_t)(row * rowstep) + (voff[k] & 127u);
        }
        issue_slot<32>(gb, vt, gs, (uint32_t)((lane < rl ? lane : rl - 1) * a.stride * 4), dst);
      } else {
        issue_slot<32>(gb, voff, gs, soff, dst);
      }
      pbuf = (pbuf + 1 == NBUF) ? 0 : pbuf + 1;
      ++inflight;
      if (NSL > 1 && ++psl < NSL) continue;
      psl = 0;
      ++pb;
    }
  };
  top_up();

  // ---- this wavefront's queries as MFMA B fragments (16-bit, exactly as maxsim_fp8_stream_kernel holds them) ----------
  short8 qf[NQT][NSL][8];
  int qid[NQT];
  float tau[NQT];
#pragma unroll
  for (int n = 0; n < NQT; ++n) {
    const int qq = q0 + 32 * n + r;
    qid[n] = qq < a.nq ? qq : -1;
    tau[n] = (MODE == DOTF_FILTER && qid[n] >= 0) ? a.tau[qid[n]] : __builtin_huge_valf();
    const char* qrow = (const char*)a.q + (int64_t)(qq < a.nq ? qq : a.nq - 1) * (2 * RB) + h * 16;
#pragma unroll
    for (int sl = 0; sl < NSL; ++sl) {
      // two tiles at dim >= 512 exceed the 256 VGPRs: the second tile lives in AGPRs (maxsim.hip)
      if (NQT == 2 && NSL >= 4 && n == 1) load_q_frags_agpr(qrow + sl * 256, qf[n][sl]);
      else load_q_frags(qrow + sl * 256, qf[n][sl]);
    }
  }
  // the thresholds are in their registers HERE (the fragment loads end in vmcnt(0)): no compiler wait inside the block loop
#pragma unroll
  for (int n = 0; n < NQT; ++n) asm volatile("" : "+v"(tau[n]));

  for (int64_t b = b_lo; b < b_hi; ++b) {
    f32x16 acc[NQT];
#pragma unroll
    for (int n = 0; n < NQT; ++n) acc[n] = f32x16{0};
    const char* sbuf = smem;
#pragma unroll
    for (int sl = 0; sl < NSL; ++sl) {
      top_up();
      wait_slot<S::kVm>(inflight - 1);
      const char* buf = smem + cbuf * S::kBytes;
#pragma unroll
      for (int kk = 0; kk < 8; ++kk) {
        const short8 av = cvt8<DT>(*(const u32x2*)(buf + lo[kk]));
#pragma unroll
        for (int n = 0; n < NQT; ++n) acc[n] = Mfma32x16<DT>::run(av, qf[n][sl][kk], acc[n]);
      }
      sbuf = buf + S::kCodes;           // every slice carries the block's scales; the last one is read below
      cbuf = (cbuf + 1 == NBUF) ? 0 : cbuf + 1;
      --inflight;
    }
    // accumulator register i of lane half h is row (i & 3) + 8 (i >> 2) + 4 h of the block: four 16-byte reads (one address
    // per lane half: broadcast) fetch its 16 scales.  The slot is not refilled before the next top_up().
    f32x4 sc[4];
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4) sc[g4] = *(const f32x4*)(sbuf + (8 * g4 + 4 * h) * 4);
    const int64_t d0 = b * 32 + 4 * h;                 // visited index of this lane's accumulator register 0
    const int64_t left = a.ndocs - b * 32;
    const int rem = left < 32 ? (int)left : 32;        // rows of this block that exist
#pragma unroll
    for (int n = 0; n < NQT; ++n) {
      float s[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) s[i] = acc[n][i] * sc[i >> 2][i & 3];   // exact: a power of two
      if constexpr (MODE == DOTF_SAMPLE) {
        if (qid[n] < 0) continue;
        float* dst = a.all_out + (int64_t)qid[n] * a.ld_all + d0;
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {   // rows 8 g4 .. 8 g4 + 3 (+ 4h) are consecutive visited rows
          if (8 * g4 + 4 * h + 3 < rem) {
            *(f32x4*)(dst + 8 * g4) = f32x4{s[4 * g4], s[4 * g4 + 1], s[4 * g4 + 2], s[4 * g4 + 3]};
          } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
              if (8 * g4 + 4 * h + e < rem) dst[8 * g4 + e] = s[4 * g4 + e];
          }
        }
      } else {
        // every element: the lanes whose score passes take consecutive staging slots (ballot + mbcnt); the branch is
        // wave-uniform and rare (~2.5 k survivors per query in the whole store)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int row = rowof(i) + 4 * h;
          const bool pass = s[i] >= tau[n] && row < rem;
          const unsigned long long bal = __builtin_amdgcn_ballot_w64(pass);
          if (bal != 0) {
            const int cnt = __builtin_popcountll(bal);
            if (scnt + cnt > kFp8Stage) flush_wave();
            if (pass) {
              const int pos = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, (uint32_t)scnt));
              st_s[pos] = s[i];
              st_d[pos] = (int)(b * 32 + row);      // FILTER visits every row: stride 1
              st_q[pos] = q0 + 32 * n + r;
            }
            scnt += cnt;
          }
        }
      }
    }
  }
  if (MODE == DOTF_FILTER) flush_wave();
}

// Launch geometry: G query groups of 32 * NQT, T sub-slices per XCD so that the launch is about one full round of the device
// at the instantiation's occupancy (DESIGN §3.18's resource table) and a wavefront keeps >= 4 blocks (the query tile load is
// a prologue).
struct DotFp8Geom {
  int nqt, G, T;
};
static DotFp8Geom dot_fp8_geom(int64_t n_docs, int nq, int E) {
  const int nsl = E / 128;
  DotFp8Geom g;
  g.nqt = nq > 32 ? 2 : 1;
  g.G = (nq + 32 * g.nqt - 1) / (32 * g.nqt);
  // wavefronts per SIMD: one where the registers allow no more, else two (the ring + staging, 18.5 KiB per wavefront, fit
  // eight times into a CU's 160 KiB of LDS)
  const int occ = g.nqt == 2 ? (nsl >= 2 ? 1 : 2) : (nsl >= 6 ? 1 : 2);
  const int64_t per_xcd = ((n_docs + 31) / 32 + 7) / 8;
  int64_t T = (kCUs * 4 * occ / 8 + g.G - 1) / g.G;   // 8 * G * T ~ one full round of the device
  if (T > per_xcd / 4) T = per_xcd / 4;
  if (T < 1) T = 1;
  g.T = (int)T;
  return g;
}

template <int DT, int NSL, int NQT, int MODE>
static int launch_dot_fp8(const DotFp8Args& a0, const DotFp8Geom& g, hipStream_t stream) {
  DotFp8Args a = a0;
  a.G = g.G;
  a.T = g.T;
  if (31.0 * (double)a.stride * (NSL * 128) >= 4294967296.0)
    return set_error(MM_EUNSUPPORTED, "dot_topk_fp8: sample stride too large for 32-bit row offsets");
  const int64_t grid = 8LL * a.G * a.T;
  if (grid > 0x7fffffffLL) return set_error(MM_EUNSUPPORTED, "dot_topk_fp8: too many queries for one launch");
  constexpr int lds = Fp8Slot<32>::kNbuf * Fp8Slot<32>::kBytes + kFp8Stage * 12;
  hipLaunchKernelGGL((dot_fp8_stream_kernel<DT, NSL, NQT, MODE>), dim3((unsigned)grid), dim3(64), lds, stream, a);
  return check_launch("dot_fp8_stream_kernel");
}

template <int DT, int MODE>
static int launch_dot_fp8_e(const DotFp8Args& a, int E, const DotFp8Geom& g, hipStream_t stream) {
  return with_nsl(E, [&](auto nsl) {
    return g.nqt == 2 ? launch_dot_fp8<DT, MM_V(nsl), 2, MODE>(a, g, stream) : launch_dot_fp8<DT, MM_V(nsl), 1, MODE>(a, g, stream);
  });
}

}  // namespace mm

using namespace mm;

extern "C" size_t mm_dot_topk_fp8_workspace_bytes(int64_t n_rows, int nq, int k) { return dot_sel_bytes(n_rows, nq, k); }

extern "C" int mm_dot_topk_fp8_fwd(const void* queries, const uint8_t* codes, const float* scales, int64_t n_rows, int nq, int E,
                                   int q_dtype, int k, float m_scale, float* out_scores, int64_t* out_idx, int32_t* status,
                                   void* workspace, size_t workspace_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!queries || !codes || !scales || !out_scores || !out_idx || !status) return set_error(MM_EINVAL, "dot_topk_fp8: null pointer");
  if (n_rows <= 0 || nq <= 0 || E <= 0 || k <= 0) return set_error(MM_EINVAL, "dot_topk_fp8: non-positive shape");
  if (q_dtype == MM_F32)
    return set_error(MM_EUNSUPPORTED, "dot_topk_fp8: the query is fp16 or bf16 (an fp32 query has no exact 16-bit MFMA operand)");
  if (q_dtype != MM_F16 && q_dtype != MM_BF16) return set_error(MM_EINVAL, "dot_topk_fp8: bad dtype %d", q_dtype);
  if (!stream_width(E))
    return set_error(MM_EUNSUPPORTED, "dot_topk_fp8: E=%d (supported: 128, 256, 384, 512, 768; pad the vectors)", E);
  if (n_rows >= (1LL << 31)) return set_error(MM_EUNSUPPORTED, "dot_topk_fp8: more than 2^31-1 rows in one call");
  if (k > 4096) return set_error(MM_EUNSUPPORTED, "dot_topk_fp8: k=%d exceeds the candidate sorter (k <= 4096)", k);
  if ((((uintptr_t)queries | (uintptr_t)codes) & 15) || ((uintptr_t)scales & 3))
    return set_error(MM_EINVAL, "dot_topk_fp8: queries / codes must be 16-byte aligned, scales 4-byte aligned");
  const size_t need = dot_sel_bytes(n_rows, nq, k);
  if (!workspace || workspace_bytes < need) return set_error(MM_EWORKSPACE, "dot_topk_fp8: workspace needs %zu bytes", need);
  if (!(m_scale > 0.0f)) m_scale = 1.0f;

  WsCursor ws(workspace, workspace_bytes);
  const DotSel sel = dot_sel_carve(ws, n_rows, nq, k);
  const bool small = n_rows <= 4096;  // everything is a candidate: no sampling
  DotFp8Args a{};
  a.q = queries; a.codes = codes; a.scales = scales; a.nq = nq;
  a.tau = sel.tau; a.count = sel.count; a.cand_score = sel.cand_score; a.cand_idx = sel.cand_idx; a.cap = sel.cap;

  // phase 1: threshold per query
  if (small) {
    launch_fill_tau(sel, nq, -__builtin_huge_valf(), stream);
  } else {
    a.ndocs = sel.S; a.stride = n_rows / sel.S; a.all_out = sel.all; a.ld_all = sel.S;
    const DotFp8Geom gs = dot_fp8_geom(sel.S, nq, E);
    const int e = with_dtype16(q_dtype, [&](auto dt) { return launch_dot_fp8_e<MM_V(dt), DOTF_SAMPLE>(a, E, gs, stream); });
    if (e) return e;
    launch_sample_tau(sel, nq, dot_sample_m(n_rows, sel.S, k, m_scale), stream);
  }
  if (int e = check_launch("dot_topk_fp8 threshold")) return e;

  // phase 2: full product + threshold filter
  if (hipMemsetAsync(sel.count, 0, (size_t)nq * 4, stream) != hipSuccess) return set_error(MM_ELAUNCH, "dot_topk_fp8: memset failed");
  a.ndocs = n_rows; a.stride = 1;
  {
    const DotFp8Geom g = dot_fp8_geom(n_rows, nq, E);
    const int e = with_dtype16(q_dtype, [&](auto dt) { return launch_dot_fp8_e<MM_V(dt), DOTF_FILTER>(a, E, g, stream); });
    if (e) return e;
  }
  // phase 3: exact top-k of the survivors
  return launch_topk_rows(sel, nq, k, n_rows, out_scores, out_idx, status, stream);
}
