// Backward of the all-pairs ColBERT MaxSim (in-batch negatives) for MI355X (gfx950 / CDNA4).
//
//   out[i, j] = sum_{t < Q, qmask[i, t]}  max_{p < D} ( dmask[m, p] ? <q[i, t], d[j, p]> : -1000 )        m = j  (m = i: bug-compatible)
//
// Reference semantics: autograd through matchmaker/models/colbert.py:154-162 (the [Bq, Bd] score matrix of in-batch-negative
// training; train.py:434-467 builds it, loss.backward() at train.py:503-524 differentiates it).  With
//   j*(i, j, t) = the FIRST arg-max over the document positions p < D of the masked similarities (torch.max's tie rule)
// nothing flows for a padded query token (:160) or when the arg-max is a masked position (the -1000 of :158 is a constant), and
//   grad_q[i, t, :] = sum_j               grad_out[i, j] * d[j, j*(i, j, t), :]
//   grad_d[j, p, :] = sum_i sum_{t : j*(i, j, t) = p}  grad_out[i, j] * q[i, t, :]
//
// The arg-max rule is the paired backward's (mm_maxsim_bwd, maxsim.hip): it is taken on the RECOMPUTED similarities, accumulated
// in fp32 by the MFMA, and ignores the forward's sim_round flag — rounding is monotone, so an arg-max of the fp32 similarities
// is also an arg-max of the rounded ones.
//
// Three launches on one stream, no atomics on floating-point data anywhere, every output byte written exactly once:
//   1. inb_argmax_kernel: one wavefront per (query, document) pair recomputes the 32 x 32 similarity tiles with the MFMA maps of
//      the forward's generic kernel (document tokens on M, query tokens on N) and writes j* as int16 [Bq, Bd, Q] (-1 = no gradient).
//   2. inb_gradq_kernel: one thread per 16-byte chunk of a grad_q row gathers the document rows in ascending j, fp32, one store.
//   3. inb_gradd_kernel: one workgroup per (document, column tile) keeps the [D, tile] fp32 accumulator in LDS and walks the
//      (query, token) entries of its document in ascending order; accumulator cell (p, column) belongs to ONE thread
//      (wavefront p & 3, lane = column), so the order of every sum is fixed.  The tile narrows until D * tile * 4 bytes fit.
// A null grad_q or grad_d is a gradient the caller does not need (a frozen encoder): launch 2 or 3 is left out.
// The result is a pure function of the inputs: two calls give the same bits.
#include "mm_internal.h"
#include "elem_device.h"

namespace mm {
namespace {

struct InbBwdArgs {
  const void* q;
  const void* d;
  PackedMask qm, dm;
  const float* go;
  void* gq;
  void* gd;
  int16_t* tab;      // [Bq, Bd, Q] first arg-max document position, -1 = no gradient
  int64_t Bq, Bd;
  int Q, D, E;
  int bug;           // mask pair (i, j) with the mask row of i (colbert.py:158)
  int et, ntile;     // grad_d: columns per workgroup, ceil(E / et)
};

constexpr int kEnt = 1024;   // (query, token) entries staged per round of inb_gradd_kernel

template <int DT>
__global__ void __launch_bounds__(256) inb_argmax_kernel(const InbBwdArgs a) {
  const int lane = threadIdx.x & 63;
  const int wv = threadIdx.x >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int64_t pair = (int64_t)blockIdx.x * 4 + wv;
  if (pair >= a.Bq * a.Bd) return;             // wave-uniform; the kernel has no barrier
  const int64_t qi = pair / a.Bd, dj = pair - qi * a.Bd;
  const int64_t mi = a.bug ? qi : dj;
  const int D = a.D, Q = a.Q, E = a.E;
  constexpr int ES = (DT == MM_F32) ? 4 : 2;
  const int64_t rowb = (int64_t)E * ES;
  const int words = (D + 31) >> 5, qwords = (Q + 31) >> 5;
  int len = a.dm.len ? a.dm.len[mi] : D;
  len = len < 0 ? 0 : (len > D ? D : len);
  const int nb = (len + 31) >> 5;
  const int qlen = a.qm.len ? a.qm.len[qi] : Q;
  const char* dbase = (const char*)a.d + dj * D * rowb;
  const char* qbase = (const char*)a.q + qi * Q * rowb;
  int16_t* trow = a.tab + pair * Q;

  for (int n = 0; n < qwords; ++n) {
    const int qtok = 32 * n + r;
    const int qr = qtok < Q ? qtok : Q - 1;
    bool qvalid = qtok < Q && qtok < qlen;
    if (a.qm.bits) qvalid = qvalid && ((a.qm.bits[qi * qwords + n] >> r) & 1u);
    // this lane's rows come in ascending position order (t, then i): a strict > keeps the first arg-max
    float best = neg_inf();
    int bpos = 0x7fffffff;
    for (int t = 0; t < nb; ++t) {
      const int drow = 32 * t + r;
      const int dr = drow < D ? drow : D - 1;
      const f32x16 acc = dot_block<DT>(dbase + dr * rowb, qbase + qr * rowb, E, h);
      const int rem = len - 32 * t, remd = D - 32 * t;
      const uint32_t ex = rem >= 32 ? 0xffffffffu : ((1u << rem) - 1u);
      const uint32_t ind = remd >= 32 ? 0xffffffffu : ((1u << remd) - 1u);    // rows that exist; the others take no part
      const uint32_t va = a.dm.bits ? (a.dm.bits[mi * words + t] & ex) : ex;
      const uint32_t vas = va >> (4 * h), ins = ind >> (4 * h);
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int bit = rowof(i);
        if ((ins >> bit) & 1u) {
          const float v = ((vas >> bit) & 1u) ? acc[i] : -1000.0f;
          if (v > best) { best = v; bpos = 32 * t + bit + 4 * h; }
        }
      }
    }
    // the padded tail behind the last block that was computed: all -1000, its first position stands for it
    if (32 * nb < D && -1000.0f > best) { best = -1000.0f; bpos = 32 * nb; }
    const float ob = __shfl_xor(best, 32, 64);
    const int op = __shfl_xor(bpos, 32, 64);
    if (ob > best || (ob == best && op < bpos)) { best = ob; bpos = op; }
    bool real = bpos < len;
    if (real && a.dm.bits) real = (a.dm.bits[mi * words + (bpos >> 5)] >> (bpos & 31)) & 1u;
    if (h == 0 && qtok < Q) trow[qtok] = (int16_t)((qvalid && real) ? bpos : -1);
  }
}

// grad_q[i, t, chunk] = sum_j grad_out[i, j] d[j, j*(i, j, t), chunk]: ascending j, fp32, stored once (zeros without a gradient)
template <int DT, int GT>
__global__ void __launch_bounds__(256) inb_gradq_kernel(const InbBwdArgs a) {
  constexpr int ES = (DT == MM_F32) ? 4 : 2;
  constexpr int PER = 16 / ES;
  const int Q = a.Q, D = a.D, E = a.E;
  const int nch = E / PER;
  const int64_t item = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (item >= a.Bq * Q * nch) return;
  const int64_t row = item / nch;
  const int c = (int)(item - row * nch);
  const int64_t qi = row / Q;
  const int t = (int)(row - qi * Q);
  const int64_t rowb = (int64_t)E * ES;
  const int16_t* tp = a.tab + qi * a.Bd * Q + t;
  const float* gp = a.go + qi * a.Bd;
  const char* dc = (const char*)a.d + c * 16;
  float v[PER], x[PER];
#pragma unroll
  for (int k = 0; k < PER; ++k) v[k] = 0.0f;
#pragma unroll 4
  for (int64_t j = 0; j < a.Bd; ++j) {
    const int p = tp[j * Q];
    if (p >= 0) {
      const float g = gp[j];
      load_chunk<DT>(dc + (j * D + p) * rowb, x);
#pragma unroll
      for (int k = 0; k < PER; ++k) v[k] += g * x[k];
    }
  }
  store_chunk<GT, PER>((char*)a.gq, row * E + (int64_t)c * PER, v);
}

// grad_d[j, p, e0 + col] = sum over (i, t) ascending with j*(i, j, t) = p of grad_out[i, j] q[i, t, e0 + col]
template <int DT, int GT>
__global__ void __launch_bounds__(256) inb_gradd_kernel(const InbBwdArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem_f[];
  const int Q = a.Q, D = a.D, E = a.E, et = a.et;
  int* ent_p = (int*)smem_f;                 // [kEnt] arg-max position of the staged entries (-1: none)
  float* ent_g = smem_f + kEnt;              // [kEnt] grad_out of their pair
  float* acc = smem_f + 2 * kEnt;            // [D][et]
  const int tid = threadIdx.x;
  const int col = tid & 63, s = tid >> 6;
  const int64_t dj = blockIdx.x / a.ntile;
  const int tile = (int)(blockIdx.x - dj * a.ntile);
  const int e0 = tile * et;
  const int w = E - e0 < et ? E - e0 : et;
  for (int k = tid; k < D * et; k += 256) acc[k] = 0.0f;
  const int64_t NE = a.Bq * Q;               // entry e = i * Q + t is also the row of q
  for (int64_t base = 0; base < NE; base += kEnt) {
    __syncthreads();                          // the previous round's entries have been consumed (first round: acc is zero)
#pragma unroll
    for (int u = 0; u < kEnt / 256; ++u) {
      const int k = tid + 256 * u;
      const int64_t e = base + k;
      int p = -1;
      float g = 0.0f;
      if (e < NE) {
        const int64_t i = e / Q;
        const int t = (int)(e - i * Q);
        p = a.tab[(i * a.Bd + dj) * Q + t];
        if (p >= 0) g = a.go[i * a.Bd + dj];
      }
      ent_p[k] = p;
      ent_g[k] = g;
    }
    __syncthreads();
    const int64_t left = NE - base;
    const int n = left < kEnt ? (int)left : kEnt;
    if (col < w) {
      for (int k0 = 0; k0 < n; k0 += 8) {     // (entries past n are -1)
        const int4 pa = *(const int4*)&ent_p[k0], pb = *(const int4*)&ent_p[k0 + 4];
        const int pp[8] = {pa.x, pa.y, pa.z, pa.w, pb.x, pb.y, pb.z, pb.w};
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int p = pp[u];
          if (p >= 0 && (p & 3) == s) {        // wave-uniform: cell (p, col) is this thread's alone
            const float x = load_elem<DT>(a.q, (base + k0 + u) * E + e0 + col);
            acc[p * et + col] += ent_g[k0 + u] * x;
          }
        }
      }
    }
  }
  __syncthreads();
  for (int k = tid; k < D * w; k += 256) {
    const int p = k / w, c = k - p * w;
    store_elem<GT>(a.gd, (dj * D + p) * (int64_t)E + e0 + c, acc[p * et + c]);
  }
}

size_t table_bytes(int64_t Bq, int64_t Bd, int Q) {
  return (((size_t)Bq * (size_t)Bd * (size_t)Q * 2) + 255) & ~(size_t)255;
}

template <int DT, int GT>
int launch(const InbBwdArgs& a, hipStream_t stream) {
  constexpr int PER = DT == MM_F32 ? 4 : 8;
  const int64_t pairs = a.Bq * a.Bd;
  hipLaunchKernelGGL(inb_argmax_kernel<DT>, dim3((unsigned)((pairs + 3) / 4)), dim3(256), 0, stream, a);
  if (int e = check_launch("inb_argmax_kernel")) return e;
  if (a.gq) {                                   // a null gradient is not wanted: its pass is skipped
    const int64_t items = a.Bq * a.Q * (a.E / PER);
    hipLaunchKernelGGL((inb_gradq_kernel<DT, GT>), dim3((unsigned)((items + 255) / 256)), dim3(256), 0, stream, a);
    if (int e = check_launch("inb_gradq_kernel")) return e;
  }
  if (!a.gd) return MM_OK;
  const size_t lds = ((size_t)2 * kEnt + (size_t)a.D * a.et) * 4;
  hipLaunchKernelGGL((inb_gradd_kernel<DT, GT>), dim3((unsigned)(a.Bd * a.ntile)), dim3(256), lds, stream, a);
  return check_launch("inb_gradd_kernel");
}

}  // namespace
}  // namespace mm

using namespace mm;

extern "C" size_t mm_maxsim_inbatch_bwd_workspace_bytes(int64_t Bq, int64_t Bd, int Q, int D, int E, int q_mask_kind,
                                                         int d_mask_kind) {
  (void)E;
  if (Bq <= 0 || Bd <= 0 || Q <= 0 || D <= 0) return 0;
  return packed_mask_bytes(q_mask_kind, Bq, Q) + packed_mask_bytes(d_mask_kind, Bd, D) + table_bytes(Bq, Bd, Q);
}

extern "C" int mm_maxsim_inbatch_bwd(const void* q, const void* d, const void* q_mask, int q_mask_kind, const void* d_mask,
                                     int d_mask_kind, const float* grad_out, void* grad_q, void* grad_d, int grad_dtype,
                                     int64_t Bq, int64_t Bd, int Q, int D, int E, int dtype, int bug_compatible,
                                     void* workspace, size_t workspace_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (Bq < 0 || Bd < 0 || Q <= 0 || D <= 0 || E <= 0) return set_error(MM_EINVAL, "maxsim_inbatch_bwd: bad shape");
  if (dtype != MM_F32 && dtype != MM_F16 && dtype != MM_BF16) return set_error(MM_EINVAL, "maxsim_inbatch_bwd: bad dtype %d", dtype);
  if (grad_dtype != MM_F32 && grad_dtype != dtype)
    return set_error(MM_EINVAL, "maxsim_inbatch_bwd: gradients are float32 or have the token vectors' own type (got %d for %d)",
                     grad_dtype, dtype);
  if (bug_compatible && Bq != Bd)
    return set_error(MM_EINVAL, "maxsim_inbatch_bwd: bug_compatible masking (colbert.py:158) requires Bq == Bd (got %lld, %lld)",
                     (long long)Bq, (long long)Bd);
  const int per16 = dtype == MM_F32 ? 4 : 8;
  if (E % per16)
    return set_error(MM_EUNSUPPORTED, "maxsim_inbatch_bwd: E=%d rows are not 16-byte multiples (pad E to a multiple of %d)", E, per16);
  const size_t gs = grad_dtype == MM_F32 ? 4 : 2;
  if (Bq == 0 || Bd == 0) {                     // no pair: whichever gradient has elements is all zeros
    if (Bq && grad_q && hipMemsetAsync(grad_q, 0, (size_t)Bq * Q * E * gs, stream) != hipSuccess)
      return set_error(MM_ELAUNCH, "maxsim_inbatch_bwd: memset of grad_q failed");
    if (Bd && grad_d && hipMemsetAsync(grad_d, 0, (size_t)Bd * D * E * gs, stream) != hipSuccess)
      return set_error(MM_ELAUNCH, "maxsim_inbatch_bwd: memset of grad_d failed");
    return MM_OK;
  }
  if (!q || !d || !grad_out) return set_error(MM_EINVAL, "maxsim_inbatch_bwd: null tensor pointer");
  if (!grad_q && !grad_d) return MM_OK;         // neither gradient is wanted
  if (((uintptr_t)q | (uintptr_t)d | (uintptr_t)grad_q | (uintptr_t)grad_d) & 15)
    return set_error(MM_EINVAL, "maxsim_inbatch_bwd: q, d and the gradients must be 16-byte aligned");
  if (D > 32767)
    return set_error(MM_EUNSUPPORTED, "maxsim_inbatch_bwd: D = %d document positions exceed the int16 arg-max table", D);
  InbBwdArgs a{};
  a.q = q; a.d = d; a.go = grad_out; a.gq = grad_q; a.gd = grad_d; a.Bq = Bq; a.Bd = Bd; a.Q = Q; a.D = D; a.E = E;
  a.bug = bug_compatible ? 1 : 0;
  // grad_d's accumulator: [D, et] floats in LDS next to the 8 KiB of staged entries, 64 KiB per workgroup in all
  int64_t et = (int64_t)(64 * 1024 - 2 * kEnt * 4) / ((int64_t)D * 4);
  if (et > 64) et = 64;
  if (et > E) et = E;
  if (et < 1)
    return set_error(MM_EUNSUPPORTED, "maxsim_inbatch_bwd: D = %d document positions exceed the LDS accumulator of grad_d", D);
  a.et = (int)et;
  a.ntile = (E + a.et - 1) / a.et;
  const int64_t lim = 0x7fffffffLL;
  if ((Bq * Bd + 3) / 4 > lim || (Bq * Q * (E / per16) + 255) / 256 > lim || Bd * a.ntile > lim)
    return set_error(MM_EUNSUPPORTED, "maxsim_inbatch_bwd: %lld x %lld pairs exceed one launch", (long long)Bq, (long long)Bd);
  WsCursor ws(workspace, workspace_bytes);
  if (int e = resolve_mask(q_mask, q_mask_kind, Bq, Q, ws, stream, &a.qm)) return e;
  if (int e = resolve_mask(d_mask, d_mask_kind, Bd, D, ws, stream, &a.dm)) return e;
  const size_t tb = table_bytes(Bq, Bd, Q);
  if (!ws.p || ws.left < tb)
    return set_error(MM_EWORKSPACE, "maxsim_inbatch_bwd: workspace too small for the arg-max table: need %zu more bytes, have %zu", tb, ws.left);
  a.tab = (int16_t*)ws.p;
  if (dtype == MM_F32) return launch<MM_F32, MM_F32>(a, stream);
  if (dtype == MM_F16) return grad_dtype == MM_F32 ? launch<MM_F16, MM_F32>(a, stream) : launch<MM_F16, MM_F16>(a, stream);
  return grad_dtype == MM_F32 ? launch<MM_BF16, MM_F32>(a, stream) : launch<MM_BF16, MM_BF16>(a, stream);
}
