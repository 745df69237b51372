// Internal helpers shared by the HIP translation units of libmm_native.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdarg.h>
#include <type_traits>

#include "../../include/mm_native.h"
#include "launch_geometry.h"

namespace mm {

typedef __attribute__((ext_vector_type(8))) short short8;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) float f32x4;

constexpr int kWave = 64;   // (kCUs: launch_geometry.h)

int set_error(int code, const char* fmt, ...);

// Tuning / A-B knobs read from the environment ONCE per process.  env() returns a function-local static const
// (C++11 guarantees thread-safe initialisation), so the library holds no unsynchronised mutable state: the
// operators are called concurrently from nn.DataParallel's per-GPU threads (matchmaker/train.py:201).
struct EnvCfg {
  int maxsim_nbuf = 2;      // MM_MAXSIM_NBUF: LDS ring depth of the MaxSim roofline kernel (2..4)
  int maxsim_wpc = 4;       // MM_MAXSIM_WPC: wavefronts per CU to launch (0 = what LDS allows)
  int maxsim_nt = 1;        // MM_MAXSIM_NT: non-temporal LDS-DMA
  int maxsim_generic = 0;   // MM_MAXSIM_GENERIC: force the generic MaxSim kernel
  int maxsim_inb_untiled = 0;  // MM_MAXSIM_INB_UNTILED: all-pairs MaxSim with one query per wavefront (A/B runs)
  int maxsim_no_inline_masks = 0;  // MM_MAXSIM_NO_INLINE_MASKS: pack int64 masks in their own launch even for one-pair-per-wavefront calls (A/B runs)
  int maxsim_no_wpp2 = 0;          // MM_MAXSIM_NO_WPP2: one wavefront per pair also in eval.py-sized calls (A/B runs)
  int maxsim_inb_nowg = 0;     // MM_MAXSIM_INB_NOWG: all-pairs MaxSim without the workgroup-shared ring (A/B runs)
  int maxsim_f32_terms = 3; // MM_MAXSIM_F32_TERMS: 2 = two-term split for fp32 MaxSim (A/B), default three terms
  int kp_generic = 0;       // MM_KP_GENERIC: force the generic pooling kernel
  int kp_f32mfma = 0;       // MM_KP_F32MFMA: exact-f32 MFMA pooling kernel instead of split-bf16
  int dot_prof = 0;         // MM_DOT_PROF: in-kernel phase counters of the dot top-k kernel
  int kp_bwd_threads = 1024; // MM_KP_BWD_THREADS: 1024 (when its LDS fits) | 512 threads per pair in kernel_pool_bwd_tiled_kernel (A/B runs)
  int kp_bwd_nsplit = 0;    // MM_KP_BWD_NSPLIT=n: workgroups per pair of the split backward (0: by batch size — 4 up to 128 pairs, else 1)
  int kp_bwd_f32 = 0;       // MM_KP_BWD_F32=1: pooling backward on the exact-f32 tiled kernel of rounds 4-5 instead of the split-bf16 streaming kernel (parity twin, A/B runs)
  int kp_bwd_untiled = 0;   // MM_KP_BWD_UNTILED: pooling backward on the per-element kernel of rounds 1-3 (A/B runs)
  int kp_multi_loop = -1;     // MM_KP_MULTI_LOOP: Conv-KNRM's multi launch as one wavefront per (pair range, document tensor) looping over the query
                              // tensors (kernel_pool_multi128_kernel: every document block crosses HBM once, 22.5 GB fetched instead of 47.3).
                              // -1 = by launch size (>= 2,048 pairs), 0 / 1 = never / always (A/B runs)
  int kp_multi_2d = 0;        // MM_KP_MULTI_2D=1: Conv-KNRM's multi launch on the 2-D grid of rounds 1-4 instead of the flat XCD-grouped order (A/B runs)
  int kp128_occ = 0;          // MM_KP128_OCC: 0 = choose by shape, 1 / 2 = wavefronts per SIMD of the 64n-wide pooling kernel (A/B runs)
  int tkl_bwd_nosplit = 0;    // MM_TKL_BWD_NOSPLIT=1: TKL's backward with one workgroup per document at every batch size (A/B runs)
  int mp_generic = 0;       // MM_MP_GENERIC=1: MatchPyramid on the generic kernel also at the reference config (bit-equal twin, A/B runs)
};
const EnvCfg& env();

inline int check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return set_error(MM_ELAUNCH, "%s: %s", what, hipGetErrorString(e));
  return MM_OK;
}

// ---- mask handling -------------------------------------------------------------------------
// The kernels consume, per mask row, an int32 "effective length" (positions >= len are padding
// and never need to be loaded) and optionally one validity bit per position (for non-prefix
// masks).  LEN_I32 masks are used as-is; U8/I64/F32 masks are packed by pack_mask_kernel.
struct PackedMask {
  const int32_t* len = nullptr;    // [rows] or null (all positions real)
  const uint32_t* bits = nullptr;  // [rows, ceil(L/32)] or null
};

size_t packed_mask_bytes(int kind, int64_t rows, int L);
// Resolves a user mask to a PackedMask, launching the pack kernel into `ws` when needed.
// Advances *ws / *ws_left.  Returns MM_OK or an error code.
// Dense masks may be strided: row i starts at mask + i*row_stride + col0 (row_stride 0 = L).
int resolve_mask(const void* mask, int kind, int64_t rows, int L, char** ws, size_t* ws_left,
                 hipStream_t stream, PackedMask* out, int64_t row_stride = 0, int col0 = 0);

// Both masks of a call: two dense masks of one element type are packed by ONE launch (else one resolve_mask each).
int resolve_mask_pair(const void* m0, int kind0, int64_t rows0, int L0, PackedMask* out0, const void* m1, int kind1,
                      int64_t rows1, int L1, PackedMask* out1, char** ws, size_t* ws_left, hipStream_t stream);
// ... the same two on an entry point's workspace cursor
inline int resolve_mask(const void* mask, int kind, int64_t rows, int L, WsCursor& ws, hipStream_t stream, PackedMask* out) {
  return resolve_mask(mask, kind, rows, L, &ws.p, &ws.left, stream, out);
}
inline int resolve_mask_pair(const void* m0, int kind0, int64_t rows0, int L0, PackedMask* out0, const void* m1, int kind1,
                             int64_t rows1, int L1, PackedMask* out1, WsCursor& ws, hipStream_t stream) {
  return resolve_mask_pair(m0, kind0, rows0, L0, out0, m1, kind1, rows1, L1, out1, &ws.p, &ws.left, stream);
}

// Run-time value -> template argument: f is a generic lambda, called with std::integral_constant<int, V> (`decltype(v)::value`
// is the template argument inside it).  One instantiation per value named here, as the ladders these replace had.
template <int V>
using Int = std::integral_constant<int, V>;
#define MM_V(v) decltype(v)::value
template <class F>
inline int with_nsl(int E, F&& f) {          // NSL = E / 128 of a stream_width(E): 1, 2, 3, 4, 6
  switch (E / 128) {
    case 1: return f(Int<1>{});
    case 2: return f(Int<2>{});
    case 3: return f(Int<3>{});
    case 4: return f(Int<4>{});
    default: return f(Int<6>{});
  }
}
template <class F>
inline int with_ns(int E, F&& f) {           // NS = E / 100 of a kp_stream_width(E): 1, 2, 3
  return E == 100 ? f(Int<1>{}) : E == 200 ? f(Int<2>{}) : f(Int<3>{});
}
template <class F>
inline int with_dtype16(int dtype, F&& f) {   // MM_BF16, else MM_F16
  return dtype == MM_BF16 ? f(Int<MM_BF16>{}) : f(Int<MM_F16>{});
}
template <class F>
inline int with_dtype(int dtype, F&& f) {     // ... and MM_F32
  return dtype == MM_F32 ? f(Int<MM_F32>{}) : with_dtype16(dtype, f);
}

// a.pairs_per_wave and the grid of a launch whose wavefronts (or workgroups) each take a range of the a.n_pairs pairs
template <class Args>
inline unsigned split_pairs(Args& a, int64_t max_waves) {
  const WaveSplit s = wave_split(a.n_pairs, max_waves);
  a.pairs_per_wave = s.pairs_per_wave;
  return (unsigned)s.grid;
}

constexpr int kK = 11;   // RBF kernels of TK / TKL (tk.yaml:18-19, tkl.yaml)
constexpr int kKC = 12;  // K + the non-zero-count channel of TKL's pair sums

// RBF kernels by middle-out recurrence where the kernel set allows it (kp_device.h rbf_geo_one, tkl.hip's window staging);
// -DMM_RBF_GEO=0 builds the direct form everywhere (A/B libraries).
#ifndef MM_RBF_GEO
#define MM_RBF_GEO 1
#endif
constexpr float kGeoClamp = 13.0f;   // exp2(-13^2) = 0 exactly (below the smallest denormal): a clamped masked row adds exactly 0

struct TklParams {            // offsets into the packed float parameter vector (see mm_native.h)
  __host__ __device__ static int mu() { return 0; }
  __host__ __device__ static int sigma() { return kK; }
  __host__ __device__ static int dense() { return 2 * kK; }
  __host__ __device__ static int kmult() { return 3 * kK; }
  __host__ __device__ static int sat() { return 4 * kK; }       // w1[2] b1 w2[2] b2 w3[2] b3 lnw[2] lnb[2]
  __host__ __device__ static int chunk_scoring() { return 4 * kK + 13; }
  __host__ __device__ static int emb() { return 4 * kK + 13 + 15; }
};

// kernel_pool.hip exports used by tkl.hip
bool kp_stream_supported(int Q, int E);
int tkl_stage1_stream(const float* q_ctx, const float* chunks, PackedMask dm, const int32_t* q_len,
                      const int32_t* chunk_slot, int C, const float* mu, const float* sigma, float* ps_out, int64_t P,
                      int Q, int E, int32_t* slot2p, int64_t n_slots, hipStream_t stream, float* cos_out = nullptr);
bool tkl_cos_supported(int Q, int E);

// kernel_pool128.hip: fp32 MaxSim on the split-bf16 streaming kernel (E = 64n <= 384, 512, 768; Q <= 32), called from maxsim.hip
bool kp128_maxsim_supported(int Q, int E);
int kp128_maxsim_f32(const float* q, const float* d, PackedMask qm, PackedMask dm, float* out, int64_t n_pairs,
                     int64_t pairs_per_query, int Q, int D, int E, hipStream_t stream);

// dot_topk.hip: the selection phases of the flat inner-product top-k (threshold from a sample, candidate lists, exact top-k
// of the survivors), shared by mm_dot_topk_fwd and mm_dot_topk_fp8_fwd (dot_topk_fp8.hip), which differ in the streaming
// kernel between them only.  The workspace of a call is laid out by dot_sel_carve (dot_sel_bytes() runs it on a measuring
// cursor): sample scores [nq, S] | tau [nq] | survivor counts [nq] | candidate scores and rows [nq, cap] each.
constexpr int kDotSample = 16384;  // sample size (documents) of phase 1 when the shard is larger
struct DotSel {
  float* all;         // [nq, S] scores of the strided sample
  float* tau;         // [nq] thresholds
  int32_t* count;     // [nq] survivors (may exceed cap: overflow)
  float* cand_score;  // [nq, cap]
  int32_t* cand_idx;  // [nq, cap]
  int cap;
  int64_t S;          // min(n_docs, kDotSample)
};
int dot_cap(int64_t n_docs, int k);
size_t dot_sel_bytes(int64_t n_docs, int nq, int k);
DotSel dot_sel_carve(WsCursor& ws, int64_t n_docs, int nq, int k);
int dot_sample_m(int64_t n_docs, int64_t S, int k, float m_scale);   // the sample rank that becomes the threshold
void launch_fill_tau(const DotSel& d, int nq, float v, hipStream_t stream);             // fill_tau_kernel
void launch_sample_tau(const DotSel& d, int nq, int m, hipStream_t stream);             // sample_tau_kernel
int launch_topk_rows(const DotSel& d, int nq, int k, int64_t n_total, float* out_scores, int64_t* out_idx, int32_t* status,
                     hipStream_t stream);                                                // topk_rows_kernel

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// C/D layout of the 32x32 MFMA: lane l holds column (l & 31), rows rowof(i) + 4*(l >> 5).
__device__ __forceinline__ constexpr int rowof(int i) { return (i & 3) + 8 * (i >> 2); }

// Wave-uniform 32-bit load through the scalar cache.  The compiler cannot use s_load here on its
// own (the asm "memory" clobbers of the LDS-DMA pipeline make every global look written), and a
// vector load would make it wait vmcnt(0) and drain the D stream once per pair.  Lengths / mask
// words are never written by these kernels, so the (non-coherent) scalar cache is safe.
__device__ __forceinline__ uint32_t sload_u32(const void* base, int64_t idx) {
  uint32_t v;
  const uint32_t* p = (const uint32_t*)base + idx;
  asm volatile("s_load_dword %0, %1, 0x0\n\ts_waitcnt lgkmcnt(0)" : "=s"(v) : "s"(p));
  return v;
}

__device__ __forceinline__ float neg_inf() { return -__builtin_huge_valf(); }

constexpr float kTiny = 1e-13f;   // allennlp's cosine (mm_native.h, kernel pooling): x / (|x| + kTiny)

// guarded 16-byte load: zeros where the row or the chunk does not exist
__device__ __forceinline__ f32x4 load4_or0(const float* p, bool ok) {
  return ok ? *(const f32x4*)p : f32x4{0.0f, 0.0f, 0.0f, 0.0f};
}

}  // namespace mm
