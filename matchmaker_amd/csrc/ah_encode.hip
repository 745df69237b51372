// Anisotropic 4-bit encoder (dense retrieval, faiss_index_type: scann) for MI355X (gfx950 / CDNA4).
//
// Replaces the encoding step of the reference's ScaNN index (matchmaker/retrieval/scann_index.py:24-47:
// `score_ah(2, anisotropic_quantization_threshold=0.2)` = one of 16 codewords per 2-dimensional block of the residual to
// the row's leaf centre, chosen under the anisotropic loss).  Semantics: mm_native.h, mm_ah_encode.
//
// One 16-lane row per vector (four vectors per wavefront, sixteen per workgroup), lane c = candidate codeword c of the
// block at hand; the blocks are walked in ascending order, the best candidate of a block is found by a 4-step butterfly
// over the row's lanes that carries (cost, code) and prefers the lower code on equal cost.  The codebook sits in LDS as
// one dword per (block, codeword) (32 E bytes: 24 KB at E 768; the 16 lanes of a row read 16 consecutive dwords, the four
// rows of a wavefront the same ones), the codes chosen so far as one byte per block.  Every fp32 operation is a single
// rounded +, -, x (no contraction into fused multiply-adds), in the order mm_native.h states, so a host restatement in
// float32 reproduces the codes.  One launch, no atomics, no workspace.
#include "mm_internal.h"

namespace mm {

template <int DT>
__device__ __forceinline__ void enc_unpack(uint32_t d, float* lo, float* hi);
template <>
__device__ __forceinline__ void enc_unpack<MM_F16>(uint32_t d, float* lo, float* hi) {
  *lo = (float)__builtin_bit_cast(_Float16, (uint16_t)(d & 0xffffu));
  *hi = (float)__builtin_bit_cast(_Float16, (uint16_t)(d >> 16));
}
template <>
__device__ __forceinline__ void enc_unpack<MM_BF16>(uint32_t d, float* lo, float* hi) {
  *lo = __uint_as_float(d << 16);
  *hi = __uint_as_float(d & 0xffff0000u);
}

// (cost, code) of the row's best candidate in every lane of the row: least cost, lowest code on equal cost
__device__ __forceinline__ int enc_argmin16(float v, int c) {
  int bi = c;
#pragma unroll
  for (int m = 8; m >= 1; m >>= 1) {
    const float ov = __shfl_xor(v, m, 16);
    const int oi = __shfl_xor(bi, m, 16);
    if (ov < v || (ov == v && oi < bi)) { v = ov; bi = oi; }
  }
  return bi;
}

template <int DT>
__global__ void __launch_bounds__(256) ah_encode_kernel(const void* x_, const int32_t* list, const void* cent_, const void* cb_,
                                                        float eta, int passes, uint8_t* codes, int64_t n, int nlist, int E) {
  extern __shared__ __attribute__((aligned(16))) uint32_t sm[];
  const int S = E >> 1;                       // blocks
  uint32_t* tab = sm;                         // [S * 16] (block, codeword) -> two 16-bit values
  uint8_t* cur = (uint8_t*)(sm + S * 16) + (threadIdx.x >> 4) * S;   // [S] this vector's codes
  {
    const uint32_t* cb = (const uint32_t*)cb_;
    for (int i = threadIdx.x; i < S * 16; i += 256) tab[i] = cb[i];
  }
  __syncthreads();
  const int c = threadIdx.x & 15;
  const int64_t vec = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
  const bool valid = vec < n;
  const int64_t vv = valid ? vec : n - 1;     // lanes past the end repeat the last vector: every shuffle has its 16 lanes
  const int l = list[vv];
  const bool has_c = l >= 0 && l < nlist;     // a list outside [0, nlist) counts as a zero centre
  const uint32_t* xrow = (const uint32_t*)((const char*)x_ + vv * E * 2);
  const uint32_t* crow = (const uint32_t*)((const char*)cent_ + (int64_t)(has_c ? l : 0) * E * 2);

  // |x|^2: lane c sums its blocks c, c + 16, ... (x0 x0 then x1 x1, in that order), then the butterfly 8, 4, 2, 1
  float nn = 0.0f;
  for (int s = c; s < S; s += 16) {
    float x0, x1;
    enc_unpack<DT>(xrow[s], &x0, &x1);
    nn = __fadd_rn(nn, __fmul_rn(x0, x0));
    nn = __fadd_rn(nn, __fmul_rn(x1, x1));
  }
#pragma unroll
  for (int m = 8; m >= 1; m >>= 1) nn = __fadd_rn(nn, __shfl_xor(nn, m, 16));
  const float nrm = __fsqrt_rn(nn);
  const float inv = nrm > 0.0f ? __fdiv_rn(1.0f, nrm) : 0.0f;
  const float em1 = nrm > 0.0f ? __fsub_rn(eta, 1.0f) : 0.0f;   // an all-zero row: eta = 1

  float p = 0.0f;                             // the parallel error: sum over the blocks of <e_s, xhat_s>
  for (int pass = 0; pass <= passes; ++pass) {
    for (int s = 0; s < S; ++s) {
      float x0, x1, c0 = 0.0f, c1 = 0.0f, w0, w1;
      enc_unpack<DT>(xrow[s], &x0, &x1);
      if (has_c) enc_unpack<DT>(crow[s], &c0, &c1);
      enc_unpack<DT>(tab[s * 16 + c], &w0, &w1);
      const float e0 = __fsub_rn(__fsub_rn(x0, c0), w0), e1 = __fsub_rn(__fsub_rn(x1, c1), w1);
      const float nk = __fadd_rn(__fmul_rn(e0, e0), __fmul_rn(e1, e1));
      const float tk = __fadd_rn(__fmul_rn(e0, __fmul_rn(x0, inv)), __fmul_rn(e1, __fmul_rn(x1, inv)));
      int best;
      if (pass == 0) {
        best = enc_argmin16(nk, c);
        p = __fadd_rn(p, __shfl(tk, best, 16));
      } else {
        const float po = __fsub_rn(p, __shfl(tk, (int)cur[s], 16));
        const float u = __fadd_rn(po, tk);
        best = enc_argmin16(__fadd_rn(nk, __fmul_rn(em1, __fmul_rn(u, u))), c);
        p = __fadd_rn(po, __shfl(tk, best, 16));
      }
      cur[s] = (uint8_t)best;                 // every lane of the row writes the same byte, and reads back its own write
    }
  }
  if (valid)
    for (int i = c; i < (S >> 1); i += 16) codes[vec * (E >> 2) + i] = (uint8_t)(cur[2 * i] | (cur[2 * i + 1] << 4));
}

}  // namespace mm

using namespace mm;

extern "C" int mm_ah_encode(const void* x, const int32_t* list, const void* centroids, const void* codebook, int64_t n,
                            int nlist, int E, int dtype, float eta, int passes, uint8_t* codes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (n == 0) return MM_OK;
  if (!x || !list || !centroids || !codebook || !codes) return set_error(MM_EINVAL, "ah_encode: null pointer");
  if (n < 0 || nlist <= 0) return set_error(MM_EINVAL, "ah_encode: non-positive shape");
  if (dtype != MM_F16 && dtype != MM_BF16) return set_error(MM_EUNSUPPORTED, "ah_encode: float16 / bfloat16 vectors only");
  if (E != 128 && E != 256 && E != 384 && E != 512 && E != 768)
    return set_error(MM_EUNSUPPORTED, "ah_encode: E=%d is not one of 128, 256, 384, 512, 768 (pad the vectors)", E);
  if (!(eta >= 0.0f) || !(eta <= 3.0e38f) || passes < 0 || passes > 64)
    return set_error(MM_EUNSUPPORTED, "ah_encode: eta=%g must be finite and >= 0, passes=%d in 0 .. 64", (double)eta, passes);
  if (n >= (1LL << 35)) return set_error(MM_EUNSUPPORTED, "ah_encode: more than 2^35-1 vectors in one call");
  if (((uintptr_t)x | (uintptr_t)centroids | (uintptr_t)codebook) & 3) return set_error(MM_EINVAL, "ah_encode: 4-byte alignment required");
  const size_t lds = (size_t)E * 32 + (size_t)16 * (E / 2);
  const dim3 grid((unsigned)((n + 15) / 16)), block(256);
  if (dtype == MM_BF16)
    hipLaunchKernelGGL(ah_encode_kernel<MM_BF16>, grid, block, lds, stream, x, list, centroids, codebook, eta, passes, codes, n, nlist, E);
  else
    hipLaunchKernelGGL(ah_encode_kernel<MM_F16>, grid, block, lds, stream, x, list, centroids, codebook, eta, passes, codes, n, nlist, E);
  return check_launch("ah_encode_kernel");
}
