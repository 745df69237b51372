// Self-attention core of the TK-family contextualiser (matchmaker/models/published/ecai20_tk.py:138, sigir20_tkl.py:296-308,
// sigir21_idcm.py:174-175: nn.TransformerEncoder with a key-padding mask, whose layers run F.multi_head_attention_forward):
//
//   out[b, i, h dh + d] = sum_j softmax_j(q[b,i,h] . k[b,j,h] / sqrt(dh) + (mask[b,j] ? 0 : -inf)) v[b,j,h,d]
//
//   mm_self_attention_fwd   one workgroup per (sequence, head), up to four wavefronts.  The head's K and V are staged once in
//                           LDS, V as fp32 (16-bit inputs widened exactly) and K in the input type, zero-padded to DP = 32 or
//                           64 columns and to a multiple of 32 rows; the mask becomes one additive fp32 term per key (0 or -inf).  Each wavefront
//                           owns 32-row query blocks.  Per block:
//                             S^T = K Q^T   v_mfma_f32_32x32x2_f32 for fp32 inputs, v_mfma_f32_32x32x16_{f16,bf16} for 16-bit ones
//                                           (every product exact in fp32), A = K rows from LDS, B = the lane's query row held in
//                                           registers; lane (r, h) then holds, for query r, the scores of the keys
//                                           32 t + rowof(i) + 4 h of every key tile t: a whole score row sits in two lanes.
//                             softmax       in those registers: scale and mask by one fma (log2 domain), the row maximum and
//                                           the row sum by an in-lane reduction and one exchange between the lane halves,
//                                           v_exp_f32.  Nothing is normalised yet.
//                             O^T = V^T P^T v_mfma_f32_32x32x2_f32 for every input type (the weights are not rounded to 16 bits), with the k index walking the keys in the order the lanes
//                                           hold them: step (t, i) pairs the keys 32 t + rowof(i) and 32 t + rowof(i) + 4, so
//                                           B is the register the lane already has and A is one LDS read of V.  No LDS round
//                                           trip for P.
//                             store         lane (r, h) holds, for query r, the d columns 8 g + 4 h + (0..3): divided by the
//                                           row sum, rounded once to the output type, stored four at a time as far as the
//                                           alignment allows.
//                           A sequence with no unmasked key has row sum 0 and gets exactly +0.
// Head slices are not 16-byte aligned in general (dh 30: 120 bytes in fp32, 60 in fp16), so every global access is made in
// chunks of `cb` bytes, the largest of 16 / 8 / 4 / 2 that divides the two base addresses, the row stride and the head slice;
// the values loaded and the arithmetic do not depend on cb, so the result does not depend on the alignment.
// No atomics, no workspace, no read-back, one launch, vector stores only, every output element stored exactly once: graph-capturable,
// and two calls give the same bits.
#include "mm_internal.h"
#include "elem_device.h"

#include <math.h>

namespace mm {

constexpr int kSaMaxL = 256;     // longest sequence: a whole score row of a query lives in two lanes' registers
constexpr int kSaMaxDh = 64;     // widest head

// CB >= 4 bytes at p (CB-aligned) as 32-bit words
template <int CB>
__device__ __forceinline__ void sa_load_words(const char* p, uint32_t* w) {
  if constexpr (CB == 16) {
    const uint4 x = *(const uint4*)p;
    w[0] = x.x; w[1] = x.y; w[2] = x.z; w[3] = x.w;
  } else if constexpr (CB == 8) {
    const uint2 x = *(const uint2*)p;
    w[0] = x.x; w[1] = x.y;
  } else {
    w[0] = *(const uint32_t*)p;
  }
}

// ... as CB / 2 raw 16-bit elements (CB >= 2)
template <int CB>
__device__ __forceinline__ void sa_load_h(const char* p, uint16_t* e) {
  if constexpr (CB == 2) {
    e[0] = *(const uint16_t*)p;
  } else {
    uint32_t w[CB / 4];
    sa_load_words<CB>(p, w);
#pragma unroll
    for (int k = 0; k < CB / 2; ++k) e[k] = (uint16_t)(w[k >> 1] >> (16 * (k & 1)));
  }
}

// ... as CB / sizeof(element) floats, exactly
template <int DT, int CB>
__device__ __forceinline__ void sa_load(const char* p, float* v) {
  if constexpr (DT == MM_F32) {
    uint32_t w[CB / 4];
    sa_load_words<CB>(p, w);
#pragma unroll
    for (int k = 0; k < CB / 4; ++k) v[k] = __uint_as_float(w[k]);
  } else {
    uint16_t e[CB / 2];
    sa_load_h<CB>(p, e);
#pragma unroll
    for (int k = 0; k < CB / 2; ++k) v[k] = bits_to_f32<DT>(e[k]);
  }
}

template <int DT>
__device__ __forceinline__ uint32_t sa_bits16(float v) {
  if constexpr (DT == MM_F16) return (uint32_t)__builtin_bit_cast(uint16_t, (_Float16)v);
  else return bf16_rne_bits_nan(v);
}

// four consecutive output columns d0 .. d0 + 3 at p, those below dh, each rounded once; stores of min(CB, 4 elements) bytes
template <int DT, int CB>
__device__ __forceinline__ void sa_store4(char* p, const float* v, int d0, int dh) {
  if constexpr (DT == MM_F32) {
    if constexpr (CB == 16) {
      if (d0 < dh) *(f32x4*)p = f32x4{v[0], v[1], v[2], v[3]};
    } else if constexpr (CB == 8) {
#pragma unroll
      for (int k = 0; k < 4; k += 2)
        if (d0 + k < dh) *(float2*)(p + 4 * k) = float2{v[k], v[k + 1]};
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (d0 + k < dh) ((float*)p)[k] = v[k];
    }
  } else {
    const uint32_t b0 = sa_bits16<DT>(v[0]), b1 = sa_bits16<DT>(v[1]), b2 = sa_bits16<DT>(v[2]), b3 = sa_bits16<DT>(v[3]);
    if constexpr (CB >= 8) {
      if (d0 < dh) *(uint2*)p = uint2{b0 | (b1 << 16), b2 | (b3 << 16)};
    } else if constexpr (CB == 4) {
      if (d0 < dh) *(uint32_t*)p = b0 | (b1 << 16);
      if (d0 + 2 < dh) *(uint32_t*)(p + 4) = b2 | (b3 << 16);
    } else {
      const uint32_t b[4] = {b0, b1, b2, b3};
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (d0 + k < dh) ((uint16_t*)p)[k] = (uint16_t)b[k];
    }
  }
}

// K and V of one head, rows [0, L), into the zeroed LDS arrays (row strides KS / VS floats)
template <int DT, int CB>
__device__ __forceinline__ void sa_stage(const char* krow0, const char* vrow0, int64_t rs, int L, int dh, float* Ks, int KS,
                                         float* Vs, int VS, int tid, int nthr) {
  constexpr int ES = DT == MM_F32 ? 4 : 2, N = CB / ES;
  const int cpr = dh / N;      // chunks per row (dh is a multiple of N)
  for (int idx = tid; idx < L * cpr; idx += nthr) {
    const int j = idx / cpr, c = idx - j * cpr;
    float kv[N], vv[N];
    sa_load<DT, CB>(krow0 + j * rs + c * CB, kv);
    sa_load<DT, CB>(vrow0 + j * rs + c * CB, vv);
#pragma unroll
    for (int k = 0; k < N; ++k) {
      Ks[j * KS + c * N + k] = kv[k];
      Vs[j * VS + c * N + k] = vv[k];
    }
  }
}

// 16-bit inputs: K stays 16-bit in LDS (the operand of the 16-bit MFMA, row stride K16S elements), V is widened for the fp32 product
template <int DT, int CB>
__device__ __forceinline__ void sa_stage16(const char* krow0, const char* vrow0, int64_t rs, int L, int dh, uint16_t* K16, int K16S,
                                           float* Vs, int VS, int tid, int nthr) {
  constexpr int N = CB / 2;
  const int cpr = dh / N;
  for (int idx = tid; idx < L * cpr; idx += nthr) {
    const int j = idx / cpr, c = idx - j * cpr;
    uint16_t kb[N];
    float vv[N];
    sa_load_h<CB>(krow0 + j * rs + c * CB, kb);
    sa_load<DT, CB>(vrow0 + j * rs + c * CB, vv);
#pragma unroll
    for (int k = 0; k < N; ++k) {
      K16[j * K16S + c * N + k] = kb[k];
      Vs[j * VS + c * N + k] = vv[k];
    }
  }
}

// the lane's operand of the 16-bit score product: q[c] = Q[row][16 c + 8 half .. + 7], zeros beyond the head slice and for absent rows
template <int CB, int NC>
__device__ __forceinline__ void sa_load_q16(const char* qrow, bool row_ok, int half, int dh, short8* q) {
  constexpr int N = CB / 2;
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    uint16_t e[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) e[k] = 0;
#pragma unroll
    for (int p = 0; p < 8 / N; ++p) {
      const int e0 = 16 * c + 8 * half + p * N;
      if (row_ok && e0 < dh) sa_load_h<CB>(qrow + e0 * 2, e + p * N);
    }
    q[c] = short8{(short)e[0], (short)e[1], (short)e[2], (short)e[3], (short)e[4], (short)e[5], (short)e[6], (short)e[7]};
  }
}

// the lane's half of its query row: q[c] = Q[row][half * hd + c] for c < hd, zeros beyond the head slice and for absent rows
template <int DT, int CB, int HQ>
__device__ __forceinline__ void sa_load_q(const char* qrow, bool row_ok, int half, int hd, int dh, float* q) {
  constexpr int ES = DT == MM_F32 ? 4 : 2, N = CB / ES;
#pragma unroll
  for (int c = 0; c < HQ; c += N) {
    float v[N];
#pragma unroll
    for (int k = 0; k < N; ++k) v[k] = 0.0f;
    const int e0 = half * hd + c;
    if (row_ok && c < hd && e0 < dh) sa_load<DT, CB>(qrow + e0 * ES, v);
#pragma unroll
    for (int k = 0; k < N; ++k) q[c + k] = v[k];
  }
}

template <int DT, int CB>
__device__ __forceinline__ void sa_store_tile(char* orow, const f32x16& o, float l, int half, int dbase, int dh) {
  constexpr int ES = DT == MM_F32 ? 4 : 2;
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const int d0 = dbase + 8 * g + 4 * half;
    float v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = l > 0.0f ? o[4 * g + k] / l : 0.0f;
    sa_store4<DT, CB>(orow + d0 * ES, v, d0, dh);
  }
}

// run-time cb -> template argument (wave-uniform)
#define SA_WITH_CB(cb, CALL)                                   \
  do {                                                         \
    if constexpr (DT == MM_F32) {                              \
      switch (cb) {                                            \
        case 16: { constexpr int CB = 16; CALL; } break;       \
        case 8: { constexpr int CB = 8; CALL; } break;         \
        default: { constexpr int CB = 4; CALL; } break;        \
      }                                                        \
    } else {                                                   \
      switch (cb) {                                            \
        case 16: { constexpr int CB = 16; CALL; } break;       \
        case 8: { constexpr int CB = 8; CALL; } break;         \
        case 4: { constexpr int CB = 4; CALL; } break;         \
        default: { constexpr int CB = 2; CALL; } break;        \
      }                                                        \
    }                                                          \
  } while (0)

// floats per K row in LDS: fp32 rows of DP + 1 (odd: the 32 key rows of an A read fall into 32 banks), 16-bit rows of DP + 8
// elements (16-byte aligned for the 16-byte operand reads)
constexpr int sa_k_row_floats(int DT, int DP) { return DT == MM_F32 ? DP + 1 : (DP + 8) / 2; }

inline size_t sa_lds_bytes(int L, int DP, int DT) {
  const int LP = (L + 31) & ~31;
  return (size_t)LP * (sa_k_row_floats(DT, DP) + (DP + 8) + 1) * sizeof(float);
}

// NT = key tiles the registers hold: 4 (L <= 128) or 8.  Two wavefronts per SIMD wherever the score rows leave the registers for it
// (one hides the other's loads and softmax behind its own matrix work: 721 -> 448 us on 512 x 200 x 10 heads of 30).
template <int DT, int DP, int NT>
__global__ void __launch_bounds__(256, (DP == 32 || NT == 4) ? 2 : 1)
    self_attention_kernel(const char* __restrict__ qkv, const void* __restrict__ mask, int mask_kind, int L, int H, int dh, int cb,
                          float c2, char* __restrict__ out) {
  constexpr int ES = DT == MM_F32 ? 4 : 2;
  constexpr int KS = sa_k_row_floats(DT, DP);
  constexpr int VS = DP + 8;                  // 4 rows apart = 32 banks apart: the two lane halves of a V read do not collide
  constexpr int HQ = DP / 2;
  extern __shared__ __align__(16) float sa_lds[];
  const int LP = (L + 31) & ~31, nt = LP >> 5;
  float* Ks = sa_lds;                         // [LP][KS]
  float* Vs = Ks + LP * KS;                   // [LP][VS]
  float* mb = Vs + LP * VS;                   // [LP]: 0 for a token, -inf for a masked or absent key
  const int tid = threadIdx.x, nthr = blockDim.x, lane = tid & 63, wave = tid >> 6, nw = nthr >> 6;
  const int64_t b = blockIdx.x / H;
  const int head = blockIdx.x % H;
  const int E = H * dh;
  const int64_t rs = (int64_t)3 * E * ES;     // bytes between token rows of qkv
  const char* qrow0 = qkv + (b * L * 3 * E + head * dh) * ES;

  for (int i = tid; i < LP * (KS + VS); i += nthr) sa_lds[i] = 0.0f;
  for (int j = tid; j < LP; j += nthr) {
    bool ok = j < L;
    if (ok) {
      switch (mask_kind) {
        case MM_MASK_LEN_I32: ok = j < ((const int32_t*)mask)[b]; break;
        case MM_MASK_U8: ok = ((const uint8_t*)mask)[b * L + j] != 0; break;
        case MM_MASK_I64: ok = ((const int64_t*)mask)[b * L + j] != 0; break;
        case MM_MASK_F32: ok = ((const float*)mask)[b * L + j] != 0.0f; break;
        default: break;
      }
    }
    mb[j] = ok ? 0.0f : neg_inf();
  }
  __syncthreads();
  if constexpr (DT == MM_F32)
    SA_WITH_CB(cb, (sa_stage<DT, CB>(qrow0 + (int64_t)E * ES, qrow0 + (int64_t)2 * E * ES, rs, L, dh, Ks, KS, Vs, VS, tid, nthr)));
  else
    SA_WITH_CB(cb, (sa_stage16<DT, CB>(qrow0 + (int64_t)E * ES, qrow0 + (int64_t)2 * E * ES, rs, L, dh, (uint16_t*)Ks, 2 * KS, Vs, VS,
                                       tid, nthr)));
  __syncthreads();

  const int r = lane & 31, half = lane >> 5;
  // the k index of the score product pairs column c with column hd + c: the first lane half walks [0, hd), the second [hd, 2 hd)
  // (hd a multiple of 8 elements, the widest chunk: the pairing, and with it the accumulation order, does not depend on cb)
  const int hd = (((dh + 1) >> 1) + 7) & ~7;
  for (int qb = wave; qb < nt; qb += nw) {
    const int row = 32 * qb + r;
    const bool row_ok = row < L;
    f32x16 s[NT];
    if constexpr (DT == MM_F32) {
      float q[HQ];
      SA_WITH_CB(cb, (sa_load_q<DT, CB, HQ>(qrow0 + row * rs, row_ok, half, hd, dh, q)));
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        if (t < nt) {
          f32x16 acc = {0};
          const float* kr = Ks + (32 * t + r) * KS + half * hd;
#pragma unroll
          for (int c = 0; c < HQ; ++c)
            if (c < hd) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(kr[c], q[c], acc, 0, 0, 0);
          s[t] = acc;
        }
      }
    } else {      // v_mfma_f32_32x32x16_{f16,bf16}: every product exact in fp32, the k index is the column itself
      constexpr int NC = DP / 16;
      short8 q[NC];
      SA_WITH_CB(cb, (sa_load_q16<CB, NC>(qrow0 + row * rs, row_ok, half, dh, q)));
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        if (t < nt) {
          f32x16 acc = {0};
          const uint16_t* kr = (const uint16_t*)Ks + (32 * t + r) * (2 * KS) + 8 * half;
#pragma unroll
          for (int c = 0; c < NC; ++c)
            if (16 * c < dh) acc = Mfma32x16<DT == MM_F32 ? MM_BF16 : DT>::run(*(const short8*)(kr + 16 * c), q[c], acc);
          s[t] = acc;
        }
      }
    }

    float m = neg_inf();
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      if (t < nt) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const float y = fmaf(s[t][i], c2, mb[32 * t + rowof(i) + 4 * half]);
          s[t][i] = y;
          m = fmaxf(m, y);
        }
      }
    }
    m = fmaxf(m, __shfl_xor(m, 32, 64));
    const float ms = m == neg_inf() ? 0.0f : m;      // no unmasked key: every weight is exp2(-inf) = 0
    float l = 0.0f;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      if (t < nt) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const float p = __builtin_amdgcn_exp2f(s[t][i] - ms);
          s[t][i] = p;
          l += p;
        }
      }
    }
    l += __shfl_xor(l, 32, 64);

    f32x16 o0 = {0}, o1 = {0};
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      if (t < nt) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const float* vr = Vs + (32 * t + rowof(i) + 4 * half) * VS + r;
          o0 = __builtin_amdgcn_mfma_f32_32x32x2f32(vr[0], s[t][i], o0, 0, 0, 0);
          if constexpr (DP == 64) o1 = __builtin_amdgcn_mfma_f32_32x32x2f32(vr[32], s[t][i], o1, 0, 0, 0);
        }
      }
    }

    if (row_ok) {
      char* orow = out + ((b * L + row) * E + head * dh) * ES;
      SA_WITH_CB(cb, (sa_store_tile<DT, CB>(orow, o0, l, half, 0, dh)));
      if constexpr (DP == 64) SA_WITH_CB(cb, (sa_store_tile<DT, CB>(orow, o1, l, half, 32, dh)));
    }
  }
}

static bool sa_supported(int dtype, int L, int H, int dh) {
  if (dtype != MM_F32 && dtype != MM_F16 && dtype != MM_BF16) return false;
  if (L < 1 || H < 1 || dh < 1 || (int64_t)H * dh > (1 << 20)) return false;
  if (dtype != MM_F32 && (dh & 1)) return false;
  return dh <= kSaMaxDh && L <= kSaMaxL;
}

template <int DT, int DP, int NT>
static int sa_launch(const void* qkv, const void* mask, int mask_kind, int B, int L, int H, int dh, int cb, float c2, void* out,
                     hipStream_t stream) {
  const size_t lds = sa_lds_bytes(L, DP, DT);
  if (lds > 64 * 1024) {
    const hipError_t e = hipFuncSetAttribute((const void*)self_attention_kernel<DT, DP, NT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess)
      return set_error(MM_ELAUNCH, "self_attention: %d bytes of dynamic LDS refused: %s", (int)lds, hipGetErrorString(e));
  }
  const int nt = (L + 31) / 32;
  hipLaunchKernelGGL((self_attention_kernel<DT, DP, NT>), dim3((unsigned)((int64_t)B * H)), dim3(64 * (nt < 4 ? nt : 4)), lds, stream,
                     (const char*)qkv, mask, mask_kind, L, H, dh, cb, c2, (char*)out);
  return check_launch("self_attention_kernel");
}

}  // namespace mm

using namespace mm;

extern "C" int mm_self_attention_supported(int dtype, int L, int H, int dh) { return sa_supported(dtype, L, H, dh) ? 1 : 0; }

extern "C" int mm_self_attention_fwd(const void* qkv, int dtype, const void* mask, int mask_kind, int B, int L, int H, int dh,
                                     void* out, void* stream_) {
  if (dtype != MM_F32 && dtype != MM_F16 && dtype != MM_BF16) return set_error(MM_EINVAL, "self_attention: unknown dtype %d", dtype);
  if (B < 0 || L < 0 || H < 1 || dh < 1) return set_error(MM_EINVAL, "self_attention: B=%d L=%d H=%d dh=%d", B, L, H, dh);
  if (mask_kind != MM_MASK_NONE && mask_kind != MM_MASK_LEN_I32 && mask_kind != MM_MASK_U8 && mask_kind != MM_MASK_I64 &&
      mask_kind != MM_MASK_F32)
    return set_error(MM_EINVAL, "self_attention: unknown mask kind %d", mask_kind);
  if (!sa_supported(dtype, L, H, dh))
    return set_error(MM_EUNSUPPORTED,
                     "self_attention: L=%d H=%d dh=%d dtype=%d outside 1 <= L <= %d, 1 <= dh <= %d, dh even for 16-bit types", L, H, dh,
                     dtype, kSaMaxL, kSaMaxDh);
  if (B == 0) return MM_OK;
  if ((int64_t)B * H > 0x7fffffffLL) return set_error(MM_EUNSUPPORTED, "self_attention: B * H = %lld workgroups", (long long)B * H);
  if (!qkv || !out || (mask_kind != MM_MASK_NONE && !mask)) return set_error(MM_EINVAL, "self_attention: null pointer");
  const int es = dtype == MM_F32 ? 4 : 2;
  const uintptr_t bits = (uintptr_t)qkv | (uintptr_t)out;
  if (bits % es) return set_error(MM_EINVAL, "self_attention: qkv and out must be aligned to their element type");
  const uintptr_t all = bits | (uintptr_t)((int64_t)H * dh * es) | (uintptr_t)(dh * es);
  const int cb = all % 16 == 0 ? 16 : all % 8 == 0 ? 8 : all % 4 == 0 ? 4 : 2;
  const float c2 = (float)(1.4426950408889634 / sqrt((double)dh));      // log2(e) / sqrt(dh): the softmax runs on exp2
  hipStream_t stream = (hipStream_t)stream_;
  return with_dtype(dtype, [&](auto dt) {
    constexpr int DT = MM_V(dt);
    if (L <= 128)
      return dh <= 32 ? sa_launch<DT, 32, 4>(qkv, mask, mask_kind, B, L, H, dh, cb, c2, out, stream)
                      : sa_launch<DT, 64, 4>(qkv, mask, mask_kind, B, L, H, dh, cb, c2, out, stream);
    return dh <= 32 ? sa_launch<DT, 32, kSaMaxL / 32>(qkv, mask, mask_kind, B, L, H, dh, cb, c2, out, stream)
                    : sa_launch<DT, 64, kSaMaxL / 32>(qkv, mask, mask_kind, B, L, H, dh, cb, c2, out, stream);
  });
}
