// The element layer below the kernels' phases, one copy of each: float -> bf16 bits, 16-bit bits -> float, one element and one
// 16-byte row chunk of type DT as floats and back, the 32x32x16 MFMA on short8 operands and the generic 32 x 32 similarity tile.
// The fp16 arms are the hardware conversions (v_cvt: nearest even, overflow to inf).  The bf16 rounding is plain C++17 without
// a HIP compiler (tests/test_device_primitives_cpu.py compiles it on its own); the rest needs one.
#pragma once
#include <stdint.h>

#include "launch_geometry.h"

namespace mm {

// float -> bf16 bits, round to nearest even, overflow to inf.  For finite input and infinities: the result for a NaN is
// unspecified (callers that can meet one take bf16_rne_bits_nan).
MM_HD uint32_t bf16_rne_bits(float f) {
  const uint32_t u = __builtin_bit_cast(uint32_t, f);
  return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}
// ... with every NaN as the quiet NaN 0x7fc0
MM_HD uint32_t bf16_rne_bits_nan(float f) { return f != f ? 0x7fc0u : bf16_rne_bits(f); }

}  // namespace mm

#ifdef __HIPCC__
#include "mm_internal.h"

namespace mm {

// v_mfma_f32_32x32x16_{bf16,f16}: 8 elements of k per lane half, as the 16 bytes they are loaded as
template <int DT>
struct Mfma32x16;
template <>
struct Mfma32x16<MM_BF16> {
  static __device__ __forceinline__ f32x16 run(short8 a, short8 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
  }
};
template <>
struct Mfma32x16<MM_F16> {
  static __device__ __forceinline__ f32x16 run(short8 a, short8 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
  }
};

// the bits of a 16-bit element of type DT as a float (exact)
template <int DT>
__device__ __forceinline__ float bits_to_f32(uint16_t b) {
  if constexpr (DT == MM_F16) return (float)__builtin_bit_cast(_Float16, b);
  else return __uint_as_float((uint32_t)b << 16);
}

// element i of an array of type DT as a float; a float rounded once (to nearest even) into element i
template <int DT>
__device__ __forceinline__ float load_elem(const void* base, int64_t i) {
  if constexpr (DT == MM_F32) return ((const float*)base)[i];
  else if constexpr (DT == MM_F16) return (float)((const _Float16*)base)[i];
  else return bits_to_f32<MM_BF16>(((const uint16_t*)base)[i]);
}
template <int DT>
__device__ __forceinline__ void store_elem(void* base, int64_t i, float v) {
  if constexpr (DT == MM_F32) ((float*)base)[i] = v;
  else if constexpr (DT == MM_F16) ((_Float16*)base)[i] = (_Float16)v;
  else ((uint16_t*)base)[i] = (uint16_t)bf16_rne_bits(v);
}
// ... for a dtype known at run time
__device__ __forceinline__ float load_elem(const void* base, int dt, int64_t i) {
  if (dt == MM_F32) return load_elem<MM_F32>(base, i);
  if (dt == MM_F16) return load_elem<MM_F16>(base, i);
  return load_elem<MM_BF16>(base, i);
}

// One 16-byte chunk of a row of type DT as floats (4 for float32 rows, 8 for 16-bit rows), and the matching store of PER floats
// at element `elem` of an array of type GT (16 bytes for 16-bit arrays, 16 or 2 x 16 for float32 ones).
template <int DT>
__device__ __forceinline__ void load_chunk(const char* p, float* v) {
  if constexpr (DT == MM_F32) {
    const f32x4 x = *(const f32x4*)p;
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = x[k];
  } else if constexpr (DT == MM_F16) {
    const f16x8 x = *(const f16x8*)p;
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = (float)x[k];
  } else {
    const short8 x = *(const short8*)p;
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = bits_to_f32<MM_BF16>((uint16_t)x[k]);
  }
}
template <int GT, int PER>
__device__ __forceinline__ void store_chunk(char* base, int64_t elem, const float* v) {
  if constexpr (GT == MM_F32) {
    f32x4* o = (f32x4*)(base + elem * 4);
#pragma unroll
    for (int k = 0; k < PER / 4; ++k) o[k] = f32x4{v[4 * k], v[4 * k + 1], v[4 * k + 2], v[4 * k + 3]};
  } else {
    static_assert(PER == 8, "16-bit arrays are written from 16-bit rows");
    if constexpr (GT == MM_F16) {
      f16x8 o;
#pragma unroll
      for (int k = 0; k < 8; ++k) o[k] = (_Float16)v[k];
      *(f16x8*)(base + elem * 2) = o;
    } else {
      short8 o;
#pragma unroll
      for (int k = 0; k < 8; ++k) o[k] = (short)(uint16_t)bf16_rne_bits(v[k]);
      *(short8*)(base + elem * 2) = o;
    }
  }
}

// <document rows 32t.., query rows 32n..> as one 32 x 32 MFMA tile, any E (16-byte aligned rows), bf16 / f16 / f32: lane (r, h)
// supplies the K chunks of parity h of document row r (A) and query row r (B); C: lane holds query column r, document rows
// rowof(i) + 4h.  K is walked in 16-byte chunks.
template <int DT>
__device__ __forceinline__ f32x16 dot_block(const char* drow, const char* qrow, int E, int h) {
  f32x16 acc = {0};
  if constexpr (DT == MM_F32) {
    // v_mfma_f32_32x32x2_f32: lane (r,h) supplies A[r][k=h].  Chunk pair (2c, 2c+1) -> h=0 takes chunk 2c, h=1 chunk 2c+1; the
    // 4 floats of a chunk are 4 steps.
    const int nch = E >> 2;
    for (int c = 0; c < nch; c += 2) {
      const int cc = c + h;
      f32x4 av = {0, 0, 0, 0}, bv = {0, 0, 0, 0};
      if (cc < nch) {
        av = *(const f32x4*)(drow + cc * 16);
        bv = *(const f32x4*)(qrow + cc * 16);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[j], bv[j], acc, 0, 0, 0);
    }
  } else {
    const int nch = E >> 3;
    // four K steps per trip: their eight 16-byte loads are issued before the first MFMA waits for any of them (the one
    // load pair -> one MFMA form ran a row block as nch / 2 dependent memory round trips); same accumulation order
    for (int c = 0; c < nch; c += 8) {
      short8 av[4], bv[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int cc = c + 2 * u + h;
        av[u] = short8{0, 0, 0, 0, 0, 0, 0, 0};
        bv[u] = av[u];
        if (cc < nch) {
          av[u] = *(const short8*)(drow + cc * 16);
          bv[u] = *(const short8*)(qrow + cc * 16);
        }
      }
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (c + 2 * u < nch) acc = Mfma32x16<DT == MM_F32 ? MM_BF16 : DT>::run(av[u], bv[u], acc);   // wave-uniform
    }
  }
  return acc;
}

}  // namespace mm
#endif
