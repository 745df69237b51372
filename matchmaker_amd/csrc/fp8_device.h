// Device helpers of the fp8 token store kernels (maxsim_fp8.hip, dot_topk_fp8.hip, store_writer.hip): code conversion, the
// row quantiser and the LDS-DMA ring slot of one-byte elements.  gfx950 only.
#pragma once
#include "mm_internal.h"
#include "lds_dma_device.h"

namespace mm {

typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_t;
typedef __attribute__((ext_vector_type(2))) _Float16 f16x2_t;
typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;
typedef __attribute__((ext_vector_type(2))) uint32_t u32x2;

// 8 e4m3fn codes -> 8 elements of the query's 16-bit type, in memory order (code j of the pair of dwords = element j)
template <int DT>
__device__ __forceinline__ short8 cvt8(u32x2 c) {
  u32x4 o;
  if constexpr (DT == MM_BF16) {
    o[0] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(c[0], 1.0f, false));
    o[1] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(c[0], 1.0f, true));
    o[2] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(c[1], 1.0f, false));
    o[3] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(c[1], 1.0f, true));
  } else {
    o[0] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(c[0], 1.0f, false));
    o[1] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(c[0], 1.0f, true));
    o[2] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(c[1], 1.0f, false));
    o[3] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(c[1], 1.0f, true));
  }
  return __builtin_bit_cast(short8, o);
}

// ---------------------------------------------------------------------------------------------
// Row quantiser (the store format of include/mm_native.h), shared by fp8_quantize_rows_kernel (maxsim_fp8.hip) and the store
// writer's scatter kernel (store_writer.hip).  One 16-lane group per row: a lane owns the 8-element units l, l + 16, ... of
// its row (one 16-byte load of 16-bit input, one 8-byte store of codes), so a dim-128 row is exactly one unit per lane and
// is read once; wider rows re-read the units after the first from L1/L2 in the second pass.
// ---------------------------------------------------------------------------------------------
template <int DT>
__device__ __forceinline__ void load8(const void* row, int u, float (&v)[8]) {
  if constexpr (DT == MM_F32) {
    const f32x4 a = *(const f32x4*)((const char*)row + u * 32), b = *(const f32x4*)((const char*)row + u * 32 + 16);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      v[j] = a[j];
      v[4 + j] = b[j];
    }
  } else if constexpr (DT == MM_F16) {
    const f16x8 s = *(const f16x8*)((const char*)row + u * 16);
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (float)s[j];
  } else {
    const u32x4 s = *(const u32x4*)((const char*)row + u * 16);     // bf16 pairs: the low half is the even element
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      v[2 * j] = __uint_as_float(s[j] << 16);
      v[2 * j + 1] = __uint_as_float(s[j] & 0xffff0000u);
    }
  }
}

__device__ __forceinline__ u32x2 quant8(const float (&v)[8], float inv) {
  // x * inv is exact (inv is a power of two) unless it underflows fp32, far below half of e4m3's smallest subnormal
  int w0 = __builtin_amdgcn_cvt_pk_fp8_f32(v[0] * inv, v[1] * inv, 0, false);
  w0 = __builtin_amdgcn_cvt_pk_fp8_f32(v[2] * inv, v[3] * inv, w0, true);
  int w1 = __builtin_amdgcn_cvt_pk_fp8_f32(v[4] * inv, v[5] * inv, 0, false);
  w1 = __builtin_amdgcn_cvt_pk_fp8_f32(v[6] * inv, v[7] * inv, w1, true);
  return u32x2{(uint32_t)w0, (uint32_t)w1};
}

// Lane l (0..15) of the group that owns the row at xr [E] of type DT: the row's codes to cr [E], its scale to *scale.
// The whole 16-lane group must call it together (the maximum is reduced with shuffles inside the group).
template <int DT>
__device__ __forceinline__ void fp8_quantize_row(const char* xr, int E, int l, uint8_t* cr, float* scale) {
  const int nu = E >> 3;
  float first[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) first[j] = 0.0f;
  float a = 0.0f;
  for (int u = l; u < nu; u += 16) {
    float v[8];
    load8<DT>(xr, u, v);
#pragma unroll
    for (int j = 0; j < 8; ++j) a = fmaxf(a, fabsf(v[j]));
    if (u == l) {
#pragma unroll
      for (int j = 0; j < 8; ++j) first[j] = v[j];
    }
  }
#pragma unroll
  for (int o = 8; o >= 1; o >>= 1) a = fmaxf(a, __shfl_xor(a, o, 64));
  // s = 2^clamp(floor(log2 a) - 7, -126, 120), 1.0 for a zero row.  A subnormal a has exponent field 0 -> -127 - 7 clamps
  // to -126 like its true logarithm would.
  int k = (int)((__float_as_uint(a) >> 23) & 0xffu) - 127 - 7;
  k = k < -126 ? -126 : (k > 120 ? 120 : k);
  if (a == 0.0f) k = 0;
  const float inv = __uint_as_float((uint32_t)(127 - k) << 23);
  if (l == 0) *scale = __uint_as_float((uint32_t)(127 + k) << 23);
  for (int u = l; u < nu; u += 16) {
    if (u == l) {
      *(u32x2*)(cr + u * 8) = quant8(first, inv);
    } else {
      float v[8];
      load8<DT>(xr, u, v);
      *(u32x2*)(cr + u * 8) = quant8(v, inv);
    }
  }
}

// A ring slot holds ROWS token rows x one 128-code slice, and behind them the rows' scales (a 256-byte tail).
// ROWS = 64 (8 KiB of codes, two slots) everywhere but at two query tiles x dim 768, whose 384 registers of B fragments
// leave room for one 32-row accumulator per tile only: ROWS = 32 (4 KiB of codes, four slots — the same bytes in flight).
template <int ROWS>
struct Fp8Slot {
  static constexpr int kCodes = ROWS * 128;
  static constexpr int kBytes = kCodes + 256;
  static constexpr int kInstr = ROWS / 8;       // code instructions per slot
  static constexpr int kVm = kInstr + 1;        // + the scale instruction: vector-memory operations per slot
  static constexpr int kNbuf = 128 / ROWS;      // 16 KiB of codes in flight per wavefront, as the 16-bit kernel keeps
};

// ROWS / 8 + 1 LDS-DMA instructions = one ring slot.  Code instruction k moves 1 KiB, rows 8k..8k+7: 8 lanes per row,
// each lane one 16-byte chunk of the row's 128-byte slice (row-major 128-byte rows in LDS).  Source-side bank swizzle (in
// voff): the chunk stored at slot p of row R is chunk p ^ ((R >> 1) & 7).  The A-fragment read of K step kk is a
// ds_read_b64 of half h of chunk kk of row (lane & 31), at slot kk ^ ((R >> 1) & 7).  ds_read_b64 is served in two groups of 32 lanes, and a group has ONE h: its reads touch only the
// 8-byte halves h of the 16-byte chunks, i.e. 32 of the 64 banks, so 32 lanes x 2 banks cannot be conflict-free — 2-way
// is the floor for this layout.  The swizzle reaches it: 8-byte bank pair = 16 (R & 1) + 2 slot + h, and over the 32 rows
// of a group (R & 1, (R >> 1) & 7) takes each of its 16 values exactly twice.  Unswizzled (slot = kk for every row) the
// same read would be 16-way.
// The last instruction moves the row scales (4 bytes per lane, 64 lanes) behind the codes.  Every slice of a block carries
// them, so a slot is always the same number of vector-memory operations and the vmcnt arithmetic stays a multiplication.
template <int ROWS>
__device__ __forceinline__ void issue_slot(const uint8_t* gbase, const uint32_t (&voff)[8], const float* sbase, uint32_t soff,
                                           uint32_t lds_dst) {
  static_assert(ROWS == 32 || ROWS == 64, "Fp8Slot");
  uint32_t v[ROWS / 8];
#pragma unroll
  for (int n = 0; n < ROWS / 8; ++n) v[n] = voff[n];
  lds_dma_two<0x400, true, false>(gbase, v, sbase, soff, lds_dst);
}

// Wait until at most `younger` slots (VM vector-memory operations each) issued after the one we need are pending.
template <int VM>
__device__ __forceinline__ void wait_slot(int younger) { wait_ring<VM, 3>(younger); }

}  // namespace mm
