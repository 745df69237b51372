// Device helpers of the fp8 token store kernels (maxsim_fp8.hip, dot_topk_fp8.hip): code conversion and the LDS-DMA ring slot
// of one-byte elements.  gfx950 only.
#pragma once
#include "mm_internal.h"

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
// each lane one 16-byte chunk of the row's 128-byte slice.  The LDS destination is lane-linear (M0 + lane*16: row-major
// 128-byte rows), so the bank swizzle is applied on the SOURCE side: the chunk stored at slot p of row R is chunk
// p ^ ((R >> 1) & 7).  The A-fragment read of K step kk is a ds_read_b64 of half h of chunk kk of row (lane & 31), at slot
// kk ^ ((R >> 1) & 7).  ds_read_b64 is served in two groups of 32 lanes, and a group has ONE h: its reads touch only the
// 8-byte halves h of the 16-byte chunks, i.e. 32 of the 64 banks, so 32 lanes x 2 banks cannot be conflict-free — 2-way
// is the floor for this layout.  The swizzle reaches it: 8-byte bank pair = 16 (R & 1) + 2 slot + h, and over the 32 rows
// of a group (R & 1, (R >> 1) & 7) takes each of its 16 values exactly twice.  Unswizzled (slot = kk for every row) the
// same read would be 16-way.
// The last instruction moves the row scales (4 bytes per lane, 64 lanes) behind the codes.  Every slice of a block carries
// them, so a slot is always the same number of vector-memory operations and the vmcnt arithmetic stays a multiplication.
template <int ROWS>
__device__ __forceinline__ void issue_slot(const uint8_t* gbase, const uint32_t (&voff)[8], const float* sbase, uint32_t soff,
                                           uint32_t lds_dst) {
  uint32_t keep;
  if constexpr (ROWS == 64) {
    asm volatile(
        "s_waitcnt lgkmcnt(0)\n\t"
        "s_mov_b32 %0, m0\n\t"
        "s_mov_b32 m0, %12\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dwordx4 %1, %10 nt\n\t"
        "s_add_u32 m0, m0, 0x400\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dwordx4 %2, %10 nt\n\t"
        "s_add_u32 m0, m0, 0x400\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dwordx4 %3, %10 nt\n\t"
        "s_add_u32 m0, m0, 0x400\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dwordx4 %4, %10 nt\n\t"
        "s_add_u32 m0, m0, 0x400\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dwordx4 %5, %10 nt\n\t"
        "s_add_u32 m0, m0, 0x400\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dwordx4 %6, %10 nt\n\t"
        "s_add_u32 m0, m0, 0x400\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dwordx4 %7, %10 nt\n\t"
        "s_add_u32 m0, m0, 0x400\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dwordx4 %8, %10 nt\n\t"
        "s_add_u32 m0, m0, 0x400\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dword %9, %11\n\t"
        "s_mov_b32 m0, %0"
        : "=&s"(keep)
        : "v"(voff[0]), "v"(voff[1]), "v"(voff[2]), "v"(voff[3]), "v"(voff[4]), "v"(voff[5]), "v"(voff[6]), "v"(voff[7]),
          "v"(soff), "s"(gbase), "s"(sbase), "s"(lds_dst)
        : "memory", "scc");
  } else {
    asm volatile(
        "s_waitcnt lgkmcnt(0)\n\t"
        "s_mov_b32 %0, m0\n\t"
        "s_mov_b32 m0, %8\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dwordx4 %1, %6 nt\n\t"
        "s_add_u32 m0, m0, 0x400\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dwordx4 %2, %6 nt\n\t"
        "s_add_u32 m0, m0, 0x400\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dwordx4 %3, %6 nt\n\t"
        "s_add_u32 m0, m0, 0x400\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dwordx4 %4, %6 nt\n\t"
        "s_add_u32 m0, m0, 0x400\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dword %5, %7\n\t"
        "s_mov_b32 m0, %0"
        : "=&s"(keep)
        : "v"(voff[0]), "v"(voff[1]), "v"(voff[2]), "v"(voff[3]), "v"(soff), "s"(gbase), "s"(sbase), "s"(lds_dst)
        : "memory", "scc");
  }
}

// Wait until at most `younger` slots (VM vector-memory operations each) issued after the one we need are pending.
template <int VM>
__device__ __forceinline__ void wait_slot(int younger) {
  switch (younger) {
    case 0: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
    case 1: asm volatile("s_waitcnt vmcnt(%0)" ::"n"(VM) : "memory"); break;
    case 2: asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * VM) : "memory"); break;
    default: asm volatile("s_waitcnt vmcnt(%0)" ::"n"(3 * VM) : "memory"); break;
  }
}

}  // namespace mm
