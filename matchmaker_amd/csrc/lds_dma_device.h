// LDS-DMA (global_load_lds_*): the issue sequences that feed every streaming kernel's LDS ring, and the counted vmcnt
// waits that tell when a ring slot has landed.  The only place in csrc/ where either is spelled.
//
// One instruction moves 64 lanes x 16 bytes (dwordx4) or x 4 bytes (dword) from global (gbase + voff of the lane
// [+ instruction offset]) to LDS (M0 + instruction offset + lane x 16 or x 4), with no register in between.  The protocol:
//
//   * M0 holds the LDS destination.  The compiler reserves M0 and neither preserves it around a statement nor accepts it as a
//     clobber ("inline asm clobber list contains reserved registers: m0"), so every statement here saves M0 in an SGPR of its
//     own (%[keep], early-clobber), writes it, uses it and restores it before it ends.  M0 is never named as a clobber.
//   * `s_nop 0` after every write of M0: the vector-memory instruction reads M0 one wait state after a scalar write at the
//     earliest (s_mov_b32 or s_add_u32 alike).
//   * `s_waitcnt lgkmcnt(0)` in front wherever a ds_read of the destination slot may still be in flight: the DMA would
//     overwrite what that read has yet to return.  It may be dropped only where every read of the slot was consumed (its
//     result used, or an lgkmcnt wait / LDS barrier passed) before the statement: the group and single forms below.
//   * `scc` is clobbered by every statement that steps M0 with s_add_u32.
//   * The destination is lane-linear: a lane cannot choose where its bytes land, only where they come from.  Bank swizzles
//     and row gathers therefore go on the SOURCE side, into voff.
//   * hipcc does not count these loads: it places no s_waitcnt for them, and __syncthreads() does not wait for them.  The
//     consumer waits itself, with wait_ring / wait_vm below, for exactly the instructions issued after the slot it needs
//     (vector-memory operations of a wavefront retire in issue order), then passes a barrier if other wavefronts read the slot.
//
// A wrapper at the call site says what its kernel moves: the geometry, the swizzle, the ring depth.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mm {

// MM_LDS_REPn(F, A): F(0, A) F(1, A) ... F(n-1, A)
#define MM_LDS_REP0(F, A)
#define MM_LDS_REP1(F, A) F(0, A)
#define MM_LDS_REP2(F, A) MM_LDS_REP1(F, A) F(1, A)
#define MM_LDS_REP3(F, A) MM_LDS_REP2(F, A) F(2, A)
#define MM_LDS_REP4(F, A) MM_LDS_REP3(F, A) F(3, A)
#define MM_LDS_REP5(F, A) MM_LDS_REP4(F, A) F(4, A)
#define MM_LDS_REP6(F, A) MM_LDS_REP5(F, A) F(5, A)
#define MM_LDS_REP7(F, A) MM_LDS_REP6(F, A) F(6, A)
#define MM_LDS_REP8(F, A) MM_LDS_REP7(F, A) F(7, A)
#define MM_LDS_REP9(F, A) MM_LDS_REP8(F, A) F(8, A)
#define MM_LDS_REP10(F, A) MM_LDS_REP9(F, A) F(9, A)
#define MM_LDS_REP11(F, A) MM_LDS_REP10(F, A) F(10, A)
#define MM_LDS_REP12(F, A) MM_LDS_REP11(F, A) F(11, A)
#define MM_LDS_REP13(F, A) MM_LDS_REP12(F, A) F(12, A)

#define MM_LDS_OPEN "s_mov_b32 %[keep], m0\n\ts_mov_b32 m0, %[dst]\n\t"
#define MM_LDS_OPEN_LGKM "s_waitcnt lgkmcnt(0)\n\t" MM_LDS_OPEN
#define MM_LDS_CLOSE "s_mov_b32 m0, %[keep]"
#define MM_LDS_STEP "s_add_u32 m0, m0, %[step]\n\t"
#define MM_LDS_LD(I, NTS) "s_nop 0\n\tglobal_load_lds_dwordx4 %[v" #I "], %[g]" NTS "\n\t"
#define MM_LDS_LD_STEP(I, NTS) MM_LDS_LD(I, NTS) MM_LDS_STEP
#define MM_LDS_V(I, A) [v##I] "v"(voff[I]),

// N loads, M0 stepped after each but the last (LAST: MM_LDS_STEP there as well, or nothing)
#define MM_LDS_STEPPED(N, NM1, NTS, LAST)                                                                               \
  asm volatile(MM_LDS_OPEN_LGKM MM_LDS_REP##NM1(MM_LDS_LD_STEP, NTS) MM_LDS_LD(NM1, NTS) LAST MM_LDS_CLOSE              \
               : [keep] "=&s"(keep)                                                                                     \
               : MM_LDS_REP##N(MM_LDS_V, ) [g] "s"(gbase), [dst] "s"(lds_dst), [step] "n"(STEP)                         \
               : "memory", "scc")
#define MM_LDS_STEPPED_CASE(N, NM1)                                        \
  if constexpr (N_ == N) {                                                 \
    if constexpr (NT && STEP_LAST) MM_LDS_STEPPED(N, NM1, " nt", MM_LDS_STEP); \
    else if constexpr (NT) MM_LDS_STEPPED(N, NM1, " nt", "");              \
    else if constexpr (STEP_LAST) MM_LDS_STEPPED(N, NM1, "", MM_LDS_STEP); \
    else MM_LDS_STEPPED(N, NM1, "", "");                                   \
  }

// Stepped issue: N_ x dwordx4 (nt or plain), instruction n from gbase + voff[n] to lds_dst + n * STEP, behind an lgkmcnt(0)
// wait.  STEP_LAST keeps the (dead) step of M0 behind the last load that the slice and dot kernels have always executed:
// their device code stays what it was.
template <int STEP, bool NT, bool STEP_LAST = false, int N_>
__device__ __forceinline__ void lds_dma(const void* gbase, const uint32_t (&voff)[N_], uint32_t lds_dst) {
  static_assert(N_ == 1 || N_ == 2 || N_ == 3 || N_ == 4 || N_ == 6 || N_ == 8 || N_ == 13, "add a MM_LDS_STEPPED_CASE");
  uint32_t keep;
  MM_LDS_STEPPED_CASE(1, 0)
  MM_LDS_STEPPED_CASE(2, 1)
  MM_LDS_STEPPED_CASE(3, 2)
  MM_LDS_STEPPED_CASE(4, 3)
  MM_LDS_STEPPED_CASE(6, 5)
  MM_LDS_STEPPED_CASE(8, 7)
  MM_LDS_STEPPED_CASE(13, 12)
}

#define MM_LDS_TWO(N, NTS, WIDTH)                                                                                       \
  asm volatile(MM_LDS_OPEN_LGKM MM_LDS_REP##N(MM_LDS_LD_STEP, NTS) "s_nop 0\n\tglobal_load_lds_" WIDTH " %[vt], %[gt]\n\t" \
                   MM_LDS_CLOSE                                                                                         \
               : [keep] "=&s"(keep)                                                                                     \
               : MM_LDS_REP##N(MM_LDS_V, ) [vt] "v"(voff_t), [g] "s"(gbase), [gt] "s"(gbase_t), [dst] "s"(lds_dst),     \
                 [step] "n"(STEP)                                                                                       \
               : "memory", "scc")
#define MM_LDS_TWO_CASE(N)                                             \
  if constexpr (N_ == N) {                                             \
    if constexpr (NT && WIDE_T) MM_LDS_TWO(N, " nt", "dwordx4");       \
    else if constexpr (NT) MM_LDS_TWO(N, " nt", "dword");              \
    else if constexpr (WIDE_T) MM_LDS_TWO(N, "", "dwordx4");           \
    else MM_LDS_TWO(N, "", "dword");                                   \
  }

// Two-base form: the N_ stepped loads of lds_dma, then one plain trailing load from a second base to lds_dst + N_ * STEP:
// a dwordx4 (WIDE_T) or a dword per lane.
template <int STEP, bool NT, bool WIDE_T, int N_>
__device__ __forceinline__ void lds_dma_two(const void* gbase, const uint32_t (&voff)[N_], const void* gbase_t, uint32_t voff_t,
                                            uint32_t lds_dst) {
  static_assert(N_ == 2 || N_ == 4 || N_ == 8, "add a MM_LDS_TWO_CASE");
  uint32_t keep;
  MM_LDS_TWO_CASE(2)
  MM_LDS_TWO_CASE(4)
  MM_LDS_TWO_CASE(8)
}

#define MM_LDS_GROUP(MORE)                                                                                \
  asm volatile(MM_LDS_OPEN "s_nop 0\n\tglobal_load_lds_dwordx4 %[v0], %[g]\n\t" MORE MM_LDS_CLOSE          \
               : [keep] "=&s"(keep)                                                                       \
               : [v0] "v"(voff), [g] "s"(gbase), [dst] "s"(lds_dst)                                       \
               : "memory")
#define MM_LDS_AT(OFF) "global_load_lds_dwordx4 %[v0], %[g] offset:" #OFF "\n\t"

// Offset-group form: N x dwordx4 from gbase + voff + 1024 n to lds_dst + 1024 n.  The instruction offset advances the global
// AND the LDS address, so the group shares one M0 / base pair.  No lgkmcnt wait.
template <int N>
__device__ __forceinline__ void lds_dma_group(const void* gbase, uint32_t voff, uint32_t lds_dst) {
  static_assert(N >= 1 && N <= 4, "instruction offsets reach 3 x 1024");
  uint32_t keep;
  if constexpr (N == 4) MM_LDS_GROUP(MM_LDS_AT(1024) MM_LDS_AT(2048) MM_LDS_AT(3072));
  else if constexpr (N == 3) MM_LDS_GROUP(MM_LDS_AT(1024) MM_LDS_AT(2048));
  else if constexpr (N == 2) MM_LDS_GROUP(MM_LDS_AT(1024));
  else MM_LDS_GROUP("");
}

// Single-instruction form: one dwordx4 per lane, global (gbase + voff) -> LDS (lds_dst + 16 lane).  No lgkmcnt wait.
__device__ __forceinline__ void lds_dma_one(const void* gbase, uint32_t voff, uint32_t lds_dst) {
  lds_dma_group<1>(gbase, voff, lds_dst);
}

// ... and its dword variant: 4 bytes per lane -> LDS (lds_dst + 4 lane), behind an lgkmcnt(0) wait.
__device__ __forceinline__ void lds_dma_one_dword(const void* gbase, uint32_t voff, uint32_t lds_dst) {
  uint32_t keep;
  asm volatile(MM_LDS_OPEN_LGKM "s_nop 0\n\tglobal_load_lds_dword %[v0], %[g]\n\t" MM_LDS_CLOSE
               : [keep] "=&s"(keep)
               : [v0] "v"(voff), [g] "s"(gbase), [dst] "s"(lds_dst)
               : "memory");
}

#undef MM_LDS_AT
#undef MM_LDS_GROUP
#undef MM_LDS_TWO_CASE
#undef MM_LDS_TWO
#undef MM_LDS_STEPPED_CASE
#undef MM_LDS_STEPPED
#undef MM_LDS_V
#undef MM_LDS_LD_STEP
#undef MM_LDS_LD
#undef MM_LDS_STEP
#undef MM_LDS_CLOSE
#undef MM_LDS_OPEN_LGKM
#undef MM_LDS_OPEN
#undef MM_LDS_REP13
#undef MM_LDS_REP12
#undef MM_LDS_REP11
#undef MM_LDS_REP10
#undef MM_LDS_REP9
#undef MM_LDS_REP8
#undef MM_LDS_REP7
#undef MM_LDS_REP6
#undef MM_LDS_REP5
#undef MM_LDS_REP4
#undef MM_LDS_REP3
#undef MM_LDS_REP2
#undef MM_LDS_REP1
#undef MM_LDS_REP0

// s_waitcnt vmcnt(N) for a compile-time N
template <int N>
__device__ __forceinline__ void wait_vm_n() {
  static_assert(N >= 0 && N <= 63, "vmcnt has 6 bits");
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// Ring wait: until at most `younger` slots of PER vector-memory operations each, issued after the one we need, are still
// pending: s_waitcnt vmcnt(PER * min(younger, MAXY)).  MAXY is the most slots a ring can have behind the oldest one; further
// vector-memory operations in the queue (a query tile, a store) only make the wait longer, never shorter.
template <int PER, int MAXY, int Y = 0>
__device__ __forceinline__ void wait_ring(int younger) {
  static_assert(PER * MAXY <= 63, "vmcnt has 6 bits: a deeper ring cannot be counted");
  if constexpr (Y == MAXY) {
    wait_vm_n<PER * MAXY>();
  } else {
    if (younger == Y) wait_vm_n<PER * Y>();
    else wait_ring<PER, MAXY, Y + 1>(younger);
  }
}

// s_waitcnt vmcnt(n) for a wave-uniform run-time n.  n >= 63 needs no wait: the counter has 6 bits, so at most 63
// vector-memory operations are outstanding and anything with that many younger ones behind it has completed.
// On gfx9-family hardware loads and stores of a wavefront retire in issue order (one counter, one event class in
// LLVM's SIInsertWaitcnts for targets without vscnt), so stores may be counted like the LDS-DMA loads around them.
__device__ __forceinline__ void wait_vm(int n) {
  switch (n) {
    case 0: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
    case 1: asm volatile("s_waitcnt vmcnt(1)" ::: "memory"); break;
    case 2: asm volatile("s_waitcnt vmcnt(2)" ::: "memory"); break;
    case 3: asm volatile("s_waitcnt vmcnt(3)" ::: "memory"); break;
    case 4: asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); break;
    case 5: asm volatile("s_waitcnt vmcnt(5)" ::: "memory"); break;
    case 6: asm volatile("s_waitcnt vmcnt(6)" ::: "memory"); break;
    case 7: asm volatile("s_waitcnt vmcnt(7)" ::: "memory"); break;
    case 8: asm volatile("s_waitcnt vmcnt(8)" ::: "memory"); break;
    case 9: asm volatile("s_waitcnt vmcnt(9)" ::: "memory"); break;
    case 10: asm volatile("s_waitcnt vmcnt(10)" ::: "memory"); break;
    case 11: asm volatile("s_waitcnt vmcnt(11)" ::: "memory"); break;
    case 12: asm volatile("s_waitcnt vmcnt(12)" ::: "memory"); break;
    case 13: asm volatile("s_waitcnt vmcnt(13)" ::: "memory"); break;
    case 14: asm volatile("s_waitcnt vmcnt(14)" ::: "memory"); break;
    case 15: asm volatile("s_waitcnt vmcnt(15)" ::: "memory"); break;
    case 16: asm volatile("s_waitcnt vmcnt(16)" ::: "memory"); break;
    case 17: asm volatile("s_waitcnt vmcnt(17)" ::: "memory"); break;
    case 18: asm volatile("s_waitcnt vmcnt(18)" ::: "memory"); break;
    case 19: asm volatile("s_waitcnt vmcnt(19)" ::: "memory"); break;
    case 20: asm volatile("s_waitcnt vmcnt(20)" ::: "memory"); break;
    case 21: asm volatile("s_waitcnt vmcnt(21)" ::: "memory"); break;
    case 22: asm volatile("s_waitcnt vmcnt(22)" ::: "memory"); break;
    case 23: asm volatile("s_waitcnt vmcnt(23)" ::: "memory"); break;
    case 24: asm volatile("s_waitcnt vmcnt(24)" ::: "memory"); break;
    case 25: asm volatile("s_waitcnt vmcnt(25)" ::: "memory"); break;
    case 26: asm volatile("s_waitcnt vmcnt(26)" ::: "memory"); break;
    case 27: asm volatile("s_waitcnt vmcnt(27)" ::: "memory"); break;
    case 28: asm volatile("s_waitcnt vmcnt(28)" ::: "memory"); break;
    case 29: asm volatile("s_waitcnt vmcnt(29)" ::: "memory"); break;
    case 30: asm volatile("s_waitcnt vmcnt(30)" ::: "memory"); break;
    case 31: asm volatile("s_waitcnt vmcnt(31)" ::: "memory"); break;
    case 32: asm volatile("s_waitcnt vmcnt(32)" ::: "memory"); break;
    case 33: asm volatile("s_waitcnt vmcnt(33)" ::: "memory"); break;
    case 34: asm volatile("s_waitcnt vmcnt(34)" ::: "memory"); break;
    case 35: asm volatile("s_waitcnt vmcnt(35)" ::: "memory"); break;
    case 36: asm volatile("s_waitcnt vmcnt(36)" ::: "memory"); break;
    case 37: asm volatile("s_waitcnt vmcnt(37)" ::: "memory"); break;
    case 38: asm volatile("s_waitcnt vmcnt(38)" ::: "memory"); break;
    case 39: asm volatile("s_waitcnt vmcnt(39)" ::: "memory"); break;
    case 40: asm volatile("s_waitcnt vmcnt(40)" ::: "memory"); break;
    case 41: asm volatile("s_waitcnt vmcnt(41)" ::: "memory"); break;
    case 42: asm volatile("s_waitcnt vmcnt(42)" ::: "memory"); break;
    case 43: asm volatile("s_waitcnt vmcnt(43)" ::: "memory"); break;
    case 44: asm volatile("s_waitcnt vmcnt(44)" ::: "memory"); break;
    case 45: asm volatile("s_waitcnt vmcnt(45)" ::: "memory"); break;
    case 46: asm volatile("s_waitcnt vmcnt(46)" ::: "memory"); break;
    case 47: asm volatile("s_waitcnt vmcnt(47)" ::: "memory"); break;
    case 48: asm volatile("s_waitcnt vmcnt(48)" ::: "memory"); break;
    case 49: asm volatile("s_waitcnt vmcnt(49)" ::: "memory"); break;
    case 50: asm volatile("s_waitcnt vmcnt(50)" ::: "memory"); break;
    case 51: asm volatile("s_waitcnt vmcnt(51)" ::: "memory"); break;
    case 52: asm volatile("s_waitcnt vmcnt(52)" ::: "memory"); break;
    case 53: asm volatile("s_waitcnt vmcnt(53)" ::: "memory"); break;
    case 54: asm volatile("s_waitcnt vmcnt(54)" ::: "memory"); break;
    case 55: asm volatile("s_waitcnt vmcnt(55)" ::: "memory"); break;
    case 56: asm volatile("s_waitcnt vmcnt(56)" ::: "memory"); break;
    case 57: asm volatile("s_waitcnt vmcnt(57)" ::: "memory"); break;
    case 58: asm volatile("s_waitcnt vmcnt(58)" ::: "memory"); break;
    case 59: asm volatile("s_waitcnt vmcnt(59)" ::: "memory"); break;
    case 60: asm volatile("s_waitcnt vmcnt(60)" ::: "memory"); break;
    case 61: asm volatile("s_waitcnt vmcnt(61)" ::: "memory"); break;
    case 62: asm volatile("s_waitcnt vmcnt(62)" ::: "memory"); break;
    default: break;
  }
}

}  // namespace mm
