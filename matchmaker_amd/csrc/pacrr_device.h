// Device helpers shared by the PACRR family (pacrr.hip, co_pacrr.hip): limits, the packed conv-weight layout, the fp32 MFMA,
// guarded 16-byte loads and the whole-wave sorted top-k insertion.
#pragma once
#include "mm_internal.h"

namespace mm {
namespace pacrr_dev {

constexpr int kPQmax = 64, kPDmax = 2048, kPEmax = 1024, kPCmax = 64, kPNmax = 5, kPKmax = 32;
constexpr float kTiny = 1e-13f;   // allennlp's cosine (mm_native.h, kernel pooling)
constexpr int kPB = 3;           // chunks of 8 elements whose loads a wavefront issues together (cosine phase)
constexpr int kRing = 65;         // ring row stride in floats (64 columns + 1: rows land on distinct banks)

// sum of m^2 for m = 2 .. n - 1: offset of width n's taps in the packed weights (per channel), in units of C floats
__host__ __device__ __forceinline__ int tap_off(int n) { return (n - 1) * n * (2 * n - 1) / 6 - 1; }

__device__ __forceinline__ f32x16 mfma32(float a, float b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}

__device__ __forceinline__ f32x4 load4_or0(const float* p, bool ok) {
  return ok ? *(const f32x4*)p : f32x4{0.0f, 0.0f, 0.0f, 0.0f};
}

// Whole-wave insertion of up to 32 new values (lanes 0..31: v / id of column c0 + lane, `ok` = the column exists) into the
// sorted list held by lanes 0..k-1 (lv / li, cnt entries).  A value enters when the list is not full or when it is STRICTLY
// greater than the k-th: with the columns visited in ascending order, equal values keep the lower column first.
__device__ __forceinline__ void topk_insert(float& lv, int& li, int& cnt, float v, int id, bool ok, int k, int lane) {
  float thr = __shfl(lv, k - 1, 64);
  unsigned long long cand = __ballot(lane < 32 && ok && v == v && (cnt < k || v > thr));
  while (cand) {
    const int c = __builtin_ctzll(cand);
    cand &= cand - 1;
    const float vc = __shfl(v, c, 64);
    const int ic = __shfl(id, c, 64);
    if (cnt == k && !(vc > thr)) continue;
    const int pos = __popcll(__ballot(lane < cnt && lv >= vc));
    const float pv = __shfl(lv, lane > 0 ? lane - 1 : 0, 64);
    const int pi = __shfl(li, lane > 0 ? lane - 1 : 0, 64);
    if (lane == pos) {
      lv = vc;
      li = ic;
    } else if (lane > pos && lane <= cnt && lane < k) {
      lv = pv;
      li = pi;
    }
    cnt = cnt < k ? cnt + 1 : k;
    thr = __shfl(lv, k - 1, 64);
  }
}

}  // namespace pacrr_dev
}  // namespace mm
