// Device code of the training losses, shared by losses.hip (mm_pair_loss_fwd, mm_list_loss_fwd) and inbatch_loss.hip (the in-batch
// negatives of mm_inbatch_select_loss_fwd / mm_inbatch_dot_loss_fwd): the per-element term of every pair kind, the list-loss body
// with its two policies and kernels, the fixed-order float64 sums.  ONE copy of every loss formula.
#pragma once
#include "mm_internal.h"
#include "elem_device.h"
#include "bitonic_device.h"

namespace mm {

constexpr int kLossMaxList = MM_LOSS_MAX_LIST;
constexpr int kPairShare = 4096;        // elements per workgroup before the grid grows
constexpr int kPairMaxGrid = 1024;      // workgroups (= float64 partials) at most
constexpr float kEps = 1e-6f;           // listnet.py:10, lambdarank.py:4
constexpr float kInvLn2 = 1.44269504088896340736f;
constexpr float kNegLog2Eps = 19.93156857296663f;        // -log2 of the fp32 value 1e-6f

// the fp32 value rounded once (to nearest even) to the scores' dtype; a NaN gradient stays a NaN in bf16 too
__device__ __forceinline__ void st_grad(void* p, int dt, int64_t i, float v) {
  if (dt == MM_F32) store_elem<MM_F32>(p, i, v);
  else if (dt == MM_F16) store_elem<MM_F16>(p, i, v);
  else ((uint16_t*)p)[i] = (uint16_t)bf16_rne_bits_nan(v);
}

// p = sigmoid(x) and q = 1 - p = sigmoid(-x), each to fp32 accuracy at both ends, from one expf
__device__ __forceinline__ void sigmoid2(float x, float* p, float* q) {
  const float e = expf(-fabsf(x));
  const float big = 1.0f / (1.0f + e), small = e / (1.0f + e);
  *p = x >= 0.0f ? big : small;
  *q = x >= 0.0f ? small : big;
}

// max(x, 0) + log1p(exp(-|x|)) = softplus(x) = -log(sigmoid(-x)), accurate at both ends
__device__ __forceinline__ float softplus(float x) { return fmaxf(x, 0.0f) + log1pf(expf(-fabsf(x))); }

// torch.xlogy(t, t): 0 at t == 0, NaN for t < 0 (and NaN)
__device__ __forceinline__ float xlogx(float t) { return t == 0.0f ? 0.0f : t * logf(t); }

__device__ __forceinline__ double wave_sum_f64(double v) {      // the same tree in every lane: all 64 hold the same bits
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// sum over a 256-thread workgroup, the same bits in every thread; red: 4 doubles of LDS.  Two barriers.
__device__ __forceinline__ double block_sum_f64(double v, double* red) {
  v = wave_sum_f64(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  const double t = ((red[0] + red[1]) + red[2]) + red[3];
  __syncthreads();
  return t;
}

// The pairwise kinds are evaluated in float64 per element (a few hundred elements to a few ten thousand: latency-bound).  fp32
// terms miss the bounds this operator is held to in two places: sigmoid(x) - y cancels (a 16-bit gradient must be the rounded
// float64 value to one ulp), and KLDiv's terms of either sign cancel in the mean.
__device__ __forceinline__ void sigmoid2_f64(double x, double* p, double* q) {
  const double e = exp(-fabs(x));
  const double big = 1.0 / (1.0 + e), small = e / (1.0 + e);
  *p = x >= 0.0 ? big : small;
  *q = x >= 0.0 ? small : big;
}
__device__ __forceinline__ double softplus_f64(double x) { return fmax(x, 0.0) + log1p(exp(-fabs(x))); }
__device__ __forceinline__ double xlogx_f64(double t) { return t == 0.0 ? 0.0 : t * log(t); }      // NaN for t < 0, as torch.xlogy

// The per-element term of the pair kinds and its derivatives, p in the `pos` role and g in the `neg` role (the header has the
// table): mm_pair_loss_fwd feeds it (pos_i, neg_i), the in-batch entries (sp_i, S_ij).  x = p - g is exact in float64.
__device__ __forceinline__ void pair_term(int kind, double p, double g, double a, double b, double* term, double* gp, double* gn) {
  const double x = p - g;      // exact
  switch (kind) {
    case MM_PAIR_RANKNET: {
      double s, q;
      sigmoid2_f64(x, &s, &q);
      *term = softplus_f64(x) - x * a;
      *gp = s - a;
      *gn = -*gp;
    } break;
    case MM_PAIR_MARGIN: {
      const double h = 1.0 - a * x;
      *term = fmax(h, 0.0);
      *gp = h >= 0.0 ? -a : 0.0;
      *gn = -*gp;
    } break;
    case MM_PAIR_MARGIN_MSE: {
      const double d = x - (a - b);
      *term = d * d;
      *gp = 2.0 * d;
      *gn = -*gp;
    } break;
    case MM_PAIR_MSE_POINTWISE: {
      const double dp = p - a, dn = g - b;
      *term = 0.5 * (dp * dp + dn * dn);
      *gp = dp;
      *gn = dn;
    } break;
    case MM_PAIR_KLDIV_POINTWISE: {
      *term = 0.5 * ((xlogx_f64(a) - a * p) + (xlogx_f64(b) - b * g));
      *gp = -0.5 * a;
      *gn = -0.5 * b;
    } break;
    case MM_PAIR_RANKNET_TEACHER: {
      double s, q;
      sigmoid2_f64(x, &s, &q);
      const double w = a - b;
      *term = w * softplus_f64(-x);      // sp(x) - x without the cancellation
      *gp = -w * q;                      // (a - b)(sigmoid(x) - 1)
      *gn = -*gp;
    } break;
    default: {      // MM_PAIR_MSE_RANKNET
      double s, q;
      sigmoid2_f64(x, &s, &q);
      const double dp = p - a, dn = g - b;
      *term = 0.5 * (dp * dp + dn * dn) + softplus_f64(-x);
      *gp = dp - q;
      *gn = dn + q;
    } break;
  }
}

// loss = (sum of v[0 .. m)) / denom in float64, one workgroup, fixed order; m == 0 and denom == 0 give 0 / 0 = NaN, which is
// torch.mean of an empty tensor
template <class T>
__global__ void __launch_bounds__(256) loss_finish_kernel(const T* v, int64_t m, double denom, float* loss) {
  __shared__ double red[4];
  double acc = 0.0;
  for (int64_t i = threadIdx.x; i < m; i += 256) acc += (double)v[i];
  acc = block_sum_f64(acc, red);
  if (threadIdx.x == 0) *loss = (float)(acc / denom);
}

// ---- listwise ----------------------------------------------------------------------------------------------------------
// A list is row `list` of a [B, split] matrix followed by row `list` of a [B, L - split] one (the in-batch entries: cat([Sp, Sn], 1)
// without the copy); split == L is one [B, L] matrix and the second pointers are never looked at.
struct ListArgs {
  const void* scores;
  const float* labels;
  int B, L, dtype;
  double inv_B;
  float* per_list;
  void* grad;
  const void* scores2;
  const float* labels2;
  void* grad2;
  int split;
};

enum { SL_S = 0, SL_Y, SL_K, SL_R, SL_G, SL_D, SL_COUNT };      // shared slots: score, label, key, rank, gain, discount delta

// One list per wavefront: entry i lives in lane i, a shared slot is a register, another entry's value is a lane broadcast.
// Every lane runs every loop (there is no early exit), so the source lane of a broadcast is always active.
struct WaveList {
  static constexpr int NPT = 1;
  int lane;
  float slot[SL_COUNT];
  __device__ __forceinline__ int idx(int) const { return lane; }
  __device__ __forceinline__ void share(int s, int, float v) { slot[s] = v; }
  __device__ __forceinline__ float at(int s, int j) const { return __shfl(slot[s], j, 64); }
  __device__ __forceinline__ void sync() const {}
  __device__ __forceinline__ double sum(double v) const { return wave_sum_f64(v); }
  __device__ __forceinline__ float maxf(float v) const {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
  }
  __device__ __forceinline__ int mini(int v) const {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
    return v;
  }
};

// One list per 256-thread workgroup: entry i = tid + 256 k, the shared slots are LDS rows of kLossMaxList floats.
struct BlockList {
  static constexpr int NPT = kLossMaxList / 256;
  int tid;
  float* lds;        // [SL_COUNT][kLossMaxList]
  double* red;       // [4]
  __device__ __forceinline__ int idx(int k) const { return tid + 256 * k; }
  __device__ __forceinline__ void share(int s, int k, float v) { lds[s * kLossMaxList + idx(k)] = v; }
  __device__ __forceinline__ float at(int s, int j) const { return lds[s * kLossMaxList + j]; }
  __device__ __forceinline__ void sync() const { __syncthreads(); }
  __device__ __forceinline__ double sum(double v) const { return block_sum_f64(v, red); }
  __device__ __forceinline__ float maxf(float v) const {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    if ((tid & 63) == 0) red[tid >> 6] = (double)v;
    __syncthreads();
    const float t = fmaxf(fmaxf((float)red[0], (float)red[1]), fmaxf((float)red[2], (float)red[3]));
    __syncthreads();
    return t;
  }
  __device__ __forceinline__ int mini(int v) const {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
    if ((tid & 63) == 0) red[tid >> 6] = (double)v;
    __syncthreads();
    const int t = min(min((int)red[0], (int)red[1]), min((int)red[2], (int)red[3]));
    __syncthreads();
    return t;
  }
};

// softmax over the list in fp32 terms: exp of the shifted value, the float64 sum, one division rounded to fp32; pd: the
// quotient before that rounding (the largest entry's exp is exactly 1, so 1 - p keeps its digits there when p is next to 1)
template <class P>
__device__ __forceinline__ void list_softmax(const P& p, int L, const float (&v)[P::NPT], float (&out)[P::NPT],
                                             double* pd = nullptr) {
  float m = neg_inf();
#pragma unroll
  for (int k = 0; k < P::NPT; ++k)
    if (p.idx(k) < L) m = fmaxf(m, v[k]);
  m = p.maxf(m);
  float e[P::NPT];
  double z = 0.0;
#pragma unroll
  for (int k = 0; k < P::NPT; ++k) {
    e[k] = p.idx(k) < L ? expf(v[k] - m) : 0.0f;
    z += (double)e[k];
  }
  z = p.sum(z);
#pragma unroll
  for (int k = 0; k < P::NPT; ++k) {
    const double r = p.idx(k) < L ? (double)e[k] / z : 0.0;
    out[k] = (float)r;
    if (pd) pd[k] = r;
  }
}

template <class P, int KIND>
__device__ __forceinline__ void list_body(P& p, const ListArgs& A, int list) {
  constexpr int N = P::NPT;
  const int L = A.L;
  float s[N], y[N], g[N];
  bool in[N], second[N];
  int64_t at[N];      // the entry's element of its matrix
#pragma unroll
  for (int k = 0; k < N; ++k) {
    in[k] = p.idx(k) < L;
    second[k] = p.idx(k) >= A.split;
    at[k] = second[k] ? (int64_t)list * (L - A.split) + (p.idx(k) - A.split) : (int64_t)list * A.split + p.idx(k);
    s[k] = in[k] ? load_elem(second[k] ? A.scores2 : A.scores, A.dtype, at[k]) : 0.0f;
    y[k] = in[k] ? (second[k] ? A.labels2 : A.labels)[at[k]] : 0.0f;
    g[k] = 0.0f;
  }
  double lt = 0.0;      // this thread's share of the list's own term

  if constexpr (KIND == MM_LIST_LISTNET || KIND == MM_LIST_KLDIV) {
    float ps[N], T[N], q[N];
    double pd[N];
    list_softmax(p, L, s, ps, pd);
    list_softmax(p, L, y, T);
    double Q = 0.0;
#pragma unroll
    for (int k = 0; k < N; ++k) {
      if (KIND == MM_LIST_LISTNET) {
        // p + eps next to 1 rounds away the digits log() turns into the term: that sum and its log are float64 (O(L) per list)
        q[k] = in[k] ? (float)((double)T[k] * pd[k] / (pd[k] + (double)kEps)) : 0.0f;
        if (in[k]) lt += -((double)T[k] * log(pd[k] + (double)kEps));
      } else {
        q[k] = in[k] ? T[k] * ps[k] : 0.0f;
        if (in[k]) lt += (double)(xlogx(T[k]) - q[k]);
      }
      Q += (double)q[k];
    }
    Q = p.sum(Q);
#pragma unroll
    for (int k = 0; k < N; ++k) g[k] = (float)(-((double)q[k] - (double)ps[k] * Q) * A.inv_B);      // -(1/B) sum_i q_i (d_ik - p_k)
  } else if constexpr (KIND == MM_LIST_SMOOTH_MRR) {
#pragma unroll
    for (int k = 0; k < N; ++k) p.share(SL_S, k, s[k]);
    p.sync();
    double rk[N];
#pragma unroll
    for (int k = 0; k < N; ++k) rk[k] = 0.0;
    for (int j = 0; j < L; ++j) {
      const float sj = p.at(SL_S, j);
#pragma unroll
      for (int k = 0; k < N; ++k) {
        float sg, q;
        sigmoid2(sj - s[k], &sg, &q);
        rk[k] += (double)sg;      // j == i included: 0.5
      }
    }
    float rr[N], best = -1.0f;      // (entries past L: -1, below every real rr >= 0)
#pragma unroll
    for (int k = 0; k < N; ++k) {
      const float rank = (float)(0.5 + rk[k]);
      p.share(SL_R, k, rank);
      rr[k] = !in[k] ? -1.0f : (y[k] > 0.0f ? 1.0f / rank : 0.0f);
      best = fmaxf(best, rr[k]);
    }
    best = p.maxf(best);
    int bi = INT32_MAX;
#pragma unroll
    for (int k = N - 1; k >= 0; --k)
      if (in[k] && rr[k] == best) bi = p.idx(k);
    bi = p.mini(bi);      // STATED CHOICE: the lowest index among tied maxima
    p.sync();
    const bool live = best > 0.0f;      // (an all-zero rr row has gradient 0: rr = 0 / rank there)
    const int b = live ? bi : 0;
    const float sb = L > 0 ? p.at(SL_S, b) : 0.0f, rb = L > 0 ? p.at(SL_R, b) : 1.0f;
    float ds[N];
    double tot = 0.0;
#pragma unroll
    for (int k = 0; k < N; ++k) {
      float sg, q;
      sigmoid2(s[k] - sb, &sg, &q);
      ds[k] = in[k] && p.idx(k) != b ? sg * q : 0.0f;      // d rank_b / d s_k
      tot += (double)ds[k];
    }
    tot = p.sum(tot);
    const double c = live ? A.inv_B / ((double)rb * (double)rb) : 0.0;
#pragma unroll
    for (int k = 0; k < N; ++k) g[k] = (float)((p.idx(k) == b ? -tot : (double)ds[k]) * c);
    lt = p.idx(0) == 0 ? 1.0 - (double)fmaxf(best, 0.0f) : 0.0;
  } else {      // MM_LIST_LAMBDA_NDCG2, MM_LIST_LAMBDA_NDCG2_TEACHER
    if constexpr (KIND == MM_LIST_LAMBDA_NDCG2_TEACHER) {
      float T[N];
      list_softmax(p, L, y, T);
#pragma unroll
      for (int k = 0; k < N; ++k) y[k] = T[k] > 0.001f ? T[k] + 2.0f : T[k];
    } else {
#pragma unroll
      for (int k = 0; k < N; ++k)
        if (y[k] == -1.0f) s[k] = y[k] = neg_inf();      // padded (in registers: the inputs are never modified)
    }
    uint32_t key[N];
#pragma unroll
    for (int k = 0; k < N; ++k) {
      key[k] = desc_key_nan_last(s[k]);      // the key of rank_metrics.hip: descending score, -0 == +0, every NaN behind -inf
      p.share(SL_S, k, s[k]);
      p.share(SL_Y, k, y[k]);
      p.share(SL_K, k, __uint_as_float(key[k]));
    }
    p.sync();
    // rank among the scores (stable descending) and among the labels (descending; tied labels have equal gains)
    int rs[N], ry[N];
#pragma unroll
    for (int k = 0; k < N; ++k) rs[k] = ry[k] = 0;
    for (int j = 0; j < L; ++j) {
      const uint32_t kj = __float_as_uint(p.at(SL_K, j));
      const float yj = p.at(SL_Y, j);
#pragma unroll
      for (int k = 0; k < N; ++k) {
        const bool first = j < p.idx(k);
        rs[k] += (kj < key[k] || (kj == key[k] && first)) ? 1 : 0;
        ry[k] += (yj > y[k] || (yj == y[k] && first)) ? 1 : 0;
      }
    }
    float gain[N];
    double dcg = 0.0;
#pragma unroll
    for (int k = 0; k < N; ++k) {
      gain[k] = in[k] ? exp2f(fmaxf(y[k], 0.0f)) - 1.0f : 0.0f;
      if (in[k]) dcg += (double)gain[k] / log2((double)(ry[k] + 2));
    }
    const float maxdcg = fmaxf((float)p.sum(dcg), kEps);
    float G[N];
#pragma unroll
    for (int k = 0; k < N; ++k) {
      G[k] = gain[k] / maxdcg;
      p.share(SL_R, k, __int_as_float(rs[k]));
      p.share(SL_G, k, G[k]);
      // |1 / D[d - 1] - 1 / D[d]|, D[m] = log2(2 + m), for d = this entry's index: the difference of two reciprocals that agree
      // in ever more digits as d grows, so it is formed in float64 and rounded once (O(L) per list)
      const int d = p.idx(k);
      p.share(SL_D, k, d >= 1 && in[k] ? (float)fabs(1.0 / log2((double)(d + 1)) - 1.0 / log2((double)(d + 2))) : 0.0f);
    }
    p.sync();
    double ga[N];
    bool fin[N];
#pragma unroll
    for (int k = 0; k < N; ++k) {
      ga[k] = 0.0;
      fin[k] = in[k] && fabsf(y[k]) < __builtin_huge_valf();
    }
    for (int j = 0; j < L; ++j) {
      const float sj = p.at(SL_S, j), yj = p.at(SL_Y, j), Gj = p.at(SL_G, j);
      const int rj = __float_as_int(p.at(SL_R, j));
      const bool fj = fabsf(yj) < __builtin_huge_valf();
#pragma unroll
      for (int k = 0; k < N; ++k) {
        int d = rs[k] - rj;
        d = d < 0 ? -d : d;
        const float dl = p.at(SL_D, in[k] ? d : 0);      // (outside every branch: a lane broadcast in the wavefront form)
        if (!(fin[k] && fj) || yj == y[k]) continue;
        const bool mine = y[k] > yj;                     // this entry is the pair's i (the higher label), else its j
        const float w = dl * fabsf(G[k] - Gj);
        float x = mine ? s[k] - sj : sj - s[k];
        x = x != x ? 0.0f : fminf(fmaxf(x, -1e4f), 1e4f);
        float pr, q;
        sigmoid2(x, &pr, &q);
        // -log2(max(max(p, eps)^w, eps)) = min(w * -log2(max(p, eps)), -log2(eps)), and -log2(p) = softplus(-x) / ln 2: the same
        // value without p^w next to 1 (w is 1e-6 .. 1e-1: the power keeps a handful of the term's bits) and without log(p) next to 1
        const float raw = w * (pr >= kEps ? softplus(-x) * kInvLn2 : kNegLog2Eps);
        const float gx = pr >= kEps && raw <= kNegLog2Eps ? -w * q * kInvLn2 : 0.0f;      // p >= eps and p^w >= eps
        if (mine) {
          lt += (double)fminf(raw, kNegLog2Eps);
          ga[k] += (double)gx;
        } else {
          ga[k] -= (double)gx;
        }
      }
    }
#pragma unroll
    for (int k = 0; k < N; ++k) g[k] = (float)ga[k];
  }

  lt = p.sum(lt);
#pragma unroll
  for (int k = 0; k < N; ++k)
    if (in[k]) st_grad(second[k] ? A.grad2 : A.grad, A.dtype, at[k], g[k]);
  if (p.idx(0) == 0) A.per_list[list] = (float)lt;
}

template <int KIND>
__global__ void __launch_bounds__(256) list_loss_wave_kernel(const ListArgs A) {
  const int list = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (list >= A.B) return;      // wave-uniform; this form has no barrier
  WaveList p;
  p.lane = threadIdx.x & 63;
  list_body<WaveList, KIND>(p, A, list);
}

template <int KIND>
__global__ void __launch_bounds__(256) list_loss_block_kernel(const ListArgs A) {
  __shared__ float lds[SL_COUNT * kLossMaxList];
  __shared__ double red[4];
  BlockList p;
  p.tid = threadIdx.x;
  p.lds = lds;
  p.red = red;
  list_body<BlockList, KIND>(p, A, blockIdx.x);
}

template <class F>
inline int with_list_kind(int kind, F&& f) {
  switch (kind) {
    case MM_LIST_LISTNET: return f(Int<MM_LIST_LISTNET>{});
    case MM_LIST_KLDIV: return f(Int<MM_LIST_KLDIV>{});
    case MM_LIST_SMOOTH_MRR: return f(Int<MM_LIST_SMOOTH_MRR>{});
    case MM_LIST_LAMBDA_NDCG2: return f(Int<MM_LIST_LAMBDA_NDCG2>{});
    default: return f(Int<MM_LIST_LAMBDA_NDCG2_TEACHER>{});
  }
}

inline bool loss_dtype_ok(int dtype) { return dtype == MM_F32 || dtype == MM_F16 || dtype == MM_BF16; }

inline bool list_kind_sums(int kind) { return kind == MM_LIST_LAMBDA_NDCG2 || kind == MM_LIST_LAMBDA_NDCG2_TEACHER; }      // reduction="sum"

// the list kernel of `kind` over A (B > 0): one wavefront per list up to 64 entries, one workgroup per list above
inline void launch_list_loss(const ListArgs& A, int kind, hipStream_t stream) {
  with_list_kind(kind, [&](auto k) {
    if (A.L <= 64)
      hipLaunchKernelGGL(list_loss_wave_kernel<MM_V(k)>, dim3((unsigned)((A.B + 3) / 4)), dim3(256), 0, stream, A);
    else
      hipLaunchKernelGGL(list_loss_block_kernel<MM_V(k)>, dim3((unsigned)A.B), dim3(256), 0, stream, A);
    return MM_OK;
  });
}

}  // namespace mm
