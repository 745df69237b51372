// MatchPyramid (matchmaker/models/matchpyramid.py:74-92): cosine match matrix -> L x (pad, Conv2d, ReLU, AdaptiveMaxPool2d)
// -> the flattened features, fused.  ONE launch per call; a persistent grid of workgroups (four wavefronts each), workgroup g
// takes pairs g, g + grid, ..; it goes layer by layer and keeps every activation plane in LDS when it fits, otherwise in its
// own slice ("slot") of the workspace.  The number of slots is bounded, so the workspace does not grow with the batch.
//
// Arithmetic:
//   cosine   the PACRR family's block (pacrr_device.h): <q_i, d_j> * 1/(|q_i| + 1e-13) * 1/(|d_j| + 1e-13), the dot on
//            v_mfma_f32_32x32x2_f32, the four wavefronts split E and their partial tiles are summed in fixed order;
//   conv     an im2col product [C_l x C_{l-1} kh kw] x [C_{l-1} kh kw x 16 positions] on v_mfma_f32_16x16x4_f32 (exact fp32, a
//            k-ordered fma chain), k = (in-channel, kernel row, kernel column) in the weight tensor's own order, the accumulator
//            initialised with the bias;
//   pooling  a wavefront owns (pooled row, group of pooled columns): it walks the conv rows of the row window two at a time
//            (two independent accumulator chains) and keeps max(0, .) of them in registers (ReLU + the row max), then takes the
//            column-window max from a wavefront-private 32 x 16 tile in LDS.  Every pooled element is written once, by one
//            wavefront: no atomics, and a pair's result depends on nothing but the pair.
// Planes are stored WITH the consumer's zero padding (ConstantPad2d: k[0] - 1 columns right, k[1] - 1 rows below), so the
// im2col loads need no bounds checks: element k of a window is at a per-layer table offset from the window's corner.
//
// Two instantiations of one kernel template: the generic one (every shape of the envelope, run-time kernel sizes, planes
// behind generic pointers) and the reference-config one (3 x 3 kernels, 16 channels, plane 0 and planes >= 2 in LDS, plane 1
// in the workspace: address spaces and trip counts known at compile time).  Both run the same per-element instruction
// sequence, so their results are bit-equal; MM_MP_GENERIC=1 selects the generic one.
#include <algorithm>

#include "pacrr_device.h"

namespace mm {

namespace {

using pacrr_dev::cosine_block_finish;
using pacrr_dev::cosine_block_partials;
using pacrr_dev::query_rnorms;

constexpr int kMpLmax = 8, kMpCmax = 32, kMpKmax = 5, kMpQmax = 64, kMpDmax = 2048, kMpEmax = 1024, kMpPHmax = 64,
              kMpPWmax = 256;
constexpr int kSlack = 16;            // floats past a plane: a 16-column tile may start at the plane's last column
constexpr int kScr = 32 * 17;         // wavefront-private tile [32 channels][16 columns + 1]
constexpr int kKoff = kMpCmax * kMpKmax * kMpKmax;   // im2col offsets of one layer
constexpr int kWt = 5600;             // floats of LDS for one layer's weights (32 channels x (16 x 9 + 1) and below)
constexpr int kFixed = 64 + 32 + 256; // rq, rd, dn
constexpr int kUnion = 4 * kScr + kKoff + kWt;   // the cosine's partial tiles (<= 8 x 32 x 33) alias scratch + offsets + weights
constexpr int kLdsFloats = 160 * 1024 / 4;
constexpr int kArenaMax = kLdsFloats - kFixed - kUnion;
constexpr size_t kWsBudget = (size_t)256 << 20;   // workspace bound: slots x slot size

static_assert(kUnion >= 8 * 32 * 33, "partial tiles must fit the union region");

__device__ __forceinline__ f32x4 mfma16(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

struct MpLayer {
  int C, Cin, kh, kw, K;      // conv [C, Cin, kh, kw]; K = Cin kh kw
  int Hp, Wp;                 // input plane as stored: H + kw - 1 rows, W + kh - 1 columns (the reference's transposed pad)
  int Hc, Wc;                 // conv output
  int oh, ow;                 // pooled output
  int YHp, YWp;               // output plane as stored (the next layer's padding; oh, ow for the last layer)
  int G, ngroups, multi;      // pooled columns per work item; multi: one pooled column whose window spans several tiles
  int x_off, x_lds;           // input plane: offset in the LDS arena or in the slot
  int y_off, y_lds;           // output plane (unused for the last layer: it goes to `out`)
  int w_off, b_off, w_lds;    // offsets into the packed weights / biases; weights staged in LDS
};

struct MpArgs {
  const float* q;
  const float* d;
  const float* w;
  const float* b;
  float* out;
  float* ws;
  int64_t n_pairs, ppq, slot_floats;
  int Q, D, E, L, feat;
  MpLayer lay[kMpLmax];
};

// One layer for one pair.  X: the stored input plane, Y: the stored output plane (row stride YWp, channel stride YHp YWp).
template <bool FAST>
__device__ __forceinline__ void conv_pool_layer(const MpLayer& g, const float* X, float* Y, const float* wt, int wstride,
                                                const float* bias, const int* koff, float* scr, int w, int lane) {
  const int n = lane & 15, kq = lane >> 4;
  const int C = FAST ? 16 : g.C, K = g.K, steps = (K + 3) >> 2, Wp = g.Wp;
  const int nct = FAST ? 1 : (C + 15) >> 4;
  const bool guard = FAST ? false : !g.w_lds;
  const int Hc = g.Hc, Wc = g.Wc, oh = g.oh, ow = g.ow, G = g.G, ngroups = g.ngroups;
  const int items = oh * ngroups;
  f32x4 bias0, bias1;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int ch = 4 * kq + e;
    bias0[e] = ch < C ? bias[ch] : 0.0f;
    bias1[e] = 16 + ch < C ? bias[16 + ch] : 0.0f;
  }
  for (int it = w; it < items; it += 4) {
    const int i = it / ngroups, gi = it - i * ngroups;
    const int j0 = gi * G, j1 = min(j0 + G, ow);
    const int r0 = (i * Hc) / oh, r1 = ((i + 1) * Hc + oh - 1) / oh;
    const int cbeg = (j0 * Wc) / ow, cend = (j1 * Wc + ow - 1) / ow;
    float run = 0.0f;
    for (int c = cbeg; c < cend; c += 16) {
      f32x4 m0 = {0.0f, 0.0f, 0.0f, 0.0f}, m1 = {0.0f, 0.0f, 0.0f, 0.0f};   // ReLU: the max starts at 0
      for (int r = r0; r < r1; r += 2) {
        const int rb = r + 1 < r1 ? r + 1 : r;
        const float* x0 = X + r * Wp + c + n;
        const float* x1 = X + rb * Wp + c + n;
        f32x4 a00 = bias0, a01 = bias0, a10 = bias1, a11 = bias1;
        for (int s = 0; s < steps; ++s) {
          const int k = 4 * s + kq;
          const int o = koff[k];
          const float b0 = x0[o], b1 = x1[o];
          const float w0 = (!guard || (k < K && n < C)) ? wt[n * wstride + k] : 0.0f;
          a00 = mfma16(w0, b0, a00);
          a01 = mfma16(w0, b1, a01);
          if (nct > 1) {
            const float w1 = (!guard || (k < K && 16 + n < C)) ? wt[(16 + n) * wstride + k] : 0.0f;
            a10 = mfma16(w1, b0, a10);
            a11 = mfma16(w1, b1, a11);
          }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          m0[e] = fmaxf(m0[e], fmaxf(a00[e], a01[e]));
          m1[e] = fmaxf(m1[e], fmaxf(a10[e], a11[e]));
        }
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        scr[(4 * kq + e) * 17 + n] = m0[e];
        if (nct > 1) scr[(16 + 4 * kq + e) * 17 + n] = m1[e];
      }
      __builtin_amdgcn_wave_barrier();
      if (!FAST && g.multi) {
        if (lane < C) {
          const int hi = min(cend, c + 16);
          for (int col = c; col < hi; ++col) run = fmaxf(run, scr[lane * 17 + col - c]);
        }
      } else {
        const int Gn = j1 - j0;
        for (int p = lane; p < C * Gn; p += 64) {
          const int ch = p / Gn, j = j0 + p - ch * Gn;
          const int lo = (j * Wc) / ow, hi = ((j + 1) * Wc + ow - 1) / ow;
          float m = 0.0f;
          for (int col = lo; col < hi; ++col) m = fmaxf(m, scr[ch * 17 + col - c]);
          Y[(ch * g.YHp + i) * g.YWp + j] = m;
        }
      }
      __builtin_amdgcn_wave_barrier();
    }
    if (!FAST && g.multi && lane < C) Y[(lane * g.YHp + i) * g.YWp + j0] = run;
  }
}

template <bool FAST>
__global__ void __launch_bounds__(256) matchpyramid_kernel(MpArgs a) {
  extern __shared__ float lds[];
  const int Q = a.Q, D = a.D, E = a.E, L = a.L;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  float* rq = lds;
  float* rd = lds + 64;
  float* dn = lds + 96;
  float* part = lds + kFixed;                       // cosine phase only
  float* scr = lds + kFixed + w * kScr;
  int* koff = (int*)(lds + kFixed + 4 * kScr);
  float* wt = lds + kFixed + 4 * kScr + kKoff;
  float* arena = lds + kFixed + kUnion;
  float* slot = a.ws ? a.ws + (int64_t)blockIdx.x * a.slot_floats : nullptr;
  const int nb = (D + 31) / 32;

  for (int64_t pair = blockIdx.x; pair < a.n_pairs; pair += gridDim.x) {
    const float* q = a.q + (pair / a.ppq) * (int64_t)Q * E;
    const float* d = a.d + pair * (int64_t)D * E;
    const MpLayer& g0 = a.lay[0];
    float* X0 = (FAST || g0.x_lds) ? arena + g0.x_off : slot + g0.x_off;
    const int Wp0 = g0.Wp;
    __syncthreads();                                  // the previous pair's last layer still reads its planes and weights

    // ---- plane 0: zero padding, query norms (one wavefront per row)
    for (int i = tid; i < Q * (Wp0 - D); i += 256) {
      const int r = i / (Wp0 - D);
      X0[r * Wp0 + D + i - r * (Wp0 - D)] = 0.0f;
    }
    for (int i = tid; i < (g0.Hp - Q) * Wp0; i += 256) X0[Q * Wp0 + i] = 0.0f;
    query_rnorms(q, Q, E, rq, w, lane);
    __syncthreads();

    // ---- cosine, 32 document columns per step (the PACRR family's block, pacrr_device.h), written to plane 0
    for (int s = 0; s < nb; ++s) {
      const int j0 = 32 * s;
      cosine_block_partials(q, d, Q, D, E, j0, part, dn, w, lane);
      __syncthreads();
      cosine_block_finish(Q, part, dn, rq, rd, tid, [&](int i, int j, float v) {
        if (j0 + j < D) X0[i * Wp0 + j0 + j] = v;
      });
      __syncthreads();
    }

    // ---- the pyramid
    for (int l = 0; l < L; ++l) {
      const MpLayer& g = a.lay[l];
      const bool last = l == L - 1;
      const int K = g.K, Kr = (K + 3) & ~3, kh = FAST ? 3 : g.kh, kw = FAST ? 3 : g.kw;
      const bool wl = FAST || g.w_lds;
      const int wstride = wl ? Kr + 1 : K;
      const float* wg = a.w + g.w_off;
      // im2col offsets ((in-channel, kernel row, kernel column) -> stored plane), zero for the tail of the last step
      for (int k = tid; k < Kr; k += 256) {
        int o = 0;
        if (k < K) {
          const int ci = k / (kh * kw), rem = k - ci * kh * kw, ka = rem / kw, kb = rem - ka * kw;
          o = (ci * g.Hp + ka) * g.Wp + kb;
        }
        koff[k] = o;
      }
      if (wl) {
        const int rows = FAST ? 16 : ((g.C + 15) & ~15);
        for (int i = tid; i < rows * (Kr + 1); i += 256) {
          const int ch = i / (Kr + 1), k = i - ch * (Kr + 1);
          wt[i] = (ch < g.C && k < K) ? wg[ch * K + k] : 0.0f;
        }
      }
      float* Y;
      if (last) {
        Y = a.out + pair * (int64_t)a.feat;
      } else {
        if (FAST) Y = l == 0 ? slot + g.y_off : arena + g.y_off;
        else Y = g.y_lds ? arena + g.y_off : slot + g.y_off;
        // the next layer's padding: right columns of every stored row, then the rows below
        const int pw = g.YWp - g.ow, ph = g.YHp - g.oh;
        for (int i = tid; i < g.C * g.oh * pw; i += 256) {
          const int row = i / pw, cc = i - row * pw, ch = row / g.oh, rr = row - ch * g.oh;
          Y[(ch * g.YHp + rr) * g.YWp + g.ow + cc] = 0.0f;
        }
        for (int i = tid; i < g.C * ph * g.YWp; i += 256) {
          const int ch = i / (ph * g.YWp), rem = i - ch * ph * g.YWp;
          Y[(ch * g.YHp + g.oh) * g.YWp + rem] = 0.0f;
        }
      }
      __syncthreads();
      const float* wp = wl ? wt : wg;
      const float* bp = a.b + g.b_off;
      if (FAST) {
        // address spaces known here: plane 0 and planes >= 2 in LDS, plane 1 in the slot
        if (l == 0) conv_pool_layer<true>(g, arena + g.x_off, Y, wp, wstride, bp, koff, scr, w, lane);
        else if (l == 1) conv_pool_layer<true>(g, slot + g.x_off, Y, wp, wstride, bp, koff, scr, w, lane);
        else conv_pool_layer<true>(g, arena + g.x_off, Y, wp, wstride, bp, koff, scr, w, lane);
      } else {
        const float* X = g.x_lds ? arena + g.x_off : slot + g.x_off;
        conv_pool_layer<false>(g, X, Y, wp, wstride, bp, koff, scr, w, lane);
      }
      __syncthreads();
    }
  }
}

struct MpPlan {
  MpArgs a;
  int arena_floats;     // LDS arena actually used
  bool fast;
};

int64_t plane_floats(int C, int Hp, int Wp) { return (int64_t)C * Hp * Wp + kSlack; }

// Validates the shape and lays out planes, weights and work groups.  layers: n_layers x (C, k0, k1, ph, pw) on the host.
int make_plan(int Q, int D, int E, int L, const int32_t* layers, MpPlan* P, const char* what) {
  if (L < 1 || L > kMpLmax || Q < 1 || Q > kMpQmax || D < 1 || D > kMpDmax || E < 4 || E > kMpEmax || E % 4)
    return set_error(MM_EUNSUPPORTED,
                     "%s: Q = %d, D = %d, E = %d, layers = %d outside 1 <= Q <= 64, 1 <= D <= 2048, 4 <= E <= 1024 (a multiple "
                     "of 4), 1 <= layers <= 8",
                     what, Q, D, E, L);
  MpArgs& a = P->a;
  a.Q = Q; a.D = D; a.E = E; a.L = L;
  int H = Q, W = D, Cin = 1, w_off = 0, b_off = 0;
  int64_t size[kMpLmax];
  for (int l = 0; l < L; ++l) {
    const int32_t* s = layers + 5 * l;
    MpLayer& g = a.lay[l];
    g.C = s[0]; g.kh = s[1]; g.kw = s[2]; g.oh = s[3]; g.ow = s[4]; g.Cin = Cin;
    if (g.C < 1 || g.C > kMpCmax || g.kh < 1 || g.kh > kMpKmax || g.kw < 1 || g.kw > kMpKmax || g.oh < 1 ||
        g.oh > kMpPHmax || g.ow < 1 || g.ow > kMpPWmax)
      return set_error(MM_EUNSUPPORTED,
                       "%s: layer %d has %d channels, kernel %d x %d, pool %d x %d outside 1 <= channels <= 32, kernel sides "
                       "1 .. 5, pool <= 64 x 256",
                       what, l, g.C, g.kh, g.kw, g.oh, g.ow);
    g.K = Cin * g.kh * g.kw;
    g.Hp = H + g.kw - 1;              // matchpyramid.py:50: the pad is (0, k[0] - 1, 0, k[1] - 1), the kernel k[0] x k[1]
    g.Wp = W + g.kh - 1;
    g.Hc = H + g.kw - g.kh;
    g.Wc = W + g.kh - g.kw;
    if (g.Hc < 1 || g.Wc < 1)
      return set_error(MM_EUNSUPPORTED, "%s: layer %d maps %d x %d to %d x %d", what, l, H, W, g.Hc, g.Wc);
    // pooled columns per work item: the largest group size whose conv columns fit one 16-column tile
    auto clo = [&](int j) { return j * g.Wc / g.ow; };
    auto chi = [&](int j) { return ((j + 1) * g.Wc + g.ow - 1) / g.ow; };
    int G = 1;
    for (int t = g.ow; t >= 1; --t) {
      bool ok = true;
      for (int j0 = 0; j0 < g.ow && ok; j0 += t) ok = chi(std::min(j0 + t, g.ow) - 1) - clo(j0) <= 16;
      if (ok || t == 1) {
        G = t;
        g.multi = ok ? 0 : 1;
        break;
      }
    }
    g.G = G;
    g.ngroups = (g.ow + G - 1) / G;
    g.w_off = w_off; g.b_off = b_off;
    g.w_lds = ((g.C + 15) & ~15) * (((g.K + 3) & ~3) + 1) <= kWt;
    w_off += g.C * g.K;
    b_off += g.C;
    size[l] = plane_floats(Cin, g.Hp, g.Wp);
    H = g.oh; W = g.ow; Cin = g.C;
  }
  a.feat = Cin * H * W;
  for (int l = 0; l < L; ++l) {
    MpLayer& g = a.lay[l];
    g.YHp = l + 1 < L ? a.lay[l + 1].Hp : g.oh;
    g.YWp = l + 1 < L ? a.lay[l + 1].Wp : g.ow;
  }
  // plane p (the input of layer p): LDS when it fits beside its LDS-resident predecessor, else the slot
  bool in_lds[kMpLmax];
  int64_t slot = 0, arena = 0;
  for (int p = 0; p < L; ++p) {
    const int64_t prev = (p > 0 && in_lds[p - 1]) ? size[p - 1] : 0;
    in_lds[p] = size[p] + prev <= kArenaMax;
    if (in_lds[p]) arena = std::max(arena, size[p] + prev);
  }
  for (int p = 0; p < L; ++p) {
    MpLayer& g = a.lay[p];
    g.x_lds = in_lds[p];
    if (in_lds[p]) {
      g.x_off = (p & 1) ? (int)(arena - size[p]) : 0;       // even planes grow from the bottom, odd ones hang from the top
    } else {
      g.x_off = (int)slot;
      slot += size[p];
    }
    if (p > 0) {
      a.lay[p - 1].y_lds = g.x_lds;
      a.lay[p - 1].y_off = g.x_off;
    }
  }
  a.lay[L - 1].y_lds = 0;
  a.lay[L - 1].y_off = 0;
  a.slot_floats = slot;
  P->arena_floats = (int)arena;
  bool fast = L >= 2 && Q <= 32 && D <= 256;
  for (int l = 0; l < L && fast; ++l) {
    const MpLayer& g = a.lay[l];
    fast = g.C == 16 && g.kh == 3 && g.kw == 3 && !g.multi && g.w_lds && g.x_lds == (l != 1);
  }
  P->fast = fast;
  return MM_OK;
}

int lds_bytes(const MpPlan& P) { return (kFixed + kUnion + P.arena_floats) * (int)sizeof(float); }

int64_t n_slots(const MpPlan& P, int64_t n_pairs) {
  const int per_cu = std::max(1, std::min(4, kLdsFloats * 4 / lds_bytes(P)));
  int64_t n = std::min<int64_t>(n_pairs, (int64_t)kCUs * per_cu);
  if (P.a.slot_floats > 0) n = std::min<int64_t>(n, std::max<int64_t>(1, (int64_t)(kWsBudget / (P.a.slot_floats * sizeof(float)))));
  return std::max<int64_t>(n, 1);
}

}  // namespace
}  // namespace mm

using namespace mm;

extern "C" size_t mm_matchpyramid_workspace_bytes(int64_t n_pairs, int Q, int D, int n_layers, const int32_t* layers) {
  if (n_pairs <= 0 || !layers) return 0;
  MpPlan P;
  if (make_plan(Q, D, 4, n_layers, layers, &P, "mm_matchpyramid_workspace_bytes") != MM_OK) return 0;
  return (size_t)n_slots(P, n_pairs) * (size_t)P.a.slot_floats * sizeof(float);
}

extern "C" int mm_matchpyramid_fwd(const float* q, const float* d, const float* conv_w, const float* conv_b, float* features,
                                   int64_t n_pairs, int64_t pairs_per_query, int Q, int D, int E, int n_layers,
                                   const int32_t* layers, void* workspace, size_t workspace_bytes, void* stream) {
  if (!q || !d || !conv_w || !conv_b || !features || !layers)
    return set_error(MM_EINVAL, "mm_matchpyramid_fwd: null q / d / conv_w / conv_b / features / layers");
  if (n_pairs < 0 || pairs_per_query < 1)
    return set_error(MM_EINVAL, "mm_matchpyramid_fwd: n_pairs = %lld, pairs_per_query = %lld", (long long)n_pairs,
                     (long long)pairs_per_query);
  MpPlan P;
  int rc = make_plan(Q, D, E, n_layers, layers, &P, "mm_matchpyramid_fwd");
  if (rc != MM_OK) return rc;
  if (n_pairs == 0) return MM_OK;
  const int64_t slots = n_slots(P, n_pairs);
  const size_t need = (size_t)slots * (size_t)P.a.slot_floats * sizeof(float);
  if (need && (!workspace || workspace_bytes < need))
    return set_error(MM_EWORKSPACE, "mm_matchpyramid_fwd: workspace of %zu bytes, needs %zu", workspace_bytes, need);
  MpArgs& a = P.a;
  a.q = q; a.d = d; a.w = conv_w; a.b = conv_b; a.out = features;
  a.ws = need ? (float*)workspace : nullptr;
  a.n_pairs = n_pairs;
  a.ppq = pairs_per_query;
  const int lds = lds_bytes(P);
  const bool fast = P.fast && !env().mp_generic;
  const void* fn = fast ? (const void*)matchpyramid_kernel<true> : (const void*)matchpyramid_kernel<false>;
  const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
  if (e != hipSuccess)
    return set_error(MM_ELAUNCH, "mm_matchpyramid_fwd: %d bytes of dynamic LDS refused: %s", lds, hipGetErrorString(e));
  if (fast)
    hipLaunchKernelGGL(matchpyramid_kernel<true>, dim3((unsigned)slots), dim3(256), (size_t)lds, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL(matchpyramid_kernel<false>, dim3((unsigned)slots), dim3(256), (size_t)lds, (hipStream_t)stream, a);
  return check_launch("mm_matchpyramid_fwd");
}
