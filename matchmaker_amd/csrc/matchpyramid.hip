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
// sequence, so their results are bit-equal; MM_MP_GENERIC=1 selects the generic one.  A second template flag, SAVE, is the
// training entry (mm_matchpyramid_fwd_save): the same sequence for the values, plus every layer's pooled output and arg-max
// for mm_matchpyramid_bwd at the end of this file.
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
  // the training entry (SAVE): every layer's pooled output and its arg-max, [sv_stride] per pair, layer l at sv_off[l]
  float* sv_pooled;
  int32_t* sv_arg;
  int64_t sv_stride;
  int sv_off[kMpLmax];
  int idx_off;                // the wavefronts' row-index tiles, in floats past the arena
};

// One layer for one pair.  X: the stored input plane, Y: the stored output plane (row stride YWp, channel stride YHp YWp).
// SAVE: the same instruction sequence for the values, and beside it the arg-max of every pooled element — the flat index
// row * Wc + col into the channel's conv output, the FIRST maximum in row-major order of the window (the convention and
// the tie rule of F.adaptive_max_pool2d(return_indices=True)): a candidate replaces the held one when it is larger, or
// equal with a lower flat index.  The held value starts at 0 (ReLU) with the window's first element, so a window without a
// positive value reports that element.  P / A [C, oh, ow]: the pooled values and indices of this pair's layer; iscr: the
// wavefront's row-index tile, laid out like scr.
template <bool FAST, bool SAVE>
__device__ __forceinline__ void conv_pool_layer(const MpLayer& g, const float* X, float* Y, const float* wt, int wstride,
                                                const float* bias, const int* koff, float* scr, int w, int lane, float* P,
                                                int32_t* A, int* iscr) {
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
    int runi = r0 * Wc + cbeg;
    for (int c = cbeg; c < cend; c += 16) {
      f32x4 m0 = {0.0f, 0.0f, 0.0f, 0.0f}, m1 = {0.0f, 0.0f, 0.0f, 0.0f};   // ReLU: the max starts at 0
      int i0[4] = {r0, r0, r0, r0}, i1[4] = {r0, r0, r0, r0};               // SAVE: the first row that holds the column's max
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
        if (SAVE) {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            float t = m0[e];
            if (a00[e] > t) { t = a00[e]; i0[e] = r; }
            if (a01[e] > t) i0[e] = rb;
            if (nct > 1) {
              t = m1[e];
              if (a10[e] > t) { t = a10[e]; i1[e] = r; }
              if (a11[e] > t) i1[e] = rb;
            }
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
        if (SAVE) {
          iscr[(4 * kq + e) * 17 + n] = i0[e];
          if (nct > 1) iscr[(16 + 4 * kq + e) * 17 + n] = i1[e];
        }
      }
      __builtin_amdgcn_wave_barrier();
      if (!FAST && g.multi) {
        if (lane < C) {
          const int hi = min(cend, c + 16);
          for (int col = c; col < hi; ++col) {
            const float v = scr[lane * 17 + col - c];
            if (SAVE) {
              const int f = iscr[lane * 17 + col - c] * Wc + col;
              if (v > run || (v == run && f < runi)) runi = f;
            }
            run = fmaxf(run, v);
          }
        }
      } else {
        const int Gn = j1 - j0;
        for (int p = lane; p < C * Gn; p += 64) {
          const int ch = p / Gn, j = j0 + p - ch * Gn;
          const int lo = (j * Wc) / ow, hi = ((j + 1) * Wc + ow - 1) / ow;
          float m = 0.0f;
          int best = r0 * Wc + lo;
          for (int col = lo; col < hi; ++col) {
            const float v = scr[ch * 17 + col - c];
            if (SAVE) {
              const int f = iscr[ch * 17 + col - c] * Wc + col;
              if (v > m || (v == m && f < best)) best = f;
            }
            m = fmaxf(m, v);
          }
          Y[(ch * g.YHp + i) * g.YWp + j] = m;
          if (SAVE) {
            P[(ch * oh + i) * ow + j] = m;
            A[(ch * oh + i) * ow + j] = best;
          }
        }
      }
      __builtin_amdgcn_wave_barrier();
    }
    if (!FAST && g.multi && lane < C) {
      Y[(lane * g.YHp + i) * g.YWp + j0] = run;
      if (SAVE) {
        P[(lane * oh + i) * ow + j0] = run;
        A[(lane * oh + i) * ow + j0] = runi;
      }
    }
  }
}

template <bool FAST, bool SAVE>
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
  int* iscr = SAVE ? (int*)(arena + a.idx_off) + w * kScr : nullptr;
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
      float* P = SAVE ? a.sv_pooled + pair * a.sv_stride + a.sv_off[l] : nullptr;
      int32_t* A = SAVE ? a.sv_arg + pair * a.sv_stride + a.sv_off[l] : nullptr;
      if (FAST) {
        // address spaces known here: plane 0 and planes >= 2 in LDS, plane 1 in the slot
        if (l == 0) conv_pool_layer<true, SAVE>(g, arena + g.x_off, Y, wp, wstride, bp, koff, scr, w, lane, P, A, iscr);
        else if (l == 1) conv_pool_layer<true, SAVE>(g, slot + g.x_off, Y, wp, wstride, bp, koff, scr, w, lane, P, A, iscr);
        else conv_pool_layer<true, SAVE>(g, arena + g.x_off, Y, wp, wstride, bp, koff, scr, w, lane, P, A, iscr);
      } else {
        const float* X = g.x_lds ? arena + g.x_off : slot + g.x_off;
        conv_pool_layer<false, SAVE>(g, X, Y, wp, wstride, bp, koff, scr, w, lane, P, A, iscr);
      }
      __syncthreads();
    }
  }
}

struct MpPlan {
  MpArgs a;
  int arena_floats;     // LDS arena actually used
  int reserve;          // floats of LDS past the arena (the training entry's row-index tiles)
  bool fast;
};

int64_t plane_floats(int C, int Hp, int Wp) { return (int64_t)C * Hp * Wp + kSlack; }

// Validates the shape and lays out planes, weights and work groups.  layers: n_layers x (C, k0, k1, ph, pw) on the host.
// reserve: floats of LDS the arena leaves free (where a plane lives changes no bit of the result).
int make_plan(int Q, int D, int E, int L, const int32_t* layers, MpPlan* P, const char* what, int reserve = 0) {
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
  a.sv_pooled = nullptr;
  a.sv_arg = nullptr;
  a.sv_stride = 0;
  for (int l = 0; l < L; ++l) {
    a.sv_off[l] = (int)a.sv_stride;
    a.sv_stride += (int64_t)a.lay[l].C * a.lay[l].oh * a.lay[l].ow;
  }
  const int arena_max = kArenaMax - reserve;
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
    in_lds[p] = size[p] + prev <= arena_max;
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
  P->reserve = reserve;
  a.idx_off = (int)arena;
  bool fast = L >= 2 && Q <= 32 && D <= 256;
  for (int l = 0; l < L && fast; ++l) {
    const MpLayer& g = a.lay[l];
    fast = g.C == 16 && g.kh == 3 && g.kw == 3 && !g.multi && g.w_lds && g.x_lds == (l != 1);
  }
  P->fast = fast;
  return MM_OK;
}

int lds_bytes(const MpPlan& P) { return (kFixed + kUnion + P.arena_floats + P.reserve) * (int)sizeof(float); }

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

namespace mm {
namespace {

constexpr int kSaveReserve = 4 * kScr;   // the training entry: one row-index tile per wavefront

// Both forward entries.  pooled / argmax: the training entry's saved state, or null.
int run_fwd(const char* what, const float* q, const float* d, const float* conv_w, const float* conv_b, float* features,
            float* pooled, int32_t* argmax, int64_t n_pairs, int64_t pairs_per_query, int Q, int D, int E, int n_layers,
            const int32_t* layers, void* workspace, size_t workspace_bytes, void* stream) {
  const bool save = pooled != nullptr;
  if (n_pairs < 0 || pairs_per_query < 1)
    return set_error(MM_EINVAL, "%s: n_pairs = %lld, pairs_per_query = %lld", what, (long long)n_pairs,
                     (long long)pairs_per_query);
  MpPlan P;
  int rc = make_plan(Q, D, E, n_layers, layers, &P, what, save ? kSaveReserve : 0);
  if (rc != MM_OK) return rc;
  if (n_pairs == 0) return MM_OK;
  const int64_t slots = n_slots(P, n_pairs);
  const size_t need = (size_t)slots * (size_t)P.a.slot_floats * sizeof(float);
  if (need && (!workspace || workspace_bytes < need))
    return set_error(MM_EWORKSPACE, "%s: workspace of %zu bytes, needs %zu", what, workspace_bytes, need);
  MpArgs& a = P.a;
  a.q = q; a.d = d; a.w = conv_w; a.b = conv_b; a.out = features;
  a.sv_pooled = pooled;
  a.sv_arg = argmax;
  a.ws = need ? (float*)workspace : nullptr;
  a.n_pairs = n_pairs;
  a.ppq = pairs_per_query;
  const int lds = lds_bytes(P);
  const bool fast = P.fast && !env().mp_generic;
  const void* fn = save ? (fast ? (const void*)matchpyramid_kernel<true, true> : (const void*)matchpyramid_kernel<false, true>)
                        : (fast ? (const void*)matchpyramid_kernel<true, false> : (const void*)matchpyramid_kernel<false, false>);
  const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
  if (e != hipSuccess)
    return set_error(MM_ELAUNCH, "%s: %d bytes of dynamic LDS refused: %s", what, lds, hipGetErrorString(e));
  const dim3 grid((unsigned)slots), block(256);
  if (save) {
    if (fast) hipLaunchKernelGGL((matchpyramid_kernel<true, true>), grid, block, (size_t)lds, (hipStream_t)stream, a);
    else hipLaunchKernelGGL((matchpyramid_kernel<false, true>), grid, block, (size_t)lds, (hipStream_t)stream, a);
  } else {
    if (fast) hipLaunchKernelGGL((matchpyramid_kernel<true, false>), grid, block, (size_t)lds, (hipStream_t)stream, a);
    else hipLaunchKernelGGL((matchpyramid_kernel<false, false>), grid, block, (size_t)lds, (hipStream_t)stream, a);
  }
  return check_launch(what);
}

}  // namespace
}  // namespace mm

extern "C" int mm_matchpyramid_fwd(const float* q, const float* d, const float* conv_w, const float* conv_b, float* features,
                                   int64_t n_pairs, int64_t pairs_per_query, int Q, int D, int E, int n_layers,
                                   const int32_t* layers, void* workspace, size_t workspace_bytes, void* stream) {
  if (!q || !d || !conv_w || !conv_b || !features || !layers)
    return set_error(MM_EINVAL, "mm_matchpyramid_fwd: null q / d / conv_w / conv_b / features / layers");
  return run_fwd("mm_matchpyramid_fwd", q, d, conv_w, conv_b, features, nullptr, nullptr, n_pairs, pairs_per_query, Q, D, E,
                 n_layers, layers, workspace, workspace_bytes, stream);
}

extern "C" size_t mm_matchpyramid_fwd_save_workspace_bytes(int64_t n_pairs, int Q, int D, int n_layers, const int32_t* layers) {
  if (n_pairs <= 0 || !layers) return 0;
  MpPlan P;
  if (make_plan(Q, D, 4, n_layers, layers, &P, "mm_matchpyramid_fwd_save_workspace_bytes", kSaveReserve) != MM_OK) return 0;
  return (size_t)n_slots(P, n_pairs) * (size_t)P.a.slot_floats * sizeof(float);
}

extern "C" int mm_matchpyramid_fwd_save(const float* q, const float* d, const float* conv_w, const float* conv_b,
                                        float* features, float* pooled, int32_t* argmax, int64_t n_pairs,
                                        int64_t pairs_per_query, int Q, int D, int E, int n_layers, const int32_t* layers,
                                        void* workspace, size_t workspace_bytes, void* stream) {
  if (!q || !d || !conv_w || !conv_b || !features || !pooled || !argmax || !layers)
    return set_error(MM_EINVAL, "mm_matchpyramid_fwd_save: null q / d / conv_w / conv_b / features / pooled / argmax / layers");
  return run_fwd("mm_matchpyramid_fwd_save", q, d, conv_w, conv_b, features, pooled, argmax, n_pairs, pairs_per_query, Q, D, E,
                 n_layers, layers, workspace, workspace_bytes, stream);
}

// ------------------------------------------------------------------------------------------------------------ backward
// mm_matchpyramid_bwd: from the state mm_matchpyramid_fwd_save left (every layer's pooled output and arg-max) no conv output
// is recomputed.  ONE launch over a persistent grid (a workgroup of sixteen wavefronts takes pairs g, g + grid, ..) and one small
// launch that adds the workgroups' weight / bias partials in workgroup order.  Per pair, from the last layer down:
//   E   eg[c, e] = the pooled element's gradient where pooled > 0, else 0 (ReLU's backward, 0 at 0); ep = its (row, col)
//   G   the conv-output gradient as a dense plane, by GATHER: position (c, r, col) adds, in (i, j) order, the eg of the pooled
//       elements whose window holds it and whose arg-max it is (the windows that hold a position are a contiguous range per
//       axis: floor(r oh / Hc) .. ceil((r + 1) oh / Hc) - 1); stored in a frame of zeros as wide as the kernel
//   W   grad_w[c, k] += sum_e eg In[arg-max_e + k], grad_b[c] += sum_e eg: a thread per output, e in order; In = the saved
//       pooled output of the layer below (the cosine plane for layer 0), zero outside it
//   X   the input gradient, a transposed convolution as a gather over G: (c, kernel row, kernel column) order
// then the cosine's backward through both normalisations (zero rows: only g / (|x| + 1e-13), torch's zero subgradient of the
// norm).  Plain fp32 fma chains in fixed orders, every output element written by one thread: no atomics, bit-reproducible,
// and grad_q / grad_d of a pair depend on nothing but the pair.
namespace mm {
namespace {

struct MpBwdArgs {
  const float* q;
  const float* d;
  const float* w;
  const float* pooled;
  const int32_t* arg;
  const float* go;
  float* gq;
  float* gd;
  float* part;                // [grid, np]: the workgroups' sums of grad_w | grad_b over their pairs, in pair order
  float* slots;               // [grid, slot_floats]
  int64_t n_pairs, ppq, sv_stride, slot_floats;
  int Q, D, E, L, feat, wtot, np;
  int o_cos, o_g0, o_g1, o_G, o_eg, o_ep;   // the slot: cosine plane, two input-gradient planes, G, eg, ep
  int sv_off[kMpLmax];
  MpLayer lay[kMpLmax];
};

constexpr int kBwdStage = 8 * 32 * 33;   // floats of LDS the phases take turns in: cosine partials, weights, tables, coefficient tiles
constexpr int kNT = 1024, kNW = kNT / 64;   // sixteen wavefronts per pair: every phase waits on memory, and a 64-pair batch
                                          // fills a quarter of the CUs (the cosine block keeps its four-wavefront form)

// X: the input gradient of one layer, gin[ci, y, x] = sum over (c, ka, kb) in that order of w[c, ci, ka, kb] Gp[c, y - ka, x - kb].
// Gp is stored with kh - 1 zero rows above and below and kw - 1 zero columns left and right, so no load needs a bounds
// check.  A thread takes two positions and CT input channels at a time: every G value it loads feeds CT fmas and every
// weight (a broadcast LDS read; the layer's weights are staged [c][ka][kb][ci], as many output channels at a time as fit) two.
template <int CT>
__device__ __forceinline__ void input_grad(const MpLayer& g, int H, int W, const float* wsrc, const float* Gp, float* gin,
                                           float* wl, int tid) {
  const int C = g.C, Cin = g.Cin, kh = g.kh, kw = g.kw, kk = kh * kw;
  const int Hg = g.Hc + 2 * (kh - 1), Wg = g.Wc + 2 * (kw - 1);
  const int CinP = (Cin + CT - 1) / CT * CT, HW = H * W;
  const int cmax = max(1, kBwdStage / (kk * CinP));
  for (int c0 = 0; c0 < C; c0 += cmax) {
    const int cn = min(cmax, C - c0);
    __syncthreads();
    for (int i = tid; i < cn * kk * CinP; i += kNT) {
      const int cl = i / (kk * CinP), rem = i - cl * kk * CinP, kidx = rem / CinP, ci = rem - kidx * CinP;
      wl[i] = ci < Cin ? wsrc[((c0 + cl) * Cin + ci) * kk + kidx] : 0.0f;
    }
    __syncthreads();
    for (int pos = tid; pos < HW; pos += 2 * kNT) {
      const int pos2 = pos + kNT < HW ? pos + kNT : pos;
      const int y0 = pos / W, x0 = pos - y0 * W, y1 = pos2 / W, x1 = pos2 - y1 * W;
      const float* G0 = Gp + (c0 * Hg + y0) * Wg + x0;
      const float* G1 = Gp + (c0 * Hg + y1) * Wg + x1;
      for (int ci0 = 0; ci0 < Cin; ci0 += CT) {
        float a0[CT], a1[CT];
#pragma unroll
        for (int t = 0; t < CT; ++t) {
          const bool in = c0 > 0 && ci0 + t < Cin;
          a0[t] = in ? gin[(ci0 + t) * HW + pos] : 0.0f;
          a1[t] = in ? gin[(ci0 + t) * HW + pos2] : 0.0f;
        }
        for (int cl = 0; cl < cn; ++cl)
          for (int ka = 0; ka < kh; ++ka)
            for (int kb = 0; kb < kw; ++kb) {
              const int off = (cl * Hg + kh - 1 - ka) * Wg + kw - 1 - kb;
              const float g0 = G0[off], g1 = G1[off];
              const float* wk = wl + (cl * kk + ka * kw + kb) * CinP + ci0;
#pragma unroll
              for (int t = 0; t < CT; ++t) {
                a0[t] = fmaf(wk[t], g0, a0[t]);
                a1[t] = fmaf(wk[t], g1, a1[t]);
              }
            }
#pragma unroll
        for (int t = 0; t < CT; ++t)
          if (ci0 + t < Cin) {
            gin[(ci0 + t) * HW + pos] = a0[t];
            if (pos2 != pos) gin[(ci0 + t) * HW + pos2] = a1[t];
          }
      }
    }
  }
  __syncthreads();
}

__global__ void __launch_bounds__(kNT) matchpyramid_bwd_kernel(MpBwdArgs a) {
  __shared__ float rq[64], nq[64], sq[64], rd[32], dn[256];
  __shared__ __attribute__((aligned(16))) float part[kBwdStage];
  __shared__ float rdv[kMpDmax], ndv[kMpDmax], tj[kMpDmax];
  const int Q = a.Q, D = a.D, E = a.E, L = a.L;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  float* wpart = a.part + (int64_t)blockIdx.x * a.np;
  float* slot = a.slots + (int64_t)blockIdx.x * a.slot_floats;
  float* cosp = slot + a.o_cos;
  float* G = slot + a.o_G;
  float* eg = slot + a.o_eg;
  int* ep = (int*)(slot + a.o_ep);
  const int nb = (D + 31) / 32;
  for (int i = tid; i < a.np; i += kNT) wpart[i] = 0.0f;

  for (int64_t pair = blockIdx.x; pair < a.n_pairs; pair += gridDim.x) {
    const float* q = a.q + (pair / a.ppq) * (int64_t)Q * E;
    const float* d = a.d + pair * (int64_t)D * E;
    __syncthreads();                                  // the previous pair's last phase still reads the slot and the LDS
    if (w < 4) query_rnorms(q, Q, E, rq, w, lane, nq);
    __syncthreads();
    // ---- the cosine plane again (the forward's block, on the first four wavefronts), and every document row's norm
    for (int s = 0; s < nb; ++s) {
      const int j0 = 32 * s;
      if (w < 4) cosine_block_partials(q, d, Q, D, E, j0, part, dn, w, lane);
      __syncthreads();
      cosine_block_finish(Q, part, dn, rq, rd, w < 4 ? tid : 1 << 30, [&](int i, int j, float v) {
        if (j0 + j < D) cosp[i * D + j0 + j] = v;
      });
      if (tid < 32 && j0 + tid < D) {
        float t = 0.0f;
        for (int u = 0; u < 8; ++u) t += dn[u * 32 + tid];
        ndv[j0 + tid] = sqrtf(t);
        rdv[j0 + tid] = rd[tid];
      }
      __syncthreads();
    }

    // ---- the pyramid, from the last layer down
    for (int l = L - 1; l >= 0; --l) {
      const MpLayer& g = a.lay[l];
      const int C = g.C, kh = g.kh, kw = g.kw, K = g.K, Hc = g.Hc, Wc = g.Wc, oh = g.oh, ow = g.ow;
      const int npool = oh * ow, H = g.Hp - (kw - 1), W = g.Wp - (kh - 1);
      const int Hg = Hc + 2 * (kh - 1), Wg = Wc + 2 * (kw - 1);
      const float* gy = l == L - 1 ? a.go + pair * (int64_t)a.feat : slot + (((l + 1) & 1) ? a.o_g1 : a.o_g0);
      const float* Pl = a.pooled + pair * a.sv_stride + a.sv_off[l];
      const int32_t* Al = a.arg + pair * a.sv_stride + a.sv_off[l];
      const float* In = l ? a.pooled + pair * a.sv_stride + a.sv_off[l - 1] : cosp;
      float* gin = slot + ((l & 1) ? a.o_g1 : a.o_g0);
      // E: the pooled elements' gradients behind the ReLU, their positions (an index outside the plane is clamped into it)
      for (int e = tid; e < C * npool; e += kNT) {
        const int ai = min(max(Al[e], 0), Hc * Wc - 1), row = ai / Wc;
        eg[e] = Pl[e] > 0.0f ? gy[e] : 0.0f;
        ep[e] = (row << 16) | (ai - row * Wc);
      }
      // the pooled rows / columns whose window holds conv row r / column col: first | last << 16 (last < first outside the plane)
      int* rtab = (int*)part;
      int* ctab = rtab + Hg;
      for (int t = tid; t < Hg + Wg; t += kNT) {
        const bool isr = t < Hg;
        const int x = isr ? t - (kh - 1) : t - Hg - (kw - 1), n = isr ? Hc : Wc, o = isr ? oh : ow;
        const bool in = x >= 0 && x < n;
        rtab[t] = in ? (x * o / n) | ((((x + 1) * o + n - 1) / n - 1) << 16) : 1;
      }
      __syncthreads();
      // G: the dense conv-output gradient in its zero frame, a wavefront per stored row
      for (int cr = w; cr < C * Hg; cr += kNW) {
        const int c = cr / Hg, rp = cr - c * Hg, r = rp - (kh - 1);
        const int rt = rtab[rp], ilo = rt & 0xffff, ihi = rt >> 16;
        for (int cp = lane; cp < Wg; cp += 64) {
          const int col = cp - (kw - 1);
          const int ct = ctab[cp], jlo = ct & 0xffff, jhi = ct >> 16;
          const int me = (r << 16) | col;
          float s = 0.0f;
          for (int i = ilo; i <= ihi; ++i)
            for (int j = jlo; j <= jhi; ++j) {
              const int e = (c * oh + i) * ow + j;
              const int pe = ep[e];
              const float gv = eg[e];
              s += pe == me ? gv : 0.0f;
            }
          G[cr * Wg + cp] = s;
        }
      }
      // W: this pair's weight and bias gradients, added to the workgroup's partials: a thread per output walks the
      // channel's pooled elements in order (their values and positions are the same address in every lane of a channel).
      // A layer with fewer outputs than threads cuts the elements into S runs, a thread per (output, run), and adds the
      // runs' sums in run order.
      {
        const int nout = C * (K + 1), S = nout < kNT ? max(1, min(kNT / nout, 32)) : 1, len = (npool + S - 1) / S;
        float* runs = part + Hg + Wg;                  // [nout, S], S > 1 only (nout S <= kNT)
        for (int t = tid; t < nout * S; t += kNT) {
          const int o = t / S, s0 = (t - o * S) * len, s1 = min(s0 + len, npool);
          float acc = 0.0f;
          if (o < C * K) {
            const int c = o / K, k = o - c * K, ci = k / (kh * kw), rem = k - ci * kh * kw, ka = rem / kw, kb = rem - ka * kw;
            const float* egc = eg + c * npool;
            const int* epc = ep + c * npool;
            const int base = (ci * H + ka) * W + kb;
#pragma unroll 8
            for (int e = s0; e < s1; ++e) {
              const int pe = epc[e], rr = pe >> 16, cc = pe & 0xffff;
              const bool ok = rr + ka < H && cc + kb < W;
              const float x = In[ok ? base + rr * W + cc : 0];
              acc = fmaf(egc[e], ok ? x : 0.0f, acc);
            }
          } else {
            const float* egc = eg + (o - C * K) * npool;
#pragma unroll 8
            for (int e = s0; e < s1; ++e) acc += egc[e];
          }
          if (S == 1) wpart[o < C * K ? g.w_off + o : a.wtot + g.b_off + o - C * K] += acc;
          else runs[t] = acc;
        }
        if (S > 1) {
          __syncthreads();
          for (int o = tid; o < nout; o += kNT) {
            float acc = runs[o * S];
            for (int u = 1; u < S; ++u) acc += runs[o * S + u];
            wpart[o < C * K ? g.w_off + o : a.wtot + g.b_off + o - C * K] += acc;
          }
        }
      }
      __syncthreads();
      // X: the input gradient (the pooled gradient of the layer below; grad_cos for layer 0)
      if (g.Cin == 1) input_grad<1>(g, H, W, a.w + g.w_off, G, gin, part, tid);
      else input_grad<16>(g, H, W, a.w + g.w_off, G, gin, part, tid);
    }

    // ---- the cosine's backward: gc = grad_cos [Q, D]
    float* gc = slot + a.o_g0;
    for (int i = w; i < Q; i += kNW) {
      float s = 0.0f;
      for (int j = lane; j < D; j += 64) s = fmaf(gc[i * D + j], cosp[i * D + j], s);
      s = wave_sum(s);
      if (lane == 0) sq[i] = s;
    }
    for (int j = tid; j < D; j += kNT) {
      float t = 0.0f;
      for (int i = 0; i < Q; ++i) t = fmaf(gc[i * D + j], cosp[i * D + j], t);
      tj[j] = t;
    }
    __syncthreads();
    for (int p = tid; p < Q * D; p += kNT) {
      const int i = p / D, j = p - i * D;
      gc[p] = (gc[p] * rq[i]) * rdv[j];
    }
    float* gqp = a.gq + pair * (int64_t)Q * E;
    float* gdp = a.gd + pair * (int64_t)D * E;
    // grad_q[i, e] = sum_j gc[i, j] d[j, e] - q[i, e] f_i: a thread per (16 query rows, e), j in order; the coefficients of
    // 128 document rows at a time are a tile [j][Qp] in LDS
    {
      const int nit = (Q + 15) / 16, Qp = 16 * nit, ntask = nit * E;
      for (int t0 = 0; t0 < ntask; t0 += kNT) {
        const int t = t0 + tid, it = t / E, e = t - it * E;
        const bool on = t < ntask;
        float acc[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) acc[u] = 0.0f;
        for (int j0 = 0; j0 < D; j0 += 128) {
          const int jn = min(128, D - j0);
          __syncthreads();
          for (int u = tid; u < jn * Qp; u += kNT) {
            const int jj = u / Qp, i = u - jj * Qp;
            part[u] = i < Q ? gc[i * D + j0 + jj] : 0.0f;
          }
          __syncthreads();
          if (on)
            for (int jj = 0; jj < jn; ++jj) {
              const float dv = d[(j0 + jj) * E + e];
              const float* al = part + jj * Qp + it * 16;
#pragma unroll
              for (int u = 0; u < 16; ++u) acc[u] = fmaf(al[u], dv, acc[u]);
            }
        }
        if (on) {
#pragma unroll
          for (int u = 0; u < 16; ++u) {
            const int i = it * 16 + u;
            if (i < Q) {
              const float f = nq[i] > 0.0f ? sq[i] * rq[i] / nq[i] : 0.0f;
              gqp[i * E + e] = acc[u] - q[i * E + e] * f;
            }
          }
        }
      }
    }
    // grad_d[j, e] = sum_i gc[i, j] q[i, e] - d[j, e] f_j: a thread per (16 document rows, e), i in order; the coefficients of
    // JT such row tiles at a time are a tile [i][16 JT] in LDS
    {
      const int JT = max(1, min(min((D + 15) / 16, kBwdStage / (Q * 16)), (kNT + E - 1) / E)), Dp = 16 * JT;
      for (int j0 = 0; j0 < D; j0 += Dp) {
        __syncthreads();
        for (int u = tid; u < Q * Dp; u += kNT) {
          const int i = u / Dp, jj = u - i * Dp;
          part[u] = j0 + jj < D ? gc[i * D + j0 + jj] : 0.0f;
        }
        __syncthreads();
        for (int t = tid; t < JT * E; t += kNT) {
          const int jt = t / E, e = t - jt * E;
          if (j0 + 16 * jt >= D) continue;
          float acc[16];
#pragma unroll
          for (int u = 0; u < 16; ++u) acc[u] = 0.0f;
          for (int i = 0; i < Q; ++i) {
            const float qv = q[i * E + e];
            const float* al = part + i * Dp + jt * 16;
#pragma unroll
            for (int u = 0; u < 16; ++u) acc[u] = fmaf(al[u], qv, acc[u]);
          }
#pragma unroll
          for (int u = 0; u < 16; ++u) {
            const int j = j0 + 16 * jt + u;
            if (j < D) {
              const float f = ndv[j] > 0.0f ? tj[j] * rdv[j] / ndv[j] : 0.0f;
              gdp[j * E + e] = acc[u] - d[j * E + e] * f;
            }
          }
        }
      }
    }
  }
}

// grad_w | grad_b = the workgroups' partials added in workgroup order
__global__ void __launch_bounds__(256) matchpyramid_bwd_reduce_kernel(const float* part, int grid, int np, int wtot, float* gw,
                                                                      float* gb) {
  const int o = blockIdx.x * 256 + threadIdx.x;
  if (o >= np) return;
  float s = 0.0f;
  for (int g = 0; g < grid; ++g) s += part[(int64_t)g * np + o];
  if (o < wtot) gw[o] = s;
  else gb[o - wtot] = s;
}

// The backward's slot layout and grid from a validated plan.
int64_t bwd_layout(const MpPlan& P, MpBwdArgs* b, int64_t n_pairs) {
  const MpArgs& a = P.a;
  int64_t gmax = (int64_t)a.Q * a.D, Gmax = 0, emax = 0;
  int wtot = 0, btot = 0;
  for (int l = 0; l < a.L; ++l) {
    const MpLayer& g = a.lay[l];
    const int64_t H = g.Hp - (g.kw - 1), W = g.Wp - (g.kh - 1);
    gmax = std::max(gmax, (int64_t)g.Cin * H * W);
    Gmax = std::max(Gmax, (int64_t)g.C * (g.Hc + 2 * (g.kh - 1)) * (g.Wc + 2 * (g.kw - 1)));   // G in its zero frame
    emax = std::max(emax, (int64_t)g.C * g.oh * g.ow);
    wtot += g.C * g.K;
    btot += g.C;
    b->lay[l] = g;
    b->sv_off[l] = a.sv_off[l];
  }
  b->Q = a.Q; b->D = a.D; b->E = a.E; b->L = a.L; b->feat = a.feat;
  b->sv_stride = a.sv_stride;
  b->wtot = wtot;
  b->np = wtot + btot;
  b->o_cos = 0;
  b->o_g0 = a.Q * a.D;
  b->o_g1 = (int)(b->o_g0 + gmax);
  b->o_G = (int)(b->o_g1 + gmax);
  b->o_eg = (int)(b->o_G + Gmax);
  b->o_ep = (int)(b->o_eg + emax);
  b->slot_floats = b->o_ep + emax;
  const int64_t per = (b->slot_floats + b->np) * (int64_t)sizeof(float);
  int64_t grid = std::min<int64_t>(n_pairs, (int64_t)kCUs);     // 60 KB of LDS and sixteen wavefronts: one workgroup per CU
  grid = std::min<int64_t>(grid, std::max<int64_t>(1, (int64_t)(kWsBudget / per)));
  return std::max<int64_t>(grid, 1);
}

}  // namespace
}  // namespace mm

extern "C" size_t mm_matchpyramid_bwd_workspace_bytes(int64_t n_pairs, int Q, int D, int n_layers, const int32_t* layers) {
  if (n_pairs <= 0 || !layers) return 0;
  MpPlan P;
  if (make_plan(Q, D, 4, n_layers, layers, &P, "mm_matchpyramid_bwd_workspace_bytes") != MM_OK) return 0;
  MpBwdArgs b;
  const int64_t grid = bwd_layout(P, &b, n_pairs);
  return (size_t)grid * (size_t)(b.slot_floats + b.np) * sizeof(float);
}

extern "C" int mm_matchpyramid_bwd(const float* q, const float* d, const float* conv_w, const float* pooled,
                                   const int32_t* argmax, const float* grad_features, float* grad_q, float* grad_d,
                                   float* grad_w, float* grad_b, int64_t n_pairs, int64_t pairs_per_query, int Q, int D, int E,
                                   int n_layers, const int32_t* layers, void* workspace, size_t workspace_bytes, void* stream) {
  if (!q || !d || !conv_w || !pooled || !argmax || !grad_features || !grad_q || !grad_d || !grad_w || !grad_b || !layers)
    return set_error(MM_EINVAL, "mm_matchpyramid_bwd: null q / d / conv_w / pooled / argmax / grad_features / grad_q / grad_d / "
                                "grad_w / grad_b / layers");
  if (n_pairs < 0 || pairs_per_query < 1)
    return set_error(MM_EINVAL, "mm_matchpyramid_bwd: n_pairs = %lld, pairs_per_query = %lld", (long long)n_pairs,
                     (long long)pairs_per_query);
  MpPlan P;
  int rc = make_plan(Q, D, E, n_layers, layers, &P, "mm_matchpyramid_bwd");
  if (rc != MM_OK) return rc;
  if (n_pairs == 0) return MM_OK;
  MpBwdArgs b;
  const int64_t grid = bwd_layout(P, &b, n_pairs);
  const size_t need = (size_t)grid * (size_t)(b.slot_floats + b.np) * sizeof(float);
  if (!workspace || workspace_bytes < need)
    return set_error(MM_EWORKSPACE, "mm_matchpyramid_bwd: workspace of %zu bytes, needs %zu", workspace_bytes, need);
  b.q = q; b.d = d; b.w = conv_w; b.pooled = pooled; b.arg = argmax; b.go = grad_features;
  b.gq = grad_q; b.gd = grad_d;
  b.part = (float*)workspace;
  b.slots = b.part + grid * b.np;
  b.n_pairs = n_pairs;
  b.ppq = pairs_per_query;
  hipLaunchKernelGGL(matchpyramid_bwd_kernel, dim3((unsigned)grid), dim3(kNT), 0, (hipStream_t)stream, b);
  rc = check_launch("mm_matchpyramid_bwd");
  if (rc != MM_OK) return rc;
  hipLaunchKernelGGL(matchpyramid_bwd_reduce_kernel, dim3((unsigned)((b.np + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     b.part, (int)grid, b.np, b.wtot, grad_w, grad_b);
  return check_launch("mm_matchpyramid_bwd (reduce)");
}
