// In-batch negatives of dense-retriever training (matchmaker/train.py:434-472) on the device: from the vectors (or from the
// [B, B] score matrices) to the in-batch loss, its three statistics and every gradient in a fixed chain of launches.
//
//   mm_inbatch_dot_loss_fwd      1. ib_dot_kernel     Sp = Q Dp^T, Sn = Q Dn^T on the matrix cores (32 x 32 x 16 for 16-bit vectors,
//                                                     the fp32 instruction for fp32 ones; fp32 accumulation in blocks of 64 k added in float64, S stays fp32), one
//                                                     32 x 32 tile per wavefront, four per workgroup, and the epilogue below on the
//                                                     accumulator registers
//                                2. list family only: the list kernel of loss_device.h on S, writing G
//                                3. ib_finish_kernel  one workgroup: the float64 partials in a fixed order -> loss, stats, grad_sp
//                                4. ib_grad_kernel    grad_Q = G [Dp; Dn], grad_Dp = G_p^T Q, grad_Dn = G_n^T Q on the fp32 matrix
//                                                     instruction over exactly widened vectors, G not rounded, one rounding at the store
//   mm_inbatch_select_loss_fwd   1. ib_select_kernel  the same tiles and the same epilogue, the scores read from Sp / Sn
//                                2., 3. as above
// The epilogue (ib_epilogue) is ONE function: lane (c, h) of a tile holds column c of 16 rows; per off-diagonal element it forms the
// pair term (pair_term of loss_device.h: float64), the statistics and G = d loss / d S, keeps four float64 sums per lane, reduces
// them per wavefront and per workgroup in a fixed order into partial[workgroup][4], and leaves the row sums of d term / d sp of its
// 32 columns in rowpart[column tile][row].  Both entries walk the elements in the same order, so the dot entry and the select entry
// fed the dot entry's S give the same bits.  No atomics, no allocation, no read-back, vector stores only.
#include "loss_device.h"

namespace mm {

constexpr int kIbMaxB = 1024, kIbMinE = 8, kIbMaxE = 1024;
constexpr int kIbBlockK = 64;      // k values per fp32 accumulation block of the scores kernel

struct IbArgs {
  const void* Q;       // dot entry: [B, E] each of vdt
  const void* Dp;
  const void* Dn;
  const void* Sp;      // select entry: [B, B] each of sdt
  const void* Sn;
  const void* sp;      // [B] of spdt
  const float* Tp;     // [B, B] or NULL
  const float* Tn;
  int vdt, sdt, spdt, E, B, family, kind;
  double scale;        // pair family: 0.5 / M, 0 when M == 0
  float* S0;           // dot entry: Sp and Sn [B, B] fp32, else NULL
  float* S1;
  void* G0;            // d loss / d Sp[i, j] at G0[i gld + j], d loss / d Sn[i, j] at G1[i gld + j], of gdt
  void* G1;
  int gdt;
  int64_t gld;
  double* partial;     // [workgroups][4]: term, greater, difference, teacher greater
  double* rowpart;     // [column tiles][B]
};

// s: the wavefront's 32 x 32 tile of cat([Sp, Sn], 1) at (row0, col0) in the accumulator layout.  red: 16 doubles of LDS.
__device__ __forceinline__ void ib_epilogue(const IbArgs& A, const f32x16& s, int row0, int col0, double* red) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, h = lane >> 5;
  const int B = A.B, c = col0 + (lane & 31);
  const bool second = c >= B, cin = c < 2 * B;
  const int j = second ? c - B : c;
  const bool pair = A.family == MM_INBATCH_PAIR;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int v = 0; v < 16; ++v) {
    const int i = row0 + (rowof(v) + 4 * h);
    const bool in = cin && i < B, off = in && i != j;
    double rs = 0.0;
    float gv = 0.0f;
    if (off) {
      const double p = (double)load_elem(A.sp, A.spdt, i), g = (double)s[v];
      acc[1] += p > g ? 1.0 : 0.0;
      acc[2] += p - g;
      if (pair) {
        const double a = A.Tp ? (double)A.Tp[(int64_t)i * B + i] : 1.0;
        const double b = A.Tp ? (double)(second ? A.Tn : A.Tp)[(int64_t)i * B + j] : 0.0;
        double term, gp, gn;
        pair_term(A.kind, p, g, a, b, &term, &gp, &gn);
        acc[0] += term;
        acc[3] += A.Tp && a > b ? 1.0 : 0.0;
        gv = (float)(gn * A.scale);
        rs = gp;
      }
    }
    if (in) {
      if (A.S0) (second ? A.S1 : A.S0)[(int64_t)i * B + j] = s[v];
      if (pair) st_grad(second ? A.G1 : A.G0, A.gdt, (int64_t)i * A.gld + j, gv);      // the diagonal: 0
    }
    if (pair) {      // (uniform) the sum over the tile's 32 columns of row i: the lanes of this half, the same tree in each
#pragma unroll
      for (int o = 16; o >= 1; o >>= 1) rs += __shfl_xor(rs, o, 64);
      if ((lane & 31) == 0 && i < B && col0 < 2 * B) A.rowpart[(int64_t)(col0 >> 5) * B + i] = rs;      // (a wavefront past the last column tile has no slot)
    }
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    acc[q] = wave_sum_f64(acc[q]);
    if (lane == 0) red[wave * 4 + q] = acc[q];
  }
  __syncthreads();
  if (threadIdx.x < 4) {
    const int q = threadIdx.x;
    A.partial[(int64_t)(blockIdx.y * gridDim.x + blockIdx.x) * 4 + q] = ((red[q] + red[4 + q]) + red[8 + q]) + red[12 + q];
  }
}

template <int DT>
struct IbMfma {      // the 16-bit types
  static constexpr int STEP = 16;      // k per step; a lane half supplies 8 of them: 16 bytes
  static __device__ __forceinline__ f32x16 run(const f32x4& a, const f32x4& b, f32x16 c) {
    return Mfma32x16<DT>::run(__builtin_bit_cast(short8, a), __builtin_bit_cast(short8, b), c);
  }
};
template <>
struct IbMfma<MM_F32> {
  static constexpr int STEP = 8;       // a lane half supplies 4 floats: four steps of the k = 2 instruction, k order permuted alike in A and B
  static __device__ __forceinline__ f32x16 run(const f32x4& a, const f32x4& b, f32x16 c) {
#pragma unroll
    for (int j = 0; j < 4; ++j) c = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j], b[j], c, 0, 0, 0);
    return c;
  }
};

// grid (ceil(ceil(2B / 32) / 4), ceil(B / 32)), 256 threads: wavefront w owns columns 32 (4 blockIdx.x + w) .. + 31 of cat([Sp, Sn], 1)
template <int DT>
__global__ void __launch_bounds__(256) ib_dot_kernel(const IbArgs A) {
  __shared__ double red[16];
  constexpr int ES = DT == MM_F32 ? 4 : 2;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, h = lane >> 5, r = lane & 31;
  const int row0 = blockIdx.y * 32, col0 = (blockIdx.x * 4 + wave) * 32;
  const int B = A.B, E = A.E;
  // fp32 accumulation inside blocks of kIbBlockK k values, the blocks added in float64 and S rounded once: a chain of E fp32
  // roundings would leave S (and through a softmax every list gradient) several times further from the exact dot than torch's mm
  f32x16 acc = {0};
  double wide[16];
#pragma unroll
  for (int v = 0; v < 16; ++v) wide[v] = 0.0;
  if (col0 < 2 * B) {      // wave-uniform
    const int i = row0 + r, c = col0 + r;
    const bool ain = i < B, bin = c < 2 * B;
    const char* arow = (const char*)A.Q + (int64_t)(ain ? i : 0) * E * ES;
    const char* brow = (const char*)(c >= B ? A.Dn : A.Dp) + (int64_t)(bin ? (c >= B ? c - B : c) : 0) * E * ES;
    constexpr int HALF = IbMfma<DT>::STEP / 2;
    for (int k0 = 0; k0 < E; k0 += IbMfma<DT>::STEP) {
      const int k = k0 + HALF * h;      // (E is a multiple of HALF: a chunk is inside the row or wholly past it)
      f32x4 av = {0.0f, 0.0f, 0.0f, 0.0f}, bv = {0.0f, 0.0f, 0.0f, 0.0f};
      if (k < E && ain) av = *(const f32x4*)(arow + (int64_t)k * ES);
      if (k < E && bin) bv = *(const f32x4*)(brow + (int64_t)k * ES);
      acc = IbMfma<DT>::run(av, bv, acc);
      if ((k0 + IbMfma<DT>::STEP) % kIbBlockK == 0) {
#pragma unroll
        for (int v = 0; v < 16; ++v) {
          wide[v] += (double)acc[v];
          acc[v] = 0.0f;
        }
      }
    }
  }
#pragma unroll
  for (int v = 0; v < 16; ++v) acc[v] = (float)(wide[v] + (double)acc[v]);
  ib_epilogue(A, acc, row0, col0, red);
}

__global__ void __launch_bounds__(256) ib_select_kernel(const IbArgs A) {
  __shared__ double red[16];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, h = lane >> 5;
  const int row0 = blockIdx.y * 32, col0 = (blockIdx.x * 4 + wave) * 32;
  const int B = A.B, c = col0 + (lane & 31);
  f32x16 s = {0};
#pragma unroll
  for (int v = 0; v < 16; ++v) {
    const int i = row0 + (rowof(v) + 4 * h);
    if (c < 2 * B && i < B) s[v] = load_elem(c >= B ? A.Sn : A.Sp, A.sdt, (int64_t)i * B + (c >= B ? c - B : c));
  }
  ib_epilogue(A, s, row0, col0, red);
}

struct IbFinishArgs {
  const double* partial;
  const double* rowpart;
  const float* per_list;      // list family
  int nwg, ntile, B, family, teacher, spdt;
  double scale, list_denom;
  float* loss;
  float* stats;
  void* grad_sp;              // or NULL
};

// One workgroup.  B == 0: every sum is empty and every mean 0 / 0 = NaN, as torch.
__global__ void __launch_bounds__(256) ib_finish_kernel(const IbFinishArgs A) {
  __shared__ double red[4];
  double sum[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    double acc = 0.0;
    for (int w = threadIdx.x; w < A.nwg; w += 256) acc += A.partial[(int64_t)w * 4 + q];
    sum[q] = block_sum_f64(acc, red);
  }
  const bool pair = A.family == MM_INBATCH_PAIR;
  double lsum = 0.0;
  if (!pair) {
    for (int i = threadIdx.x; i < A.B; i += 256) lsum += (double)A.per_list[i];
    lsum = block_sum_f64(lsum, red);
  }
  const double M2 = 2.0 * (double)A.B * (double)(A.B - 1);      // both matrices
  if (threadIdx.x == 0) {
    *A.loss = (float)(pair ? sum[0] / M2 : lsum / A.list_denom);
    A.stats[0] = (float)(sum[1] / M2);
    A.stats[1] = (float)(sum[2] / M2);
    A.stats[2] = pair && A.teacher ? (float)(sum[3] / M2) : __builtin_nanf("");
  }
  if (!A.grad_sp) return;
  for (int i = threadIdx.x; i < A.B; i += 256) {
    double r = 0.0;
    if (pair)
      for (int t = 0; t < A.ntile; ++t) r += A.rowpart[(int64_t)t * A.B + i];
    st_grad(A.grad_sp, A.spdt, i, (float)(r * A.scale));
  }
}

struct IbGradArgs {
  const void* Q;
  const void* Dp;
  const void* Dn;
  const float* Gp;     // [B, B] each: d loss / d Sp, d loss / d Sn
  const float* Gn;
  int vdt, B, E;
  void* out[3];        // grad_Q, grad_Dp, grad_Dn; a NULL one is skipped
};

// grid (ceil(E / 32), ceil(B / 32), 3), one wavefront: a 32 x 32 tile of out[z] = A X with
//   z = 0  A[i][k] = [Gp Gn][i][k], k < 2B;   X[k] = row k of [Dp; Dn]
//   z = 1  A[j][k] = Gp[k][j], k < B;         X[k] = row k of Q
//   z = 2  A[j][k] = Gn[k][j], k < B;         X[k] = row k of Q
// Lane (r, h) supplies A[row0 + r][k0 + h] and X[k0 + h][e0 + r]; what lies past the matrices is an exact 0 on both sides.
__global__ void __launch_bounds__(64) ib_grad_kernel(const IbGradArgs A) {
  const int z = blockIdx.z;
  if (!A.out[z]) return;
  const int lane = threadIdx.x, h = lane >> 5, r = lane & 31;
  const int B = A.B, E = A.E, K = z == 0 ? 2 * B : B;
  const int row = blockIdx.y * 32 + r, e = blockIdx.x * 32 + r;
  const bool rin = row < B, ein = e < E;
  const int rc = rin ? row : 0;
  f32x16 acc = {0};
  for (int k0 = 0; k0 < K; k0 += 2) {
    const int k = k0 + h;
    const bool kin = k < K;
    const int kc = kin ? k : 0;
    const bool second = z == 0 && kc >= B;
    const int kr = second ? kc - B : kc;      // the row of its matrix
    float a = z == 0 ? (second ? A.Gn : A.Gp)[(int64_t)rc * B + kr] : (z == 1 ? A.Gp : A.Gn)[(int64_t)kr * B + rc];
    float b = load_elem(z == 0 ? (second ? A.Dn : A.Dp) : A.Q, A.vdt, (int64_t)kr * E + (ein ? e : 0));
    if (!kin || !rin) a = 0.0f;
    if (!kin || !ein) b = 0.0f;
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
  }
  if (!ein) return;
#pragma unroll
  for (int v = 0; v < 16; ++v) {
    const int i = blockIdx.y * 32 + (rowof(v) + 4 * h);
    if (i < B) st_grad(A.out[z], A.vdt, (int64_t)i * E + e, acc[v]);
  }
}

static size_t ib_up(size_t n) { return (n + 255) / 256 * 256; }

struct IbLayout {
  int ntile, gx, gy, nwg;
  size_t s, g, partial, rowpart, per_list, total;      // byte offsets
};

static IbLayout ib_layout(int B, bool dot) {
  IbLayout L;
  L.ntile = (2 * B + 31) / 32;
  L.gx = (L.ntile + 3) / 4;
  L.gy = (B + 31) / 32;
  L.nwg = L.gx * L.gy;
  const size_t sg = dot ? ib_up((size_t)2 * B * B * sizeof(float)) : 0;      // [2][B][B]: the Sp / Gp matrix, then the Sn / Gn one
  L.s = 0;
  L.g = sg;
  L.partial = 2 * sg;
  L.rowpart = L.partial + ib_up((size_t)L.nwg * 4 * sizeof(double));
  L.per_list = L.rowpart + ib_up((size_t)L.ntile * B * sizeof(double));
  L.total = L.per_list + ib_up((size_t)B * sizeof(float));
  return L;
}

// what both entries check alike; MM_OK, or the code set_error returned
static int ib_check(const char* op, int B, int family, int kind, const float* Tp, const float* Tn, const float* loss, const float* stats) {
  if (B < 0) return set_error(MM_EINVAL, "%s: B=%d below 0", op, B);
  if (family != MM_INBATCH_PAIR && family != MM_INBATCH_LIST) return set_error(MM_EINVAL, "%s: unknown family %d", op, family);
  if (family == MM_INBATCH_PAIR && (kind < MM_PAIR_RANKNET || kind > MM_PAIR_MSE_RANKNET)) return set_error(MM_EINVAL, "%s: unknown pair kind %d", op, kind);
  if (family == MM_INBATCH_LIST && (kind < MM_LIST_LISTNET || kind > MM_LIST_LAMBDA_NDCG2_TEACHER)) return set_error(MM_EINVAL, "%s: unknown list kind %d", op, kind);
  if (!loss || !stats) return set_error(MM_EINVAL, "%s: null loss or stats", op);
  if ((Tp == nullptr) != (Tn == nullptr)) return set_error(MM_EINVAL, "%s: one teacher matrix without the other", op);
  const bool one_label = family == MM_INBATCH_PAIR && (kind == MM_PAIR_RANKNET || kind == MM_PAIR_MARGIN);
  if (B > 0 && one_label && Tp) return set_error(MM_EINVAL, "%s: pair kind %d takes the label 1 and no teacher", op, kind);
  if (B > 0 && !one_label && !Tp) return set_error(MM_EINVAL, "%s: this kind needs the teacher matrices", op);
  if (family == MM_INBATCH_LIST && 2 * (int64_t)B > kLossMaxList)
    return set_error(MM_EUNSUPPORTED, "%s: 2 B = %lld above the native limit of %d entries per list", op, 2 * (long long)B, kLossMaxList);
  if (B > kIbMaxB) return set_error(MM_EUNSUPPORTED, "%s: B=%d above the native limit of %d", op, B, kIbMaxB);
  return MM_OK;
}

static void ib_finish(const IbArgs& A, const IbLayout& L, char* ws, float* loss, float* stats, void* grad_sp, hipStream_t stream) {
  const bool sums = A.family == MM_INBATCH_LIST && list_kind_sums(A.kind);
  IbFinishArgs F{A.partial, A.rowpart, (const float*)(ws ? ws + L.per_list : nullptr), A.B > 0 ? L.nwg : 0, L.ntile, A.B, A.family,
                 A.Tp != nullptr, A.spdt, A.scale, sums ? 1.0 : (double)A.B, loss, stats, grad_sp};
  hipLaunchKernelGGL(ib_finish_kernel, dim3(1), dim3(256), 0, stream, F);
}

}  // namespace mm

using namespace mm;

extern "C" size_t mm_inbatch_select_loss_workspace_bytes(int B, int family) {
  (void)family;
  return B <= 0 || B > kIbMaxB ? 0 : ib_layout(B, false).total;
}

extern "C" size_t mm_inbatch_dot_loss_workspace_bytes(int B, int E, int family) {
  (void)E;
  (void)family;
  return B <= 0 || B > kIbMaxB ? 0 : ib_layout(B, true).total;
}

extern "C" int mm_inbatch_select_loss_fwd(const void* sp, const void* Sp, const void* Sn, int dtype, const float* Tp, const float* Tn,
                                          int B, int family, int kind, float* loss, float* stats, void* grad_sp, void* grad_Sp,
                                          void* grad_Sn, void* workspace, size_t workspace_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const char* op = "inbatch_select_loss";
  if (const int rc = ib_check(op, B, family, kind, Tp, Tn, loss, stats)) return rc;
  if (!loss_dtype_ok(dtype)) return set_error(MM_EINVAL, "%s: unknown dtype %d", op, dtype);
  if (B > 0 && (!sp || !Sp || !Sn || !grad_sp || !grad_Sp || !grad_Sn)) return set_error(MM_EINVAL, "%s: null pointer", op);
  IbArgs A{};
  A.B = B, A.family = family, A.kind = kind, A.spdt = dtype;
  const IbLayout L = ib_layout(B > 0 ? B : 1, false);
  if (B == 0) {
    ib_finish(A, L, nullptr, loss, stats, nullptr, stream);
    return check_launch(op);
  }
  if (!workspace || workspace_bytes < L.total) return set_error(MM_EWORKSPACE, "%s: workspace of %zu bytes needed, %zu given", op, L.total, workspace_bytes);
  char* ws = (char*)workspace;
  const double M = (double)B * (double)(B - 1);
  A.Sp = Sp, A.Sn = Sn, A.sdt = dtype, A.sp = sp, A.Tp = Tp, A.Tn = Tn;
  A.scale = M > 0.0 ? 0.5 / M : 0.0;
  A.G0 = grad_Sp, A.G1 = grad_Sn, A.gdt = dtype, A.gld = B;
  A.partial = (double*)(ws + L.partial), A.rowpart = (double*)(ws + L.rowpart);
  hipLaunchKernelGGL(ib_select_kernel, dim3((unsigned)L.gx, (unsigned)L.gy), dim3(256), 0, stream, A);
  if (family == MM_INBATCH_LIST)
    launch_list_loss(ListArgs{Sp, Tp, B, 2 * B, dtype, list_kind_sums(kind) ? 1.0 : 1.0 / (double)B, (float*)(ws + L.per_list), grad_Sp, Sn,
                              Tn, grad_Sn, B}, kind, stream);
  ib_finish(A, L, ws, loss, stats, grad_sp, stream);
  return check_launch(op);
}

extern "C" int mm_inbatch_dot_loss_fwd(const void* Q, const void* Dp, const void* Dn, int dtype, const void* sp, int sp_dtype,
                                       const float* Tp, const float* Tn, int B, int E, int family, int kind, float* loss, float* stats,
                                       void* grad_Q, void* grad_Dp, void* grad_Dn, void* grad_sp, void* workspace,
                                       size_t workspace_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const char* op = "inbatch_dot_loss";
  if (const int rc = ib_check(op, B, family, kind, Tp, Tn, loss, stats)) return rc;
  if (!loss_dtype_ok(dtype) || !loss_dtype_ok(sp_dtype)) return set_error(MM_EINVAL, "%s: unknown dtype %d / %d", op, dtype, sp_dtype);
  if (E < kIbMinE || E > kIbMaxE || E % (dtype == MM_F32 ? 4 : 8) != 0)
    return set_error(MM_EUNSUPPORTED, "%s: E=%d outside %d .. %d or rows that are no multiple of 16 bytes", op, E, kIbMinE, kIbMaxE);
  if (B > 0 && (!Q || !Dp || !Dn || !sp)) return set_error(MM_EINVAL, "%s: null pointer", op);
  if (B > 0 && (((uintptr_t)Q | (uintptr_t)Dp | (uintptr_t)Dn) & 15) != 0)      // the scores kernel loads 16 bytes per lane
    return set_error(MM_EINVAL, "%s: Q, Dp and Dn must be 16-byte aligned", op);
  IbArgs A{};
  A.B = B, A.family = family, A.kind = kind, A.spdt = sp_dtype;
  const IbLayout L = ib_layout(B > 0 ? B : 1, true);
  if (B == 0) {
    ib_finish(A, L, nullptr, loss, stats, nullptr, stream);
    return check_launch(op);
  }
  if (!workspace || workspace_bytes < L.total) return set_error(MM_EWORKSPACE, "%s: workspace of %zu bytes needed, %zu given", op, L.total, workspace_bytes);
  char* ws = (char*)workspace;
  const double M = (double)B * (double)(B - 1);
  float* S = (float*)(ws + L.s);
  float* G = (float*)(ws + L.g);
  A.Q = Q, A.Dp = Dp, A.Dn = Dn, A.vdt = dtype, A.E = E, A.sp = sp, A.Tp = Tp, A.Tn = Tn;
  A.scale = M > 0.0 ? 0.5 / M : 0.0;
  A.S0 = S, A.S1 = S + (int64_t)B * B, A.G0 = G, A.G1 = G + (int64_t)B * B, A.gdt = MM_F32, A.gld = B;
  A.partial = (double*)(ws + L.partial), A.rowpart = (double*)(ws + L.rowpart);
  const dim3 grid((unsigned)L.gx, (unsigned)L.gy);
  if (dtype == MM_F32) hipLaunchKernelGGL(ib_dot_kernel<MM_F32>, grid, dim3(256), 0, stream, A);
  else if (dtype == MM_F16) hipLaunchKernelGGL(ib_dot_kernel<MM_F16>, grid, dim3(256), 0, stream, A);
  else hipLaunchKernelGGL(ib_dot_kernel<MM_BF16>, grid, dim3(256), 0, stream, A);
  if (family == MM_INBATCH_LIST)
    launch_list_loss(ListArgs{S, Tp, B, 2 * B, MM_F32, list_kind_sums(kind) ? 1.0 : 1.0 / (double)B, (float*)(ws + L.per_list), G,
                              S + (int64_t)B * B, Tn, G + (int64_t)B * B, B}, kind, stream);
  ib_finish(A, L, ws, loss, stats, grad_sp, stream);
  if (grad_Q || grad_Dp || grad_Dn) {
    IbGradArgs R{Q, Dp, Dn, G, G + (int64_t)B * B, dtype, B, E, {grad_Q, grad_Dp, grad_Dn}};
    hipLaunchKernelGGL(ib_grad_kernel, dim3((unsigned)((E + 31) / 32), (unsigned)L.gy, 3), dim3(64), 0, stream, R);
  }
  return check_launch(op);
}
