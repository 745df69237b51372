// Training losses on the device: the reduced loss AND its gradient with respect to the scores in one call, so that autograd's
// backward is one multiply by grad_output (matchmaker/losses/*.py run as chains of eager element-wise ops on tensors of 32 to
// a few thousand elements: 45 aten calls for MSMarginLoss forward + backward, 406 for LambdaLossTeacher on a 32 x 64 list).
//
//   mm_pair_loss_fwd   pairwise / pointwise kinds over pos [n], neg [n] and up to two label vectors.  A fixed grid (a function
//                      of n alone) of 256-thread workgroups strides over the elements: gradients are stored as they are formed,
//                      the loss terms go into one float64 accumulator per thread, are reduced per workgroup in a fixed order and
//                      either stored as the loss (one workgroup: n <= 4,096) or as one float64 partial per workgroup in the
//                      workspace, which a second one-workgroup launch adds in a fixed order.
//   mm_list_loss_fwd   listwise kinds over scores [B, L].  Lists of <= 64 entries take one wavefront each, four per workgroup,
//                      no LDS and no barrier (values of other entries come by lane broadcast); longer ones (<= 1,024) take one
//                      256-thread workgroup each, four entries per thread, with scores, labels, keys, ranks, gains and the
//                      discount table in LDS.  Both forms are ONE body over a small policy class.  Ranks come from counting the
//                      keys below one's own (rank_metrics.hip's seg_rank_wave_kernel; the pair loop is O(L^2) anyway), so nothing
//                      is sorted or scattered: entry i meets every j in its own loop and takes both roles of a pair.
//                      A second one-workgroup launch adds per_list [B] in a fixed order.
// Per-element terms of the list kinds are fp32 with the accurate library functions, those of the pair kinds float64; every sum
// is float64 in a fixed order, rounded once.  No
// atomics, no read-back, vector stores only, one linear chain of launches: graph-capturable, and two calls give the same bits.
#include "loss_device.h"

namespace mm {

// ---- pairwise / pointwise ---------------------------------------------------------------------------------------------
struct PairArgs {
  const void* pos;
  const void* neg;
  const float* a;
  const float* b;
  int64_t n;
  int dtype, kind;
  double inv_n;
  float* loss;
  void* gpos;
  void* gneg;
  double* partial;      // [gridDim.x] when the grid has more than one workgroup
};

__global__ void __launch_bounds__(256) pair_loss_kernel(const PairArgs A) {
  __shared__ double red[4];
  double acc = 0.0;
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < A.n; i += stride) {
    const double p = (double)load_elem(A.pos, A.dtype, i), g = (double)load_elem(A.neg, A.dtype, i);
    const double a = (double)A.a[i], b = A.b ? (double)A.b[i] : 0.0;
    double term, gp, gn;
    pair_term(A.kind, p, g, a, b, &term, &gp, &gn);
    acc += term;
    st_grad(A.gpos, A.dtype, i, (float)(gp * A.inv_n));
    st_grad(A.gneg, A.dtype, i, (float)(gn * A.inv_n));
  }
  acc = block_sum_f64(acc, red);
  if (threadIdx.x != 0) return;
  if (gridDim.x == 1) *A.loss = (float)(acc / (double)A.n);
  else A.partial[blockIdx.x] = acc;
}

static int pair_grid(int64_t n) {
  const int64_t g = (n + kPairShare - 1) / kPairShare;
  return g < 1 ? 1 : (g > kPairMaxGrid ? kPairMaxGrid : (int)g);
}

}  // namespace mm

using namespace mm;

extern "C" size_t mm_pair_loss_workspace_bytes(int64_t n) {
  const int g = pair_grid(n < 0 ? 0 : n);
  return g > 1 ? (size_t)g * sizeof(double) : 0;
}

extern "C" int mm_pair_loss_fwd(const void* pos, const void* neg, int dtype, const float* a, const float* b, int64_t n, int kind,
                                float* loss, void* grad_pos, void* grad_neg, void* workspace, size_t workspace_bytes,
                                void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (n < 0) return set_error(MM_EINVAL, "pair_loss: n=%lld below 0", (long long)n);
  if (kind < MM_PAIR_RANKNET || kind > MM_PAIR_MSE_RANKNET) return set_error(MM_EINVAL, "pair_loss: unknown kind %d", kind);
  if (!loss_dtype_ok(dtype)) return set_error(MM_EINVAL, "pair_loss: unknown dtype %d", dtype);
  if (n > (1LL << 31)) return set_error(MM_EUNSUPPORTED, "pair_loss: n=%lld above 2^31", (long long)n);
  if (!loss) return set_error(MM_EINVAL, "pair_loss: null loss");
  const bool need_b = kind != MM_PAIR_RANKNET && kind != MM_PAIR_MARGIN;
  if (n > 0 && (!pos || !neg || !grad_pos || !grad_neg || !a || (need_b && !b))) return set_error(MM_EINVAL, "pair_loss: null pointer");
  if (n == 0) {      // torch.mean of an empty tensor: NaN; nothing else is launched
    hipLaunchKernelGGL(loss_finish_kernel<double>, dim3(1), dim3(256), 0, stream, (const double*)nullptr, (int64_t)0, 0.0, loss);
    return check_launch("pair_loss");
  }
  const int grid = pair_grid(n);
  if (grid > 1 && (!workspace || workspace_bytes < (size_t)grid * sizeof(double)))
    return set_error(MM_EWORKSPACE, "pair_loss: workspace of %zu bytes needed, %zu given", (size_t)grid * sizeof(double), workspace_bytes);
  PairArgs A{pos, neg, a, need_b ? b : nullptr, n, dtype, kind, 1.0 / (double)n, loss, grad_pos, grad_neg, (double*)workspace};
  hipLaunchKernelGGL(pair_loss_kernel, dim3((unsigned)grid), dim3(256), 0, stream, A);
  if (grid > 1)
    hipLaunchKernelGGL(loss_finish_kernel<double>, dim3(1), dim3(256), 0, stream, (const double*)workspace, (int64_t)grid, (double)n, loss);
  return check_launch("pair_loss");
}

extern "C" int mm_list_loss_fwd(const void* scores, int dtype, const float* labels, int B, int L, int kind, float* loss,
                                float* per_list, void* grad, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (B < 0 || L < 0) return set_error(MM_EINVAL, "list_loss: negative size B=%d L=%d", B, L);
  if (kind < MM_LIST_LISTNET || kind > MM_LIST_LAMBDA_NDCG2_TEACHER) return set_error(MM_EINVAL, "list_loss: unknown kind %d", kind);
  if (!loss_dtype_ok(dtype)) return set_error(MM_EINVAL, "list_loss: unknown dtype %d", dtype);
  if (L > kLossMaxList)
    return set_error(MM_EUNSUPPORTED, "list_loss: L=%d above the native limit of %d entries per list", L, kLossMaxList);
  if (!loss || (B > 0 && !per_list) || (B > 0 && L > 0 && (!scores || !labels || !grad))) return set_error(MM_EINVAL, "list_loss: null pointer");
  const bool lambda = list_kind_sums(kind);      // no division by B
  if (B > 0) launch_list_loss(ListArgs{scores, labels, B, L, dtype, lambda ? 1.0 : 1.0 / (double)B, per_list, grad, nullptr, nullptr, nullptr, L}, kind, stream);
  hipLaunchKernelGGL(loss_finish_kernel<float>, dim3(1), dim3(256), 0, stream, (const float*)per_list, (int64_t)B,
                     lambda ? 1.0 : (double)B, loss);
  return check_launch("list_loss");
}
