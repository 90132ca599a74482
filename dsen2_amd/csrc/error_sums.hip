// error_sums.hip — the sums a validation pass needs, formed where the prediction is (include/dsen2_hip.h,
// "dsen2_abs_sq_error_sums" and "dsen2_loss_sums"): out = { sum rho(p - t), sum (p - t)^2 [, unmasked elements] } over float32
// pairs, every difference, product and sum in float64 and rounded on its own (__dadd_rn / __dmul_rn, contraction off: no
// v_fma_f64), as evaluate() forms them on the host.  One kernel template serves both entries: dsen2_abs_sq_error_sums is its
// (MAE, no mask) instance without the count.  The order of every addition is fixed by the element count alone (fixed_sum.h): the
// grid is a function of the count, a thread adds its elements i = block * 256 + thread, + blocks * 256, ... in index order,
// block_tree adds the workgroup's 256 threads and the block writes one partial, and the one-block finish kernel adds the
// partials.  No atomics.
#include "capi_internal.h"

#pragma clang fp contract(off)

#include "quality_common.h"
#include "loss_terms.h"

namespace dsen2 {

namespace {

constexpr int kSumPerThread = 8;               // elements per thread the grid aims at

// The n elements of an NCHW pair [n / (c * hw)][c][hw]; a thread's element i is band (i / hw) % c of pixel (i / (c * hw), i % hw).
// COUNT: partials[block] = { sum rho(d), sum d^2 }, { unmasked elements, 0 }: two "bands" of the finish kernel; else the first
// pair alone and no count is formed.  MASK: the element belongs to a pixel without ground truth when the target is 0 in all c
// bands of that pixel; the other bands are re-read (a pixel's c values are hw floats apart and were just read by neighbouring
// iterations: they sit in L2), so no mask buffer and no second pass exist.  Without MASK, c and hw are not read: n may be flat.
template <int KIND, bool MASK, bool COUNT>
__global__ __launch_bounds__(kQThreads) void loss_sums_kernel(const float* __restrict__ p, const float* __restrict__ t, size_t n, int c,
                                                              size_t hw, double param, double* __restrict__ partials) {
  constexpr int N = COUNT ? 3 : 2;
  const size_t step = (size_t)gridDim.x * kQThreads;
  double v[N] = {};                            // sum rho, sum d^2 [, elements]
  for (size_t i = (size_t)blockIdx.x * kQThreads + threadIdx.x; i < n; i += step) {
    if (MASK) {
      const size_t img = i / (hw * c), q = i % hw;
      const float* tp = t + img * hw * c + q;
      bool valid = false;
      for (int ch = 0; ch < c; ++ch) valid |= tp[(size_t)ch * hw] != 0.f;      // -0.0 is 0; NaN and negative values are data
      if (!valid) continue;
    }
    const double d = __dadd_rn((double)p[i], -(double)t[i]);
    double rho, slope;
    loss_terms<KIND>(d, param, rho, slope);
    v[0] = __dadd_rn(v[0], rho);
    v[1] = __dadd_rn(v[1], __dmul_rn(d, d));
    if constexpr (COUNT) v[2] = __dadd_rn(v[2], 1.0);
  }
  block_tree<N>(v);
  if (threadIdx.x == 0) {
    double* const mine = partials + (COUNT ? 4 : 2) * (size_t)blockIdx.x;
    mine[0] = v[0];
    mine[1] = v[1];
    if constexpr (COUNT) {
      mine[2] = v[2];
      mine[3] = 0.0;
    }
  }
}

// partial pairs of two "bands", then the four doubles the finish kernel writes (three of which are dev_out's)
size_t loss_sums_work_bytes() { return sum_work_bytes(2) + 4 * sizeof(double); }

int error_sum_blocks(size_t n) {
  const size_t per = (size_t)kQThreads * kSumPerThread;
  const size_t want = (n + per - 1) / per;
  return (int)(want < 1 ? 1 : (want > (size_t)kQMaxBlocks ? (size_t)kQMaxBlocks : want));
}

}  // namespace
}  // namespace dsen2

using namespace dsen2;

extern "C" int dsen2_abs_sq_error_sums_workspace_bytes(size_t* bytes) {
  if (!bytes) return fail(DSEN2_ERR_INVALID, "abs_sq_error_sums_workspace_bytes: NULL argument");
  *bytes = sum_work_bytes(1);
  return DSEN2_OK;
}

extern "C" int dsen2_abs_sq_error_sums(const float* dev_pred, const float* dev_target, long long count, void* dev_work, size_t work_bytes,
                                       double* dev_out, void* stream) {
  return guarded([&]() -> int {
    if (!dev_pred || !dev_target || !dev_work || !dev_out) return fail(DSEN2_ERR_INVALID, "abs_sq_error_sums: NULL argument");
    if (count <= 0 || count >= (1LL << 31)) return fail(DSEN2_ERR_INVALID, "abs_sq_error_sums: %lld pairs outside 1..2^31 - 1", count);
    if (work_bytes < sum_work_bytes(1))
      return fail(DSEN2_ERR_WORKSPACE, "abs_sq_error_sums: workspace of %zu bytes, dsen2_abs_sq_error_sums_workspace_bytes asks for %zu",
                  work_bytes, sum_work_bytes(1));
    double* const partials = static_cast<double*>(dev_work);
    const int blocks = error_sum_blocks((size_t)count);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL((loss_sums_kernel<kLossMae, false, false>), dim3(blocks), dim3(kQThreads), 0, st, dev_pred, dev_target, (size_t)count,
                       1, (size_t)count, 0.0, partials);
    if (int rc = launched("abs_sq_error_sums", hipGetLastError())) return rc;
    return launched("abs_sq_error_sums", launch_finish(partials, blocks, 1, 2, 0.0, dev_out, st));
  });
}

extern "C" int dsen2_loss_sums_workspace_bytes(size_t* bytes) {
  if (!bytes) return fail(DSEN2_ERR_INVALID, "loss_sums_workspace_bytes: NULL argument");
  *bytes = loss_sums_work_bytes();
  return DSEN2_OK;
}

extern "C" int dsen2_loss_sums(const float* dev_pred, const float* dev_target, int n, int c, long long hw, int kind, float param,
                               int mask_mode, void* dev_work, size_t work_bytes, double* dev_out3, void* stream) {
  return guarded([&]() -> int {
    if (!dev_pred || !dev_target || !dev_work || !dev_out3) return fail(DSEN2_ERR_INVALID, "loss_sums: NULL argument");
    if (n <= 0 || c <= 0 || hw <= 0) return fail(DSEN2_ERR_INVALID, "loss_sums: bad shape n=%d c=%d hw=%lld", n, c, hw);
    const long long count = (hw >= (1LL << 31) || (long long)n * c >= (1LL << 31)) ? (1LL << 31) : (long long)n * c * hw;
    if (count >= (1LL << 31)) return fail(DSEN2_ERR_INVALID, "loss_sums: %d x %d x %lld pairs outside 1..2^31 - 1", n, c, hw);
    if (int rc = check_loss("loss_sums", kind, param, mask_mode)) return rc;
    if (work_bytes < loss_sums_work_bytes())
      return fail(DSEN2_ERR_WORKSPACE, "loss_sums: workspace of %zu bytes, dsen2_loss_sums_workspace_bytes asks for %zu", work_bytes,
                  loss_sums_work_bytes());
    double* const partials = static_cast<double*>(dev_work);
    double* const sums4 = partials + (size_t)kQMaxBlocks * 4;
    const int blocks = error_sum_blocks((size_t)count);
    hipStream_t st = (hipStream_t)stream;
    with_loss(kind, mask_mode, [&](auto k, auto m) {
      hipLaunchKernelGGL((loss_sums_kernel<decltype(k)::value, decltype(m)::value, true>), dim3(blocks), dim3(kQThreads), 0, st, dev_pred,
                         dev_target, (size_t)count, c, (size_t)hw, (double)param, partials);
    });
    if (int rc = launched("loss_sums", hipGetLastError())) return rc;
    if (int rc = launched("loss_sums", launch_finish(partials, blocks, 2, 2, 0.0, sums4, st))) return rc;
    HIP_TRY(hipMemcpyAsync(dev_out3, sums4, 3 * sizeof(double), hipMemcpyDeviceToDevice, st));
    return DSEN2_OK;
  });
}
