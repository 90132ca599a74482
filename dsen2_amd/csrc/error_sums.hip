// error_sums.hip — the two sums a validation pass needs, formed where the prediction is (include/dsen2_hip.h,
// "dsen2_abs_sq_error_sums"): out = { sum |p - t|, sum (p - t)^2 } over `count` float32 pairs, every difference, product and sum in
// float64 and rounded on its own (__dadd_rn / __dmul_rn, contraction off: no v_fma_f64), as evaluate() forms them on the host.
// The order of every addition is fixed by `count` alone — the scheme of band_errors_kernel (imresize.hip) with one band: the grid
// is a function of count, a thread adds its elements i = block * 256 + thread, + blocks * 256, ... in index order, the workgroup
// adds its 256 threads in a fixed LDS tree and writes one partial pair, and quality_finish_kernel (quality_common.h), one
// workgroup, adds the partials in a fixed order.  No atomics.
#include "capi_internal.h"

#pragma clang fp contract(off)

#include "quality_common.h"
#include "loss_terms.h"

namespace dsen2 {

namespace {

constexpr int kSumPerThread = 8;               // elements per thread the grid aims at

__global__ __launch_bounds__(kQThreads) void abs_sq_error_kernel(const float* __restrict__ p, const float* __restrict__ t, size_t n,
                                                                 double* __restrict__ partials) {
  __shared__ double s[2][kQThreads];
  const size_t step = (size_t)gridDim.x * kQThreads;
  double sa = 0.0, sq = 0.0;
  for (size_t i = (size_t)blockIdx.x * kQThreads + threadIdx.x; i < n; i += step) {
    const double d = __dadd_rn((double)p[i], -(double)t[i]);
    sa = __dadd_rn(sa, fabs(d));
    sq = __dadd_rn(sq, __dmul_rn(d, d));
  }
  const int tid = threadIdx.x;
  s[0][tid] = sa;
  s[1][tid] = sq;
  __syncthreads();
  for (int half = kQThreads / 2; half > 0; half >>= 1) {
    if (tid < half) {
      s[0][tid] = __dadd_rn(s[0][tid], s[0][tid + half]);
      s[1][tid] = __dadd_rn(s[1][tid], s[1][tid + half]);
    }
    __syncthreads();
  }
  if (tid == 0) {
    partials[2 * (size_t)blockIdx.x + 0] = s[0][0];
    partials[2 * (size_t)blockIdx.x + 1] = s[1][0];
  }
}

// abs_sq_error_kernel for a loss kind and a mask mode (dsen2_loss_sums): the same grid rule, element order and tree over the
// n * c * hw elements of an NCHW pair; a thread's element i is band (i / hw) % c of pixel (i / (c * hw), i % hw).  partials[block]
// = { sum rho(d), sum d^2 }, { unmasked elements, 0 }: two "bands" of quality_finish_kernel.  MASK: the element belongs to a pixel
// without ground truth when the target is 0 in all c bands of that pixel; the other bands are re-read (a pixel's c values are hw
// floats apart and were just read by neighbouring iterations: they sit in L2), so no mask buffer and no second pass exist.
template <int KIND, bool MASK>
__global__ __launch_bounds__(kQThreads) void loss_sums_kernel(const float* __restrict__ p, const float* __restrict__ t, size_t n, int c,
                                                              size_t hw, double param, double* __restrict__ partials) {
  __shared__ double s[2][kQThreads];
  const size_t step = (size_t)gridDim.x * kQThreads;
  double sa = 0.0, sq = 0.0, cnt = 0.0;
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
    sa = __dadd_rn(sa, rho);
    sq = __dadd_rn(sq, __dmul_rn(d, d));
    cnt = __dadd_rn(cnt, 1.0);
  }
  const int tid = threadIdx.x;
  double* const mine = partials + 4 * (size_t)blockIdx.x;
  s[0][tid] = sa;
  s[1][tid] = sq;
  __syncthreads();
  for (int half = kQThreads / 2; half > 0; half >>= 1) {
    if (tid < half) {
      s[0][tid] = __dadd_rn(s[0][tid], s[0][tid + half]);
      s[1][tid] = __dadd_rn(s[1][tid], s[1][tid + half]);
    }
    __syncthreads();
  }
  if (tid == 0) {
    mine[0] = s[0][0];
    mine[1] = s[1][0];
  }
  __syncthreads();
  s[0][tid] = cnt;
  __syncthreads();
  for (int half = kQThreads / 2; half > 0; half >>= 1) {
    if (tid < half) s[0][tid] = __dadd_rn(s[0][tid], s[0][tid + half]);
    __syncthreads();
  }
  if (tid == 0) {
    mine[2] = s[0][0];
    mine[3] = 0.0;
  }
}

template <int KIND>
void launch_loss_sums_kind(bool mask, int blocks, hipStream_t st, const float* p, const float* t, size_t n, int c, size_t hw, double param,
                           double* partials) {
  if (mask)
    hipLaunchKernelGGL((loss_sums_kernel<KIND, true>), dim3(blocks), dim3(kQThreads), 0, st, p, t, n, c, hw, param, partials);
  else
    hipLaunchKernelGGL((loss_sums_kernel<KIND, false>), dim3(blocks), dim3(kQThreads), 0, st, p, t, n, c, hw, param, partials);
}

// partial pairs of two "bands", then the four doubles quality_finish_kernel writes (three of which are dev_out's)
size_t loss_sums_work_bytes() { return quality_work_bytes(2) + 4 * sizeof(double); }

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
  *bytes = quality_work_bytes(1);
  return DSEN2_OK;
}

extern "C" int dsen2_abs_sq_error_sums(const float* dev_pred, const float* dev_target, long long count, void* dev_work, size_t work_bytes,
                                       double* dev_out, void* stream) {
  return guarded([&]() -> int {
    if (!dev_pred || !dev_target || !dev_work || !dev_out) return fail(DSEN2_ERR_INVALID, "abs_sq_error_sums: NULL argument");
    if (count <= 0 || count >= (1LL << 31)) return fail(DSEN2_ERR_INVALID, "abs_sq_error_sums: %lld pairs outside 1..2^31 - 1", count);
    if (work_bytes < quality_work_bytes(1))
      return fail(DSEN2_ERR_WORKSPACE, "abs_sq_error_sums: workspace of %zu bytes, dsen2_abs_sq_error_sums_workspace_bytes asks for %zu",
                  work_bytes, quality_work_bytes(1));
    double* const partials = static_cast<double*>(dev_work);
    const int blocks = error_sum_blocks((size_t)count);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(abs_sq_error_kernel, dim3(blocks), dim3(kQThreads), 0, st, dev_pred, dev_target, (size_t)count, partials);
    if (int rc = launched("abs_sq_error_sums", hipGetLastError())) return rc;
    hipLaunchKernelGGL(quality_finish_kernel, dim3(1), dim3(kQThreads), 0, st, partials, blocks, 1, dev_out);
    return launched("abs_sq_error_sums", hipGetLastError());
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
    const bool mk = mask_mode == kMaskNoData;
    const double p = (double)param;
    switch (kind) {
      case kLossMae: launch_loss_sums_kind<kLossMae>(mk, blocks, st, dev_pred, dev_target, (size_t)count, c, (size_t)hw, p, partials); break;
      case kLossMse: launch_loss_sums_kind<kLossMse>(mk, blocks, st, dev_pred, dev_target, (size_t)count, c, (size_t)hw, p, partials); break;
      case kLossHuber: launch_loss_sums_kind<kLossHuber>(mk, blocks, st, dev_pred, dev_target, (size_t)count, c, (size_t)hw, p, partials); break;
      default: launch_loss_sums_kind<kLossCharbonnier>(mk, blocks, st, dev_pred, dev_target, (size_t)count, c, (size_t)hw, p, partials); break;
    }
    if (int rc = launched("loss_sums", hipGetLastError())) return rc;
    hipLaunchKernelGGL(quality_finish_kernel, dim3(1), dim3(kQThreads), 0, st, partials, blocks, 2, sums4);
    if (int rc = launched("loss_sums", hipGetLastError())) return rc;
    HIP_TRY(hipMemcpyAsync(dev_out3, sums4, 3 * sizeof(double), hipMemcpyDeviceToDevice, st));
    return DSEN2_OK;
  });
}
