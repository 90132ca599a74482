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
