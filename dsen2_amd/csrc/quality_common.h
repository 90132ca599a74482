// What quality_metrics.hip (UIQ, SAM) and ssim.hip share: the two image loaders their kernels are templates over and the
// argument checks of their C-ABI entries (the sums' pieces are fixed_sum.h's).  Include it below
// `#pragma clang fp contract(off)` and after capi_internal.h.
#pragma once
#include "fixed_sum.h"     // kQThreads, kQMaxBands, kQMaxBlocks, sum_work_bytes, the finish kernel
#include "resample.h"

namespace dsen2 {

template <typename T>
struct DirectImage {        // x[r][col][band] of an HWC image
  const T* p;
  int W, C;
  __device__ __forceinline__ double operator()(int r, int col, int band) const { return as_double(p[((size_t)r * W + col) * C + band]); }
};

template <typename T>
struct ResampledImage {     // the same element of the image that dsen2_imresize_axis would have written from `mid` ([A][N][B] view)
  const T* mid;
  const double* w;
  const int* idx;
  int P, M, N, B, C, axis;
  __device__ __forceinline__ double operator()(int r, int col, int band) const {
    if (axis == 0) return resample_one<T>(mid + (size_t)col * C + band, w, idx, P, M, N, B, (unsigned)r);
    return resample_one<T>(mid + (size_t)r * N * B + band, w, idx, P, M, N, B, (unsigned)col);
  }
};

static bool float_dtype(int d) { return d == DSEN2_DTYPE_F32 || d == DSEN2_DTYPE_F64; }

// the two images of a metric: pointers, dtypes, bands, and the 2^31-element limit of one launch
static int check_images(const char* who, const void* x, int x_dtype, const void* y, int y_dtype, int H, int W, int C) {
  if (!x || !y || H <= 0 || W <= 0) return fail(DSEN2_ERR_INVALID, "%s: bad argument", who);
  if (C < 1 || C > kQMaxBands) return fail(DSEN2_ERR_INVALID, "%s: %d bands outside 1..%d", who, C, kQMaxBands);
  if (!float_dtype(x_dtype) || !float_dtype(y_dtype))
    return fail(DSEN2_ERR_INVALID, "%s: dtypes %d and %d: not supported (float32 or float64 each)", who, x_dtype, y_dtype);
  if ((size_t)H * W * C >= ((size_t)1 << 31)) return fail(DSEN2_ERR_INVALID, "%s: image too large for one launch (2^31 elements)", who);
  return DSEN2_OK;
}

// a resampling pass of dev_in along `axis` measured against dev_gt, which has the OUTPUT's shape
static int check_resampled(const char* who, const void* in, int dtype, int H, int W, int C, int axis, int out_len, const double* w,
                           const int* idx, int taps, const void* gt, int gt_dtype) {
  if (!in || !w || !idx || !gt || H <= 0 || W <= 0 || out_len <= 0) return fail(DSEN2_ERR_INVALID, "%s: bad argument", who);
  if (C < 1 || C > kQMaxBands) return fail(DSEN2_ERR_INVALID, "%s: %d bands outside 1..%d", who, C, kQMaxBands);
  if (dtype != DSEN2_DTYPE_U16 && !float_dtype(dtype))
    return fail(DSEN2_ERR_INVALID, "%s: dtype %d is not supported (uint16, float32 or float64)", who, dtype);
  if (!float_dtype(gt_dtype)) return fail(DSEN2_ERR_INVALID, "%s: dtype %d is not supported for the ground truth (float32 or float64)", who, gt_dtype);
  if (axis != 0 && axis != 1) return fail(DSEN2_ERR_INVALID, "%s: axis %d (0 = rows, 1 = columns of an HWC image)", who, axis);
  if (taps < 1 || taps > kResizeMaxTaps) return fail(DSEN2_ERR_INVALID, "%s: %d taps outside 1..%d", who, taps, kResizeMaxTaps);
  const int OH = axis == 0 ? out_len : H, OW = axis == 0 ? W : out_len;
  if ((size_t)H * W * C >= ((size_t)1 << 31) || (size_t)OH * OW * C >= ((size_t)1 << 31))
    return fail(DSEN2_ERR_INVALID, "%s: image too large for one launch (2^31 elements)", who);
  return DSEN2_OK;
}

static int check_work(const char* who, int C, const void* work, size_t work_bytes, const void* out) {
  if (!work || !out) return fail(DSEN2_ERR_INVALID, "%s: bad argument", who);
  if (work_bytes < sum_work_bytes(C))
    return fail(DSEN2_ERR_WORKSPACE, "%s: workspace of %zu bytes, dsen2_quality_workspace_bytes asks for %zu", who, work_bytes, sum_work_bytes(C));
  return DSEN2_OK;
}

static int launched(const char* who, hipError_t e) {
  if (e != hipSuccess) return fail(DSEN2_ERR_HIP, "%s launch: %s", who, hipGetErrorString(e));
  return DSEN2_OK;
}

}  // namespace dsen2
