// imresize.hip — the evaluation step's two kernels: the MATLAB-compatible bicubic `imresize` of the reference (utils/imresize.py, its
// "Bicubic: RMSE ..." baseline) and the per-band error sums that score a prediction or that baseline against a ground truth.
//
// RESAMPLER.  One launch resamples ONE axis of an image with taps the host supplies (dsen2_amd/imresize.py builds them with numpy:
// no pow, no floor, no modulo on the device).  The image is seen as [A][N][B]: N = the axis that is resampled to M outputs,
// B = the contiguous elements below it (axis 0 of an HWC image: A = 1, N = H, B = W * C; axis 1: A = H, N = W, B = C).  Per output
//     out[a][o][b] = sum_k  w[k][o] * (double)in[a][idx[k][o]][b]        k = 0 .. P - 1, IN THAT ORDER,
// every product and every sum rounded on its own: the reference multiplies the P samples by the P weights (np.multiply) and adds
// them up (np.sum, sequential below 8 terms).  So __dmul_rn / __dadd_rn, `#pragma clang fp contract(off)` and the build's
// -ffp-contract=off: no v_fma_f64 may appear in this file at all (tests/test_imresize_host.py reads the ISA).  The sum starts
// from the first product, not from 0.0 (numpy's reduction does; it is what keeps a -0.0).  The input is uint16, float32 or
// float64; what a pass writes is float64 (the reference never casts back), so a second pass reads float64.
//
// Lanes run along the contiguous (o, b) index j of one slice a: consecutive lanes read consecutive addresses of each tap's row
// (axis 0) or of a span of a few pixels (axis 1) and write consecutive float64.  The tap tables are k-major ([P][M]) so that the
// lanes of a wave read consecutive weights too (axis 1: o changes every C lanes; axis 0: one o per wave, a broadcast).  The taps
// (M * P * 12 bytes) stay in L2.  An index outside 0 .. N - 1 cannot come from the host builder; it is clamped anyway so that no
// table can make the kernel read outside the image.
//
// ERROR SUMS.  Per band c of two HWC images x and gt:  sum (x - gt)^2  and  sum gt  in float64, plus the pixel count: all an RMSE or
// the paper's SRE needs.  The order of every sum is FIXED by the shape alone (no float atomics): a block has
// floor(256 / C) * C threads and steps by a multiple of C, so a thread stays on one band and adds its own elements in index
// order; the block adds its threads up in a fixed tree in LDS and writes one partial pair per band; a second one-block kernel
// adds the partials of all blocks, again in a fixed order.  The grid is a function of the shape, never of the device.
// FUSED: the same block structure runs a resampling pass and, instead of storing the float64 value, subtracts the ground truth
// and accumulates: the enlarged image (5.8 GB for the six 20 m bands of a full tile) is never written.
#include "capi_internal.h"

#pragma clang fp contract(off)

#include "fixed_sum.h"       // kQThreads, kQMaxBands, kQMaxBlocks, sum_work_bytes and the finish kernel
#include "resample.h"        // as_double, resample_one, kResizeMaxTaps: shared with quality_metrics.hip

namespace dsen2 {

// the block's per-thread pairs -> one pair per band in partials[block][c][2]; blockDim.x = npix * C, band of a thread = tid % C.
// Not fixed_sum.h's block_tree: this tree runs over the block's npix pixels with a stride of C between them, and npix is
// floor(256 / C), seldom a power of two, so its top level is ragged.
__device__ __forceinline__ void block_band_sums(double sq, double sb, int C, double* __restrict__ partials) {
  __shared__ double s_sq[kQThreads], s_sb[kQThreads];
  const int tid = threadIdx.x, npix = blockDim.x / C, pix = tid / C;
  s_sq[tid] = sq;
  s_sb[tid] = sb;
  __syncthreads();
  int half = 1;
  while (half < npix) half <<= 1;
  for (half >>= 1; half > 0; half >>= 1) {
    if (pix < half && pix + half < npix) {
      s_sq[tid] = __dadd_rn(s_sq[tid], s_sq[tid + half * C]);
      s_sb[tid] = __dadd_rn(s_sb[tid], s_sb[tid + half * C]);
    }
    __syncthreads();
  }
  if (tid < C) {
    const size_t block = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
    partials[(block * C + tid) * 2 + 0] = s_sq[tid];
    partials[(block * C + tid) * 2 + 1] = s_sb[tid];
  }
}

// FUSED = false: out[a][o][b] is written.  FUSED = true: nothing is written but the block's partial error sums against gt, which has
// the output's shape; blockDim.x is then a multiple of C and so is every step of j (M * B is one too: B is a multiple of C).
template <typename T, typename G, bool FUSED>
__global__ __launch_bounds__(kQThreads) void imresize_axis_kernel(const T* __restrict__ in, int A, int N, int B, int M,
                                                                       const double* __restrict__ w, const int* __restrict__ idx, int P,
                                                                       double* __restrict__ out, const G* __restrict__ gt, int C,
                                                                       double* __restrict__ partials) {
  const unsigned MB = (unsigned)M * (unsigned)B, step = gridDim.x * blockDim.x;
  double sq = 0.0, sb = 0.0;
  for (int a = blockIdx.y; a < A; a += gridDim.y) {
    const T* const slice = in + (size_t)a * N * B;
    for (unsigned j = blockIdx.x * blockDim.x + threadIdx.x; j < MB; j += step) {
      const unsigned o = j / (unsigned)B, b = j - o * (unsigned)B;
      const double v = resample_one<T>(slice + b, w, idx, P, M, N, B, o);
      if constexpr (FUSED) {
        const double g = as_double(gt[(size_t)a * MB + j]);
        const double d = __dadd_rn(v, -g);
        sq = __dadd_rn(sq, __dmul_rn(d, d));
        sb = __dadd_rn(sb, g);
      } else {
        out[(size_t)a * MB + j] = v;
      }
    }
  }
  if constexpr (FUSED) block_band_sums(sq, sb, C, partials);
}

// x, gt: n = pixels * C elements, HWC.  blockDim.x and the grid's step are multiples of C.
template <typename X, typename G>
__global__ __launch_bounds__(kQThreads) void band_errors_kernel(const X* __restrict__ x, const G* __restrict__ gt, size_t n, int C,
                                                                     double* __restrict__ partials) {
  const size_t step = (size_t)gridDim.x * blockDim.x;
  double sq = 0.0, sb = 0.0;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += step) {
    const double g = as_double(gt[i]);
    const double d = __dadd_rn(as_double(x[i]), -g);
    sq = __dadd_rn(sq, __dmul_rn(d, d));
    sb = __dadd_rn(sb, g);
  }
  block_band_sums(sq, sb, C, partials);
}

struct AxisShape {
  int A, N, B, M;
};

// argument checks shared by the resampling entries; fills the [A][N][B] view
static int axis_shape(const char* who, const void* in, int dtype, int H, int W, int C, int axis, int out_len, const void* w,
                      const void* idx, int taps, AxisShape* s) {
  if (!in || !w || !idx || H <= 0 || W <= 0 || C <= 0 || out_len <= 0) return fail(DSEN2_ERR_INVALID, "%s: bad argument", who);
  if (dtype != DSEN2_DTYPE_U16 && dtype != DSEN2_DTYPE_F32 && dtype != DSEN2_DTYPE_F64)
    return fail(DSEN2_ERR_INVALID, "%s: dtype %d is not supported (uint16, float32 or float64; uint8, which the reference rounds, is refused)", who, dtype);
  if (axis != 0 && axis != 1) return fail(DSEN2_ERR_INVALID, "%s: axis %d (0 = rows, 1 = columns of an HWC image)", who, axis);
  if (taps < 1 || taps > kResizeMaxTaps) return fail(DSEN2_ERR_INVALID, "%s: %d taps outside 1..%d", who, taps, kResizeMaxTaps);
  *s = AxisShape{axis == 0 ? 1 : H, axis == 0 ? H : W, 0, out_len};
  const size_t B = axis == 0 ? (size_t)W * C : (size_t)C;
  if (B * (size_t)out_len >= ((size_t)1 << 31) || (size_t)s->N * B >= ((size_t)1 << 31))
    return fail(DSEN2_ERR_INVALID, "%s: image too large for one launch (2^31 elements per slice)", who);
  s->B = (int)B;
  return DSEN2_OK;
}

static int check_bands(const char* who, int C, int gt_dtype, const void* gt, const void* work, size_t work_bytes, const void* out) {
  if (!gt || !work || !out) return fail(DSEN2_ERR_INVALID, "%s: bad argument", who);
  if (C < 1 || C > kQMaxBands) return fail(DSEN2_ERR_INVALID, "%s: %d bands outside 1..%d", who, C, kQMaxBands);
  if (gt_dtype != DSEN2_DTYPE_F32 && gt_dtype != DSEN2_DTYPE_F64)
    return fail(DSEN2_ERR_INVALID, "%s: dtype %d is not supported for the ground truth (float32 or float64)", who, gt_dtype);
  if (work_bytes < sum_work_bytes(C))
    return fail(DSEN2_ERR_WORKSPACE, "%s: workspace of %zu bytes, dsen2_band_errors_workspace_bytes asks for %zu", who, work_bytes,
                sum_work_bytes(C));
  return DSEN2_OK;
}

template <typename T, typename G, bool FUSED>
static void launch_axis(const void* in, const AxisShape& s, const double* w, const int* idx, int P, double* out, const void* gt, int C,
                        double* partials, dim3 grid, int threads, hipStream_t stream) {
  hipLaunchKernelGGL((imresize_axis_kernel<T, G, FUSED>), grid, dim3(threads), 0, stream, static_cast<const T*>(in), s.A, s.N, s.B, s.M,
                     w, idx, P, out, static_cast<const G*>(gt), C, partials);
}

}  // namespace dsen2

using namespace dsen2;

extern "C" int dsen2_imresize_axis(const void* dev_in, int dtype, int H, int W, int C, int axis, int out_len, const double* dev_weights,
                                   const int* dev_indices, int taps, double* dev_out, void* stream) {
  return guarded([&]() -> int {
    AxisShape s;
    if (!dev_out) return fail(DSEN2_ERR_INVALID, "imresize_axis: bad argument");
    if (int rc = axis_shape("imresize_axis", dev_in, dtype, H, W, C, axis, out_len, dev_weights, dev_indices, taps, &s)) return rc;
    const unsigned MB = (unsigned)s.M * (unsigned)s.B;
    const dim3 grid((MB + kQThreads - 1) / kQThreads, s.A < 65535 ? s.A : 65535);
    hipStream_t st = (hipStream_t)stream;
    if (dtype == DSEN2_DTYPE_U16)
      launch_axis<uint16_t, double, false>(dev_in, s, dev_weights, dev_indices, taps, dev_out, nullptr, C, nullptr, grid, kQThreads, st);
    else if (dtype == DSEN2_DTYPE_F32)
      launch_axis<float, double, false>(dev_in, s, dev_weights, dev_indices, taps, dev_out, nullptr, C, nullptr, grid, kQThreads, st);
    else
      launch_axis<double, double, false>(dev_in, s, dev_weights, dev_indices, taps, dev_out, nullptr, C, nullptr, grid, kQThreads, st);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(DSEN2_ERR_HIP, "imresize_axis launch: %s", hipGetErrorString(e));
    return DSEN2_OK;
  });
}

extern "C" int dsen2_band_errors_workspace_bytes(int C, size_t* bytes) {
  if (!bytes || C < 1 || C > kQMaxBands) return fail(DSEN2_ERR_INVALID, "band_errors_workspace_bytes: %d bands outside 1..%d", C, kQMaxBands);
  *bytes = sum_work_bytes(C);
  return DSEN2_OK;
}

extern "C" int dsen2_band_errors(const void* dev_x, int x_dtype, const void* dev_gt, int gt_dtype, int H, int W, int C, void* dev_work,
                                 size_t work_bytes, double* dev_out, void* stream) {
  return guarded([&]() -> int {
    if (!dev_x || H <= 0 || W <= 0) return fail(DSEN2_ERR_INVALID, "band_errors: bad argument");
    if (int rc = check_bands("band_errors", C, gt_dtype, dev_gt, dev_work, work_bytes, dev_out)) return rc;
    if (x_dtype != DSEN2_DTYPE_F32 && x_dtype != DSEN2_DTYPE_F64)
      return fail(DSEN2_ERR_INVALID, "band_errors: dtype %d is not supported (float32 or float64)", x_dtype);
    const size_t pixels = (size_t)H * W, n = pixels * C;
    const int threads = kQThreads / C * C;
    const size_t want = (n + (size_t)threads * 8 - 1) / ((size_t)threads * 8);        // about eight elements per thread
    const int blocks = (int)(want < 1 ? 1 : (want > kQMaxBlocks ? kQMaxBlocks : want));
    double* partials = static_cast<double*>(dev_work);
    hipStream_t st = (hipStream_t)stream;
    const bool x64 = x_dtype == DSEN2_DTYPE_F64, g64 = gt_dtype == DSEN2_DTYPE_F64;
    if (x64 && g64)
      hipLaunchKernelGGL((band_errors_kernel<double, double>), dim3(blocks), dim3(threads), 0, st, (const double*)dev_x, (const double*)dev_gt, n, C, partials);
    else if (x64)
      hipLaunchKernelGGL((band_errors_kernel<double, float>), dim3(blocks), dim3(threads), 0, st, (const double*)dev_x, (const float*)dev_gt, n, C, partials);
    else if (g64)
      hipLaunchKernelGGL((band_errors_kernel<float, double>), dim3(blocks), dim3(threads), 0, st, (const float*)dev_x, (const double*)dev_gt, n, C, partials);
    else
      hipLaunchKernelGGL((band_errors_kernel<float, float>), dim3(blocks), dim3(threads), 0, st, (const float*)dev_x, (const float*)dev_gt, n, C, partials);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = launch_finish(partials, blocks, C, 3, (double)pixels, dev_out, st);
    if (e != hipSuccess) return fail(DSEN2_ERR_HIP, "band_errors launch: %s", hipGetErrorString(e));
    return DSEN2_OK;
  });
}

extern "C" int dsen2_imresize_band_errors(const void* dev_in, int dtype, int H, int W, int C, int axis, int out_len,
                                          const double* dev_weights, const int* dev_indices, int taps, const void* dev_gt, int gt_dtype,
                                          void* dev_work, size_t work_bytes, double* dev_out, void* stream) {
  return guarded([&]() -> int {
    AxisShape s;
    if (int rc = axis_shape("imresize_band_errors", dev_in, dtype, H, W, C, axis, out_len, dev_weights, dev_indices, taps, &s)) return rc;
    if (int rc = check_bands("imresize_band_errors", C, gt_dtype, dev_gt, dev_work, work_bytes, dev_out)) return rc;
    const int threads = kQThreads / C * C;
    const unsigned MB = (unsigned)s.M * (unsigned)s.B;
    unsigned gx = (MB + threads - 1) / threads;
    if (gx > (unsigned)kQMaxBlocks) gx = kQMaxBlocks;
    unsigned gy = kQMaxBlocks / gx;
    if (gy > (unsigned)s.A) gy = s.A;
    const dim3 grid(gx, gy);
    double* partials = static_cast<double*>(dev_work);
    hipStream_t st = (hipStream_t)stream;
    const bool g64 = gt_dtype == DSEN2_DTYPE_F64;
#define DSEN2_FUSED(T)                                                                                                        \
  (g64 ? launch_axis<T, double, true>(dev_in, s, dev_weights, dev_indices, taps, nullptr, dev_gt, C, partials, grid, threads, st) \
       : launch_axis<T, float, true>(dev_in, s, dev_weights, dev_indices, taps, nullptr, dev_gt, C, partials, grid, threads, st))
    if (dtype == DSEN2_DTYPE_U16) DSEN2_FUSED(uint16_t);
    else if (dtype == DSEN2_DTYPE_F32) DSEN2_FUSED(float);
    else DSEN2_FUSED(double);
#undef DSEN2_FUSED
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) {
      const size_t pixels = axis == 0 ? (size_t)out_len * W : (size_t)H * out_len;
      e = launch_finish(partials, (int)(gx * gy), C, 3, (double)pixels, dev_out, st);
    }
    if (e != hipSuccess) return fail(DSEN2_ERR_HIP, "imresize_band_errors launch: %s", hipGetErrorString(e));
    return DSEN2_OK;
  });
}
