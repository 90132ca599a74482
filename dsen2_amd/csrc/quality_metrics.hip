// quality_metrics.hip — the two further metrics of the paper's evaluation: the universal image quality index (UIQ, Wang & Bovik
// 2002, img_qi.m) per band over sliding block x block windows, and the spectral angle mapper (SAM) per pixel.  All arithmetic is
// float64 with every product and every sum rounded on its own (__dmul_rn / __dadd_rn, `#pragma clang fp contract(off)` and the
// build's -ffp-contract=off), in the order tests/quality_restatement.py writes it down, so that the quality map equals the numpy
// restatement bit for bit.  The only fused multiply-adds in this file are those inside the IEEE float64 division and square root.
//
// UIQ.  Window sums are NOT sliding (add the new, subtract the old): each is the sequential sum of `block` values left to right,
// then of `block` such row sums top to bottom, of x, y, x*x, y*y and x*y.  Then, with N = block^2,
//     s12 = sx*sy   q12 = sx*sx + sy*sy   num = (4*(N*sxy - s12))*s12   den1 = N*(sxx + syy) - q12   den = den1*q12
//     q = 1;   q = (2*s12)/q12 where den1 == 0 and q12 != 0;   q = num/den where den != 0 (applied last).
// TILE: a workgroup of 256 threads produces kUiqTileH x kUiqTileW = 16 x 32 windows of ONE band at a time from a halo tile of
// (16 + block - 1) x (32 + block - 1) samples of x and of y, staged in LDS as float64 (the loader has widened or resampled them).
// Per (tile, band): stage | barrier | horizontal sums of the five quantities, 5 x (16 + block - 1) x 32 doubles in LDS | barrier |
// vertical sums, the formula, one IEEE division per window.  LDS = 8 * (RH * (2 RW + 5 * 32)) bytes with RH = 15 + block, RW = 31 +
// block: 43.8 KB at block 8 (three workgroups per CU of 160 KB), 63.0 KB at block 16 (two).  The workgroup walks the C bands of its
// tile one after the other, so the lanes of a staging load are C elements apart along the contiguous (column, band) index; the
// lines they touch are the ones the next band's loads hit in L1 / L2, and HBM sees every line of a tile once per tile (halo aside).
// Lanes run along the window column in all three phases: conflict-free 8-byte LDS accesses.
// Endings: MAP stores q to map[OH][OW][C] (float64); SUMS adds q up per band and never writes the map: per thread in index
// order, a fixed shuffle tree per wave, the four waves in order, the block's tiles in order, one partial per (block, band), and a
// one-block finish kernel over the blocks' partials.  The grid is min(tiles, kQMaxBlocks): a function of the shape alone, no
// float atomics, so the sums are the same bits on every run.
//
// SAM.  One thread per pixel: d = sum x_c*y_c, nx = sum x_c*x_c, ny = sum y_c*y_c sequentially over the bands from the first
// product; den = sqrt(nx)*sqrt(ny); a pixel with den == 0 is left out; else acos(min(1, max(-1, d/den))) * (180/pi).  Output:
// { sum of angles [deg], pixels used }, reduced like the error sums of imresize.hip (thread, fixed LDS tree, finish kernel).
//
// FUSED BASELINE.  Both kernels are templated on the loaders of x and y.  DirectImage reads x[r][col][band]; ResampledImage
// computes it as the second pass of the bicubic imresize (resample.h: resample_one over the first pass's output, either axis, the
// same tap tables), so that the enlarged image is never written.  The UIQ halo is recomputed per tile.  Same tiles, threads and
// reduction order as the direct form: the same bits as resize, store, then measure.
#include "capi_internal.h"

#pragma clang fp contract(off)

#include "quality_common.h"       // the loaders, the finish kernel and the argument checks shared with ssim.hip

namespace dsen2 {

constexpr int kUiqTileH = 16, kUiqTileW = 32;      // windows per tile (tests/test_gpu_quality_metrics.py reads these two lines)
constexpr int kUiqMinBlock = 2, kUiqMaxBlock = 16;
constexpr double kDegrees = 180.0 / 3.14159265358979323846;

// x, y: [H][W][C] through their loaders.  MAP: map[OH][OW][C] is written.  else partials[block][c] = { sum q, windows } of the block's tiles.
template <class LX, class LY, bool MAP>
__global__ __launch_bounds__(kQThreads) void uiq_kernel(LX x, LY y, int H, int W, int C, int block, int tiles_x, int tiles,
                                                        double* __restrict__ map, double* __restrict__ partials) {
  extern __shared__ double smem[];
  __shared__ double s_acc[kQMaxBands], s_cnt;
  const int RH = kUiqTileH + block - 1, RW = kUiqTileW + block - 1, plane = RH * kUiqTileW;
  double* const rx = smem;                  // [RH][RW]
  double* const ry = rx + RH * RW;          // [RH][RW]
  double* const hs = ry + RH * RW;          // [5][RH][kUiqTileW]: row sums of x, y, x*x, y*y, x*y
  const int tid = threadIdx.x, OH = H - block + 1, OW = W - block + 1;
  const double N = (double)(block * block);
  if (!MAP) {
    if (tid < C) s_acc[tid] = 0.0;
    if (tid == 0) s_cnt = 0.0;
  }
  for (int t = blockIdx.x; t < tiles; t += gridDim.x) {
    const int r0 = t / tiles_x * kUiqTileH, c0 = t % tiles_x * kUiqTileW;
    for (int band = 0; band < C; ++band) {
      for (int i = tid; i < RH * RW; i += kQThreads) {
        const int r = i / RW, gr = r0 + r, gc = c0 + (i - r * RW);
        const bool in = gr < H && gc < W;
        rx[i] = in ? x(gr, gc, band) : 0.0;
        ry[i] = in ? y(gr, gc, band) : 0.0;
      }
      __syncthreads();
      for (int i = tid; i < plane; i += kQThreads) {
        const int r = i / kUiqTileW, c = i % kUiqTileW;
        const double *px = rx + r * RW + c, *py = ry + r * RW + c;
        double a = px[0], b = py[0];
        double sx = a, sy = b, sxx = __dmul_rn(a, a), syy = __dmul_rn(b, b), sxy = __dmul_rn(a, b);
        for (int k = 1; k < block; ++k) {
          a = px[k];
          b = py[k];
          sx = __dadd_rn(sx, a);
          sy = __dadd_rn(sy, b);
          sxx = __dadd_rn(sxx, __dmul_rn(a, a));
          syy = __dadd_rn(syy, __dmul_rn(b, b));
          sxy = __dadd_rn(sxy, __dmul_rn(a, b));
        }
        hs[i] = sx;
        hs[plane + i] = sy;
        hs[2 * plane + i] = sxx;
        hs[3 * plane + i] = syy;
        hs[4 * plane + i] = sxy;
      }
      __syncthreads();
      double qsum = 0.0;
      for (int i = tid; i < kUiqTileH * kUiqTileW; i += kQThreads) {
        const double* p = hs + i;           // window (i / kUiqTileW, i % kUiqTileW): rows i / kUiqTileW .. + block - 1 of its column
        double sx = p[0], sy = p[plane], sxx = p[2 * plane], syy = p[3 * plane], sxy = p[4 * plane];
        for (int k = 1; k < block; ++k) {
          p += kUiqTileW;
          sx = __dadd_rn(sx, p[0]);
          sy = __dadd_rn(sy, p[plane]);
          sxx = __dadd_rn(sxx, p[2 * plane]);
          syy = __dadd_rn(syy, p[3 * plane]);
          sxy = __dadd_rn(sxy, p[4 * plane]);
        }
        const double s12 = __dmul_rn(sx, sy);
        const double q12 = __dadd_rn(__dmul_rn(sx, sx), __dmul_rn(sy, sy));
        const double num = __dmul_rn(__dmul_rn(4.0, __dadd_rn(__dmul_rn(N, sxy), -s12)), s12);
        const double den1 = __dadd_rn(__dmul_rn(N, __dadd_rn(sxx, syy)), -q12);
        const double den = __dmul_rn(den1, q12);
        double q = 1.0;
        if (den != 0.0) q = num / den;
        else if (den1 == 0.0 && q12 != 0.0) q = __dmul_rn(2.0, s12) / q12;
        const int wr = r0 + i / kUiqTileW, wc = c0 + i % kUiqTileW;
        if (wr < OH && wc < OW) {
          if constexpr (MAP) map[((size_t)wr * OW + wc) * C + band] = q;
          else qsum = __dadd_rn(qsum, q);
        }
      }
      if constexpr (!MAP) {
        qsum = wave_then_block_sum(qsum);
        if (tid == 0) {
          s_acc[band] = __dadd_rn(s_acc[band], qsum);
          if (band == 0) {
            const int th = OH - r0 < kUiqTileH ? OH - r0 : kUiqTileH, tw = OW - c0 < kUiqTileW ? OW - c0 : kUiqTileW;
            s_cnt = __dadd_rn(s_cnt, (double)(th * tw));
          }
        }
      }
    }
  }
  if constexpr (!MAP) {
    __syncthreads();
    if (tid < C) {
      partials[((size_t)blockIdx.x * C + tid) * 2 + 0] = s_acc[tid];
      partials[((size_t)blockIdx.x * C + tid) * 2 + 1] = s_cnt;
    }
  }
}

// partials[block] = { sum of the angles in degrees, pixels with a non-zero spectrum in both images }
template <class LX, class LY>
__global__ __launch_bounds__(kQThreads) void sam_kernel(LX x, LY y, int H, int W, int C, double* __restrict__ partials) {
  const unsigned pixels = (unsigned)H * (unsigned)W, step = gridDim.x * kQThreads;
  const int tid = threadIdx.x;
  double sa = 0.0, sn = 0.0;
  for (unsigned p = blockIdx.x * kQThreads + tid; p < pixels; p += step) {
    const int r = (int)(p / (unsigned)W), col = (int)(p - (unsigned)r * (unsigned)W);
    double a = x(r, col, 0), b = y(r, col, 0);
    double d = __dmul_rn(a, b), nx = __dmul_rn(a, a), ny = __dmul_rn(b, b);
    for (int c = 1; c < C; ++c) {
      a = x(r, col, c);
      b = y(r, col, c);
      d = __dadd_rn(d, __dmul_rn(a, b));
      nx = __dadd_rn(nx, __dmul_rn(a, a));
      ny = __dadd_rn(ny, __dmul_rn(b, b));
    }
    const double den = __dmul_rn(sqrt(nx), sqrt(ny));
    if (den != 0.0) {
      double cs = d / den;
      cs = cs < -1.0 ? -1.0 : cs;
      cs = cs > 1.0 ? 1.0 : cs;
      sa = __dadd_rn(sa, __dmul_rn(acos(cs), kDegrees));
      sn = __dadd_rn(sn, 1.0);
    }
  }
  double v[2] = {sa, sn};
  block_tree<2>(v);
  if (tid == 0) {
    partials[(size_t)blockIdx.x * 2 + 0] = v[0];
    partials[(size_t)blockIdx.x * 2 + 1] = v[1];
  }
}

struct QualityCall {
  int H, W, C, block;       // the shape of the two images the metric sees; block: UIQ only
  double *map, *partials, *out;
  hipStream_t stream;
};

template <class LX, class LY, bool MAP>
static hipError_t launch_uiq(const LX& x, const LY& y, const QualityCall& q) {
  const int OH = q.H - q.block + 1, OW = q.W - q.block + 1;
  const int tiles_x = (OW + kUiqTileW - 1) / kUiqTileW, tiles_y = (OH + kUiqTileH - 1) / kUiqTileH;
  const int tiles = tiles_x * tiles_y;          // < 2^31 / 512: H * W is below 2^31
  const int grid = tiles < kQMaxBlocks ? tiles : kQMaxBlocks;
  const int RH = kUiqTileH + q.block - 1, RW = kUiqTileW + q.block - 1;
  const size_t lds = (size_t)RH * (2 * RW + 5 * kUiqTileW) * sizeof(double);
  hipLaunchKernelGGL((uiq_kernel<LX, LY, MAP>), dim3(grid), dim3(kQThreads), lds, q.stream, x, y, q.H, q.W, q.C, q.block, tiles_x, tiles,
                     q.map, q.partials);
  hipError_t e = hipGetLastError();
  if (!MAP && e == hipSuccess) e = launch_finish(q.partials, grid, q.C, 2, 0.0, q.out, q.stream);
  return e;
}

template <class LX, class LY>
static hipError_t launch_sam(const LX& x, const LY& y, const QualityCall& q) {
  const size_t pixels = (size_t)q.H * q.W;
  const size_t want = (pixels + (size_t)kQThreads * 4 - 1) / ((size_t)kQThreads * 4);        // about four pixels per thread
  const int grid = (int)(want > (size_t)kQMaxBlocks ? (size_t)kQMaxBlocks : want);
  hipLaunchKernelGGL((sam_kernel<LX, LY>), dim3(grid), dim3(kQThreads), 0, q.stream, x, y, q.H, q.W, q.C, q.partials);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = launch_finish(q.partials, grid, 1, 2, 0.0, q.out, q.stream);
  return e;
}

enum class Metric { UiqSums, Sam };        // the two endings that reduce; the map has its own entry

template <class LX, class LY>
static hipError_t launch_metric(Metric m, const LX& x, const LY& y, const QualityCall& q) {
  if (m == Metric::Sam) return launch_sam<LX, LY>(x, y, q);
  return launch_uiq<LX, LY, false>(x, y, q);
}

// the ground truth (or second image) is always read directly, float32 or float64
template <class LX>
static hipError_t with_y(Metric m, const LX& x, const void* y, int y_dtype, const QualityCall& q) {
  if (y_dtype == DSEN2_DTYPE_F64) return launch_metric(m, x, DirectImage<double>{static_cast<const double*>(y), q.W, q.C}, q);
  return launch_metric(m, x, DirectImage<float>{static_cast<const float*>(y), q.W, q.C}, q);
}

template <typename T>
static hipError_t map_with_y(const T* x, const void* y, int y_dtype, const QualityCall& q) {
  const DirectImage<T> lx{x, q.W, q.C};
  if (y_dtype == DSEN2_DTYPE_F64) return launch_uiq<DirectImage<T>, DirectImage<double>, true>(lx, DirectImage<double>{static_cast<const double*>(y), q.W, q.C}, q);
  return launch_uiq<DirectImage<T>, DirectImage<float>, true>(lx, DirectImage<float>{static_cast<const float*>(y), q.W, q.C}, q);
}

static int check_block(const char* who, int H, int W, int block) {
  if (block < kUiqMinBlock || block > kUiqMaxBlock)
    return fail(DSEN2_ERR_INVALID, "%s: block size %d outside %d..%d", who, block, kUiqMinBlock, kUiqMaxBlock);
  if (H < block || W < block) return fail(DSEN2_ERR_INVALID, "%s: an image of %d x %d is smaller than the %d x %d block", who, H, W, block, block);
  return DSEN2_OK;
}

// UiqSums or Sam of two stored images
static int direct_metric(const char* who, Metric m, const void* x, int x_dtype, const void* y, int y_dtype, int H, int W, int C, int block,
                         void* work, size_t work_bytes, double* out, void* stream) {
  if (int rc = check_images(who, x, x_dtype, y, y_dtype, H, W, C)) return rc;
  if (m != Metric::Sam)
    if (int rc = check_block(who, H, W, block)) return rc;
  if (int rc = check_work(who, C, work, work_bytes, out)) return rc;
  const QualityCall q{H, W, C, block, nullptr, static_cast<double*>(work), out, (hipStream_t)stream};
  if (x_dtype == DSEN2_DTYPE_F64) return launched(who, with_y(m, DirectImage<double>{static_cast<const double*>(x), W, C}, y, y_dtype, q));
  return launched(who, with_y(m, DirectImage<float>{static_cast<const float*>(x), W, C}, y, y_dtype, q));
}

// UiqSums or Sam of the resampling pass of dev_in along `axis` against dev_gt, which has the OUTPUT's shape
static int resampled_metric(const char* who, Metric m, const void* in, int dtype, int H, int W, int C, int axis, int out_len, const double* w,
                            const int* idx, int taps, const void* gt, int gt_dtype, int block, void* work, size_t work_bytes, double* out,
                            void* stream) {
  if (int rc = check_resampled(who, in, dtype, H, W, C, axis, out_len, w, idx, taps, gt, gt_dtype)) return rc;
  const int OH = axis == 0 ? out_len : H, OW = axis == 0 ? W : out_len;
  if (m != Metric::Sam)
    if (int rc = check_block(who, OH, OW, block)) return rc;
  if (int rc = check_work(who, C, work, work_bytes, out)) return rc;
  const QualityCall q{OH, OW, C, block, nullptr, static_cast<double*>(work), out, (hipStream_t)stream};
  const int N = axis == 0 ? H : W, B = axis == 0 ? W * C : C;
  if (dtype == DSEN2_DTYPE_U16)
    return launched(who, with_y(m, ResampledImage<uint16_t>{static_cast<const uint16_t*>(in), w, idx, taps, out_len, N, B, C, axis}, gt, gt_dtype, q));
  if (dtype == DSEN2_DTYPE_F32)
    return launched(who, with_y(m, ResampledImage<float>{static_cast<const float*>(in), w, idx, taps, out_len, N, B, C, axis}, gt, gt_dtype, q));
  return launched(who, with_y(m, ResampledImage<double>{static_cast<const double*>(in), w, idx, taps, out_len, N, B, C, axis}, gt, gt_dtype, q));
}

}  // namespace dsen2

using namespace dsen2;

extern "C" int dsen2_quality_workspace_bytes(int C, size_t* bytes) {
  if (!bytes || C < 1 || C > kQMaxBands) return fail(DSEN2_ERR_INVALID, "quality_workspace_bytes: %d bands outside 1..%d", C, kQMaxBands);
  *bytes = sum_work_bytes(C);
  return DSEN2_OK;
}

extern "C" int dsen2_uiq_map(const void* dev_x, int x_dtype, const void* dev_y, int y_dtype, int H, int W, int C, int block, double* dev_map,
                             void* stream) {
  return guarded([&]() -> int {
    if (int rc = check_images("uiq_map", dev_x, x_dtype, dev_y, y_dtype, H, W, C)) return rc;
    if (int rc = check_block("uiq_map", H, W, block)) return rc;
    if (!dev_map) return fail(DSEN2_ERR_INVALID, "uiq_map: bad argument");
    const QualityCall q{H, W, C, block, dev_map, nullptr, nullptr, (hipStream_t)stream};
    if (x_dtype == DSEN2_DTYPE_F64) return launched("uiq_map", map_with_y(static_cast<const double*>(dev_x), dev_y, y_dtype, q));
    return launched("uiq_map", map_with_y(static_cast<const float*>(dev_x), dev_y, y_dtype, q));
  });
}

extern "C" int dsen2_uiq_sums(const void* dev_x, int x_dtype, const void* dev_y, int y_dtype, int H, int W, int C, int block, void* dev_work,
                              size_t work_bytes, double* dev_out, void* stream) {
  return guarded([&]() -> int {
    return direct_metric("uiq_sums", Metric::UiqSums, dev_x, x_dtype, dev_y, y_dtype, H, W, C, block, dev_work, work_bytes, dev_out, stream);
  });
}

extern "C" int dsen2_sam_sums(const void* dev_x, int x_dtype, const void* dev_y, int y_dtype, int H, int W, int C, void* dev_work,
                              size_t work_bytes, double* dev_out, void* stream) {
  return guarded([&]() -> int {
    return direct_metric("sam_sums", Metric::Sam, dev_x, x_dtype, dev_y, y_dtype, H, W, C, 0, dev_work, work_bytes, dev_out, stream);
  });
}

extern "C" int dsen2_imresize_uiq_sums(const void* dev_in, int dtype, int H, int W, int C, int axis, int out_len, const double* dev_weights,
                                       const int* dev_indices, int taps, const void* dev_gt, int gt_dtype, int block, void* dev_work,
                                       size_t work_bytes, double* dev_out, void* stream) {
  return guarded([&]() -> int {
    return resampled_metric("imresize_uiq_sums", Metric::UiqSums, dev_in, dtype, H, W, C, axis, out_len, dev_weights, dev_indices, taps, dev_gt,
                            gt_dtype, block, dev_work, work_bytes, dev_out, stream);
  });
}

extern "C" int dsen2_imresize_sam_sums(const void* dev_in, int dtype, int H, int W, int C, int axis, int out_len, const double* dev_weights,
                                       const int* dev_indices, int taps, const void* dev_gt, int gt_dtype, void* dev_work, size_t work_bytes,
                                       double* dev_out, void* stream) {
  return guarded([&]() -> int {
    return resampled_metric("imresize_sam_sums", Metric::Sam, dev_in, dtype, H, W, C, axis, out_len, dev_weights, dev_indices, taps, dev_gt,
                            gt_dtype, 0, dev_work, work_bytes, dev_out, stream);
  });
}
