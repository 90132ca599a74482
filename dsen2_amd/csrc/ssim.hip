// ssim.hip — the structural similarity index (Wang, Bovik, Sheikh & Simoncelli 2004, ssim_index.m without its automatic
// down-sampling) per band: a Gaussian window of P x P weights over valid windows only, the biased (population) covariance.  All
// arithmetic is float64 with every product and every sum rounded on its own (__dmul_rn / __dadd_rn, `#pragma clang fp contract(off)`
// and the build's -ffp-contract=off), in the order tests/ssim_restatement.py writes it down, so that the map equals the numpy
// restatement bit for bit.  The only fused multiply-adds in this file are those inside the IEEE float64 division.
//
// WINDOW.  P normalised weights w[0 .. P-1] (P odd, 3..15), computed by the host (metrics.ssim_window) and passed by value: the
// device never calls exp.  The filter is separable and the same for the five fields f = x, y, x*x, y*y, x*y (products first,
// each rounded):  row pass r[y][c] = w[0]*f[y][c], then r = r + w[k]*f[y][c+k] for k = 1 .. P-1 in order; column pass the same
// sequential sum over r[y+k][c].  Then, with mx, my, exx, eyy, exy the five filtered fields of a window,
//     m11 = mx*mx   m22 = my*my   m12 = mx*my   s1 = exx - m11   s2 = eyy - m22   s12 = exy - m12
//     num = (2*m12 + C1)*(2*s12 + C2)   den = ((m11 + m22) + C1)*((s1 + s2) + C2)   q = num/den.
// C1, C2 > 0 are the host's (K1 L)^2 and (K2 L)^2.
// TILE: as uiq_kernel (quality_metrics.hip).  A workgroup of 256 threads produces kSsimTileH x kSsimTileW = 16 x 32 windows of ONE
// band at a time from a halo tile of (15 + P) x (31 + P) samples of x and of y, staged in LDS as float64 through the loaders.  Per
// (tile, band): stage | barrier | row pass of the five fields, 5 x (15 + P) x 32 doubles in LDS | barrier | column pass, the
// formula, one IEEE division per window.  LDS = 8 * (15 + P) * (2 (31 + P) + 5 * 32) bytes: 48.8 KB at P = 11, 60.5 KB at P = 15.
// Lanes run along the window column in all three phases: conflict-free 8-byte LDS accesses.  The workgroup walks the C bands of
// its tile in turn.  Samples outside the image are staged as zeros and only reach windows that are neither stored nor summed.
// Endings: MAP stores q to map[OH][OW][C] (float64); SUMS adds q up per band and never writes the map: per thread in index
// order, a fixed shuffle tree per wave, the four waves in order, the block's tiles in order, one partial per (block, band), and the
// one-block finish kernel over the blocks' partials (fixed_sum.h).  The grid is min(tiles, kQMaxBlocks): a function of the
// shape alone, no float atomics, so the sums are the same bits on every run.
//
// FUSED BASELINE.  The kernel is a template over the loaders of x and y (quality_common.h).  With ResampledImage for x the halo
// tile is the second pass of the bicubic imresize, recomputed per tile and never written.  Same tiles, threads and reduction order
// as the direct form: the same bits as resize, store, then measure.
#include "capi_internal.h"

#include <cmath>

#pragma clang fp contract(off)

#include "quality_common.h"

namespace dsen2 {

constexpr int kSsimTileH = 16, kSsimTileW = 32;    // windows per tile
constexpr int kSsimMinWin = 3, kSsimMaxWin = 15;

struct SsimWindow {
  double w[kSsimMaxWin];
};

// x, y: [H][W][C] through their loaders.  MAP: map[OH][OW][C] is written.  else partials[block][c] = { sum q, windows } of the block's tiles.
template <class LX, class LY, bool MAP>
__global__ __launch_bounds__(kQThreads) void ssim_kernel(LX x, LY y, int H, int W, int C, int P, SsimWindow win, double c1, double c2,
                                                         int tiles_x, int tiles, double* __restrict__ map, double* __restrict__ partials) {
  extern __shared__ double smem[];
  __shared__ double s_w[kSsimMaxWin], s_acc[kQMaxBands], s_cnt;
  const int RH = kSsimTileH + P - 1, RW = kSsimTileW + P - 1, plane = RH * kSsimTileW;
  double* const rx = smem;                  // [RH][RW]
  double* const ry = rx + RH * RW;          // [RH][RW]
  double* const hs = ry + RH * RW;          // [5][RH][kSsimTileW]: row pass of x, y, x*x, y*y, x*y
  const int tid = threadIdx.x, OH = H - P + 1, OW = W - P + 1;
  if (tid < kSsimMaxWin) s_w[tid] = tid < P ? win.w[tid] : 0.0;          // read with a loop index below: LDS broadcasts it
  if (!MAP) {
    if (tid < C) s_acc[tid] = 0.0;
    if (tid == 0) s_cnt = 0.0;
  }
  for (int t = blockIdx.x; t < tiles; t += gridDim.x) {
    const int r0 = t / tiles_x * kSsimTileH, c0 = t % tiles_x * kSsimTileW;
    for (int band = 0; band < C; ++band) {
      for (int i = tid; i < RH * RW; i += kQThreads) {
        const int r = i / RW, gr = r0 + r, gc = c0 + (i - r * RW);
        const bool in = gr < H && gc < W;
        rx[i] = in ? x(gr, gc, band) : 0.0;
        ry[i] = in ? y(gr, gc, band) : 0.0;
      }
      __syncthreads();                      // also orders s_w before its first use
      for (int i = tid; i < plane; i += kQThreads) {
        const int r = i / kSsimTileW, c = i % kSsimTileW;
        const double *px = rx + r * RW + c, *py = ry + r * RW + c;
        double wk = s_w[0], a = px[0], b = py[0];
        double fx = __dmul_rn(wk, a), fy = __dmul_rn(wk, b);
        double fxx = __dmul_rn(wk, __dmul_rn(a, a)), fyy = __dmul_rn(wk, __dmul_rn(b, b)), fxy = __dmul_rn(wk, __dmul_rn(a, b));
        for (int k = 1; k < P; ++k) {
          wk = s_w[k];
          a = px[k];
          b = py[k];
          fx = __dadd_rn(fx, __dmul_rn(wk, a));
          fy = __dadd_rn(fy, __dmul_rn(wk, b));
          fxx = __dadd_rn(fxx, __dmul_rn(wk, __dmul_rn(a, a)));
          fyy = __dadd_rn(fyy, __dmul_rn(wk, __dmul_rn(b, b)));
          fxy = __dadd_rn(fxy, __dmul_rn(wk, __dmul_rn(a, b)));
        }
        hs[i] = fx;
        hs[plane + i] = fy;
        hs[2 * plane + i] = fxx;
        hs[3 * plane + i] = fyy;
        hs[4 * plane + i] = fxy;
      }
      __syncthreads();
      double qsum = 0.0;
      for (int i = tid; i < kSsimTileH * kSsimTileW; i += kQThreads) {
        const double* p = hs + i;           // window (i / kSsimTileW, i % kSsimTileW): rows i / kSsimTileW .. + P - 1 of its column
        double wk = s_w[0];
        double mx = __dmul_rn(wk, p[0]), my = __dmul_rn(wk, p[plane]);
        double exx = __dmul_rn(wk, p[2 * plane]), eyy = __dmul_rn(wk, p[3 * plane]), exy = __dmul_rn(wk, p[4 * plane]);
        for (int k = 1; k < P; ++k) {
          p += kSsimTileW;
          wk = s_w[k];
          mx = __dadd_rn(mx, __dmul_rn(wk, p[0]));
          my = __dadd_rn(my, __dmul_rn(wk, p[plane]));
          exx = __dadd_rn(exx, __dmul_rn(wk, p[2 * plane]));
          eyy = __dadd_rn(eyy, __dmul_rn(wk, p[3 * plane]));
          exy = __dadd_rn(exy, __dmul_rn(wk, p[4 * plane]));
        }
        const double m11 = __dmul_rn(mx, mx), m22 = __dmul_rn(my, my), m12 = __dmul_rn(mx, my);
        const double s1 = __dadd_rn(exx, -m11), s2 = __dadd_rn(eyy, -m22), s12 = __dadd_rn(exy, -m12);
        const double num = __dmul_rn(__dadd_rn(__dmul_rn(2.0, m12), c1), __dadd_rn(__dmul_rn(2.0, s12), c2));
        const double den = __dmul_rn(__dadd_rn(__dadd_rn(m11, m22), c1), __dadd_rn(__dadd_rn(s1, s2), c2));
        const double q = num / den;
        const int wr = r0 + i / kSsimTileW, wc = c0 + i % kSsimTileW;
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
            const int th = OH - r0 < kSsimTileH ? OH - r0 : kSsimTileH, tw = OW - c0 < kSsimTileW ? OW - c0 : kSsimTileW;
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

struct SsimCall {
  int H, W, C, P;           // the shape of the two images the metric sees, the window size
  SsimWindow win;
  double c1, c2;
  double *map, *partials, *out;
  hipStream_t stream;
};

template <class LX, class LY, bool MAP>
static hipError_t launch_ssim(const LX& x, const LY& y, const SsimCall& q) {
  const int OH = q.H - q.P + 1, OW = q.W - q.P + 1;
  const int tiles_x = (OW + kSsimTileW - 1) / kSsimTileW, tiles_y = (OH + kSsimTileH - 1) / kSsimTileH;
  const int tiles = tiles_x * tiles_y;          // < 2^31 / 512: H * W is below 2^31
  const int grid = tiles < kQMaxBlocks ? tiles : kQMaxBlocks;
  const int RH = kSsimTileH + q.P - 1, RW = kSsimTileW + q.P - 1;
  const size_t lds = (size_t)RH * (2 * RW + 5 * kSsimTileW) * sizeof(double);
  hipLaunchKernelGGL((ssim_kernel<LX, LY, MAP>), dim3(grid), dim3(kQThreads), lds, q.stream, x, y, q.H, q.W, q.C, q.P, q.win, q.c1, q.c2,
                     tiles_x, tiles, q.map, q.partials);
  hipError_t e = hipGetLastError();
  if (!MAP && e == hipSuccess) e = launch_finish(q.partials, grid, q.C, 2, 0.0, q.out, q.stream);
  return e;
}

// the ground truth (or second image) is always read directly, float32 or float64
template <bool MAP, class LX>
static hipError_t ssim_with_y(const LX& x, const void* y, int y_dtype, const SsimCall& q) {
  if (y_dtype == DSEN2_DTYPE_F64) return launch_ssim<LX, DirectImage<double>, MAP>(x, DirectImage<double>{static_cast<const double*>(y), q.W, q.C}, q);
  return launch_ssim<LX, DirectImage<float>, MAP>(x, DirectImage<float>{static_cast<const float*>(y), q.W, q.C}, q);
}

template <bool MAP>
static hipError_t ssim_direct(const void* x, int x_dtype, const void* y, int y_dtype, const SsimCall& q) {
  if (x_dtype == DSEN2_DTYPE_F64) return ssim_with_y<MAP>(DirectImage<double>{static_cast<const double*>(x), q.W, q.C}, y, y_dtype, q);
  return ssim_with_y<MAP>(DirectImage<float>{static_cast<const float*>(x), q.W, q.C}, y, y_dtype, q);
}

// the window, the two constants and the image against the window; fills `q`'s window
static int check_window(const char* who, int H, int W, const double* host_window, int win, double c1, double c2, SsimCall* q) {
  if (!host_window) return fail(DSEN2_ERR_INVALID, "%s: bad argument", who);
  if (win < kSsimMinWin || win > kSsimMaxWin || win % 2 == 0)
    return fail(DSEN2_ERR_INVALID, "%s: window size %d is not odd or outside %d..%d", who, win, kSsimMinWin, kSsimMaxWin);
  if (H < win || W < win) return fail(DSEN2_ERR_INVALID, "%s: an image of %d x %d is smaller than the %d x %d window", who, H, W, win, win);
  if (!std::isfinite(c1) || !std::isfinite(c2) || !(c1 > 0.0) || !(c2 > 0.0))
    return fail(DSEN2_ERR_INVALID, "%s: constants c1 = %g and c2 = %g must be finite and positive", who, c1, c2);
  for (int i = 0; i < kSsimMaxWin; ++i) q->win.w[i] = 0.0;
  for (int i = 0; i < win; ++i) {
    if (!std::isfinite(host_window[i])) return fail(DSEN2_ERR_INVALID, "%s: window entry %d is not finite", who, i);
    q->win.w[i] = host_window[i];
  }
  q->P = win;
  q->c1 = c1;
  q->c2 = c2;
  return DSEN2_OK;
}

}  // namespace dsen2

using namespace dsen2;

extern "C" int dsen2_ssim_map(const void* dev_x, int x_dtype, const void* dev_y, int y_dtype, int H, int W, int C, const double* host_window,
                              int win, double c1, double c2, double* dev_map, void* stream) {
  return guarded([&]() -> int {
    SsimCall q{H, W, C, 0, {}, 0.0, 0.0, dev_map, nullptr, nullptr, (hipStream_t)stream};
    if (int rc = check_images("ssim_map", dev_x, x_dtype, dev_y, y_dtype, H, W, C)) return rc;
    if (int rc = check_window("ssim_map", H, W, host_window, win, c1, c2, &q)) return rc;
    if (!dev_map) return fail(DSEN2_ERR_INVALID, "ssim_map: bad argument");
    return launched("ssim_map", ssim_direct<true>(dev_x, x_dtype, dev_y, y_dtype, q));
  });
}

extern "C" int dsen2_ssim_sums(const void* dev_x, int x_dtype, const void* dev_y, int y_dtype, int H, int W, int C, const double* host_window,
                               int win, double c1, double c2, void* dev_work, size_t work_bytes, double* dev_out, void* stream) {
  return guarded([&]() -> int {
    SsimCall q{H, W, C, 0, {}, 0.0, 0.0, nullptr, static_cast<double*>(dev_work), dev_out, (hipStream_t)stream};
    if (int rc = check_images("ssim_sums", dev_x, x_dtype, dev_y, y_dtype, H, W, C)) return rc;
    if (int rc = check_window("ssim_sums", H, W, host_window, win, c1, c2, &q)) return rc;
    if (int rc = check_work("ssim_sums", C, dev_work, work_bytes, dev_out)) return rc;
    return launched("ssim_sums", ssim_direct<false>(dev_x, x_dtype, dev_y, y_dtype, q));
  });
}

extern "C" int dsen2_imresize_ssim_sums(const void* dev_in, int dtype, int H, int W, int C, int axis, int out_len, const double* dev_weights,
                                        const int* dev_indices, int taps, const void* dev_gt, int gt_dtype, const double* host_window, int win,
                                        double c1, double c2, void* dev_work, size_t work_bytes, double* dev_out, void* stream) {
  return guarded([&]() -> int {
    const char* who = "imresize_ssim_sums";
    if (int rc = check_resampled(who, dev_in, dtype, H, W, C, axis, out_len, dev_weights, dev_indices, taps, dev_gt, gt_dtype)) return rc;
    const int OH = axis == 0 ? out_len : H, OW = axis == 0 ? W : out_len;
    SsimCall q{OH, OW, C, 0, {}, 0.0, 0.0, nullptr, static_cast<double*>(dev_work), dev_out, (hipStream_t)stream};
    if (int rc = check_window(who, OH, OW, host_window, win, c1, c2, &q)) return rc;
    if (int rc = check_work(who, C, dev_work, work_bytes, dev_out)) return rc;
    const int N = axis == 0 ? H : W, B = axis == 0 ? W * C : C;
    if (dtype == DSEN2_DTYPE_U16)
      return launched(who, ssim_with_y<false>(ResampledImage<uint16_t>{static_cast<const uint16_t*>(dev_in), dev_weights, dev_indices, taps, out_len, N, B, C, axis},
                                              dev_gt, gt_dtype, q));
    if (dtype == DSEN2_DTYPE_F32)
      return launched(who, ssim_with_y<false>(ResampledImage<float>{static_cast<const float*>(dev_in), dev_weights, dev_indices, taps, out_len, N, B, C, axis},
                                              dev_gt, gt_dtype, q));
    return launched(who, ssim_with_y<false>(ResampledImage<double>{static_cast<const double*>(dev_in), dev_weights, dev_indices, taps, out_len, N, B, C, axis},
                                            dev_gt, gt_dtype, q));
  });
}
