// down_pixel_aggr.hip — downPixelAggr (utils/patches.py:353-371) of the reference: the simulation of a SCALE x coarser sensor
// that training-set creation runs on every band of a tile.  scipy.ndimage.gaussian_filter(band, 1/SCALE) followed by
// skimage.measure.block_reduce(..., np.mean), reproduced OPERATION BY OPERATION:
//   * per axis (0, then 1), scipy's symmetric correlate1d in float64:  tmp = in[l] * w[r];  for ii = -r .. -1:
//     tmp += (in[l + ii] + in[l - ii]) * w[ii + r]   with the 'reflect' boundary (d c b a | a b c d);
//   * after EACH axis the value is cast to the input's dtype (scipy filters into an output of the input's dtype): uint16
//     truncates, float32 rounds to nearest even;
//   * the float64 sum of each SCALE x SCALE block (row-major), divided by SCALE^2.
// The weights arrive by value from the host (numpy computes them as scipy does): no exp on the device.
//
// NO CONTRACTION.  `tmp + s * w` as an FMA rounds once where scipy rounds twice, and the truncation to uint16 then differs near
// integer boundaries.  Every product and sum of the filter is written with __dmul_rn / __dadd_rn and the file carries
// `#pragma clang fp contract(off)` on top of the build's -ffp-contract=off.  Checked on the generated gfx950 ISA: the
// filter sums are v_mul_f64 / v_add_f64; the only v_fma_f64 of this file are the refinement steps of the IEEE division
// `sum / SCALE^2` (between its v_rcp_f64 and its v_div_fixup_f64; SCALE 2 multiplies by 0.25 and has none).
// tests/test_create_patches_host.py repeats that check on every run of the CPU suite.
//
// One fused launch per image.  A workgroup owns TY x TX output pixels of up to CC channels.  Lanes run along the contiguous
// (x, c) axis; TX is chosen so that the halo tile is ~256 such columns wide (one per thread).
//   1. a thread walks down ITS column of the (TY * S + 2r) x (TX * S + 2r) halo tile: coalesced row loads (independent of the
//      arithmetic, issued several rows ahead), the 2r + 1 rows of the filter's window kept in registers as float64, and the
//      vertical result written to LDS cast to the SOURCE dtype — which is what scipy stores between the two axes, and 2 B per
//      sample of a Sentinel-2 raster: 64 rows x 256 columns = 32 KB, four workgroups per CU.  (The first version staged the
//      input tile in LDS and filtered it in place: 7 LDS operations per sample here and 5 below made it LDS-issue bound at
//      0.20 of the HBM roofline; the window in registers leaves 1 + 3.)
//   2. after one barrier, a thread per (x, c) of the tile row walks down the tile rows (its run-time divisions are per thread,
//      not per output): per output it reads the S + 2r samples of each of its S rows once (taps CC samples apart), filters
//      horizontally, casts, adds up the block and writes one value; consecutive lanes write consecutive (x, c) addresses.
// The run-time form (any scale and radius) reads its vertical taps straight from global memory (L1 / L2 serve the re-reads).
// Measured (profiles/create_patches.md): 10980^2 x 4 uint16 at SCALE 2 in 0.63 ms = 0.29 of the HBM roofline; 34 vector-ALU
// instructions per input sample of which 11 are the un-fused float64 filter and block sum, the rest conversions, 16-bit
// unpacking and addressing: bound by vector-ALU issue, not by HBM (2 B in per sample) and not by the float64 rate.
#include "capi_internal.h"

#pragma clang fp contract(off)

namespace dsen2 {

constexpr int kDownMaxRadius = 8;
constexpr int kDownMaxScale = 32;
constexpr int kDownThreads = 256;
constexpr int kDownMaxChunk = 8;                 // channels of one workgroup (more: grid.z)
constexpr size_t kDownLdsTarget = 40 * 1024;     // four workgroups per CU (160 KB)
constexpr size_t kDownLdsLimit = 64 * 1024;

struct DownWeights {
  double w[2 * kDownMaxRadius + 1];
};

template <typename T> __device__ __forceinline__ T down_cast(double v);
template <> __device__ __forceinline__ uint16_t down_cast<uint16_t>(double v) { return (uint16_t)(unsigned)v; }   // C cast: truncates
template <> __device__ __forceinline__ float down_cast<float>(double v) { return (float)v; }                      // nearest even

// scipy 'reflect' = numpy 'symmetric'.  One reflection (radius <= min(H, W)); a partial tile's rows and columns beyond that feed
// no output and are clamped so that nothing is read outside the image.
__device__ __forceinline__ int down_reflect(int q, int n) {
  if (q < 0) q = -1 - q;
  if (q >= n) q = 2 * n - 1 - q;
  return q < 0 ? 0 : (q >= n ? n - 1 : q);
}

// one output of scipy's symmetric correlate1d (run-time radius): p points at in[l], taps are `step` elements apart
template <typename T>
__device__ __forceinline__ double down_filter(const T* p, int step, int radius, const double* w) {
  double tmp = __dmul_rn((double)p[0], w[radius]);
  for (int ii = -radius; ii < 0; ++ii)
    tmp = __dadd_rn(tmp, __dmul_rn(__dadd_rn((double)p[ii * step], (double)p[-ii * step]), w[ii + radius]));
  return tmp;
}

// S, R > 0: scale and radius at compile time (the two forms training-set creation uses: 2 / 2 and 6 / 1); 0: at run time.
template <typename T, typename OutT, int S, int R>
__global__ __launch_bounds__(kDownThreads) void down_pixel_aggr_kernel(const T* __restrict__ img, int H, int W, int C, int scale_rt,
                                                                       int radius_rt, DownWeights wt, OutT* __restrict__ out,
                                                                       int TY, int TX, int CC) {
  extern __shared__ __align__(16) unsigned char down_smem[];
  __shared__ double w_s[2 * kDownMaxRadius + 1];
  T* const tile = reinterpret_cast<T*>(down_smem);
  const int scale = S > 0 ? S : scale_rt, radius = R > 0 ? R : radius_rt;
  const int tid = threadIdx.x;
  if constexpr (R == 0) {                         // a by-value array indexed at run time would live in scratch
    if (tid <= 2 * radius) w_s[tid] = wt.w[tid];
    __syncthreads();
  }
  const int OH = H / scale, OW = W / scale;
  const int rows = TY * scale, cols = (TX * scale + 2 * radius) * CC;
  const int oy0 = blockIdx.y * TY, ox0 = blockIdx.x * TX, c0 = blockIdx.z * CC;
  const int cc_n = C - c0 < CC ? C - c0 : CC;
  const int y_in0 = oy0 * scale - radius, x_in0 = ox0 * scale - radius;
  const size_t row_stride = (size_t)W * C;

  for (int j = tid; j < cols; j += kDownThreads) {
    const int px = j / CC, cc = j - px * CC;
    if (cc >= cc_n) continue;                     // (the last channel chunk: these columns are never read)
    const T* const src = img + (size_t)down_reflect(x_in0 + px, W) * C + c0 + cc;
    T* const col = tile + j;
    auto sample = [&](int l) { return (double)src[(size_t)down_reflect(y_in0 + l, H) * row_stride]; };   // row l of the halo tile
    if constexpr (R > 0) {
      double win[2 * R + 1];                      // rows l .. l + 2R of the halo tile: the window of output row l
#pragma unroll
      for (int k = 0; k < 2 * R; ++k) win[k + 1] = sample(k);
#pragma unroll 8
      for (int l = 0; l < rows; ++l) {
#pragma unroll
        for (int k = 0; k < 2 * R; ++k) win[k] = win[k + 1];
        win[2 * R] = sample(l + 2 * R);
        double tmp = __dmul_rn(win[R], wt.w[R]);
#pragma unroll
        for (int ii = -R; ii < 0; ++ii) tmp = __dadd_rn(tmp, __dmul_rn(__dadd_rn(win[R + ii], win[R - ii]), wt.w[ii + R]));
        col[l * cols] = down_cast<T>(tmp);
      }
    } else {
      for (int l = 0; l < rows; ++l) {
        double tmp = __dmul_rn(sample(l + radius), w_s[radius]);
        for (int ii = -radius; ii < 0; ++ii)
          tmp = __dadd_rn(tmp, __dmul_rn(__dadd_rn(sample(l + radius + ii), sample(l + radius - ii)), w_s[ii + radius]));
        col[l * cols] = down_cast<T>(tmp);
      }
    }
  }
  __syncthreads();

  // a thread keeps its place (x, c) in the tile row and walks down the tile rows: the run-time divisions are per thread, not per output
  const int per_row = TX * CC;
  const int lanes = per_row < kDownThreads ? per_row : kDownThreads;      // threads along a tile row
  const int row_step = kDownThreads / lanes;                              // tile rows in flight
  const int ty0 = tid / lanes, q0 = tid - ty0 * lanes;
  const double count = (double)(scale * scale);
  for (int q = q0; q < per_row && ty0 < row_step; q += lanes) {
    const int tx = q / CC, cc = q - tx * CC;
    const int ox = ox0 + tx;
    if (cc >= cc_n || ox >= OW) continue;
    for (int ty = ty0; ty < TY && oy0 + ty < OH; ty += row_step) {
      const int oy = oy0 + ty;
      const T* const first = tile + (size_t)(ty * scale) * cols + (tx * scale + radius) * CC + cc;     // block row 0, column 0
      double sum = 0.0;
      if constexpr (S > 0 && R > 0) {
#pragma unroll
        for (int dy = 0; dy < S; ++dy) {
          double v[S + 2 * R];                      // the samples the S filters of this row share, read and converted once
#pragma unroll
          for (int k = 0; k < S + 2 * R; ++k) v[k] = (double)first[dy * cols + (k - R) * CC];
#pragma unroll
          for (int dx = 0; dx < S; ++dx) {
            double tmp = __dmul_rn(v[dx + R], wt.w[R]);
#pragma unroll
            for (int ii = -R; ii < 0; ++ii) tmp = __dadd_rn(tmp, __dmul_rn(__dadd_rn(v[dx + R + ii], v[dx + R - ii]), wt.w[ii + R]));
            sum = __dadd_rn(sum, (double)down_cast<T>(tmp));
          }
        }
      } else {
        for (int dy = 0; dy < scale; ++dy)
          for (int dx = 0; dx < scale; ++dx)
            sum = __dadd_rn(sum, (double)down_cast<T>(down_filter<T>(first + dy * cols + dx * CC, CC, radius, w_s)));
      }
      out[((size_t)oy * OW + ox) * C + c0 + cc] = (OutT)(sum / count);
    }
  }
}

template <typename T, typename OutT>
static hipError_t launch_down(const void* img, int H, int W, int C, int scale, const DownWeights& wt, int radius, void* out,
                              hipStream_t stream, const char** why) {
  int CC = C < kDownMaxChunk ? C : kDownMaxChunk;
  int TX, TY;
  size_t bytes;
  for (;;) {
    TX = (kDownThreads / CC - 2 * radius) / scale;
    if (TX < 1) TX = 1;
    const int cols = (TX * scale + 2 * radius) * CC;
    const int rows_fit = (int)(kDownLdsTarget / ((size_t)cols * sizeof(T)));
    TY = rows_fit / scale;
    TY = TY < 1 ? 1 : (TY > 32 ? 32 : TY);
    bytes = (size_t)(TY * scale) * cols * sizeof(T);
    if (bytes <= kDownLdsLimit || CC == 1) break;
    CC /= 2;
  }
  if (bytes > kDownLdsLimit) { *why = "tile does not fit the LDS"; return hipErrorInvalidValue; }
  const int OH = H / scale, OW = W / scale;
  const dim3 grid((OW + TX - 1) / TX, (OH + TY - 1) / TY, (C + CC - 1) / CC), block(kDownThreads);
  if (grid.y > 65535u || grid.z > 65535u) { *why = "image too large for one launch"; return hipErrorInvalidValue; }
  const T* in = static_cast<const T*>(img);
  OutT* o = static_cast<OutT*>(out);
  if (scale == 2 && radius == 2)
    hipLaunchKernelGGL((down_pixel_aggr_kernel<T, OutT, 2, 2>), grid, block, bytes, stream, in, H, W, C, scale, radius, wt, o, TY, TX, CC);
  else if (scale == 6 && radius == 1)
    hipLaunchKernelGGL((down_pixel_aggr_kernel<T, OutT, 6, 1>), grid, block, bytes, stream, in, H, W, C, scale, radius, wt, o, TY, TX, CC);
  else
    hipLaunchKernelGGL((down_pixel_aggr_kernel<T, OutT, 0, 0>), grid, block, bytes, stream, in, H, W, C, scale, radius, wt, o, TY, TX, CC);
  return hipGetLastError();
}

}  // namespace dsen2

using namespace dsen2;

extern "C" int dsen2_down_pixel_aggr(const void* dev_img, int dtype, int H, int W, int C, int scale, const double* host_weights,
                                     int radius, void* dev_out, int out_f64, void* stream) {
  return guarded([&]() -> int {
    if (!dev_img || !dev_out || !host_weights || H <= 0 || W <= 0 || C <= 0) return fail(DSEN2_ERR_INVALID, "bad argument");
    if (dtype != DSEN2_DTYPE_U16 && dtype != DSEN2_DTYPE_F32) return fail(DSEN2_ERR_INVALID, "dtype %d unknown (uint16 or float32)", dtype);
    if (out_f64 != 0 && out_f64 != 1) return fail(DSEN2_ERR_INVALID, "out_f64 %d (0 = float32, 1 = float64)", out_f64);
    if (scale < 1 || scale > kDownMaxScale) return fail(DSEN2_ERR_INVALID, "scale %d outside 1..%d", scale, kDownMaxScale);
    if (H % scale != 0 || W % scale != 0)
      return fail(DSEN2_ERR_INVALID, "image %d x %d is not a multiple of the scale %d (the reference's downPixelAggr raises ValueError)", H, W, scale);
    if (radius < 0 || radius > kDownMaxRadius) return fail(DSEN2_ERR_INVALID, "radius %d outside 0..%d", radius, kDownMaxRadius);
    if (radius > (H < W ? H : W)) return fail(DSEN2_ERR_INVALID, "radius %d larger than the image %d x %d", radius, H, W);
    DownWeights wt{};
    for (int i = 0; i <= 2 * radius; ++i) wt.w[i] = host_weights[i];
    const char* why = "";
    hipError_t e;
    hipStream_t s = (hipStream_t)stream;
    if (dtype == DSEN2_DTYPE_U16)
      e = out_f64 ? launch_down<uint16_t, double>(dev_img, H, W, C, scale, wt, radius, dev_out, s, &why)
                  : launch_down<uint16_t, float>(dev_img, H, W, C, scale, wt, radius, dev_out, s, &why);
    else
      e = out_f64 ? launch_down<float, double>(dev_img, H, W, C, scale, wt, radius, dev_out, s, &why)
                  : launch_down<float, float>(dev_img, H, W, C, scale, wt, radius, dev_out, s, &why);
    if (e == hipErrorInvalidValue && *why) return fail(DSEN2_ERR_INVALID, "down_pixel_aggr: %s", why);
    if (e != hipSuccess) return fail(DSEN2_ERR_HIP, "down_pixel_aggr launch: %s", hipGetErrorString(e));
    return DSEN2_OK;
  });
}
