// nodata.hip — no-data in, no-data out for tile prediction (include/dsen2_hip.h, "tile no-data").  A 10 m pixel is NO-DATA when
// every one of its bands is exactly 0 (-0.0 counts, a NaN or a negative value is data): the sensor's fill value, not the corpus
// test "band 0 < 1" of corpus_mask.hip.  Integer work only (compares, ballots, ORs; no float arithmetic, no atomics): the result is
// a function of the inputs alone.
//
// dsen2_tile_nodata, two launches on the caller's stream — the bitmap in a row pass of its own, the patch flags from the bitmap
// (the other shape, a workgroup per owned rectangle reading the raster, has to cut the rectangles' columns into 32-aligned pieces
// because two rectangles share a bitmap word; this one has no such case, and the second pass reads 1/128 of the first's bytes):
//   1. bits    nodata_bits_kernel: a workgroup takes 256 consecutive pixels of one row (lanes along x: a wave reads 64 pixels =
//              1 KiB for 4 bands, one 16-byte load per lane), a wave's ballot is two words of the bitmap, written by lanes 0 and 32.
//              Every pixel is read once, every word written once; bits at x >= W are 0.
//   2. flags   nodata_flags_kernel: a workgroup per patch ORs the bitmap words of its owned rectangle (first and last word of a
//              row masked to the rectangle's columns) and writes one byte.
// dsen2_tile_flags_from_bits: launch 2 alone, for a bitmap that came from elsewhere (valid_mask.hip: a class mask).
// dsen2_recompose_rows_nodata: recompose_kernel (patch_ops.hip) with the bitmap and a slot map in front of the patch read.
#include <cstdint>

#include "capi_internal.h"

namespace dsen2 {

namespace {

typedef float nd_f32x4 __attribute__((ext_vector_type(4)));

constexpr int kNThreads = 256;
constexpr int kNMaxBands = 16;

inline unsigned nd_grid_for(size_t work_groups) {
  const size_t cap = 256 * 16;   // 256 CUs x 16 blocks, grid-stride the rest
  return (unsigned)(work_groups < cap ? (work_groups ? work_groups : 1) : cap);
}

// the owned interval of tile t of n along an axis of `extent` pixels: [t * inner, min((t + 1) * inner, extent - inner)), the last
// tile [extent - inner, extent) — what the last patch covering a pixel decides (recompose_kernel)
__host__ __device__ __forceinline__ void owned_interval(int t, int n, int inner, int extent, int* lo, int* hi) {
  if (t == n - 1) {
    *lo = extent - inner;
    *hi = extent;
  } else {
    *lo = t * inner;
    *hi = (t + 1) * inner < extent - inner ? (t + 1) * inner : extent - inner;
  }
}

// C > 0: the band count at compile time (4: one 16-byte load, the pointer is 16-byte aligned); C == 0: c_rt bands
template <int C>
__global__ __launch_bounds__(kNThreads) void nodata_bits_kernel(const float* __restrict__ img, int W, int c_rt, int words_per_row,
                                                                int chunks, size_t items, unsigned* __restrict__ bits) {
  const int lane = threadIdx.x & 63;
  for (size_t it = blockIdx.x; it < items; it += gridDim.x) {          // (uniform over the workgroup: every lane reaches the ballot)
    const size_t y = it / chunks;
    const int x = (int)(it - y * chunks) * kNThreads + (int)threadIdx.x;
    bool valid = false;
    if (x < W) {
      const size_t pix = y * (size_t)W + x;
      if constexpr (C == 4) {
        const nd_f32x4 v = *reinterpret_cast<const nd_f32x4*>(img + pix * 4);
        valid = (v.x != 0.0f) | (v.y != 0.0f) | (v.z != 0.0f) | (v.w != 0.0f);
      } else if constexpr (C > 0) {
        const float* p = img + pix * C;
#pragma unroll
        for (int c = 0; c < C; ++c) valid |= p[c] != 0.0f;
      } else {
        const float* p = img + pix * c_rt;
        for (int c = 0; c < c_rt; ++c) valid |= p[c] != 0.0f;
      }
    }
    const unsigned long long b = __ballot(valid);
    const int word = x >> 5;                                           // lanes 0 and 32: x is a multiple of 32
    if ((lane & 31) == 0 && word < words_per_row) bits[y * (size_t)words_per_row + word] = (unsigned)(b >> lane);
  }
}

// one workgroup per patch k = ty * x_tiles + tx
__global__ __launch_bounds__(kNThreads) void nodata_flags_kernel(const unsigned* __restrict__ bits, int H, int W, int inner, int x_tiles,
                                                                 int y_tiles, int words_per_row, unsigned char* __restrict__ empty) {
  const int k = blockIdx.x;
  const int ty = k / x_tiles, tx = k - ty * x_tiles;
  int y0, y1, x0, x1;
  owned_interval(ty, y_tiles, inner, H, &y0, &y1);
  owned_interval(tx, x_tiles, inner, W, &x0, &x1);
  int any = 0;
  if (y1 > y0 && x1 > x0) {
    const int w0 = x0 >> 5, w1 = (x1 - 1) >> 5, nw = w1 - w0 + 1;
    const unsigned first = ~0u << (x0 & 31);
    const unsigned last = ~0u >> (31 - ((x1 - 1) & 31));
    const int work = (y1 - y0) * nw;
    for (int i = threadIdx.x; i < work; i += kNThreads) {
      const int r = i / nw, wi = w0 + (i - r * nw);
      unsigned word = bits[(size_t)(y0 + r) * words_per_row + wi];
      if (wi == w0) word &= first;
      if (wi == w1) word &= last;
      any |= word != 0u;
    }
  }
  any = __syncthreads_or(any);
  if (threadIdx.x == 0) empty[k] = any ? 0 : 1;
}

// One thread per output PIXEL, as recompose_kernel: a pixel whose bit is 0, or whose patch has no slot in [0, slots), is written
// as 0 and reads no patch.
template <int C>
__global__ __launch_bounds__(kNThreads) void recompose_nodata_kernel(const float* __restrict__ patches, int slots, int P, int border,
                                                                     const int* __restrict__ slot_of_patch,
                                                                     const unsigned* __restrict__ bits, int words_per_row,
                                                                     float* __restrict__ img, int H, int W, int x_tiles, int y_tiles,
                                                                     float scale, size_t first_pix, size_t total_pix, int c_rt) {
  const int inner = P - 2 * border;
  const int cc = C > 0 ? C : c_rt;
  const size_t pp = (size_t)P * P;
  for (size_t i = first_pix + (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total_pix; i += (size_t)gridDim.x * blockDim.x) {
    const int y = (int)(i / W), x = (int)(i - (size_t)y * W);
    float* dst = img + i * cc;
    int slot = -1;
    int ty = 0, tx = 0;
    if ((bits[(size_t)y * words_per_row + (x >> 5)] >> (x & 31)) & 1u) {
      // the LAST tile covering (y, x) wins, as in the reference's sequential overwrite
      ty = (y >= H - inner) ? y_tiles - 1 : y / inner;
      tx = (x >= W - inner) ? x_tiles - 1 : x / inner;
      slot = slot_of_patch[(size_t)ty * x_tiles + tx];
    }
    if (slot < 0 || slot >= slots) {
      if constexpr (C > 0) {
#pragma unroll
        for (int c = 0; c < C; ++c) dst[c] = 0.0f;
      } else {
        for (int c = 0; c < cc; ++c) dst[c] = 0.0f;
      }
      continue;
    }
    const int ys = (ty == y_tiles - 1) ? H - inner : ty * inner;
    const int xs = (tx == x_tiles - 1) ? W - inner : tx * inner;
    const float* src = patches + (size_t)slot * cc * pp + (size_t)(border + y - ys) * P + (border + x - xs);
    if constexpr (C > 0) {
#pragma unroll
      for (int c = 0; c < C; ++c) dst[c] = src[(size_t)c * pp] * scale;
    } else {
      for (int c = 0; c < cc; ++c) dst[c] = src[(size_t)c * pp] * scale;
    }
  }
}

// the geometry every entry refuses alike (dsen2_recompose_rows: inner <= 0, H < inner, W < inner)
int nodata_geometry(const char* who, int H, int W, int P, int border, int* x_tiles, int* y_tiles, int* words_per_row) {
  if (H <= 0 || W <= 0 || P <= 0 || border < 0) return fail(DSEN2_ERR_INVALID, "%s: bad argument", who);
  const long long inner = (long long)P - 2LL * border;
  if (inner <= 0 || H < inner || W < inner)
    return fail(DSEN2_ERR_INVALID, "%s geometry: P=%d border=%d H=%d W=%d", who, P, border, H, W);
  *x_tiles = (int)((W + inner - 1) / inner);
  *y_tiles = (int)((H + inner - 1) / inner);
  *words_per_row = (int)(((long long)W + 31) / 32);
  if ((long long)*x_tiles * *y_tiles >= (1LL << 31)) return fail(DSEN2_ERR_INVALID, "%s: too many patches", who);
  return DSEN2_OK;
}

}  // namespace
}  // namespace dsen2

using namespace dsen2;

extern "C" int dsen2_tile_nodata_geometry(int H, int W, int P, int border, int* x_tiles, int* y_tiles, size_t* bitmap_words) {
  return guarded([&]() -> int {
    if (!x_tiles || !y_tiles || !bitmap_words) return fail(DSEN2_ERR_INVALID, "tile_nodata_geometry: NULL argument");
    int xt = 0, yt = 0, wpr = 0;
    if (int rc = nodata_geometry("tile_nodata", H, W, P, border, &xt, &yt, &wpr)) return rc;
    *x_tiles = xt;
    *y_tiles = yt;
    *bitmap_words = (size_t)H * wpr;
    return DSEN2_OK;
  });
}

extern "C" int dsen2_tile_nodata(const float* dev_img10, int H, int W, int C10, int P, int border, unsigned char* dev_patch_empty,
                                 unsigned int* dev_valid_bits, void* stream) {
  return guarded([&]() -> int {
    if (!dev_img10 || !dev_patch_empty || !dev_valid_bits) return fail(DSEN2_ERR_INVALID, "tile_nodata: NULL argument");
    if (C10 < 1 || C10 > kNMaxBands) return fail(DSEN2_ERR_INVALID, "tile_nodata: %d bands (1..%d)", C10, kNMaxBands);
    int x_tiles = 0, y_tiles = 0, wpr = 0;
    if (int rc = nodata_geometry("tile_nodata", H, W, P, border, &x_tiles, &y_tiles, &wpr)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int chunks = (W + kNThreads - 1) / kNThreads;
    const size_t items = (size_t)H * chunks;
    const dim3 grid(nd_grid_for(items)), block(kNThreads);
    const bool aligned = (reinterpret_cast<uintptr_t>(dev_img10) & 15) == 0;
    if (C10 == 4 && aligned)
      hipLaunchKernelGGL(nodata_bits_kernel<4>, grid, block, 0, st, dev_img10, W, C10, wpr, chunks, items, dev_valid_bits);
    else if (C10 == 6)
      hipLaunchKernelGGL(nodata_bits_kernel<6>, grid, block, 0, st, dev_img10, W, C10, wpr, chunks, items, dev_valid_bits);
    else
      hipLaunchKernelGGL(nodata_bits_kernel<0>, grid, block, 0, st, dev_img10, W, C10, wpr, chunks, items, dev_valid_bits);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(nodata_flags_kernel, dim3((unsigned)(x_tiles * y_tiles)), block, 0, st, dev_valid_bits, H, W, P - 2 * border,
                       x_tiles, y_tiles, wpr, dev_patch_empty);
    HIP_TRY(hipGetLastError());
    return DSEN2_OK;
  });
}

extern "C" int dsen2_tile_flags_from_bits(const unsigned int* dev_valid_bits, int H, int W, int P, int border,
                                          unsigned char* dev_patch_empty, void* stream) {
  return guarded([&]() -> int {
    if (!dev_valid_bits || !dev_patch_empty) return fail(DSEN2_ERR_INVALID, "tile_flags_from_bits: NULL argument");
    int x_tiles = 0, y_tiles = 0, wpr = 0;
    if (int rc = nodata_geometry("tile_flags_from_bits", H, W, P, border, &x_tiles, &y_tiles, &wpr)) return rc;
    hipLaunchKernelGGL(nodata_flags_kernel, dim3((unsigned)(x_tiles * y_tiles)), dim3(kNThreads), 0, (hipStream_t)stream, dev_valid_bits,
                       H, W, P - 2 * border, x_tiles, y_tiles, wpr, dev_patch_empty);
    HIP_TRY(hipGetLastError());
    return DSEN2_OK;
  });
}

extern "C" int dsen2_recompose_rows_nodata(const float* dev_patches, int slots, int C, int P, int border, const int* dev_slot_of_patch,
                                           const unsigned int* dev_valid_bits, float* dev_img, int H, int W, float scale, int row0,
                                           int row1, void* stream) {
  return guarded([&]() -> int {
    if (!dev_slot_of_patch || !dev_valid_bits || !dev_img || (!dev_patches && slots != 0))
      return fail(DSEN2_ERR_INVALID, "recompose_rows_nodata: NULL argument");
    if (slots < 0 || C <= 0) return fail(DSEN2_ERR_INVALID, "recompose_rows_nodata: bad argument (slots=%d C=%d)", slots, C);
    int x_tiles = 0, y_tiles = 0, wpr = 0;
    if (int rc = nodata_geometry("recompose_rows_nodata", H, W, P, border, &x_tiles, &y_tiles, &wpr)) return rc;
    if (row0 < 0 || row1 > H || row0 > row1)
      return fail(DSEN2_ERR_INVALID, "recompose_rows_nodata: rows [%d, %d) of %d", row0, row1, H);
    if (row0 == row1) return DSEN2_OK;
    const size_t first_pix = (size_t)row0 * W, total_pix = (size_t)row1 * W;
    const dim3 grid(nd_grid_for((total_pix - first_pix + kNThreads - 1) / kNThreads)), block(kNThreads);
    hipStream_t st = (hipStream_t)stream;
#define DSEN2_ND_LAUNCH(CC)                                                                                                         \
  hipLaunchKernelGGL(recompose_nodata_kernel<CC>, grid, block, 0, st, dev_patches, slots, P, border, dev_slot_of_patch, dev_valid_bits, \
                     wpr, dev_img, H, W, x_tiles, y_tiles, scale, first_pix, total_pix, C)
    switch (C) {
      case 2: DSEN2_ND_LAUNCH(2); break;
      case 6: DSEN2_ND_LAUNCH(6); break;
      default: DSEN2_ND_LAUNCH(0);
    }
#undef DSEN2_ND_LAUNCH
    HIP_TRY(hipGetLastError());
    return DSEN2_OK;
  });
}
