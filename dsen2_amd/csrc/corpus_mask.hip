// corpus_mask.hip — which crop origins of a tile may be drawn (include/dsen2_hip.h, "corpus origin mask"): an origin is VALID when
// none of the 16 x 16 cells of the origin grid its crop covers is blank (a band-0 sample of the raw 10 m raster in the cell's
// F x F footprint fails v >= 1: the reference's `chan3 < 1` test, training/create_patches.py:208-211) or covered (inside a
// hold-out rectangle: a validation crop grown by `margin` cells).  Integer work only: flags, ORs, ballots and an integer count;
// the result is a function of the inputs alone.
//
// Two launches on the caller's stream, three with a hold-out table (the count is formed inside the last):
//   1. cells    blank_cells_kernel: one byte per cell from the raster (or cells_from_map_kernel: from a blank map a previous call
//               left).  Lanes run along x of the raster: a wave reads band 0 of 64 consecutive pixels, whose sectors it shares
//               with the other bands — the raster's bytes are the traffic of the whole entry.  A thread ORs its column over the
//               footprint's rows, LDS joins the F columns of a cell.
//   2. hold-out holdout_cells_kernel: one workgroup per rectangle, clipped to the grid, plain stores of the value 1 (every writer
//               of a cell stores the same byte: no order to depend on).
//   3. window   origin_window_kernel: a workgroup takes 16 rows x 64 columns of origins; it stages the 31 x 79 cells they reach in
//               LDS, ORs 16 cells along x, then 16 of those along y (the separable 16 x 16 window), and each wave turns one row of
//               64 origins into 8 bytes with one ballot: bit k of byte b of a row is origin 8 b + k, least significant bit first
//               (np.packbits(valid, axis=1, bitorder='little')); the padding bits of a row's last byte are written as 0.
//      count    in the same kernel: popcounts of the ballots, added per workgroup and then with ONE integer atomicAdd per
//               workgroup onto the count, which kernel 1 has set to 0 (integer addition: any order gives the same number).
#include "capi_internal.h"

namespace dsen2 {

namespace {

constexpr int kMCrop = 16;                      // edge of a crop on the origin grid
constexpr int kMThreads = 256;
constexpr int kMTileX = 64, kMTileY = 16;       // origins of one workgroup of origin_window_kernel
constexpr int kMCellsX = kMTileX + kMCrop - 1;  // 79 cells along x reach them
constexpr int kMCellsY = kMTileY + kMCrop - 1;  // 31 along y
constexpr int kMMaxGrid = 1 << 15;              // origin-grid extent per axis: (grid - 15)^2 origins fit the int32 count
constexpr int kMMaxMargin = 1 << 20;
constexpr int kMMaxHoldout = 1 << 24;           // rectangles per call

template <typename T>
__device__ __forceinline__ bool blank_sample(T v);
template <>
__device__ __forceinline__ bool blank_sample<unsigned short>(unsigned short v) { return v < 1; }
template <>
__device__ __forceinline__ bool blank_sample<float>(float v) { return !(v >= 1.0f); }      // a NaN is blank

// F x F samples per cell.  A workgroup: ROWS cell rows x (256 / F) cells; thread t < CPB * F is raster column x0 + t.
template <typename T, int F, int ROWS>
__global__ __launch_bounds__(kMThreads) void blank_cells_kernel(const T* __restrict__ img, int W, int C, int grid_h, int grid_w,
                                                                unsigned char* __restrict__ cells, int* __restrict__ count) {
  constexpr int CPB = kMThreads / F;            // cells of a workgroup along x: 64 (F = 4), 7 (F = 36)
  __shared__ unsigned char col[kMThreads];
  if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) *count = 0;       // (origin_window_kernel adds onto it)
  const int t = threadIdx.x;
  const int cx0 = blockIdx.x * CPB;
  const int x = cx0 * F + t;
  const bool live = t < CPB * F && x < W;
  for (int r = 0; r < ROWS; ++r) {
    const int cy = blockIdx.y * ROWS + r;
    if (cy >= grid_h) break;                    // (uniform over the workgroup)
    bool blank = false;
    if (live) {
      const T* p = img + ((size_t)cy * F * W + x) * C;
      const size_t row = (size_t)W * C;
#pragma unroll 4
      for (int dy = 0; dy < F; ++dy) blank |= blank_sample<T>(p[dy * row]);
    }
    col[t] = blank ? 1 : 0;
    __syncthreads();
    if (t < CPB && cx0 + t < grid_w) {
      unsigned char any = 0;
      for (int dx = 0; dx < F; ++dx) any |= col[t * F + dx];
      cells[(size_t)cy * grid_w + cx0 + t] = any;
    }
    __syncthreads();
  }
}

// the blank map of an earlier call (any non-zero byte: blank) -> cells
__global__ __launch_bounds__(kMThreads) void cells_from_map_kernel(const unsigned char* __restrict__ map, size_t n,
                                                                   unsigned char* __restrict__ cells, int* __restrict__ count) {
  if (blockIdx.x == 0 && threadIdx.x == 0) *count = 0;
  for (size_t i = (size_t)blockIdx.x * kMThreads + threadIdx.x; i < n; i += (size_t)gridDim.x * kMThreads) cells[i] = map[i] ? 1 : 0;
}

// one workgroup per hold-out origin (vy, vx): cells [vy - margin, vy + 16 + margin) x [vx - margin, vx + 16 + margin), clipped
__global__ __launch_bounds__(kMThreads) void holdout_cells_kernel(const int* __restrict__ origins, int margin, int grid_h, int grid_w,
                                                                  unsigned char* __restrict__ cells) {
  const long long vy = origins[2 * (size_t)blockIdx.x], vx = origins[2 * (size_t)blockIdx.x + 1];
  const long long y0 = max(vy - margin, 0LL), y1 = min(vy + kMCrop + margin, (long long)grid_h);
  const long long x0 = max(vx - margin, 0LL), x1 = min(vx + kMCrop + margin, (long long)grid_w);
  if (y1 <= y0 || x1 <= x0) return;
  const long long w = x1 - x0, area = w * (y1 - y0);
  for (long long i = threadIdx.x; i < area; i += kMThreads) {
    const long long dy = i / w, dx = i - dy * w;
    cells[(size_t)(y0 + dy) * grid_w + (size_t)(x0 + dx)] = 1;
  }
}

// grid (ceil(origins_w / 64), ceil(origins_h / 16)); origins_h = grid_h - 15, origins_w = grid_w - 15, row_bytes = ceil(origins_w / 8)
__global__ __launch_bounds__(kMThreads) void origin_window_kernel(const unsigned char* __restrict__ cells, int grid_h, int grid_w,
                                                                  int row_bytes, unsigned char* __restrict__ bitmap,
                                                                  int* __restrict__ count) {
  __shared__ unsigned char c[kMCellsY][kMCellsX + 1];
  __shared__ unsigned char h[kMCellsY][kMTileX];
  __shared__ int wave_count[kMThreads / 64];
  const int t = threadIdx.x;
  const int ox0 = blockIdx.x * kMTileX, oy0 = blockIdx.y * kMTileY;
  const int origins_h = grid_h - (kMCrop - 1), origins_w = grid_w - (kMCrop - 1);
  for (int i = t; i < kMCellsY * kMCellsX; i += kMThreads) {
    const int ry = i / kMCellsX, rx = i - ry * kMCellsX;
    const int y = oy0 + ry, x = ox0 + rx;
    // outside the grid: only origins that are not part of the bitmap reach there
    c[ry][rx] = (y < grid_h && x < grid_w) ? cells[(size_t)y * grid_w + x] : 0;
  }
  __syncthreads();
  for (int i = t; i < kMCellsY * kMTileX; i += kMThreads) {
    const int ry = i / kMTileX, rx = i - ry * kMTileX;
    unsigned char any = 0;
#pragma unroll
    for (int k = 0; k < kMCrop; ++k) any |= c[ry][rx + k];
    h[ry][rx] = any;
  }
  __syncthreads();
  const int lane = t & 63, wave = t >> 6;
  int mine = 0;
  for (int ry = wave; ry < kMTileY; ry += kMThreads / 64) {        // (uniform over the wave)
    const int oy = oy0 + ry, ox = ox0 + lane;
    unsigned char any = 0;
#pragma unroll
    for (int k = 0; k < kMCrop; ++k) any |= h[ry + k][lane];
    const bool valid = oy < origins_h && ox < origins_w && any == 0;
    const unsigned long long bits = __ballot(valid);
    if (oy < origins_h) {
      const int byte = (ox0 >> 3) + lane;
      if (lane < 8 && byte < row_bytes) bitmap[(size_t)oy * row_bytes + byte] = (unsigned char)(bits >> (8 * lane));
      mine += __popcll(bits);
    }
  }
  if (lane == 0) wave_count[wave] = mine;
  __syncthreads();
  if (t == 0) {
    int total = 0;
    for (int w = 0; w < kMThreads / 64; ++w) total += wave_count[w];
    if (total) atomicAdd(count, total);
  }
}

template <typename T>
void launch_blank_cells(const void* img, int F, int W, int C, int grid_h, int grid_w, unsigned char* cells, int* count, hipStream_t st) {
  if (F == 4) {
    constexpr int ROWS = 4;
    const dim3 grid((grid_w + 63) / 64, (grid_h + ROWS - 1) / ROWS);
    hipLaunchKernelGGL((blank_cells_kernel<T, 4, ROWS>), grid, dim3(kMThreads), 0, st, static_cast<const T*>(img), W, C, grid_h, grid_w,
                       cells, count);
  } else {
    const dim3 grid((grid_w + 6) / 7, grid_h);
    hipLaunchKernelGGL((blank_cells_kernel<T, 36, 1>), grid, dim3(kMThreads), 0, st, static_cast<const T*>(img), W, C, grid_h, grid_w,
                       cells, count);
  }
}

}  // namespace
}  // namespace dsen2

using namespace dsen2;

extern "C" int dsen2_corpus_origin_mask(const void* dev_src, int dtype, int H, int W, int C, int grid_h, int grid_w,
                                        const int* host_holdout, const int* dev_holdout, int m, int margin, unsigned char* dev_cells,
                                        unsigned char* dev_bitmap, int* dev_count, void* stream) {
  return guarded([&]() -> int {
    if (!dev_src || !dev_cells || !dev_bitmap || !dev_count) return fail(DSEN2_ERR_INVALID, "corpus_origin_mask: NULL argument");
    if (dtype != DSEN2_DTYPE_U16 && dtype != DSEN2_DTYPE_F32 && dtype != DSEN2_MASK_BLANK_MAP)
      return fail(DSEN2_ERR_INVALID, "corpus_origin_mask: dtype %d is not supported (uint16 or float32 raster, or DSEN2_MASK_BLANK_MAP)", dtype);
    if (grid_h < kMCrop || grid_w < kMCrop || grid_h > kMMaxGrid || grid_w > kMMaxGrid)
      return fail(DSEN2_ERR_INVALID, "corpus_origin_mask: an origin grid of %d x %d has no room for a %d x %d patch (or is beyond %d)",
                  grid_h, grid_w, kMCrop, kMCrop, kMMaxGrid);
    if (C < 1) return fail(DSEN2_ERR_INVALID, "corpus_origin_mask: %d bands", C);
    const int F = H / grid_h;
    if (H <= 0 || W <= 0 || H % grid_h != 0 || W % grid_w != 0 || W / grid_w != F)
      return fail(DSEN2_ERR_INVALID, "corpus_origin_mask: a raster of %d x %d is not F x the %d x %d origin grid", H, W, grid_h, grid_w);
    if (F != 4 && F != 36)
      return fail(DSEN2_ERR_INVALID, "corpus_origin_mask: footprint F = %d: a cell covers 4 x 4 samples (20 m) or 36 x 36 (60 m)", F);
    if (m < 0 || m > kMMaxHoldout) return fail(DSEN2_ERR_INVALID, "corpus_origin_mask: %d hold-out origins (0..%d)", m, kMMaxHoldout);
    if (margin < 0 || margin > kMMaxMargin) return fail(DSEN2_ERR_INVALID, "corpus_origin_mask: margin %d (0..%d)", margin, kMMaxMargin);
    if (m > 0) {
      if (!host_holdout || !dev_holdout)
        return fail(DSEN2_ERR_INVALID, "corpus_origin_mask: host_holdout and dev_holdout are both required (the host copy is checked, the device copy is read)");
      for (int k = 0; k < m; ++k) {
        const int vy = host_holdout[2 * k], vx = host_holdout[2 * k + 1];
        if (vy < 0 || vx < 0 || vy > grid_h - kMCrop || vx > grid_w - kMCrop)
          return fail(DSEN2_ERR_INVALID, "corpus_origin_mask: hold-out origin %d: (%d, %d) + %d reaches outside the %d x %d grid", k, vy, vx,
                      kMCrop, grid_h, grid_w);
      }
    }
    hipStream_t st = (hipStream_t)stream;
    if (dtype == DSEN2_MASK_BLANK_MAP) {
      const size_t n = (size_t)grid_h * grid_w;
      const size_t want = (n + kMThreads - 1) / kMThreads;
      hipLaunchKernelGGL(cells_from_map_kernel, dim3((unsigned)(want > 4096 ? 4096 : want)), dim3(kMThreads), 0, st,
                         static_cast<const unsigned char*>(dev_src), n, dev_cells, dev_count);
    } else if (dtype == DSEN2_DTYPE_U16) {
      launch_blank_cells<unsigned short>(dev_src, F, W, C, grid_h, grid_w, dev_cells, dev_count, st);
    } else {
      launch_blank_cells<float>(dev_src, F, W, C, grid_h, grid_w, dev_cells, dev_count, st);
    }
    HIP_TRY(hipGetLastError());
    if (m > 0) {
      hipLaunchKernelGGL(holdout_cells_kernel, dim3((unsigned)m), dim3(kMThreads), 0, st, dev_holdout, margin, grid_h, grid_w, dev_cells);
      HIP_TRY(hipGetLastError());
    }
    const int origins_h = grid_h - (kMCrop - 1), origins_w = grid_w - (kMCrop - 1);
    const dim3 grid((origins_w + kMTileX - 1) / kMTileX, (origins_h + kMTileY - 1) / kMTileY);
    hipLaunchKernelGGL(origin_window_kernel, grid, dim3(kMThreads), 0, st, dev_cells, grid_h, grid_w, (origins_w + 7) / 8, dev_bitmap,
                       dev_count);
    HIP_TRY(hipGetLastError());
    return DSEN2_OK;
  });
}
