// valid_mask.hip — a validity bitmap from a CLASS raster the caller brings (Sentinel-2's SCL layer, a cloud-probability layer,
// any uint8 class image at 10, 20 or 60 m), and what carries it into a raster and into a cell map (include/dsen2_hip.h, "class
// masks").  The bitmap is dsen2_tile_nodata's: uint32 [H][ceil(W/32)], bit x & 31 of word x >> 5, set = valid, bits at x >= W 0.
// Integer work only (table look-ups, compares, wave ballots, shifts, ORs; no float arithmetic, no atomics): every result is a
// function of the inputs alone.
//
// dsen2_class_valid_bits — RAW invalid: the class of the source pixel (or of any pixel of the down x down source block) of a target
// pixel has a non-zero table entry.  The 256-entry table travels in the launch itself as 256 BITS (8 words by value); every
// workgroup copies them to LDS once and a look-up is one LDS word and a shift.
//   dilate == 0   class_bits_kernel: a workgroup takes 256 consecutive pixels of one row (grid y), lanes along x (coalesced byte
//                 reads), a wave's ballot is two words of the bitmap.  No halo, no LDS beyond the table.
//   dilate  > 0   class_bits_dilate_kernel: a workgroup owns kTileRows rows x kTileWords words.
//                   1. RAW words of the tile plus halo (dilate rows above and below, ONE word left and right: dilate <= 32) into
//                      LDS, by the same ballots; what lies outside the image is valid (0).
//                   2. horizontal: per LDS row and tile word, the 64-bit pairs (cur:prev) and (next:cur) are OR-ed with their own
//                      shifts by doubling (0..d in ceil(log2(d + 1)) steps), upwards in the first, downwards in the second.
//                   3. vertical: OR over 2 * dilate + 1 LDS rows, one word per lane; NOT, padding mask, AND input, one store.
// dsen2_raster_apply_valid — one thread per SAMPLE of the HWC raster: a store of 0 where the pixel's bit is 0, nothing else.
// dsen2_cells_from_valid_bits — one thread per cell: 1 when any bit of its S x S footprint is 0.
#include <cstdint>

#include "capi_internal.h"

namespace dsen2 {

namespace {

constexpr int kVThreads = 256;
constexpr int kTileRows = 64;
constexpr int kTileWords = 8;                       // 256 pixels
constexpr int kHaloWords = kTileWords + 2;          // one word either side: dilate <= 32
constexpr int kMaxDilate = 32;
constexpr int kLdsRows = kTileRows + 2 * kMaxDilate;
constexpr int kMaxExtent = 1 << 15;
constexpr int kMaxRatio = 8;

struct ClassTable {
  unsigned w[8];                                    // bit c of the 256: class c is invalid
};

inline unsigned vm_grid_for(size_t work_groups) {
  const size_t cap = 256 * 16;   // 256 CUs x 16 blocks, grid-stride the rest
  return (unsigned)(work_groups < cap ? (work_groups ? work_groups : 1) : cap);
}

__device__ __forceinline__ void table_to_lds(const ClassTable& t, unsigned* lds) {
#pragma unroll
  for (int i = 0; i < 8; ++i)
    if (threadIdx.x == i) lds[i] = t.w[i];
  __syncthreads();
}

// v / up for 0 <= v < 2^16 without a division: a shift for a power of two, else the high word of v * ceil(2^32 / up), which is
// exact there (the reciprocal is too large by less than up / 2^32, and v * up stays far below 2^32).  A per-pixel integer
// division is a few dozen instructions, and these kernels have little else to do.
struct SmallDiv {
  unsigned magic;                                   // 0: up is the power of two 1 << shift
  int shift;
};

inline SmallDiv small_div(int up) {
  SmallDiv d{0u, 0};
  if ((up & (up - 1)) == 0) {
    while ((1 << d.shift) < up) ++d.shift;
  } else {
    d.magic = (unsigned)(((1ull << 32) + (unsigned)up - 1) / (unsigned)up);
  }
  return d;
}

__device__ __forceinline__ int div_up(int v, SmallDiv d) { return d.magic ? (int)__umulhi((unsigned)v, d.magic) : v >> d.shift; }

// RAW invalid of target pixel (y, x), 0 <= y < H and 0 <= x < W (the caller's test).  up: source (y / up, x / up), which the
// coverage rule (H - 1) / up < Hs keeps inside; down: the block [y * down, y * down + down) x [x * down, ...), inside by
// H * down <= Hs.
__device__ __forceinline__ bool raw_invalid(const unsigned char* __restrict__ cls, int Ws, SmallDiv up, int down, int y, int x,
                                            const unsigned* table) {
  if (down == 1) {
    const unsigned c = cls[(size_t)div_up(y, up) * Ws + div_up(x, up)];
    return (table[c >> 5] >> (c & 31)) & 1u;
  }
  unsigned any = 0;
  const unsigned char* p = cls + (size_t)(y * down) * Ws + (size_t)x * down;
  for (int dy = 0; dy < down; ++dy, p += Ws)
    for (int dx = 0; dx < down; ++dx) {
      const unsigned c = p[dx];
      any |= table[c >> 5] >> (c & 31);
    }
  return any & 1u;
}

// grid (ceil(W / 256), some rows): a workgroup keeps its 256 columns and strides over the rows, so the table reaches LDS once per
// workgroup and everything about a row is scalar work
__global__ __launch_bounds__(kVThreads) void class_bits_kernel(const unsigned char* __restrict__ cls, int Ws, ClassTable table,
                                                               SmallDiv up, int down, int H, int W, int words_per_row,
                                                               const unsigned* and_bits, unsigned* bits) {
  __shared__ unsigned s_table[8];
  table_to_lds(table, s_table);
  const int lane = threadIdx.x & 63;
  const int x = blockIdx.x * kVThreads + (int)threadIdx.x;
  const int word = x >> 5;                                             // lanes 0 and 32: x is a multiple of 32
  for (int y = blockIdx.y; y < H; y += gridDim.y) {                    // (uniform over the workgroup: every lane reaches the ballot)
    bool valid = false;
    if (x < W) valid = !raw_invalid(cls, Ws, up, down, y, x, s_table);
    const unsigned long long b = __ballot(valid);
    if ((lane & 31) == 0 && word < words_per_row) {
      const size_t at = (size_t)y * words_per_row + word;
      unsigned v = (unsigned)(b >> lane);
      if (and_bits) v &= and_bits[at];
      bits[at] = v;
    }
  }
}

// OR of (v << s), s = 0..d, by doubling: after a step the accumulator holds the shifts 0..k
__device__ __forceinline__ unsigned long long smear_up(unsigned long long v, int d) {
  for (int k = 0; k < d;) {
    const int step = (k + 1 < d - k) ? k + 1 : d - k;
    v |= v << step;
    k += step;
  }
  return v;
}

__device__ __forceinline__ unsigned long long smear_down(unsigned long long v, int d) {
  for (int k = 0; k < d;) {
    const int step = (k + 1 < d - k) ? k + 1 : d - k;
    v |= v >> step;
    k += step;
  }
  return v;
}

// grid (ceil(words_per_row / kTileWords), ceil(H / kTileRows)); 1 <= dilate <= kMaxDilate
__global__ __launch_bounds__(kVThreads) void class_bits_dilate_kernel(const unsigned char* __restrict__ cls, int Ws, ClassTable table,
                                                                      SmallDiv up, int down, int H, int W, int words_per_row, int dilate,
                                                                      const unsigned* and_bits, unsigned* bits) {
  __shared__ unsigned s_table[8];
  __shared__ unsigned s_raw[kLdsRows][kHaloWords];          // RAW invalid, rows y0 - dilate .., words w0 - 1 ..
  __shared__ unsigned s_hor[kLdsRows][kTileWords];          // dilated along x
  table_to_lds(table, s_table);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int w0 = blockIdx.x * kTileWords, y0 = blockIdx.y * kTileRows;
  const int rows = kTileRows + 2 * dilate;                  // <= kLdsRows
  constexpr int kSegs = kHaloWords / 2;                     // 64-pixel pieces of a halo row
  // 1. RAW words: a wave per 64 pixels (uniform over the wave: every lane reaches the ballot)
  for (int i = wave; i < rows * kSegs; i += kVThreads / 64) {
    const int r = i / kSegs, seg = i - r * kSegs;
    const int y = y0 - dilate + r;
    const int x = (w0 - 1) * 32 + seg * 64 + lane;
    bool inv = false;
    if (y >= 0 && y < H && x >= 0 && x < W) inv = raw_invalid(cls, Ws, up, down, y, x, s_table);
    const unsigned long long b = __ballot(inv);
    if ((lane & 31) == 0) s_raw[r][seg * 2 + (lane >> 5)] = (unsigned)(b >> lane);
  }
  __syncthreads();
  // 2. along x
  for (int i = threadIdx.x; i < rows * kTileWords; i += kVThreads) {
    const int r = i / kTileWords, j = i - r * kTileWords;
    const unsigned long long prev = s_raw[r][j], cur = s_raw[r][j + 1], next = s_raw[r][j + 2];
    const unsigned from_left = (unsigned)(smear_up((cur << 32) | prev, dilate) >> 32);      // pixel x - s reaches x
    const unsigned from_right = (unsigned)smear_down((next << 32) | cur, dilate);           // pixel x + s reaches x
    s_hor[r][j] = from_left | from_right;
  }
  __syncthreads();
  // 3. along y, and out
  for (int i = threadIdx.x; i < kTileRows * kTileWords; i += kVThreads) {
    const int r = i / kTileWords, j = i - r * kTileWords;
    const int y = y0 + r, word = w0 + j;
    if (y >= H || word >= words_per_row) continue;
    unsigned inv = 0;
    for (int k = 0; k <= 2 * dilate; ++k) inv |= s_hor[r + k][j];
    unsigned v = ~inv;
    const int left = W - word * 32;                          // pixels of this word inside the image: >= 1
    if (left < 32) v &= ~0u >> (32 - left);
    const size_t at = (size_t)y * words_per_row + word;
    if (and_bits) v &= and_bits[at];
    bits[at] = v;
  }
}

template <typename T>
__global__ __launch_bounds__(kVThreads) void apply_valid_kernel(T* __restrict__ img, int W, int C, int words_per_row, size_t samples,
                                                                const unsigned* __restrict__ bits) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < samples; i += (size_t)gridDim.x * blockDim.x) {
    const size_t pix = i / C;
    const size_t y = pix / W;
    const int x = (int)(pix - y * W);
    if (!((bits[y * words_per_row + (x >> 5)] >> (x & 31)) & 1u)) img[i] = T(0);
  }
}

__global__ __launch_bounds__(kVThreads) void cells_kernel(const unsigned* __restrict__ bits, int words_per_row, int S, int cells_w,
                                                          size_t cells, int accumulate, unsigned char* __restrict__ out) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < cells; i += (size_t)gridDim.x * blockDim.x) {
    if (accumulate && out[i] != 0) continue;                 // the OR into a map that holds non-zero already
    const size_t cy = i / cells_w;
    const int cx = (int)(i - cy * cells_w);
    unsigned all = 1u;
    for (int dy = 0; dy < S; ++dy) {
      const unsigned* row = bits + (cy * S + dy) * words_per_row;
      for (int dx = 0; dx < S; ++dx) {
        const int x = cx * S + dx;
        all &= row[x >> 5] >> (x & 31);
      }
    }
    out[i] = (all & 1u) ? 0 : 1;
  }
}

int extent_ok(const char* who, int H, int W) {
  if (H < 1 || W < 1 || H > kMaxExtent || W > kMaxExtent)
    return fail(DSEN2_ERR_INVALID, "%s: H=%d W=%d outside 1..%d", who, H, W, kMaxExtent);
  return DSEN2_OK;
}

}  // namespace
}  // namespace dsen2

using namespace dsen2;

extern "C" int dsen2_class_valid_bits(const unsigned char* dev_cls, int Hs, int Ws, const unsigned char* host_lut256, int up, int down,
                                      int H, int W, int dilate, const unsigned int* dev_and_bits_or_null, unsigned int* dev_valid_bits,
                                      void* stream) {
  return guarded([&]() -> int {
    if (!dev_cls || !host_lut256 || !dev_valid_bits) return fail(DSEN2_ERR_INVALID, "class_valid_bits: NULL argument");
    if (int rc = extent_ok("class_valid_bits", H, W)) return rc;
    if (up < 1 || down < 1 || up > kMaxRatio || down > kMaxRatio || (up > 1 && down > 1))
      return fail(DSEN2_ERR_INVALID, "class_valid_bits: up=%d down=%d (1..%d, at most one of them above 1)", up, down, kMaxRatio);
    if (dilate < 0 || dilate > kMaxDilate) return fail(DSEN2_ERR_INVALID, "class_valid_bits: dilate=%d outside 0..%d", dilate, kMaxDilate);
    if (Hs < 1 || Ws < 1) return fail(DSEN2_ERR_INVALID, "class_valid_bits: source of %d x %d", Hs, Ws);
    const bool covered = down > 1 ? ((long long)H * down <= Hs && (long long)W * down <= Ws) : ((H - 1) / up < Hs && (W - 1) / up < Ws);
    if (!covered)
      return fail(DSEN2_ERR_INVALID, "class_valid_bits: a source of %d x %d does not cover a target of %d x %d with up=%d down=%d", Hs,
                  Ws, H, W, up, down);
    ClassTable table;
    for (int i = 0; i < 8; ++i) table.w[i] = 0;
    for (int c = 0; c < 256; ++c)
      if (host_lut256[c]) table.w[c >> 5] |= 1u << (c & 31);
    const int wpr = (W + 31) / 32;
    hipStream_t st = (hipStream_t)stream;
    const SmallDiv by_up = small_div(up);
    if (dilate == 0) {
      const int chunks = (W + kVThreads - 1) / kVThreads;                                  // <= 128
      const int row_groups = (256 * 16 + chunks - 1) / chunks;                             // 256 CUs x 16 blocks, stride the rest
      const dim3 grid((unsigned)chunks, (unsigned)(H < row_groups ? H : row_groups));
      hipLaunchKernelGGL(class_bits_kernel, grid, dim3(kVThreads), 0, st, dev_cls, Ws, table, by_up, down, H, W, wpr,
                         dev_and_bits_or_null, dev_valid_bits);
    } else {
      const dim3 grid((unsigned)((wpr + kTileWords - 1) / kTileWords), (unsigned)((H + kTileRows - 1) / kTileRows));
      hipLaunchKernelGGL(class_bits_dilate_kernel, grid, dim3(kVThreads), 0, st, dev_cls, Ws, table, by_up, down, H, W, wpr, dilate,
                         dev_and_bits_or_null, dev_valid_bits);
    }
    HIP_TRY(hipGetLastError());
    return DSEN2_OK;
  });
}

extern "C" int dsen2_raster_apply_valid(void* dev_img, int dtype, int H, int W, int C, const unsigned int* dev_valid_bits, void* stream) {
  return guarded([&]() -> int {
    if (!dev_img || !dev_valid_bits) return fail(DSEN2_ERR_INVALID, "raster_apply_valid: NULL argument");
    if (dtype != DSEN2_DTYPE_U16 && dtype != DSEN2_DTYPE_F32) return fail(DSEN2_ERR_INVALID, "raster_apply_valid: dtype %d", dtype);
    if (int rc = extent_ok("raster_apply_valid", H, W)) return rc;
    if (C < 1 || C > 4096) return fail(DSEN2_ERR_INVALID, "raster_apply_valid: C=%d", C);
    const int wpr = (W + 31) / 32;
    const size_t samples = (size_t)H * W * C;
    const dim3 grid(vm_grid_for((samples + kVThreads - 1) / kVThreads)), block(kVThreads);
    hipStream_t st = (hipStream_t)stream;
    if (dtype == DSEN2_DTYPE_U16)
      hipLaunchKernelGGL(apply_valid_kernel<unsigned short>, grid, block, 0, st, (unsigned short*)dev_img, W, C, wpr, samples, dev_valid_bits);
    else
      hipLaunchKernelGGL(apply_valid_kernel<float>, grid, block, 0, st, (float*)dev_img, W, C, wpr, samples, dev_valid_bits);
    HIP_TRY(hipGetLastError());
    return DSEN2_OK;
  });
}

extern "C" int dsen2_cells_from_valid_bits(const unsigned int* dev_valid_bits, int H, int W, int S, int accumulate,
                                           unsigned char* dev_cells, void* stream) {
  return guarded([&]() -> int {
    if (!dev_valid_bits || !dev_cells) return fail(DSEN2_ERR_INVALID, "cells_from_valid_bits: NULL argument");
    if (int rc = extent_ok("cells_from_valid_bits", H, W)) return rc;
    if (S < 1 || S > 8 || H % S || W % S) return fail(DSEN2_ERR_INVALID, "cells_from_valid_bits: S=%d (1..8) must divide H=%d and W=%d", S, H, W);
    const int wpr = (W + 31) / 32, cells_w = W / S;
    const size_t cells = (size_t)(H / S) * cells_w;
    hipLaunchKernelGGL(cells_kernel, dim3(vm_grid_for((cells + kVThreads - 1) / kVThreads)), dim3(kVThreads), 0, (hipStream_t)stream,
                       dev_valid_bits, wpr, S, cells_w, cells, accumulate, dev_cells);
    HIP_TRY(hipGetLastError());
    return DSEN2_OK;
  });
}
