// conv3x3_items.h — what every convolution kernel file says about its ITEMS, once: which item a workgroup starts from, which
// tile an item is, and how a kernel is prepared and launched.  Included by the kernel files only (device code).
#pragma once
#include "dsen2_internal.h"

namespace dsen2 {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// XCD-contiguous logical id of workgroup `bid` in a grid of G.  The hardware deals workgroups round-robin to the 8 XCDs, so
// blocks b, b + 8, b + 16, .. share an XCD and its L2.  The logical id gives each XCD a contiguous run of ids — the first
// G % 8 XCDs one id more than the others — so that neighbouring tiles' halos and the weight stream hit in that L2.
// Bijective on [0, G) for any grid size.  A persistent workgroup walks the items lid, lid + G, ...
__device__ __forceinline__ int xcd_contiguous_id(int bid, int G) {
  const int xcd = bid & 7, q8 = G >> 3, r8 = G & 7;
  return (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (bid >> 3);
}

// item = tile * NS + slab (NS output slabs per tile, the slab fastest); tiles run image by image, row-major inside an image,
// TH x TW output pixels each.  (ty0, tx0) = the tile's first output pixel.  NS = 1: one tile per workgroup.
struct Tile { int img, ty0, tx0, slab; };
template <int NS, int TH = kTile, int TW = kTile>
__device__ __forceinline__ Tile tile_at(int item, int tiles_per_img, int tiles_x) {
  const int tile = item / NS;
  const int img = tile / tiles_per_img;
  const int trem = tile - img * tiles_per_img;
  const int tyi = trem / tiles_x;
  return Tile{img, tyi * TH, (trem - tyi * tiles_x) * TW, item - tile * NS};
}

// ---- host side: prepare, launch ----
// One KernelOnce per kernel (Kern is a template argument, so every kernel instantiation has its own function-local static):
// the dynamic-LDS limit `max_lds_bytes` is set once per (kernel, device); *cus = the device's CU count.
template <auto Kern>
hipError_t prepare_kernel(size_t max_lds_bytes, int* cus) {
  static KernelOnce once;
  return once.prepare(reinterpret_cast<const void*>(Kern), max_lds_bytes, cus);
}

template <auto Kern, typename... Args>
hipError_t launch_kernel(dim3 grid, int threads, size_t lds_bytes, hipStream_t stream, const Args&... args) {
  hipLaunchKernelGGL(Kern, grid, dim3(threads), lds_bytes, stream, args...);
  return hipGetLastError();
}

// A persistent kernel Kern(args..., int n_items): one workgroup per CU, fewer when there are fewer items or `grid_cap` (> 0)
// asks for fewer.  A workgroup that keeps ONE of `slabs` output slabs needs the item stride G to preserve item % slabs: the
// grid is a multiple of `slabs` and at least `slabs` (slabs = 1: the kernel takes the slab from each item).
// hipErrorInvalidValue: no items, or more than an int counts.
template <auto Kern, typename... Args>
hipError_t launch_persistent(size_t lds_bytes, int threads, long long items, int slabs, int grid_cap, hipStream_t stream,
                             const Args&... args) {
  int cus = 0;
  const hipError_t e = prepare_kernel<Kern>(lds_bytes, &cus);
  if (e != hipSuccess) return e;
  if (items <= 0 || items > 0x7fffffffLL) return hipErrorInvalidValue;
  int grid = (int)(items < cus ? items : cus);
  if (grid_cap > 0 && grid_cap < grid) grid = grid_cap;
  grid -= grid % slabs;
  if (grid < slabs) grid = slabs;
  return launch_kernel<Kern>(dim3(grid), threads, lds_bytes, stream, args..., (int)items);
}

}  // namespace dsen2
