// corpus_batch.hip — a whole training batch cut from a device-resident corpus of tiles in ONE launch: the random crops of
// save_random_patches / save_random_patches60 (utils/patches.py:181-271), the up-sampling of the low-resolution crops
// (interp_patches, :11-16), the `/= SCALE` of the training loader and the flip / rotation of the augmentation, for every sample
// and every tensor of the batch.  The chain it replaces is, per tile, three or four dsen2_tile_gather launches, one or two
// dsen2_upsample_mirror_bilinear launches and one dsen2_dihedral_nchw launch per tensor; its outputs are that chain's bits.
//
// Work split: one workgroup = (sample, output tensor, 32 x 32 tile of the output planes) and all the bands of that tensor — the
// sources are HWC, so a lane reads a pixel's bands as one contiguous run, as tile_gather_kernel does.  The patch edge is 32 (20 m)
// or 96 (60 m), both multiples of 32: no ragged tiles.  The tile goes through LDS exactly as dihedral.hip's does: it is FILLED
// along the source's rows (consecutive lanes = consecutive, ascending or descending, source columns for all 8 ops) and WRITTEN
// along the output's rows; a transposing op reads LDS by columns, which the row stride of 33 floats spreads over the banks.
// An up-sampled tensor first stages the window of its low-resolution crop that the tile's taps reach (at most 18 x 18 pixels;
// mirrored at the CROP's edges, since the chain up-samples each crop as an image of its own) in LDS as quotients by 30000, and
// interpolates from there with upsample_math.h's functions — the arithmetic of upsample_kernel, not a copy of it.
// No atomics; every output element has exactly one writer; a sample reads only inside its own tile's images.
#include <mutex>
#include <vector>

#include "capi_internal.h"
#include "dsen2_internal.h"
#include "upsample_math.h"

namespace dsen2 {

namespace {

constexpr int kCTile = 32;                    // tile edge
constexpr int kCStride = kCTile + 1;          // LDS row stride in floats
constexpr int kCPlane = kCTile * kCStride;    // one band's tile
constexpr int kCRows = 8;                     // rows of the tile a pass of the 256 threads covers
constexpr int kCBands = 6;                    // most bands of a tensor (the 20 m group)
constexpr int kCWin = 18;                     // most rows / columns of a low-resolution window: 32 outputs at x2 reach 18 sources
constexpr int kCrop = 16;                     // edge of a crop on the origin grid

// scale and offset of the up-sampler's coordinate map for `in` source samples per `out` outputs — launch_upsample's, to the bit
struct UpAxis {
  float s, o;
  int in;
};
inline UpAxis up_axis(int in, int out) {
  const double f = (double)in / out;
  return UpAxis{(float)f, (float)(0.5 * f - 0.5), in};
}

// where a tile of the OUTPUT sits and how its elements map back to the un-turned patch (dihedral.hip's index map, ih = iw = P)
struct TileMap {
  int i0, j0, P;
  bool tr, ry, rx;
  // LDS position (a, b), b along the source's rows -> (i, j) of the output
  __device__ __forceinline__ void out_ij(int a, int b, int* i, int* j) const {
    *i = i0 + (tr ? b : a);
    *j = j0 + (tr ? a : b);
  }
  __device__ __forceinline__ void src_yx(int i, int j, int* sy, int* sx) const {
    *sy = tr ? (ry ? P - 1 - j : j) : (ry ? P - 1 - i : i);
    *sx = tr ? (rx ? P - 1 - i : i) : (rx ? P - 1 - j : j);
  }
  // first source row / column the tile reads (it reads kCTile of each)
  __device__ __forceinline__ int sy_first() const { const int t = tr ? j0 : i0; return ry ? P - kCTile - t : t; }
  __device__ __forceinline__ int sx_first() const { const int t = tr ? i0 : j0; return rx ? P - kCTile - t : t; }
};

// a cropped tensor (data10, the target): img HWC with C bands of T, row length W pixels, the crop's corner at (y0, x0)
template <int C, typename T>
__device__ __forceinline__ void fill_cropped(const T* __restrict__ img, int W, int y0, int x0, const TileMap& m, float divisor,
                                             float* tile) {
  const int b = threadIdx.x & 31;
  for (int a = threadIdx.x >> 5; a < kCTile; a += kCRows) {
    int i, j, sy, sx;
    m.out_ij(a, b, &i, &j);
    m.src_yx(i, j, &sy, &sx);
    const T* const src = img + ((size_t)(y0 + sy) * W + (x0 + sx)) * C;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const float v = (float)src[c];                                   // (uint16 -> float32 is exact)
      tile[c * kCPlane + a * kCStride + b] = divisor == 1.0f ? v : __fdiv_rn(v, divisor);   // as tile_gather_kernel
    }
  }
}

// an up-sampled tensor (data20, data60): the crop of ax.in x ax.in pixels at (y0, x0) of img is the image the up-sampler sees
template <int C>
__device__ __forceinline__ void fill_upsampled(const float* __restrict__ img, int W, int y0, int x0, UpAxis ax, const TileMap& m,
                                               float post_div, float* tile, float* win) {
  // the window of source rows / columns the tile's taps reach (the coordinate map is monotone: first and last output decide)
  int ru0, ru1, cu0, cu1, unused;
  (void)up_coord(ax.s, ax.o, m.sy_first(), &ru0, &unused);
  (void)up_coord(ax.s, ax.o, m.sy_first() + kCTile - 1, &unused, &ru1);
  (void)up_coord(ax.s, ax.o, m.sx_first(), &cu0, &unused);
  (void)up_coord(ax.s, ax.o, m.sx_first() + kCTile - 1, &unused, &cu1);
  const int nr = min(ru1 - ru0 + 1, kCWin), nc = min(cu1 - cu0 + 1, kCWin);     // (never clipped at the scales of the launcher)
  for (int idx = threadIdx.x; idx < nr * nc; idx += 256) {
    const int wr = idx / nc, wc = idx - wr * nc;
    const int row = mirror_index_near(ru0 + wr, ax.in), col = mirror_index_near(cu0 + wc, ax.in);
    const float* const src = img + ((size_t)(y0 + row) * W + (x0 + col)) * C;
#pragma unroll
    for (int c = 0; c < C; ++c) win[c * (kCWin * kCWin) + idx] = up_quotient(src[c]);
  }
  __syncthreads();
  const int b = threadIdx.x & 31;
  for (int a = threadIdx.x >> 5; a < kCTile; a += kCRows) {
    int i, j, sy, sx, r0, r1, c0, c1;
    m.out_ij(a, b, &i, &j);
    m.src_yx(i, j, &sy, &sx);
    const float drf = up_coord(ax.s, ax.o, sy, &r0, &r1);
    const float dcf = up_coord(ax.s, ax.o, sx, &c0, &c1);
    const int t0 = (r0 - ru0) * nc, t1 = (r1 - ru0) * nc;
    c0 -= cu0; c1 -= cu0;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const float* const w = win + c * (kCWin * kCWin);
      const double top = up_hblend(dcf, w[t0 + c0], w[t0 + c1]), bot = up_hblend(dcf, w[t1 + c0], w[t1 + c1]);
      tile[c * kCPlane + a * kCStride + b] = up_vblend(drf, top, bot, post_div);
    }
  }
}

template <int C>
__device__ __forceinline__ void write_tile(const float* tile, const TileMap& m, float* __restrict__ out /* the sample's [C, P, P] */) {
  const int lj = threadIdx.x & 31;
  for (int li = threadIdx.x >> 5; li < kCTile; li += kCRows) {
    float* const o = out + (size_t)(m.i0 + li) * m.P + (m.j0 + lj);
    const int at = m.tr ? lj * kCStride + li : li * kCStride + lj;
#pragma unroll
    for (int c = 0; c < C; ++c) o[(size_t)c * m.P * m.P] = tile[c * kCPlane + at];
  }
}

// grid.x = n * tensors * (P / 32)^2.  Tensors: data10, data20, (data60,) target.
template <bool RUN60>
__global__ __launch_bounds__(256) void corpus_batch_kernel(const CorpusTileDev* __restrict__ tiles, int n_tiles,
                                                           const int* __restrict__ samples, float divisor, UpAxis up20, UpAxis up60,
                                                           float* __restrict__ x10, float* __restrict__ x20, float* __restrict__ x60,
                                                           float* __restrict__ y) {
  constexpr int P = RUN60 ? 96 : 32, TP = P / kCTile, T = TP * TP, NT = RUN60 ? 4 : 3;
  constexpr int S10 = RUN60 ? 6 : 2, S20 = RUN60 ? 3 : 1;       // image pixels per origin-grid step
  constexpr int CGT = RUN60 ? 2 : 6;
  __shared__ float tile[kCBands * kCPlane];
  __shared__ float win[kCBands * kCWin * kCWin];
  const unsigned k = blockIdx.x / (unsigned)(NT * T), rem = blockIdx.x - k * (unsigned)(NT * T);
  const int tensor = (int)(rem / T), t = (int)(rem - (unsigned)tensor * T);
  const int* const s = samples + 4 * (size_t)k;
  const int ti = s[0], oy = s[1], ox = s[2], op = s[3] & 7;
  if ((unsigned)ti >= (unsigned)n_tiles) return;                   // (uniform over the workgroup: before any barrier)
  const CorpusTileDev td = tiles[ti];
  if (oy < 0 || ox < 0 || oy > td.eh - kCrop || ox > td.ew - kCrop) return;
  const int bits = dihedral_bits(op);
  TileMap m;
  m.i0 = (t / TP) * kCTile; m.j0 = (t % TP) * kCTile; m.P = P;
  m.tr = bits & 4; m.ry = bits & 2; m.rx = bits & 1;
  const size_t pp = (size_t)P * P;
  if (tensor == 0) {
    fill_cropped<4, float>(td.lr10, S10 * td.ew, S10 * oy, S10 * ox, m, divisor, tile);
    __syncthreads();
    write_tile<4>(tile, m, x10 + k * 4 * pp);
  } else if (tensor == 1) {
    fill_upsampled<6>(td.lr20, S20 * td.ew, S20 * oy, S20 * ox, up20, m, divisor, tile, win);
    __syncthreads();
    write_tile<6>(tile, m, x20 + k * 6 * pp);
  } else if (RUN60 && tensor == 2) {
    fill_upsampled<2>(td.lr60, td.ew, oy, ox, up60, m, divisor, tile, win);
    __syncthreads();
    write_tile<2>(tile, m, x60 + k * 2 * pp);
  } else {
    if (td.gt_u16)
      fill_cropped<CGT, unsigned short>(static_cast<const unsigned short*>(td.gt), S10 * td.ew, S10 * oy, S10 * ox, m, divisor, tile);
    else
      fill_cropped<CGT, float>(static_cast<const float*>(td.gt), S10 * td.ew, S10 * oy, S10 * ox, m, divisor, tile);
    __syncthreads();
    write_tile<CGT>(tile, m, y + k * CGT * pp);
  }
}

}  // namespace

hipError_t launch_corpus_batch(const CorpusTileDev* dev_tiles, int n_tiles, bool run_60, const int* dev_samples, int n, float divisor,
                               float* x10, float* x20, float* x60, float* y, hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  const dim3 block(256);
  if (run_60) {
    const dim3 grid((unsigned)n * 4u * 9u);
    hipLaunchKernelGGL(corpus_batch_kernel<true>, grid, block, 0, stream, dev_tiles, n_tiles, dev_samples, divisor, up_axis(48, 96),
                       up_axis(16, 96), x10, x20, x60, y);
  } else {
    const dim3 grid((unsigned)n * 3u);
    hipLaunchKernelGGL(corpus_batch_kernel<false>, grid, block, 0, stream, dev_tiles, n_tiles, dev_samples, divisor, up_axis(16, 32),
                       up_axis(16, 32), x10, x20, x60, y);
  }
  return hipGetLastError();
}

}  // namespace dsen2

// ---- C ABI (include/dsen2_hip.h, "corpus") --------------------------------------------------------------------------------------
struct dsen2_corpus {
  std::vector<dsen2_corpus_tile> tiles;     // the checked table (host copy)
  int run_60 = 0;
  std::mutex mu;                            // guards the two fields below
  dsen2::CorpusTileDev* dev_tiles = nullptr;   // uploaded by the first batch that launches
  int device = -1;                          // the device that copy lives on
};

namespace dsen2 {
namespace {

constexpr int kMaxBatch = 1 << 20;          // samples per call (the grid stays far below 2^31 workgroups)
constexpr int kMaxExtent = 1 << 20;         // origin-grid extent per axis (6 x it still indexes with an int)

// the device copy of the table, made on first use on the calling thread's current device
int corpus_device_table(dsen2_corpus* c, const CorpusTileDev** out) {
  std::lock_guard<std::mutex> lock(c->mu);
  int dev = -1;
  if (hipGetDevice(&dev) != hipSuccess) return fail(DSEN2_ERR_NO_DEVICE, "no HIP device");
  if (!c->dev_tiles) {
    std::vector<CorpusTileDev> host(c->tiles.size());
    for (size_t i = 0; i < host.size(); ++i) {
      const dsen2_corpus_tile& t = c->tiles[i];
      host[i] = CorpusTileDev{t.dev_lr10, t.dev_lr20, t.dev_lr60, t.dev_gt, t.grid_h, t.grid_w, t.gt_dtype == DSEN2_DTYPE_U16 ? 1 : 0, 0};
    }
    CorpusTileDev* p = nullptr;
    HIP_TRY(hipMalloc((void**)&p, host.size() * sizeof(CorpusTileDev)));
    const hipError_t e = hipMemcpy(p, host.data(), host.size() * sizeof(CorpusTileDev), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
      (void)hipFree(p);
      return fail(DSEN2_ERR_HIP, "uploading the tile table: %s", hipGetErrorString(e));
    }
    c->dev_tiles = p;
    c->device = dev;
  } else if (dev != c->device) {
    return fail(DSEN2_ERR_INVALID, "corpus handle belongs to device %d but the calling thread's current device is %d", c->device, dev);
  }
  *out = c->dev_tiles;
  return DSEN2_OK;
}

}  // namespace
}  // namespace dsen2

using namespace dsen2;

extern "C" {

int dsen2_corpus_create(const dsen2_corpus_tile* host_tiles, int n_tiles, int run_60, dsen2_corpus** out) {
  return guarded([&]() -> int {
    if (!out) return fail(DSEN2_ERR_INVALID, "NULL argument");
    *out = nullptr;
    if (!host_tiles) return fail(DSEN2_ERR_INVALID, "NULL argument");
    if (n_tiles < 1) return fail(DSEN2_ERR_INVALID, "a corpus needs at least one tile, got %d", n_tiles);
    for (int i = 0; i < n_tiles; ++i) {
      const dsen2_corpus_tile& t = host_tiles[i];
      if (!t.dev_lr10 || !t.dev_lr20 || !t.dev_gt) return fail(DSEN2_ERR_INVALID, "tile %d: NULL image", i);
      if ((t.dev_lr60 != nullptr) != (run_60 != 0))
        return fail(DSEN2_ERR_INVALID, "tile %d: the 60 m image must be given with run_60 and only then", i);
      if (t.grid_h < kCrop || t.grid_w < kCrop || t.grid_h > kMaxExtent || t.grid_w > kMaxExtent)
        return fail(DSEN2_ERR_INVALID, "tile %d: an origin grid of %d x %d has no room for a %d x %d patch (or is beyond %d)", i, t.grid_h,
                    t.grid_w, kCrop, kCrop, kMaxExtent);
      if (t.gt_dtype != DSEN2_DTYPE_U16 && t.gt_dtype != DSEN2_DTYPE_F32)
        return fail(DSEN2_ERR_INVALID, "tile %d: the target must be uint16 or float32 (dtype %d)", i, t.gt_dtype);
    }
    dsen2_corpus* c = new dsen2_corpus;
    c->tiles.assign(host_tiles, host_tiles + n_tiles);
    c->run_60 = run_60 != 0;
    *out = c;
    return DSEN2_OK;
  });
}

void dsen2_corpus_destroy(dsen2_corpus* c) {
  if (!c) return;
  if (c->dev_tiles) (void)hipFree(c->dev_tiles);
  delete c;
}

int dsen2_corpus_batch(const dsen2_corpus* corpus, const int* host_samples, const int* dev_samples, int n, float divisor, float* dev_x10,
                       float* dev_x20, float* dev_x60_or_null, float* dev_y, void* stream) {
  return guarded([&]() -> int {
    if (!corpus || !dev_x10 || !dev_x20 || !dev_y) return fail(DSEN2_ERR_INVALID, "NULL argument");
    if ((dev_x60_or_null != nullptr) != (corpus->run_60 != 0))
      return fail(DSEN2_ERR_INVALID, corpus->run_60 ? "a run_60 corpus needs dev_x60" : "dev_x60 given, but the corpus is not a run_60 one");
    if (n < 0 || n > kMaxBatch) return fail(DSEN2_ERR_INVALID, "batch of %d samples (0..%d)", n, kMaxBatch);
    if (!(divisor != 0.f) || !(divisor - divisor == 0.f)) return fail(DSEN2_ERR_INVALID, "divisor must be finite and not 0");
    if (n == 0) return DSEN2_OK;
    if (!host_samples || !dev_samples)
      return fail(DSEN2_ERR_INVALID, "host_samples and dev_samples are both required (the host copy is checked, the device copy is read)");
    const int n_tiles = (int)corpus->tiles.size();
    for (int k = 0; k < n; ++k) {
      const int ti = host_samples[4 * k], oy = host_samples[4 * k + 1], ox = host_samples[4 * k + 2], op = host_samples[4 * k + 3];
      if (ti < 0 || ti >= n_tiles) return fail(DSEN2_ERR_INVALID, "sample %d: tile %d outside the table of %d", k, ti, n_tiles);
      const dsen2_corpus_tile& t = corpus->tiles[ti];
      if (oy < 0 || ox < 0 || oy > t.grid_h - kCrop || ox > t.grid_w - kCrop)
        return fail(DSEN2_ERR_INVALID, "sample %d: origin (%d, %d) + %d reaches outside the %d x %d grid of tile %d", k, oy, ox, kCrop,
                    t.grid_h, t.grid_w, ti);
      if (op < 0 || op > 7) return fail(DSEN2_ERR_INVALID, "sample %d: op %d outside 0..7", k, op);
    }
    const CorpusTileDev* table = nullptr;
    if (int rc = corpus_device_table(const_cast<dsen2_corpus*>(corpus), &table)) return rc;
    HIP_TRY(launch_corpus_batch(table, n_tiles, corpus->run_60 != 0, dev_samples, n, divisor, dev_x10, dev_x20, dev_x60_or_null, dev_y,
                                (hipStream_t)stream));
    return DSEN2_OK;
  });
}

}  // extern "C"
