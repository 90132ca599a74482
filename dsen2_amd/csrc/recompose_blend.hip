// recompose_blend.hip — recomposition with a feathered blend in the overlap of neighbouring patches (include/dsen2_hip.h,
// "feathered recomposition").  dsen2_recompose_rows keeps, for every pixel, the LAST patch that covers it; here every patch
// that lies within `feather` pixels of its inner square adds its value with an integer ramp weight, and the pixel is the
// weighted mean.  Gather form, as recompose_kernel (patch_ops.hip): one thread per output PIXEL, no atomics, no write race, so
// the image is a function of the inputs alone.
//
// Along an axis of length L (inner = P - 2 * border, T = ceil(L / inner)) tile t starts at s_t = t * inner, the last one at
// L - inner; its patch covers [s_t - border, s_t - border + P) and, with u = x - (s_t - border), carries the weight
//     w(u) = clamp(min(u + 1, P - u) - (border - feather), 0, 2 * feather)
// — 0 outside [s_t - feather, s_t + inner + feather), a ramp 1 .. 2 * feather across each edge of the inner square, 2 * feather
// inside.  A patch's weight at a pixel is wy * wx.  With 2 * feather <= inner (border <= P / 4) at most two regular tiles and
// the clamped last one carry weight on an axis: the candidates below, in ascending order.
//
//     out = float32( sum_k w_k * p_k / sum_k w_k ) * scale        sums in float64, in ascending (ty, tx) order
//
// Every product w_k * p_k is exact (w_k <= 4 * feather^2 < 2^14, p_k has 24 significant bits), so where ONE patch carries
// weight the quotient is p_k itself: those pixels — 73 % of the image at P = 128, border = feather = 8 — take the first branch,
// which is recompose_kernel's body, and only the overlap bands run float64 arithmetic (2 to 9 patches, neighbouring threads
// reading neighbouring x of the same patch rows).  10980^2 x 6: 2.3 ms at (8, 8) against recompose_kernel's 1.3 ms, 0.45 of the
// HBM copy rate against 0.71 (profiles/seam_blend.md: the float64 fold and division, and waves that hold both kinds of pixels).
#include <cstdint>

#include "capi_internal.h"

namespace dsen2 {

namespace {

constexpr int kBThreads = 256;

inline unsigned blend_grid_for(size_t pixels) {
  const size_t g = (pixels + kBThreads - 1) / kBThreads;
  const size_t cap = 256 * 16;   // 256 CUs x 16 blocks, grid-stride the rest
  return (unsigned)(g < cap ? (g ? g : 1) : cap);
}

// The tiles of one axis that may carry weight at coordinate x, ascending: hi - 1, hi and the clamped last one, where hi is the
// last regular start at or before x + feather.  t[] tile index, u[] the coordinate inside the patch, w[] the weight — 0 for a
// candidate that does not exist (hi = 0; the last tile is hi itself) or does not reach x, and u lies in [0, P) wherever w > 0.
__device__ __forceinline__ void axis_candidates(int x, int L, int P, int border, int feather, int inner, int tiles, int (&t)[3],
                                                int (&u)[3], int (&w)[3]) {
  int hi = (x + feather) / inner;
  if (hi > tiles - 1) hi = tiles - 1;
  t[0] = hi - 1;
  t[1] = hi;
  t[2] = tiles - 1;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const int s = t[j] == tiles - 1 ? L - inner : t[j] * inner;
    const int uu = x - s + border;
    int ww = (uu + 1 < P - uu ? uu + 1 : P - uu) - (border - feather);
    ww = ww < 0 ? 0 : (ww > 2 * feather ? 2 * feather : ww);
    u[j] = uu;
    w[j] = ww;
  }
  if (hi < 1) w[0] = 0;
  if (hi == tiles - 1) w[2] = 0;
}

// C > 0: the channel count at compile time; C == 0: c_rt channels.  MAPS: a slot map and a validity bitmap stand in front of a
// compact patch buffer of `count` slots (nodata.hip); without them patch k lies at index k.
template <int C, bool MAPS>
__global__ __launch_bounds__(kBThreads) void recompose_blend_kernel(const float* __restrict__ patches, int count, int P, int border,
                                                                    int feather, const int* __restrict__ slot_of_patch,
                                                                    const unsigned* __restrict__ bits, int words_per_row,
                                                                    float* __restrict__ img, int H, int W, int x_tiles, int y_tiles,
                                                                    float scale, size_t first_pix, size_t total_pix, int c_rt) {
  const int inner = P - 2 * border;
  const int cc = C > 0 ? C : c_rt;
  const size_t pp = (size_t)P * P;
  for (size_t i = first_pix + (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total_pix; i += (size_t)gridDim.x * blockDim.x) {
    const int y = (int)(i / W), x = (int)(i - (size_t)y * W);
    float* dst = img + i * cc;
    // the (up to 3 x 3) candidate patches of this pixel, ascending (ty, tx): weight (0: carries none, or has no slot) and where
    // the value of channel 0 lies.  Every index below is a constant once the loops are unrolled: registers, no scratch.
    int wgt[9];
    size_t off[9];
    int n = 0, wsum_i = 0;
    size_t one = 0;
    bool data = true;
    if constexpr (MAPS) data = (bits[(size_t)y * words_per_row + (x >> 5)] >> (x & 31)) & 1u;
    int ty[3], uy[3], wy[3], tx[3], ux[3], wx[3];
    axis_candidates(y, H, P, border, feather, inner, y_tiles, ty, uy, wy);
    axis_candidates(x, W, P, border, feather, inner, x_tiles, tx, ux, wx);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
      for (int b = 0; b < 3; ++b) {
        int w = 0;
        size_t o = 0;
        if (data && wy[a] * wx[b] > 0) {
          long long k = (long long)ty[a] * x_tiles + tx[b];
          if constexpr (MAPS) {
            const int slot = slot_of_patch[k];
            k = (slot >= 0 && slot < count) ? slot : -1;
          }
          if (k >= 0) {
            w = wy[a] * wx[b];
            o = (size_t)k * cc * pp + (size_t)uy[a] * P + ux[b];
            one = o;
            ++n;
            wsum_i += w;
          }
        }
        wgt[a * 3 + b] = w;
        off[a * 3 + b] = o;
      }
    }
    if (n == 1) {                       // one patch: (w * p) / w is p — the hard cut's pixel, at the hard cut's cost
      const float* src = patches + one;
      if constexpr (C > 0) {
#pragma unroll
        for (int c = 0; c < C; ++c) dst[c] = src[(size_t)c * pp] * scale;
      } else {
        for (int c = 0; c < cc; ++c) dst[c] = src[(size_t)c * pp] * scale;
      }
      continue;
    }
    if (n == 0) {                       // no data, or (a map that drops a pixel's every patch) nothing to blend: 0
      if constexpr (C > 0) {
#pragma unroll
        for (int c = 0; c < C; ++c) dst[c] = 0.0f;
      } else {
        for (int c = 0; c < cc; ++c) dst[c] = 0.0f;
      }
      continue;
    }
    // Every candidate is LOADED, a weightless one from the address of a weighted one (`one`: in bounds, and a cache hit), and
    // selected away afterwards: nine independent loads per channel in flight instead of nine branches, each waiting for its own.
    const double wsum = (double)wsum_i;
#pragma unroll
    for (int j = 0; j < 9; ++j) off[j] = wgt[j] > 0 ? off[j] : one;
    auto blend = [&](int c) -> float {
      float v[9];
#pragma unroll
      for (int j = 0; j < 9; ++j) v[j] = patches[off[j] + (size_t)c * pp];
      double acc = 0.0;
      bool first = true;
#pragma unroll
      for (int j = 0; j < 9; ++j) {
        const double term = (double)wgt[j] * (double)v[j];
        const double next = first ? term : acc + term;      // a left fold that starts at its first term
        acc = wgt[j] > 0 ? next : acc;
        first = first && !(wgt[j] > 0);
      }
      return (float)(acc / wsum) * scale;
    };
    if constexpr (C > 0) {
#pragma unroll
      for (int c = 0; c < C; ++c) dst[c] = blend(c);
    } else {
      for (int c = 0; c < cc; ++c) dst[c] = blend(c);
    }
  }
}

}  // namespace
}  // namespace dsen2

using namespace dsen2;

extern "C" int dsen2_recompose_rows_blend(const float* dev_patches, int count_or_slots, int C, int P, int border, int feather,
                                          const int* dev_slot_of_patch, const unsigned int* dev_valid_bits, float* dev_img, int H,
                                          int W, float scale, int row0, int row1, void* stream) {
  return guarded([&]() -> int {
    const char* who = "recompose_rows_blend";
    const bool maps = dev_slot_of_patch != nullptr;
    if ((dev_slot_of_patch != nullptr) != (dev_valid_bits != nullptr))
      return fail(DSEN2_ERR_INVALID, "%s: the slot map and the bitmap go together", who);
    if (!dev_img || (!dev_patches && !(maps && count_or_slots == 0))) return fail(DSEN2_ERR_INVALID, "%s: NULL argument", who);
    if (count_or_slots < 0 || C < 1) return fail(DSEN2_ERR_INVALID, "%s: bad argument (count=%d C=%d)", who, count_or_slots, C);
    if (H <= 0 || W <= 0 || P <= 0 || border < 0) return fail(DSEN2_ERR_INVALID, "%s: bad argument", who);
    const long long inner = (long long)P - 2LL * border;
    if (inner <= 0 || H < inner || W < inner)
      return fail(DSEN2_ERR_INVALID, "%s geometry: P=%d border=%d H=%d W=%d", who, P, border, H, W);
    if (4LL * border > P) return fail(DSEN2_ERR_INVALID, "%s: border %d exceeds a quarter of the patch of %d", who, border, P);
    if (feather < 1 || feather > border) return fail(DSEN2_ERR_INVALID, "%s: feather %d outside 1..%d", who, feather, border);
    const long long x_tiles = (W + inner - 1) / inner, y_tiles = (H + inner - 1) / inner;
    if (x_tiles * y_tiles >= (1LL << 31)) return fail(DSEN2_ERR_INVALID, "%s: too many patches", who);
    if (!maps && x_tiles * y_tiles > count_or_slots)
      return fail(DSEN2_ERR_INVALID, "%s: %d patches for a grid of %lld x %lld", who, count_or_slots, y_tiles, x_tiles);
    if (row0 < 0 || row1 > H || row0 > row1) return fail(DSEN2_ERR_INVALID, "%s: rows [%d, %d) of %d", who, row0, row1, H);
    if (row0 == row1) return DSEN2_OK;
    const int wpr = (int)(((long long)W + 31) / 32);
    const size_t first_pix = (size_t)row0 * W, total_pix = (size_t)row1 * W;
    const dim3 grid(blend_grid_for(total_pix - first_pix)), block(kBThreads);
    hipStream_t st = (hipStream_t)stream;
#define DSEN2_BLEND_LAUNCH(CC, MM)                                                                                                    \
  hipLaunchKernelGGL((recompose_blend_kernel<CC, MM>), grid, block, 0, st, dev_patches, count_or_slots, P, border, feather,          \
                     dev_slot_of_patch, dev_valid_bits, wpr, dev_img, H, W, (int)x_tiles, (int)y_tiles, scale, first_pix, total_pix, C)
    if (maps) {
      switch (C) {
        case 2: DSEN2_BLEND_LAUNCH(2, true); break;
        case 6: DSEN2_BLEND_LAUNCH(6, true); break;
        default: DSEN2_BLEND_LAUNCH(0, true);
      }
    } else {
      switch (C) {
        case 2: DSEN2_BLEND_LAUNCH(2, false); break;
        case 6: DSEN2_BLEND_LAUNCH(6, false); break;
        default: DSEN2_BLEND_LAUNCH(0, false);
      }
    }
#undef DSEN2_BLEND_LAUNCH
    HIP_TRY(hipGetLastError());
    return DSEN2_OK;
  });
}
