// conv3x3_wgrad.hip — weight and bias gradient of a stride-1, pad-1 3x3 convolution on the gfx950 fp32 matrix cores.
//
//   dW[tap][ci][co] = scale * sum_p a[p + (ky-1, kx-1)][ci] * g[p][co]      (tap = 3*ky + kx, zero padding)
//   db[co]          = scale * sum_p g[p][co]
// over all n*h*w pixels p.  a and g are NHWC fp32 with `ca` / `cg` channels per pixel; dW is written in keras HWIO order
// (3, 3, ci, co) for the first ci x co channels, db after it — the layout of one Conv2D inside the keras-flat vector.
// One kernel serves the three layer kinds of the network: body (ci = co = F), first (a = the NHWC16 input tensor,
// ci <= 16) and output (g = dL/dout padded to 16 channels).
//
// GEMM view: M = co (the A operand, g), N = ci (the B operand, a shifted by the tap), K = pixels.
// v_mfma_f32_32x32x2_f32: lane l gives A[co = l&31][pixel 2s + (l>>5)] and B[same pixel, shifted][ci = l&31]; one g value
// feeds the nine taps' MFMAs, so a pixel pair costs 1 + 9 LDS reads per 9 MFMAs.
//   * workgroup = 4 waves; it owns a (COB = 32*WCO) x (CIB = 32*WCI) block of (co, ci) for all nine taps; wave w owns
//     one 32 x 32 block (9 accumulators of 16 registers = 144 per lane);
//   * the pixels are cut into 4 x 16 tiles; a tile of g (64 pixels x COB) and the haloed 6 x 18 tile of a (x CIB) are
//     staged in LDS (double buffered; the next tile's global loads are issued before the current tile's MFMAs);
//   * split-K: the tiles are divided into `splits` contiguous runs, one per workgroup column; each writes its partial sums
//     to the workspace, and a second kernel adds the partials of every element in split order — no float atomics, so the
//     result is the same bits on every run.  The bias partials come from the same staged g tiles.
// Pixels outside the image are zeros in the staged g tile: they add exact zeros to the accumulators.
#include "conv3x3_items.h"

namespace dsen2 {

namespace {

constexpr int kWgTY = 4, kWgTX = 16, kWgPix = kWgTY * kWgTX;   // pixel tile
constexpr int kWgHY = kWgTY + 2, kWgHX = kWgTX + 2, kWgHalo = kWgHY * kWgHX;
constexpr int kWgThreads = 256;
constexpr int kWgTargetBlocks = 256;    // workgroups per launch the split count aims at (one per CU); fixed, so the
                                        // summation order — and the result — does not depend on the device

struct WgradParams {
  const float* a;      // NHWC [n][h][w][ca]
  const float* g;      // NHWC [n][h][w][cg]
  float* part;         // [splits][9][cip][cop]
  float* bpart;        // [splits][2][cop]
  int n, h, w, ca, cg;
  int tiles_x, tiles_y;
  int splits, cip, cop;
  long long tiles;
};

template <int WCO, int WCI>
struct WgCfg {
  static constexpr int COB = 32 * WCO, CIB = 32 * WCI;
  static constexpr int ASTR = CIB + 4, GSTR = COB + 4;            // LDS floats per pixel (16-byte aligned rows)
  static constexpr int A_FLOATS = kWgHalo * ASTR, G_FLOATS = kWgPix * GSTR;
  static constexpr int A_PIECES = kWgHalo * CIB / 4, G_PIECES = kWgPix * COB / 4;
  static constexpr int A_ROUNDS = (A_PIECES + kWgThreads - 1) / kWgThreads;
  static constexpr int G_ROUNDS = (G_PIECES + kWgThreads - 1) / kWgThreads;
  static constexpr size_t LDS_BYTES = (size_t)2 * (A_FLOATS + G_FLOATS) * sizeof(float);
  static_assert(WCO * WCI == 4, "four waves");
  static_assert(LDS_BYTES <= 160 * 1024, "LDS budget");
};

template <int WCO, int WCI>
__global__ __launch_bounds__(kWgThreads, 1) void conv3x3_wgrad_kernel(const WgradParams p) {
  using C = WgCfg<WCO, WCI>;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wco = wave % WCO, wci = wave / WCO;
  const int l31 = lane & 31, hsel = lane >> 5;
  const int nco = p.cop / C::COB;
  const int cob0 = (blockIdx.y % nco) * C::COB, cib0 = (blockIdx.y / nco) * C::CIB;
  const int split = blockIdx.x;
  const long long t_begin = p.tiles * split / p.splits, t_end = p.tiles * (split + 1) / p.splits;
  const int tiles_per_img = p.tiles_x * p.tiles_y;
  const size_t img_pix = (size_t)p.h * p.w;
  const bool bias_wave = cib0 == 0 && wci == 0;

  f32x4 ar[C::A_ROUNDS], gr[C::G_ROUNDS];
  auto load_tile = [&](long long t) {
    // (not conv3x3_items.h's tile_at: 64-bit tile counter, and through the shared function hipcc orders this kernel's scalar
    // code differently)
    const int img = (int)(t / tiles_per_img);
    const int trem = (int)(t - (long long)img * tiles_per_img);
    const int ty0 = (trem / p.tiles_x) * kWgTY, tx0 = (trem % p.tiles_x) * kWgTX;
    const float* const a_img = p.a + (size_t)img * img_pix * p.ca;
    const float* const g_img = p.g + (size_t)img * img_pix * p.cg;
#pragma unroll
    for (int r = 0; r < C::A_ROUNDS; ++r) {
      const int pc = r * kWgThreads + tid;
      const int hp = pc / (C::CIB / 4), q = pc % (C::CIB / 4);
      const int gy = ty0 - 1 + hp / kWgHX, gx = tx0 - 1 + hp % kWgHX, ch = cib0 + 4 * q;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (pc < C::A_PIECES && ch < p.ca && (unsigned)gy < (unsigned)p.h && (unsigned)gx < (unsigned)p.w)
        v = *reinterpret_cast<const f32x4*>(a_img + ((size_t)gy * p.w + gx) * p.ca + ch);
      ar[r] = v;
    }
#pragma unroll
    for (int r = 0; r < C::G_ROUNDS; ++r) {
      const int pc = r * kWgThreads + tid;
      const int px = pc / (C::COB / 4), q = pc % (C::COB / 4);
      const int gy = ty0 + px / kWgTX, gx = tx0 + px % kWgTX, ch = cob0 + 4 * q;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (pc < C::G_PIECES && ch < p.cg && gy < p.h && gx < p.w)
        v = *reinterpret_cast<const f32x4*>(g_img + ((size_t)gy * p.w + gx) * p.cg + ch);
      gr[r] = v;
    }
  };
  auto store_tile = [&](int buf) {
    float* const a_s = smem + buf * (C::A_FLOATS + C::G_FLOATS);
    float* const g_s = a_s + C::A_FLOATS;
#pragma unroll
    for (int r = 0; r < C::A_ROUNDS; ++r) {
      const int pc = r * kWgThreads + tid;
      if (pc < C::A_PIECES)
        *reinterpret_cast<f32x4*>(a_s + (pc / (C::CIB / 4)) * C::ASTR + 4 * (pc % (C::CIB / 4))) = ar[r];
    }
#pragma unroll
    for (int r = 0; r < C::G_ROUNDS; ++r) {
      const int pc = r * kWgThreads + tid;
      if (pc < C::G_PIECES)
        *reinterpret_cast<f32x4*>(g_s + (pc / (C::COB / 4)) * C::GSTR + 4 * (pc % (C::COB / 4))) = gr[r];
    }
  };

  f32x16 acc[9];
#pragma unroll
  for (int k = 0; k < 9; ++k)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[k][e] = 0.f;
  float bsum = 0.f;

  if (t_begin < t_end) {
    load_tile(t_begin);
    store_tile(0);
  }
  __syncthreads();
#pragma unroll 1
  for (long long t = t_begin; t < t_end; ++t) {
    const int cur = (int)((t - t_begin) & 1);
    const bool more = t + 1 < t_end;
    if (more) load_tile(t + 1);
    const float* const a_s = smem + cur * (C::A_FLOATS + C::G_FLOATS) + wci * 32 + l31;
    const float* const g_s = smem + cur * (C::A_FLOATS + C::G_FLOATS) + C::A_FLOATS + wco * 32 + l31;
#pragma unroll 4
    for (int s = 0; s < kWgPix / 2; ++s) {
      const int px = 2 * s + hsel;                       // this lane half's pixel of the pair
      const int py = px / kWgTX, pxx = px % kWgTX;
      const float ga = g_s[px * C::GSTR];
      if (bias_wave) bsum += ga;
      float b[9];
#pragma unroll
      for (int k = 0; k < 9; ++k) b[k] = a_s[((py + k / 3) * kWgHX + pxx + k % 3) * C::ASTR];
#pragma unroll
      for (int k = 0; k < 9; ++k) acc[k] = __builtin_amdgcn_mfma_f32_32x32x2f32(ga, b[k], acc[k], 0, 0, 0);
    }
    if (more) store_tile(cur ^ 1);
    __syncthreads();
  }

  // D[co][ci]: the lane owns column ci = l31 and rows co = (r & 3) + 8 * (r >> 2) + 4 * hsel: four consecutive co per quad
  const int ci = cib0 + wci * 32 + l31;
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    float* const dst = p.part + (((size_t)split * 9 + k) * p.cip + ci) * p.cop + cob0 + wco * 32 + 4 * hsel;
#pragma unroll
    for (int q = 0; q < 4; ++q)
      *reinterpret_cast<f32x4*>(dst + 8 * q) = f32x4{acc[k][4 * q], acc[k][4 * q + 1], acc[k][4 * q + 2], acc[k][4 * q + 3]};
  }
  if (bias_wave) p.bpart[((size_t)split * 2 + hsel) * p.cop + cob0 + wco * 32 + l31] = bsum;
}

// second pass: every weight / bias gradient element = scale * (its partials added in split order)
__global__ __launch_bounds__(256) void conv3x3_wgrad_reduce_kernel(const float* __restrict__ part, const float* __restrict__ bpart,
                                                                   float* __restrict__ dw, float* __restrict__ db, int splits,
                                                                   int cip, int cop, int ci_real, int co_real, float scale) {
  const size_t nw = (size_t)9 * ci_real * co_real;
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < nw) {
    const int co = (int)(i % co_real);
    const size_t r = i / co_real;
    const int ci = (int)(r % ci_real), tap = (int)(r / ci_real);
    const size_t stride = (size_t)9 * cip * cop;
    const float* src = part + ((size_t)tap * cip + ci) * cop + co;
    double s = 0.0;
    for (int k = 0; k < splits; ++k) s += (double)src[(size_t)k * stride];
    dw[i] = (float)(s * (double)scale);
  } else if (i < nw + (size_t)co_real) {
    const int co = (int)(i - nw);
    double s = 0.0;
    for (int k = 0; k < splits; ++k) s += (double)bpart[(size_t)2 * k * cop + co] + (double)bpart[((size_t)2 * k + 1) * cop + co];
    db[co] = (float)(s * (double)scale);
  }
}

struct WgradGeom {
  int wco, wci, cip, cop, splits, tiles_x, tiles_y;
  long long tiles;
};

bool wgrad_geom(int n, int h, int w, int ca, int cg, WgradGeom* g) {
  if (n <= 0 || h <= 0 || w <= 0 || ca <= 0 || cg <= 0 || ca % 4 != 0 || cg % 4 != 0) return false;
  if (cg % 128 == 0) {
    g->wco = 4; g->wci = 1;          // body and first layers: a 128-wide co block, 32 ci
  } else if (cg <= 32 && ca % 128 == 0) {
    g->wco = 1; g->wci = 4;          // output layer: the (padded) outputs in one 32-wide co block, 128 ci
  } else {
    return false;
  }
  const int cob = 32 * g->wco, cib = 32 * g->wci;
  g->cop = (cg + cob - 1) / cob * cob;
  g->cip = (ca + cib - 1) / cib * cib;
  g->tiles_x = (w + kWgTX - 1) / kWgTX;
  g->tiles_y = (h + kWgTY - 1) / kWgTY;
  g->tiles = (long long)n * g->tiles_x * g->tiles_y;
  const int blocks = (g->cop / cob) * (g->cip / cib);
  long long s = kWgTargetBlocks / blocks;
  if (s < 1) s = 1;
  if (s > g->tiles) s = g->tiles;
  g->splits = (int)s;
  return true;
}

template <int WCO, int WCI>
hipError_t launch_wgrad_one(const WgradParams& p, hipStream_t stream) {
  using C = WgCfg<WCO, WCI>;
  constexpr auto kern = conv3x3_wgrad_kernel<WCO, WCI>;
  const hipError_t e = prepare_kernel<kern>(C::LDS_BYTES, nullptr);
  if (e != hipSuccess) return e;
  const dim3 grid((unsigned)p.splits, (unsigned)((p.cop / C::COB) * (p.cip / C::CIB)), 1);
  return launch_kernel<kern>(grid, kWgThreads, C::LDS_BYTES, stream, p);
}

}  // namespace

size_t wgrad_workspace_floats(int n, int h, int w, int ca, int cg) {
  WgradGeom g;
  if (!wgrad_geom(n, h, w, ca, cg, &g)) return 0;
  return (size_t)g.splits * ((size_t)9 * g.cip * g.cop + (size_t)2 * g.cop);
}

bool wgrad_geometry(int n, int h, int w, int ca, int cg, long long* tiles, int* splits) {
  WgradGeom g;
  if (!wgrad_geom(n, h, w, ca, cg, &g)) return false;
  *tiles = g.tiles;
  *splits = g.splits;
  return true;
}

hipError_t launch_conv3x3_wgrad(const float* a, int ca, const float* g, int cg, int n, int h, int w, int ci_real, int co_real,
                                float scale, float* dw, float* db, float* ws, size_t ws_floats, hipStream_t stream) {
  WgradGeom geo;
  if (!wgrad_geom(n, h, w, ca, cg, &geo) || ci_real <= 0 || ci_real > ca || co_real <= 0 || co_real > cg)
    return hipErrorInvalidValue;
  if ((size_t)h * w * (ca > cg ? ca : cg) >= ((size_t)1 << 31)) return hipErrorInvalidValue;
  const size_t part_floats = (size_t)geo.splits * 9 * geo.cip * geo.cop;
  if (ws_floats < part_floats + (size_t)geo.splits * 2 * geo.cop) return hipErrorInvalidValue;
  WgradParams p;
  p.a = a; p.g = g; p.part = ws; p.bpart = ws + part_floats;
  p.n = n; p.h = h; p.w = w; p.ca = ca; p.cg = cg;
  p.tiles_x = geo.tiles_x; p.tiles_y = geo.tiles_y;
  p.splits = geo.splits; p.cip = geo.cip; p.cop = geo.cop; p.tiles = geo.tiles;
  hipError_t e = geo.wco == 4 ? launch_wgrad_one<4, 1>(p, stream) : launch_wgrad_one<1, 4>(p, stream);
  if (e != hipSuccess) return e;
  const size_t total = (size_t)9 * ci_real * co_real + co_real;
  hipLaunchKernelGGL(conv3x3_wgrad_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, p.part, p.bpart,
                     dw, db, geo.splits, geo.cip, geo.cop, ci_real, co_real, scale);
  return hipGetLastError();
}

}  // namespace dsen2
