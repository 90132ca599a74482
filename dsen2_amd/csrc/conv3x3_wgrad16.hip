// conv3x3_wgrad16.hip — weight and bias gradient of a stride-1, pad-1 3x3 convolution F -> F (F = 128, 256) as bf16x3 on the
// gfx950 bf16 matrix cores: the training counterpart of conv3x3_body16w.hip (X3).
//
//   dW[tap][ci][co] = scale * sum_p a[p + (ky-1, kx-1)][ci] * g[p][co]      (tap = 3*ky + kx, zero padding)
//   db[co]          = scale * sum_p g[p][co]
// a and g are two-plane blocked operand tensors [n][2][F/8][h][w][8] bf16, value = plane 0 + plane 1 (what conv-A writes as t,
// what launch_split3_f32 writes as hx, what launch_mask_split3 writes as du).  Every product is a0*g0 + a0*g1 + a1*g0 with
// fp32 accumulators (the a1*g1 term is 2^-18 of the product).  dW is written in keras HWIO order, db after it.
//
// GEMM view, as in conv3x3_wgrad.hip: M = co (the A operand, g), N = ci (the B operand, a shifted by the tap), K = pixels.
// v_mfma_f32_32x32x16_bf16: lane l holds A[co = l&31][k = 8*(l>>5) + j] and B[k][ci = l&31], j = 0..7 — eight consecutive K
// values of one channel in 16 bytes.  The tensors are pixel-major (8 channels per 16 bytes), so a tile is TRANSPOSED on its way
// into LDS: [plane][channel][row][column] bf16, and K runs along a tile row: one MFMA contracts the 16 pixels of one row.
//   * workgroup = 4 waves; it owns a 128 (co) x 32 (ci) block for all nine taps, wave w the 32 x 32 block of co 32w..32w+31
//     (9 accumulators of 16 registers);
//   * pixel tile 4 x 16; staged per tile: g [2][128][4][16] and the haloed a [2][32][6][20] (LDS column c = image column
//     tx0 - 2 + c, so that a staging thread's two neighbouring pixels x, x + 1 (x even) make one aligned 32-bit LDS write per
//     channel).  Global loads are 16 bytes (8 channels of a pixel); two pixels are interleaved in registers (v_perm) and
//     written as 8 ds_write_b32.  Double buffered: the next tile's global loads are issued before the current tile's MFMAs;
//   * the tap's column shift kx is a shift of kx + 1 elements = 2, 4 or 6 bytes against the aligned rows: a lane reads the
//     16 aligned columns 8*(l>>5) .. + 15 of a halo row once (two ds_read_b128) and forms the three shifted operands in
//     registers (v_alignbyte_b32 / whole dwords); that one read feeds up to 27 MFMAs (3 kx x 3 ky x 3 products).  No
//     sub-dword LDS read anywhere;
//   * channel pitches of 76 (a) and 36 (g) dwords: by address arithmetic the ds_read_b128 of 16 consecutive lanes start in 16
//     different groups of four of the 64 banks (not confirmed with a counter);
//   * one g tile is staged by every ci block of its co block (F / 32 workgroups: 4 at F = 128, 8 at F = 256) and the kernel
//     runs one workgroup per CU (292 VGPRs, 110 KiB of LDS): what that costs is in profiles/train_bf16x3.md;
//   * split-K exactly as conv3x3_wgrad.hip: contiguous tile runs, a split count that does not depend on the device, partial
//     sums to a workspace, a second kernel adds them in split order (double) — no float atomics, the same bits on every run.
// Pixels outside the image (ragged tiles, the halo) are staged as zeros in both planes: they add exact zeros.
//
// ONE-PLANE INSTANCE (PL = 1; mixed-precision training of an fp32 model, capi_train.hip gradients_amp): a and g are one-plane
// blocked bf16 tensors [n][F/8][h][w][8] (conv-A's bf16 t, the hi plane of a residual stream, launch_mask_round16's du) and a
// product is the one MFMA a*g: one v_mfma_f32_32x32x16_bf16 per tap and row where PL = 2 issues three; the staging registers
// and the LDS tile are half as large (55 KiB), everything else above — block, pixel tile, transposed staging, alignbyte
// shifts, split count, second pass, zeros outside the image — is the same code.  Resource usage and what it allows: see
// kMinBlocks below.
#include "conv3x3_bf16_common.h"

namespace dsen2 {

namespace {

using bf16k::bf16x8;

constexpr int kTY = 4, kTX = 16;                  // pixel tile
constexpr int kHY = kTY + 2;                      // halo rows of a
// LDS columns per halo row (48 B).  Columns 0..19 are staged, 1..18 feed MFMAs.  Columns 20..23 are never written: the upper
// lane half's second ds_read_b128 (columns 16..23) brings them into w1[2], w1[3], which no operand is formed from.
constexpr int kACols = 24;
constexpr int kAPairs = 10, kGPairs = kTX / 2;    // staged pixel pairs per row
constexpr int kACh = kHY * kACols + 8;            // bf16 per channel of a: 152 (76 dwords)
constexpr int kGCh = kTY * kTX + 8;               // bf16 per channel of g: 72 (36 dwords)
constexpr int kCOB = 128, kCIB = 32;
constexpr int kThreads = 256;
constexpr int kAPlane = kCIB * kACh, kGPlane = kCOB * kGCh;
// what depends on the number of operand planes PL (2 = bf16x3, 1 = bf16)
template <int PL>
struct Planes {
  static constexpr int kBufElems = PL * kAPlane + PL * kGPlane;
  static constexpr size_t kLdsBytes = (size_t)2 * kBufElems * 2;      // 110 KiB / 55 KiB
  static constexpr int kAPieces = PL * (kCIB / 8) * kHY * kAPairs;    // (plane, 8-channel block, row, pixel pair): 480 / 240
  static constexpr int kGPieces = PL * (kCOB / 8) * kTY * kGPairs;    // 1024 / 512
  static constexpr int kARounds = (kAPieces + kThreads - 1) / kThreads, kGRounds = kGPieces / kThreads;
  // Workgroups per CU the kernel is compiled for.  PL = 2: 148 VGPRs + 144 AGPRs and 110 KiB of LDS, one.  PL = 1: compiled
  // for two, hipcc's resource usage is 226 registers (accumulators included, no AGPRs) with no spill and no scratch — inside
  // the 256 a wave gets at two waves per SIMD — and 2 x 55 KiB of LDS fit the CU's 160 KiB.  A launch has at most
  // kTargetBlocks = 256 workgroups, one per CU of a whole MI355X, and there a build for one workgroup per CU measures the same
  // (65.5 / 65.7 us at F = 128 batch 128, 24.8 / 24.8 us at F = 256 batch 8: profiles/train_amp_bf16.md); two is kept because it
  // costs nothing and is what a device with fewer CUs than workgroups (a compute partition) uses.  The split count is not
  // raised to fill the slot: by byte count the partials at F = 256, batch 8 (16 splits x 2.36 MB written and read back)
  // already outweigh the operands (2 x 4.2 MB).
  static constexpr int kMinBlocks = PL == 1 ? 2 : 1;
  static_assert(kGPieces % kThreads == 0, "g pieces");
  static_assert(kLdsBytes * kMinBlocks <= 160 * 1024, "LDS budget");
};
constexpr int kTargetBlocks = 256;    // workgroups per launch the split count aims at; fixed, so the summation order — and
                                      // the result — does not depend on the device
static_assert(kACh % 8 == 0 && kGCh % 8 == 0 && (kACh / 8) % 2 == 1 && (kGCh / 8) % 2 == 1, "16-byte rows, odd 16-byte pitch");

struct Wgrad16Params {
  const u32x4* a;      // [n][PL][F/8][h][w] pixels of 8 bf16
  const u32x4* g;
  float* part;         // [splits][9][F][F]
  float* bpart;        // [splits][2][F]
  int n, h, w, nblk;   // nblk = F / 8
  int tiles_x, tiles_y;
  int splits, feat;
  long long tiles;
};

template <int PL>
__global__ __launch_bounds__(kThreads, Planes<PL>::kMinBlocks) void conv3x3_wgrad16_kernel(const Wgrad16Params p) {
  constexpr int kBufElems = Planes<PL>::kBufElems, kAPieces = Planes<PL>::kAPieces;
  constexpr int kARounds = Planes<PL>::kARounds, kGRounds = Planes<PL>::kGRounds;
  extern __shared__ __attribute__((aligned(16))) unsigned short smem16[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, khalf = lane >> 5;
  const int nco = p.feat / kCOB;
  const int cob0 = (blockIdx.y % nco) * kCOB, cib0 = (blockIdx.y / nco) * kCIB;
  const int split = blockIdx.x;
  const long long t_begin = p.tiles * split / p.splits, t_end = p.tiles * (split + 1) / p.splits;
  const int tiles_per_img = p.tiles_x * p.tiles_y;
  const size_t img_pix = (size_t)p.h * p.w;
  const bool bias_block = cib0 == 0;

  const u32x4 zero4 = {0u, 0u, 0u, 0u};
  u32x4 ar[kARounds][2], gr[kGRounds][2];
  auto load_tile = [&](long long t) {
    const int img = (int)(t / tiles_per_img);
    const int trem = (int)(t - (long long)img * tiles_per_img);
    const int ty0 = (trem / p.tiles_x) * kTY, tx0 = (trem % p.tiles_x) * kTX;
#pragma unroll
    for (int r = 0; r < kARounds; ++r) {
      const int pc = r * kThreads + tid;
      const int cp = pc % kAPairs, row = (pc / kAPairs) % kHY, blk = (pc / (kAPairs * kHY)) % (kCIB / 8), plane = pc / (kAPairs * kHY * (kCIB / 8));
      const int gy = ty0 - 1 + row, gx = tx0 - 2 + 2 * cp;
      const bool ok = pc < kAPieces && (unsigned)gy < (unsigned)p.h;
      const u32x4* src = p.a + (((size_t)img * PL + plane) * p.nblk + (cib0 >> 3) + blk) * img_pix + (size_t)(ok ? gy : 0) * p.w;
      ar[r][0] = ok && (unsigned)gx < (unsigned)p.w ? src[gx] : zero4;
      ar[r][1] = ok && (unsigned)(gx + 1) < (unsigned)p.w ? src[gx + 1] : zero4;
    }
#pragma unroll
    for (int r = 0; r < kGRounds; ++r) {
      const int pc = r * kThreads + tid;
      const int cp = pc % kGPairs, row = (pc / kGPairs) % kTY, blk = (pc / (kGPairs * kTY)) % (kCOB / 8), plane = pc / (kGPairs * kTY * (kCOB / 8));
      const int gy = ty0 + row, gx = tx0 + 2 * cp;
      const bool ok = gy < p.h;
      const u32x4* src = p.g + (((size_t)img * PL + plane) * p.nblk + (cob0 >> 3) + blk) * img_pix + (size_t)(ok ? gy : 0) * p.w;
      gr[r][0] = ok && gx < p.w ? src[gx] : zero4;
      gr[r][1] = ok && gx + 1 < p.w ? src[gx + 1] : zero4;
    }
  };
  // two pixels x 8 channels -> 8 dwords (channel j: pixel x in the low half, x + 1 in the high half) at [channel][row][2 * cp]
  auto store_pair = [&](unsigned* dst, int ch_pitch_dwords, const u32x4& p0, const u32x4& p1) {
#pragma unroll
    for (int j = 0; j < 8; ++j)
      dst[j * ch_pitch_dwords] = __builtin_amdgcn_perm(p1[j >> 1], p0[j >> 1], (j & 1) ? 0x07060302u : 0x05040100u);
  };
  auto store_tile = [&](int buf) {
    unsigned* const a_s = reinterpret_cast<unsigned*>(smem16 + buf * kBufElems);
    unsigned* const g_s = a_s + PL * kAPlane / 2;         // (dwords: behind the PL planes of a)
#pragma unroll
    for (int r = 0; r < kARounds; ++r) {
      const int pc = r * kThreads + tid;
      const int cp = pc % kAPairs, row = (pc / kAPairs) % kHY, blk = (pc / (kAPairs * kHY)) % (kCIB / 8), plane = pc / (kAPairs * kHY * (kCIB / 8));
      if (pc < kAPieces) store_pair(a_s + (plane * kAPlane + blk * 8 * kACh + row * kACols) / 2 + cp, kACh / 2, ar[r][0], ar[r][1]);
    }
#pragma unroll
    for (int r = 0; r < kGRounds; ++r) {
      const int pc = r * kThreads + tid;
      const int cp = pc % kGPairs, row = (pc / kGPairs) % kTY, blk = (pc / (kGPairs * kTY)) % (kCOB / 8), plane = pc / (kGPairs * kTY * (kCOB / 8));
      store_pair(g_s + (plane * kGPlane + blk * 8 * kGCh + row * kTX) / 2 + cp, kGCh / 2, gr[r][0], gr[r][1]);
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
    const unsigned short* const a_l = smem16 + cur * kBufElems + l31 * kACh + 8 * khalf;
    const unsigned short* const g_l = smem16 + cur * kBufElems + PL * kAPlane + (wave * 32 + l31) * kGCh + 8 * khalf;
    // the A operands of the tile: this lane's 8 pixels of every row, every plane
    u32x4 gop[PL][kTY];
#pragma unroll
    for (int pl = 0; pl < PL; ++pl)
#pragma unroll
      for (int y = 0; y < kTY; ++y) gop[pl][y] = *reinterpret_cast<const u32x4*>(g_l + pl * kGPlane + y * kTX);
    if (bias_block) {
#pragma unroll
      for (int y = 0; y < kTY; ++y)
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
          for (int pl = 0; pl < PL; ++pl) {
            bsum += __builtin_bit_cast(float, gop[pl][y][k] << 16);
            bsum += __builtin_bit_cast(float, gop[pl][y][k] & 0xffff0000u);
          }
    }
#pragma unroll
    for (int r = 0; r < kHY; ++r) {
      // halo row r, columns 8*khalf .. + 15 (dwords w[0..7]); the operand of tap column kx is columns + kx + 1 .. + kx + 8
      u32x4 bop[PL][3];
#pragma unroll
      for (int pl = 0; pl < PL; ++pl) {
        const u32x4 w0 = *reinterpret_cast<const u32x4*>(a_l + pl * kAPlane + r * kACols);
        const u32x4 w1 = *reinterpret_cast<const u32x4*>(a_l + pl * kAPlane + r * kACols + 8);
        const unsigned w[6] = {w0[0], w0[1], w0[2], w0[3], w1[0], w1[1]};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          bop[pl][0][i] = __builtin_amdgcn_alignbyte(w[i + 1], w[i], 2);
          bop[pl][1][i] = w[i + 1];
          bop[pl][2][i] = __builtin_amdgcn_alignbyte(w[i + 2], w[i + 1], 2);
        }
      }
#pragma unroll
      for (int ky = 0; ky < 3; ++ky) {
        const int y = r - ky;            // halo row r = image row ty0 - 1 + r = output row y + tap row ky - 1
        if (y < 0 || y >= kTY) continue;
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
          const int tap = 3 * ky + kx;
          const bf16x8 g0 = __builtin_bit_cast(bf16x8, gop[0][y]), a0 = __builtin_bit_cast(bf16x8, bop[0][kx]);
          acc[tap] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(g0, a0, acc[tap], 0, 0, 0);
          if constexpr (PL == 2) {
            const bf16x8 g1 = __builtin_bit_cast(bf16x8, gop[1][y]), a1 = __builtin_bit_cast(bf16x8, bop[1][kx]);
            acc[tap] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(g1, a0, acc[tap], 0, 0, 0);
            acc[tap] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(g0, a1, acc[tap], 0, 0, 0);
          }
        }
      }
    }
    if (more) store_tile(cur ^ 1);
    __syncthreads();
  }

  // D[co][ci]: the lane owns column ci = l31 and rows co = (r & 3) + 8 * (r >> 2) + 4 * khalf: four consecutive co per quad
  const int ci = cib0 + l31;
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    float* const dst = p.part + (((size_t)split * 9 + k) * p.feat + ci) * p.feat + cob0 + wave * 32 + 4 * khalf;
#pragma unroll
    for (int q = 0; q < 4; ++q)
      *reinterpret_cast<f32x4*>(dst + 8 * q) = f32x4{acc[k][4 * q], acc[k][4 * q + 1], acc[k][4 * q + 2], acc[k][4 * q + 3]};
  }
  if (bias_block) p.bpart[((size_t)split * 2 + khalf) * p.feat + cob0 + wave * 32 + l31] = bsum;
}

// second pass: every weight / bias gradient element = scale * (its partials added in split order)
__global__ __launch_bounds__(256) void conv3x3_wgrad16_reduce_kernel(const float* __restrict__ part, const float* __restrict__ bpart,
                                                                     float* __restrict__ dw, float* __restrict__ db, int splits,
                                                                     int feat, float scale) {
  const size_t nw = (size_t)9 * feat * feat;
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < nw) {
    double s = 0.0;
    for (int k = 0; k < splits; ++k) s += (double)part[(size_t)k * nw + i];
    dw[i] = (float)(s * (double)scale);
  } else if (i < nw + (size_t)feat) {
    const int co = (int)(i - nw);
    double s = 0.0;
    for (int k = 0; k < splits; ++k) s += (double)bpart[(size_t)2 * k * feat + co] + (double)bpart[((size_t)2 * k + 1) * feat + co];
    db[co] = (float)(s * (double)scale);
  }
}

struct Wgrad16Geom {
  int splits, tiles_x, tiles_y;
  long long tiles;
};

bool wgrad16_geom(int n, int h, int w, int feat, Wgrad16Geom* g) {
  if (n <= 0 || h <= 0 || w <= 0 || (feat != 128 && feat != 256)) return false;
  g->tiles_x = (w + kTX - 1) / kTX;
  g->tiles_y = (h + kTY - 1) / kTY;
  g->tiles = (long long)n * g->tiles_x * g->tiles_y;
  const int blocks = (feat / kCOB) * (feat / kCIB);
  long long s = kTargetBlocks / blocks;
  if (s > g->tiles) s = g->tiles;
  g->splits = (int)s;
  return true;
}

}  // namespace

size_t wgrad16_workspace_floats(int n, int h, int w, int feat) {
  Wgrad16Geom g;
  if (!wgrad16_geom(n, h, w, feat, &g)) return 0;
  return (size_t)g.splits * ((size_t)9 * feat * feat + (size_t)2 * feat);
}

bool wgrad16_geometry(int n, int h, int w, int feat, long long* tiles, int* splits) {
  Wgrad16Geom g;
  if (!wgrad16_geom(n, h, w, feat, &g)) return false;
  *tiles = g.tiles;
  *splits = g.splits;
  return true;
}

namespace {

template <int PL>
hipError_t launch_wgrad16(const void* a_planes, const void* g_planes, int n, int h, int w, int feat, float scale, float* dw, float* db,
                          float* ws, size_t ws_floats, hipStream_t stream) {
  Wgrad16Geom geo;
  if (!a_planes || !g_planes || !dw || !db || !ws || !wgrad16_geom(n, h, w, feat, &geo)) return hipErrorInvalidValue;
  if ((size_t)h * w * feat >= ((size_t)1 << 29)) return hipErrorInvalidValue;
  const size_t part_floats = (size_t)geo.splits * 9 * feat * feat;
  if (ws_floats < part_floats + (size_t)geo.splits * 2 * feat) return hipErrorInvalidValue;
  Wgrad16Params p;
  p.a = reinterpret_cast<const u32x4*>(a_planes);
  p.g = reinterpret_cast<const u32x4*>(g_planes);
  p.part = ws; p.bpart = ws + part_floats;
  p.n = n; p.h = h; p.w = w; p.nblk = feat / 8;
  p.tiles_x = geo.tiles_x; p.tiles_y = geo.tiles_y;
  p.splits = geo.splits; p.feat = feat; p.tiles = geo.tiles;
  constexpr auto kern = conv3x3_wgrad16_kernel<PL>;
  constexpr size_t kLdsBytes = Planes<PL>::kLdsBytes;
  hipError_t e = prepare_kernel<kern>(kLdsBytes, nullptr);
  if (e != hipSuccess) return e;
  const dim3 grid((unsigned)geo.splits, (unsigned)((feat / kCOB) * (feat / kCIB)), 1);
  e = launch_kernel<kern>(grid, kThreads, kLdsBytes, stream, p);
  if (e != hipSuccess) return e;
  const size_t total = (size_t)9 * feat * feat + feat;
  hipLaunchKernelGGL(conv3x3_wgrad16_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, p.part, p.bpart,
                     dw, db, geo.splits, feat, scale);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_conv3x3_wgrad16(const void* a_planes, const void* g_planes, int n, int h, int w, int feat, float scale, float* dw,
                                  float* db, float* ws, size_t ws_floats, hipStream_t stream) {
  return launch_wgrad16<2>(a_planes, g_planes, n, h, w, feat, scale, dw, db, ws, ws_floats, stream);
}

hipError_t launch_conv3x3_wgrad16_bf16(const void* a, const void* g, int n, int h, int w, int feat, float scale, float* dw, float* db,
                                       float* ws, size_t ws_floats, hipStream_t stream) {
  return launch_wgrad16<1>(a, g, n, h, w, feat, scale, dw, db, ws, ws_floats, stream);
}

}  // namespace dsen2
