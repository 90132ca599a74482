// conv3x3_first.hip — the network's FIRST convolution (utils/DSen2Net.py:24-29): Concatenate(axis=1) of the two or
// three NCHW inputs, Conv2D(F, 3x3, 'same') + bias + ReLU -> NHWC fp32, exact fp32 arithmetic (precision 0).  The bf16-operand
// modes run this layer on the bf16 matrix cores and write the residual stream's planes: conv3x3_first16.hip.
//
// Round 2 ran this layer as pack_inputs_kernel (NCHW -> NHWC16, a 54 MB round trip) + conv3x3_mfma_kernel<16, 16, ...>:
// one 16x16-pixel tile per workgroup, the 72 KB of weights streamed from L2 for EVERY tile with a barrier per tap.
// With K = 9 x 10 the layer has 77 us of MFMA work and 268 MB of output at the bench config: it is bound by how well
// the two overlap, not by either.  This kernel:
//   * is persistent (one workgroup of 8 waves per CU walks tiles lid, lid + G, ...): the weights of the workgroup's output
//     slab (the three k-groups the 10 / 12 real channels use: 54 KB) and the bias are copied to LDS ONCE, the tap loop
//     has no barrier — one barrier per tile;
//   * reads the NCHW inputs directly: the halo tile of the next item is gathered plane by plane (18-pixel row
//     segments, coalesced) into registers while the current tile computes, then written to the other half of a double
//     buffer in the MFMA's operand layout ([halo pixel][channel], 20-float pixel pitch) — the Concatenate is an address
//     computation;
//   * DEFERS its epilogue like the body kernel: a finished tile's accumulators are copied to a second register set and
//     written out two 16-byte pieces per tap inside the NEXT tile's tap loop, so the 128 KB of stores per tile leave
//     under MFMAs instead of in a phase of their own (measured before: MFMA loop alone 97 us, stores alone 47 us, the
//     two in sequence 126 us — profiles/archive/r03_d_first_conv_ablation.log).
// The MFMA sequence per accumulator is exactly conv3x3_mfma_kernel's first-layer form (per tap: channels (j, 4 + j) for
// j = 0..3, then the pairs (8, 9)(, (10, 11)); taps in order), so every output bit is the same
// (tests/test_gpu_forward.py::test_first_layer_without_padding_mfmas_gives_the_same_bits pins it against the generic kernel).
#include "conv3x3_first_common.h"

namespace dsen2 {

namespace {

namespace first {
using firstk::THREADS; using firstk::NT;
constexpr int PSTR = 20;                            // floats per halo pixel in LDS: conflict-free ds_read_b128 over 16 pixels
constexpr int IN_FLOATS = kHaloPix * PSTR;          // 6480
constexpr int WCH = 16 * NT;                        // floats per tap of packed weights [g: 4][o: 128][j: 4]
constexpr int WCH3 = 12 * NT;                       // ... of which k-groups 0-2 (channels 0-11) are kept in LDS
constexpr int W_FLOATS = 9 * WCH;                   // one slab, all taps, in global memory
constexpr int W3_FLOATS = 9 * WCH3;                 // 13,824 floats = 54 KB in LDS
constexpr size_t LDS_BYTES = (size_t)(W3_FLOATS + 2 * IN_FLOATS + NT) * sizeof(float);      // 107,648 B
static_assert(LDS_BYTES <= 160 * 1024, "LDS budget");
// the gather's operand format (conv3x3_first_common.h): [halo pixel][channel], floats; a lane without an element does not write
struct Fmt {
  static constexpr int PITCH = PSTR;
  static __device__ __forceinline__ int none(int, int) { return -1; }
  static __device__ __forceinline__ bool has(int pk) { return pk >= 0; }
};
}  // namespace first

}  // namespace

// CREAL: real input channels (10 = 4 + 6 or 12 = 4 + 6 + 2; c10 + c20 + c60 must equal it).  EPI: kEpiRelu (p.out fp32
// NHWC).  p.in = x10, p.aux = x20, p.diag unused; x60 and the channel counts come in `f`.
// ABL (diagnostic builds, timing only): 1 no stores, 2 no MFMAs, 4 no input gather.
template <int CREAL, int COUT, int EPI, int ABL = 0>
__global__ __launch_bounds__(first::THREADS, 2) void conv3x3_first_kernel(const ConvParams p, const FirstInputs f, const int n_items) {
  using namespace first;
  constexpr int NS = COUT / NT;
  constexpr int MB = 2, PB = 2;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* const w_s = smem;                                          // [9][3][128][4]
  float* const in_s = smem + W3_FLOATS;                             // [2][324][PSTR]
  float* const bias_s = in_s + 2 * IN_FLOATS;                       // [128]

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wn = wave & 1;
  const int wp = wave >> 1;
  const int l31 = lane & 31;
  const int hsel = lane >> 5;

  // persistent schedule (conv3x3_items.h); a workgroup keeps ONE output slab: item = tile * NS + slab
  const int G = gridDim.x;
  const int lid = xcd_contiguous_id(blockIdx.x, G);
  if (lid >= n_items) return;
  const int slab = lid % NS;                                        // G is a multiple of NS (launch_persistent)
  const int my_items = (n_items - lid + G - 1) / G;
  const int tiles_per_img = p.tiles_x * p.tiles_y;
  const size_t plane = (size_t)p.h * p.w;

  // ---- weights of this slab: global -> LDS once (the packed layout is the LDS image) ----
  {
    const f32x4* src = reinterpret_cast<const f32x4*>(p.wpk + (size_t)slab * W_FLOATS);
    f32x4* dst = reinterpret_cast<f32x4*>(w_s);
    // per tap 3 x 128 pieces of 16 bytes (k-groups 0-2 of the packed [g: 4][o: 128][4])
    for (int i = tid; i < 9 * (WCH3 / 4); i += THREADS) {
      const int tap = i / (WCH3 / 4), q = i - tap * (WCH3 / 4);
      dst[i] = src[tap * (WCH / 4) + q];
    }
    if (tid < NT) bias_s[tid] = p.bias[slab * NT + tid];
  }

  // ---- gather geometry of one halo tile (conv3x3_first_common.h) ----
  using Ga = firstk::Gather<CREAL, Fmt>;
  constexpr int ROUNDS = Ga::ROUNDS;
  int pk[ROUNDS];
  Ga::setup(tid, pk, Ga::X10);
  Ga::setup(tid, pk, Ga::X20);
  if constexpr (Ga::R60 > 0) Ga::setup(tid, pk, Ga::X60);
  auto tile_of = [&](int item) -> Tile { return tile_at<NS>(item, tiles_per_img, p.tiles_x); };
  auto gather = [&](const Tile& t, float (&v)[ROUNDS]) __attribute__((always_inline)) {
    Ga::fetch(pk, v, Ga::X10, p.in, t, p, plane);
    Ga::fetch(pk, v, Ga::X20, p.aux, t, p, plane);
    if constexpr (Ga::R60 > 0) Ga::fetch(pk, v, Ga::X60, f.x60, t, p, plane);
  };
  auto scatter = [&](float* buf, const float (&v)[ROUNDS]) __attribute__((always_inline)) {
#pragma unroll
    for (int r = 0; r < ROUNDS; ++r)
      if (pk[r] >= 0) buf[pk[r] >> 13] = v[r];
  };

  // ---- per-lane operand addresses (floats): conv3x3_mfma_kernel<16, 16, ., 128, ., 8, 2, CREAL>'s ----
  // B (pixels): lane -> pixel (row l31 >> 4, column l31 & 15) of a 2 x 16 block; lanes 32-63 take channels + 4
  const int b_lane = ((l31 >> 4) * kHalo + (l31 & 15)) * PSTR + 4 * hsel + (2 * wp * PB) * kHalo * PSTR;
  // A (weights): [g = hsel][o][4]
  const int a_lane = (hsel * NT + wn * (32 * MB) + l31) * 4;

  // ---- prologue: first tile's input ----
  {
    float v[ROUNDS];
    gather(tile_of(lid), v);
    scatter(in_s, v);
  }
  __syncthreads();

  const size_t img_pix = plane;
  // one 16-byte piece of a finished tile: register quad g of accumulator (mb, pb) = channels 8g + 4*hsel .. +3 of one
  // pixel (conv3x3_mfma_kernel's epilogue); j = 8*pb + 4*mb + g
  auto store_piece = [&](int j, const f32x16 (&h)[MB][PB], const Tile& t, bool valid) __attribute__((always_inline)) {
    const int pb = j >> 3, mb = (j >> 2) & 1, g = j & 3;
    const int blk = wp * PB + pb;
    const int y = t.ty0 + 2 * blk + (l31 >> 4);
    const int x = t.tx0 + (l31 & 15);
    if (valid && y < p.h && x < p.w) {
      const size_t pix = (size_t)t.img * img_pix + (size_t)y * p.w + x;
      const int c0 = slab * NT + wn * (32 * MB) + mb * 32 + 8 * g + 4 * hsel;
      f32x4 v = {h[mb][pb][4 * g], h[mb][pb][4 * g + 1], h[mb][pb][4 * g + 2], h[mb][pb][4 * g + 3]};
      v += *reinterpret_cast<const f32x4*>(bias_s + c0 - slab * NT);
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.f);
      if constexpr ((ABL & 1) != 0) {
        asm volatile("" ::"v"(v));
      } else {
        static_assert(EPI == kEpiRelu, "fp32 NHWC output only: the plane-writing forms are conv3x3_first16.hip's");
        *reinterpret_cast<f32x4*>(p.out + pix * COUT + c0) = v;
      }
    }
  };

  // Rotated loop: iteration `it` first takes over tile it-1's accumulators (`held`), then computes tile `it` while
  // held's sixteen pieces leave two per tap; one extra iteration writes the last tile out at once.
  f32x16 acc[MB][PB], held[MB][PB];
#pragma unroll
  for (int mb = 0; mb < MB; ++mb)
#pragma unroll
    for (int pb = 0; pb < PB; ++pb)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[mb][pb][e] = 0.f;
  for (int it = 0; it <= my_items; ++it) {
    const Tile tprev = tile_of(it > 0 ? lid + (it - 1) * G : lid);
    const bool vprev = it > 0;
#pragma unroll
    for (int mb = 0; mb < MB; ++mb)
#pragma unroll
      for (int pb = 0; pb < PB; ++pb) held[mb][pb] = acc[mb][pb];
    if (it == my_items) {
#pragma unroll
      for (int j = 0; j < 16; ++j) store_piece(j, held, tprev, vprev);
      break;
    }
    const int item = lid + it * G;
    const float* const ib = in_s + (it & 1) * IN_FLOATS;
    float* const ib_next = in_s + ((it + 1) & 1) * IN_FLOATS;
    // the next tile's input: its loads fly under this tile's MFMAs (past the last item: this tile again, never read)
    float nv[ROUNDS];
    if constexpr (!(ABL & 4)) gather(tile_of(it + 1 < my_items ? item + G : item), nv);
    else for (int r = 0; r < ROUNDS; ++r) nv[r] = 1.f;

#pragma unroll
    for (int mb = 0; mb < MB; ++mb)
#pragma unroll
      for (int pb = 0; pb < PB; ++pb)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[mb][pb][e] = 0.f;

#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      const int dy = tap / 3, dx = tap - dy * 3;
      const float* const bp = ib + b_lane + (dy * kHalo + dx) * PSTR;
      const float* const ap = w_s + tap * WCH3 + a_lane;
      if constexpr (!(ABL & 2)) {
        // channels 0-7: MFMA j pairs channel j (lanes 0-31) with channel 4 + j (lanes 32-63)
        f32x4 a[MB], b[PB];
#pragma unroll
        for (int mb = 0; mb < MB; ++mb) a[mb] = *reinterpret_cast<const f32x4*>(ap + (mb * 32) * 4);
#pragma unroll
        for (int pb = 0; pb < PB; ++pb) b[pb] = *reinterpret_cast<const f32x4*>(bp + pb * 2 * kHalo * PSTR);
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int mb = 0; mb < MB; ++mb)
#pragma unroll
            for (int pb = 0; pb < PB; ++pb)
              acc[mb][pb] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[mb][j], b[pb][j], acc[mb][pb], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
        // channels 8 .. CREAL-1: lanes 0-31 supply channel 8 + 2m, lanes 32-63 channel 9 + 2m (both from k-group 2)
#pragma unroll
        for (int m = 0; m < (CREAL - 8) / 2; ++m) {
          float a1[MB], b1[PB];
#pragma unroll
          for (int mb = 0; mb < MB; ++mb) a1[mb] = ap[(2 * NT + mb * 32) * 4 - hsel * NT * 4 + 2 * m + hsel];
#pragma unroll
          for (int pb = 0; pb < PB; ++pb) b1[pb] = bp[pb * 2 * kHalo * PSTR + 8 - 4 * hsel + 2 * m + hsel];
#pragma unroll
          for (int mb = 0; mb < MB; ++mb)
#pragma unroll
            for (int pb = 0; pb < PB; ++pb)
              acc[mb][pb] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[mb], b1[pb], acc[mb][pb], 0, 0, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
      // two pieces of the previous tile, issued behind this tap's MFMAs (a version that also read the operand fragments one
      // tap ahead and put the pieces between MFMA groups was slower: 125 vs 117 us)
      if (tap < 8) {
        store_piece(2 * tap, held, tprev, vprev);
        store_piece(2 * tap + 1, held, tprev, vprev);
        __builtin_amdgcn_sched_barrier(0);
      }
    }

    // the next tile's halo into the other buffer (every wave read it for the last time one barrier ago)
    scatter(ib_next, nv);
    __syncthreads();
  }
}

template <int CREAL, int COUT, int EPI, int ABL = 0>
static hipError_t launch_first_one(const ConvParams& p, const FirstInputs& f, hipStream_t stream) {
  return firstk::launch_first_kernel<conv3x3_first_kernel<CREAL, COUT, EPI, ABL>, COUT>(first::LDS_BYTES, p, f, stream);
}

// p.in = x10, p.aux = x20 (NCHW), p.wpk / p.bias: weights packed for the tile kernel (KC 16, NT 128); p.out NHWC fp32
// (kEpiRelu only: the output is written through pointers, so only the inputs bound the image size).  hipErrorNotSupported:
// see check_first_launch.
hipError_t launch_conv3x3_first(const ConvParams& p, const FirstInputs& f, int cout, int epilogue, hipStream_t stream, int ablate) {
  const int creal = f.c10 + f.c20 + f.c60;
  const hipError_t e = firstk::check_first_launch(p, f, 0, false);
  if (e != hipSuccess) return e;
  if (epilogue != kEpiRelu) return hipErrorInvalidValue;      // the (hi, lo) / (hi | xl, lo16) plane forms: conv3x3_first16.hip
#ifdef DSEN2_DIAG
  if (creal == 10 && cout == 128) {
#define DSEN2_ABL(M) \
  if (ablate == M) return launch_first_one<10, 128, kEpiRelu, M>(p, f, stream);
    DSEN2_ABL(1) DSEN2_ABL(2) DSEN2_ABL(4) DSEN2_ABL(3) DSEN2_ABL(5) DSEN2_ABL(7) DSEN2_ABL(6)
#undef DSEN2_ABL
  }
#endif
#define DSEN2_CASE(CR, CO) \
  if (creal == CR && cout == CO) return launch_first_one<CR, CO, kEpiRelu>(p, f, stream);
  DSEN2_CASE(10, 128) DSEN2_CASE(12, 128) DSEN2_CASE(10, 256) DSEN2_CASE(12, 256)
#undef DSEN2_CASE
  return hipErrorNotSupported;
}

}  // namespace dsen2
