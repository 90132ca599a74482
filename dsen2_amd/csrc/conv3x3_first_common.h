// conv3x3_first_common.h — the skeleton the two first-convolution kernels share (conv3x3_first.hip: exact fp32;
// conv3x3_first16.hip: bf16 operands): the gather of a halo tile from the two or three NCHW inputs, the launcher of one
// instantiation (a workgroup keeps one output slab) and the entry functions' checks.  The MFMA loops, the scatter into LDS and
// the stores are each file's own.
#pragma once
#include "conv3x3_bf16_common.h"

namespace dsen2 {
namespace firstk {

constexpr int THREADS = 512;                        // 8 waves: 2 (64-channel halves) x 4 (pixel quarters: 4 rows x 16)
constexpr int NT = 128;                             // output channels per item (slab)

// Gather geometry of one halo tile (the same for every tile).  Per input tensor T (10 m: 4 channels, 20 m: 6, 60 m: CREAL - 10)
// the CT x 324 values of a halo tile are fetched in rounds of 512 threads, channel outer / halo pixel inner: consecutive lanes
// read consecutive pixels of an 18-pixel row segment of ONE plane, through a per-image buffer descriptor (an out-of-range
// offset returns the zero padding; the Concatenate is an address computation).  One register per round:
//   pk = hx | hy << 5 | (channel inside its tensor) << 10 | (LDS element index of the value) << 13
// What the operand format decides is FMT's:
//   FMT::PITCH           LDS elements per halo pixel: (halo pixel hp, channel slot ch of the concatenated input) is element
//                        hp * PITCH + ch
//   FMT::none(hp, c)     pk of a lane without an element in this round
//   FMT::has(pk)         whether pk carries an element (a lane without one fetches the out-of-range offset: zero)
template <int CREAL, class FMT>
struct Gather {
  struct Input { int r0, rounds, ct, cbase; };      // first round, rounds, channels, first channel slot of one input tensor
  static constexpr int C10 = 4, C20 = 6, C60 = CREAL - 10;
  static constexpr int R10 = (C10 * kHaloPix + THREADS - 1) / THREADS, R20 = (C20 * kHaloPix + THREADS - 1) / THREADS,
                       R60 = (C60 * kHaloPix + THREADS - 1) / THREADS;
  static constexpr int ROUNDS = R10 + R20 + R60;                    // 7 (10 channels) or 9 (12)
  static constexpr Input X10{0, R10, C10, 0}, X20{R10, R20, C20, C10}, X60{R10 + R20, R60, C60, C10 + C20};
  static_assert(CREAL % 2 == 0 && CREAL > 8 && CREAL <= 16, "first-layer form");

  // pk of the rounds of one input tensor.  (One call per tensor from the kernel, and `tid` by reference: with one function over
  // all tensors, or the thread id by value, hipcc generates different kernels — profiles/conv_kernel_skeleton_refactor.md.)
  static __device__ __forceinline__ void setup(const int& tid, int (&pk)[ROUNDS], const Input in) {
#pragma unroll
    for (int r = 0; r < in.rounds; ++r) {
      const int e = r * THREADS + tid;
      const int c = e / kHaloPix, hp = e - c * kHaloPix;
      const int hy = hp / kHalo, hx = hp - hy * kHalo;
      const bool have = e < in.ct * kHaloPix;
      pk[in.r0 + r] = have ? hx | hy << 5 | c << 10 | (hp * FMT::PITCH + in.cbase + c) << 13 : FMT::none(hp, c);
    }
  }

  // the halo of tile t in input tensor x (`in`'s) into v; plane = p.h * p.w.  Every offset inside one image's tensor is below
  // 2^31 (check_first_launch)
  static __device__ __forceinline__ void fetch(const int (&pk)[ROUNDS], float (&v)[ROUNDS], const Input in, const float* x,
                                               const Tile& t, const ConvParams& p, const size_t& plane) {
    const auto rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(x) + (size_t)t.img * in.ct * plane, 0,
                                                        (unsigned)(in.ct * plane * 4), 0x00020000);
#pragma unroll
    for (int r = 0; r < in.rounds; ++r) {
      int k = pk[in.r0 + r];
      asm volatile("" : "+v"(k));      // derive the addresses here, every tile: hoisted out of the item loop they are spilled
      const int gy = t.ty0 - 1 + ((k >> 5) & 31), gx = t.tx0 - 1 + (k & 31);
      const bool inb = FMT::has(k) && (unsigned)gy < (unsigned)p.h && (unsigned)gx < (unsigned)p.w;
      const unsigned voff = inb ? (unsigned)((((k >> 10) & 7) * (int)plane + gy * p.w + gx) * 4) : 0x80000000u;
      v[in.r0 + r] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsrc, (int)voff, 0, 0));
    }
  }
};

// ---- host side ----
// one instantiation Kern(ConvParams, FirstInputs, int n_items) with COUT / NT slabs
template <auto Kern, int COUT>
hipError_t launch_first_kernel(size_t lds_bytes, const ConvParams& p, const FirstInputs& f, hipStream_t stream) {
  constexpr int NS = COUT / NT;
  return launch_persistent<Kern>(lds_bytes, THREADS, (long long)p.n * p.tiles_x * p.tiles_y * NS, NS, 0, stream, p, f);
}

// What both entry functions check.  hipErrorNotSupported: band groups other than Sentinel-2's 4 + 6 (+ 2) (the generic
// pack_inputs + conv3x3_mfma path handles those), or an image whose per-image buffer descriptors would not keep 0x80000000 out
// of range — the kernels drop padding loads and masked stores there, so EVERY descriptor they build must span less than 2^31
// bytes: the 20 m input (6 fp32 planes, the largest input) and the output tensors (`out_px_bytes` per pixel and image in the
// larger of them; 0 = written through pointers).  Every caller inside the library has passed check_shape (capi_internal.h:
// h * w * F < 2^29, i.e. at most 4 F bytes per pixel below 2^31) before it gets here, so this refuses nothing the C ABI accepts.
inline hipError_t check_first_launch(const ConvParams& p, const FirstInputs& f, size_t out_px_bytes, bool two_outputs) {
  if (f.c10 != 4 || f.c20 != 6 || (f.c60 != 0 && f.c60 != 2)) return hipErrorNotSupported;
  const size_t px_bytes = out_px_bytes > 6 * 4 ? out_px_bytes : 6 * 4;
  if ((size_t)p.h * p.w * px_bytes >= ((size_t)1 << 31)) return hipErrorNotSupported;
  if (!p.in || !p.aux || (f.c60 > 0 && !f.x60) || !p.out || (two_outputs && !p.out2) || !p.wpk || !p.bias) return hipErrorInvalidValue;
  return hipSuccess;
}

}  // namespace firstk
}  // namespace dsen2
