// conv3x3_dma.h — the LDS-DMA staging of conv3x3_body32.hip (fp32 body convolution; the bf16 kernel,
// conv3x3_body16w.hip, carries its own wide-tile version of the same scheme).
//
// Byte geometry (identical for both: a step is (tap, 128 bytes of input channels per pixel)):
//   input chunk  : [channel group q: 8][pixel slot: 336][16 B]  = 43,008 B, double buffered; slots 0..323 = the
//                  18x18 halo tile in row-major order, group q = bytes 16q..16q+15 of the pixel's 128-byte chunk
//   weight chunk : [k-group: 8][row: 128][16 B] = 16 KiB, verbatim the packed layout of dsen2_internal.h; 4-slot ring
//   bias         : [COUT] floats
//
// Movement: `buffer_load_dwordx4 ... offen lds` — 1 KiB per wave instruction, LDS address = M0 + 16*lane, a lane whose
// offset is out of the descriptor's range writes zeros (= the convolution's zero padding), an EXEC-masked lane
// writes nothing.  Issued from inline asm: through the builtin hipcc tracks the DMA in its waitcnt model and turns
// every counted lgkmcnt(N) of the fragment pipeline into lgkmcnt(0).  hipcc therefore knows neither about these
// vector-memory operations nor about the LDS they write (M0 is saved and restored inside every asm statement), and
// the kernels spell the synchronisation out:
//   * vmcnt retires in ISSUE ORDER, all vector-memory operations of a wave together (loads, stores, DMAs);
//   * weight chunk c is issued in step c-3 into ring slot c%4 (last read in step c-4, which ended with a barrier),
//     retired by every wave's `s_waitcnt vmcnt(N)` at the END of step c-2 — N = a lower bound of what that wave
//     issued after it — followed by that step's barrier, and first read by the fragment prefetch at the end of c-1;
//   * the six rounds of an input chunk are issued in taps 0-5 of the previous chunk's steps (wave q moves channel
//     group q of 64 halo pixels per round) and are older than the weight DMA awaited at the end of tap 6; the chunk
//     is first read at the end of tap 8;
//   * a wait that assumes FEWER younger operations than there are is stricter, never weaker — so is every wait
//     hipcc inserts for the loads it does track (it counts none of the DMAs);
//   * a workgroup must not end with a DMA in flight (its LDS may already belong to the next one): vmcnt(0) at exit.
//
// Role::Issuer (Body32Form::DeferAsym): waves 0-3 move everything, waves 4-7 never touch a Stage and run a copy of the
// item loop without a DMA statement, set_stage_item or hand-counted wait.  Same chunks, same steps, same slots — only who
// issues changes, so every rule above holds with these counts:
//   * a weight chunk is 16 wave instructions = FOUR per issuing wave (bytes 1024*wave + 4096*k, k = 0..3, of the chunk:
//     N_W = 4), in one asm statement with one M0 save and restore;
//   * an input round is TWO instructions per issuing wave: wave q moves channel groups q and q + 4 of the round's 64 halo
//     pixels (the second one 64 bytes further into the pixel — through soffset, which the range check ignores, so an
//     out-of-range lane stays out of range and writes the zero padding — and 4*QS*16 bytes further into LDS); the 16-lane
//     tail round keeps its EXEC mask around both;
//   * the step-end wait of an issuing wave retires the weight chunk of the PREVIOUS step: younger than it are at least this
//     step's input round (2, taps 0-5) and weight chunk (4), so vmcnt(6) in taps 0-5 and vmcnt(4) in taps 6-8.  Whatever
//     else the wave issued in between (two residual quads, two stores of the deferred epilogue) only makes the wait
//     stricter.  The six rounds of an input chunk are still older than the weight chunk of tap 5, retired at the end of
//     tap 6;
//   * waves 4-7 take the data from the barrier that follows the issuers' wait (a DMA that has left vmcnt has written its
//     LDS); their own vmcnt queue holds only their epilogue's loads and stores, which hipcc counts exactly;
//   * in flight per issuing wave: a step issues at most 2 residual loads + 2 + 4 DMAs + 2 stores = 10 and ends with at most
//     6 + 2 outstanding, so the peak is below 20; the prologue (12 input + 12 weight DMAs + the bias load) reaches 25 and
//     the last item's epilogue 32 on top of at most 8 — all far below the 6-bit field's 63;
//   * LDS addresses: an input DMA ends at most at (7*QS + 64*4)*16 + 1024 = 42,752 <= IN_BYTES (tail round: (7*QS + 320)*16
//     + 256 = IN_BYTES exactly), a weight DMA at 1024*3 + 4096*3 + 1024 = WCH*4 inside its ring slot;
//   * every wave still ends with vmcnt(0).
#pragma once
#include "conv3x3_items.h"

namespace dsen2 {
namespace dma {

constexpr int KC = 32;                      // 32-bit words per pixel and step (32 fp32 or 64 bf16 channels)
constexpr int NT = 128;                     // output channels per item
constexpr int THREADS = 512;                // 8 waves
constexpr int QS = 336;                     // pixel slots per channel-group row (>= 324 halo pixels, = 0 mod 16)
constexpr int IN_BYTES = 8 * QS * 16;       // one input chunk buffer
constexpr int IN_BLOCKS = 6;                // DMA rounds per chunk: 64 pixels each (the last one 16: slots 320-335)
constexpr int WCH = KC * NT;                // words per weight chunk (16 KiB)
constexpr int NWBUF = 4;
constexpr size_t LDS_BYTES = (size_t)2 * IN_BYTES + (size_t)NWBUF * WCH * 4 + 256 * 4;
static_assert(QS >= kHaloPix && QS % 16 == 0 && 64 * (IN_BLOCKS - 1) + 16 == QS, "input chunk geometry");
static_assert(LDS_BYTES <= 160 * 1024, "LDS budget");

template <int N>
__device__ __forceinline__ void wait_vmcnt() {
  static_assert(N >= 0 && N <= 63, "vmcnt is a 6-bit field");
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

__device__ __forceinline__ unsigned lds_address(const float* p) {
  return (unsigned)(size_t)(__attribute__((address_space(3))) const float*)p;
}

// Who issues the DMAs: All = every one of the eight waves its share (wave q: channel group q, 2 KiB of a weight chunk);
// Issuer = waves 0-3 everything (the rules above), waves 4-7 never call into the Stage.
enum class Role { All, Issuer };

// Per-thread state of the two streams.  CINW = 32-bit words per input pixel; NS = output slabs per tile.
// LAZY_VOFF: do not keep the six per-lane input offsets in registers across the item but recompute the one a round
// needs from the staged tile's origin (a dozen VALU operations per step; for kernels that are out of VGPRs).
template <int CINW, int NS, bool LAZY_VOFF = false, Role ROLE = Role::All>
struct Stage {
  static constexpr int N_W = ROLE == Role::Issuer ? 4 : 2;      // wave instructions per weight chunk and issuing wave
  static constexpr int N_IN = ROLE == Role::Issuer ? 2 : 1;     // ... per input round
  static constexpr int NCC = CINW / KC;
  static constexpr int NCHUNK = NCC * 9;

  const float* in;                  // NHWC activations, CINW words per pixel
  int h, w, tiles_x, tiles_per_img;
  size_t img_pix;
  int lane, wave, lid, G, n_items;
  unsigned lds_in, lds_w;
  unsigned in_voff[LAZY_VOFF ? 1 : IN_BLOCKS];   // byte offset of (halo pixel 64*b + lane, group `wave`) inside the image; out of range = zero
  int st_y0, st_x0;                 // origin of the staged tile (LAZY_VOFF)
  __amdgpu_buffer_rsrc_t in_rsrc, w_rsrc;
  unsigned w_voff;
  int wl_item, wl_chunk, st_slot;   // item / chunk of the next weight DMA, ring slot it goes to

  __device__ __forceinline__ void init(const ConvParams& p, const float* in_s, const float* w_s, int lane_, int wave_,
                                       int lid_, int G_, int n_items_) {
    in = p.in; h = p.h; w = p.w; tiles_x = p.tiles_x; tiles_per_img = p.tiles_x * p.tiles_y;
    img_pix = (size_t)p.h * p.w;
    lane = lane_; wave = wave_; lid = lid_; G = G_; n_items = n_items_;
    lds_in = lds_address(in_s);
    lds_w = lds_address(w_s);
    in_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.in), 0, 0, 0x00020000);
    w_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.wpk), 0, (unsigned)(NS * NCHUNK * WCH * 4), 0x00020000);
    w_voff = lane * 16;
    wl_item = lid; wl_chunk = 0; st_slot = 0;
    st_y0 = st_x0 = 0;
  }

  __device__ __forceinline__ unsigned voff_of(int b, int ty0, int tx0) const {
    const int hp = 64 * b + lane;
    const int hy = hp / kHalo, hx = hp - hy * kHalo;
    const int gy = ty0 - 1 + hy, gx = tx0 - 1 + hx;
    const bool inb = hp < kHaloPix && (unsigned)gy < (unsigned)h && (unsigned)gx < (unsigned)w;
    return inb ? (unsigned)(((gy * w + gx) * CINW + wave * 4) * 4) : 0x80000000u;
  }

  // the tile whose input the following issue_in() calls fetch
  __device__ __forceinline__ void set_stage_item(int item) {
    const Tile t = tile_at<NS>(item, tiles_per_img, tiles_x);
    in_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(in) + (size_t)t.img * img_pix * CINW, 0,
                                                (unsigned)(img_pix * CINW * 4), 0x00020000);
    if constexpr (LAZY_VOFF) {
      st_y0 = t.ty0;
      st_x0 = t.tx0;
    } else {
#pragma unroll
      for (int b = 0; b < IN_BLOCKS; ++b) in_voff[b] = voff_of(b, t.ty0, t.tx0);
    }
  }

  // round b of input chunk cc into buffer `buf` (N_IN wave instructions per issuing wave)
  __device__ __forceinline__ void issue_in(int buf, int b, int cc) {
    const unsigned m0v = lds_in + buf * IN_BYTES + (wave * QS + 64 * b) * 16;
    const unsigned so = cc * (KC * 4);
    const unsigned voff = LAZY_VOFF ? voff_of(b, st_y0, st_x0) : in_voff[LAZY_VOFF ? 0 : b];
    if constexpr (ROLE == Role::Issuer) {
      // channel groups `wave` and `wave + 4`: 64 bytes further into the pixel, 4 group rows further into LDS
      const unsigned m1v = m0v + 4 * QS * 16, so1 = so + 64;
      unsigned saved_m0;
      if (b < IN_BLOCKS - 1) {
        asm volatile("s_mov_b32 %0, m0\n\t"
                     "s_mov_b32 m0, %1\n\ts_nop 0\n\tbuffer_load_dwordx4 %3, %4, %5 offen lds\n\t"
                     "s_mov_b32 m0, %2\n\ts_nop 0\n\tbuffer_load_dwordx4 %3, %4, %6 offen lds\n\t"
                     "s_mov_b32 m0, %0"
                     : "=&s"(saved_m0) : "s"(m0v), "s"(m1v), "v"(voff), "s"(in_rsrc), "s"(so), "s"(so1) : "memory");
      } else if (lane < 16) {
        asm volatile("s_mov_b32 %0, m0\n\t"
                     "s_mov_b32 m0, %1\n\ts_nop 0\n\tbuffer_load_dwordx4 %3, %4, %5 offen lds\n\t"
                     "s_mov_b32 m0, %2\n\ts_nop 0\n\tbuffer_load_dwordx4 %3, %4, %6 offen lds\n\t"
                     "s_mov_b32 m0, %0"
                     : "=&s"(saved_m0) : "s"(m0v), "s"(m1v), "v"(voff), "s"(in_rsrc), "s"(so), "s"(so1) : "memory");
      }
      return;
    }
    // M0 is saved and restored inside the statement: hipcc reserves M0 and rejects it in a clobber list, so the
    // compiler's own uses of M0 (none today) must never see the DMA's value
    unsigned saved_m0;
    if (b < IN_BLOCKS - 1) {
      asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %1\n\ts_nop 0\n\tbuffer_load_dwordx4 %2, %3, %4 offen lds\n\ts_mov_b32 m0, %0"
                   : "=&s"(saved_m0) : "s"(m0v), "v"(voff), "s"(in_rsrc), "s"(so) : "memory");
    } else if (lane < 16) {          // slots 320-335 only: the next group's row starts at 336
      asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %1\n\ts_nop 0\n\tbuffer_load_dwordx4 %2, %3, %4 offen lds\n\ts_mov_b32 m0, %0"
                   : "=&s"(saved_m0) : "s"(m0v), "v"(voff), "s"(in_rsrc), "s"(so) : "memory");
    }
  }

  // the next weight chunk of the stream (16 wave instructions of 1 KiB, N_W per issuing wave) into the next ring slot;
  // the stream runs over item boundaries and, past the last item, wraps to this workgroup's first one (harmless)
  __device__ __forceinline__ void issue_w() {
    const unsigned so = (unsigned)(((wl_item % NS) * NCHUNK + wl_chunk) * (WCH * 4) + wave * 1024);
    const unsigned l0 = lds_w + st_slot * (WCH * 4) + wave * 1024;
    unsigned saved_m0;
    if constexpr (ROLE == Role::Issuer)
      asm volatile(
          "s_mov_b32 %0, m0\n\t"
          "s_mov_b32 m0, %1\n\ts_nop 0\n\tbuffer_load_dwordx4 %5, %6, %7 offen lds\n\t"
          "s_mov_b32 m0, %2\n\ts_nop 0\n\tbuffer_load_dwordx4 %5, %6, %8 offen lds\n\t"
          "s_mov_b32 m0, %3\n\ts_nop 0\n\tbuffer_load_dwordx4 %5, %6, %9 offen lds\n\t"
          "s_mov_b32 m0, %4\n\ts_nop 0\n\tbuffer_load_dwordx4 %5, %6, %10 offen lds\n\t"
          "s_mov_b32 m0, %0"
          : "=&s"(saved_m0)
          : "s"(l0), "s"(l0 + 4096u), "s"(l0 + 8192u), "s"(l0 + 12288u), "v"(w_voff), "s"(w_rsrc), "s"(so), "s"(so + 4096u),
            "s"(so + 8192u), "s"(so + 12288u)
          : "memory");
    else
    asm volatile(
        "s_mov_b32 %0, m0\n\t"
        "s_mov_b32 m0, %1\n\ts_nop 0\n\tbuffer_load_dwordx4 %3, %4, %5 offen lds\n\t"
        "s_mov_b32 m0, %2\n\ts_nop 0\n\tbuffer_load_dwordx4 %3, %4, %6 offen lds\n\t"
        "s_mov_b32 m0, %0"
        : "=&s"(saved_m0) : "s"(l0), "s"(l0 + 8192u), "v"(w_voff), "s"(w_rsrc), "s"(so), "s"(so + 8192u)
        : "memory");
    if (++wl_chunk == NCHUNK) {
      wl_chunk = 0;
      wl_item = wl_item + G < n_items ? wl_item + G : lid;
    }
    st_slot = st_slot == NWBUF - 1 ? 0 : st_slot + 1;
  }
};

}  // namespace dma
}  // namespace dsen2
