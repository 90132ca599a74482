// conv3x3_body32.hip — fp32 F->F 3x3 'same' convolution (F = 128 or 256): v_mfma_f32_32x32x2_f32 fed by LDS-DMA.
//
// The fp32 sibling of conv3x3_body16w.hip (the DMA streams and their synchronisation rules: conv3x3_dma.h; the
// byte geometry is identical: a step is (tap, 32 channels) = 128 B per pixel and a 16 KiB weight chunk):
//
//   * weight chunks and input chunks go global -> LDS by `buffer_load_dwordx4 ... lds` issued from inline asm and
//     retired by hand-counted `s_waitcnt vmcnt(N)` + the step barrier: no staging VGPRs, ds_writes or selects
//     (out-of-range lanes write the zero padding);
//   * the input chunk lives in LDS as [channel group q: 8][pixel slot: 336][16 B]; a wave's 32-pixel block is rows
//     (R, R + 8) x 16 columns of the tile — 8 halo rows = 144 slots = 0 mod 16 apart — so every ds_read_b128 of the
//     loop is bank-conflict free (an adjacent-row 2x16 block is 2-way);
//   * the WEIGHTS are the MFMA's A operand: D[row = output channel][col = pixel].  A lane owns one pixel and, per
//     accumulator, channels (r & 3) + 8*(r >> 2) + 4*(lane >> 5): register quad g = 16 contiguous bytes of NHWC,
//     the two half-waves together 32 contiguous bytes per pixel.  The epilogue is 16-byte loads/stores with no
//     cross-lane transposes (the X-as-A form needs 64 dword stores or 256 DPP moves per lane and item);
//   * default (DEFER): the finished accumulators are copied to a second register set — the DMA staging freed the
//     registers — and written out in 16 pieces inside the next item's first 8 steps, residual quads fetched one
//     step ahead; without DEFER the residual tile is fetched under the item's last step (PRE) and the epilogue's
//     stores drain under the next item's first step (3.5 us);
//   * waves 4-7 issue their DMAs half a step after waves 0-3 (STG 1), or waves 0-3 issue every DMA and waves 4-7 none
//     (STG 2 and up, Body32Form::DeferAsym: dma::Role::Issuer in conv3x3_dma.h).
//
// Per wave: 64 channels x 64 pixels = 2 x 2 accumulators of 32x32; one step = 4 k-steps of 16 MFMAs and
// 4 ds_read_b128.  Same arithmetic order per output element as the one-tile-per-workgroup kernel of conv3x3_mfma.hip:
// results are bit-identical (tests/test_gpu_conv.py).
#include <type_traits>

#include "conv3x3_dma.h"

namespace dsen2 {

namespace {

using dma::KC; using dma::NT; using dma::THREADS; using dma::QS; using dma::IN_BYTES; using dma::IN_BLOCKS;
using dma::WCH; using dma::NWBUF; using dma::LDS_BYTES; using dma::wait_vmcnt;
constexpr int KSTEPS = 4;                   // 8 channels per k-step: one ds_read_b128 feeds 4 MFMAs (k = 2 each)
constexpr int PB = 2, MB = 2;               // 32-pixel blocks x 32-channel blocks per wave
static_assert((8 * kHalo) % 16 == 0, "rows R and R+8 of a pixel block sit on the same banks");

}  // namespace

// ABL: timing-only ablation mask (1 no stores, 2 no residual loads, 4 no weight stream, 8 no input stream,
// 16 no barriers).  PRE: 32-channel blocks (0-2) whose residual values are fetched under the item's last step.
// STG: 1 = waves 4-7 issue their DMAs half a step after waves 0-3 (two copies of the item loop); 2 and up = waves 0-3 issue
// every DMA, waves 4-7 run a copy of the item loop with no DMA statement and no hand-counted wait: STG - 2 = the k-step
// (0-3) at which the issuers issue, + 4 for waves 4-7 at s_setprio 1 (the product's is 4: half a step into the step, measured
// in profiles/body32_asym.md; the others exist in the diagnostic build only).
// DEFER: the epilogue of item i is cut into 16 pieces (one 16-byte register quad each) that run inside the first
// 8 steps of item i+1, out of a copy of the accumulators: loads and stores trickle out under MFMAs instead of in a
// burst between items (PRE is then unused: a piece's residual quad is fetched one step before the piece runs).
template <int CIN, int COUT, int EPI, int ABL, int PRE, int STG, bool DEFER>
__global__ __launch_bounds__(THREADS, 2) void conv3x3_body32_kernel(const ConvParams p, const int n_items) {
  constexpr int NCC = CIN / KC;
  constexpr int NS = COUT / NT;
  static_assert(NCC % 2 == 0, "input double buffer parity");
  constexpr bool ASYM = STG >= 2;
  using Stage = dma::Stage<CIN, NS, false, ASYM ? dma::Role::Issuer : dma::Role::All>;
  constexpr int N_W = (ABL & 4) ? 0 : Stage::N_W;          // weight DMAs per issuing wave and step

  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* const in_s = smem;                            // [2][8][QS][4 words]
  float* const w_s = smem + 2 * IN_BYTES / 4;          // [4][8 k-groups][128 rows][4 words]
  float* const bias_s = w_s + NWBUF * WCH;             // [COUT]

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wn = wave & 1;                 // 64-channel half of the slab
  const int wp = wave >> 1;                // rows 2*wp, 2*wp + 1 and the same + 8
  const int l31 = lane & 31;
  const int hsel = lane >> 5;
  const int rh = l31 >> 4, c16 = l31 & 15;

  // persistent schedule (conv3x3_items.h): items lid, lid + G, ...
  const int G = gridDim.x;
  const int lid = xcd_contiguous_id(blockIdx.x, G);
  if (lid >= n_items) return;
  const int my_items = (n_items - lid + G - 1) / G;
  const int tiles_per_img = p.tiles_x * p.tiles_y;
  const size_t img_pix = (size_t)p.h * p.w;

  // ---- the two DMA streams (conv3x3_dma.h) ----
  Stage st;
  st.init(p, in_s, w_s, lane, wave, lid, G, n_items);

  // ---- per-lane operand addresses (words) ----
  // B operand (pixels): lane -> pixel (row 2*wp + pb + 8*rh, column c16), channel group 2*s + hsel of the chunk
  // A operand (weights): [k-group = 2*s + hsel][row = wn*64 + 32*mb + l31][4 words]
  const int x_lane = (hsel * QS + (2 * wp + 8 * rh) * kHalo + c16) * 4;
  const int w_lane = (hsel * NT + wn * 64 + l31) * 4;

  // ---- prologue: first item's input chunk 0, weight chunks 0-2 ----
  if (!ASYM || wave < 4) {
    st.set_stage_item(lid);
    if constexpr (!(ABL & 8)) {
#pragma unroll
      for (int b = 0; b < IN_BLOCKS; ++b) st.issue_in(0, b, 0);
    }
    if constexpr (!(ABL & 4)) {
      st.issue_w();
      st.issue_w();
      st.issue_w();
    }
  }
  if (tid < COUT) bias_s[tid] = p.bias[tid];
  wait_vmcnt<0>();
  __syncthreads();

  f32x4 w_cur[MB], x_cur[PB], w_nxt[MB], x_nxt[PB];
  int mf_slot = 0;
  auto read_frags = [&](f32x4 (&wf)[MB], f32x4 (&xf)[PB], const float* ib, const float* wb, int tap, int s) {
    const int dy = tap / 3, dx = tap - dy * 3;
    const float* wp_ = wb + w_lane + (2 * s * NT) * 4;
    const float* xp_ = ib + x_lane + (2 * s * QS + dy * kHalo + dx) * 4;
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) wf[mb] = *reinterpret_cast<const f32x4*>(wp_ + mb * 32 * 4);
#pragma unroll
    for (int pb = 0; pb < PB; ++pb) xf[pb] = *reinterpret_cast<const f32x4*>(xp_ + pb * kHalo * 4);
  };
  read_frags(w_cur, x_cur, in_s, w_s, 0, 0);

  // geometry of one item's output: its image, the lane's element offset (row 2*wp + 8*rh, column c16, channel
  // base of the lane), validity of the lane's column
  struct OutGeom { int img; unsigned lane_eoff; int ey; bool col_ok; int chb; };
  auto out_geom = [&](int item, bool valid) -> OutGeom {
    const Tile t = tile_at<NS>(item, tiles_per_img, p.tiles_x);
    const int chb = t.slab * NT + wn * 64 + 4 * hsel;
    const int ex = t.tx0 + c16, ey = t.ty0 + 2 * wp + 8 * rh;
    return OutGeom{t.img, (unsigned)((ey * p.w + ex) * COUT + chb), ey, valid && ex < p.w, chb};
  };
  auto aux_desc = [&](int img) {
    return __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(p.aux) + (EPI == kEpiResidual ? (size_t)img * img_pix * COUT : 0), 0,
        EPI == kEpiResidual ? (unsigned)(img_pix * COUT * 4) : 0, 0x00020000);
  };
  // byte offset of register quad g of accumulator (mb, pb); out of range for pixels outside a ragged tile
  auto byte_off = [&](const OutGeom& g_, int mb, int pb, int g) -> unsigned {
    return g_.col_ok && g_.ey + pb < p.h ? (g_.lane_eoff + (unsigned)(pb * p.w * COUT + mb * 32 + 8 * g)) * 4u : 0x80000000u;
  };

  // ISSUE: this copy of the item loop issues DMAs (and waits for them); without it the copy holds no DMA statement
  auto run = [&](auto mid_c, auto issue_c) {
  constexpr int MIDS = decltype(mid_c)::value;
  constexpr bool ISSUE = decltype(issue_c)::value;
  f32x16 acc[MB][PB];
#pragma unroll
  for (int mb = 0; mb < MB; ++mb)
#pragma unroll
    for (int pb = 0; pb < PB; ++pb)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[mb][pb][e] = 0.f;
  // residual values of the first PRE 32-channel blocks, fetched at the head of an item's last step
  constexpr int kPre = EPI == kEpiResidual && !(ABL & 2) && !DEFER ? PRE : 0;
  f32x4 resv[kPre ? kPre : 1][PB][4];
#pragma unroll
  for (int mb = 0; mb < (kPre ? kPre : 1); ++mb)
#pragma unroll
    for (int pb = 0; pb < PB; ++pb)
#pragma unroll
      for (int g = 0; g < 4; ++g) resv[mb][pb][g] = f32x4{0.f, 0.f, 0.f, 0.f};

  // Rotated item loop: an iteration first takes over the PREVIOUS item's accumulators (writes them out, or with
  // DEFER copies them to `held`), then runs this item's steps (one extra iteration handles the last item; the
  // first one stores zeros to out-of-range offsets, which are dropped).
  f32x16 held[DEFER ? MB : 1][DEFER ? PB : 1];
  f32x4 rq[DEFER && EPI == kEpiResidual ? 4 : 1];      // residual quads in flight: pieces 2t, 2t+1 and 2t+2, 2t+3
  for (int it = 0; it <= my_items; ++it) {
    const OutGeom g_ = out_geom(it > 0 ? lid + (it - 1) * G : lid, it > 0);
    const auto aux_rsrc = aux_desc(g_.img);
    const auto out_rsrc = __builtin_amdgcn_make_buffer_rsrc(
        p.out + (size_t)g_.img * img_pix * COUT, 0, (unsigned)(img_pix * COUT * 4), 0x00020000);
    // piece j = register quad g of accumulator (mb, pb): j = 8*mb + 4*pb + g, so that the two pieces of a step are
    // 64 contiguous, 64-byte aligned bytes of one pixel (with j = 8*mb + 2*g + pb — 32-byte fragments of two pixels,
    // their neighbours written microseconds later — WRITE_SIZE read 1.56 x the tensor)
    auto load_res = [&](int j) -> f32x4 {
      const int mb = j >> 3, pb = (j >> 2) & 1, g = j & 3;
      return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(aux_rsrc, byte_off(g_, mb, pb, g), 0, 0));
    };
    auto finish = [&](int j, const f32x16& a, f32x4 rr) {
      const int mb = j >> 3, pb = (j >> 2) & 1, g = j & 3;
      const f32x4 bias = *reinterpret_cast<const f32x4*>(bias_s + g_.chb + mb * 32 + 8 * g);
      f32x4 v = {a[4 * g], a[4 * g + 1], a[4 * g + 2], a[4 * g + 3]};
      v = v + bias;
      if constexpr (EPI == kEpiRelu) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.f);
      } else {
        v = rr + v * p.res_scale;       // -ffp-contract=off: two roundings, as keras
      }
      if constexpr (!(ABL & 1))
        // soffset must NOT be a register here: gfx950 reads the 128-bit store data late (the last quad of each
        // 16-lane row last), and hipcc (ROCm 7.2) only pads the "store data overwritten too early" hazard when
        // soffset is an immediate — with an SGPR soffset the next VALU write of v's first register corrupted lanes
        // 12-15 / 28-31 on some schedules (experiments/README.md; tests/test_gpu_stress.py is the screen).
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), out_rsrc, byte_off(g_, mb, pb, g), 0, 0);
      else
        asm volatile("" ::"v"(v));
    };
    constexpr bool kRes = EPI == kEpiResidual && !(ABL & 2);
    if constexpr (!DEFER) {
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const int mb = j >> 3, pb = (j >> 2) & 1, g = j & 3;
        f32x4 rr = {1.f, 1.f, 1.f, 1.f};
        if constexpr (kRes) rr = mb < kPre ? resv[mb][pb][g] : load_res(j);
        finish(j, acc[mb][pb], rr);
      }
    } else {
#pragma unroll
      for (int mb = 0; mb < MB; ++mb)
#pragma unroll
        for (int pb = 0; pb < PB; ++pb) held[mb][pb] = acc[mb][pb];
      if (it == my_items) {       // nothing left to hide behind: write the last item out in one go
#pragma unroll
        for (int j = 0; j < 16; ++j) {
          f32x4 rr = {1.f, 1.f, 1.f, 1.f};
          if constexpr (kRes) rr = load_res(j);
          finish(j, held[j >> 3][(j >> 2) & 1], rr);
        }
      } else if constexpr (kRes) {
        rq[0] = load_res(0);      // pieces 0 and 1 run in the first step
        rq[1] = load_res(1);
      }
    }
    if (it == my_items) break;
    const int item = lid + it * G;
    const bool have_next_item = it + 1 < my_items;
#pragma unroll
    for (int mb = 0; mb < MB; ++mb)
#pragma unroll
      for (int pb = 0; pb < PB; ++pb)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[mb][pb][e] = 0.f;

    auto do_cc = [&](const int cc, auto first_c) {
      constexpr bool kFirst = decltype(first_c)::value;      // cc == 0 is its own copy of the step code
      (void)kFirst;
      const float* const ib = in_s + (cc & 1) * (IN_BYTES / 4);
      const float* const ib_next = in_s + ((cc + 1) & 1) * (IN_BYTES / 4);
      // what is staged into ib_next during this cc: (this item, cc+1), or on the last cc the NEXT item's chunk 0
      // (on the very last item: its own chunk 0 again, which nobody reads)
      const bool last_cc = cc == NCC - 1;
      const int in_cc = last_cc ? 0 : cc + 1;
      if constexpr (ISSUE) {
        if (last_cc && have_next_item) st.set_stage_item(item + G);
      }
#pragma unroll
      for (int tap = 0; tap < 9; ++tap) {
        const float* const wb = w_s + mf_slot * WCH;
        const int nx_slot = mf_slot == NWBUF - 1 ? 0 : mf_slot + 1;
        const float* const wb_nx = w_s + nx_slot * WCH;
        constexpr int kNoIn = (ABL & 8) ? 1 : 0;
        const int n_in = (tap < IN_BLOCKS && !kNoIn) ? Stage::N_IN : 0;     // folds: tap is an unrolled constant

#pragma unroll
        for (int s = 0; s < KSTEPS; ++s) {
          if (s < KSTEPS - 1) {
            read_frags(w_nxt, x_nxt, ib, wb, tap, s + 1);
          } else if (tap < 8) {
            read_frags(w_nxt, x_nxt, ib, wb_nx, tap + 1, 0);
          } else {
            read_frags(w_nxt, x_nxt, ib_next, wb_nx, 0, 0);
          }
          if constexpr (DEFER) {
            // first input chunk of an item only (this copy of the code): step `tap` finishes pieces 2*tap and
            // 2*tap + 1 of the previous item; their residual quads were fetched one step earlier, BEFORE that
            // step's DMAs in issue order, so waiting for them never waits for a DMA younger than a step (issuers of
            // the DeferAsym form, which issue at k-step 2 and finish piece 2*tap at k-step 1: three quarters of a step;
            // issuing at k-step 0 put six fresh DMAs in front of that wait and cost conv-B 0.5 %)
            if (kFirst && tap < 8) {
              if (s == MIDS && kRes && tap < 7) {
                rq[2 * ((tap + 1) & 1)] = load_res(2 * tap + 2);
                rq[2 * ((tap + 1) & 1) + 1] = load_res(2 * tap + 3);
              }
            }
          }
          if constexpr (ISSUE) {
            if (s == MIDS) {
              // this step's DMAs: input round first, then the weight chunk three steps ahead
              if (n_in) st.issue_in((cc + 1) & 1, tap < IN_BLOCKS ? tap : 0, in_cc);
              if constexpr (!(ABL & 4)) st.issue_w();
            }
          }
          if constexpr (DEFER) {
            if (kFirst && tap < 8 && (s == 1 || s == 3)) {
              const int j = 2 * tap + (s >> 1);
              f32x4 rr = {1.f, 1.f, 1.f, 1.f};
              if constexpr (kRes) rr = rq[2 * (tap & 1) + (s >> 1)];
              finish(j, held[j >> 3][(j >> 2) & 1], rr);
            }
          }
          if constexpr (kPre > 0 && !DEFER) {
            // the item's last step: its residual values, younger than every DMA this wave waits for before the
            // epilogue, land under the step's 64 MFMAs
            if (tap == 8 && last_cc && s == (MIDS < KSTEPS - 1 ? MIDS + 1 : MIDS)) {
              const OutGeom g_ = out_geom(item, true);
              const auto aux_rsrc = aux_desc(g_.img);
#pragma unroll
              for (int mb = 0; mb < kPre; ++mb)
#pragma unroll
                for (int pb = 0; pb < PB; ++pb)
#pragma unroll
                  for (int g = 0; g < 4; ++g)
                    resv[mb][pb][g] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(
                                                                    aux_rsrc, byte_off(g_, mb, pb, g), 0, 0));
            }
          }
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int mb = 0; mb < MB; ++mb)
#pragma unroll
              for (int pb = 0; pb < PB; ++pb)
                acc[mb][pb] = __builtin_amdgcn_mfma_f32_32x32x2f32(w_cur[mb][j], x_cur[pb][j], acc[mb][pb], 0, 0, 0);
#pragma unroll
          for (int q = 0; q < MB; ++q) w_cur[q] = w_nxt[q];
#pragma unroll
          for (int q = 0; q < PB; ++q) x_cur[q] = x_nxt[q];
        }
        mf_slot = nx_slot;
        __builtin_amdgcn_sched_barrier(0);
        // retire the weight chunk issued in the PREVIOUS step (and everything older): what this wave issued after
        // it is AT LEAST this step's input round and weight chunk (anything more only makes the wait stricter)
        // (a copy that issues none takes the data from the barrier behind the issuers' wait)
        if constexpr (ISSUE) {
          if (n_in) wait_vmcnt<N_W + Stage::N_IN>(); else wait_vmcnt<N_W>();
        }
        if constexpr (!(ABL & 16)) __syncthreads();
      }
    };
    do_cc(0, std::true_type{});
#pragma unroll 1
    for (int cc = 1; cc < NCC; ++cc) do_cc(cc, std::false_type{});
  }
  };   // run
  if constexpr (ASYM) {
    if (wave < 4) {
      run(std::integral_constant<int, (STG - 2) % KSTEPS>{}, std::true_type{});
    } else {
      // static priority for the half that is dispatched second (wave-uniform: `wave` is a scalar)
      if constexpr ((STG - 2) / KSTEPS == 1) __builtin_amdgcn_s_setprio(1);
      run(std::integral_constant<int, 0>{}, std::false_type{});
    }
  } else if constexpr (STG == 1) {
    if (wave < 4)
      run(std::integral_constant<int, 0>{}, std::true_type{});
    else
      run(std::integral_constant<int, KSTEPS / 2>{}, std::true_type{});
  } else {
    run(std::integral_constant<int, 0>{}, std::true_type{});
  }
  wait_vmcnt<0>();       // no DMA may still be writing this workgroup's LDS when it is released
}

template <int CIN, int COUT, int EPI, int ABL = 0, int PRE = 0, int STG = 0, bool DEFER = false>
static hipError_t launch_body32_one(const ConvParams& p, hipStream_t stream) {
  const long long items = (long long)p.n * p.tiles_x * p.tiles_y * (COUT / NT);
  return launch_persistent<conv3x3_body32_kernel<CIN, COUT, EPI, ABL, PRE, STG, DEFER>>(LDS_BYTES, THREADS, items, 1, 0, stream, p);
}

constexpr int kAsym = 2 + KSTEPS / 2;      // STG of Body32Form::DeferAsym: the issuers' DMAs half a step into the step

template <int F>
static hipError_t launch_body32_feat(const ConvParams& p, int epilogue, Body32Form form, hipStream_t stream) {
  const bool relu = epilogue == kEpiRelu;
#ifdef DSEN2_DIAG
  if (form == Body32Form::Plain || form == Body32Form::StaggerA) {
    if (!relu) return launch_body32_one<F, F, kEpiResidual, 0, 2, 0>(p, stream);
    return form == Body32Form::Plain ? launch_body32_one<F, F, kEpiRelu, 0, 0, 0>(p, stream) : launch_body32_one<F, F, kEpiRelu, 0, 0, 1>(p, stream);
  }
  if (form == Body32Form::DeferStaggerA && !relu) return launch_body32_one<F, F, kEpiResidual, 0, 0, 0, true>(p, stream);
  if (form == Body32Form::DeferStagger || form == Body32Form::DeferStaggerA)
    return relu ? launch_body32_one<F, F, kEpiRelu, 0, 0, 1, true>(p, stream) : launch_body32_one<F, F, kEpiResidual, 0, 0, 1, true>(p, stream);
#define DSEN2_ASYM(FORM, STG)                                                                                      \
  if (form == Body32Form::FORM)                                                                                    \
    return relu ? launch_body32_one<F, F, kEpiRelu, 0, 0, STG, true>(p, stream) : launch_body32_one<F, F, kEpiResidual, 0, 0, STG, true>(p, stream);
  DSEN2_ASYM(DeferAsymS0, 2) DSEN2_ASYM(DeferAsymS1, 3) DSEN2_ASYM(DeferAsymS3, 5) DSEN2_ASYM(DeferAsymPrio, 8)
#undef DSEN2_ASYM
#else
  if (form != Body32Form::DeferAsym) return hipErrorInvalidValue;     // the other forms exist in the diagnostic build only
#endif
  return relu ? launch_body32_one<F, F, kEpiRelu, 0, 0, kAsym, true>(p, stream) : launch_body32_one<F, F, kEpiResidual, 0, 0, kAsym, true>(p, stream);
}

hipError_t launch_conv3x3_body32(const ConvParams& p, int feat, int epilogue, Body32Form form, int ablate, hipStream_t stream) {
  // per-image buffer descriptors address bytes with 32 bits (and keep 0x80000000 out of range)
  if ((size_t)p.h * p.w * feat * 4 >= 0x80000000ull) return hipErrorNotSupported;
#ifdef DSEN2_DIAG
  if (feat == 128 && ablate != 0) {
    // the masks of the DeferAsym form that the mask table of profiles/body32_asym.md needs
#define DSEN2_ABL_ASYM(M)                                                                                \
  if (ablate == M && form == Body32Form::DeferAsym)                                                      \
    return epilogue == kEpiRelu ? launch_body32_one<128, 128, kEpiRelu, M, 0, kAsym, true>(p, stream)    \
                                : launch_body32_one<128, 128, kEpiResidual, M, 0, kAsym, true>(p, stream);
    DSEN2_ABL_ASYM(3) DSEN2_ABL_ASYM(15) DSEN2_ABL_ASYM(16)
#undef DSEN2_ABL_ASYM
#define DSEN2_ABL(M)                                                                             \
  if (ablate == M)                                                                               \
    return epilogue == kEpiRelu ? launch_body32_one<128, 128, kEpiRelu, M>(p, stream)            \
                                : launch_body32_one<128, 128, kEpiResidual, M, 2>(p, stream);
    DSEN2_ABL(1) DSEN2_ABL(2) DSEN2_ABL(3) DSEN2_ABL(4) DSEN2_ABL(8) DSEN2_ABL(12) DSEN2_ABL(15) DSEN2_ABL(16) DSEN2_ABL(31)
#undef DSEN2_ABL
    return hipErrorInvalidValue;
  }
#endif
  if (ablate != 0) return hipErrorInvalidValue;     // timing-only ablations exist in the diagnostic build only
  if (feat == 128) return launch_body32_feat<128>(p, epilogue, form, stream);
  if (feat == 256) return launch_body32_feat<256>(p, epilogue, form, stream);
  return hipErrorInvalidValue;
}

}  // namespace dsen2
