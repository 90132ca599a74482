// conv_plan.hip — the one decision of which kernel runs a layer (conv_plan.h), the weight packers that belong to no single
// kernel file, and the dispatch to the kernel files' launchers.  Host code only.
#include <cstring>
#include <vector>

#include "conv_plan.h"

namespace dsen2 {

namespace {

constexpr int kBody16Chunk = 32;   // input channels per weight chunk of conv3x3_body16w.hip

bool sentinel2(const BandGroups* b) { return b && b->c10 == 4 && b->c20 == 6 && (b->c60 == 0 || b->c60 == 2); }

// host_kernel HWIO (3,3,cin,cout) -> wpk[slab][cc][tap][g][o][j] (dsen2_internal.h), zero padded
void pack_tile_weights(const float* k, const ConvPlan& pl, float* dst) {
  const int ncc = pl.cin_pad / pl.kc, nslab = pl.cout_pad / pl.nt, ng = pl.kc / 4;
  size_t i = 0;
  for (int slab = 0; slab < nslab; ++slab)
    for (int cc = 0; cc < ncc; ++cc)
      for (int tap = 0; tap < 9; ++tap)
        for (int gg = 0; gg < ng; ++gg)
          for (int o = 0; o < pl.nt; ++o)
            for (int j = 0; j < 4; ++j, ++i) {
              const int c = cc * pl.kc + 4 * gg + j, oc = slab * pl.nt + o;
              dst[i] = (c < pl.cin && oc < pl.cout) ? k[((size_t)tap * pl.cin + c) * pl.cout + oc] : 0.f;
            }
}

// kernel HWIO fp32 -> bf16 [slab][cc (32 channels)][step][g (groups of 8 ch)][o (128)][8]: one (slab, cc, step) chunk is the LDS
// image of conv3x3_body16w.hip; dst holds 9*cin*cout uint16.  The kernel walks the taps dx-major to keep its pixel-row fragments
// over the three dy of one dx: step s carries tap (dy, dx) = (s % 3, s / 3).  perm16: row o of a slab holds output channel
// 32*(o>>5) + 8*((o&15)>>2) + 4*((o>>4)&1) + (o&3), so that the two 16-row accumulators of a 32-channel pair give a lane 8
// consecutive channels.
void pack_conv_weights_bf16_host(const float* k, int cin, int cout, uint16_t* dst) {
  const int ncc = cin / kBody16Chunk, nslab = cout / 128, ng = kBody16Chunk / 8;
  size_t i = 0;
  for (int slab = 0; slab < nslab; ++slab)
    for (int cc = 0; cc < ncc; ++cc)
      for (int step = 0; step < 9; ++step) {
        const int tap = (step % 3) * 3 + step / 3;
        for (int g = 0; g < ng; ++g)
          for (int o = 0; o < 128; ++o)
            for (int j = 0; j < 8; ++j, ++i) {
              const int ch = 32 * (o >> 5) + 8 * ((o & 15) >> 2) + 4 * ((o >> 4) & 1) + (o & 3);
              const int c = cc * kBody16Chunk + 8 * g + j, oc = slab * 128 + ch;
              dst[i] = f32_to_bf16_rne(k[((size_t)tap * cin + c) * cout + oc]);
            }
      }
}

// kernel HWIO fp32 (3,3,cin,cout) -> the packed bf16 layout of a virtual (3,3,3*cin,cout) kernel: input chunk 3*cc + j of 32
// channels = plane (wh, wl, wh)[j] of real chunk cc (wh = RNE bf16 of w, wl = RNE bf16 of w - wh) — the order in which
// conv3x3_body16w.hip (X3) walks the activation planes (xh, xh, xl); dst holds 27*cin*cout uint16
void pack_conv_weights_bf16x3_host(const float* k, int cin, int cout, uint16_t* dst) {
  const int vcin = 3 * cin;
  std::vector<float> v((size_t)9 * vcin * cout);
  for (int tap = 0; tap < 9; ++tap)
    for (int c = 0; c < cin; ++c)
      for (int o = 0; o < cout; ++o) {
        const float w = k[((size_t)tap * cin + c) * cout + o];
        const uint32_t hu = (uint32_t)f32_to_bf16_rne(w) << 16;
        float wh;
        memcpy(&wh, &hu, 4);
        const float wl = w - wh;                       // exact; rounded to bf16 by the packer below
        const int cc = c / kBody16Chunk, j = c % kBody16Chunk;
        float* base = v.data() + ((size_t)tap * vcin + (size_t)cc * 3 * kBody16Chunk + j) * cout + o;
        base[0] = wh;
        base[(size_t)kBody16Chunk * cout] = wl;
        base[(size_t)2 * kBody16Chunk * cout] = wh;
      }
  pack_conv_weights_bf16_host(v.data(), vcin, cout, dst);
}

size_t tap_floats(const ConvPlan& pl) { return (size_t)9 * pl.cin_pad * pl.cout_pad; }

}  // namespace

bool plan_conv(ConvRole role, int cin, int cout, int precision, const Tuning& tune, const BandGroups* bands, ConvPlan* plan) {
  if (cin <= 0 || cout <= 0 || precision < 0 || precision > 2) return false;
  ConvPlan& pl = *plan;
  pl = ConvPlan{};
  pl.role = role; pl.cin = cin; pl.cout = cout; pl.body32 = tune.body32;
  const bool feat_out = cout == 128 || cout == 256;
  switch (role) {
    case ConvRole::Output:          // always fp32: the last block writes an fp32 tensor in every precision
      if (cout > 32 || (cin != 128 && cin != 256)) return false;
      pl.epilogue = kEpiSkipNCHW; pl.cin_pad = cin;
      pl.kernel = ConvKernel::Tile; pl.kc = 32; pl.nt = 32; pl.cout_pad = 32;
      if (cout <= 8 && tune.out != OutKernel::Tile) {
        pl.kernel = ConvKernel::Out; pl.kc = pl.nt = 0; pl.cout_pad = 8; pl.out_mfma = tune.out == OutKernel::MfmaThenValu;
      }
      break;
    case ConvRole::First:
    case ConvRole::DgradOutput:     // 16 -> F on dL/dout padded to 16 channels: all of them
      if (!feat_out || cin > 16) return false;
      pl.kernel = ConvKernel::Tile; pl.kc = 16; pl.nt = 128; pl.cin_pad = 16; pl.cout_pad = cout;
      pl.epilogue = kEpiResidual;
      if (role == ConvRole::DgradOutput) break;
      // a precision-1 model's first convolution writes the residual stream directly as its two blocked 16-bit planes; a
      // precision-2 model's generic one writes fp32, which launch_split3_f32 then splits
      pl.epilogue = precision == 1 ? kEpiReluSplit : kEpiRelu;
      if (tune.first == FirstKernel::Direct && (cin == 10 || cin == 12)) pl.real_channels = cin;
      // the Sentinel-2 band groups 4 + 6 (+ 2) have kernels that read the NCHW inputs themselves: fp32 conv3x3_first.hip (same
      // weights), 16-bit models conv3x3_first16.hip (its own image; the fp32 form stays for the shapes it does not take)
      pl.first_direct = precision == 0 && tune.first == FirstKernel::Direct && sentinel2(bands);
      if (precision != 0 && sentinel2(bands)) pl.first16_planes = precision;
      break;
    case ConvRole::BodyA:
    case ConvRole::BodyB:
    case ConvRole::DgradBody:
      if (!feat_out || cin != cout) return false;
      pl.epilogue = role == ConvRole::BodyA ? kEpiRelu : kEpiResidual;
      pl.cin_pad = cin; pl.cout_pad = cout; pl.kc = 32; pl.nt = 128;     // every fp32 structure reads the same packing
      pl.kernel = precision == 1   ? ConvKernel::Body16
                  : precision == 2 ? ConvKernel::Body16x3
                  : tune.body == BodyKernel::Body32 ? ConvKernel::Body32 : ConvKernel::Tile;
      break;
  }
  // the layer's buffer: the one place a weight-buffer size is computed
  const size_t taps = tap_floats(pl);
  pl.weight_floats = pl.kernel == ConvKernel::Body16     ? taps / 2          // bf16
                     : pl.kernel == ConvKernel::Body16x3 ? 3 * taps / 2      // three bf16 planes
                                                         : taps + (pl.out_mfma ? out_mfma_weight_floats(cin) : 0);
  pl.bias_off = align_up(pl.weight_floats);
  pl.floats = pl.first16_off = pl.bias_off + align_up((size_t)pl.cout_pad);
  if (pl.first16_planes) pl.floats += align_up((first16_weight_u16(cout, pl.first16_planes == 2) + 1) / 2);
  return true;
}

void pack(const ConvPlan& pl, const float* k, const float* bias, float* dst) {
  memset(dst, 0, sizeof(float) * (bias ? pl.floats : pl.weight_floats));
  switch (pl.kernel) {
    case ConvKernel::Tile:
    case ConvKernel::Body32: pack_tile_weights(k, pl, dst); break;
    case ConvKernel::Body16: pack_conv_weights_bf16_host(k, pl.cin, pl.cout, reinterpret_cast<uint16_t*>(dst)); break;
    case ConvKernel::Body16x3: pack_conv_weights_bf16x3_host(k, pl.cin, pl.cout, reinterpret_cast<uint16_t*>(dst)); break;
    case ConvKernel::Out:          // the output kernels have their own operand orders, restated beside them
      pack_out_valu_weights_host(k, pl.cin, pl.cout, dst);
      if (pl.out_mfma) pack_out_mfma_weights_host(k, pl.cin, pl.cout, dst + tap_floats(pl));
      break;
  }
  if (!bias) return;
  memcpy(dst + pl.bias_off, bias, sizeof(float) * pl.cout);
  if (pl.first16_planes)
    pack_first16_weights_host(k, pl.cin, pl.cout, pl.first16_planes == 2, reinterpret_cast<uint16_t*>(dst + pl.first16_off));
}

hipError_t launch(const ConvPlan& pl, const ConvParams& p, int epilogue, const Tuning& t, hipStream_t stream) {
  switch (pl.kernel) {
    case ConvKernel::Out: {
      ConvParams pm = p;
      pm.wpk += tap_floats(pl);     // behind the vector-unit packing
      bool done = false;
      const hipError_t e = pl.out_mfma ? try_launch(launch_conv3x3_out_mfma(pm, pl.cin_pad, stream, t.out_ablate), &done) : hipSuccess;
      return e != hipSuccess || done ? e : launch_conv3x3_out_valu(p, pl.cin_pad, stream);
    }
    // An image conv3x3_body32.hip cannot address (>= 2 GiB of activations) is an error, not a silent switch of kernels:
    // dsen2's entry points reject such shapes up front.
    case ConvKernel::Body32: return launch_conv3x3_body32(p, pl.cin_pad, epilogue, pl.body32, t.ablate, stream);
    // (masks from 1024 up belong to the chain kernel; the precision-2 kernels have no ablation builds)
    case ConvKernel::Body16: return launch_conv3x3_body16w(p, pl.cin_pad, epilogue, false, t.ablate & 1023, stream, t.grid_cap);
    case ConvKernel::Body16x3: return launch_conv3x3_body16w(p, pl.cin_pad, epilogue, true, 0, stream);
    case ConvKernel::Tile: {
      // timing-only ablations exist for the persistent kernels only
      const int mask = pl.role == ConvRole::Output ? t.out_ablate : pl.cin_pad == pl.cout_pad ? t.ablate : 0;
      if (mask != 0) return hipErrorInvalidValue;
      return launch_conv3x3_tile(p, pl.cin_pad, pl.cout_pad, epilogue, pl.real_channels, stream);
    }
  }
  return hipErrorInvalidValue;
}

bool plan_network(int c10, int c20, int c60, int num_layers, int feat, int precision, const Tuning& tune, NetworkPlan* net) {
  const BandGroups bands{c10, c20, c60};
  *net = NetworkPlan{};
  auto add = [&](ConvRole role, int ci, int co, int prec) {
    Layer L;
    if (!plan_conv(role, ci, co, prec, tune, &bands, &L.plan)) return false;
    L.flat_off = net->n_params;
    net->n_params += (size_t)9 * ci * co + co;
    L.off = net->dev_param_floats;
    net->dev_param_floats += L.plan.floats;
    net->layers.push_back(L);
    return true;
  };
  // a network without residual blocks is fp32 throughout; the output convolution (utils/DSen2Net.py:35 — input_shape[-1][0]) always
  if (!add(ConvRole::First, c10 + c20 + c60, feat, num_layers > 0 ? precision : 0)) return false;
  for (int i = 0; i < num_layers; ++i)
    if (!add(ConvRole::BodyA, feat, feat, precision) || !add(ConvRole::BodyB, feat, feat, precision)) return false;
  if (!add(ConvRole::Output, feat, c60 > 0 ? c60 : c20, 0)) return false;
  // the body layers share one plan, so their buffers lie one plan apart
  if (num_layers > 0 && precision != 0) net->chain_stride = net->layers[1].plan.floats * sizeof(float);
  return true;
}

}  // namespace dsen2
