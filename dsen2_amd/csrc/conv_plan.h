// conv_plan.h — which kernel runs a convolution, what format its weights have and how many floats that is: decided once per
// layer (plan_conv) and carried as one value that sizes the buffer, fills it (pack) and launches the kernel (launch).
// conv_plan.hip is host code only; a new kernel or weight format plugs in there and in its own kernel file.
#pragma once
#include <vector>

#include "dsen2_internal.h"

namespace dsen2 {

// DSen2Net.py's graph: First (Concatenate + Conv2D + ReLU), the residual blocks' BodyA (+ ReLU) / BodyB (x 0.1 + block input),
// Output (+ skip, NCHW); training's input gradients of a body (any precision: 1 is the mixed-precision step of an fp32 model) /
// of the output convolution (capi_train.hip)
enum class ConvRole { First, BodyA, BodyB, Output, DgradBody, DgradOutput };
enum class ConvKernel {
  Tile,       // conv3x3_mfma.hip: weights [slab][cc][tap][g][o][j] (dsen2_internal.h) with (kc, nt)
  Body32,     // conv3x3_body32.hip: the same packing, kc 32, nt 128
  Body16,     // conv3x3_body16w.hip: bf16 `perm16` chunks of 32 channels
  Body16x3,   // conv3x3_body16w.hip (X3): the (wh, wl, wh) planes as a virtual 3F -> F bf16 kernel
  Out         // conv3x3_out.hip's packing, and conv3x3_out_mfma.hip's behind it when out_mfma
};

constexpr size_t kAlignFloats = 64;   // 256-byte alignment of every device sub-buffer
inline size_t align_up(size_t v) { return (v + kAlignFloats - 1) / kAlignFloats * kAlignFloats; }

struct ConvPlan {
  ConvRole role;
  ConvKernel kernel;
  int epilogue;             // what the role computes (the last block's BodyB of a 16-bit model launches kEpiResidualF32 instead)
  int cin, cout;            // real (keras) channel counts
  int cin_pad, cout_pad;    // channels of the input tensor / of the bias buffer
  int kc, nt;               // Tile, Body32: input-channel chunk and output-channel slab of the packing
  int real_channels;        // Tile, First: input channels whose MFMAs are issued (10 / 12); 0 = all cin_pad
  Body32Form body32;        // Body32
  bool out_mfma;            // Out: conv3x3_out_mfma.hip's packing follows the vector-unit packing, and that kernel is tried first
  bool first_direct;        // First, fp32: conv3x3_first.hip (reads the NCHW inputs itself, same weights) is tried first
  int first16_planes;       // First, 16-bit model: conv3x3_first16.hip is tried first; its 1 (wh) / 2 (wh | wl) weight planes lie at first16_off
  // the layer's device buffer, in floats: weights at 0 | bias | first16 image, each part 256-byte aligned
  size_t weight_floats, bias_off, first16_off, floats;
};

struct BandGroups { int c10, c20, c60; };   // of the network's inputs (First only; NULL = a bare cin -> cout convolution)
// precision (0 fp32, 1 bf16 operands, 2 bf16x3) of the residual stream the layer reads or writes.  false: no kernel for this shape.
bool plan_conv(ConvRole role, int cin, int cout, int precision, const Tuning& tune, const BandGroups* bands, ConvPlan* plan);
// kernel HWIO (3, 3, cin, cout) fp32 + bias[cout] -> dst[plan.floats], zero padded; bias == NULL: the weights alone, dst[plan.weight_floats]
void pack(const ConvPlan& plan, const float* kernel_hwio, const float* bias, float* dst);
// One launch of the layer's kernel (First: the generic form behind launch_pack_inputs; capi.hip tries the direct kernels first)
hipError_t launch(const ConvPlan& plan, const ConvParams& p, int epilogue, const Tuning& tune, hipStream_t stream);

// "This kernel does not take this shape, use the next one" is hipErrorNotSupported, with nothing launched.  *done = `e` was a
// launch; returns what the caller has to fail on (hipSuccess: go on — done, or try the next kernel).
inline hipError_t try_launch(hipError_t e, bool* done) { *done = e == hipSuccess; return e == hipErrorNotSupported ? hipSuccess : e; }

struct Layer {
  ConvPlan plan;
  size_t off, flat_off;   // float offsets of the layer's buffer inside dev_params / of its kernel (+ bias) inside the keras-flat array
  const float* weights(const float* params) const { return params + off; }
  const float* bias(const float* params) const { return params + off + plan.bias_off; }
  const float* first16(const float* params) const { return params + off + plan.first16_off; }
};
struct NetworkPlan {            // a whole network, utils/DSen2Net.py:29-35 in graph order
  std::vector<Layer> layers;
  size_t n_params = 0;          // keras-flat floats
  size_t dev_param_floats = 0;
  size_t chain_stride = 0;      // 16-bit models: the chain kernels address body layer l's weights and bias at l * chain_stride bytes
};
bool plan_network(int c10, int c20, int c60, int num_layers, int feat, int precision, const Tuning& tune, NetworkPlan* net);

}  // namespace dsen2
