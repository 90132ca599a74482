// Internal declarations shared by the HIP translation units of libdsen2_hip.so (gfx950 only): the tensor layouts, ConvParams,
// Tuning, and one launcher per kernel file.  Which launcher runs a layer, which weight format it reads and how many floats that
// is, is decided in conv_plan.h.  A launcher that does not take a shape returns hipErrorNotSupported and has launched nothing.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <mutex>

namespace dsen2 {

// ---- data layout ------------------------------------------------------------------------------
// Activations inside the network: NHWC float32, [n][y][x][c], c contiguous (512 B per pixel at F=128).
// Packed conv weights of the tile kernel (conv3x3_mfma.hip) and of conv3x3_body32.hip (conv_plan.hip: pack_tile_weights; the
// other kernels' formats are described at their packers, there or beside the kernel):
//   wpk[slab][cc][tap][g][o][j]  float32
//     slab : output-channel slab of NT channels handled by one workgroup      (COUT_PAD / NT)
//     cc   : input-channel chunk of KC channels                               (CIN_PAD / KC)
//     tap  : dy*3 + dx                                                        (9)
//     g    : group of 4 input channels inside the chunk                       (KC / 4)
//     o    : output channel inside the slab                                   (NT)
//     j    : input channel inside the group                                   (4)
//   value = K_hwio[dy][dx][cc*KC + 4g + j][slab*NT + o]   (0 where the index is padding)
// so one (slab, cc, tap) chunk is KC*NT contiguous floats that are copied verbatim into LDS, and one
// ds_read_b128 at [g][o] hands a lane the 4 A-operand values W[o][4g .. 4g+3].

constexpr int kTile = 16;                 // output pixels per workgroup edge (16 x 16 tile)
constexpr int kHalo = kTile + 2;          // 18
constexpr int kHaloPix = kHalo * kHalo;   // 324

enum Epilogue : int {
  kEpiRelu = 0, kEpiResidual = 1, kEpiSkipNCHW = 2,
  kEpiResidualF32 = 3,   // bf16 body kernel only
  kEpiReluSplit = 4      // generic first convolution of a precision-1 model (conv3x3_mfma.hip; band groups conv3x3_first16.hip does
                         // not take): relu(conv + b) written as blocked (hi, lo) planes (out, out2)
};

struct ConvParams {
  const float* in;     // NHWC [n][h][w][CIN_PAD]            (bf16 body kernel: bf16 NHWC)
  const float* wpk;    // packed weights (layout above)
  const float* bias;   // [COUT_PAD]
  const float* aux;    // kEpiResidual: NHWC [n][h][w][COUT]; kEpiSkipNCHW: NCHW [n][cout_real][h][w]
                       // (bf16 body kernel, residual epilogues: the `hi` plane of the residual stream)
  float* out;          // NHWC [n][h][w][COUT] or NCHW [n][cout_real][h][w]  (bf16 body kernel, kEpiRelu: bf16 NHWC)
  void* out2;          // bf16 body kernel, residual epilogues: the `lo` plane of the residual stream; otherwise unused
  int n, h, w;
  int tiles_x, tiles_y;
  int cout_real;       // kEpiSkipNCHW only
  float res_scale;     // residual epilogues only
  unsigned long long* diag;   // DSEN2_DIAG builds, ablation bit 32: in-kernel time stamps (tools/stamp_body_conv.py); else NULL
};

// Kernel-structure choices of a model.  The product library always uses the defaults; the diagnostic build
// (-DDSEN2_DIAG, tools/ only) can change them through dsen2_diag_set for A/B measurements.
// First: Direct = conv3x3_first.hip / conv3x3_first16.hip where they take the band groups, else the tile kernel issuing the
// MFMAs of the 10 / 12 real channels only; Tile16 = the tile kernel over all 16 padded channels.  Body (fp32 F->F):
// conv3x3_body32.hip, or one tile per workgroup (conv3x3_mfma.hip, the independent first implementation).  Body32Form:
// DeferStagger = deferred epilogue + wave-group stagger for both convolutions; DeferStaggerA = conv-B not staggered;
// StaggerA = no deferral: conv-A staggered, conv-B with the whole residual tile prefetched under the last step; Plain = StaggerA without the stagger; DeferAsym = deferred epilogue, waves 0-3 issue every
// DMA, half a step into the step, and waves 4-7 none (conv3x3_dma.h, Role::Issuer): the product's at both widths and the only
// one outside DSEN2_DIAG builds (profiles/body32_asym.md); DeferAsymS0 / S1 / S3 / DeferAsymPrio = its measured alternatives
// (the issuers' DMAs at another k-step / waves 4-7 at s_setprio 1).  Out (Cout <= 8): conv3x3_out_mfma.hip where the shape
// fits it, else conv3x3_out.hip; always conv3x3_out.hip; Tile (and Cout > 8) = padded 32-wide block of conv3x3_mfma.hip.
enum class FirstKernel { Direct, Tile16 };
enum class BodyKernel { Body32, Tile };
enum class Body32Form { StaggerA, Plain, DeferStaggerA, DeferStagger, DeferAsym, DeferAsymS0, DeferAsymS1, DeferAsymS3, DeferAsymPrio };
enum class OutKernel { MfmaThenValu, Valu, Tile };
struct Tuning {
  FirstKernel first = FirstKernel::Direct;
  BodyKernel body = BodyKernel::Body32;
  Body32Form body32 = Body32Form::DeferAsym;
  OutKernel out = OutKernel::MfmaThenValu;
  int ablate = 0;          // timing-only ablation mask of the persistent body kernels (DSEN2_DIAG builds; wrong outputs)
  int grid_cap = 0;        // DSEN2_DIAG builds: launch at most this many workgroups of the bf16 body kernel (0 = one per CU)
  int first_ablate = 0;    // DSEN2_DIAG builds: timing-only ablation mask of the first convolution (conv3x3_first.hip)
  int out_ablate = 0;      // DSEN2_DIAG builds: timing-only ablation mask of conv3x3_out_mfma.hip
  int chain = 1;           // precision 1: one persistent launch over all body layers when the batch gives every CU whole patches
  // the one-tile-per-workgroup kernels of conv3x3_mfma.hip for every layer shape (dsen2_conv3x3_nhwc_ref)
  static Tuning reference() { Tuning t; t.first = FirstKernel::Tile16; t.body = BodyKernel::Tile; t.out = OutKernel::Tile; return t; }
};

// Per-kernel launch preparation: the dynamic-LDS attribute is a property of (kernel, device) and is set once per pair,
// under a mutex — host threads driving different devices (or one device from several streams) may reach a launcher
// at the same time.  One function-local static instance per kernel instantiation (its construction is thread-safe).
struct KernelOnce {
  std::mutex mu;
  bool done[64] = {};
  int cus[64] = {};
  // current device -> *dev_cus (its CU count); sets MaxDynamicSharedMemorySize of `kern` there on first use
  hipError_t prepare(const void* kern, size_t lds_bytes, int* dev_cus) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (dev < 0 || dev >= 64) return hipErrorInvalidDevice;
    std::lock_guard<std::mutex> lock(mu);
    if (!done[dev]) {
      if (lds_bytes > 0) {
        e = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
        if (e != hipSuccess) return e;
      }
      e = hipDeviceGetAttribute(&cus[dev], hipDeviceAttributeMultiprocessorCount, dev);
      if (e != hipSuccess) return e;
      done[dev] = true;
    }
    if (dev_cus) *dev_cus = cus[dev];
    return hipSuccess;
  }
};

// One 16 x 16 tile per workgroup (conv3x3_mfma.hip); layout above with (KC, NT) = (16, 128) for 16 -> F, (32, 128) for F -> F,
// (32, 32) for F -> 32 (kEpiSkipNCHW).  real_channels (16 -> F): issue the MFMAs of the first 10 / 12 input channels only (0 = all).
hipError_t launch_conv3x3_tile(const ConvParams& p, int cin_pad, int cout_pad, int epilogue, int real_channels, hipStream_t stream);
// last layer, F -> Cout <= 8, on the vector units (conv3x3_out.hip; weights packed by pack_out_valu_weights_host)
hipError_t launch_conv3x3_out_valu(const ConvParams& p, int feat, hipStream_t stream);
void pack_out_valu_weights_host(const float* kernel_hwio, int cin, int cout, float* dst);
// last layer, F -> Cout <= 6, the nine taps expanded into the M side of one GEMM (conv3x3_out_mfma.hip); weights packed by
// pack_out_mfma_weights_host.  hipErrorNotSupported: the shape does not fit it (row of Q too wide for LDS, more than 6 outputs).
hipError_t launch_conv3x3_out_mfma(const ConvParams& p, int feat, hipStream_t stream, int ablate = 0);
size_t out_mfma_weight_floats(int cin);
void pack_out_mfma_weights_host(const float* kernel_hwio, int cin, int cout, float* dst);
// First convolution reading the NCHW inputs directly (conv3x3_first.hip, exact fp32): p.in = x10, p.aux = x20; weights packed
// for the tile kernel (KC 16, NT 128); epilogue kEpiRelu only (p.out fp32 NHWC).
// hipErrorNotSupported for channel counts other than 10 / 12 (then: launch_pack_inputs + launch_conv3x3_tile).
struct FirstInputs { const float* x60; int c10, c20, c60; };
hipError_t launch_conv3x3_first(const ConvParams& p, const FirstInputs& f, int cout, int epilogue, hipStream_t stream, int ablate = 0);
// ... of a precision-1 / -2 model, on the bf16 matrix cores (conv3x3_first16.hip): same inputs; p.wpk = the buffer
// pack_first16_weights_host fills (first16_weight_u16(cout, x3) uint16); x3 = false: p.out / p.out2 = the blocked (hi, lo)
// planes of the residual stream (bf16 operands: out = relu(bf16(x) * bf16(w) + b)); x3 = true: p.out = hx (hi | xl planes),
// p.out2 = lo16 — launch_split3_f32's tensors — with three-MFMA products (xh*wh + xh*wl + xl*wh).  hipErrorNotSupported as above.
hipError_t launch_conv3x3_first16(const ConvParams& p, const FirstInputs& f, int cout, bool x3, hipStream_t stream);
size_t first16_weight_u16(int cout, bool x3);
void pack_first16_weights_host(const float* kernel_hwio, int cin, int cout, bool x3, uint16_t* dst);
// DMA-fed fp32 kernel (conv3x3_body32.hip): F = 128 or 256; weights packed for the tile kernel (KC 32, NT 128).
// hipErrorNotSupported: an image of 2 GiB or more (its per-image descriptors address bytes with 32 bits).
hipError_t launch_conv3x3_body32(const ConvParams& p, int feat, int epilogue, Body32Form form, int ablate, hipStream_t stream);
// bf16-operand body convolution, wide tile (conv3x3_body16w.hip), F = 128 or 256.  16-bit tensors are BLOCKED:
// [n][C/8][h][w][8] (an 8-channel block = a plane of 16-byte pixels).  p.in bf16 blocked; weights packed by
// pack_conv_weights_bf16_host (conv_plan.hip).  kEpiRelu: p.out bf16 blocked.  kEpiResidual: the residual
// stream as two blocked 16-bit tensors p.aux (hi = bf16 rounding, the next operand) / p.out2 (lo), updated in place.
// kEpiResidualF32: same inputs, result to p.out as fp32 NHWC (last block).  `ablate` != 0 only in DSEN2_DIAG builds.
// x3 = precision 2 ("bf16x3", conv3x3_body16w.hip X3): fp32-grade products on the bf16 matrix cores — every operand is two bf16
// numbers (hi + lo), a product is hi*hi + hi*lo + lo*hi.  16-bit OPERAND tensors carry two planes per image,
// [n][2][F/8][h][w][8] (hi | lo).  p.in = such a tensor; weights packed by pack_conv_weights_bf16x3_host.
//   kEpiRelu: p.out = relu(conv + bias) as a two-plane tensor.
//   kEpiResidual: the residual stream = p.aux (two planes: hi = bf16 rounding (ties away) of the bit pattern, xl = bf16(x - hi))
//     + p.out2 (lo16: the low halves, one plane): (hi, lo16) hold the exact fp32 value as in precision 1; updated in place.
//   kEpiResidualF32: same inputs, result to p.out as fp32 NHWC.
hipError_t launch_conv3x3_body16w(const ConvParams& p, int feat, int epilogue, bool x3, int ablate, hipStream_t stream, int grid_cap = 0);
// fp32 NHWC -> the precision-2 residual stream: hx [n][2][C/8][h][w][8] (hi | xl), lo [n][C/8][h][w][8] (c % 8 == 0)
hipError_t launch_split3_f32(const float* in_nhwc, void* hx, void* lo, int n, int h, int w, int c, hipStream_t stream);
// One launch over all 2d residual-block convolutions of a precision-1 network (conv3x3_body16w.hip, CHAIN): a workgroup
// owns whole patches through every layer, so layers need no cross-workgroup synchronisation.
struct ChainArgs {
  void* hi;                   // residual stream: bf16 rounding plane (the convolutions' operand) ...
  void* lo;                   // ... and low halves
  void* t;                    // relu(conv-A), bf16 blocked
  float* out_f32;             // last block's output, fp32 NHWC
  unsigned layer_stride;      // bytes between the packed weights (and between the biases) of consecutive body layers
  int n_layers;               // 2 * d
  int patches_per_wg;
  int seamless;               // layer boundaries without a drain (conv3x3_body16w.hip; filled in by the launcher)
};
// p.wpk / p.bias = the first body layer's packed weights / bias (the following layers' lie layer_stride bytes further
// each); p.n, p.h, p.w, p.res_scale as usual; the tensors come from `c`.  c.patches_per_wg is filled in here.
// x3: the precision-2 form (c.hi = the stream's two-plane operand tensor hi | xl, c.t two planes, weights packed by
// pack_conv_weights_bf16x3_host)
hipError_t launch_conv3x3_body16w_chain(const ConvParams& p, const ChainArgs& c, int feat, hipStream_t stream, int ablate = 0,
                                        bool x3 = false);
// > 0: the chain kernel keeps every CU as busy as the per-layer launches do for this batch (that many patches per
// workgroup); 0: use the per-layer kernels
int body16w_chain_patches_per_wg(int n, int h, int w, int feat, int cus);
// fp32 NHWC tensor <-> blocked (hi, lo) tensors: hi = (u + 0x8000) >> 16, lo = u & 0xffff per value (c % 8 == 0)
hipError_t launch_split_f32(const float* in_nhwc, void* hi, void* lo, int n, int h, int w, int c, hipStream_t stream);
hipError_t launch_join_f32(const void* hi, const void* lo, float* out_nhwc, int n, int h, int w, int c, hipStream_t stream);
// RNE bf16 of an fp32 value: the one rounding of every host packer of 16-bit weights
inline uint16_t f32_to_bf16_rne(float f) {
  uint32_t u = __builtin_bit_cast(uint32_t, f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);   // NaN stays NaN
  u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}

// ---- elementwise / gather kernels (patch_ops.hip) ---------------------------------------------
// concat(x10,x20,x60) NCHW -> NHWC with 16 channels (zero padded): folds keras Concatenate(axis=1).
hipError_t launch_pack_inputs(const float* x10, const float* x20, const float* x60, int c10, int c20, int c60,
                              float* out_nhwc16, int n, int h, int w, hipStream_t stream);
// general = true: always the general kernel (the windowed one otherwise takes up-sampling by 2 or more)
hipError_t launch_upsample(const float* in, float* out, int planes, int h, int w, int oh, int ow, float post_div,
                           hipStream_t stream, bool general = false);
hipError_t launch_tile_gather(const float* img, int H, int W, int C, int border, const int* origins, int count,
                              int P, float divisor, float* patches, hipStream_t stream);
// rows [row0, row1) of the image (0, H = all of it)
hipError_t launch_recompose(const float* patches, int count, int C, int P, int border, float* img, int H, int W,
                            float scale, int row0, int row1, hipStream_t stream);

// ---- flips and rotations (dihedral.hip) ------------------------------------------------------------
// out = D_op(in) (inverse: D_op^-1(in)) on n * c planes of ih x iw; out's planes are iw x ih for odd op & 3.  dev_ops (or NULL;
// needs ih == iw): int32 [n], sample s takes dev_ops[s] & 7 and `op` is not used.  No argument checks (dsen2_dihedral_nchw).
hipError_t launch_dihedral(const float* in, float* out, int n, int c, int ih, int iw, int op, const int* dev_ops, bool inverse,
                           hipStream_t stream);
// acc (n * c planes of h x w) = acc + D_op^-1(in); count > 0: = (acc + D_op^-1(in)) / (float)count, a correctly rounded divide
hipError_t launch_dihedral_accumulate(const float* in, float* acc, int n, int c, int h, int w, int op, int count, hipStream_t stream);
// (transposing, ry, rx) of op 0..7 as bits 2, 1, 0 — the index map of dihedral.hip's header comment, shared with corpus_batch.hip
__host__ __device__ __forceinline__ int dihedral_bits(int op) {
  // op:      0  1  2  3  4  5  6  7
  // bits:    0  5  3  6  1  4  2  7      (one hex digit each, op 0 lowest)
  return (int)(0x72416350u >> (4 * (op & 7))) & 7;
}

// ---- a training batch cut from a device-resident corpus (corpus_batch.hip) -------------------------------
// One tile's device images (HWC): lr10 [s*eh, s*ew, 4] with s = 2 (6 with run_60), lr20 [eh, ew, 6] ([3 eh, 3 ew, 6]), lr60 [eh, ew,
// 2] (run_60 only), gt [s*eh, s*ew, 6 (2)] of uint16 (gt_u16) or float32; (eh, ew) is the extent of the origin grid.
struct CorpusTileDev {
  const float *lr10, *lr20, *lr60;
  const void* gt;
  int eh, ew, gt_u16, pad_;
};
// ONE launch: every sample of dev_samples ([n, 4] int32: tile, oy, ox, op), every output tensor.  No argument checks
// (dsen2_corpus_batch); a sample whose tile or origin does not belong to the table is skipped by the kernel (nothing is read or
// written for it).
hipError_t launch_corpus_batch(const CorpusTileDev* dev_tiles, int n_tiles, bool run_60, const int* dev_samples, int n, float divisor,
                               float* x10, float* x20, float* x60, float* y, hipStream_t stream);

// ---- training (conv3x3_wgrad.hip, train_ops.hip) --------------------------------------------------
// Weight / bias gradient of a 3x3 'same' convolution: dw (HWIO (3,3,ci_real,co_real)) = scale * sum_p a[p + tap][ci] g[p][co],
// db[co_real] = scale * sum_p g[p][co]; a NHWC with ca channels, g NHWC with cg.  Shapes: cg % 128 == 0 (body, first layer), or
// cg <= 32 with ca % 128 == 0 (output layer); ca, cg multiples of 4.  ws: wgrad_workspace_floats() floats of split-K partials
// (0 = shape not supported).  Fixed-order reduction: the same bits on every run.
size_t wgrad_workspace_floats(int n, int h, int w, int ca, int cg);
// what a launch at this shape does: the number of 4 x 16 pixel tiles and of split-K runs (false = shape not supported)
bool wgrad_geometry(int n, int h, int w, int ca, int cg, long long* tiles, int* splits);
hipError_t launch_conv3x3_wgrad(const float* a, int ca, const float* g, int cg, int n, int h, int w, int ci_real, int co_real,
                                float scale, float* dw, float* db, float* ws, size_t ws_floats, hipStream_t stream);
// The same for F -> F (F = 128, 256) as bf16x3 on the bf16 matrix cores (conv3x3_wgrad16.hip): a and g are two-plane blocked
// operand tensors [n][2][F/8][h][w][8] bf16 (value = plane 0 + plane 1), every product a0*g0 + a0*g1 + a1*g0 in fp32; dw HWIO
// (3,3,F,F), db[F].  Same split-K with a fixed-order reduction.
size_t wgrad16_workspace_floats(int n, int h, int w, int feat);
bool wgrad16_geometry(int n, int h, int w, int feat, long long* tiles, int* splits);
hipError_t launch_conv3x3_wgrad16(const void* a_planes, const void* g_planes, int n, int h, int w, int feat, float scale, float* dw,
                                  float* db, float* ws, size_t ws_floats, hipStream_t stream);
// The one-plane instance of that kernel (mixed-precision training): a and g are one-plane blocked bf16 tensors [n][F/8][h][w][8],
// every product is the one bf16 MFMA a*g in fp32, db = scale * sum of the bf16 values of g.  Same workspace, same reduction.
hipError_t launch_conv3x3_wgrad16_bf16(const void* a, const void* g, int n, int h, int w, int feat, float scale, float* dw, float* db,
                                       float* ws, size_t ws_floats, hipStream_t stream);
// ---- losses (include/dsen2_hip.h, "losses and the no-data mask") ----
// The training step's loss of kind `kind` with parameter `param` (Huber's delta, Charbonnier's epsilon; read by those two alone)
// under mask mode `mask`, over NCHW out / y ([n][c][h][w], c <= 16); gpad = dL/dout as NHWC16 (channels >= c zero); partial:
// loss_partial_doubles(n*h*w) doubles of scratch.  e = out - y in float32, d = (double)e; loss2 = ((float)(sum rho(d) / N),
// (float)(sum d^2 / N)), gpad = (float)(rho'(d) * (double)inv) with inv = (float)(1.0 / N), N = n*c*h*w in EVERY mask mode: a batch's loss keeps the weight
// of its sample count (dsen2_nadam_step_shards, weighted_loss, the ranks of a data-parallel group and fit_corpus's epoch sums stay
// exact) and every valid pixel of a run weighs the same, however many of its neighbours are blank.  rho' in double, every
// operation rounded on its own.  kMaskNoData: a pixel whose target is 0 (-0 included; NaN and negatives are data) in all c bands
// adds nothing to either sum and has gpad = 0 in every band.  (kLossMae, kMaskNone), keras mean_absolute_error with gpad =
// sign(e) / N, is an instance of the one kernel template like the other seven pairs (loss_terms.h, with_loss).
enum { kLossMae = 0, kLossMse = 1, kLossHuber = 2, kLossCharbonnier = 3, kLossKinds = 4 };
enum { kMaskNone = 0, kMaskNoData = 1, kMaskModes = 2 };
size_t loss_partial_doubles(size_t pixels);
// The SSIM term of the loss (ssim_loss.hip): weight 0 = off.  w: the normalised separable window of `win` taps (odd, 3..11).
constexpr int kSsimLossMinWin = 3, kSsimLossMaxWin = 11;
struct SsimLossTerm {
  float weight = 0.f;
  int win = 0;
  double w[kSsimLossMaxWin] = {};
  double c1 = 0.0, c2 = 0.0;
};
// work: ssim_loss_work_doubles() doubles; its last three receive { sum (1 - q) over the unmasked windows, Nw [, unmasked windows
// (three)] }.  gpad != NULL: gpad[pixel][band] = (float)((double)gpad[pixel][band] - ((double)weight / Nw) * G); NULL: sums alone.
size_t ssim_loss_work_doubles();
hipError_t launch_ssim_loss(const float* out, const float* y, int n, int c, int h, int w, const SsimLossTerm& term, int mask, float* gpad,
                            double* work, bool three, hipStream_t stream);
// ssim (or NULL; weight > 0) with ssim_work (ssim_loss_work_doubles() doubles): the term's gradient is added to gpad after the
// pointwise kernel wrote it, and loss2[0] = (float)(sum rho / N + ((double)weight / Nw) * sum (1 - q)): one cast
hipError_t launch_loss_grad(const float* out, const float* y, float* gpad, double* partial, float* loss2, int n, int c, int h, int w,
                            int kind, float param, int mask, hipStream_t stream, const SsimLossTerm* ssim = nullptr,
                            double* ssim_work = nullptr);
// v = m > 0 ? v : 0 (count % 4 == 0, 16-byte aligned)
hipError_t launch_relu_mask(float* v, const float* m, size_t count, hipStream_t stream);
// the precision-2 residual stream (hx: hi | xl planes, lo16) -> fp32 NHWC: the exact inverse of launch_split3_f32 (xl is not read)
hipError_t launch_join3_f32(const void* hx, const void* lo, float* out_nhwc, int n, int h, int w, int c, hipStream_t stream);
// du = t > 0 ? v : 0 written as a two-plane operand tensor [n][2][c/8][h][w][8] (hi = RNE bf16 of the value, lo = RNE bf16 of
// value - hi): v fp32 NHWC, t a two-plane tensor (conv-A's output of a precision-2 model)
hipError_t launch_mask_split3(const float* v_nhwc, const void* t_planes, void* du_planes, int n, int h, int w, int c, hipStream_t stream);
// du = bf16(t > 0 ? v : 0), RNE (f32_to_bf16_rne's arithmetic), written as a one-plane blocked tensor [n][c/8][h][w][8]: v fp32
// NHWC, t a one-plane blocked bf16 tensor (conv-A's output of a precision-1 plan)
hipError_t launch_mask_round16(const float* v_nhwc, const void* t_plane, void* du_plane, int n, int h, int w, int c, hipStream_t stream);
hipError_t launch_nadam(float* p, const float* g, float* m, float* v, size_t count, float lr, float b1, float b2, float eps,
                        float mc_t, float mc_t1, float ms_new, float ms_next, float b2_pow_t, hipStream_t stream);
// The data-parallel / gradient-accumulation step: g = (float)(sum over r, in order, of counts.n[r] * g_shards[r * shard_stride + i],
// in double, / the sum of the counts), then launch_nadam's arithmetic on g; g_mean (or NULL) receives g.  A shard whose count is
// 0 is never read.  The counts travel as a kernel argument.  The caller has checked the arguments (dsen2_nadam_step_shards:
// shards in 1..kMaxShards, every count in [0, 2^24), a positive total, shard_stride >= count); nothing is checked again here.
constexpr int kMaxShards = 64;
struct ShardCounts {
  int n[kMaxShards];
};
hipError_t launch_nadam_shards(float* p, const float* g_shards, size_t shard_stride, int shards, const ShardCounts& counts, float* g_mean,
                               float* m, float* v, size_t count, float lr, float b1, float b2, float eps, float mc_t, float mc_t1,
                               float ms_new, float ms_next, float b2_pow_t, hipStream_t stream);
// dst[i] = map[i] ? src[map[i] - 1] : 0   /   flat[map[i] - 1] = packed[i] where map[i] != 0
hipError_t launch_gather(float* dst, const float* src, const int* map, size_t n, hipStream_t stream);
hipError_t launch_scatter(float* flat, const float* packed, const int* map, size_t n, hipStream_t stream);
// The repack of a precision-2 model, whose packed buffers mix bf16 (hi, lo) planes and fp32 words: one map entry per 16-bit
// half of the `words` 32-bit words of a layer's buffer, 0 = zero, else 4 * (1 + index into the layer's keras-flat values) +
// kind (kGatherHi = RNE bf16 of the value, kGatherLo = RNE bf16 of (value - hi), kGatherF32Low / High = the halves of the fp32
// bit pattern) — the host packers' arithmetic (f32_to_bf16_rne).  `layers` layers with the same map: dst_stride words /
// src_stride floats apart.
enum : int { kGatherHi = 0, kGatherLo = 1, kGatherF32Low = 2, kGatherF32High = 3 };
hipError_t launch_gather16(void* dst, const float* src, const int* map, size_t words, int layers, size_t dst_stride, size_t src_stride,
                           hipStream_t stream);

}  // namespace dsen2
