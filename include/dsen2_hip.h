/*
 * dsen2_hip.h — C ABI of libdsen2_hip.so: the MI355X (gfx950) DSen2 / VDSen2 inference path.
 *
 * The reference (ACMEAtronOmatic/DSen2) is pure Python and has no FFI layer; the "operator API"
 * below the drop-in boundary is keras' Model object.  Each entry point names the reference
 * interface it stands in for (paths relative to the reference checkout).
 *
 * Conventions
 *   - plain C types only; every `const float* dev_*` / `float* dev_*` is a DEVICE pointer owned by
 *     the caller (e.g. a PyTorch-ROCm tensor's data_ptr()); `host_*` pointers are host memory.
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream).  All work is enqueued on
 *     it; nothing synchronises unless stated.
 *   - every function returns DSEN2_OK (0) or a negative error code and never throws;
 *     dsen2_last_error() returns a thread-local description of the last failure.
 *   - the library uses the calling thread's current HIP device; one model handle per device: a handle belongs to the
 *     device that was current when it was created, and every call that takes a handle returns DSEN2_ERR_INVALID when the
 *     calling thread's current device is another one (its weights live on the handle's device).
 *   - no C++ exception crosses the ABI and no path of the library calls abort(): host-side failures (out of memory
 *     included) come back as an error code.  (A fault raised by the GPU itself is the HIP runtime's to report.)
 *   - activations handed across the ABI are NCHW float32 (the reference runs keras in
 *     'channels_first', utils/DSen2Net.py:6); NHWC is internal.
 */
#ifndef DSEN2_HIP_H
#define DSEN2_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DSEN2_OK 0
#define DSEN2_ERR_INVALID (-1)     /* bad argument / unsupported shape */
#define DSEN2_ERR_HIP (-2)         /* a HIP runtime call failed */
#define DSEN2_ERR_NO_WEIGHTS (-3)  /* forward before load_weights */
#define DSEN2_ERR_WORKSPACE (-4)   /* workspace too small */
#define DSEN2_ERR_NO_DEVICE (-5)   /* no gfx950 device visible */
#define DSEN2_ERR_NOMEM (-6)       /* the HOST ran out of memory inside the library (std::bad_alloc) — not a caller error */
#define DSEN2_ERR_INTERNAL (-7)    /* any other C++ exception caught at the boundary (a library bug, never a caller error) */
/* Shape limit of every entry point that takes (n, h, w): ONE image's activation tensor must stay below 2^31 bytes
 * (h * w * feature_size < 2^29 values) — the kernels address an image through a 32-bit buffer descriptor.  Checked up
 * front (DSEN2_ERR_INVALID before anything is enqueued), the same for all three precisions; there is no limit on n. */

typedef struct dsen2_model dsen2_model;

const char *dsen2_version(void);
const char *dsen2_last_error(void);
/* Number of visible HIP devices whose gcnArchName starts with "gfx950"; <0 on error. */
int dsen2_device_count(void);

/* ---- network object -------------------------------------------------------------------------
 * dsen2_model_create  <->  s2model(input_shape, num_layers, feature_size)   utils/DSen2Net.py:18-43
 *   c10/c20/c60: channel counts of the 10 m / 20 m / 60 m inputs (c60 = 0 for the 2-input net).
 *   Accepted: c10 >= 1, c20 >= 1, c60 >= 0, c10 + c20 + c60 <= 16 (the first convolution reads the concatenated inputs as 16
 *   channel lanes, the unused ones zero), num_layers >= 0; anything else is DSEN2_ERR_INVALID and *out stays NULL.
 *   The output has the channel count of the last input and that input is added back (:35-41): so at most 15 output channels
 *   through a model (the single-layer entry dsen2_conv3x3_nhwc takes up to 32).  The Sentinel-2 groupings 4 + 6 (+ 2) have
 *   first-layer kernels of their own; every other grouping runs a generic one (tests/test_gpu_band_groups.py).
 *   feature_size must be 128 or 256 (what the reference uses, testing/supres.py:56,59).
 *   precision: 0 = fp32 everywhere (exact-f32 MFMA); 1 = bf16 operands for the residual-block convolutions
 *   (v_mfma_f32_16x16x32_bf16), fp32 accumulation, an exact fp32 residual stream (kept as two 16-bit planes, see
 *   dsen2_split_f32), the FIRST convolution in the same arithmetic (bf16 operands, fp32 accumulate: dsen2_conv3x3_first_planes;
 *   band groups other than 4 + 6 (+ 2): fp32), fp32 last convolution; 2 = "bf16x3": the first and the residual-block convolutions on the bf16 matrix
 *   cores with every fp32 operand split into two bf16 numbers (x = hi + lo, 16 significant bits) and a product taken as
 *   hi*hi + hi*lo + lo*hi — three MFMAs at 16 x the fp32 MFMA rate, fp32 accumulation, the same exact fp32 residual
 *   stream; whole-network error ~1e-5 in the normalised domain (fp32: 3e-7, precision 1: 4e-3), inside the 1e-4 gate.
 *   Opt-in: it is not the reference's arithmetic (keras computes in fp32) and never the headline benchmark's.
 *   A model's kernel structures are fixed when it is created; the only process-global state of the library are
 *   per-(kernel, device) launch attributes, set once under a mutex — any number of handles (one per rank / device)
 *   coexist, and host threads may drive different devices, or one handle from several streams (each call with
 *   its own workspace), concurrently.
 */
int dsen2_model_create(dsen2_model **out, int c10, int c20, int c60, int num_layers, int feature_size,
                       int precision);
void dsen2_model_destroy(dsen2_model *m);

/* Number of float32 parameters in keras order (kernels HWIO (3,3,Cin,Cout) then bias, per Conv2D,
 * in graph order: conv_in, d x (convA, convB), conv_out). */
size_t dsen2_model_num_params(const dsen2_model *m);

/* dsen2_model_load_weights  <->  model.load_weights(predict_file)        testing/supres.py:63
 *   host_flat: `count` float32 in the order above (what a keras-HDF5 -> flat converter emits).
 *   Packs into the MFMA operand layout and uploads; synchronises the device once. */
int dsen2_model_load_weights(dsen2_model *m, const float *host_flat, size_t count);

/* Scratch the caller must provide to dsen2_model_forward for a batch of n patches of h x w. */
int dsen2_model_workspace_bytes(const dsen2_model *m, int n, int h, int w, size_t *bytes);

/* dsen2_model_forward  <->  model.predict([p10, p20(, p60)])             testing/supres.py:65
 *   dev_x10 [n,c10,h,w], dev_x20 [n,c20,h,w], dev_x60 [n,c60,h,w] or NULL, dev_out [n,cout,h,w];
 *   all NCHW float32 device pointers, all at the same (already up-sampled) h x w. */
int dsen2_model_forward(dsen2_model *m, const float *dev_x10, const float *dev_x20, const float *dev_x60,
                        float *dev_out, int n, int h, int w, void *dev_workspace, size_t workspace_bytes,
                        void *stream);

/* How many kernel launches the 2*num_layers residual-block convolutions of one forward of n patches of h x w take on
 * the current device: 2*num_layers (one per convolution), or 1 — a precision-1 or -2 model runs them as ONE persistent
 * "chain" launch when the batch gives every CU whole patches (each workgroup then owns its patches through all layers;
 * e.g. 256 patches of 32x32 on 256 CUs) and the patches are at most 64 x 64 (beyond that the per-layer launches are
 * measured faster).  Same results either way, bit for bit.  <0 on error. */
int dsen2_model_body_launches(const dsen2_model *m, int n, int h, int w);

/* Measurement hook (no reference counterpart): `iters` forward passes exactly as dsen2_model_forward enqueues them,
 * with a HIP event recorded on `stream` before the first and after the last residual-block convolution of each
 * pass.  *body_ms_per_launch = that interval / (2*num_layers): the mean duration of ONE of those convolutions inside
 * the running network, whether they are 2*num_layers launches or one chain launch (bench.py's roofline figure).
 * Synchronises the stream. */
int dsen2_model_forward_timed(dsen2_model *m, const float *x10, const float *x20, const float *x60, float *out,
                              int n, int h, int w, void *workspace, size_t workspace_bytes, void *stream, int iters,
                              float *body_ms_per_launch);

/* Measurement hook (no reference counterpart): `warm` plain forward passes, then — without a synchronisation in between,
 * so that the GPU never idles and is at its steady clock — `iters` forward passes exactly as dsen2_model_forward enqueues
 * them, each with FOUR HIP events recorded on `stream`: before the first convolution, before the first and after the last
 * residual-block convolution, after the output convolution.  ms5[0] = mean whole forward, ms5[1] = first convolution,
 * ms5[2] = all residual-block convolutions together, ms5[3] = output convolution — consecutive intervals between the same
 * time stamps, so ms5[1] + ms5[2] + ms5[3] = ms5[0]; ms5[4] = mean time per instrumented pass from the first pass's first
 * event to the last pass's last event (what a pass costs WITH its event records and the gap to the next pass).
 * bench.py's `roofline` object is built from these.  Synchronises the stream at the end. */
int dsen2_model_forward_profile(dsen2_model *m, const float *x10, const float *x20, const float *x60, float *out,
                                int n, int h, int w, void *workspace, size_t workspace_bytes, void *stream, int warm,
                                int iters, float *ms5);

/* ---- dihedral: the 8 flips and rotations of a patch; the geometric self-ensemble ("EDSR+") -----------------------------
 * No reference counterpart (the reference neither augments nor ensembles); opt-in everywhere.
 * Convention: op = k + 4 f with k in 0..3, f in 0..1, and for a [..., H, W] array a
 *     D_op(a)    = np.rot90(a[..., ::-1] if f else a, k, axes=(-2, -1))          (counter-clockwise; odd k swaps H and W)
 *     D_op^-1(b) = t[..., ::-1] if f else t,  t = np.rot90(b, -k, axes=(-2, -1))
 * One kernel family (csrc/dihedral.hip): 32 x 32 tiles through LDS, reads and writes coalesced for all 8 ops, ragged edges by
 * bounds, no atomics, any pointer alignment (16-byte reads where the width and the pointer allow; same bits).
 *
 * dsen2_dihedral_nchw: dev_out = D_op(dev_in), or D_op^-1(dev_in) when `inverse`; dev_in [n,c,h,w] float32, dev_out [n,c,h,w]
 *   or [n,c,w,h] (odd k).  Pure data movement: every bit pattern survives.  dev_ops (or NULL): int32 device array [n], sample s
 *   takes op dev_ops[s] & 7 instead of `op` (which must still be 0..7); needs h == w.
 * dsen2_dihedral_accumulate: dev_acc = dev_acc + D_op^-1(dev_in) in fp32; h, w are those of dev_acc, dev_in is [n,c,w,h] for
 *   odd k.  count_or_0 > 0: dev_acc = (dev_acc + D_op^-1(dev_in)) / (float)count_or_0, a correctly rounded fp32 divide.
 * Both: DSEN2_ERR_INVALID (nothing launched) for a NULL pointer, op outside 0..7, a negative count, 2^31 elements or more,
 *   dev_ops with h != w, an output that overlaps the input.  n == 0 returns DSEN2_OK.
 *
 * dsen2_model_forward_ensemble: the mean over the members selected by `mask` (bit op = member op, 1..255) of
 *   y_op = D_op^-1(forward(D_op x)).  Members run in ascending op order; the running sum is s = y_first, then s = s + y_next in
 *   fp32, and after the last member s = s / (float)count (not computed for one member).  Member 0 is the plain forward written
 *   straight into dev_out: mask = 1 is dsen2_model_forward bit for bit, at its cost and with its workspace.
 *   Workspace (dsen2_model_ensemble_workspace_bytes, same mask): the forward's, plus — for any member but 0 — the turned inputs
 *   and one member's output.  The library allocates nothing.  DSEN2_ERR_INVALID for mask 0 or above 255, a NULL pointer,
 *   dev_out overlapping an input, an image beyond the forward's limit in either orientation, 2^31 elements or more in a tensor;
 *   DSEN2_ERR_WORKSPACE for a short workspace; n == 0 returns DSEN2_OK.
 *   The accuracy gain of the ensemble has not been measured in this project (it needs the trained checkpoints). */
int dsen2_dihedral_nchw(const float *dev_in, float *dev_out, int n, int c, int h, int w, int op, const int *dev_ops_or_null,
                        int inverse, void *stream);
int dsen2_dihedral_accumulate(const float *dev_in, float *dev_acc, int n, int c, int h, int w, int op, int count_or_0,
                              void *stream);
int dsen2_model_ensemble_workspace_bytes(const dsen2_model *m, int n, int h, int w, int mask, size_t *bytes);
int dsen2_model_forward_ensemble(dsen2_model *m, const float *dev_x10, const float *dev_x20, const float *dev_x60,
                                 float *dev_out, int n, int h, int w, int mask, void *dev_workspace, size_t workspace_bytes,
                                 void *stream);

/* ---- single-layer entry points (kernel-level parity tests and benchmarks) -------------------
 * One 3x3 'same' convolution (keras Conv2D as used at utils/DSen2Net.py:10,12,29,35) on NHWC
 * float32 device tensors.  host_kernel is HWIO (3,3,cin,cout), host_bias is [cout].
 *   epilogue 0: out = relu(conv + bias)                         DSen2Net.py:10-11 / :29
 *   epilogue 1: out = dev_aux + res_scale * (conv + bias)       DSen2Net.py:12-15   (aux NHWC [n,h,w,cout])
 *   epilogue 2: out = conv + bias + dev_aux, NCHW out and aux   DSen2Net.py:35,38,41 (aux/out [n,cout,h,w])
 * cin must be a multiple of 16 (zero-pad channels), cout a multiple of 128 for epilogues 0/1 and
 * <= 32 for epilogue 2.  Packs the weights on every call (test path, not the hot path). */
int dsen2_conv3x3_nhwc(const float *dev_in, const float *host_kernel, const float *host_bias,
                       const float *dev_aux, float *dev_out, int n, int h, int w, int cin, int cout,
                       int epilogue, float res_scale, void *stream);

/* The same convolution on the one-tile-per-workgroup kernel (the library's first, register-staged structure):
 * an independent implementation of the arithmetic for cross-checks of the persistent DMA-fed kernels
 * (tests/test_gpu_conv.py, tools/stress_body_conv.py).  Bit-identical results are expected. */
int dsen2_conv3x3_nhwc_ref(const float *dev_in, const float *host_kernel, const float *host_bias,
                           const float *dev_aux, float *dev_out, int n, int h, int w, int cin, int cout,
                           int epilogue, float res_scale, void *stream);

/* 16-bit tensors of a precision-1 model are BLOCKED: [n][C/8][h][w][8] — an 8-channel block is a plane of
 * 16-byte pixels (the layout in which the bf16 kernel's loads, stores and LDS-DMA reads are contiguous runs).
 *
 * The residual stream of such a model: each fp32 value u (its bit pattern) is held in two blocked 16-bit tensors,
 *   hi = (u + 0x8000) >> 16   the bf16 rounding of u (ties away from zero) = the next convolution's operand
 *   lo = u & 0xffff
 * and u = ((hi - (lo >> 15)) << 16) | lo restores it bit for bit (all arithmetic mod 2^16 / 2^32; every bit
 * pattern, NaNs included, round-trips).  dsen2_split_f32: fp32 NHWC [n,h,w,c] -> blocked hi, lo (n*h*w*c uint16
 * each); dsen2_join_f32 is the inverse.  c % 8 == 0, c <= 512. */
int dsen2_split_f32(const float *dev_in_nhwc, void *dev_hi, void *dev_lo, int n, int h, int w, int c, void *stream);
int dsen2_join_f32(const void *dev_hi, const void *dev_lo, float *dev_out_nhwc, int n, int h, int w, int c, void *stream);

/* bf16-operand form of one residual-block convolution (feat -> feat, feat = 128 or 256): dev_in_bf16 is a BLOCKED
 * bf16 tensor; the fp32 HWIO kernel is rounded to bf16 (RNE) while packing; accumulation is fp32, starting from the bias.
 *   epilogue 0: dev_out (bf16 blocked, RNE) = relu(conv + bias)                           DSen2Net.py:10-11
 *   epilogue 1: (dev_res_hi, dev_res_lo) = split(join(hi, lo) + res_scale * (conv + bias)), in place; dev_out unused
 *   epilogue 3: dev_out (fp32 NHWC) = join(hi, lo) + res_scale * (conv + bias)            DSen2Net.py:12-15
 * Test path (packs on every call, synchronises). */
int dsen2_conv3x3_body_bf16(const void *dev_in_bf16, const float *host_kernel, const float *host_bias,
                            void *dev_res_hi, void *dev_res_lo, void *dev_out, int n, int h, int w, int feat,
                            int epilogue, float res_scale, void *stream);

/* precision 2 ("bf16x3") at kernel level.  16-bit OPERAND tensors carry two blocked planes per image:
 * [n][2][C/8][h][w][8], plane 0 = hi (bf16), plane 1 = lo (bf16), value ~ hi + lo.
 * dsen2_split3_f32: fp32 NHWC [n,h,w,c] -> the residual stream of a precision-2 model: dev_hx (two planes: hi = the bf16
 *   rounding of the bit pattern, ties away, as in dsen2_split_f32; xl = bf16(x - hi), round to nearest even) and dev_lo
 *   ([n][c/8][h][w][8], the low halves: (hi, lo) restore x bit for bit with dsen2_join_f32 applied to plane 0).
 * dsen2_conv3x3_body_bf16x3: one residual-block convolution, feat -> feat; the fp32 HWIO kernel is split into (wh, wl) while
 *   packing; dev_in_planes is a two-plane operand tensor.
 *   epilogue 0: dev_out (two planes, RNE both) = relu(conv + bias)
 *   epilogue 1: the stream (dev_res_hx planes hi | xl, dev_res_lo) <- split3(join(hi, lo) + res_scale * (conv + bias)), in place
 *   epilogue 3: dev_out (fp32 NHWC) = join(hi, lo) + res_scale * (conv + bias)
 * Test path (packs on every call, synchronises). */
int dsen2_split3_f32(const float *dev_in_nhwc, void *dev_hx, void *dev_lo, int n, int h, int w, int c, void *stream);
int dsen2_conv3x3_body_bf16x3(const void *dev_in_planes, const float *host_kernel, const float *host_bias,
                              void *dev_res_hx, void *dev_res_lo, void *dev_out, int n, int h, int w, int feat,
                              int epilogue, float res_scale, void *stream);

/* The FIRST convolution of a precision-1 / -2 model at kernel level (utils/DSen2Net.py:24-29: Concatenate(axis=1) of the
 * NCHW inputs + Conv2D(feat, 3x3, 'same') + bias + ReLU) on the bf16 matrix cores, writing the residual stream in the form the
 * residual-block kernels read.  Band groups 4 + 6 (+ 2) only; host_kernel HWIO (3, 3, c10 + c20 + c60, feat).
 *   precision 1: out = relu(sum bf16(x) * bf16(w) + bias) (RNE roundings, fp32 accumulate);
 *                dev_out / dev_out2 = its blocked (hi, lo) planes — dsen2_split_f32's tensors
 *   precision 2: x = xh + xl, w = wh + wl (bf16 each), products xh*wh + xh*wl + xl*wh in fp32;
 *                dev_out = hx (two planes per image: hi | xl), dev_out2 = lo16 — dsen2_split3_f32's tensors
 * Test path (packs on every call, synchronises). */
int dsen2_conv3x3_first_planes(const float *dev_x10, const float *dev_x20, const float *dev_x60, int c10, int c20, int c60,
                               const float *host_kernel, const float *host_bias, int feat, int precision,
                               void *dev_out, void *dev_out2, int n, int h, int w, void *stream);

/* Body-convolution micro-benchmark hook: runs `iters` launches of the 128->128 (or F->F) kernel on
 * caller-provided NHWC buffers with already-packed weights held by `m` (layer index `layer`, 1-based
 * body conv number), after 24 untimed launches of the same kernel (the chip's clock after an idle stretch), and reports the
 * mean kernel time in milliseconds measured with HIP events on `stream`.  Used by bench.py (each epilogue alone on dense
 * random operands, beside the in-network figure).
 * precision-1 models: dev_in is bf16 blocked; odd layers write bf16 blocked to dev_out; even (residual) layers take
 * dev_aux = one fp32-sized buffer holding the blocked hi tensor followed by the lo tensor and update it in place
 * (the last block's residual layer writes fp32 NHWC to dev_out instead). */
int dsen2_model_time_body_conv(dsen2_model *m, int layer, const float *dev_in, const float *dev_aux,
                               float *dev_out, int n, int h, int w, int iters, void *stream,
                               float *ms_per_launch);

/* ---- training (fp32 and bf16x3 models) --------------------------------------------------------
 * The counterpart of training/supres_train.py's model.fit: MAE loss (keras mean_absolute_error, MSE as a metric), the
 * gradients of every parameter, keras-2 Nadam.  Precision 0 and 2 handles train; every training entry returns
 * DSEN2_ERR_INVALID ("training needs an fp32 model or a bf16x3 one") for a precision-1 handle.  No float atomics: the same
 * inputs give the same bits, run to run.
 * A precision-2 model trains in its own arithmetic: the forward on the bf16x3 per-layer kernels (never the chain kernel),
 * the residual blocks' input gradients on the same kernels with flipped, transposed weights, their weight gradients on
 * dsen2_conv3x3_wgrad_bf16x3's kernel; the first and the output convolution's gradients stay on the fp32 kernels.  The
 * master weights, the gradient, the optimizer state and dsen2_model_get_weights' vector are fp32 keras-flat in every
 * precision; after each dsen2_model_set_weights_device the packed (wh, wl) planes are the host packers' bits.
 * Host memory: the packed planes of a precision-2 model with residual blocks hold 16 significant bits per weight, so
 * dsen2_model_load_weights keeps a host copy of the fp32 vector it was given (4 * num_params bytes, 151 MB for VDSen2) for
 * dsen2_model_get_weights and the first training call, which moves it to the device and frees it.  An inference-only
 * precision-2 model carries that copy until dsen2_model_destroy.
 * A precision-2 model without residual blocks (num_layers 0) is fp32 in every layer (dsen2_model_create) and trains exactly
 * as the precision-0 model of the same shape does.
 * Mixed precision: dsen2_model_set_train_precision(m, 1) makes the training step of an fp32 (precision-0) model run on bf16
 * operands with fp32 accumulation — the arithmetic of a precision-1 model — while the model itself, its master weights, the
 * gradient, the optimizer state, dsen2_model_get_weights' vector and dsen2_model_forward stay fp32.  0 (the default) is the
 * model's own arithmetic.  DSEN2_ERR_INVALID for a precision-1 or precision-2 handle and for any other value.  Changing the
 * setting drops the training state and rebuilds it (the master copy comes back from the packed fp32 weights, exactly);
 * dsen2_model_train_workspace_bytes and dsen2_model_gradients follow it.  With train precision 1:
 *   - the state owns a precision-1 plan of the same network, whose packed buffers (what a precision-1 model of these weights
 *     holds: weights rounded to bf16, round to nearest even) are rebuilt from the master vector after every
 *     dsen2_model_set_weights_device / dsen2_model_load_weights, next to the model's own fp32 buffers;
 *   - dev_out_or_NULL receives the forward of a precision-1 model with the same weights run layer by layer: the first
 *     convolution on bf16(x), bf16(w) (round to nearest even; band groups other than 4 + 6 (+ 2): in fp32, as in every
 *     precision-1 model, dsen2_model_create); each block t = bf16(relu(convA(hi(x)) + b)) (nearest even),
 *     x += 0.1 * (convB(t) + b) in fp32, hi(x) = the stream's operand plane (u + 0x8000) >> 16 of the fp32 bit pattern u
 *     (nearest, ties away from zero); the output convolution in fp32;
 *   - backward through the blocks, g = dL/dx in fp32: dWB = 0.1 * wgrad(t, hi(g)), dbB = 0.1 * sum hi(g),
 *     du = bf16([t > 0] * 0.1 * dgradB(hi(g))) (nearest even), dWA = wgrad(hi(x), du), dbA = sum du, g += dgradA(du); every
 *     product is one bf16 MFMA with fp32 accumulation.  bf16 has fp32's exponent range: no loss scaling.
 *   - the loss, the output convolution's gradients and the first convolution's weight gradient (on the fp32 inputs, the
 *     ReLU mask from the fp32 x_0) are the fp32 kernels'.
 * Without residual blocks the setting changes nothing: such a plan is fp32 in every layer.
 *
 * dsen2_model_train_workspace_bytes: scratch dsen2_model_gradients needs for n patches of h x w (the saved activations
 *   x0 .. x_d and t_1 .. t_d, two gradient tensors, the weight-gradient partials; ~1 GB for DSen2 at 128 x 32 x 32).
 * dsen2_model_gradients: one forward with every activation kept and its backward.  x10 / x20 / x60 as dsen2_model_forward,
 *   target [n,cout,h,w] NCHW; dev_out_or_NULL receives the forward output (bit-identical to dsen2_model_forward's), or NULL;
 *   dev_grad_flat [num_params] receives dLoss/dParameter in keras-flat order (the order dsen2_model_load_weights takes);
 *   dev_loss2 (or NULL) receives [mean |out - target|, mean (out - target)^2].  dL/dout = sign(out - target) / (n*cout*h*w),
 *   sign(0) = 0; the ReLU gradient passes where the saved ReLU output is > 0.
 * dsen2_model_get_weights: the model's weights, keras-flat, into dev_flat [num_params].
 * dsen2_model_set_weights_device: new keras-flat weights from device memory, repacked on the device (no host round trip);
 *   dsen2_model_forward uses them afterwards.  Bit-identical to dsen2_model_load_weights of the same values.
 * dsen2_nadam_step: keras 2.2 Nadam on `count` parameters p with gradients g and state m, v (updated in place).  The
 *   per-step scalars come from the host, t = the 1-based step, sd = schedule_decay, m_schedule starting at 1:
 *     mc_t = b1 (1 - 0.5 * 0.96^(t sd)),  mc_t1 = b1 (1 - 0.5 * 0.96^((t+1) sd)),  ms_new = m_schedule * mc_t,
 *     ms_next = ms_new * mc_t1,  b2_pow_t = b2^t;
 *   g' = g / (1 - ms_new), m = b1 m + (1 - b1) g, m' = m / (1 - ms_next), v = b2 v + (1 - b2) g^2, v' = v / (1 - b2_pow_t),
 *   p -= lr ((1 - mc_t) g' + mc_t1 m') / (sqrt(v') + eps).
 * dsen2_nadam_step_shards: the step of data-parallel training and of gradient accumulation: the count-weighted mean of `shards`
 *   gradient vectors and dsen2_nadam_step on it, in one pass.  dev_g_shards holds the vectors, `count` floats each, vector r at
 *   dev_g_shards + r * shard_stride (shard_stride >= count, in floats); host_counts[r] >= 0 (host memory, copied into the launch:
 *   it may be reused at once) is the number of samples behind vector r, total = their sum > 0.  Per parameter i, in this order:
 *     acc = 0 (double);  for r = 0 .. shards-1 with host_counts[r] > 0:  acc = acc + (double)host_counts[r] * (double)g_r[i];
 *     g = (float)(acc / (double)total);  then dsen2_nadam_step's arithmetic on g.
 *   The order is fixed, so the same inputs give the same bits on every run and on every rank of a data-parallel group.  A count
 *   below 2^24 times a float is exact in double, so a fused multiply-add and a multiply followed by an add round alike.  With one
 *   shard acc / total is g_0[i] for any count: the call is dsen2_nadam_step, bit for bit.  A vector whose count is 0 is never
 *   read: its slot may hold anything.  dev_g_mean_or_NULL [count] receives g.  dev_g_shards is not modified.  16-byte accesses
 *   are used when every pointer is 16-byte aligned and (with more than one shard) shard_stride is a multiple of 4; any other
 *   alignment and stride gives the same bits, more slowly.  DSEN2_ERR_INVALID, nothing launched: shards outside 1..64, a negative
 *   count, a count >= 2^24, a zero total, shard_stride < count, a NULL pointer.
 * dsen2_conv3x3_wgrad: the weight-gradient kernel alone (kernel-level tests): dev_dw (3,3,ci,co) = scale * sum over all pixels
 *   of a[p + tap][c] g[p][o], dev_db [co] = scale * sum g[p][o]; dev_a NHWC [n,h,w,ca], dev_g NHWC [n,h,w,cg]; ci <= ca, co <= cg.
 *   Shapes: cg a multiple of 128 (ca a multiple of 4), or cg <= 32 with ca a multiple of 128.  Lanes ci .. ca-1 of dev_a and
 *   co .. cg-1 of dev_g are read but reach neither dev_dw nor dev_db (each element of dW sums the products of ONE lane of a with
 *   ONE lane of g): they may hold anything.  Allocates its scratch and synchronises (test path). */
int dsen2_model_train_workspace_bytes(const dsen2_model *m, int n, int h, int w, size_t *bytes);
int dsen2_model_gradients(dsen2_model *m, const float *x10, const float *x20, const float *x60, const float *target,
                          float *dev_out_or_NULL, float *dev_grad_flat, float *dev_loss2, int n, int h, int w, void *ws,
                          size_t ws_bytes, void *stream);
int dsen2_model_set_train_precision(dsen2_model *m, int precision);
int dsen2_model_get_weights(const dsen2_model *m, float *dev_flat, void *stream);
int dsen2_model_set_weights_device(dsen2_model *m, const float *dev_flat, void *stream);
int dsen2_nadam_step(float *p, const float *g, float *m, float *v, size_t count, float lr, float b1, float b2, float eps,
                     float mc_t, float mc_t1, float ms_new, float ms_next, float b2_pow_t, void *stream);
int dsen2_nadam_step_shards(float *p, const float *dev_g_shards, size_t shard_stride, int shards, const int *host_counts,
                            float *dev_g_mean_or_NULL, float *m, float *v, size_t count, float lr, float b1, float b2, float eps,
                            float mc_t, float mc_t1, float ms_new, float ms_next, float b2_pow_t, void *stream);
int dsen2_conv3x3_wgrad(const float *dev_a, const float *dev_g, float *dev_dw, float *dev_db, int n, int h, int w, int ca,
                        int cg, int ci, int co, float scale, void *stream);

/* ---- the optimiser step with options (csrc/optimizer_step.hip) -------------------------------
 * dsen2_optimizer_step: dsen2_nadam_step_shards with a choice of update rule, gradient clipping and decoupled weight decay.  p,
 *   dev_g_shards, shard_stride, shards, host_counts, dev_g_mean_or_NULL, m and count are that entry's, with its arithmetic for the
 *   mean gradient g (added in row order in double, a row whose count is 0 never read, dev_g_shards not modified); dev_g_mean_or_NULL
 *   receives the mean BEFORE clipping.  The descriptor is host memory, read during the call (it and host_ranges may be reused at
 *   once); its scalars are floats, widened to double in the kernel.  Every operation below is done in double and rounded on its own
 *   (no fused multiply-add; double sqrt and divide are correctly rounded), left to right; (float) marks a rounding to float32.
 *   Clipping, keras 2.2 get_gradients:
 *     clipnorm c > 0:  sq = the sum over all `count` parameters of (double)g * (double)g, in an order fixed by `count` alone (the
 *       grid, per-thread order, workgroup tree and one-block finish of dsen2_loss_sums: blocks = min(max(ceil(count / 2048), 1),
 *       4096), thread j of all adds elements j, j + 256 blocks, ... onto 0.0); n = sqrt(sq); s = n >= c ? c / n : 1.0;
 *       g = (float)((double)g * s).  One norm over all tensors.  n stays in device memory: the host never waits for it.
 *     clipvalue cv > 0, after clipnorm:  g = g < -cv ? -cv : g > cv ? cv : g  (a NaN passes).
 *   Update, with p_old the parameter before it:
 *     kind 0  Nadam: dsen2_nadam_step's arithmetic on g with lr, b1, b2, eps, mc_t, mc_t1, ms_new, ms_next, b2_pow_t.
 *     kind 1  Adam (keras 2.2, no amsgrad), lr_t = lr sqrt(1 - b2^t) / (1 - b1^t) computed by the host in double:
 *               m = (float)(b1 m + (1 - b1) g);  v = (float)(b2 v + (1 - b2) g g);  p = (float)(p - lr_t m / (sqrt(v) + eps)).
 *     kind 2  SGD (keras 2.2) with momentum mu and optional Nesterov; the velocity lives in m, v is neither read nor written
 *             and may be NULL:
 *               vel = (float)(mu m - lr g);  m = vel;  p = (float)(p + vel)   or, nesterov != 0,   p = (float)(p + mu vel - lr g).
 *   Decay, weight_decay wd > 0 (decoupled, as AdamW), after the update:  p = (float)((double)p - lr wd p_old)  for every parameter
 *   whose index lies in one of the n_ranges half-open ranges [host_ranges[2k], host_ranges[2k+1]), sorted and disjoint; every
 *   other parameter is not decayed.  With n_ranges == 0 nothing is.
 *   dev_norm_or_NULL receives n, the global norm of the unclipped mean gradient, whenever it is non-NULL, with or without
 *   clipnorm.  dev_work: scratch of dsen2_optimizer_step_work_bytes(desc, count, shards, dev_g_mean != NULL, dev_norm != NULL)
 *   bytes on a 16-byte boundary: 0 bytes (dev_work may be NULL) unless clipnorm > 0 or dev_norm is given; then the partial sums
 *   and, with more than one shard and no dev_g_mean, the mean gradient.  With one shard the mean is the row itself and no copy of
 *   it is made.  16-byte accesses under dsen2_nadam_step_shards' alignment rule, the same bits otherwise.
 *   With kind 0, no clipping and no decay the result is dsen2_nadam_step_shards' bit for bit.
 *   DSEN2_ERR_INVALID, nothing launched and nothing written: a kind outside 0..2; clipnorm, clipvalue, weight_decay or momentum
 *   negative, NaN or infinite; momentum >= 1; n_ranges outside 0..128 or ranges without host_ranges; a range that is empty,
 *   starts before its predecessor's end or ends behind count; shards outside 1..64; v NULL for kinds 0 and 1; scratch that is
 *   NULL, misaligned or too small; and every refusal of dsen2_nadam_step_shards. */
typedef struct dsen2_optimizer_desc {
  int kind;                                      /* 0 Nadam, 1 Adam, 2 SGD */
  float lr, b1, b2, eps;
  float mc_t, mc_t1, ms_new, ms_next, b2_pow_t;  /* Nadam's per-step scalars */
  float lr_t;                                    /* Adam's */
  float momentum;                                /* SGD's, in [0, 1) */
  int nesterov;
  float clipnorm, clipvalue;                     /* 0 = off */
  float weight_decay;                            /* 0 = off */
  int n_ranges;
  const unsigned *host_ranges;                   /* [2 * n_ranges] */
} dsen2_optimizer_desc;
int dsen2_optimizer_step_work_bytes(const dsen2_optimizer_desc *desc, size_t count, int shards, int have_g_mean, int want_norm,
                                    size_t *bytes);
int dsen2_optimizer_step(const dsen2_optimizer_desc *desc, float *p, const float *dev_g_shards, size_t shard_stride, int shards,
                         const int *host_counts, float *dev_g_mean_or_NULL, float *m, float *v_or_NULL, size_t count,
                         void *dev_work, size_t work_bytes, double *dev_norm_or_NULL, void *stream);

/* dsen2_conv3x3_wgrad_bf16x3: the weight gradient of a feat -> feat convolution (feat = 128, 256) as bf16x3 on the bf16 matrix
 *   cores, alone (kernel-level tests).  dev_a_planes / dev_g_planes are two-plane operand tensors [n][2][feat/8][h][w][8] bf16
 *   (value = plane 0 + plane 1: dsen2_split3_f32's dev_hx, epilogue 0's dev_out); every product is a0*g0 + a0*g1 + a1*g0 with
 *   fp32 accumulators.  dev_dw (3,3,feat,feat) HWIO, dev_db [feat], both times `scale`.  Allocates its scratch and synchronises.
 * dsen2_conv3x3_wgrad_bf16: the one-plane instance of that kernel (mixed-precision training), alone: dev_a / dev_g are one-plane
 *   blocked bf16 tensors [n][feat/8][h][w][8] (dsen2_split_f32's dev_hi, dsen2_conv3x3_body_bf16's epilogue-0 dev_out); every
 *   product is one bf16 MFMA with fp32 accumulators; dev_db = scale * the sum of dev_g's bf16 values.  The same checks and
 *   refusals as dsen2_conv3x3_wgrad_bf16x3.
 * dsen2_join3_f32: the exact inverse of dsen2_split3_f32: (dev_hx plane 0, dev_lo16) -> fp32 NHWC [n,h,w,c], bit for bit
 *   (plane 1, xl, is not read). */
int dsen2_conv3x3_wgrad_bf16x3(const void *dev_a_planes, const void *dev_g_planes, float *dev_dw, float *dev_db, int n, int h,
                               int w, int feat, float scale, void *stream);
int dsen2_conv3x3_wgrad_bf16(const void *dev_a, const void *dev_g, float *dev_dw, float *dev_db, int n, int h, int w, int feat,
                             float scale, void *stream);
/* dsen2_conv3x3_wgrad_geometry: what a launch of one of the three weight-gradient kernels does at a shape, computed on the host;
 *   nothing is launched and no device is touched.  kind 0 = dsen2_conv3x3_wgrad (ca, cg as there), 1 = dsen2_conv3x3_wgrad_bf16x3,
 *   2 = dsen2_conv3x3_wgrad_bf16 (ca = cg = feat).  *tiles = the number of 4 x 16 pixel tiles, n * ceil(h / 4) * ceil(w / 16);
 *   *splits = the number of contiguous tile runs, run s = tiles [tiles * s / splits, tiles * (s + 1) / splits), one per workgroup
 *   column; *workspace_floats = the floats of partial sums the launch needs, splits * (9 * cip * cop + 2 * cop) with the
 *   channel counts padded to the kernel's (co, ci) block.  DSEN2_ERR_INVALID for a shape the kernel refuses. */
int dsen2_conv3x3_wgrad_geometry(int kind, int n, int h, int w, int ca, int cg, long long *tiles, int *splits,
                                 size_t *workspace_floats);
int dsen2_join3_f32(const void *dev_hx, const void *dev_lo16, float *dev_out_nhwc, int n, int h, int w, int c, void *stream);

/* ---- losses and the no-data mask (csrc/loss_terms.h, train_ops.hip, error_sums.hip) -----------
 * What dsen2_model_gradients minimises is state on the handle, like the train precision.  kind: 0 MAE (the default), 1 MSE,
 * 2 Huber(delta = param), 3 Charbonnier(epsilon = param).  mask_mode: 0 none (the default); 1 no-data: a pixel (sample, y, x)
 * whose TARGET is exactly 0 in every one of the cout bands carries no ground truth — the rule of "no-data in, no-data out"
 * (csrc/nodata.hip) applied to the target: -0.0 counts as 0, NaN and negative values are data.  A masked pixel adds 0 to both
 * sums of dev_loss2 and has dL/dout = 0 in every band.
 * The denominator is N = n*cout*h*w in EVERY mask mode, never the number of valid elements: a batch's loss and gradient keep the
 * weight of its sample count, so dsen2_nadam_step_shards' count-weighted mean, the ranks of a data-parallel group and epoch sums
 * formed without a host wait stay exact, and every valid pixel of a run weighs the same however many of its neighbours are blank.
 * Arithmetic: e = out - target in float32 (as the MAE always did), d = (double)e; rho' in double, every operation rounded on its
 * own (no FMA; double sqrt and divide are correctly rounded); dL/dout = (float)(rho'(d) * (double)inv), inv = (float)(1.0 / N).
 * delta and epsilon are the (double) of the float32 `param`.  sign(0) = 0.
 *     kind         rho                                   rho'
 *     MAE          |d|                                   sign(d)                 (dL/dout = +-inv: the bits of every earlier release)
 *     MSE          d*d                                   2*d
 *     Huber        |d| <= delta: 0.5*(d*d)               d
 *                  otherwise:    delta*(|d| - 0.5*delta) delta*sign(d)
 *     Charbonnier  s = sqrt(d*d + eps*eps)               d / s
 * dev_loss2 = { (float)(sum rho / N), (float)(sum d*d / N) }, both sums over the unmasked elements in one fixed-order tree; for
 * kind 1 the two are the same bits.
 * dsen2_model_set_loss: sets (kind, param, mask_mode) of a trainable handle.  It does not drop the training state (no workspace
 *   size changes) and does not change dsen2_model_gradients' signature; with (0, anything, 0) every bit of a step is what it was
 *   before this entry existed.  param is read by kinds 2 and 3 alone.  DSEN2_ERR_INVALID, nothing changed: an unknown kind or
 *   mask mode, a param that is not finite or not > 0 for kinds 2 and 3, a precision-1 handle ("training needs an fp32 model or a
 *   bf16x3 one").
 * dsen2_loss_grad: the step's loss kernel alone (kernel-level tests): dev_out, dev_target NCHW [n,c,h,w] float32, c in 1..15;
 *   dev_g_nhwc16 [n*h*w][16] receives dL/dout with lanes >= c zero, dev_loss2 the pair above.  Allocates its scratch and
 *   synchronises.
 * dsen2_loss_sums: the validation pass's sums for a loss kind and mask mode, next to dsen2_abs_sq_error_sums (same grid rule,
 *   element order, trees and finish kernel): dev_out3 = { sum rho(d), sum d*d, number of unmasked elements } as float64 over the
 *   n*c*hw elements of an NCHW [n, c, hw] pair, d = (double)p - (double)t; masked elements add nothing.  The mask re-reads the c
 *   target values of the element's pixel (they sit in L2); there is no mask buffer.  With kind 0 and mask 0 the first two
 *   outputs are dsen2_abs_sq_error_sums' bits.  dev_work: dsen2_loss_sums_workspace_bytes() bytes of device scratch.  Refusals as
 *   there (NULL, n*c*hw outside 1..2^31 - 1: DSEN2_ERR_INVALID; a short workspace: DSEN2_ERR_WORKSPACE) and dsen2_model_set_loss's
 *   for (kind, param, mask_mode). */
int dsen2_model_set_loss(dsen2_model *m, int kind, float param, int mask_mode);
int dsen2_loss_grad(const float *dev_out, const float *dev_target, int n, int c, int h, int w, int kind, float param,
                    int mask_mode, float *dev_g_nhwc16, float *dev_loss2, void *stream);
int dsen2_loss_sums_workspace_bytes(size_t *bytes);
int dsen2_loss_sums(const float *dev_pred, const float *dev_target, int n, int c, long long hw, int kind, float param,
                    int mask_mode, void *dev_work, size_t work_bytes, double *dev_out3, void *stream);

/* ---- the SSIM loss term (csrc/ssim_loss.hip) ---------------------------------------------------
 * Zhao et al. 2017's restoration objective: what dsen2_model_gradients minimises becomes  pointwise loss + T,
 *     T = weight * (1/Nw) * sum over the unmasked windows of (1 - q),      Nw = n*cout*(h-P+1)*(w-P+1),
 * q the SSIM of dsen2_ssim_map (same filter over valid windows, same operation order, float32 promoted to float64) of every
 * window of every (sample, band) plane of out against target, for a normalised separable window g[0 .. P-1] and c1, c2 > 0.
 * A sample's band of q equals dsen2_ssim_map of that plane bit for bit.  With
 *     A1 = 2*mx*my + c1   A2 = 2*(exy - mx*my) + c2   B1 = mx*mx + my*my + c1   B2 = (exx - mx*mx) + (eyy - my*my) + c2
 *     a = 2*my*(A2 - A1)/(B1*B2) - 2*mx*q*(B2 - B1)/(B1*B2)     b = -q/B2     d = 2*A1/(B1*B2)
 * and Gt the transposed ("full") separable filter,  G = Gt a + 2*x*Gt b + y*Gt d  and  dT/dout = -(weight/Nw) * G.  It ADDS to
 * what the pointwise kernel wrote:  g[pixel][band] = (float)((double)g[pixel][band] + scale*G), scale = -(double)weight/Nw: one
 * rounding.  T is added to the loss in double before dev_loss2[0]'s one cast to float; dev_loss2[1] (the MSE) is untouched.
 * Float64 throughout, every operation rounded on its own, taps summed k = 0 .. P-1 in order; csrc/ssim_loss.hip lists every
 * operation, tests/ssim_loss_restatement.py and dsen2_amd/losses.py restate them in numpy.  Sums run in an order the shape alone
 * fixes (no atomics): the same bits on every run.
 * Mask mode 1 (the no-data mask above): a window that holds at least one pixel whose target is 0 in all bands of that sample
 * adds nothing to the sum and has a = b = d = 0, so a masked pixel's SSIM gradient is 0.  Nw stays the number of ALL windows,
 * for the reason N does above.
 * dsen2_model_set_loss_ssim: state on a trainable handle next to dsen2_model_set_loss.  weight 0 (the default): nothing of the
 *   term is launched and every bit of a step is what it was without it (the window and constants are still checked).
 *   DSEN2_ERR_INVALID, nothing changed: a weight that is not finite or < 0; win even or outside 3..11; a window entry that is not
 *   finite; c1 or c2 not finite or not > 0; a precision-1 handle.  With weight > 0 dsen2_model_gradients returns
 *   DSEN2_ERR_INVALID with nothing launched when h < win or w < win.
 * dsen2_ssim_loss_grad: the kernel alone (kernel-level tests): dev_out, dev_target NCHW [n,c,h,w] float32, c in 1..15; it
 *   ACCUMULATES into lanes 0 .. c-1 of dev_g_nhwc16 [n*h*w][16] (the other lanes are not touched) and writes dev_sums2 =
 *   { sum (1 - q) over the unmasked windows, Nw } as float64.  Allocates its scratch and synchronises.
 * dsen2_ssim_loss_sums: the sums alone, for validation: dev_out3 = { sum (1 - q), Nw, unmasked windows } as float64, the first
 *   the bits dsen2_ssim_loss_grad gives.  dev_work: dsen2_ssim_loss_sums_workspace_bytes() bytes of device scratch.  Refusals:
 *   NULL, a bad shape, window or constants, h or w < win: DSEN2_ERR_INVALID; a short workspace: DSEN2_ERR_WORKSPACE. */
int dsen2_model_set_loss_ssim(dsen2_model *m, float weight, const double *host_window, int win, double c1, double c2);
int dsen2_ssim_loss_grad(const float *dev_out, const float *dev_target, int n, int c, int h, int w, float weight,
                         const double *host_window, int win, double c1, double c2, int mask_mode, float *dev_g_nhwc16,
                         double *dev_sums2, void *stream);
int dsen2_ssim_loss_sums_workspace_bytes(size_t *bytes);
int dsen2_ssim_loss_sums(const float *dev_pred, const float *dev_target, int n, int c, int h, int w, const double *host_window,
                         int win, double c1, double c2, int mask_mode, void *dev_work, size_t work_bytes, double *dev_out3,
                         void *stream);

/* ---- tiling / up-sampling / recomposition (utils/patches.py) --------------------------------
 * dsen2_upsample_mirror_bilinear  <->  interp_patches            utils/patches.py:11-16
 *   planes x [h,w] -> planes x [oh,ow]; half-pixel-centre bilinear with mirror boundary (skimage
 *   resize mode='reflect'), including the /30000 .. *30000 round trip — scikit-image 0.18.3's float32 arithmetic operation
 *   by operation: the reference's outputs bit for bit.  The result is then divided by
 *   `post_divisor` (1.0 = exact no-op, 2000 folds `p20 /= SCALE`, testing/supres.py:24). */
int dsen2_upsample_mirror_bilinear(const float *dev_in, float *dev_out, int planes, int h, int w, int oh,
                                   int ow, float post_divisor, void *stream);
/* The same on the general kernel (any scale; samples fetched on demand) whatever the scale — the windowed kernel that
 * up-sampling by 2 or more normally takes must give its bits (kernel-level cross-check, like dsen2_conv3x3_nhwc_ref). */
int dsen2_upsample_mirror_bilinear_ref(const float *dev_in, float *dev_out, int planes, int h, int w, int oh,
                                       int ow, float post_divisor, void *stream);

/* dsen2_tile_gather  <->  the pad + crop loops of get_test_patches{,60}   patches.py:27-28,58-72 / :93-95,127-143
 *   dev_img: one HWC float32 image [H,W,C] (unpadded); writes patches [count,C,P,P] NCHW where patch k
 *   has its origin at (dev_origins[2k], dev_origins[2k+1]) in PADDED coordinates (np.pad mode
 *   'symmetric' by `border`, materialised on the fly).  Values are divided by `divisor`
 *   (1.0 = exact copy, 2000 folds `p10 /= SCALE`, testing/supres.py:23; an IEEE float32 divide, so the
 *   result is bit-identical to numpy's). */
int dsen2_tile_gather(const float *dev_img, int H, int W, int C, int border, const int *dev_origins,
                      int count, int P, float divisor, float *dev_patches, void *stream);

/* dsen2_recompose  <->  recompose_images                          utils/patches.py:374-405
 *   dev_patches [count,C,P,P] NCHW (the "a.shape[0] == 1 -> return a[0] uncropped" quirk of
 *   patches.py:375-376 is a host-side transpose, not this function); writes the HWC image [H,W,C].  Tile grid as the
 *   reference: inner = P - 2*border, x_tiles = ceil(W/inner), y_tiles = ceil(H/inner), row-major patch
 *   order, last row/column origin clamped to size - inner.  The reference's sequential loop lets later
 *   patches overwrite earlier ones where the clamped tile overlaps its neighbour; here every output
 *   pixel reads the LAST patch that covers it, which is the same image without a write race.
 *   Values are multiplied by `scale` (1.0, or 2000 to fold testing/supres.py:29).
 *   Requires count >= x_tiles*y_tiles, H >= inner, W >= inner. */
int dsen2_recompose(const float *dev_patches, int count, int C, int P, int border, float *dev_img, int H,
                    int W, float scale, void *stream);
/* The same for rows [row0, row1) of the image only: the rows a caller can finish (and start downloading) while later patches
 * are still being computed.  Only the patches those rows read need to have been written — for rows below
 * min(t * inner, H - inner), t = number of complete tile rows, those are the first t * x_tiles patches (the last
 * `inner` rows belong to the clamped last tile row).  dev_patches / count describe the whole [count,C,P,P] buffer. */
int dsen2_recompose_rows(const float *dev_patches, int count, int C, int P, int border, float *dev_img, int H,
                         int W, float scale, int row0, int row1, void *stream);

/* ---- tile no-data: which pixels and patches of a tile hold data, and the recomposition that honours it (csrc/nodata.hip) ----------
 * Not in the reference.  Definitions, for a 10 m raster dev_img10 [H,W,C10] (HWC float32) and dsen2_recompose's tile grid
 * (inner = P - 2*border, x_tiles = ceil(W/inner), y_tiles = ceil(H/inner)):
 *   NO-DATA PIXEL    every one of its C10 bands is exactly 0 (-0.0 counts as 0; a NaN or a negative value is data): the sensor's
 *                    fill value.  This is NOT the corpus test "band 0 < 1" below: a dark pixel with one zero band is data.
 *   OWNED RECTANGLE  of tile (ty, tx): the pixels dsen2_recompose takes from that patch — rows [ty*inner, min((ty+1)*inner,
 *                    H-inner)) for ty < y_tiles-1 and [H-inner, H) for the last tile row, columns alike.  They partition the image.
 *   EMPTY PATCH      its owned rectangle holds no pixel with data.
 * dsen2_tile_nodata_geometry (host only, touches no device): the grid and the size of the bitmap, bitmap_words = H * ceil(W/32).
 * dsen2_tile_nodata reads the raster exactly once and writes
 *   dev_patch_empty  uint8 [y_tiles*x_tiles], row-major, 1 = empty;
 *   dev_valid_bits   uint32 [H][ceil(W/32)]: pixel (y, x) is bit x & 31 of word y*ceil(W/32) + (x >> 5), set when the pixel holds
 *                    data; the bits at x >= W are 0.
 *   Two launches on `stream` (the bitmap in a row pass, the flags from the bitmap); compares, wave ballots and ORs only, no
 *   atomics: the result depends on the inputs alone.  Nothing synchronises.
 * dsen2_recompose_rows_nodata is dsen2_recompose_rows with the bitmap and a slot map dev_slot_of_patch (int32 [y_tiles*x_tiles]) in
 *   front of a COMPACT patch buffer dev_patches [slots,C,P,P]: an output pixel whose bit is 0 becomes 0.0f in all C channels and no
 *   patch is read for it; any other pixel reads patch dev_slot_of_patch[k] where dsen2_recompose_rows reads patch k.  A slot outside
 *   [0, slots) is treated as no-data (0 is written, nothing is read): no map can make the kernel read outside dev_patches.  slots
 *   may be 0: every pixel of the rows becomes 0 and dev_patches may be NULL.
 * DSEN2_ERR_INVALID with nothing launched: the geometry dsen2_recompose_rows refuses (inner <= 0, H < inner, W < inner, a row range
 *   outside 0 <= row0 <= row1 <= H), C10 outside 1..16, C < 1, slots < 0, a NULL pointer. */
int dsen2_tile_nodata_geometry(int H, int W, int P, int border, int *x_tiles, int *y_tiles, size_t *bitmap_words);
int dsen2_tile_nodata(const float *dev_img10, int H, int W, int C10, int P, int border, unsigned char *dev_patch_empty,
                      unsigned int *dev_valid_bits, void *stream);
int dsen2_recompose_rows_nodata(const float *dev_patches, int slots, int C, int P, int border, const int *dev_slot_of_patch,
                                const unsigned int *dev_valid_bits, float *dev_img, int H, int W, float scale, int row0, int row1,
                                void *stream);

/* ---- feathered recomposition: a weighted blend in the overlap of neighbouring patches (csrc/recompose_blend.hip) -------------------
 * Not in the reference.  dsen2_recompose_rows with a blend in place of "the last patch wins".  The grid is dsen2_recompose's: along
 * an axis of length L, inner = P - 2*border, T = ceil(L/inner), tile t starts at s_t = t*inner, the last one at L - inner; patch t
 * covers image coordinates [s_t - border, s_t - border + P) (what falls outside [0, L) is padding and is never read).
 *   WEIGHT   for u = x - (s_t - border) in [0, P):  w(u) = clamp(min(u + 1, P - u) - (border - feather), 0, 2*feather); a patch's
 *            weight at a pixel is wy * wx, an integer.  It is positive on [s_t - feather, s_t + inner + feather) only.
 *   OUTPUT   out[y][x][c] = float32( sum_k w_k * p_k[c] / sum_k w_k ) * scale: the sums over the patches with w_k > 0 in ascending
 *            (ty, tx) order, a left fold that starts at its first term, products and sums in float64 (every product is exact), one
 *            float64 division, one rounding to float32, then the float32 multiply by `scale` of dsen2_recompose.
 *   Where one patch carries weight the pixel is that patch's value, bit for bit what dsen2_recompose_rows writes there; at most 3
 *   patches per axis carry weight (3 where the clamped last tile reaches back over two neighbours).  The weights of (P, border,
 *   feather) are those of (P - 2*(border - feather), feather, feather) on patches cropped by border - feather.
 *   One thread per output pixel, no atomics: the image depends on the inputs alone, and any split of [0, H) into row bands gives
 *   the bits of the whole-image call.
 * dev_slot_of_patch and dev_valid_bits (dsen2_tile_nodata; both or neither): dev_patches is the compact buffer [slots,C,P,P]; a
 *   pixel whose bit is 0 becomes 0.0f and reads nothing; a patch whose slot is outside [0, slots) has weight 0 and is never read; a
 *   pixel left without any weighted patch becomes 0.0f.  slots may be 0 (dev_patches may then be NULL).  Without the maps
 *   count_or_slots is the patch count of dsen2_recompose_rows (>= x_tiles*y_tiles).
 * DSEN2_ERR_INVALID with nothing launched: the geometry dsen2_recompose_rows refuses (inner <= 0, H < inner, W < inner, too few
 *   patches, a row range outside 0 <= row0 <= row1 <= H), border > P/4, feather outside 1..border, C < 1, a negative count, a NULL
 *   pointer, one of the two maps without the other. */
int dsen2_recompose_rows_blend(const float *dev_patches, int count_or_slots, int C, int P, int border, int feather,
                               const int *dev_slot_of_patch, const unsigned int *dev_valid_bits, float *dev_img, int H, int W,
                               float scale, int row0, int row1, void *stream);

/* dsen2_down_pixel_aggr  <->  downPixelAggr                       utils/patches.py:353-371
 *   dev_img: one HWC image [H,W,C] of uint16 or float32 samples; writes the HWC image [H/scale, W/scale, C] as float32
 *   (out_f64 = 0) or float64 (1).  scipy.ndimage.gaussian_filter(band, 1/scale) + skimage block_reduce(np.mean), operation by
 *   operation: per axis (0, then 1) the symmetric float64 correlation tmp = in[l]*w[r]; tmp += (in[l+ii] + in[l-ii])*w[ii+r]
 *   for ii = -r..-1 with the 'reflect' boundary, un-fused; after EACH axis a cast to the input's dtype (uint16 truncates,
 *   float32 rounds); then the float64 block sum / scale^2.  The reference's float64 result bit for bit (out_f64 = 1), or its
 *   float32 cast.  host_weights: the 2*radius + 1 normalised Gaussian weights, computed by the caller as scipy does (they are
 *   passed to the kernel by value).  DSEN2_ERR_INVALID, with nothing launched: H or W not a multiple of scale (the reference
 *   raises ValueError), scale outside 1..32, radius > 8, radius > min(H, W), unknown dtype.  Any C. */
#define DSEN2_DTYPE_U16 0
#define DSEN2_DTYPE_F32 1
int dsen2_down_pixel_aggr(const void *dev_img, int dtype, int H, int W, int C, int scale, const double *host_weights,
                          int radius, void *dev_out, int out_f64, void *stream);

/* ---- corpus: training batches cut from tiles that live on the device (csrc/corpus_batch.hip) ---------------------------------
 * No reference counterpart as a function: the reference writes a fixed set of random crops per tile to disk (save_random_patches /
 * save_random_patches60, utils/patches.py:181-271) and trains from those files.  Here the downsampled images of every tile and the
 * ground truth stay in device memory and EVERY batch is cut from them, in one launch, with the geometry of those two functions.
 *
 * A tile (dsen2_corpus_tile) is the device pointers of its HWC images and the extent (grid_h, grid_w) of its ORIGIN GRID, the
 * lowest-resolution low-res image; with S = 2 (run_60: 6):
 *                  run_60 = 0                                   run_60 = 1
 *   dev_lr10       float32 [2 grid_h, 2 grid_w, 4]               float32 [6 grid_h, 6 grid_w, 4]
 *   dev_lr20       float32 [grid_h, grid_w, 6]                   float32 [3 grid_h, 3 grid_w, 6]
 *   dev_lr60       NULL                                         float32 [grid_h, grid_w, 2]
 *   dev_gt         [2 grid_h, 2 grid_w, 6]                       [6 grid_h, 6 grid_w, 2]      uint16 or float32 (gt_dtype)
 * A sample is four ints (tile, oy, ox, op): the 16 x 16 crop of the origin grid at (oy, ox), turned by the dihedral op.  Outputs,
 * NCHW float32 with P = 32 (run_60: 96), sample k at index k:
 *   dev_x10 [n,4,P,P]   dev_lr10 at (S oy, S ox), P x P, each value / divisor
 *   dev_x20 [n,6,P,P]   dev_lr20 at (oy, ox), 16 x 16 (run_60: at (3 oy, 3 ox), 48 x 48), up-sampled to P x P as
 *                       dsen2_upsample_mirror_bilinear up-samples a patch of that size on its own, post_divisor = divisor
 *   dev_x60 [n,2,P,P]   run_60 only: dev_lr60 at (oy, ox), 16 x 16, up-sampled likewise
 *   dev_y   [n,6|2,P,P] dev_gt at (S oy, S ox), P x P, widened to float32 (exact), each value / divisor
 *   and then D_op of every one of them (the convention of "dihedral" above).  divisor == 1 skips the divide exactly.
 * Bit for bit what dsen2_tile_gather (border 0), dsen2_upsample_mirror_bilinear and dsen2_dihedral_nchw give for the same origins,
 * in ONE launch: a workgroup per (sample, tensor, 32 x 32 output tile) with all the tensor's bands, low-resolution crops
 * interpolated from LDS, the op applied through a padded LDS tile so that the stores are coalesced for all 8 ops.  No atomics.
 *
 * dsen2_corpus_create checks the table (DSEN2_ERR_INVALID: a NULL image, dev_lr60 given or missing against run_60, a grid below
 *   16 x 16, another gt_dtype, no tile) and copies it; it touches no device, and nothing of the images is read.  The device copy of
 *   the table is made by the first dsen2_corpus_batch that launches (one synchronous copy), on the calling thread's current
 *   device, to which the handle belongs from then on.  The images stay the caller's and must outlive the handle.
 * dsen2_corpus_batch: host_samples and dev_samples are the same [n, 4] int32 table in host and in device memory: the host copy is
 *   what is checked, the device copy is what the kernel reads (the caller uploads what it had checked; a device sample that does
 *   not fit its tile is skipped by the kernel, so no byte outside a tile's images is ever read).  DSEN2_ERR_INVALID with nothing
 *   launched: a NULL pointer, dev_x60 given or missing against run_60, either sample table missing, a tile index outside the
 *   table, an origin with oy + 16 > grid_h or ox + 16 > grid_w (grid - 16 itself is the last valid origin) or negative, an op
 *   outside 0..7, a divisor that is 0 or not finite, n negative or above 2^20.  n == 0 returns DSEN2_OK.  Nothing synchronises
 *   after the first call. */
typedef struct dsen2_corpus dsen2_corpus;
typedef struct dsen2_corpus_tile {
  const float *dev_lr10, *dev_lr20, *dev_lr60;
  const void *dev_gt;
  int grid_h, grid_w;
  int gt_dtype; /* DSEN2_DTYPE_U16 or DSEN2_DTYPE_F32 */
} dsen2_corpus_tile;
int dsen2_corpus_create(const dsen2_corpus_tile *host_tiles, int n_tiles, int run_60, dsen2_corpus **out);
void dsen2_corpus_destroy(dsen2_corpus *corpus);
int dsen2_corpus_batch(const dsen2_corpus *corpus, const int *host_samples, const int *dev_samples, int n, float divisor,
                       float *dev_x10, float *dev_x20, float *dev_x60_or_null, float *dev_y, void *stream);

/* ---- corpus origin mask: which crop origins of a tile may be drawn (csrc/corpus_mask.hip) -------------------------------------------
 * Definitions, for ONE tile whose origin grid is grid_h x grid_w (as dsen2_corpus_tile has it):
 *   CELL FOOTPRINT  with S = 2 (run_60: 6), one cell of the origin grid covers F x F samples of the raw 10 m raster d10 [H, W, C],
 *                   F = S * S (4, or 36 for run_60): H = grid_h * F, W = grid_w * F.
 *   BLANK CELL      any BAND-0 sample v of d10 in the cell's footprint fails v >= 1 — the reference's `chan3 < 1` test on the same
 *                   band (training/create_patches.py:208-211); a NaN of a float32 raster counts as blank.  No other band is read.
 *   COVERED CELL    the cell lies inside [vy - margin, vy + 16 + margin) x [vx - margin, vx + 16 + margin) for some hold-out origin
 *                   (vy, vx); margin >= 0 is in cells.  With margin 0, "the window of origin (oy, ox) contains a covered cell" is
 *                   exactly "the crop at (oy, ox) overlaps the crop at a hold-out origin".
 *   VALID ORIGIN    (oy, ox), 0 <= oy <= grid_h - 16, 0 <= ox <= grid_w - 16, is valid when no cell of [oy, oy + 16) x [ox, ox + 16)
 *                   is blank or covered.
 * dsen2_corpus_origin_mask writes
 *   dev_bitmap  one bit per origin: grid_h - 15 rows of ceil((grid_w - 15) / 8) bytes, bit k of byte b = origin column 8 b + k
 *               (least significant bit first), set when the origin is valid, the padding bits of a row's last byte 0: exactly
 *               np.packbits(valid, axis=1, bitorder='little');
 *   dev_count   the number of valid origins (one int32);
 *   dev_cells   scratch of grid_h * grid_w bytes, which holds the cell map afterwards (1 = blank or covered, else 0): with m == 0
 *               it is the BLANK MAP, which a later call may be given in place of the raster.
 * dev_src: the raster d10 in device memory, uint16 (DSEN2_DTYPE_U16) or float32 (DSEN2_DTYPE_F32), any C >= 1 — or, with dtype ==
 *   DSEN2_MASK_BLANK_MAP, a blank map [grid_h, grid_w] of bytes (non-zero = blank; all zero: nothing is blank), H, W and C as they
 *   were for the raster; dev_src and dev_cells must then not be the same buffer.
 * host_holdout / dev_holdout: the same [m, 2] int32 table of hold-out origins (vy, vx) in host and in device memory, as
 *   dsen2_corpus_batch takes its samples: the host copy is checked, the device copy is read (a rectangle is clipped to the grid on
 *   the device, so no table can make the kernel write outside dev_cells).  Both may be NULL when m == 0.
 * Two launches on `stream`, three with m > 0 (the count is formed inside the last), integer work only (flags, ORs, wave ballots, an integer count; no float arithmetic, no float
 *   atomics): the result depends on the inputs alone.  Nothing synchronises.
 * DSEN2_ERR_INVALID with nothing launched: a NULL pointer, an unknown dtype, C < 1, grid_h or grid_w below 16 (or above 2^15 = 32768: the number of origins, (grid_h - 15) * (grid_w - 15), then fits the int32 count), H or
 *   W not grid * F, F other than 4 or 36, m or margin negative (or above 2^24 / 2^20), a table missing with m > 0, a hold-out origin
 *   outside [0, grid - 16]. */
#define DSEN2_MASK_BLANK_MAP 3
int dsen2_corpus_origin_mask(const void *dev_src, int dtype, int H, int W, int C, int grid_h, int grid_w, const int *host_holdout,
                             const int *dev_holdout, int m, int margin, unsigned char *dev_cells, unsigned char *dev_bitmap,
                             int *dev_count, void *stream);

/* ---- class masks: a validity bitmap from a class raster the caller brings (csrc/valid_mask.hip) ---------------------------------------
 * Not in the reference.  The bitmap is dsen2_tile_nodata's: uint32 [H][ceil(W/32)], pixel (y, x) is bit x & 31 of word
 * y*ceil(W/32) + (x >> 5), a set bit means valid, the bits at x >= W are 0.  Definitions, for a class raster dev_cls (uint8 [Hs, Ws]:
 * Sentinel-2's SCL layer, a cloud-probability layer, any class image at 10, 20 or 60 m) and a target grid of H x W pixels:
 *   TABLE      host_lut256: 256 bytes in HOST memory, read during the call and passed by value into the launch (as 256 bits); a
 *              non-zero entry means the class is invalid.  A probability layer with a threshold is just another table.
 *   RAW        with up > 1 (source coarser than the target, replicated) target pixel (y, x) is RAW-invalid when source pixel
 *              (y / up, x / up) has an invalid class: needs (H-1)/up < Hs and (W-1)/up < Ws.  With down > 1 (source finer) it is
 *              RAW-invalid when ANY source pixel of its down x down block, rows [y*down, (y+1)*down) and columns alike, has one:
 *              needs H*down <= Hs and W*down <= Ws.  up == down == 1: pixel for pixel.  Surplus source rows and columns are never
 *              read.
 *   DILATED    a pixel is invalid when any RAW-invalid pixel lies within |dy| <= dilate, |dx| <= dilate INSIDE the image; what
 *              lies outside the image is valid.  dilate is in target pixels, 0..32 (one bitmap word: a tile's halo is one word
 *              either side).
 *   OUTPUT     bit = not DILATED, ANDed with the same bit of dev_and_bits_or_null when one is given (it may be the output buffer
 *              itself: a word is read and written by the same lane); padding bits 0.
 * dsen2_class_valid_bits: one launch on `stream`; dilate == 0 takes a kernel of its own without halo or LDS tile.  Integer work
 *   only, no atomics: the result depends on the inputs alone.  Nothing synchronises.
 * dsen2_tile_flags_from_bits: the second launch of dsen2_tile_nodata — dev_patch_empty (uint8 [y_tiles*x_tiles], 1 = the patch's
 *   owned rectangle holds no set bit) from ANY bitmap in this format, by the same kernel.  Geometry and refusals of
 *   dsen2_tile_nodata.
 * dsen2_raster_apply_valid: in place on the HWC raster dev_img [H,W,C] of uint16 (DSEN2_DTYPE_U16) or float32 (DSEN2_DTYPE_F32)
 *   samples: every one of the C samples of a pixel whose bit is 0 becomes 0 (+0.0f); no other byte of the raster is written.  Any
 *   C in 1..4096.
 * dsen2_cells_from_valid_bits: dev_cells uint8 [H/S, W/S]; a cell becomes 1 when any pixel of its S x S footprint has bit 0, else
 *   0; with accumulate != 0 a cell that already holds non-zero is left as it is (the OR into a blank map, which
 *   dsen2_corpus_origin_mask then takes as DSEN2_MASK_BLANK_MAP).  H and W multiples of S, S in 1..8.
 * DSEN2_ERR_INVALID with nothing launched: a NULL pointer (dev_and_bits_or_null excepted), H or W below 1 or above 2^15 = 32768,
 *   up or down outside 1..8 or both above 1, a coverage rule broken, dilate outside 0..32, another dtype, C outside 1..4096, S
 *   outside 1..8 or not dividing H and W, the geometry dsen2_tile_nodata refuses. */
int dsen2_class_valid_bits(const unsigned char *dev_cls, int Hs, int Ws, const unsigned char *host_lut256, int up, int down, int H,
                           int W, int dilate, const unsigned int *dev_and_bits_or_null, unsigned int *dev_valid_bits, void *stream);
int dsen2_tile_flags_from_bits(const unsigned int *dev_valid_bits, int H, int W, int P, int border, unsigned char *dev_patch_empty,
                               void *stream);
int dsen2_raster_apply_valid(void *dev_img, int dtype, int H, int W, int C, const unsigned int *dev_valid_bits, void *stream);
int dsen2_cells_from_valid_bits(const unsigned int *dev_valid_bits, int H, int W, int S, int accumulate, unsigned char *dev_cells,
                                void *stream);

/* dsen2_abs_sq_error_sums (csrc/error_sums.hip): dev_out[0 .. 1] = { sum |p - t|, sum (p - t)^2 } over `count` float32 pairs, as
 *   float64: what a validation pass needs of a prediction that is already on the device.  Every difference, product and sum is
 *   float64 and rounded on its own (no FMA).  The order of every addition is fixed by `count` alone: blocks = clamp(ceil(count /
 *   2048), 1, 4096) workgroups of 256 threads; thread t of workgroup b adds elements b * 256 + t, + blocks * 256, ... in index
 *   order (|d| and d * d onto 0.0); the workgroup adds its threads in a halving tree (128, 64, ... 1); one workgroup adds the
 *   partial pairs likewise (thread t: partials t, t + 256, ...; then the tree).  The grid never depends on the device: the same
 *   bits on every run and every GPU.  dev_work: dsen2_abs_sq_error_sums_workspace_bytes() bytes of device scratch.
 *   DSEN2_ERR_INVALID: a NULL pointer, count <= 0 or >= 2^31; DSEN2_ERR_WORKSPACE: a workspace that is too small. */
int dsen2_abs_sq_error_sums_workspace_bytes(size_t *bytes);
int dsen2_abs_sq_error_sums(const float *dev_pred, const float *dev_target, long long count, void *dev_work, size_t work_bytes,
                            double *dev_out, void *stream);

/* ---- evaluation: MATLAB-compatible bicubic resize and per-band errors (utils/imresize.py, testing/demoDSen2.py:31-35) ----
 * dsen2_imresize_axis  <->  imresizemex(inimg, weights, indices, dim)          utils/imresize.py:50-74
 *   One resampling pass along `axis` (0 = rows, 1 = columns) of the HWC image dev_in [H,W,C] of uint16, float32 or float64
 *   samples; writes float64 [out_len,W,C] (axis 0) or [H,out_len,C] (axis 1).  Per output, sequentially in k and un-fused:
 *   out = sum_k w[k][o] * (double)in[idx[k][o]].  dev_weights (float64) and dev_indices (int32) are DEVICE tables of `taps` rows
 *   of out_len entries each (k-major: the transpose of what contributions() returns); the caller builds them
 *   (dsen2_amd/imresize.py).  imresize = two such passes, the smaller scale first, the second reading the first's float64.
 *   Refused with DSEN2_ERR_INVALID and nothing launched: any other dtype (uint8: the reference rounds it; not supported), taps
 *   outside 1..256, an axis other than 0 / 1, a slice of 2^31 elements or more.  Indices are clamped to the axis on the device. */
#define DSEN2_DTYPE_F64 2
int dsen2_imresize_axis(const void *dev_in, int dtype, int H, int W, int C, int axis, int out_len, const double *dev_weights,
                        const int *dev_indices, int taps, double *dev_out, void *stream);

/* dsen2_band_errors: per band c of the HWC images dev_x and dev_gt [H,W,C] (float32 or float64 each), dev_out[3c .. 3c+2] =
 *   { sum (x - gt)^2, sum gt, H * W } as float64: RMSE_c = sqrt(out[3c] / out[3c+2]), SRE_c = 10 log10((out[3c+1] / out[3c+2])^2 /
 *   (out[3c] / out[3c+2])).  The order of every addition depends on the shape only (no float atomics): the same bits on every
 *   run.  dev_work: dsen2_band_errors_workspace_bytes(C) bytes of device scratch.  1 <= C <= 64.
 * dsen2_imresize_band_errors: dsen2_imresize_axis followed by dsen2_band_errors against dev_gt (which has the OUTPUT's shape) in
 *   one pass that never stores the resampled image — the second pass of the bicubic baseline of a whole tile. */
int dsen2_band_errors_workspace_bytes(int C, size_t *bytes);
int dsen2_band_errors(const void *dev_x, int x_dtype, const void *dev_gt, int gt_dtype, int H, int W, int C, void *dev_work,
                      size_t work_bytes, double *dev_out, void *stream);
int dsen2_imresize_band_errors(const void *dev_in, int dtype, int H, int W, int C, int axis, int out_len, const double *dev_weights,
                               const int *dev_indices, int taps, const void *dev_gt, int gt_dtype, void *dev_work,
                               size_t work_bytes, double *dev_out, void *stream);

/* ---- evaluation: the paper's two further metrics, UIQ (Wang & Bovik 2002, img_qi.m) and SAM (csrc/quality_metrics.hip) ----
 * All arithmetic is float64, every product and every sum rounded on its own, in the order DESIGN §7 writes down; the images are
 * HWC [H,W,C], float32 or float64 each, 1 <= C <= 64, fewer than 2^31 elements.
 * dsen2_uiq_map: per band the quality index of every block x block window (2 <= block <= 16, valid windows only, NOT sliding
 *   sums: each window sum is `block` sequential additions along the row, then `block` along the column):
 *   dev_map_f64 [H-block+1, W-block+1, C].  The map is a pure function of its inputs: the same bits on every run.
 * dsen2_uiq_sums: dev_out[2c .. 2c+1] = { sum of that map over band c, number of windows } without ever storing the map; the
 *   UIQ of band c is their quotient, the UIQ of the image the mean over the bands.
 * dsen2_sam_sums: dev_out[0 .. 1] = { sum over the pixels of acos(clamp(<x,y> / (|x| |y|), -1, 1)) in degrees, pixels counted }; a
 *   pixel whose spectrum is zero in either image is left out.  SAM is the quotient.
 * dsen2_imresize_uiq_sums / dsen2_imresize_sam_sums: the same sums for x = the resampling pass dsen2_imresize_axis(dev_in, ...)
 *   would write, against dev_gt (which has the OUTPUT's shape), computed tile by tile and never stored: the second pass of the
 *   bicubic baseline.  The same bits as dsen2_imresize_axis followed by dsen2_uiq_sums / dsen2_sam_sums.
 * The order of every addition depends on the shapes only (no float atomics).  dev_work: dsen2_quality_workspace_bytes(C) bytes
 * of device scratch.  DSEN2_ERR_INVALID with nothing launched: H or W (of the image the metric sees) below block, block outside
 * 2..16, C outside 1..64, any other dtype, a null pointer, 2^31 elements or more; DSEN2_ERR_WORKSPACE: a short workspace. */
int dsen2_quality_workspace_bytes(int C, size_t *bytes);
int dsen2_uiq_map(const void *dev_x, int x_dtype, const void *dev_y, int y_dtype, int H, int W, int C, int block,
                  double *dev_map_f64, void *stream);
int dsen2_uiq_sums(const void *dev_x, int x_dtype, const void *dev_y, int y_dtype, int H, int W, int C, int block, void *dev_work,
                   size_t work_bytes, double *dev_out, void *stream);
int dsen2_sam_sums(const void *dev_x, int x_dtype, const void *dev_y, int y_dtype, int H, int W, int C, void *dev_work,
                   size_t work_bytes, double *dev_out, void *stream);
int dsen2_imresize_uiq_sums(const void *dev_in, int dtype, int H, int W, int C, int axis, int out_len, const double *dev_weights,
                            const int *dev_indices, int taps, const void *dev_gt, int gt_dtype, int block, void *dev_work,
                            size_t work_bytes, double *dev_out, void *stream);
int dsen2_imresize_sam_sums(const void *dev_in, int dtype, int H, int W, int C, int axis, int out_len, const double *dev_weights,
                            const int *dev_indices, int taps, const void *dev_gt, int gt_dtype, void *dev_work, size_t work_bytes,
                            double *dev_out, void *stream);

/* ---- evaluation: the structural similarity index, SSIM (Wang, Bovik, Sheikh & Simoncelli 2004, ssim_index.m without its
 * automatic down-sampling; csrc/ssim.hip) ----
 * Per band, over valid windows only, with a separable window of `win` normalised weights host_window[0 .. win-1] (HOST memory,
 * read during the call; win odd, 3..15; the Gaussian of the paper is win 11, sigma 1.5) and the biased covariance.  All arithmetic
 * is float64, every product and every sum rounded on its own, in this order.  The same filter for each of the five
 * fields f = x, y, x*x, y*y, x*y, the products formed first:  row pass r[y][c] = w[0]*f[y][c], then r = r + w[k]*f[y][c+k] for
 * k = 1 .. win-1 in order; column pass the same sequential sum over r[y+k][c].  With mx, my, exx, eyy, exy the filtered fields:
 *   m11 = mx*mx  m22 = my*my  m12 = mx*my  s1 = exx - m11  s2 = eyy - m22  s12 = exy - m12
 *   num = (2*m12 + c1)*(2*s12 + c2)   den = ((m11 + m22) + c1)*((s1 + s2) + c2)   q = num/den (an IEEE division)
 * c1 = (K1 L)^2 and c2 = (K2 L)^2 are the caller's, L being the data range.  The images are HWC [H,W,C], float32 or float64 each
 * (dev_in of the fused form: uint16 as well), 1 <= C <= 64, fewer than 2^31 elements.
 * dsen2_ssim_map: dev_map_f64 [H-win+1, W-win+1, C].  A pure function of its inputs: the same bits on every run.
 * dsen2_ssim_sums: dev_out[2c .. 2c+1] = { sum of that map over band c, number of windows } without ever storing the map; the
 *   SSIM of band c is their quotient, the SSIM of the image the mean over the bands.
 * dsen2_imresize_ssim_sums: the same sums for x = the resampling pass dsen2_imresize_axis(dev_in, ...) would write, against
 *   dev_gt (which has the OUTPUT's shape), computed tile by tile and never stored.  The same bits as dsen2_imresize_axis followed
 *   by dsen2_ssim_sums.
 * The order of every addition depends on the shapes only (no float atomics).  dev_work: dsen2_quality_workspace_bytes(C) bytes
 * of device scratch.  DSEN2_ERR_INVALID with nothing launched: win even or outside 3..15, H or W (of the image the metric sees)
 * below win, C outside 1..64, any other dtype, a null pointer, 2^31 elements or more, c1 or c2 not finite or not > 0 (which keeps
 * den > 0), a window entry that is not finite; DSEN2_ERR_WORKSPACE: a short workspace. */
int dsen2_ssim_map(const void *dev_x, int x_dtype, const void *dev_y, int y_dtype, int H, int W, int C, const double *host_window,
                   int win, double c1, double c2, double *dev_map_f64, void *stream);
int dsen2_ssim_sums(const void *dev_x, int x_dtype, const void *dev_y, int y_dtype, int H, int W, int C, const double *host_window,
                    int win, double c1, double c2, void *dev_work, size_t work_bytes, double *dev_out, void *stream);
int dsen2_imresize_ssim_sums(const void *dev_in, int dtype, int H, int W, int C, int axis, int out_len, const double *dev_weights,
                             const int *dev_indices, int taps, const void *dev_gt, int gt_dtype, const double *host_window, int win,
                             double c1, double c2, void *dev_work, size_t work_bytes, double *dev_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* DSEN2_HIP_H */
