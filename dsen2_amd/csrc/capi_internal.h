// The one host-side vocabulary of the two C-ABI translation units (capi.hip: network object, the forward, single-layer and
// patch entries; capi_train.hip: the training entries): the error setter and HIP_TRY, guarded(), the model object (its layers are conv_plan.h's), the shape
// and device checks, make_params, the RAII holders of events and of a temporary device buffer, and the declarations of the
// forward's launch sequence (capi.hip), which inference and training both run.
#pragma once
#include <exception>
#include <new>
#include <vector>

#include "../../include/dsen2_hip.h"
#include "conv_plan.h"

namespace dsen2 {

// sets the thread-local text of dsen2_last_error() and returns `code` (capi.hip)
int fail(int code, const char* fmt, ...);

#define HIP_TRY(expr)                                                                                              \
  do {                                                                                                             \
    hipError_t e_ = (expr);                                                                                        \
    if (e_ != hipSuccess) return dsen2::fail(DSEN2_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_));   \
  } while (0)

// Nothing may leave an extern "C" entry point as a C++ exception (std::bad_alloc from a staging vector, std::system_error
// from a mutex): through a C / ctypes caller that is std::terminate -> abort() of the host process.  Every entry point
// that can allocate or lock runs its body through this and reports DSEN2_ERR_* with dsen2_last_error() instead.
template <class F>
int guarded(F&& body) noexcept {
  try {
    return body();
  } catch (const std::bad_alloc&) {
    return fail(DSEN2_ERR_NOMEM, "out of host memory");            // not the caller's arguments: its own code
  } catch (const std::exception& e) {
    return fail(DSEN2_ERR_INTERNAL, "unexpected C++ exception: %s", e.what());
  } catch (...) {
    return fail(DSEN2_ERR_INTERNAL, "unexpected C++ exception");
  }
}

// Training state of an fp32 or bf16x3 model (capi_train.hip), created by the first training call: the master weights as a
// device keras-flat fp32 vector and the gather maps that rebuild every packed buffer from it.
struct TrainState;
void train_state_destroy(TrainState* t);
// after dsen2_model_load_weights replaced the packed weights: bring the master vector and the dgrad weights up to date
int train_state_after_load(dsen2_model* m);

}  // namespace dsen2

struct dsen2_model : dsen2::NetworkPlan {   // every layer's plan and place inside dev_params (conv_plan.h)
  int c10, c20, c60, cin, cout, num_layers, feat, precision;
  int device;
  dsen2::Tuning tune;   // kernel structures, fixed at creation
  float* dev_params;
  bool loaded;
  dsen2::TrainState* train;   // NULL until the first training call
  int train_precision = 0;    // dsen2_model_set_train_precision: 0 = the model's own arithmetic, 1 = bf16 operands (fp32 models)
  // dsen2_model_set_loss: what dsen2_model_gradients minimises (dsen2_internal.h, "losses"); the default is the MAE, unmasked
  int loss_kind = 0, loss_mask = 0;
  float loss_param = 0.f;
  dsen2::SsimLossTerm loss_ssim;      // dsen2_model_set_loss_ssim: weight 0 (the default) = no SSIM term, nothing of it is launched
  // precision 2 with residual blocks: the packed planes (hi + lo, 16 significant bits) do not hold the fp32 weights, so the
  // keras-flat vector dsen2_model_load_weights was given is kept until a training state takes it over as its master copy
  std::vector<float> host_flat;
  // How the model trains (capi_train.hip, StepFormat): the bf16 planes of a 16-bit tensor of its step.  0: fp32 tensors (an
  // fp32 model; any model without residual blocks, whose plan is all fp32), 2: bf16x3, 1: an fp32 model whose step runs on
  // a precision-1 companion plan (and that companion itself)
  int train_planes() const { return num_layers == 0 ? 0 : precision == 0 ? train_precision : precision; }
};

namespace dsen2 {

// the (kind, param, mask mode) triple of dsen2_model_set_loss, dsen2_loss_grad and dsen2_loss_sums
inline bool loss_reads_param(int kind) { return kind == kLossHuber || kind == kLossCharbonnier; }
inline int check_loss(const char* who, int kind, float param, int mask_mode) {
  if (kind < 0 || kind >= kLossKinds) return fail(DSEN2_ERR_INVALID, "%s: loss kind %d unknown (0 MAE, 1 MSE, 2 Huber, 3 Charbonnier)", who, kind);
  if (mask_mode < 0 || mask_mode >= kMaskModes) return fail(DSEN2_ERR_INVALID, "%s: mask mode %d unknown (0 none, 1 no-data)", who, mask_mode);
  if (loss_reads_param(kind) && !(param > 0.f && param <= 3.402823466e38f))
    return fail(DSEN2_ERR_INVALID, "%s: loss kind %d needs a finite parameter > 0, got %g", who, kind, (double)param);
  return DSEN2_OK;
}

// the SSIM term of dsen2_model_set_loss_ssim, dsen2_ssim_loss_grad and dsen2_ssim_loss_sums; fills *term, or changes nothing
inline int check_ssim_loss_term(const char* who, float weight, const double* host_window, int win, double c1, double c2, SsimLossTerm* term) {
  if (!(weight >= 0.f && weight <= 3.402823466e38f)) return fail(DSEN2_ERR_INVALID, "%s: the SSIM weight must be finite and >= 0, got %g", who, (double)weight);
  if (win < kSsimLossMinWin || win > kSsimLossMaxWin || win % 2 == 0)
    return fail(DSEN2_ERR_INVALID, "%s: window size %d is not odd or outside %d..%d", who, win, kSsimLossMinWin, kSsimLossMaxWin);
  if (!host_window) return fail(DSEN2_ERR_INVALID, "%s: NULL window", who);
  for (int i = 0; i < win; ++i)
    if (!(host_window[i] - host_window[i] == 0.0)) return fail(DSEN2_ERR_INVALID, "%s: window entry %d is not finite", who, i);
  if (!(c1 > 0.0 && c1 - c1 == 0.0) || !(c2 > 0.0 && c2 - c2 == 0.0))
    return fail(DSEN2_ERR_INVALID, "%s: constants c1 = %g and c2 = %g must be finite and positive", who, c1, c2);
  SsimLossTerm t;
  t.weight = weight;
  t.win = win;
  for (int i = 0; i < win; ++i) t.w[i] = host_window[i];
  t.c1 = c1;
  t.c2 = c2;
  *term = t;
  return DSEN2_OK;
}

inline int check_shape(const dsen2_model* m, int n, int h, int w) {
  if (n <= 0 || h <= 0 || w <= 0) return fail(DSEN2_ERR_INVALID, "bad shape n=%d h=%d w=%d", n, h, w);
  if ((size_t)h * w * (size_t)(m ? m->feat : 256) >= ((size_t)1 << 29))
    return fail(DSEN2_ERR_INVALID, "one image of %dx%d exceeds 2^31 activation bytes", h, w);
  return DSEN2_OK;
}

// A handle belongs to the device that was current when it was created (its packed weights live there): a call made with
// another current device would hand device A's pointers to kernels launched on device B.
inline int check_device(const dsen2_model* m) {
  int dev = -1;
  if (hipGetDevice(&dev) != hipSuccess) return fail(DSEN2_ERR_NO_DEVICE, "no HIP device");
  if (dev != m->device)
    return fail(DSEN2_ERR_INVALID, "model handle belongs to device %d but the calling thread's current device is %d "
                     "(one handle per device: hipSetDevice(%d) before the call)", m->device, dev, m->device);
  return DSEN2_OK;
}

inline ConvParams make_params(const float* in, const float* wpk, const float* bias, const float* aux, float* out, int n, int h,
                              int w, int cout_real, float scale) {
  ConvParams p;
  p.in = in; p.wpk = wpk; p.bias = bias; p.aux = aux; p.out = out; p.out2 = nullptr;
  p.n = n; p.h = h; p.w = w;
  p.tiles_x = (w + kTile - 1) / kTile; p.tiles_y = (h + kTile - 1) / kTile;
  p.cout_real = cout_real; p.res_scale = scale; p.diag = nullptr;
  return p;
}

// events that are destroyed on every path
struct Events {
  std::vector<hipEvent_t> ev;
  int create(size_t count) {
    ev.assign(count, nullptr);
    for (hipEvent_t& e : ev) HIP_TRY(hipEventCreate(&e));
    return DSEN2_OK;
  }
  ~Events() {
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
  }
};

// a temporary device buffer that is freed on every path
struct DeviceBuffer {
  char* p = nullptr;
  ~DeviceBuffer() {
    if (p) (void)hipFree(p);
  }
};

// The single-layer entries (tests and tools; they own the stream until they return): one temporary device buffer, copied from
// the host (host == NULL: scratch the kernel fills itself), one launch(buffer), synchronise.
template <class Launch>
int launch_once_with_temp(const char* what, const void* host, size_t bytes, hipStream_t stream, Launch&& launch) {
  DeviceBuffer dev;
  HIP_TRY(hipMalloc((void**)&dev.p, bytes));
  if (host) HIP_TRY(hipMemcpy(dev.p, host, bytes, hipMemcpyHostToDevice));
  hipError_t e = launch(dev.p);
  if (e == hipSuccess) e = hipStreamSynchronize(stream);
  if (e != hipSuccess) return fail(DSEN2_ERR_HIP, "%s launch: %s", what, hipGetErrorString(e));
  return DSEN2_OK;
}

// ---- the forward's launch sequence (capi.hip) ----
// The activations of one forward pass.  Inference carves them from the caller's workspace (forward_ws), the residual blocks
// running in place on `a` and `t`; training (capi_train.hip) points x0 / a / t into its own workspace and keeps every block's
// activations (forward_launches, keep_step).
struct ForwardWs {
  float* x0 = nullptr;                                // NHWC16 packed input
  float* a = nullptr;                                 // residual stream x, fp32 (16-bit precisions: the first convolution's
                                                      // output where it is the generic kernel's, and the last block's)
  float* t = nullptr;                                 // precision 0: relu(convA(x))
  // precision 1 / 2: the stream as s0, the operand tensor of the next convolution (precision 1: the hi plane; precision 2:
  // hx, the hi | xl planes), and s1, the low halves; t16 = relu(convA(x)) as an operand tensor (bf16; hi | lo planes)
  void *s0 = nullptr, *s1 = nullptr, *t16 = nullptr;
  void* xkeep = nullptr;                              // precision 1 / 2, keep_step > 0: copies of s0, x_l at xkeep + l * keep_step floats (l < d)
  float* x0f = nullptr;                               // precision 1 / 2, keep_step > 0: x_0 as fp32 NHWC
  size_t bytes = 0;
};
// the inference workspace for n images of h x w: its size and, with base != NULL, its sub-buffers
ForwardWs forward_ws(const dsen2_model* m, int n, int h, int w, char* base);
// Every launch of one forward pass, in stream order; no argument checks.  keep_step = 0: the blocks run in place.  keep_step
// > 0 (training; floats): every block's activations are kept.  Precision 0: block l reads x_{l-1} at B.a + (l - 1) * keep_step
// and writes t_l at B.t + (l - 1) * keep_step and x_l at B.a + l * keep_step.  Precision 1 / 2 with residual blocks (a bf16x3
// model; the companion plan of a mixed-precision step): always layer by layer, never the chain kernel; conv-A writes t_l at
// B.t16 + (l - 1) * keep_step; conv-B runs in place on (B.s0, B.s1), so s0 — what the backward reads — is copied to B.xkeep +
// l * keep_step after the first convolution (l = 0) and after every block but the last, whose output is the fp32 tensor B.a;
// B.x0f receives x_0 joined to fp32.
// x0_packed: the caller has already run launch_pack_inputs into B.x0.
// ev (optional, 4 events): recorded on the stream before the first convolution, before the first and after the last
// residual-block convolution, and after the output convolution.
int forward_launches(const dsen2_model* m, const float* x10, const float* x20, const float* x60, float* out, int n, int h, int w,
                     const ForwardWs& B, size_t keep_step, bool x0_packed, hipStream_t stream, const hipEvent_t* ev);

}  // namespace dsen2
