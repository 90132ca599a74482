// capi.hip — the extern "C" boundary of libdsen2_hip.so (declared in include/dsen2_hip.h).
// Host-side orchestration only: argument checks, weight packing/upload, workspace carving and the
// launch sequence of one forward pass.  No torch types, no allocation inside the forward path.
// Every entry point that can allocate, lock or launch runs its body through guarded() (capi_internal.h): no C++ exception
// crosses the ABI.

#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <exception>
#include <new>
#include <vector>

#include "capi_internal.h"

using namespace dsen2;

namespace {

thread_local char g_err[512] = "";

#ifdef DSEN2_DIAG
// Diagnostic build only (tools/): defaults copied into models and single-layer calls made AFTER dsen2_diag_set.
// The product library has no mutable globals — a model's kernel structures are fixed constants.
Tuning g_diag_tuning;
unsigned long long* g_diag_stamps = nullptr;   // device buffer for ablation bit 32 (dsen2_diag_set_stamps)
#endif
Tuning default_tuning() {
#ifdef DSEN2_DIAG
  return g_diag_tuning;
#else
  return Tuning{};
#endif
}

constexpr int kWarmLaunches = 24;      // dsen2_model_time_body_conv: untimed launches before the timed ones

}  // namespace

namespace dsen2 {
int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}
}  // namespace dsen2

// One persistent launch over all 2d body convolutions of a precision-1 / -2 model may be tried (the launcher still answers
// hipErrorNotSupported for a batch that keeps more CUs busy layer by layer); the precision-2 chain has no ablation build.
static bool may_chain(const dsen2_model* m) {
  return m->chain_stride != 0 && m->tune.chain && m->tune.grid_cap == 0 && (m->precision == 1 || m->tune.ablate == 0);
}

// DSen2Net.py:24-29: Concatenate + Conv2D + ReLU.  Leaves the residual stream where the body reads it: fp32 B.a (precision 0,
// or no residual blocks) or the 16-bit tensors (B.s0, B.s1) (precision 1 / 2).
static int first_layer(const dsen2_model* m, const float* x10, const float* x20, const float* x60, int n, int h, int w,
                       const ForwardWs& B, bool x0_packed, hipStream_t stream) {
  const Layer& L = m->layers[0];
  const ConvPlan& pl = L.plan;
  const float* P = m->dev_params;
  const bool x3 = m->precision == 2 && m->num_layers > 0;
  ConvParams pf = make_params(B.x0, L.weights(P), L.bias(P), nullptr, B.a, n, h, w, 0, 0.f);
  if (pl.epilogue == kEpiReluSplit) {
    // a precision-1 model's first convolution writes the residual stream directly as its two blocked 16-bit planes
    pf.out = reinterpret_cast<float*>(B.s0);
    pf.out2 = B.s1;
  }
  // the direct kernels read the NCHW inputs themselves; other channel counts, and the reference structure, pack them to
  // NHWC16 first
  const FirstInputs fi{x60, m->c10, m->c20, m->c60};
  ConvParams pd = pf;
  pd.in = x10;
  pd.aux = x20;
  bool done = false;
  if (pl.first16_planes) {
    // precision 1 / 2: on the bf16 matrix cores, writing the residual stream's planes itself (conv3x3_first16.hip) —
    // precision 1: (hi, lo); precision 2: hx (hi | xl planes) and lo16
    pd.wpk = L.first16(P);
    pd.out = reinterpret_cast<float*>(B.s0);
    pd.out2 = B.s1;
    HIP_TRY(try_launch(launch_conv3x3_first16(pd, fi, m->feat, x3, stream), &done));
  } else if (pl.first_direct) {
    HIP_TRY(try_launch(launch_conv3x3_first(pd, fi, m->feat, pl.epilogue, stream, m->tune.first_ablate), &done));
  }
  if (!done) {
    if (!x0_packed) HIP_TRY(launch_pack_inputs(x10, x20, x60, m->c10, m->c20, m->c60, B.x0, n, h, w, stream));
    HIP_TRY(launch(pl, pf, pl.epilogue, m->tune, stream));
    if (x3) HIP_TRY(launch_split3_f32(B.a, B.s0, B.s1, n, h, w, m->feat, stream));   // (generic first layer: fp32 `a`)
  }
  return DSEN2_OK;
}

// bytes of a 16-bit operand tensor of the model's body convolutions: two bf16 planes (precision 2) or one (precision 1)
static size_t operand16_bytes(const dsen2_model* m, int n, int h, int w) {
  return (size_t)n * h * w * m->feat * (m->precision == 2 ? 4 : 2);
}

// The residual blocks of a precision-1 / -2 model on the stream's tensors (s0, s1) and t16.
// Precision 1: bf16 operands, fp32 accumulate, exact fp32 residual stream held as two 16-bit planes (s0 = hi, the bf16 operand
// of the next convolution, s1 = lo, the low halves): conv-A reads hi, conv-B updates (hi, lo) in place.
// Precision 2, bf16x3 (conv3x3_body16w.hip, X3): fp32-grade products from three bf16 MFMAs; s0 = hx (hi | xl planes), s1 = lo16;
// conv-A reads hx, writes t16 (hi | lo planes); conv-B reads t16, updates (hx, lo16) in place.
// Either way the last block's conv-B writes plain fp32 out_f32 for the (fp32) output convolution.
// keep_step > 0 (training): layer by layer, t_l at t16 + (l - 1) * keep_step floats, s0 — the next conv-A's operand tensor: hx's
// two planes (precision 2) or the one hi plane (precision 1) — copied to xkeep + l * keep_step after every block but the last.
static int body16(const dsen2_model* m, void* s0, void* s1, void* t16, float* out_f32, int n, int h, int w, hipStream_t stream,
                  size_t keep_step = 0, void* xkeep = nullptr) {
  const float* P = m->dev_params;
  // One persistent launch over all 2d body convolutions when every CU gets whole patches (batch >= one patch per CU,
  // e.g. BASELINE configs[4]); hipErrorNotSupported = this batch keeps more CUs busy layer by layer.
  if (keep_step == 0 && may_chain(m)) {
    const Layer& L1 = m->layers[1];
    const bool x3 = L1.plan.kernel == ConvKernel::Body16x3;
    ConvParams pc = make_params(nullptr, L1.weights(P), L1.bias(P), nullptr, nullptr, n, h, w, 0, 0.1f);
#ifdef DSEN2_DIAG
    if (!x3) pc.diag = g_diag_stamps;
#endif
    ChainArgs ca;
    ca.hi = s0; ca.lo = s1; ca.t = t16; ca.out_f32 = out_f32;
    ca.layer_stride = (unsigned)m->chain_stride; ca.n_layers = 2 * m->num_layers; ca.patches_per_wg = 0; ca.seamless = 0;
    bool done = false;
    HIP_TRY(try_launch(launch_conv3x3_body16w_chain(pc, ca, m->feat, stream, m->tune.ablate, x3), &done));   // (x3: ablate is 0)
    if (done) return DSEN2_OK;
  }
  for (int l = 1; l <= m->num_layers; ++l) {
    const Layer& LA = m->layers[2 * l - 1];
    const Layer& LB = m->layers[2 * l];
    float* const t = reinterpret_cast<float*>(t16) + (size_t)(l - 1) * keep_step;
    HIP_TRY(launch(LA.plan, make_params(reinterpret_cast<const float*>(s0), LA.weights(P), LA.bias(P), nullptr, t, n, h, w, 0, 0.f),
                   kEpiRelu, m->tune, stream));
    const bool last = l == m->num_layers;
    ConvParams pb = make_params(t, LB.weights(P), LB.bias(P),
                                reinterpret_cast<const float*>(s0), last ? out_f32 : reinterpret_cast<float*>(s0), n, h, w, 0, 0.1f);
    pb.out2 = s1;
    HIP_TRY(launch(LB.plan, pb, last ? kEpiResidualF32 : kEpiResidual, m->tune, stream));
    if (keep_step > 0 && !last)
      HIP_TRY(hipMemcpyAsync(reinterpret_cast<float*>(xkeep) + (size_t)l * keep_step, s0, operand16_bytes(m, n, h, w),
                             hipMemcpyDeviceToDevice, stream));
  }
  return DSEN2_OK;
}

namespace dsen2 {

// fp32: x0 | a | t.   bf16, bf16x3: x0 | a (fp32: the last block's output, and a generic first convolution's) | s0 | s1 | t16:
// s0 and t16 operand tensors (bf16: one plane, half an fp32 tensor; bf16x3: two planes), s1 the stream's low halves (one plane)
ForwardWs forward_ws(const dsen2_model* m, int n, int h, int w, char* base) {
  const size_t pix = (size_t)n * h * w;
  const size_t full = align_up(pix * m->feat), half = align_up(pix * m->feat / 2);
  ForwardWs r;
  size_t off = 0;
  auto take = [&](size_t floats) -> float* {
    float* p = base ? reinterpret_cast<float*>(base) + off : nullptr;
    off += floats;
    return p;
  };
  r.x0 = take(align_up(pix * 16));
  r.a = take(full);
  if (m->precision == 0) {
    r.t = take(full);
  } else {
    const size_t operand = m->precision == 2 ? full : half;
    r.s0 = take(operand); r.s1 = take(half); r.t16 = take(operand);
  }
  r.bytes = off * sizeof(float);
  return r;
}

int forward_launches(const dsen2_model* m, const float* x10, const float* x20, const float* x60, float* out, int n, int h, int w,
                     const ForwardWs& B, size_t keep_step, bool x0_packed, hipStream_t stream, const hipEvent_t* ev) {
  const float* P = m->dev_params;
  const int d = m->num_layers;
  if (ev) HIP_TRY(hipEventRecord(ev[0], stream));
  if (int rc = first_layer(m, x10, x20, x60, n, h, w, B, x0_packed, stream)) return rc;
  if (ev) HIP_TRY(hipEventRecord(ev[1], stream));
  if (m->precision != 0 && d > 0) {
    if (keep_step > 0) {
      HIP_TRY((m->precision == 2 ? launch_join3_f32 : launch_join_f32)(B.s0, B.s1, B.x0f, n, h, w, m->feat, stream));
      HIP_TRY(hipMemcpyAsync(B.xkeep, B.s0, operand16_bytes(m, n, h, w), hipMemcpyDeviceToDevice, stream));
    }
    if (int rc = body16(m, B.s0, B.s1, B.t16, B.a, n, h, w, stream, keep_step, B.xkeep)) return rc;
  } else {
    // (the ablation mask is 0 in the product library; a diagnostic build that sets it times the ablated kernels in the
    // inference and in the training forward)
    for (int l = 1; l <= d; ++l) {      // DSen2Net.py:31-32 -> :9-15
      const Layer& LA = m->layers[2 * l - 1];
      const Layer& LB = m->layers[2 * l];
      const float* x_in = B.a + (size_t)(l - 1) * keep_step;
      float* t = B.t + (size_t)(l - 1) * keep_step;
      HIP_TRY(launch(LA.plan, make_params(x_in, LA.weights(P), LA.bias(P), nullptr, t, n, h, w, 0, 0.f), LA.plan.epilogue, m->tune, stream));
      // keep_step = 0: in place on the residual stream: every workgroup reads aux and writes out at its own pixels only
      HIP_TRY(launch(LB.plan, make_params(t, LB.weights(P), LB.bias(P), x_in, B.a + (size_t)l * keep_step, n, h, w, 0, 0.1f),
                     LB.plan.epilogue, m->tune, stream));
    }
  }
  if (ev) HIP_TRY(hipEventRecord(ev[2], stream));
  {
    const Layer& L = m->layers.back();           // DSen2Net.py:35,38,41
    const float* skip = m->c60 > 0 ? x60 : x20;  // utils/DSen2Net.py:38,41
    const float* x_d = B.a + (m->precision == 0 ? (size_t)d * keep_step : 0);     // 16-bit models: the last block's fp32 output
    ConvParams po = make_params(x_d, L.weights(P), L.bias(P), skip, out, n, h, w, m->cout, 0.f);
#ifdef DSEN2_DIAG
    po.diag = g_diag_stamps;
#endif
    HIP_TRY(launch(L.plan, po, L.plan.epilogue, m->tune, stream));
  }
  if (ev) HIP_TRY(hipEventRecord(ev[3], stream));
  return DSEN2_OK;
}

}  // namespace dsen2

// the checks of one inference forward, then its launches (ev: forward_launches)
static int forward(dsen2_model* m, const float* x10, const float* x20, const float* x60, float* out, int n, int h, int w,
                   void* workspace, size_t workspace_bytes, void* stream, const hipEvent_t* ev) {
  if (!m || !x10 || !x20 || !out || !workspace) return fail(DSEN2_ERR_INVALID, "NULL argument");
  if ((m->c60 > 0) != (x60 != nullptr)) return fail(DSEN2_ERR_INVALID, "x60 must be given iff the model has a 60 m input");
  if (!m->loaded) return fail(DSEN2_ERR_NO_WEIGHTS, "dsen2_model_load_weights has not been called");
  if (int rc = check_shape(m, n, h, w)) return rc;
  if (int rc = check_device(m)) return rc;
  const ForwardWs B = forward_ws(m, n, h, w, reinterpret_cast<char*>(workspace));
  if (workspace_bytes < B.bytes) return fail(DSEN2_ERR_WORKSPACE, "workspace %zu < %zu bytes", workspace_bytes, B.bytes);
  return forward_launches(m, x10, x20, x60, out, n, h, w, B, 0, false, (hipStream_t)stream, ev);
}

// `iters` forward passes with four events each (forward_launches); ms[0..3] = mean of (whole forward, first convolution,
// all residual-block convolutions, output convolution) — three consecutive intervals between the same four time stamps,
// so ms[1] + ms[2] + ms[3] = ms[0] by construction; ms[4] = host wall-clock per pass of this instrumented run (enqueue
// of the first pass to completion of the last, / iters): what the events themselves cost shows as ms[4] against an
// un-instrumented loop of the same passes.
//
// `warm` un-instrumented passes are enqueued right before the instrumented ones, with no synchronisation in between: after
// any idle stretch of a few milliseconds (a host-side allocation, a synchronisation followed by host work) this GPU needs
// ~25 launches of the body convolution (~25 ms) to come back to its steady clock — launches are up to 16 % slower meanwhile
// (profiles/r04_ablation.md §2: the per-dispatch timeline) — so intervals measured cold are not the running network's.
static int forward_profile(dsen2_model* m, const float* x10, const float* x20, const float* x60, float* out, int n, int h, int w,
                           void* workspace, size_t workspace_bytes, void* stream, int warm, int iters, float* ms) {
  if (iters <= 0 || iters > 4096 || warm < 0 || warm > 4096 || !ms) return fail(DSEN2_ERR_INVALID, "bad warm / iters / NULL result");
  if (!m) return fail(DSEN2_ERR_INVALID, "NULL model");
  Events evs;
  if (int rc = evs.create(4 * (size_t)iters)) return rc;
  for (int i = 0; i < warm; ++i) {
    int rc = forward(m, x10, x20, x60, out, n, h, w, workspace, workspace_bytes, stream, nullptr);
    if (rc != DSEN2_OK) return rc;
  }
  // (the host clock starts when the warm passes are enqueued, not when they finish: a synchronisation here would be the
  // idle stretch the warm passes exist to avoid; ms[4] is corrected for them below)
  const auto t0 = std::chrono::steady_clock::now();
  for (int i = 0; i < iters; ++i) {
    int rc = forward(m, x10, x20, x60, out, n, h, w, workspace, workspace_bytes, stream, &evs.ev[4 * (size_t)i]);
    if (rc != DSEN2_OK) {
      (void)hipStreamSynchronize((hipStream_t)stream);     // nothing recorded may outlive its event
      return rc;
    }
  }
  HIP_TRY(hipEventSynchronize(evs.ev.back()));
  const auto t1 = std::chrono::steady_clock::now();
  double sum[4] = {0.0, 0.0, 0.0, 0.0};
  for (int i = 0; i < iters; ++i) {
    const hipEvent_t* e = &evs.ev[4 * (size_t)i];
    float v = 0.f;
    HIP_TRY(hipEventElapsedTime(&v, e[0], e[3])); sum[0] += v;
    HIP_TRY(hipEventElapsedTime(&v, e[0], e[1])); sum[1] += v;
    HIP_TRY(hipEventElapsedTime(&v, e[1], e[2])); sum[2] += v;
    HIP_TRY(hipEventElapsedTime(&v, e[2], e[3])); sum[3] += v;
  }
  for (int k = 0; k < 4; ++k) ms[k] = (float)(sum[k] / iters);
  // host wall clock per instrumented pass: enqueue of the first instrumented pass to completion of the last one; when warm
  // passes are still running at t0, the interval from the first instrumented event (GPU clock) is the truthful one
  double wall = std::chrono::duration<double, std::milli>(t1 - t0).count();
  if (warm > 0) {
    float span = 0.f;
    HIP_TRY(hipEventElapsedTime(&span, evs.ev.front(), evs.ev.back()));
    wall = span;
  }
  ms[4] = (float)(wall / iters);
  return DSEN2_OK;
}

// tune: the model-independent kernel structures of this build, or the reference structures (dsen2_conv3x3_nhwc_ref)
static int conv3x3_nhwc(const float* dev_in, const float* host_kernel, const float* host_bias, const float* dev_aux, float* dev_out,
                        int n, int h, int w, int cin, int cout, int epilogue, float res_scale, void* stream_, const Tuning& tune) {
  if (!dev_in || !host_kernel || !host_bias || !dev_out) return fail(DSEN2_ERR_INVALID, "NULL argument");
  if (epilogue != kEpiRelu && epilogue != kEpiResidual && epilogue != kEpiSkipNCHW) return fail(DSEN2_ERR_INVALID, "epilogue %d", epilogue);
  if (epilogue != kEpiRelu && !dev_aux) return fail(DSEN2_ERR_INVALID, "epilogue %d needs dev_aux", epilogue);
  if (int rc = check_shape(nullptr, n, h, w)) return rc;
  // the layer of DSen2Net.py's graph (or of its backward pass) that has this shape and epilogue
  const ConvRole role = epilogue == kEpiSkipNCHW ? ConvRole::Output
                        : cin <= 16 ? (epilogue == kEpiRelu ? ConvRole::First : ConvRole::DgradOutput)
                        : epilogue == kEpiRelu ? ConvRole::BodyA : ConvRole::BodyB;
  ConvPlan pl;
  if (!plan_conv(role, cin, cout, 0, tune, nullptr, &pl) || pl.cin_pad != cin)
    return fail(DSEN2_ERR_INVALID, "unsupported conv %d->%d epilogue %d", cin, cout, epilogue);
  hipStream_t stream = (hipStream_t)stream_;
  std::vector<float> staged(pl.floats);
  pack(pl, host_kernel, host_bias, staged.data());
  return launch_once_with_temp("conv3x3", staged.data(), staged.size() * sizeof(float), stream, [&](char* dev) {
    const float* wpk = reinterpret_cast<const float*>(dev);
    return launch(pl, make_params(dev_in, wpk, wpk + pl.bias_off, dev_aux, dev_out, n, h, w, cout, res_scale), epilogue, tune, stream);
  });
}

// dsen2_conv3x3_body_bf16 (precision 1) and dsen2_conv3x3_body_bf16x3 (precision 2): s0 / s1 = the residual stream's tensors
static int conv3x3_body16(int precision, const void* dev_in, const float* host_kernel, const float* host_bias, void* s0, void* s1,
                          void* dev_out, int n, int h, int w, int feat, int epilogue, float res_scale, void* stream_) {
  const bool x3 = precision == 2;
  if (!dev_in || !host_kernel || !host_bias) return fail(DSEN2_ERR_INVALID, "NULL argument");
  if (feat != 128 && feat != 256) return fail(DSEN2_ERR_INVALID, "feat %d unsupported", feat);
  if (epilogue != kEpiRelu && epilogue != kEpiResidual && epilogue != kEpiResidualF32) return fail(DSEN2_ERR_INVALID, "epilogue %d", epilogue);
  if (epilogue != kEpiRelu && (!s0 || !s1))
    return fail(DSEN2_ERR_INVALID, x3 ? "residual epilogue needs the stream's tensors" : "residual epilogue needs the hi and lo planes");
  if (epilogue != kEpiResidual && !dev_out) return fail(DSEN2_ERR_INVALID, "dev_out is NULL");
  if (int rc = check_shape(nullptr, n, h, w)) return rc;
  hipStream_t stream = (hipStream_t)stream_;
  const Tuning tune = default_tuning();
  ConvPlan pl;
  if (!plan_conv(epilogue == kEpiRelu ? ConvRole::BodyA : ConvRole::BodyB, feat, feat, precision, tune, nullptr, &pl))
    return fail(DSEN2_ERR_INVALID, "feat %d unsupported", feat);
  std::vector<float> staged(pl.floats);
  pack(pl, host_kernel, host_bias, staged.data());
  return launch_once_with_temp(x3 ? "bf16x3 conv" : "bf16 conv", staged.data(), staged.size() * sizeof(float), stream, [&](char* dev) {
    const float* wpk = reinterpret_cast<const float*>(dev);
    ConvParams p = make_params(reinterpret_cast<const float*>(dev_in), wpk, wpk + pl.bias_off, reinterpret_cast<const float*>(s0),
                               reinterpret_cast<float*>(epilogue == kEpiResidual ? s0 : dev_out), n, h, w, 0, res_scale);
    p.out2 = s1;
    return launch(pl, p, epilogue, tune, stream);
  });
}

// the one argument check of dsen2_split_f32 / dsen2_join_f32 / dsen2_split3_f32 / dsen2_join3_f32 (a, b, c: their three tensors)
static int check_split_args(const void* a, const void* b, const void* c_, int n, int h, int w, int c) {
  if (!a || !b || !c_ || n < 0 || h <= 0 || w <= 0 || c <= 0 || c % 8 != 0 || c > 512)
    return fail(DSEN2_ERR_INVALID, "bad argument (c must be a multiple of 8, at most 512)");
  return DSEN2_OK;
}

static int upsample(const float* dev_in, float* dev_out, int planes, int h, int w, int oh, int ow, float post_divisor, void* stream,
                    bool general) {
  if (!dev_in || !dev_out || planes < 0 || h <= 0 || w <= 0 || oh <= 0 || ow <= 0 || post_divisor == 0.f)
    return fail(DSEN2_ERR_INVALID, "bad argument");
  if ((size_t)h * w >= ((size_t)1 << 31) || (size_t)oh * ow >= ((size_t)1 << 31))
    return fail(DSEN2_ERR_INVALID, "plane too large");
  if (planes == 0) return DSEN2_OK;
  HIP_TRY(launch_upsample(dev_in, dev_out, planes, h, w, oh, ow, post_divisor, (hipStream_t)stream, general));
  return DSEN2_OK;
}

static int recompose_rows(const float* dev_patches, int count, int C, int P, int border, float* dev_img, int H, int W, float scale,
                          int row0, int row1, void* stream) {
  if (!dev_patches || !dev_img || count <= 0 || C <= 0 || P <= 0 || border < 0 || H <= 0 || W <= 0)
    return fail(DSEN2_ERR_INVALID, "bad argument");
  hipError_t e = launch_recompose(dev_patches, count, C, P, border, dev_img, H, W, scale, row0, row1, (hipStream_t)stream);
  if (e == hipErrorInvalidValue)
    return fail(DSEN2_ERR_INVALID, "recompose geometry: count=%d P=%d border=%d H=%d W=%d rows [%d, %d)", count, P, border, H, W, row0, row1);
  if (e != hipSuccess) return fail(DSEN2_ERR_HIP, "recompose launch: %s", hipGetErrorString(e));
  return DSEN2_OK;
}

// ---- flips and rotations, the geometric self-ensemble --------------------------------------------------------------------------
// the byte ranges [a, a + a_bytes) and [b, b + b_bytes) share a byte
static bool overlaps(const void* a, size_t a_bytes, const void* b, size_t b_bytes) {
  const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
  return x < y + b_bytes && y < x + a_bytes;
}

// the one argument check of dsen2_dihedral_nchw / dsen2_dihedral_accumulate; *elems = n * c * h * w
static int check_dihedral_args(const void* in, const void* out, int n, int c, int h, int w, int op, size_t* elems) {
  if (!in || !out) return fail(DSEN2_ERR_INVALID, "NULL argument");
  if (n < 0 || c <= 0 || h <= 0 || w <= 0) return fail(DSEN2_ERR_INVALID, "bad shape n=%d c=%d h=%d w=%d", n, c, h, w);
  if (op < 0 || op > 7) return fail(DSEN2_ERR_INVALID, "op %d outside 0..7", op);
  *elems = (size_t)n * c * h * w;
  if (*elems >= ((size_t)1 << 31)) return fail(DSEN2_ERR_INVALID, "tensor of %zu elements (2^31 or more)", *elems);
  if (*elems > 0 && overlaps(in, *elems * sizeof(float), out, *elems * sizeof(float))) return fail(DSEN2_ERR_INVALID, "the output aliases the input");
  return DSEN2_OK;
}

namespace {
// The ensemble's workspace: the forward's | the turned inputs | one member's output (the last two only where a member other
// than the plain forward is asked for).
struct EnsembleWs {
  char* fwd = nullptr;
  size_t fwd_bytes = 0;
  float *x10 = nullptr, *x20 = nullptr, *x60 = nullptr, *y = nullptr;
  size_t bytes = 0;
};
}  // namespace

static EnsembleWs ensemble_ws(const dsen2_model* m, int n, int h, int w, int mask, char* base) {
  const size_t pix = (size_t)n * h * w;
  EnsembleWs r;
  r.fwd = base;
  r.fwd_bytes = forward_ws(m, n, h, w, nullptr).bytes;       // (a function of n * h * w: the same for h x w and w x h)
  size_t off = r.fwd_bytes / sizeof(float);
  auto take = [&](size_t floats) -> float* {
    float* p = base ? reinterpret_cast<float*>(base) + off : nullptr;
    off += align_up(floats);
    return p;
  };
  if (mask & ~1) {
    r.x10 = take(pix * m->c10);
    r.x20 = take(pix * m->c20);
    if (m->c60 > 0) r.x60 = take(pix * m->c60);
    r.y = take(pix * m->cout);
  }
  r.bytes = off * sizeof(float);
  return r;
}

static int check_ensemble_shape(const dsen2_model* m, int n, int h, int w, int mask) {
  if (mask <= 0 || mask > 255) return fail(DSEN2_ERR_INVALID, "ensemble mask %d outside 1..255", mask);
  if (int rc = check_shape(m, n, h, w)) return rc;
  if (int rc = check_shape(m, n, w, h)) return rc;           // the turned orientation
  int cmax = m->cout;
  for (int c : {m->c10, m->c20, m->c60}) cmax = c > cmax ? c : cmax;
  if ((size_t)n * h * w * cmax >= ((size_t)1 << 31))
    return fail(DSEN2_ERR_INVALID, "batch of %d images of %dx%d: a tensor of 2^31 elements or more", n, h, w);
  return DSEN2_OK;
}

static int forward_ensemble(dsen2_model* m, const float* x10, const float* x20, const float* x60, float* out, int n, int h, int w,
                            int mask, void* workspace, size_t workspace_bytes, void* stream_) {
  if (!m || !x10 || !x20 || !out || !workspace) return fail(DSEN2_ERR_INVALID, "NULL argument");
  if ((m->c60 > 0) != (x60 != nullptr)) return fail(DSEN2_ERR_INVALID, "x60 must be given iff the model has a 60 m input");
  if (mask <= 0 || mask > 255) return fail(DSEN2_ERR_INVALID, "ensemble mask %d outside 1..255", mask);
  if (n == 0) return DSEN2_OK;
  if (!m->loaded) return fail(DSEN2_ERR_NO_WEIGHTS, "dsen2_model_load_weights has not been called");
  if (int rc = check_ensemble_shape(m, n, h, w, mask)) return rc;
  if (int rc = check_device(m)) return rc;
  const size_t pix = (size_t)n * h * w;
  const float* const ins[3] = {x10, x20, x60};
  const int cs[3] = {m->c10, m->c20, m->c60};
  for (int k = 0; k < 3; ++k)
    if (ins[k] && overlaps(ins[k], pix * cs[k] * sizeof(float), out, pix * m->cout * sizeof(float)))
      return fail(DSEN2_ERR_INVALID, "the output aliases an input");
  const EnsembleWs E = ensemble_ws(m, n, h, w, mask, reinterpret_cast<char*>(workspace));
  if (workspace_bytes < E.bytes) return fail(DSEN2_ERR_WORKSPACE, "workspace %zu < %zu bytes", workspace_bytes, E.bytes);
  hipStream_t stream = (hipStream_t)stream_;
  int count = 0;
  for (int op = 0; op < 8; ++op) count += (mask >> op) & 1;
  int done = 0;
  for (int op = 0; op < 8; ++op) {
    if (!((mask >> op) & 1)) continue;
    const bool first = done == 0, last = done + 1 == count;
    if (op == 0) {
      // the plain forward, straight into out (always the first member)
      const ForwardWs B = forward_ws(m, n, h, w, E.fwd);
      if (int rc = forward_launches(m, x10, x20, x60, out, n, h, w, B, 0, false, stream, nullptr)) return rc;
    } else {
      const bool tr = op & 1;
      const int th = tr ? w : h, tw = tr ? h : w;                // the turned images
      float* const turned[3] = {E.x10, E.x20, E.x60};
      for (int k = 0; k < 3; ++k)
        if (ins[k]) HIP_TRY(launch_dihedral(ins[k], turned[k], n, cs[k], h, w, op, nullptr, false, stream));
      const ForwardWs B = forward_ws(m, n, th, tw, E.fwd);
      if (int rc = forward_launches(m, E.x10, E.x20, E.x60, E.y, n, th, tw, B, 0, false, stream, nullptr)) return rc;
      if (first) HIP_TRY(launch_dihedral(E.y, out, n, m->cout, th, tw, op, nullptr, true, stream));
      else HIP_TRY(launch_dihedral_accumulate(E.y, out, n, m->cout, h, w, op, last ? count : 0, stream));
    }
    ++done;
  }
  return DSEN2_OK;
}

extern "C" {

const char* dsen2_version(void) {
#ifdef DSEN2_DIAG
  return "dsen2_hip 0.3-diag (gfx950; fp32 MFMA 32x32x2 / bf16 MFMA 16x16x32 / bf16x3; DIAGNOSTIC build)";
#else
  return "dsen2_hip 0.3 (gfx950; fp32 MFMA 32x32x2 / bf16 MFMA 16x16x32 / bf16x3)";
#endif
}
const char* dsen2_last_error(void) { return g_err; }

#ifdef DSEN2_DIAG
// Diagnostic build only — not declared in include/dsen2_hip.h.  The integer keys and values are the wire format of tools/ and
// of DSEN2_DIAG_SET, translated to Tuning's typed fields here and nowhere else.  key 0: fp32 body convolution (15 default, 11-14
// and 16-19 the other forms of conv3x3_body32.hip, 0 one tile per workgroup — and the first convolution over all 16 padded channels);
// key 1: timing-only ablation mask of the persistent body kernels (outputs are WRONG while non-zero); key 2: output-layer
// kernel (2 = matrix cores where the shape fits, 3 = vector units, 0 = padded MFMA block).
int dsen2_diag_set(int key, int value) {
  Tuning& t = g_diag_tuning;
  switch (key) {
    case 0:
      if (value != 0 && (value < 11 || value > 19)) return fail(DSEN2_ERR_INVALID, "body variant %d unknown", value);
      t.first = value == 0 ? FirstKernel::Tile16 : FirstKernel::Direct;
      t.body = value == 0 ? BodyKernel::Tile : BodyKernel::Body32;
      t.body32 = value == 0 ? Body32Form::DeferAsym : static_cast<Body32Form>(value - 11);
      return DSEN2_OK;
    case 2:
      if (value != 0 && value != 2 && value != 3) return fail(DSEN2_ERR_INVALID, "output variant %d unknown", value);
      t.out = value == 2 ? OutKernel::MfmaThenValu : value == 3 ? OutKernel::Valu : OutKernel::Tile;
      return DSEN2_OK;
    case 1: t.ablate = value; return DSEN2_OK;
    case 3: t.grid_cap = value; return DSEN2_OK;       // at most `value` workgroups for the bf16 body kernel (0 = one per CU): per-CU vs chip-wide limits
    case 4: t.chain = value; return DSEN2_OK;          // 0 = always launch the bf16 body convolutions layer by layer (A/B against the chain kernel)
    case 5: t.first_ablate = value; return DSEN2_OK;   // timing-only ablation mask of the first convolution (1 no stores, 2 no MFMAs, 4 no gather)
    case 6: t.out_ablate = value; return DSEN2_OK;     // timing-only ablation mask of the matrix-core output convolution (conv3x3_out_mfma.hip)
  }
  return fail(DSEN2_ERR_INVALID, "unknown diagnostic key %d", key);
}
// device buffer (>= 64 KiB) the stamping build of the bf16 body kernel (ablation mask 32) writes s_memtime values to
int dsen2_diag_set_stamps(void* dev_buffer) {
  g_diag_stamps = reinterpret_cast<unsigned long long*>(dev_buffer);
  return DSEN2_OK;
}
#endif

int dsen2_device_count(void) {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return fail(DSEN2_ERR_NO_DEVICE, "hipGetDeviceCount: %s", hipGetErrorString(e));
  }
  int good = 0;
  for (int i = 0; i < n; ++i) {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, i) == hipSuccess && strncmp(prop.gcnArchName, "gfx950", 6) == 0) ++good;
  }
  return good;
}

int dsen2_model_create(dsen2_model** out, int c10, int c20, int c60, int num_layers, int feature_size, int precision) {
  return guarded([&]() -> int {
    if (!out) return fail(DSEN2_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (c10 <= 0 || c20 <= 0 || c60 < 0 || num_layers < 0) return fail(DSEN2_ERR_INVALID, "bad channel/layer counts");
    if (feature_size != 128 && feature_size != 256)
      return fail(DSEN2_ERR_INVALID, "feature_size %d unsupported (128 or 256)", feature_size);
    if (precision < 0 || precision > 2)
      return fail(DSEN2_ERR_INVALID, "precision %d unknown (0 = fp32, 1 = bf16 operands, 2 = bf16x3)", precision);
    const int cin = c10 + c20 + c60;
    const int cout = c60 > 0 ? c60 : c20;   // utils/DSen2Net.py:35 — input_shape[-1][0]
    // (cout <= cin - 1 <= 15: inside what the output layer's plan takes, 32)
    if (cin > 16) return fail(DSEN2_ERR_INVALID, "%d input channels > 16", cin);
    dsen2_model* m = new (std::nothrow) dsen2_model();
    if (!m) return fail(DSEN2_ERR_INVALID, "out of host memory");
    m->c10 = c10; m->c20 = c20; m->c60 = c60; m->cin = cin; m->cout = cout;
    m->num_layers = num_layers; m->feat = feature_size; m->precision = precision;
    m->dev_params = nullptr; m->loaded = false; m->train = nullptr;
    m->tune = default_tuning();
    if (hipGetDevice(&m->device) != hipSuccess) {
      delete m;
      return fail(DSEN2_ERR_NO_DEVICE, "no HIP device");
    }
    if (!plan_network(c10, c20, c60, num_layers, feature_size, precision, m->tune, m)) {
      delete m;
      return fail(DSEN2_ERR_INVALID, "no kernel for a layer of this network");
    }
    *out = m;
    return DSEN2_OK;
  });
}

void dsen2_model_destroy(dsen2_model* m) {
  if (!m) return;
  train_state_destroy(m->train);
  if (m->dev_params) (void)hipFree(m->dev_params);
  delete m;
}

size_t dsen2_model_num_params(const dsen2_model* m) { return m ? m->n_params : 0; }

int dsen2_model_load_weights(dsen2_model* m, const float* host_flat, size_t count) {
  return guarded([&]() -> int {
    if (!m || !host_flat) return fail(DSEN2_ERR_INVALID, "NULL argument");
    if (count != m->n_params)
      return fail(DSEN2_ERR_INVALID, "expected %zu parameters, got %zu", m->n_params, count);
    if (int rc = check_device(m)) return rc;      // the packed weights are allocated on the current device
    std::vector<float> staged(m->dev_param_floats);
    for (const Layer& L : m->layers) {
      const float* k = host_flat + L.flat_off;
      pack(L.plan, k, k + (size_t)9 * L.plan.cin * L.plan.cout, staged.data() + L.off);
    }
    if (!m->dev_params) HIP_TRY(hipMalloc((void**)&m->dev_params, m->dev_param_floats * sizeof(float)));
    HIP_TRY(hipMemcpy(m->dev_params, staged.data(), m->dev_param_floats * sizeof(float), hipMemcpyHostToDevice));
    m->loaded = true;
    if (m->train_planes() == 2) m->host_flat.assign(host_flat, host_flat + count);
    if (m->train) return train_state_after_load(m);     // a model being trained: its master weights follow
    return DSEN2_OK;
  });
}

int dsen2_model_workspace_bytes(const dsen2_model* m, int n, int h, int w, size_t* bytes) {
  if (!m || !bytes || n <= 0 || h <= 0 || w <= 0) return fail(DSEN2_ERR_INVALID, "bad argument");
  *bytes = forward_ws(m, n, h, w, nullptr).bytes;
  return DSEN2_OK;
}

int dsen2_model_forward(dsen2_model* m, const float* x10, const float* x20, const float* x60, float* out, int n, int h, int w,
                        void* workspace, size_t workspace_bytes, void* stream) {
  return guarded([&] { return forward(m, x10, x20, x60, out, n, h, w, workspace, workspace_bytes, stream, nullptr); });
}

int dsen2_model_body_launches(const dsen2_model* m, int n, int h, int w) {
  return guarded([&]() -> int {
    if (!m) return fail(DSEN2_ERR_INVALID, "NULL model");
    if (int rc = check_shape(m, n, h, w)) return rc;
    if (int rc = check_device(m)) return rc;
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
      return fail(DSEN2_ERR_NO_DEVICE, "no HIP device");
    return may_chain(m) && body16w_chain_patches_per_wg(n, h, w, m->feat, cus) > 0 ? 1 : 2 * m->num_layers;
  });
}

int dsen2_model_forward_timed(dsen2_model* m, const float* x10, const float* x20, const float* x60, float* out, int n, int h, int w,
                              void* workspace, size_t workspace_bytes, void* stream, int iters, float* body_ms_per_launch) {
  return guarded([&]() -> int {
    if (!body_ms_per_launch) return fail(DSEN2_ERR_INVALID, "NULL result");
    if (!m || m->num_layers <= 0) return fail(DSEN2_ERR_INVALID, "model has no residual blocks");
    float ms[5];
    int rc = forward_profile(m, x10, x20, x60, out, n, h, w, workspace, workspace_bytes, stream, 0, iters, ms);
    if (rc == DSEN2_OK) *body_ms_per_launch = ms[2] / (2.0f * m->num_layers);
    return rc;
  });
}

int dsen2_model_forward_profile(dsen2_model* m, const float* x10, const float* x20, const float* x60, float* out, int n, int h,
                                int w, void* workspace, size_t workspace_bytes, void* stream, int warm, int iters, float* ms5) {
  return guarded([&] { return forward_profile(m, x10, x20, x60, out, n, h, w, workspace, workspace_bytes, stream, warm, iters, ms5); });
}

int dsen2_conv3x3_nhwc(const float* dev_in, const float* host_kernel, const float* host_bias, const float* dev_aux, float* dev_out,
                       int n, int h, int w, int cin, int cout, int epilogue, float res_scale, void* stream) {
  return guarded([&] {
    return conv3x3_nhwc(dev_in, host_kernel, host_bias, dev_aux, dev_out, n, h, w, cin, cout, epilogue, res_scale, stream, default_tuning());
  });
}

int dsen2_conv3x3_nhwc_ref(const float* dev_in, const float* host_kernel, const float* host_bias, const float* dev_aux,
                           float* dev_out, int n, int h, int w, int cin, int cout, int epilogue, float res_scale, void* stream) {
  return guarded([&] {
    return conv3x3_nhwc(dev_in, host_kernel, host_bias, dev_aux, dev_out, n, h, w, cin, cout, epilogue, res_scale, stream,
                        Tuning::reference());
  });
}

int dsen2_split_f32(const float* dev_in, void* dev_hi, void* dev_lo, int n, int h, int w, int c, void* stream) {
  return guarded([&]() -> int {
    if (int rc = check_split_args(dev_in, dev_hi, dev_lo, n, h, w, c)) return rc;
    if (n == 0) return DSEN2_OK;
    HIP_TRY(launch_split_f32(dev_in, dev_hi, dev_lo, n, h, w, c, (hipStream_t)stream));
    return DSEN2_OK;
  });
}

int dsen2_join_f32(const void* dev_hi, const void* dev_lo, float* dev_out, int n, int h, int w, int c, void* stream) {
  return guarded([&]() -> int {
    if (int rc = check_split_args(dev_hi, dev_lo, dev_out, n, h, w, c)) return rc;
    if (n == 0) return DSEN2_OK;
    HIP_TRY(launch_join_f32(dev_hi, dev_lo, dev_out, n, h, w, c, (hipStream_t)stream));
    return DSEN2_OK;
  });
}

int dsen2_split3_f32(const float* dev_in, void* dev_hx, void* dev_lo, int n, int h, int w, int c, void* stream) {
  return guarded([&]() -> int {
    if (int rc = check_split_args(dev_in, dev_hx, dev_lo, n, h, w, c)) return rc;
    if (n == 0) return DSEN2_OK;
    HIP_TRY(launch_split3_f32(dev_in, dev_hx, dev_lo, n, h, w, c, (hipStream_t)stream));
    return DSEN2_OK;
  });
}

int dsen2_join3_f32(const void* dev_hx, const void* dev_lo16, float* dev_out, int n, int h, int w, int c, void* stream) {
  return guarded([&]() -> int {
    if (int rc = check_split_args(dev_hx, dev_lo16, dev_out, n, h, w, c)) return rc;
    if (n == 0) return DSEN2_OK;
    HIP_TRY(launch_join3_f32(dev_hx, dev_lo16, dev_out, n, h, w, c, (hipStream_t)stream));
    return DSEN2_OK;
  });
}

int dsen2_conv3x3_body_bf16(const void* dev_in_bf16, const float* host_kernel, const float* host_bias, void* dev_res_hi,
                            void* dev_res_lo, void* dev_out, int n, int h, int w, int feat, int epilogue, float res_scale,
                            void* stream) {
  return guarded([&] {
    return conv3x3_body16(1, dev_in_bf16, host_kernel, host_bias, dev_res_hi, dev_res_lo, dev_out, n, h, w, feat, epilogue, res_scale, stream);
  });
}

int dsen2_conv3x3_body_bf16x3(const void* dev_in_planes, const float* host_kernel, const float* host_bias, void* dev_res_hx,
                              void* dev_res_lo, void* dev_out, int n, int h, int w, int feat, int epilogue, float res_scale,
                              void* stream) {
  return guarded([&] {
    return conv3x3_body16(2, dev_in_planes, host_kernel, host_bias, dev_res_hx, dev_res_lo, dev_out, n, h, w, feat, epilogue, res_scale, stream);
  });
}

int dsen2_conv3x3_first_planes(const float* dev_x10, const float* dev_x20, const float* dev_x60, int c10, int c20, int c60,
                               const float* host_kernel, const float* host_bias, int feat, int precision, void* dev_out,
                               void* dev_out2, int n, int h, int w, void* stream_) {
  return guarded([&]() -> int {
    if (!dev_x10 || !dev_x20 || !host_kernel || !host_bias || !dev_out || !dev_out2) return fail(DSEN2_ERR_INVALID, "NULL argument");
    if ((c60 > 0) != (dev_x60 != nullptr)) return fail(DSEN2_ERR_INVALID, "dev_x60 must be given iff c60 > 0");
    if (feat != 128 && feat != 256) return fail(DSEN2_ERR_INVALID, "feat %d unsupported", feat);
    if (precision != 1 && precision != 2) return fail(DSEN2_ERR_INVALID, "precision %d (1 = bf16 operands, 2 = bf16x3)", precision);
    if (c10 != 4 || c20 != 6 || (c60 != 0 && c60 != 2)) return fail(DSEN2_ERR_INVALID, "band groups %d + %d + %d (4 + 6 (+ 2) only)", c10, c20, c60);
    if (int rc = check_shape(nullptr, n, h, w)) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    const BandGroups bands{c10, c20, c60};
    ConvPlan pl;
    if (!plan_conv(ConvRole::First, c10 + c20 + c60, feat, precision, default_tuning(), &bands, &pl) || !pl.first16_planes)
      return fail(DSEN2_ERR_INVALID, "no bf16 first convolution for this shape");
    std::vector<float> staged(pl.floats);
    pack(pl, host_kernel, host_bias, staged.data());
    return launch_once_with_temp("first convolution (bf16 matrix cores)", staged.data(), staged.size() * sizeof(float), stream, [&](char* dev) {
      const float* buf = reinterpret_cast<const float*>(dev);
      ConvParams p = make_params(dev_x10, buf + pl.first16_off, buf + pl.bias_off, dev_x20, reinterpret_cast<float*>(dev_out), n, h, w, 0, 0.f);
      p.out2 = dev_out2;
      return launch_conv3x3_first16(p, FirstInputs{dev_x60, c10, c20, c60}, feat, precision == 2, stream);
    });
  });
}

int dsen2_model_time_body_conv(dsen2_model* m, int layer, const float* dev_in, const float* dev_aux, float* dev_out, int n, int h,
                               int w, int iters, void* stream_, float* ms_per_launch) {
  return guarded([&]() -> int {
    if (!m || !dev_in || !dev_out || !ms_per_launch || iters <= 0) return fail(DSEN2_ERR_INVALID, "bad argument");
    if (!m->loaded) return fail(DSEN2_ERR_NO_WEIGHTS, "weights not loaded");
    if (layer < 1 || layer > 2 * m->num_layers) return fail(DSEN2_ERR_INVALID, "layer %d out of range", layer);
    if (int rc = check_shape(m, n, h, w)) return rc;
    if (int rc = check_device(m)) return rc;
    const Layer& L = m->layers[layer];
    if (L.plan.kernel == ConvKernel::Body16x3) return fail(DSEN2_ERR_INVALID, "dsen2_model_time_body_conv: not available for precision 2 (use dsen2_model_forward_profile)");
    if (L.plan.epilogue == kEpiResidual && !dev_aux) return fail(DSEN2_ERR_INVALID, "residual layer needs dev_aux");
    hipStream_t stream = (hipStream_t)stream_;
    const float* P = m->dev_params;
    ConvParams p = make_params(dev_in, L.weights(P), L.bias(P), dev_aux, dev_out, n, h, w, 0, 0.1f);
    int epi = L.plan.epilogue;
    if (L.plan.kernel == ConvKernel::Body16 && epi == kEpiResidual) {
      // dev_aux = hi plane followed by lo plane (one fp32-sized buffer), updated in place; the last block's layer
      // writes fp32 to dev_out instead
      const bool last = layer == 2 * m->num_layers;
      p.out2 = reinterpret_cast<char*>(const_cast<float*>(dev_aux)) + (size_t)n * h * w * m->feat * 2;
      p.out = last ? dev_out : const_cast<float*>(dev_aux);
      epi = last ? kEpiResidualF32 : kEpiResidual;
    }
#ifdef DSEN2_DIAG
    p.diag = g_diag_stamps;
#endif
    auto launch = [&]() -> hipError_t { return dsen2::launch(L.plan, p, epi, m->tune, stream); };
    Events ev;
    if (int rc = ev.create(2)) return rc;
    // warm-up: ~25 ms of this kernel bring the chip back to its steady clock after an idle stretch (see forward_profile)
    for (int i = 0; i < kWarmLaunches; ++i) HIP_TRY(launch());
    HIP_TRY(hipEventRecord(ev.ev[0], stream));
    for (int i = 0; i < iters; ++i) HIP_TRY(launch());
    HIP_TRY(hipEventRecord(ev.ev[1], stream));
    HIP_TRY(hipEventSynchronize(ev.ev[1]));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, ev.ev[0], ev.ev[1]));
    *ms_per_launch = ms / iters;
    return DSEN2_OK;
  });
}

int dsen2_upsample_mirror_bilinear(const float* dev_in, float* dev_out, int planes, int h, int w, int oh, int ow, float post_divisor,
                                   void* stream) {
  return guarded([&] { return upsample(dev_in, dev_out, planes, h, w, oh, ow, post_divisor, stream, false); });
}

int dsen2_upsample_mirror_bilinear_ref(const float* dev_in, float* dev_out, int planes, int h, int w, int oh, int ow,
                                       float post_divisor, void* stream) {
  return guarded([&] { return upsample(dev_in, dev_out, planes, h, w, oh, ow, post_divisor, stream, true); });
}

int dsen2_tile_gather(const float* dev_img, int H, int W, int C, int border, const int* dev_origins, int count, int P, float divisor,
                      float* dev_patches, void* stream) {
  return guarded([&]() -> int {
    if (!dev_img || !dev_patches || (!dev_origins && count > 0) || H <= 0 || W <= 0 || C <= 0 || border < 0 ||
        count < 0 || P <= 0 || divisor == 0.f)
      return fail(DSEN2_ERR_INVALID, "bad argument");
    if (border > H || border > W) return fail(DSEN2_ERR_INVALID, "border %d larger than the image", border);
    if ((size_t)C * P * P >= ((size_t)1 << 31)) return fail(DSEN2_ERR_INVALID, "patch too large");
    HIP_TRY(launch_tile_gather(dev_img, H, W, C, border, dev_origins, count, P, divisor, dev_patches, (hipStream_t)stream));
    return DSEN2_OK;
  });
}

int dsen2_recompose(const float* dev_patches, int count, int C, int P, int border, float* dev_img, int H, int W, float scale,
                    void* stream) {
  return guarded([&] { return recompose_rows(dev_patches, count, C, P, border, dev_img, H, W, scale, 0, H, stream); });
}

int dsen2_recompose_rows(const float* dev_patches, int count, int C, int P, int border, float* dev_img, int H, int W, float scale,
                         int row0, int row1, void* stream) {
  return guarded([&] { return recompose_rows(dev_patches, count, C, P, border, dev_img, H, W, scale, row0, row1, stream); });
}

int dsen2_dihedral_nchw(const float* dev_in, float* dev_out, int n, int c, int h, int w, int op, const int* dev_ops, int inverse,
                        void* stream) {
  return guarded([&]() -> int {
    size_t elems = 0;
    if (int rc = check_dihedral_args(dev_in, dev_out, n, c, h, w, op, &elems)) return rc;
    if (dev_ops && h != w) return fail(DSEN2_ERR_INVALID, "per-sample ops need square images (an odd rotation swaps H and W), got %dx%d", h, w);
    if (elems == 0) return DSEN2_OK;
    HIP_TRY(launch_dihedral(dev_in, dev_out, n, c, h, w, op, dev_ops, inverse != 0, (hipStream_t)stream));
    return DSEN2_OK;
  });
}

int dsen2_dihedral_accumulate(const float* dev_in, float* dev_acc, int n, int c, int h, int w, int op, int count, void* stream) {
  return guarded([&]() -> int {
    size_t elems = 0;
    if (int rc = check_dihedral_args(dev_in, dev_acc, n, c, h, w, op, &elems)) return rc;
    if (count < 0) return fail(DSEN2_ERR_INVALID, "count %d is negative", count);
    if (elems == 0) return DSEN2_OK;
    HIP_TRY(launch_dihedral_accumulate(dev_in, dev_acc, n, c, h, w, op, count, (hipStream_t)stream));
    return DSEN2_OK;
  });
}

int dsen2_model_ensemble_workspace_bytes(const dsen2_model* m, int n, int h, int w, int mask, size_t* bytes) {
  if (!m || !bytes) return fail(DSEN2_ERR_INVALID, "NULL argument");
  if (int rc = check_ensemble_shape(m, n, h, w, mask)) return rc;
  *bytes = ensemble_ws(m, n, h, w, mask, nullptr).bytes;
  return DSEN2_OK;
}

int dsen2_model_forward_ensemble(dsen2_model* m, const float* dev_x10, const float* dev_x20, const float* dev_x60, float* dev_out,
                                 int n, int h, int w, int mask, void* dev_workspace, size_t workspace_bytes, void* stream) {
  return guarded([&] {
    return forward_ensemble(m, dev_x10, dev_x20, dev_x60, dev_out, n, h, w, mask, dev_workspace, workspace_bytes, stream);
  });
}

}  // extern "C"
