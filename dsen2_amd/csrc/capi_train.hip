// capi_train.hip — the training entries of libdsen2_hip.so (include/dsen2_hip.h, "training"): the gradients of one batch
// (forward with every activation kept, MAE loss, backward), the device copy of the weights and the Nadam step.
//
// Backward structure (g = dL/dx_l, walking the residual blocks from the last one):
//   du  = [t_l > 0] * 0.1 * dgradB(g)        dWB = 0.1 * wgrad(t_l, g)      dbB = 0.1 * sum g
//   dWA = wgrad(x_{l-1}, du)                dbA = sum du                    g  <- g + dgradA(du)
// dgrad runs on the forward kernels with flipped, transposed weights W'[ky][kx][co][ci] = W[2-ky][2-kx][ci][co] and a zero
// bias: dgradA + g is the body kernel's residual epilogue with res_scale 1; dgradB is the same epilogue on a zeroed buffer
// with res_scale 0.1, then the ReLU mask.  wgrad is conv3x3_wgrad.hip; loss, masks and Nadam are train_ops.hip.
//
// The weights of a model being trained live as a device keras-flat vector (the master copy).  Every packed buffer — the
// forward's and the dgrad weights — is rebuilt from it by one gather kernel whose index maps are made once, by running the
// host packers on per-layer iota + 1 kernels (0 = padding): the repacked weights are the host packers' bits by construction.
#include <cstdarg>
#include <cstdio>
#include <cstring>

#include "capi_internal.h"

using namespace dsen2;

namespace dsen2 {

struct TrainState {
  float* master = nullptr;     // [n_params] keras-flat
  int* fwd_map = nullptr;      // [dev_param_floats]: 1 + flat index of every packed forward value, 0 = padding
  float* dg = nullptr;         // flipped / transposed packed weights of every layer with an input gradient, + zero bias
  int* dg_map = nullptr;       // [dg_floats]
  size_t dg_floats = 0;
  std::vector<size_t> dg_off;  // per layer: float offset of its dgrad weights in dg (layer 0: none)
  size_t zero_off = 0;         // feat zeros (the dgrad convolutions' bias)
  ConvPlan body_plan{}, out_plan{};   // the dgrad convolutions of a body layer (F -> F) and of the output layer (16 -> F)
};

void train_state_destroy(TrainState* t) {
  if (!t) return;
  if (t->master) (void)hipFree(t->master);
  if (t->fwd_map) (void)hipFree(t->fwd_map);
  if (t->dg) (void)hipFree(t->dg);
  if (t->dg_map) (void)hipFree(t->dg_map);
  delete t;
}

}  // namespace dsen2

namespace {

int check_train_model(const dsen2_model* m) {
  if (!m) return fail(DSEN2_ERR_INVALID, "NULL model");
  if (m->precision != 0) return fail(DSEN2_ERR_INVALID, "training needs an fp32 model");
  return check_device(m);
}

// map value for a packed float that holds iota value v of the layer starting at flat_off: 1 + flat index, 0 = padding
inline int map_value(float v, size_t flat_off) { return v > 0.f ? (int)(flat_off + (size_t)v) : 0; }

int ensure_train_state(dsen2_model* m) {
  if (m->train) return DSEN2_OK;
  if (m->n_params >= (size_t)0x7fffffff) return fail(DSEN2_ERR_INVALID, "too many parameters for the gather maps");
  TrainState* t = new TrainState();
  struct Guard {                    // freed unless handed to the model
    TrainState* t;
    ~Guard() { train_state_destroy(t); }
  } guard{t};
  const int F = m->feat;
  const size_t L = m->layers.size();
  if (!plan_conv(ConvRole::DgradBody, F, F, 0, m->tune, nullptr, &t->body_plan) ||
      !plan_conv(ConvRole::DgradOutput, 16, F, 0, m->tune, nullptr, &t->out_plan))
    return fail(DSEN2_ERR_INVALID, "no dgrad kernel for feature size %d", F);
  // forward map: dsen2_model_load_weights' pack() on iota kernels (kernel, then bias, as in the keras-flat array)
  std::vector<int> fmap(m->dev_param_floats, 0);
  std::vector<float> buf, k;
  for (const Layer& Ly : m->layers) {
    const size_t nk = (size_t)9 * Ly.plan.cin * Ly.plan.cout;
    k.resize(nk + Ly.plan.cout);
    for (size_t i = 0; i < k.size(); ++i) k[i] = (float)(i + 1);
    buf.resize(Ly.plan.floats);
    pack(Ly.plan, k.data(), k.data() + nk, buf.data());
    for (size_t i = 0; i < buf.size(); ++i) fmap[Ly.off + i] = map_value(buf[i], Ly.flat_off);
  }
  // dgrad weights: W'[tap][c'][o'] = W[8 - tap][o'][c'] for the body layers (F -> F) and the output layer (16 -> F, the
  // outputs zero-padded to 16 input channels); layer 0 needs no input gradient
  t->dg_off.assign(L, 0);
  size_t off = 0;
  for (size_t li = 1; li < L; ++li) {
    t->dg_off[li] = off;
    off += align_up((li + 1 == L ? t->out_plan : t->body_plan).weight_floats);
  }
  t->zero_off = off;
  off += align_up((size_t)F);
  t->dg_floats = off;
  std::vector<int> dmap(off, 0);
  for (size_t li = 1; li < L; ++li) {
    const int ci = m->layers[li].plan.cin, co = m->layers[li].plan.cout;
    const ConvPlan& g = li + 1 == L ? t->out_plan : t->body_plan;    // the dgrad convolution: forward outputs -> forward inputs
    k.assign((size_t)9 * g.cin * g.cout, 0.f);
    for (int tap = 0; tap < 9; ++tap)
      for (int c = 0; c < co; ++c)
        for (int o = 0; o < ci; ++o)
          k[((size_t)tap * g.cin + c) * g.cout + o] = (float)(((size_t)(8 - tap) * ci + o) * co + c + 1);
    buf.resize(g.weight_floats);
    pack(g, k.data(), nullptr, buf.data());
    for (size_t i = 0; i < buf.size(); ++i) dmap[t->dg_off[li] + i] = map_value(buf[i], m->layers[li].flat_off);
  }
  HIP_TRY(hipMalloc((void**)&t->master, m->n_params * sizeof(float)));
  HIP_TRY(hipMalloc((void**)&t->fwd_map, fmap.size() * sizeof(int)));
  HIP_TRY(hipMalloc((void**)&t->dg, t->dg_floats * sizeof(float)));
  HIP_TRY(hipMalloc((void**)&t->dg_map, dmap.size() * sizeof(int)));
  HIP_TRY(hipMemcpy(t->fwd_map, fmap.data(), fmap.size() * sizeof(int), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(t->dg_map, dmap.data(), dmap.size() * sizeof(int), hipMemcpyHostToDevice));
  m->train = t;
  guard.t = nullptr;
  if (m->loaded) return train_state_after_load(m);
  return DSEN2_OK;
}

// master <- the packed forward weights (inverse gather), dgrad weights <- master
int refresh_from_packed(dsen2_model* m, hipStream_t s) {
  TrainState* t = m->train;
  HIP_TRY(launch_scatter(t->master, m->dev_params, t->fwd_map, m->dev_param_floats, s));
  HIP_TRY(launch_gather(t->dg, t->master, t->dg_map, t->dg_floats, s));
  return DSEN2_OK;
}

struct TrainWs {
  float *in16, *out, *gpad, *G, *DU, *wg, *loss2;
  double* partial;
  std::vector<float*> X, T;
  size_t keep_step;   // X[l] = X[0] + l * keep_step, T[l] = T[1] + (l - 1) * keep_step: what forward_launches writes
  size_t wg_floats;
  size_t bytes;
};

// carve (or, with base == NULL, only size) the training workspace
TrainWs carve(const dsen2_model* m, int n, int h, int w, char* base) {
  const size_t pix = (size_t)n * h * w, F = m->feat;
  const size_t full = align_up(pix * F);
  size_t wg = wgrad_workspace_floats(n, h, w, m->feat, m->feat);
  const size_t wg1 = wgrad_workspace_floats(n, h, w, 16, m->feat), wg2 = wgrad_workspace_floats(n, h, w, m->feat, 16);
  if (wg1 > wg) wg = wg1;
  if (wg2 > wg) wg = wg2;
  TrainWs r;
  size_t off = 0;
  auto take = [&](size_t floats) -> float* {
    float* p = base ? reinterpret_cast<float*>(base) + off : nullptr;
    off += align_up(floats);
    return p;
  };
  r.in16 = take(pix * 16);
  r.keep_step = full;
  for (int l = 0; l <= m->num_layers; ++l) r.X.push_back(take(full));
  r.T.push_back(nullptr);
  for (int l = 1; l <= m->num_layers; ++l) r.T.push_back(take(full));
  r.out = take(pix * m->cout);
  r.gpad = take(pix * 16);
  r.G = take(full);
  r.DU = take(full);
  r.wg = take(wg);
  r.wg_floats = wg;
  r.partial = reinterpret_cast<double*>(take(2 * mae_loss_partial_doubles(pix)));
  r.loss2 = take(2);
  r.bytes = off * sizeof(float);
  return r;
}

}  // namespace

namespace dsen2 {

int train_state_after_load(dsen2_model* m) {
  if (int rc = refresh_from_packed(m, nullptr)) return rc;
  HIP_TRY(hipStreamSynchronize(nullptr));
  return DSEN2_OK;
}

}  // namespace dsen2

extern "C" {

int dsen2_model_train_workspace_bytes(const dsen2_model* m, int n, int h, int w, size_t* bytes) {
  return guarded([&]() -> int {
    if (!bytes) return fail(DSEN2_ERR_INVALID, "NULL argument");
    if (int rc = check_train_model(m)) return rc;
    if (int rc = check_shape(m, n, h, w)) return rc;
    *bytes = carve(m, n, h, w, nullptr).bytes;
    return DSEN2_OK;
  });
}

int dsen2_model_gradients(dsen2_model* m, const float* x10, const float* x20, const float* x60, const float* target, float* dev_out,
                          float* grad, float* loss2, int n, int h, int w, void* ws, size_t ws_bytes, void* stream_) {
  return guarded([&]() -> int {
    if (int rc = check_train_model(m)) return rc;
    if (!x10 || !x20 || !target || !grad || !ws) return fail(DSEN2_ERR_INVALID, "NULL argument");
    if ((m->c60 > 0) != (x60 != nullptr)) return fail(DSEN2_ERR_INVALID, "x60 must be given iff the model has a 60 m input");
    if (!m->loaded) return fail(DSEN2_ERR_NO_WEIGHTS, "no weights: dsen2_model_load_weights or dsen2_model_set_weights_device first");
    if (int rc = check_shape(m, n, h, w)) return rc;
    const size_t need = carve(m, n, h, w, nullptr).bytes;
    if (ws_bytes < need) return fail(DSEN2_ERR_WORKSPACE, "workspace %zu < %zu bytes", ws_bytes, need);
    if (int rc = ensure_train_state(m)) return rc;
    TrainWs W = carve(m, n, h, w, reinterpret_cast<char*>(ws));
    if (!dev_out) dev_out = W.out;
    if (!loss2) loss2 = W.loss2;
    hipStream_t s = (hipStream_t)stream_;
    const TrainState* t = m->train;
    const float* zero = t->dg + t->zero_off;
    const int F = m->feat, d = m->num_layers;
    const size_t pix = (size_t)n * h * w;
    const Layer& LO = m->layers.back();

    // ---- forward, every activation kept: dsen2_model_forward's own launches (forward_launches), so the same bits.  The
    // NHWC16 input is packed here whatever the first convolution reads: the first layer's weight gradient needs it ----
    HIP_TRY(launch_pack_inputs(x10, x20, x60, m->c10, m->c20, m->c60, W.in16, n, h, w, s));
    ForwardWs B;
    B.x0 = W.in16;
    B.a = W.X[0];
    B.t = d > 0 ? W.T[1] : nullptr;
    if (int rc = forward_launches(m, x10, x20, x60, dev_out, n, h, w, B, W.keep_step, true, s, nullptr)) return rc;

    // ---- loss, output layer ----
    HIP_TRY(launch_mae_loss_grad(dev_out, target, W.gpad, W.partial, loss2, n, m->cout, h, w, s));
    auto wgrad = [&](const float* a, int ca, const float* g, int cg, const Layer& Ly, float scale) -> hipError_t {
      float* dw = grad + Ly.flat_off;
      return launch_conv3x3_wgrad(a, ca, g, cg, n, h, w, Ly.plan.cin, Ly.plan.cout, scale, dw, dw + (size_t)9 * Ly.plan.cin * Ly.plan.cout, W.wg,
                                  W.wg_floats, s);
    };
    HIP_TRY(wgrad(W.X[d], F, W.gpad, 16, LO, 1.f));
    const size_t fbytes = pix * F * sizeof(float);
    HIP_TRY(hipMemsetAsync(W.G, 0, fbytes, s));
    HIP_TRY(launch(t->out_plan, make_params(W.gpad, t->dg + t->dg_off[m->layers.size() - 1], zero, W.G, W.G, n, h, w, 0, 1.f), kEpiResidual,
                   m->tune, s));
    // ---- residual blocks, last to first ----
    for (int l = d; l >= 1; --l) {
      const Layer& LA = m->layers[2 * l - 1];
      const Layer& LB = m->layers[2 * l];
      HIP_TRY(wgrad(W.T[l], F, W.G, F, LB, 0.1f));
      HIP_TRY(hipMemsetAsync(W.DU, 0, fbytes, s));
      HIP_TRY(launch(t->body_plan, make_params(W.G, t->dg + t->dg_off[2 * l], zero, W.DU, W.DU, n, h, w, 0, 0.1f), kEpiResidual, m->tune, s));
      HIP_TRY(launch_relu_mask(W.DU, W.T[l], pix * F, s));
      HIP_TRY(wgrad(W.X[l - 1], F, W.DU, F, LA, 1.f));
      HIP_TRY(launch(t->body_plan, make_params(W.DU, t->dg + t->dg_off[2 * l - 1], zero, W.G, W.G, n, h, w, 0, 1.f), kEpiResidual, m->tune, s));
    }
    // ---- first convolution ----
    HIP_TRY(launch_relu_mask(W.G, W.X[0], pix * F, s));
    HIP_TRY(wgrad(W.in16, 16, W.G, F, m->layers[0], 1.f));
    return DSEN2_OK;
  });
}

int dsen2_model_get_weights(const dsen2_model* mc, float* dev_flat, void* stream) {
  return guarded([&]() -> int {
    if (int rc = check_train_model(mc)) return rc;
    if (!dev_flat) return fail(DSEN2_ERR_INVALID, "NULL argument");
    if (!mc->loaded) return fail(DSEN2_ERR_NO_WEIGHTS, "no weights loaded");
    dsen2_model* m = const_cast<dsen2_model*>(mc);     // the training state is a cache of the weights the model holds
    if (int rc = ensure_train_state(m)) return rc;
    HIP_TRY(hipMemcpyAsync(dev_flat, m->train->master, m->n_params * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return DSEN2_OK;
  });
}

int dsen2_model_set_weights_device(dsen2_model* m, const float* dev_flat, void* stream) {
  return guarded([&]() -> int {
    if (int rc = check_train_model(m)) return rc;
    if (!dev_flat) return fail(DSEN2_ERR_INVALID, "NULL argument");
    if (!m->dev_params) HIP_TRY(hipMalloc((void**)&m->dev_params, m->dev_param_floats * sizeof(float)));
    if (int rc = ensure_train_state(m)) return rc;
    hipStream_t s = (hipStream_t)stream;
    TrainState* t = m->train;
    if (dev_flat != t->master)
      HIP_TRY(hipMemcpyAsync(t->master, dev_flat, m->n_params * sizeof(float), hipMemcpyDeviceToDevice, s));
    HIP_TRY(launch_gather(m->dev_params, t->master, t->fwd_map, m->dev_param_floats, s));
    HIP_TRY(launch_gather(t->dg, t->master, t->dg_map, t->dg_floats, s));
    m->loaded = true;
    return DSEN2_OK;
  });
}

int dsen2_nadam_step(float* p, const float* g, float* m, float* v, size_t count, float lr, float b1, float b2, float eps, float mc_t,
                     float mc_t1, float ms_new, float ms_next, float b2_pow_t, void* stream) {
  return guarded([&]() -> int {
    if (count > 0 && (!p || !g || !m || !v)) return fail(DSEN2_ERR_INVALID, "NULL argument");
    HIP_TRY(launch_nadam(p, g, m, v, count, lr, b1, b2, eps, mc_t, mc_t1, ms_new, ms_next, b2_pow_t, (hipStream_t)stream));
    return DSEN2_OK;
  });
}

int dsen2_conv3x3_wgrad(const float* dev_a, const float* dev_g, float* dev_dw, float* dev_db, int n, int h, int w, int ca, int cg,
                        int ci, int co, float scale, void* stream) {
  return guarded([&]() -> int {
    if (!dev_a || !dev_g || !dev_dw || !dev_db) return fail(DSEN2_ERR_INVALID, "NULL argument");
    if (n <= 0 || h <= 0 || w <= 0 || ci <= 0 || co <= 0 || ci > ca || co > cg) return fail(DSEN2_ERR_INVALID, "bad shape");
    const size_t wf = wgrad_workspace_floats(n, h, w, ca, cg);
    if (wf == 0) return fail(DSEN2_ERR_INVALID, "no wgrad kernel for %d -> %d channels", ca, cg);
    hipStream_t s = (hipStream_t)stream;
    return launch_once_with_temp("wgrad", nullptr, wf * sizeof(float), s, [&](char* dev) {
      return launch_conv3x3_wgrad(dev_a, ca, dev_g, cg, n, h, w, ci, co, scale, dev_dw, dev_db, reinterpret_cast<float*>(dev), wf, s);
    });
  });
}

}  // extern "C"
