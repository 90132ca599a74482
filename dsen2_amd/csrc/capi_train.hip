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
//
// A precision-2 (bf16x3) model with residual blocks trains in its own formats (gradients_x3): the forward on the bf16x3 per-layer
// kernels with t_l and copies of the stream's operand tensor hx kept; g lives as a precision-2 residual stream (hx, lo16), so
// g + dgradA(du) is the X3 body kernel's in-place residual epilogue and 0.1 * dgradB(g) its fp32 epilogue over a zero stream,
// followed by launch_mask_split3 (ReLU mask of t_l, du as a two-plane operand tensor); the block weight gradients are
// conv3x3_wgrad16.hip.  The first and the output convolution's gradients stay on the fp32 kernels, reached through
// launch_split3_f32 / launch_join3_f32.  The master copy is still the fp32 keras-flat vector; the packed buffers hold bf16
// (hi, lo) planes next to fp32 words, so their maps have one entry per 16-bit half (launch_gather16) and are read off the host
// packers digit by digit: an iota does not survive a bf16 split, but a base-128 digit d packed as the value d + 1 does (exact
// in bf16: it lands in the hi plane, the lo plane gets 0), and packed as 1 + (d + 1) * 2^-16 it lands in the lo plane (hi = 1).
// Three passes of each kind give every half its flat index and its kind.  The body layers share one plan and so one map.
//
// Mixed precision (dsen2_model_set_train_precision(m, 1) on an fp32 model with residual blocks; gradients_amp): the model, its
// master weights and its packed fp32 buffers stay as they are, and the training state owns a COMPANION: a precision-1 plan of
// the same network with the packed buffers a precision-1 model of these weights would hold (first16 image, bf16 body planes,
// fp32 output layer) and its own 16-bit training state (the bf16 flipped / transposed dgrad weights), both rebuilt from the
// one master vector by launch_gather16 after every weight change — the same maps, read off the precision-1 host packers.  The
// step is gradients_x3 with one-plane tensors: the companion's forward layer by layer, t_l (bf16, RNE) and the stream's hi
// plane kept; g as a precision-1 residual stream (hi, lo) = exact fp32, hi = (u + 0x8000) >> 16 the dgrads' and conv-B wgrad's
// operand; 0.1 * dgradB(hi(g)) through the fp32 epilogue over a zero stream, du = bf16_rne of its masked value
// (launch_mask_round16); g + dgradA(du) in place; the block weight gradients on the one-plane instance of conv3x3_wgrad16.hip
// (db = the sum of the bf16 operand g).  Loss, output layer and first layer as in gradients_x3: fp32 kernels on fp32 tensors.
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <stdexcept>

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
  // a 16-bit plan with residual blocks (a precision-2 model; the precision-1 companion of a mixed-precision step): launch_gather16
  // maps of the first layer's, a body layer's and the output layer's forward buffer and of a body layer's and the output layer's
  // dgrad weights (fwd_map / dg_map stay NULL)
  bool packed16 = false;
  int* map16[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  size_t dg_body_stride = 0;          // floats between the dgrad weights of consecutive body layers
  // mixed precision: the precision-1 companion plan (owned; its own state has packed16 set and borrows `master`)
  dsen2_model* amp = nullptr;
  bool owns_master = true;
};
enum { kMapFirst = 0, kMapBody = 1, kMapOut = 2, kMapDgBody = 3, kMapDgOut = 4 };

void train_state_destroy(TrainState* t) {
  if (!t) return;
  if (t->amp) {
    train_state_destroy(t->amp->train);
    if (t->amp->dev_params) (void)hipFree(t->amp->dev_params);
    delete t->amp;
  }
  if (t->master && t->owns_master) (void)hipFree(t->master);
  if (t->fwd_map) (void)hipFree(t->fwd_map);
  if (t->dg) (void)hipFree(t->dg);
  if (t->dg_map) (void)hipFree(t->dg_map);
  for (int* p : t->map16)
    if (p) (void)hipFree(p);
  delete t;
}

}  // namespace dsen2

namespace {

int check_train_model(const dsen2_model* m) {
  if (!m) return fail(DSEN2_ERR_INVALID, "NULL model");
  if (m->precision == 1) return fail(DSEN2_ERR_INVALID, "training needs an fp32 model or a bf16x3 one (precision 0 or 2), not bf16 operands");
  return check_device(m);
}

// map value for a packed float that holds iota value v of the layer starting at flat_off: 1 + flat index, 0 = padding
inline int map_value(float v, size_t flat_off) { return v > 0.f ? (int)(flat_off + (size_t)v) : 0; }

// One 16-bit-granular gather map (launch_gather16) of a layer buffer, read off the host packers: src[e] = the index, inside the
// layer's keras-flat values, of element e of the kernel (+ bias) handed to pack(), or -1 for a zero.  See the file comment.
// Three base-128 digits hold indices below 2^21 (the largest layer, 256 -> 256, has 590,080 values); a larger one is refused
// (std::length_error: DSEN2_ERR_INTERNAL through guarded()), never aliased.
std::vector<int> build_gather16_map(const ConvPlan& pl, bool with_bias, const std::vector<int>& src) {
  const size_t nk = (size_t)9 * pl.cin * pl.cout;
  const size_t words = with_bias ? pl.floats : pl.weight_floats;
  for (int v : src)
    if (v >= (1 << 21)) throw std::length_error("gather map: a layer of more than 2^21 values");
  std::vector<float> k(src.size()), buf[6];
  for (int pass = 0; pass < 6; ++pass) {
    const int shift = 7 * (pass % 3);
    for (size_t e = 0; e < src.size(); ++e) {
      const float digit1 = (float)(((src[e] >> shift) & 127) + 1);
      k[e] = src[e] < 0 ? 0.f : pass < 3 ? digit1 : 1.f + digit1 * (1.f / 65536.f);
    }
    buf[pass].assign(words, 0.f);
    pack(pl, k.data(), with_bias ? k.data() + nk : nullptr, buf[pass].data());
  }
  auto half_value = [&](int pass, size_t i, int hf) {        // the bf16 in half hf of word i, as a float
    uint32_t u;
    memcpy(&u, &buf[pass][i], 4);
    u = hf ? u & 0xffff0000u : u << 16;
    float f;
    memcpy(&f, &u, 4);
    return f;
  };
  const bool packed16 = pl.kernel == ConvKernel::Body16 || pl.kernel == ConvKernel::Body16x3;
  std::vector<int> map(2 * words, 0);
  for (size_t i = 0; i < words; ++i) {
    const bool is16 = (packed16 && i < pl.weight_floats) || (pl.first16_planes && i >= pl.first16_off);
    if (!is16) {
      if (buf[0][i] == 0.f) continue;
      int idx = 0;
      for (int q = 0; q < 3; ++q) idx |= ((int)buf[q][i] - 1) << (7 * q);
      map[2 * i] = 4 * (idx + 1) + kGatherF32Low;
      map[2 * i + 1] = 4 * (idx + 1) + kGatherF32High;
      continue;
    }
    for (int hf = 0; hf < 2; ++hf) {
      int idx = 0;
      if (half_value(0, i, hf) != 0.f) {
        for (int q = 0; q < 3; ++q) idx |= ((int)half_value(q, i, hf) - 1) << (7 * q);
        map[2 * i + hf] = 4 * (idx + 1) + kGatherHi;
      } else if (half_value(3, i, hf) != 0.f) {
        for (int q = 0; q < 3; ++q) idx |= ((int)(half_value(3 + q, i, hf) * 65536.f) - 1) << (7 * q);
        map[2 * i + hf] = 4 * (idx + 1) + kGatherLo;
      }
    }
  }
  return map;
}

struct StateGuard {                 // freed unless handed to the model
  TrainState* t;
  ~StateGuard() { train_state_destroy(t); }
};

int upload_map(const std::vector<int>& map, int** dev) {
  HIP_TRY(hipMalloc((void**)dev, map.size() * sizeof(int)));
  HIP_TRY(hipMemcpy(*dev, map.data(), map.size() * sizeof(int), hipMemcpyHostToDevice));
  return DSEN2_OK;
}

// the training state of a 16-bit plan with residual blocks: a precision-2 model (master == NULL: its own master vector), or the
// precision-1 companion of a mixed-precision step, which borrows its owner's
int ensure_train_state_x3(dsen2_model* m, float* master = nullptr) {
  TrainState* t = new TrainState();
  StateGuard guard{t};
  t->packed16 = true;
  const int F = m->feat;
  const size_t L = m->layers.size();
  if (!plan_conv(ConvRole::DgradBody, F, F, m->precision, m->tune, nullptr, &t->body_plan) ||
      !plan_conv(ConvRole::DgradOutput, 16, F, 0, m->tune, nullptr, &t->out_plan))
    return fail(DSEN2_ERR_INVALID, "no dgrad kernel for feature size %d", F);
  auto iota = [](size_t count) {
    std::vector<int> v(count);
    for (size_t i = 0; i < count; ++i) v[i] = (int)i;
    return v;
  };
  // the packers' kernel of a dgrad convolution: W'[tap][c'][o'] = W[8 - tap][o'][c'] (ensure_train_state)
  auto flipped = [](const ConvPlan& g, int ci, int co) {
    std::vector<int> v((size_t)9 * g.cin * g.cout, -1);
    for (int tap = 0; tap < 9; ++tap)
      for (int c = 0; c < co; ++c)
        for (int o = 0; o < ci; ++o) v[((size_t)tap * g.cin + c) * g.cout + o] = (int)(((size_t)(8 - tap) * ci + o) * co + c);
    return v;
  };
  const Layer &L0 = m->layers[0], &L1 = m->layers[1], &LO = m->layers[L - 1];
  auto layer_values = [](const Layer& Ly) { return (size_t)9 * Ly.plan.cin * Ly.plan.cout + Ly.plan.cout; };
  if (int rc = upload_map(build_gather16_map(L0.plan, true, iota(layer_values(L0))), &t->map16[kMapFirst])) return rc;
  if (int rc = upload_map(build_gather16_map(L1.plan, true, iota(layer_values(L1))), &t->map16[kMapBody])) return rc;
  if (int rc = upload_map(build_gather16_map(LO.plan, true, iota(layer_values(LO))), &t->map16[kMapOut])) return rc;
  if (int rc = upload_map(build_gather16_map(t->body_plan, false, flipped(t->body_plan, F, F)), &t->map16[kMapDgBody])) return rc;
  if (int rc = upload_map(build_gather16_map(t->out_plan, false, flipped(t->out_plan, LO.plan.cin, LO.plan.cout)), &t->map16[kMapDgOut]))
    return rc;
  t->dg_body_stride = align_up(t->body_plan.weight_floats);
  t->dg_off.assign(L, 0);
  size_t off = 0;
  for (size_t li = 1; li < L; ++li) {
    t->dg_off[li] = off;
    off += li + 1 == L ? align_up(t->out_plan.weight_floats) : t->dg_body_stride;
  }
  t->zero_off = off;
  off += align_up((size_t)F);
  t->dg_floats = off;
  t->owns_master = master == nullptr;
  t->master = master;
  if (t->owns_master) HIP_TRY(hipMalloc((void**)&t->master, m->n_params * sizeof(float)));
  HIP_TRY(hipMalloc((void**)&t->dg, t->dg_floats * sizeof(float)));
  HIP_TRY(hipMemset(t->dg, 0, t->dg_floats * sizeof(float)));        // the zero bias; the padding between the layers
  m->train = t;
  guard.t = nullptr;
  if (t->owns_master && m->loaded) return train_state_after_load(m);
  return DSEN2_OK;
}

// the packed forward buffers (fwd) and / or the dgrad weights of a 16-bit plan <- master
int repack_x3(dsen2_model* m, bool fwd, hipStream_t s) {
  TrainState* t = m->train;
  const size_t L = m->layers.size();
  const Layer &L0 = m->layers[0], &L1 = m->layers[1], &LO = m->layers[L - 1];
  const size_t body_values = (size_t)9 * m->feat * m->feat + m->feat;
  if (fwd) {
    HIP_TRY(launch_gather16(m->dev_params + L0.off, t->master + L0.flat_off, t->map16[kMapFirst], L0.plan.floats, 1, 0, 0, s));
    HIP_TRY(launch_gather16(m->dev_params + L1.off, t->master + L1.flat_off, t->map16[kMapBody], L1.plan.floats, 2 * m->num_layers,
                            L1.plan.floats, body_values, s));
    HIP_TRY(launch_gather16(m->dev_params + LO.off, t->master + LO.flat_off, t->map16[kMapOut], LO.plan.floats, 1, 0, 0, s));
  }
  HIP_TRY(launch_gather16(t->dg + t->dg_off[1], t->master + L1.flat_off, t->map16[kMapDgBody], t->body_plan.weight_floats,
                          2 * m->num_layers, t->dg_body_stride, body_values, s));
  HIP_TRY(launch_gather16(t->dg + t->dg_off[L - 1], t->master + LO.flat_off, t->map16[kMapDgOut], t->out_plan.weight_floats, 1, 0, 0, s));
  return DSEN2_OK;
}

// the precision-1 companion of a mixed-precision step: the same network planned with bf16 operands, its packed buffers allocated
// (filled by repack_x3) and its 16-bit training state on the owner's master vector
int create_amp_companion(const dsen2_model* m, float* master, dsen2_model** out) {
  struct Guard {
    dsen2_model* c;
    ~Guard() {
      if (!c) return;
      train_state_destroy(c->train);
      if (c->dev_params) (void)hipFree(c->dev_params);
      delete c;
    }
  } g{new dsen2_model()};
  dsen2_model* c = g.c;
  c->c10 = m->c10; c->c20 = m->c20; c->c60 = m->c60; c->cin = m->cin; c->cout = m->cout;
  c->num_layers = m->num_layers; c->feat = m->feat; c->precision = 1; c->device = m->device; c->tune = m->tune;
  c->dev_params = nullptr; c->loaded = false; c->train = nullptr;
  if (!plan_network(m->c10, m->c20, m->c60, m->num_layers, m->feat, 1, c->tune, c) || c->n_params != m->n_params)
    return fail(DSEN2_ERR_INVALID, "no bf16 kernel for a layer of this network");
  HIP_TRY(hipMalloc((void**)&c->dev_params, c->dev_param_floats * sizeof(float)));
  if (int rc = ensure_train_state_x3(c, master)) return rc;
  *out = c;
  g.c = nullptr;
  return DSEN2_OK;
}

int ensure_train_state(dsen2_model* m) {
  if (m->train) return DSEN2_OK;
  if (m->n_params >= (size_t)0x7fffffff) return fail(DSEN2_ERR_INVALID, "too many parameters for the gather maps");
  if (m->trains_x3()) return ensure_train_state_x3(m);
  TrainState* t = new TrainState();
  StateGuard guard{t};
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
  // (mixed precision: the step runs on the companion's bf16 dgrad weights; the fp32 ones are neither built nor kept)
  const bool own_dgrad = !m->trains_amp();
  std::vector<int> dmap;
  if (own_dgrad) {
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
    dmap.assign(off, 0);
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
  }
  HIP_TRY(hipMalloc((void**)&t->master, m->n_params * sizeof(float)));
  HIP_TRY(hipMalloc((void**)&t->fwd_map, fmap.size() * sizeof(int)));
  HIP_TRY(hipMemcpy(t->fwd_map, fmap.data(), fmap.size() * sizeof(int), hipMemcpyHostToDevice));
  if (own_dgrad) {
    HIP_TRY(hipMalloc((void**)&t->dg, t->dg_floats * sizeof(float)));
    HIP_TRY(hipMalloc((void**)&t->dg_map, dmap.size() * sizeof(int)));
    HIP_TRY(hipMemcpy(t->dg_map, dmap.data(), dmap.size() * sizeof(int), hipMemcpyHostToDevice));
  }
  if (m->trains_amp())
    if (int rc = create_amp_companion(m, t->master, &t->amp)) return rc;
  m->train = t;
  guard.t = nullptr;
  if (m->loaded) return train_state_after_load(m);
  return DSEN2_OK;
}

// master <- the packed forward weights (inverse gather), dgrad weights (where the state has its own) <- master
int refresh_from_packed(dsen2_model* m, hipStream_t s) {
  TrainState* t = m->train;
  HIP_TRY(launch_scatter(t->master, m->dev_params, t->fwd_map, m->dev_param_floats, s));
  if (t->dg) HIP_TRY(launch_gather(t->dg, t->master, t->dg_map, t->dg_floats, s));
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

// ---- precision 2 with residual blocks ----
struct TrainWs3 {
  float *in16, *a32, *x0f, *out, *gpad, *g32, *wg, *loss2;
  char *hx, *lo16, *xkeep, *tkeep, *ghx, *glo, *du, *zhx, *zlo;     // 16-bit tensors
  double* partial;
  size_t keep_step;   // floats between the kept x_l (hx copies) and between the kept t_l
  size_t wg_floats;
  size_t bytes;
};

TrainWs3 carve_x3(const dsen2_model* m, int n, int h, int w, char* base) {
  const size_t pix = (size_t)n * h * w, F = m->feat;
  const size_t full = align_up(pix * F), half = align_up(pix * F / 2);     // a two-plane 16-bit tensor is `full` floats
  size_t wg = wgrad16_workspace_floats(n, h, w, m->feat);
  const size_t wg1 = wgrad_workspace_floats(n, h, w, 16, m->feat), wg2 = wgrad_workspace_floats(n, h, w, m->feat, 16);
  if (wg1 > wg) wg = wg1;
  if (wg2 > wg) wg = wg2;
  TrainWs3 r;
  size_t off = 0;
  auto take = [&](size_t floats) -> float* {
    float* p = base ? reinterpret_cast<float*>(base) + off : nullptr;
    off += align_up(floats);
    return p;
  };
  auto take16 = [&](size_t floats) { return reinterpret_cast<char*>(take(floats)); };
  const size_t d = (size_t)m->num_layers;
  r.in16 = take(pix * 16);
  r.a32 = take(full);
  r.x0f = take(full);
  r.hx = take16(full);
  r.lo16 = take16(half);
  r.keep_step = full;
  r.xkeep = take16(d * full);      // hx of x_0 .. x_{d-1}
  r.tkeep = take16(d * full);      // t_1 .. t_d
  r.out = take(pix * m->cout);
  r.gpad = take(pix * 16);
  r.g32 = take(full);
  r.ghx = take16(full);
  r.glo = take16(half);
  r.du = take16(full);
  r.zhx = take16(full);
  r.zlo = take16(half);
  r.wg = take(wg);
  r.wg_floats = wg;
  r.partial = reinterpret_cast<double*>(take(2 * mae_loss_partial_doubles(pix)));
  r.loss2 = take(2);
  r.bytes = off * sizeof(float);
  return r;
}

// ---- mixed precision: an fp32 model's step on its precision-1 companion ----
struct TrainWsAmp {
  float *in16, *a32, *x0f, *out, *gpad, *g32, *wg, *loss2;
  char *hi, *lo, *xkeep, *tkeep, *ghi, *glo, *du, *zhi, *zlo;     // one-plane 16-bit tensors
  double* partial;
  size_t keep_step;   // floats between the kept hi planes of x_l and between the kept t_l
  size_t wg_floats;
  size_t bytes;
};

TrainWsAmp carve_amp(const dsen2_model* m, int n, int h, int w, char* base) {
  const size_t pix = (size_t)n * h * w, F = m->feat;
  const size_t full = align_up(pix * F), half = align_up(pix * F / 2);     // a one-plane 16-bit tensor is `half` floats
  size_t wg = wgrad16_workspace_floats(n, h, w, m->feat);
  const size_t wg1 = wgrad_workspace_floats(n, h, w, 16, m->feat), wg2 = wgrad_workspace_floats(n, h, w, m->feat, 16);
  if (wg1 > wg) wg = wg1;
  if (wg2 > wg) wg = wg2;
  TrainWsAmp r;
  size_t off = 0;
  auto take = [&](size_t floats) -> float* {
    float* p = base ? reinterpret_cast<float*>(base) + off : nullptr;
    off += align_up(floats);
    return p;
  };
  auto take16 = [&](size_t floats) { return reinterpret_cast<char*>(take(floats)); };
  const size_t d = (size_t)m->num_layers;
  r.in16 = take(pix * 16);
  r.a32 = take(full);
  r.x0f = take(full);
  r.hi = take16(half);
  r.lo = take16(half);
  r.keep_step = half;
  r.xkeep = take16(d * half);      // hi of x_0 .. x_{d-1}
  r.tkeep = take16(d * half);      // t_1 .. t_d
  r.out = take(pix * m->cout);
  r.gpad = take(pix * 16);
  r.g32 = take(full);
  r.ghi = take16(half);
  r.glo = take16(half);
  r.du = take16(half);
  r.zhi = take16(half);
  r.zlo = take16(half);
  r.wg = take(wg);
  r.wg_floats = wg;
  r.partial = reinterpret_cast<double*>(take(2 * mae_loss_partial_doubles(pix)));
  r.loss2 = take(2);
  r.bytes = off * sizeof(float);
  return r;
}

size_t train_ws_bytes(const dsen2_model* m, int n, int h, int w) {
  return m->trains_x3()    ? carve_x3(m, n, h, w, nullptr).bytes
         : m->trains_amp() ? carve_amp(m, n, h, w, nullptr).bytes
                           : carve(m, n, h, w, nullptr).bytes;
}

// dsen2_model_gradients of an fp32 model with train precision 1 (arguments checked, training state present): on the companion
// plan c; see the file comment
int gradients_amp(dsen2_model* m, const float* x10, const float* x20, const float* x60, const float* target, float* dev_out, float* grad,
                  float* loss2, int n, int h, int w, void* ws, hipStream_t s) {
  TrainWsAmp W = carve_amp(m, n, h, w, reinterpret_cast<char*>(ws));
  if (!dev_out) dev_out = W.out;
  if (!loss2) loss2 = W.loss2;
  const dsen2_model* c = m->train->amp;
  const TrainState* t = c->train;
  const float* zero = t->dg + t->zero_off;
  const int F = c->feat, d = c->num_layers;
  const size_t pix = (size_t)n * h * w;
  const size_t fbytes = pix * F * sizeof(float);
  const Layer& LO = c->layers.back();
  auto kept = [&](char* base, int l) { return base + (size_t)l * W.keep_step * sizeof(float); };

  // ---- forward on the precision-1 per-layer launches, t_l and the hi plane of every x_l kept ----
  HIP_TRY(launch_pack_inputs(x10, x20, x60, c->c10, c->c20, c->c60, W.in16, n, h, w, s));
  ForwardWs B;
  B.x0 = W.in16; B.a = W.a32; B.hi = W.hi; B.lo = W.lo; B.tbf = W.tkeep; B.xkeep = W.xkeep; B.x0f = W.x0f;
  if (int rc = forward_launches(c, x10, x20, x60, dev_out, n, h, w, B, W.keep_step, true, s, nullptr)) return rc;

  // ---- loss, output layer (fp32 kernels) ----
  HIP_TRY(launch_mae_loss_grad(dev_out, target, W.gpad, W.partial, loss2, n, c->cout, h, w, s));
  auto wgrad32 = [&](const float* a, int ca, const float* g, int cg, const Layer& Ly) -> hipError_t {
    float* dw = grad + Ly.flat_off;
    return launch_conv3x3_wgrad(a, ca, g, cg, n, h, w, Ly.plan.cin, Ly.plan.cout, 1.f, dw, dw + (size_t)9 * Ly.plan.cin * Ly.plan.cout, W.wg,
                                W.wg_floats, s);
  };
  auto wgrad16 = [&](const void* a, const void* g, const Layer& Ly, float scale) -> hipError_t {
    float* dw = grad + Ly.flat_off;
    return launch_conv3x3_wgrad16_bf16(a, g, n, h, w, F, scale, dw, dw + (size_t)9 * F * F, W.wg, W.wg_floats, s);
  };
  HIP_TRY(wgrad32(W.a32, F, W.gpad, 16, LO));
  HIP_TRY(hipMemsetAsync(W.g32, 0, fbytes, s));
  HIP_TRY(launch(t->out_plan, make_params(W.gpad, t->dg + t->dg_off[c->layers.size() - 1], zero, W.g32, W.g32, n, h, w, 0, 1.f), kEpiResidual,
                 c->tune, s));
  // g as a precision-1 residual stream; the zero stream 0.1 * dgradB is added to (its fp32 epilogue never writes it)
  HIP_TRY(launch_split_f32(W.g32, W.ghi, W.glo, n, h, w, F, s));
  HIP_TRY(hipMemsetAsync(W.zhi, 0, fbytes / 2, s));
  HIP_TRY(hipMemsetAsync(W.zlo, 0, fbytes / 2, s));
  // ---- residual blocks, last to first ----
  for (int l = d; l >= 1; --l) {
    const Layer& LA = c->layers[2 * l - 1];
    const Layer& LB = c->layers[2 * l];
    const char* t_l = kept(W.tkeep, l - 1);
    HIP_TRY(wgrad16(t_l, W.ghi, LB, 0.1f));
    ConvParams pb = make_params(reinterpret_cast<const float*>(W.ghi), t->dg + t->dg_off[2 * l], zero, reinterpret_cast<const float*>(W.zhi),
                                W.g32, n, h, w, 0, 0.1f);
    pb.out2 = W.zlo;
    HIP_TRY(launch(t->body_plan, pb, kEpiResidualF32, c->tune, s));
    HIP_TRY(launch_mask_round16(W.g32, t_l, W.du, n, h, w, F, s));
    HIP_TRY(wgrad16(kept(W.xkeep, l - 1), W.du, LA, 1.f));
    ConvParams pa = make_params(reinterpret_cast<const float*>(W.du), t->dg + t->dg_off[2 * l - 1], zero, reinterpret_cast<const float*>(W.ghi),
                                reinterpret_cast<float*>(W.ghi), n, h, w, 0, 1.f);
    pa.out2 = W.glo;
    HIP_TRY(launch(t->body_plan, pa, kEpiResidual, c->tune, s));
  }
  // ---- first convolution (fp32 kernels) ----
  HIP_TRY(launch_join_f32(W.ghi, W.glo, W.g32, n, h, w, F, s));
  HIP_TRY(launch_relu_mask(W.g32, W.x0f, pix * F, s));
  HIP_TRY(wgrad32(W.in16, 16, W.g32, F, c->layers[0]));
  return DSEN2_OK;
}

// dsen2_model_gradients of a precision-2 model (arguments checked, training state present); see the file comment
int gradients_x3(dsen2_model* m, const float* x10, const float* x20, const float* x60, const float* target, float* dev_out, float* grad,
                 float* loss2, int n, int h, int w, void* ws, hipStream_t s) {
  TrainWs3 W = carve_x3(m, n, h, w, reinterpret_cast<char*>(ws));
  if (!dev_out) dev_out = W.out;
  if (!loss2) loss2 = W.loss2;
  const TrainState* t = m->train;
  const float* zero = t->dg + t->zero_off;
  const int F = m->feat, d = m->num_layers;
  const size_t pix = (size_t)n * h * w;
  const size_t fbytes = pix * F * sizeof(float);
  const Layer& LO = m->layers.back();
  auto kept = [&](char* base, int l) { return base + (size_t)l * W.keep_step * sizeof(float); };

  // ---- forward on the precision-2 per-layer launches, t_l and hx of every x_l kept ----
  HIP_TRY(launch_pack_inputs(x10, x20, x60, m->c10, m->c20, m->c60, W.in16, n, h, w, s));
  ForwardWs B;
  B.x0 = W.in16; B.a = W.a32; B.hx = W.hx; B.lo16 = W.lo16; B.t2 = W.tkeep; B.xkeep = W.xkeep; B.x0f = W.x0f;
  if (int rc = forward_launches(m, x10, x20, x60, dev_out, n, h, w, B, W.keep_step, true, s, nullptr)) return rc;

  // ---- loss, output layer (fp32 kernels) ----
  HIP_TRY(launch_mae_loss_grad(dev_out, target, W.gpad, W.partial, loss2, n, m->cout, h, w, s));
  auto wgrad32 = [&](const float* a, int ca, const float* g, int cg, const Layer& Ly) -> hipError_t {
    float* dw = grad + Ly.flat_off;
    return launch_conv3x3_wgrad(a, ca, g, cg, n, h, w, Ly.plan.cin, Ly.plan.cout, 1.f, dw, dw + (size_t)9 * Ly.plan.cin * Ly.plan.cout, W.wg,
                                W.wg_floats, s);
  };
  auto wgrad16 = [&](const void* a, const void* g, const Layer& Ly, float scale) -> hipError_t {
    float* dw = grad + Ly.flat_off;
    return launch_conv3x3_wgrad16(a, g, n, h, w, F, scale, dw, dw + (size_t)9 * F * F, W.wg, W.wg_floats, s);
  };
  HIP_TRY(wgrad32(W.a32, F, W.gpad, 16, LO));
  HIP_TRY(hipMemsetAsync(W.g32, 0, fbytes, s));
  HIP_TRY(launch(t->out_plan, make_params(W.gpad, t->dg + t->dg_off[m->layers.size() - 1], zero, W.g32, W.g32, n, h, w, 0, 1.f), kEpiResidual,
                 m->tune, s));
  // g as a precision-2 residual stream; the zero stream 0.1 * dgradB is added to (its epilogue never writes it)
  HIP_TRY(launch_split3_f32(W.g32, W.ghx, W.glo, n, h, w, F, s));
  HIP_TRY(hipMemsetAsync(W.zhx, 0, fbytes, s));
  HIP_TRY(hipMemsetAsync(W.zlo, 0, fbytes / 2, s));
  // ---- residual blocks, last to first ----
  for (int l = d; l >= 1; --l) {
    const Layer& LA = m->layers[2 * l - 1];
    const Layer& LB = m->layers[2 * l];
    const char* t_l = kept(W.tkeep, l - 1);
    HIP_TRY(wgrad16(t_l, W.ghx, LB, 0.1f));
    ConvParams pb = make_params(reinterpret_cast<const float*>(W.ghx), t->dg + t->dg_off[2 * l], zero, reinterpret_cast<const float*>(W.zhx),
                                W.g32, n, h, w, 0, 0.1f);
    pb.out2 = W.zlo;
    HIP_TRY(launch(t->body_plan, pb, kEpiResidualF32, m->tune, s));
    HIP_TRY(launch_mask_split3(W.g32, t_l, W.du, n, h, w, F, s));
    HIP_TRY(wgrad16(kept(W.xkeep, l - 1), W.du, LA, 1.f));
    ConvParams pa = make_params(reinterpret_cast<const float*>(W.du), t->dg + t->dg_off[2 * l - 1], zero, reinterpret_cast<const float*>(W.ghx),
                                reinterpret_cast<float*>(W.ghx), n, h, w, 0, 1.f);
    pa.out2 = W.glo;
    HIP_TRY(launch(t->body_plan, pa, kEpiResidual, m->tune, s));
  }
  // ---- first convolution (fp32 kernels) ----
  HIP_TRY(launch_join3_f32(W.ghx, W.glo, W.g32, n, h, w, F, s));
  HIP_TRY(launch_relu_mask(W.g32, W.x0f, pix * F, s));
  HIP_TRY(wgrad32(W.in16, 16, W.g32, F, m->layers[0]));
  return DSEN2_OK;
}

}  // namespace

namespace dsen2 {

int train_state_after_load(dsen2_model* m) {
  if (m->train->packed16) {
    // the packed planes do not hold the fp32 weights: the master copy is the vector dsen2_model_load_weights was given
    if (m->host_flat.size() != m->n_params) return fail(DSEN2_ERR_INTERNAL, "the loaded weights were not kept");
    HIP_TRY(hipMemcpy(m->train->master, m->host_flat.data(), m->n_params * sizeof(float), hipMemcpyHostToDevice));
    std::vector<float>().swap(m->host_flat);
    if (int rc = repack_x3(m, false, nullptr)) return rc;
    HIP_TRY(hipStreamSynchronize(nullptr));
    return DSEN2_OK;
  }
  if (int rc = refresh_from_packed(m, nullptr)) return rc;
  if (dsen2_model* c = m->train->amp) {       // the companion's packed buffers follow the master copy
    if (int rc = repack_x3(c, true, nullptr)) return rc;
    c->loaded = true;
  }
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
    *bytes = train_ws_bytes(m, n, h, w);
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
    const size_t need = train_ws_bytes(m, n, h, w);
    if (ws_bytes < need) return fail(DSEN2_ERR_WORKSPACE, "workspace %zu < %zu bytes", ws_bytes, need);
    if (int rc = ensure_train_state(m)) return rc;
    if (m->train->packed16) return gradients_x3(m, x10, x20, x60, target, dev_out, grad, loss2, n, h, w, ws, (hipStream_t)stream_);
    if (m->train->amp) return gradients_amp(m, x10, x20, x60, target, dev_out, grad, loss2, n, h, w, ws, (hipStream_t)stream_);
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
    if (t->packed16) {
      std::vector<float>().swap(m->host_flat);
      if (int rc = repack_x3(m, true, s)) return rc;
      m->loaded = true;
      return DSEN2_OK;
    }
    HIP_TRY(launch_gather(m->dev_params, t->master, t->fwd_map, m->dev_param_floats, s));     // predict / evaluate read these
    if (t->amp) {       // the step runs on the companion: its packed buffers and bf16 dgrad weights, not the fp32 dgrad weights
      if (int rc = repack_x3(t->amp, true, s)) return rc;
      t->amp->loaded = true;
    } else {
      HIP_TRY(launch_gather(t->dg, t->master, t->dg_map, t->dg_floats, s));
    }
    m->loaded = true;
    return DSEN2_OK;
  });
}

int dsen2_model_set_train_precision(dsen2_model* m, int precision) {
  return guarded([&]() -> int {
    if (!m) return fail(DSEN2_ERR_INVALID, "NULL model");
    if (m->precision != 0)
      return fail(DSEN2_ERR_INVALID, "the train precision is an option of an fp32 model (this one has precision %d)", m->precision);
    if (precision != 0 && precision != 1)
      return fail(DSEN2_ERR_INVALID, "train precision %d unknown (0 = the model's own arithmetic, 1 = bf16 operands)", precision);
    if (precision == m->train_precision) return DSEN2_OK;
    const bool had_state = m->train != nullptr;
    if (had_state) {      // drop it (nothing may still be running on its buffers) and build the other one: the master copy is
                          // restored from the packed fp32 weights, which hold every value exactly
      if (int rc = check_device(m)) return rc;
      HIP_TRY(hipDeviceSynchronize());
      train_state_destroy(m->train);
      m->train = nullptr;
    }
    m->train_precision = precision;
    return had_state ? ensure_train_state(m) : DSEN2_OK;
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

int dsen2_nadam_step_shards(float* p, const float* dev_g_shards, size_t shard_stride, int shards, const int* host_counts,
                            float* dev_g_mean, float* m, float* v, size_t count, float lr, float b1, float b2, float eps, float mc_t,
                            float mc_t1, float ms_new, float ms_next, float b2_pow_t, void* stream) {
  return guarded([&]() -> int {
    if (!host_counts || (count > 0 && (!p || !dev_g_shards || !m || !v))) return fail(DSEN2_ERR_INVALID, "NULL argument");
    if (shards < 1 || shards > kMaxShards) return fail(DSEN2_ERR_INVALID, "shards %d outside 1..%d", shards, kMaxShards);
    if (shard_stride < count) return fail(DSEN2_ERR_INVALID, "shard_stride %zu < count %zu", shard_stride, count);
    ShardCounts counts{};
    long long total = 0;
    for (int r = 0; r < shards; ++r) {
      if (host_counts[r] < 0) return fail(DSEN2_ERR_INVALID, "negative sample count %d of shard %d", host_counts[r], r);
      if (host_counts[r] >= (1 << 24)) return fail(DSEN2_ERR_INVALID, "sample count %d of shard %d is not below 2^24", host_counts[r], r);
      counts.n[r] = host_counts[r];
      total += host_counts[r];
    }
    if (total <= 0) return fail(DSEN2_ERR_INVALID, "the sample counts of the %d shards add up to zero", shards);
    HIP_TRY(launch_nadam_shards(p, dev_g_shards, shard_stride, shards, counts, dev_g_mean, m, v, count, lr, b1, b2, eps, mc_t, mc_t1,
                                ms_new, ms_next, b2_pow_t, (hipStream_t)stream));
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

// dsen2_conv3x3_wgrad_bf16x3 (planes 2) and dsen2_conv3x3_wgrad_bf16 (planes 1): one set of checks
static int conv3x3_wgrad16(int planes, const void* dev_a, const void* dev_g, float* dev_dw, float* dev_db, int n, int h, int w, int feat,
                           float scale, void* stream) {
  return guarded([&]() -> int {
    if (!dev_a || !dev_g || !dev_dw || !dev_db) return fail(DSEN2_ERR_INVALID, "NULL argument");
    if (feat != 128 && feat != 256) return fail(DSEN2_ERR_INVALID, "feat %d unsupported (128 or 256)", feat);
    if (int rc = check_shape(nullptr, n, h, w)) return rc;
    const size_t wf = wgrad16_workspace_floats(n, h, w, feat);
    hipStream_t s = (hipStream_t)stream;
    return launch_once_with_temp(planes == 2 ? "bf16x3 wgrad" : "bf16 wgrad", nullptr, wf * sizeof(float), s, [&](char* dev) {
      return (planes == 2 ? launch_conv3x3_wgrad16 : launch_conv3x3_wgrad16_bf16)(dev_a, dev_g, n, h, w, feat, scale, dev_dw, dev_db,
                                                                                   reinterpret_cast<float*>(dev), wf, s);
    });
  });
}

int dsen2_conv3x3_wgrad_bf16x3(const void* dev_a_planes, const void* dev_g_planes, float* dev_dw, float* dev_db, int n, int h, int w,
                               int feat, float scale, void* stream) {
  return conv3x3_wgrad16(2, dev_a_planes, dev_g_planes, dev_dw, dev_db, n, h, w, feat, scale, stream);
}

int dsen2_conv3x3_wgrad_bf16(const void* dev_a, const void* dev_g, float* dev_dw, float* dev_db, int n, int h, int w, int feat,
                             float scale, void* stream) {
  return conv3x3_wgrad16(1, dev_a, dev_g, dev_dw, dev_db, n, h, w, feat, scale, stream);
}

int dsen2_conv3x3_wgrad_geometry(int kind, int n, int h, int w, int ca, int cg, long long* tiles, int* splits,
                                 size_t* workspace_floats) {
  return guarded([&]() -> int {
    if (!tiles || !splits || !workspace_floats) return fail(DSEN2_ERR_INVALID, "NULL argument");
    if (kind < 0 || kind > 2) return fail(DSEN2_ERR_INVALID, "kind %d unsupported (0 fp32, 1 bf16x3, 2 bf16)", kind);
    if (n <= 0 || h <= 0 || w <= 0) return fail(DSEN2_ERR_INVALID, "bad shape n=%d h=%d w=%d", n, h, w);
    if (kind == 0) {
      if (!wgrad_geometry(n, h, w, ca, cg, tiles, splits)) return fail(DSEN2_ERR_INVALID, "no wgrad kernel for %d -> %d channels", ca, cg);
      *workspace_floats = wgrad_workspace_floats(n, h, w, ca, cg);
    } else {
      if (ca != cg || (cg != 128 && cg != 256)) return fail(DSEN2_ERR_INVALID, "feat %d -> %d unsupported (128 or 256)", ca, cg);
      if (!wgrad16_geometry(n, h, w, cg, tiles, splits)) return fail(DSEN2_ERR_INVALID, "bad shape n=%d h=%d w=%d", n, h, w);
      *workspace_floats = wgrad16_workspace_floats(n, h, w, cg);
    }
    return DSEN2_OK;
  });
}

}  // extern "C"
