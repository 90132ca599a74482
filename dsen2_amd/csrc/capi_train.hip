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
// One walk (gradients) serves every model.  A StepFormat says which plan it runs on and how many bf16 planes a 16-bit tensor
// of the step has.  In every format the forward is forward_launches with every t_l and x_l kept, and the loss, the output and
// the first convolution's gradients run on the fp32 kernels on fp32 tensors; the formats differ in the residual blocks:
//   planes 0  (an fp32 model; any model without residual blocks): fp32 tensors and the kernels above; g is updated in place,
//             du is zeroed for every block.
//   planes 2  (a bf16x3 model): the forward's bf16x3 per-layer kernels.  g lives as a precision-2 residual stream (s0 = hx: hi | xl
//             planes, the dgrads' operand; s1 = lo16), reached through launch_split3_f32 / launch_join3_f32, so g + dgradA(du) is
//             the body kernel's in-place residual epilogue and 0.1 * dgradB(g) its fp32 epilogue over a zero stream it never
//             writes, followed by launch_mask_split3 (ReLU mask of t_l, du as a two-plane operand tensor); the block weight
//             gradients are conv3x3_wgrad16.hip.  A 16-bit operand tensor (s0, t_l, the kept copies of s0, du) has the size of
//             an fp32 tensor.
//   planes 1  (mixed precision: dsen2_model_set_train_precision(m, 1) on an fp32 model with residual blocks): the same on
//             one-plane tensors of half that size, on the model's COMPANION plan.  g is a precision-1 residual stream (hi, lo) =
//             exact fp32 (launch_split_f32 / launch_join_f32), hi = (u + 0x8000) >> 16 the dgrads' and conv-B wgrad's operand;
//             t_l is bf16 (RNE), du = bf16_rne of the masked value (launch_mask_round16); the block weight gradients are the
//             one-plane instance of conv3x3_wgrad16.hip (db = the sum of the bf16 operand g).
//
// The weights of a model being trained live as a device keras-flat fp32 vector (the master copy).  Every packed buffer — the
// forward's and the dgrad weights — is rebuilt from it (repack_from_master) by gather kernels whose index maps are made once,
// by running the host packers on index-valued kernels: the repacked weights are the host packers' bits by construction.
// fp32 buffers have one map entry per float (launch_gather; the packers run on 1 + index, 0 = padding).  The buffers of a
// 16-bit plan hold bf16 (hi, lo) planes next to fp32 words, so their maps have one entry per 16-bit half (launch_gather16) and
// are read off the host packers digit by digit: an index does not survive a bf16 split, but a base-128 digit d packed as the
// value d + 1 does (exact in bf16: it lands in the hi plane, the lo plane gets 0), and packed as 1 + (d + 1) * 2^-16 it lands
// in the lo plane (hi = 1).  Three passes of each kind give every half its flat index and its kind.  The body layers share
// one plan and so one map.
//
// The companion of a mixed-precision model is owned by its training state: a precision-1 plan of the same network with the
// packed buffers a precision-1 model of these weights would hold (first16 image, bf16 body planes, fp32 output layer) and its
// own 16-bit training state (the bf16 flipped / transposed dgrad weights) on the owner's master vector.  The model, its master
// weights and its packed fp32 buffers stay as they are; it builds no fp32 dgrad weights.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <memory>
#include <stdexcept>

#include "capi_internal.h"
#include "optimizer_step.h"

using namespace dsen2;

namespace dsen2 {

struct TrainState {
  float* master = nullptr;     // [n_params] keras-flat
  bool owns_master = true;     // (a companion borrows its owner's)
  float* dg = nullptr;         // flipped / transposed packed weights of every layer with an input gradient, + zero bias
  size_t dg_floats = 0;
  std::vector<size_t> dg_off;  // per layer: float offset of its dgrad weights in dg (layer 0: none)
  size_t dg_body_stride = 0;   // floats between the dgrad weights of consecutive body layers
  size_t zero_off = 0;         // feat zeros (the dgrad convolutions' bias)
  ConvPlan body_plan{}, out_plan{};   // the dgrad convolutions of a body layer (F -> F) and of the output layer (16 -> F)
  // fp32 buffers: launch_gather / launch_scatter maps, 1 + flat index of every packed value, 0 = padding
  int* fwd_map = nullptr;      // [dev_param_floats]
  int* dg_map = nullptr;       // [dg_floats]
  // a 16-bit plan (packed16): launch_gather16 maps of the first layer's, a body layer's and the output layer's forward buffer
  // and of a body layer's and the output layer's dgrad weights
  int* map16[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  dsen2_model* amp = nullptr;  // mixed precision: the companion plan (owned)
};
enum { kMapFirst = 0, kMapBody = 1, kMapOut = 2, kMapDgBody = 3, kMapDgOut = 4 };

void train_state_destroy(TrainState* t) {
  if (!t) return;
  dsen2_model_destroy(t->amp);
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

// How a model trains: `plan` is the model whose packed buffers and dgrad weights the step runs on (m itself, or its companion
// once the training state exists); `planes` is dsen2_model::train_planes().  A companion has the network, feature size and
// tuning of its owner, so a workspace may be sized from either.
struct StepFormat {
  const dsen2_model* plan;
  int planes;
};
bool has_companion(const dsen2_model* m) { return m->precision == 0 && m->train_planes() == 1; }
// m's own packed buffers are a 16-bit plan's (a bf16x3 model, a companion): 16-bit-granular maps, the master copy not
// recoverable from them
bool packed16(const dsen2_model* m) { return m->precision != 0 && m->train_planes() != 0; }
StepFormat step_format(const dsen2_model* m) { return {has_companion(m) && m->train ? m->train->amp : m, m->train_planes()}; }

int check_train_model(const dsen2_model* m) {
  if (!m) return fail(DSEN2_ERR_INVALID, "NULL model");
  if (m->precision == 1) return fail(DSEN2_ERR_INVALID, "training needs an fp32 model or a bf16x3 one (precision 0 or 2), not bf16 operands");
  return check_device(m);
}

// What the packers are run on, as indices into a layer's keras-flat values (-1 = a zero).  A layer's own buffer: the kernel,
// then the bias, as they lie there.
std::vector<int> layer_values(const Layer& Ly) {
  std::vector<int> v((size_t)9 * Ly.plan.cin * Ly.plan.cout + Ly.plan.cout);
  for (size_t i = 0; i < v.size(); ++i) v[i] = (int)i;
  return v;
}
// The kernel of the dgrad convolution g of a layer ci -> co: W'[tap][c'][o'] = W[8 - tap][o'][c'] (the output layer: 16 -> F,
// the outputs zero-padded to 16 input channels)
std::vector<int> flipped_values(const ConvPlan& g, int ci, int co) {
  std::vector<int> v((size_t)9 * g.cin * g.cout, -1);
  for (int tap = 0; tap < 9; ++tap)
    for (int c = 0; c < co; ++c)
      for (int o = 0; o < ci; ++o) v[((size_t)tap * g.cin + c) * g.cout + o] = (int)(((size_t)(8 - tap) * ci + o) * co + c);
  return v;
}

// the float-granular map (launch_gather / launch_scatter) of a layer buffer whose values start at flat_off
void build_gather_map(const ConvPlan& pl, bool with_bias, const std::vector<int>& src, size_t flat_off, int* map) {
  std::vector<float> k(src.size()), buf(with_bias ? pl.floats : pl.weight_floats);
  for (size_t e = 0; e < src.size(); ++e) k[e] = (float)(src[e] + 1);
  pack(pl, k.data(), with_bias ? k.data() + (size_t)9 * pl.cin * pl.cout : nullptr, buf.data());
  for (size_t i = 0; i < buf.size(); ++i) map[i] = buf[i] > 0.f ? (int)(flat_off + (size_t)buf[i]) : 0;
}

// The 16-bit-granular map (launch_gather16) of a layer buffer, relative to the layer's values; see the file comment.
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
  const bool body16 = pl.kernel == ConvKernel::Body16 || pl.kernel == ConvKernel::Body16x3;
  std::vector<int> map(2 * words, 0);
  for (size_t i = 0; i < words; ++i) {
    const bool is16 = (body16 && i < pl.weight_floats) || (pl.first16_planes && i >= pl.first16_off);
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

int upload_map(const std::vector<int>& map, int** dev) {
  HIP_TRY(hipMalloc((void**)dev, map.size() * sizeof(int)));
  HIP_TRY(hipMemcpy(*dev, map.data(), map.size() * sizeof(int), hipMemcpyHostToDevice));
  return DSEN2_OK;
}

int ensure_train_state(dsen2_model* m, float* borrowed_master = nullptr);

// the precision-1 companion of a mixed-precision step: the same network planned with bf16 operands, its packed buffers allocated
// (filled by repack_from_master) and its training state on the owner's master vector
int create_amp_companion(const dsen2_model* m, float* master, dsen2_model** out) {
  std::unique_ptr<dsen2_model, void (*)(dsen2_model*)> guard(new dsen2_model(), dsen2_model_destroy);
  dsen2_model* c = guard.get();
  c->c10 = m->c10; c->c20 = m->c20; c->c60 = m->c60; c->cin = m->cin; c->cout = m->cout;
  c->num_layers = m->num_layers; c->feat = m->feat; c->precision = 1; c->device = m->device; c->tune = m->tune;
  c->dev_params = nullptr; c->loaded = false; c->train = nullptr;
  if (!plan_network(m->c10, m->c20, m->c60, m->num_layers, m->feat, 1, c->tune, c) || c->n_params != m->n_params)
    return fail(DSEN2_ERR_INVALID, "no bf16 kernel for a layer of this network");
  HIP_TRY(hipMalloc((void**)&c->dev_params, c->dev_param_floats * sizeof(float)));
  if (int rc = ensure_train_state(c, master)) return rc;
  *out = guard.release();
  return DSEN2_OK;
}

// The training state of m: its master vector (borrowed_master: a companion's, which is its owner's), the dgrad weights of its
// plan where the step runs on it, the maps that rebuild its packed buffers, and its companion where it has one.
int ensure_train_state(dsen2_model* m, float* borrowed_master) {
  if (m->train) return DSEN2_OK;
  if (m->n_params >= (size_t)0x7fffffff) return fail(DSEN2_ERR_INVALID, "too many parameters for the gather maps");
  std::unique_ptr<TrainState, void (*)(TrainState*)> guard(new TrainState(), train_state_destroy);
  TrainState* t = guard.get();
  const int F = m->feat;
  const size_t L = m->layers.size();
  // (mixed precision: the step runs on the companion's bf16 dgrad weights; the fp32 ones are neither built nor kept)
  const bool p16 = packed16(m), own_dgrad = !has_companion(m);
  if (!plan_conv(ConvRole::DgradBody, F, F, p16 ? m->precision : 0, m->tune, nullptr, &t->body_plan) ||
      !plan_conv(ConvRole::DgradOutput, 16, F, 0, m->tune, nullptr, &t->out_plan))
    return fail(DSEN2_ERR_INVALID, "no dgrad kernel for feature size %d", F);
  auto dgrad_plan = [&](size_t li) -> const ConvPlan& { return li + 1 == L ? t->out_plan : t->body_plan; };
  if (own_dgrad) {     // dg: the dgrad weights of layers 1 .. L - 1 (layer 0 needs no input gradient), then the zero bias
    t->dg_body_stride = align_up(t->body_plan.weight_floats);
    t->dg_off.assign(L, 0);
    size_t off = 0;
    for (size_t li = 1; li < L; ++li) {
      t->dg_off[li] = off;
      off += align_up(dgrad_plan(li).weight_floats);
    }
    t->zero_off = off;
    t->dg_floats = off + align_up((size_t)F);
  }
  if (p16) {
    const Layer &L0 = m->layers[0], &L1 = m->layers[1], &LO = m->layers[L - 1];
    if (int rc = upload_map(build_gather16_map(L0.plan, true, layer_values(L0)), &t->map16[kMapFirst])) return rc;
    if (int rc = upload_map(build_gather16_map(L1.plan, true, layer_values(L1)), &t->map16[kMapBody])) return rc;
    if (int rc = upload_map(build_gather16_map(LO.plan, true, layer_values(LO)), &t->map16[kMapOut])) return rc;
    if (int rc = upload_map(build_gather16_map(t->body_plan, false, flipped_values(t->body_plan, F, F)), &t->map16[kMapDgBody])) return rc;
    if (int rc = upload_map(build_gather16_map(t->out_plan, false, flipped_values(t->out_plan, LO.plan.cin, LO.plan.cout)), &t->map16[kMapDgOut]))
      return rc;
  } else {
    std::vector<int> fmap(m->dev_param_floats, 0), dmap(t->dg_floats, 0);
    for (const Layer& Ly : m->layers) build_gather_map(Ly.plan, true, layer_values(Ly), Ly.flat_off, &fmap[Ly.off]);
    for (size_t li = 1; own_dgrad && li < L; ++li) {
      const Layer& Ly = m->layers[li];
      build_gather_map(dgrad_plan(li), false, flipped_values(dgrad_plan(li), Ly.plan.cin, Ly.plan.cout), Ly.flat_off, &dmap[t->dg_off[li]]);
    }
    if (int rc = upload_map(fmap, &t->fwd_map)) return rc;
    if (own_dgrad)
      if (int rc = upload_map(dmap, &t->dg_map)) return rc;
  }
  t->owns_master = borrowed_master == nullptr;
  t->master = borrowed_master;
  if (t->owns_master) HIP_TRY(hipMalloc((void**)&t->master, m->n_params * sizeof(float)));
  if (own_dgrad) {
    HIP_TRY(hipMalloc((void**)&t->dg, t->dg_floats * sizeof(float)));
    HIP_TRY(hipMemset(t->dg, 0, t->dg_floats * sizeof(float)));        // the zero bias; the padding between the layers
  }
  if (has_companion(m))
    if (int rc = create_amp_companion(m, t->master, &t->amp)) return rc;
  m->train = guard.release();
  if (t->owns_master && m->loaded) return train_state_after_load(m);
  return DSEN2_OK;
}

// Every packed buffer that depends on the master vector <- master: m's forward buffers (forward_too), its dgrad weights
// where it has them, and all of its companion's
int repack_from_master(dsen2_model* m, bool forward_too, hipStream_t s) {
  TrainState* t = m->train;
  if (packed16(m)) {
    const size_t L = m->layers.size();
    const Layer &L0 = m->layers[0], &L1 = m->layers[1], &LO = m->layers[L - 1];
    const size_t body_values = (size_t)9 * m->feat * m->feat + m->feat;
    if (forward_too) {
      HIP_TRY(launch_gather16(m->dev_params + L0.off, t->master + L0.flat_off, t->map16[kMapFirst], L0.plan.floats, 1, 0, 0, s));
      HIP_TRY(launch_gather16(m->dev_params + L1.off, t->master + L1.flat_off, t->map16[kMapBody], L1.plan.floats, 2 * m->num_layers,
                              L1.plan.floats, body_values, s));
      HIP_TRY(launch_gather16(m->dev_params + LO.off, t->master + LO.flat_off, t->map16[kMapOut], LO.plan.floats, 1, 0, 0, s));
    }
    HIP_TRY(launch_gather16(t->dg + t->dg_off[1], t->master + L1.flat_off, t->map16[kMapDgBody], t->body_plan.weight_floats,
                            2 * m->num_layers, t->dg_body_stride, body_values, s));
    HIP_TRY(launch_gather16(t->dg + t->dg_off[L - 1], t->master + LO.flat_off, t->map16[kMapDgOut], t->out_plan.weight_floats, 1, 0, 0, s));
  } else {
    if (forward_too) HIP_TRY(launch_gather(m->dev_params, t->master, t->fwd_map, m->dev_param_floats, s));     // predict / evaluate read these
    if (t->dg) HIP_TRY(launch_gather(t->dg, t->master, t->dg_map, t->dg_floats, s));
  }
  if (t->amp) {
    if (int rc = repack_from_master(t->amp, true, s)) return rc;
    t->amp->loaded = true;
  }
  return DSEN2_OK;
}

// The training workspace, by role.  char*: a tensor in the step's format (fp32, or a 16-bit operand tensor of `planes` planes).
struct TrainWs {
  float *in16, *out, *gpad, *wg, *loss2;   // NHWC16 packed input; the forward's output and the loss where the caller passes none
  float *x0f, *xd, *g;                     // fp32 x_0, fp32 x_d (the output layer's input), fp32 g
  char *xkeep, *tkeep;                     // x_l at xkeep + l * keep_step floats, t_l at tkeep + (l - 1) * keep_step, as the
  size_t keep_step;                        // forward keeps them (planes 0: x_0 .. x_d, so x0f and xd lie inside; else l < d)
  char* du;
  void *s0, *s1, *gs0, *gs1, *zs0, *zs1;   // planes 1 / 2: the forward's stream, g as a stream, the zero stream
  double *partial, *ssim_work;              // the loss kernel's partial pairs; the SSIM term's partials and sums
  size_t wg_floats;
  size_t bytes;
};

// carve (or, with base == NULL, only size) the training workspace
TrainWs carve(const StepFormat& f, int n, int h, int w, char* base) {
  const dsen2_model* m = f.plan;
  const size_t pix = (size_t)n * h * w, F = m->feat, d = (size_t)m->num_layers;
  const size_t full = align_up(pix * F), half = align_up(pix * F / 2);
  const size_t operand = f.planes == 1 ? half : full;     // a tensor in the step's format: fp32, or one or two bf16 planes
  size_t wg = f.planes ? wgrad16_workspace_floats(n, h, w, m->feat) : wgrad_workspace_floats(n, h, w, m->feat, m->feat);
  for (size_t other : {wgrad_workspace_floats(n, h, w, 16, m->feat), wgrad_workspace_floats(n, h, w, m->feat, 16)})
    if (other > wg) wg = other;
  TrainWs r{};
  size_t off = 0;
  auto take = [&](size_t floats) -> float* {
    float* p = base ? reinterpret_cast<float*>(base) + off : nullptr;
    off += align_up(floats);
    return p;
  };
  auto take16 = [&](size_t floats) { return reinterpret_cast<char*>(take(floats)); };
  r.in16 = take(pix * 16);
  r.keep_step = operand;
  if (f.planes == 0) {       // the forward writes x_0 .. x_d into the kept x
    r.xkeep = take16((d + 1) * full);
    r.x0f = reinterpret_cast<float*>(r.xkeep);
    r.xd = base ? r.x0f + d * full : nullptr;
  } else {                   // the forward keeps copies of s0 for x_0 .. x_{d-1}
    r.xd = take(full);
    r.x0f = take(full);
    r.s0 = take(operand);
    r.s1 = take(half);
    r.xkeep = take16(d * operand);
  }
  r.tkeep = take16(d * operand);
  r.out = take(pix * m->cout);
  r.gpad = take(pix * 16);
  r.g = take(full);
  if (f.planes) {
    r.gs0 = take(operand);
    r.gs1 = take(half);
  }
  r.du = take16(operand);
  if (f.planes) {
    r.zs0 = take(operand);
    r.zs1 = take(half);
  }
  r.wg = take(wg);
  r.wg_floats = wg;
  r.partial = reinterpret_cast<double*>(take(2 * loss_partial_doubles(pix)));
  r.loss2 = take(2);
  r.ssim_work = reinterpret_cast<double*>(take(2 * ssim_loss_work_doubles()));
  r.bytes = off * sizeof(float);
  return r;
}

// dsen2_model_gradients (arguments checked, training state present) in the step format f; see the file comment.  owner: the
// handle the caller holds (f.plan is its companion under mixed precision), whose dsen2_model_set_loss settings the loss follows
int gradients(const StepFormat& f, const dsen2_model* owner, const float* x10, const float* x20, const float* x60, const float* target, float* dev_out, float* grad,
              float* loss2, int n, int h, int w, void* ws, hipStream_t s) {
  const dsen2_model* m = f.plan;
  TrainWs W = carve(f, n, h, w, reinterpret_cast<char*>(ws));
  if (!dev_out) dev_out = W.out;
  if (!loss2) loss2 = W.loss2;
  const TrainState* t = m->train;
  const float* zero = t->dg + t->zero_off;
  const int F = m->feat, d = m->num_layers;
  const size_t pix = (size_t)n * h * w;
  const size_t fbytes = pix * F * sizeof(float);
  auto kept = [&](char* base, int l) { return base + (size_t)l * W.keep_step * sizeof(float); };
  auto kept32 = [&](char* base, int l) { return reinterpret_cast<float*>(kept(base, l)); };
  auto wgrad32 = [&](const float* a, int ca, const float* g, int cg, const Layer& Ly, float scale) -> hipError_t {
    float* dw = grad + Ly.flat_off;
    return launch_conv3x3_wgrad(a, ca, g, cg, n, h, w, Ly.plan.cin, Ly.plan.cout, scale, dw, dw + (size_t)9 * Ly.plan.cin * Ly.plan.cout, W.wg,
                                W.wg_floats, s);
  };
  auto dgrad = [&](const void* in, size_t li, const void* aux, void* out, void* out2, float scale, int epilogue) -> hipError_t {
    ConvParams p = make_params(reinterpret_cast<const float*>(in), t->dg + t->dg_off[li], zero, reinterpret_cast<const float*>(aux),
                               reinterpret_cast<float*>(out), n, h, w, 0, scale);
    p.out2 = out2;
    return launch(li + 1 == m->layers.size() ? t->out_plan : t->body_plan, p, epilogue, m->tune, s);
  };

  // ---- forward, every activation kept: dsen2_model_forward's own launches (forward_launches), so the same bits.  The
  // NHWC16 input is packed here whatever the first convolution reads: the first layer's weight gradient needs it ----
  HIP_TRY(launch_pack_inputs(x10, x20, x60, m->c10, m->c20, m->c60, W.in16, n, h, w, s));
  ForwardWs B;
  B.x0 = W.in16; B.a = f.planes ? W.xd : W.x0f; B.t = kept32(W.tkeep, 0);
  B.s0 = W.s0; B.s1 = W.s1; B.t16 = W.tkeep; B.xkeep = W.xkeep; B.x0f = W.x0f;
  if (int rc = forward_launches(m, x10, x20, x60, dev_out, n, h, w, B, W.keep_step, true, s, nullptr)) return rc;

  // ---- loss, output layer (fp32 kernels) ----
  const bool ssim = owner->loss_ssim.weight > 0.f;
  HIP_TRY(launch_loss_grad(dev_out, target, W.gpad, W.partial, loss2, n, m->cout, h, w, owner->loss_kind, owner->loss_param,
                           owner->loss_mask, s, ssim ? &owner->loss_ssim : nullptr, ssim ? W.ssim_work : nullptr));
  HIP_TRY(wgrad32(W.xd, F, W.gpad, 16, m->layers.back(), 1.f));
  HIP_TRY(hipMemsetAsync(W.g, 0, fbytes, s));
  HIP_TRY(dgrad(W.gpad, m->layers.size() - 1, W.g, W.g, nullptr, 1.f, kEpiResidual));

  // ---- residual blocks, last to first ----
  if (f.planes == 0) {
    for (int l = d; l >= 1; --l) {
      float* du = reinterpret_cast<float*>(W.du);
      HIP_TRY(wgrad32(kept32(W.tkeep, l - 1), F, W.g, F, m->layers[2 * l], 0.1f));
      HIP_TRY(hipMemsetAsync(du, 0, fbytes, s));
      HIP_TRY(dgrad(W.g, 2 * l, du, du, nullptr, 0.1f, kEpiResidual));
      HIP_TRY(launch_relu_mask(du, kept32(W.tkeep, l - 1), pix * F, s));
      HIP_TRY(wgrad32(kept32(W.xkeep, l - 1), F, du, F, m->layers[2 * l - 1], 1.f));
      HIP_TRY(dgrad(du, 2 * l - 1, W.g, W.g, nullptr, 1.f, kEpiResidual));
    }
  } else {
    const bool x3 = f.planes == 2;
    const size_t operand_bytes = x3 ? fbytes : fbytes / 2;
    auto wgrad16 = [&](const void* a, const void* g, const Layer& Ly, float scale) -> hipError_t {
      float* dw = grad + Ly.flat_off;
      return (x3 ? launch_conv3x3_wgrad16 : launch_conv3x3_wgrad16_bf16)(a, g, n, h, w, F, scale, dw, dw + (size_t)9 * F * F, W.wg, W.wg_floats, s);
    };
    // g as a residual stream of the plan's precision; the zero stream 0.1 * dgradB is added to (its fp32 epilogue never writes it)
    HIP_TRY((x3 ? launch_split3_f32 : launch_split_f32)(W.g, W.gs0, W.gs1, n, h, w, F, s));
    HIP_TRY(hipMemsetAsync(W.zs0, 0, operand_bytes, s));
    HIP_TRY(hipMemsetAsync(W.zs1, 0, fbytes / 2, s));
    for (int l = d; l >= 1; --l) {
      const char* t_l = kept(W.tkeep, l - 1);
      HIP_TRY(wgrad16(t_l, W.gs0, m->layers[2 * l], 0.1f));
      HIP_TRY(dgrad(W.gs0, 2 * l, W.zs0, W.g, W.zs1, 0.1f, kEpiResidualF32));
      HIP_TRY((x3 ? launch_mask_split3 : launch_mask_round16)(W.g, t_l, W.du, n, h, w, F, s));
      HIP_TRY(wgrad16(kept(W.xkeep, l - 1), W.du, m->layers[2 * l - 1], 1.f));
      HIP_TRY(dgrad(W.du, 2 * l - 1, W.gs0, W.gs0, W.gs1, 1.f, kEpiResidual));
    }
    HIP_TRY((x3 ? launch_join3_f32 : launch_join_f32)(W.gs0, W.gs1, W.g, n, h, w, F, s));
  }

  // ---- first convolution (fp32 kernels) ----
  HIP_TRY(launch_relu_mask(W.g, W.x0f, pix * F, s));
  HIP_TRY(wgrad32(W.in16, 16, W.g, F, m->layers[0], 1.f));
  return DSEN2_OK;
}

}  // namespace

namespace dsen2 {

int train_state_after_load(dsen2_model* m) {
  TrainState* t = m->train;
  if (packed16(m)) {
    // the packed planes do not hold the fp32 weights: the master copy is the vector dsen2_model_load_weights was given
    if (m->host_flat.size() != m->n_params) return fail(DSEN2_ERR_INTERNAL, "the loaded weights were not kept");
    HIP_TRY(hipMemcpy(t->master, m->host_flat.data(), m->n_params * sizeof(float), hipMemcpyHostToDevice));
    std::vector<float>().swap(m->host_flat);
  } else {
    HIP_TRY(launch_scatter(t->master, m->dev_params, t->fwd_map, m->dev_param_floats, nullptr));     // the inverse gather
  }
  if (int rc = repack_from_master(m, false, nullptr)) return rc;
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
    *bytes = carve(step_format(m), n, h, w, nullptr).bytes;
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
    if (m->loss_ssim.weight > 0.f && (h < m->loss_ssim.win || w < m->loss_ssim.win))
      return fail(DSEN2_ERR_INVALID, "a patch of %d x %d is smaller than the %d x %d window of the SSIM term", h, w, m->loss_ssim.win,
                  m->loss_ssim.win);
    const size_t need = carve(step_format(m), n, h, w, nullptr).bytes;
    if (ws_bytes < need) return fail(DSEN2_ERR_WORKSPACE, "workspace %zu < %zu bytes", ws_bytes, need);
    if (int rc = ensure_train_state(m)) return rc;
    return gradients(step_format(m), m, x10, x20, x60, target, dev_out, grad, loss2, n, h, w, ws, (hipStream_t)stream_);
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
    if (dev_flat != m->train->master)
      HIP_TRY(hipMemcpyAsync(m->train->master, dev_flat, m->n_params * sizeof(float), hipMemcpyDeviceToDevice, s));
    std::vector<float>().swap(m->host_flat);      // (a bf16x3 model's kept load: the master copy has taken its place)
    if (int rc = repack_from_master(m, true, s)) return rc;
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

int dsen2_model_set_loss(dsen2_model* m, int kind, float param, int mask_mode) {
  return guarded([&]() -> int {
    if (int rc = check_train_model(m)) return rc;
    if (int rc = check_loss("model_set_loss", kind, param, mask_mode)) return rc;
    m->loss_kind = kind;
    m->loss_param = loss_reads_param(kind) ? param : 0.f;
    m->loss_mask = mask_mode;
    return DSEN2_OK;
  });
}

int dsen2_model_set_loss_ssim(dsen2_model* m, float weight, const double* host_window, int win, double c1, double c2) {
  return guarded([&]() -> int {
    if (int rc = check_train_model(m)) return rc;
    return check_ssim_loss_term("model_set_loss_ssim", weight, host_window, win, c1, c2, &m->loss_ssim);
  });
}

int dsen2_loss_grad(const float* dev_out, const float* dev_target, int n, int c, int h, int w, int kind, float param, int mask_mode,
                    float* dev_g_nhwc16, float* dev_loss2, void* stream) {
  return guarded([&]() -> int {
    if (!dev_out || !dev_target || !dev_g_nhwc16 || !dev_loss2) return fail(DSEN2_ERR_INVALID, "loss_grad: NULL argument");
    if (n <= 0 || h <= 0 || w <= 0 || c < 1 || c > 15) return fail(DSEN2_ERR_INVALID, "loss_grad: bad shape n=%d c=%d h=%d w=%d (c in 1..15)", n, c, h, w);
    if ((size_t)n * h * w * 16 >= ((size_t)1 << 31)) return fail(DSEN2_ERR_INVALID, "loss_grad: %d x %d x %d pixels exceed one launch", n, h, w);
    if (int rc = check_loss("loss_grad", kind, param, mask_mode)) return rc;
    hipStream_t s = (hipStream_t)stream;
    const size_t doubles = loss_partial_doubles((size_t)n * h * w);
    return launch_once_with_temp("loss_grad", nullptr, doubles * sizeof(double), s, [&](char* dev) {
      return launch_loss_grad(dev_out, dev_target, dev_g_nhwc16, reinterpret_cast<double*>(dev), dev_loss2, n, c, h, w, kind, param, mask_mode, s);
    });
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

// ---- dsen2_optimizer_step: every check before any launch ----
namespace {

// dev_work of dsen2_optimizer_step: { the sum of squares, one double of padding }, the blocks' partials, then (with_mean) the mean
// gradient; every piece starts on a multiple of 16 bytes
struct OptimizerWork {
  size_t partials_off, mean_off, bytes;
};
OptimizerWork optimizer_work(size_t count, bool with_norm, bool with_mean) {
  OptimizerWork w{2 * sizeof(double), 0, 0};
  if (!with_norm) return w;
  w.mean_off = w.partials_off + sqsum_partial_doubles() * sizeof(double);
  w.bytes = w.mean_off + (with_mean ? (count + 3) / 4 * 16 : 0);
  return w;
}
bool needs_norm(const dsen2_optimizer_desc* d, bool want_norm) { return d->clipnorm > 0.f || want_norm; }
// the norm pass leaves the mean gradient somewhere for the step to read: with several rows and no buffer of the caller's, in dev_work
bool mean_in_work(const dsen2_optimizer_desc* d, int shards, bool have_g_mean, bool want_norm) {
  return needs_norm(d, want_norm) && shards > 1 && !have_g_mean;
}
bool bad_option(float x) { return !(x >= 0.f) || !std::isfinite(x); }      // negative, NaN or infinite

int check_optimizer_desc(const dsen2_optimizer_desc* d, size_t count, DecayRanges* ranges) {
  if (!d) return fail(DSEN2_ERR_INVALID, "optimizer_step: NULL descriptor");
  if (d->kind < 0 || d->kind >= kOptKinds) return fail(DSEN2_ERR_INVALID, "optimizer_step: kind %d unknown (0 Nadam, 1 Adam, 2 SGD)", d->kind);
  if (bad_option(d->clipnorm) || bad_option(d->clipvalue) || bad_option(d->weight_decay) || bad_option(d->momentum))
    return fail(DSEN2_ERR_INVALID, "optimizer_step: clipnorm %g, clipvalue %g, weight_decay %g and momentum %g must be finite and >= 0",
                (double)d->clipnorm, (double)d->clipvalue, (double)d->weight_decay, (double)d->momentum);
  if (d->momentum >= 1.f) return fail(DSEN2_ERR_INVALID, "optimizer_step: momentum %g is not below 1", (double)d->momentum);
  if (d->n_ranges < 0 || d->n_ranges > kMaxDecayRanges)
    return fail(DSEN2_ERR_INVALID, "optimizer_step: %d decay ranges outside 0..%d", d->n_ranges, kMaxDecayRanges);
  if (d->n_ranges > 0 && !d->host_ranges) return fail(DSEN2_ERR_INVALID, "optimizer_step: %d decay ranges and a NULL host_ranges", d->n_ranges);
  ranges->n = d->n_ranges;
  size_t behind = 0;
  for (int k = 0; k < d->n_ranges; ++k) {
    const unsigned lo = d->host_ranges[2 * k], hi = d->host_ranges[2 * k + 1];
    if (lo >= hi || (size_t)lo < behind || (size_t)hi > count)
      return fail(DSEN2_ERR_INVALID, "optimizer_step: decay range %d = [%u, %u) is empty, unsorted, overlaps its predecessor or ends behind %zu",
                  k, lo, hi, count);
    ranges->lo[k] = lo;
    ranges->hi[k] = hi;
    behind = hi;
  }
  return DSEN2_OK;
}

}  // namespace

int dsen2_optimizer_step_work_bytes(const dsen2_optimizer_desc* d, size_t count, int shards, int have_g_mean, int want_norm, size_t* bytes) {
  return guarded([&]() -> int {
    if (!bytes) return fail(DSEN2_ERR_INVALID, "optimizer_step_work_bytes: NULL argument");
    DecayRanges ranges{};
    if (int rc = check_optimizer_desc(d, count, &ranges)) return rc;
    if (shards < 1 || shards > kMaxShards) return fail(DSEN2_ERR_INVALID, "shards %d outside 1..%d", shards, kMaxShards);
    *bytes = optimizer_work(count, needs_norm(d, want_norm != 0), mean_in_work(d, shards, have_g_mean != 0, want_norm != 0)).bytes;
    return DSEN2_OK;
  });
}

int dsen2_optimizer_step(const dsen2_optimizer_desc* d, float* p, const float* dev_g_shards, size_t shard_stride, int shards,
                         const int* host_counts, float* dev_g_mean, float* m, float* v, size_t count, void* dev_work, size_t work_bytes,
                         double* dev_norm, void* stream) {
  return guarded([&]() -> int {
    DecayRanges ranges{};
    if (int rc = check_optimizer_desc(d, count, &ranges)) return rc;
    if (!host_counts || (count > 0 && (!p || !dev_g_shards || !m))) return fail(DSEN2_ERR_INVALID, "optimizer_step: NULL argument");
    if (count > 0 && d->kind != kOptSgd && !v) return fail(DSEN2_ERR_INVALID, "optimizer_step: kind %d needs the second-moment vector v", d->kind);
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
    const bool norm = needs_norm(d, dev_norm != nullptr), in_work = mean_in_work(d, shards, dev_g_mean != nullptr, dev_norm != nullptr);
    const OptimizerWork W = optimizer_work(count, norm, in_work);
    if (W.bytes > 0 && (!dev_work || work_bytes < W.bytes || (uintptr_t)dev_work % 16 != 0))
      return fail(DSEN2_ERR_INVALID, "optimizer_step: scratch of %zu bytes at %p, dsen2_optimizer_step_work_bytes asks for %zu on a 16-byte boundary",
                  work_bytes, dev_work, W.bytes);
    OptimizerScalars s{};
    s.kind = d->kind;
    s.nadam = NadamScalars{d->lr, d->b1, d->b2, d->eps, d->mc_t, d->mc_t1, d->ms_new, d->ms_next, d->b2_pow_t};
    s.lr_t = d->lr_t;
    s.momentum = d->momentum;
    s.nesterov = d->nesterov != 0;
    s.clipnorm = d->clipnorm;
    s.clipvalue = d->clipvalue;
    s.weight_decay = d->weight_decay;
    hipStream_t st = (hipStream_t)stream;
    if (!norm) {      // one pass: the mean and the step, as dsen2_nadam_step_shards
      HIP_TRY(launch_optimizer_step(s, p, dev_g_shards, shard_stride, shards, counts, dev_g_mean, m, v, count, nullptr, ranges, st));
      return DSEN2_OK;
    }
    char* const work = static_cast<char*>(dev_work);
    double* const sqsum = reinterpret_cast<double*>(work);
    if (count == 0) {
      HIP_TRY(hipMemsetAsync(sqsum, 0, sizeof(double), st));
      if (dev_norm) HIP_TRY(hipMemsetAsync(dev_norm, 0, sizeof(double), st));
      return DSEN2_OK;
    }
    // two passes: the mean (kept where several rows make one: the caller's buffer, else the scratch) with its sum of squares, then
    // the step on that mean; one row is read twice and never copied (both passes form its mean, (0.0 + c * g) / c, alike)
    float* const mean = dev_g_mean ? dev_g_mean : in_work ? reinterpret_cast<float*>(work + W.mean_off) : nullptr;
    HIP_TRY(launch_grad_mean_sqsum(dev_g_shards, shard_stride, shards, counts, mean, count, reinterpret_cast<double*>(work + W.partials_off),
                                   sqsum, dev_norm, st));
    if (mean)
      HIP_TRY(launch_optimizer_step(s, p, mean, count, 0, counts, nullptr, m, v, count, sqsum, ranges, st));
    else
      HIP_TRY(launch_optimizer_step(s, p, dev_g_shards, shard_stride, shards, counts, nullptr, m, v, count, sqsum, ranges, st));
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
