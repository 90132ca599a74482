// Host-side declarations shared by the two C-ABI translation units (capi.hip: network object and forward; capi_train.hip:
// the training entries).
#pragma once
#include <exception>
#include <new>
#include <vector>

#include "../../include/dsen2_hip.h"
#include "dsen2_internal.h"

namespace dsen2 {

// sets the thread-local text of dsen2_last_error() and returns `code` (capi.hip)
int capi_fail(int code, const char* fmt, ...);

// Nothing may leave an extern "C" entry point as a C++ exception (std::bad_alloc from a staging vector, std::system_error
// from a mutex): through a C / ctypes caller that is std::terminate -> abort() of the host process.  Every entry point
// that can allocate or lock runs its body through this and reports DSEN2_ERR_* with dsen2_last_error() instead.
template <class F>
int guarded(F&& body) noexcept {
  try {
    return body();
  } catch (const std::bad_alloc&) {
    return capi_fail(DSEN2_ERR_NOMEM, "out of host memory");            // not the caller's arguments: its own code
  } catch (const std::exception& e) {
    return capi_fail(DSEN2_ERR_INTERNAL, "unexpected C++ exception: %s", e.what());
  } catch (...) {
    return capi_fail(DSEN2_ERR_INTERNAL, "unexpected C++ exception");
  }
}

struct Layer {
  int cin, cout;        // real channel counts (keras)
  int epilogue;
  bool bf16;            // weights packed as bf16 for the bf16-operand body kernel (conv3x3_body16w.hip)
  bool x3;              // ... as the (wh, wl, wh) planes of the bf16x3 form (precision 2): 3 x the bf16 weights
  PackGeom geom;
  size_t w_off, b_off;  // float offsets inside dev_params
  size_t w16_off;       // first layer of a precision-1 / -2 model: its bf16 (wh | wl) form for conv3x3_first16.hip; 0 = none
  size_t flat_off;      // float offset of the kernel inside the keras-flat array
};

constexpr size_t kAlignFloats = 64;   // 256-byte alignment of every device sub-buffer
inline size_t align_up(size_t v) { return (v + kAlignFloats - 1) / kAlignFloats * kAlignFloats; }

// Training state of an fp32 model (capi_train.hip), created by the first training call: the master weights as a device
// keras-flat vector and the gather maps that rebuild every packed buffer from it.
struct TrainState;
void train_state_destroy(TrainState* t);
// after dsen2_model_load_weights replaced the packed weights: bring the master vector and the dgrad weights up to date
int train_state_after_load(dsen2_model* m);

}  // namespace dsen2

struct dsen2_model {
  int c10, c20, c60, cin, cout, num_layers, feat, precision;
  int device;
  dsen2::Tuning tune;   // kernel structures, fixed at creation
  std::vector<dsen2::Layer> layers;
  size_t n_params;
  size_t chain_stride;  // precision 1 / 2: bytes between the packed weights (= between the biases) of consecutive body layers; 0 = not uniform
  size_t dev_param_floats;
  float* dev_params;
  bool loaded;
  dsen2::TrainState* train;   // NULL until the first training call
};
