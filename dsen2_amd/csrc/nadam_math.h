// keras 2.2 Nadam on one parameter, operation by operation in double: the arithmetic nadam_kernel, nadam_shards_kernel
// (train_ops.hip) and optimizer_step_kernel (optimizer_step.hip) share.  The product is built with -ffp-contract=off, so every
// operator below rounds on its own.  Needs the HIP runtime alone.
#pragma once
#include <hip/hip_runtime.h>

namespace dsen2 {

// the per-step scalars, computed on the host in double and passed as floats (include/dsen2_hip.h, dsen2_nadam_step)
struct NadamScalars {
  float lr, b1, b2, eps, mc_t, mc_t1, ms_new, ms_next, b2_pow_t;
};

// nadam_kernel's arithmetic on one parameter, operation by operation, for a gradient already held in double
__device__ __forceinline__ void nadam_one(double gi, float& p, float& m, float& v, const NadamScalars& s) {
  const double gp = gi / (1.0 - (double)s.ms_new);
  const float mt = (float)((double)s.b1 * m + (1.0 - (double)s.b1) * gi);
  const float vt = (float)((double)s.b2 * v + (1.0 - (double)s.b2) * gi * gi);
  const double mp = (double)mt / (1.0 - (double)s.ms_next);
  const double vp = (double)vt / (1.0 - (double)s.b2_pow_t);
  const double mbar = (1.0 - (double)s.mc_t) * gp + (double)s.mc_t1 * mp;
  p = (float)((double)p - (double)s.lr * mbar / (sqrt(vp) + (double)s.eps));
  m = mt;
  v = vt;
}

}  // namespace dsen2
