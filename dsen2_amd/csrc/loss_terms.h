// The loss table of dsen2_internal.h ("losses"), shared by the training step's loss kernel (train_ops.hip) and the validation
// sums (error_sums.hip): rho(d) and rho'(d) of one error d in double, every operation rounded on its own — __dmul_rn /
// __dadd_rn, never an FMA; double sqrt and divide are correctly rounded.  sign(0) = 0.  p = (double) of the float32 parameter
// that crossed the ABI (Huber's delta, Charbonnier's epsilon).
//
//   kind          rho                                   rho'
//   MAE           |d|                                   sign(d)
//   MSE           d*d                                   2*d
//   Huber         |d| <= p: 0.5*(d*d)                   d
//                 else:     p*(|d| - 0.5*p)             p*sign(d)
//   Charbonnier   s = sqrt(d*d + p*p)                   d / s
#pragma once
#include <type_traits>

#include "dsen2_internal.h"

namespace dsen2 {

template <int KIND>
__device__ __forceinline__ void loss_terms(double d, double p, double& rho, double& slope) {
  const double a = fabs(d);
  const double sgn = d > 0.0 ? 1.0 : (d < 0.0 ? -1.0 : 0.0);
  if (KIND == kLossMae) {
    rho = a;
    slope = sgn;
  } else if (KIND == kLossMse) {
    rho = __dmul_rn(d, d);
    slope = __dmul_rn(2.0, d);
  } else if (KIND == kLossHuber) {
    if (a <= p) {
      rho = __dmul_rn(0.5, __dmul_rn(d, d));
      slope = d;
    } else {
      rho = __dmul_rn(p, __dadd_rn(a, -__dmul_rn(0.5, p)));
      slope = __dmul_rn(p, sgn);
    }
  } else {
    rho = sqrt(__dadd_rn(__dmul_rn(d, d), __dmul_rn(p, p)));
    slope = d / rho;
  }
}

// f(kind, mask) with the two as compile-time constants (std::integral_constant / std::bool_constant; decltype(kind)::value
// names a template argument): the one place that turns the pair of a checked call (check_loss, launch_loss_grad) into kernels
template <class F>
void with_loss(int kind, int mask, F&& f) {
  using std::integral_constant;
  switch (kind * kMaskModes + mask) {
    case kLossMae * kMaskModes + kMaskNone: f(integral_constant<int, kLossMae>{}, std::false_type{}); break;
    case kLossMae * kMaskModes + kMaskNoData: f(integral_constant<int, kLossMae>{}, std::true_type{}); break;
    case kLossMse * kMaskModes + kMaskNone: f(integral_constant<int, kLossMse>{}, std::false_type{}); break;
    case kLossMse * kMaskModes + kMaskNoData: f(integral_constant<int, kLossMse>{}, std::true_type{}); break;
    case kLossHuber * kMaskModes + kMaskNone: f(integral_constant<int, kLossHuber>{}, std::false_type{}); break;
    case kLossHuber * kMaskModes + kMaskNoData: f(integral_constant<int, kLossHuber>{}, std::true_type{}); break;
    case kLossCharbonnier * kMaskModes + kMaskNone: f(integral_constant<int, kLossCharbonnier>{}, std::false_type{}); break;
    default: f(integral_constant<int, kLossCharbonnier>{}, std::true_type{}); break;
  }
}

}  // namespace dsen2
