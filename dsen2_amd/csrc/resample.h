// What imresize.hip's resampling passes and quality_metrics.hip's fused bicubic loader share: the exact widening of a sample and
// one resampled output, the sequential un-fused float64 sum of P products.  Include it below `#pragma clang fp contract(off)`.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace dsen2 {

constexpr int kResizeMaxTaps = 256;

template <typename T> __device__ __forceinline__ double as_double(T v) { return (double)v; }        // exact for all three

// one output: slice = in + a * N * B + b, taps of output o at w[k * M + o] / idx[k * M + o]
template <typename T>
__device__ __forceinline__ double resample_one(const T* __restrict__ column, const double* __restrict__ w, const int* __restrict__ idx,
                                               int P, int M, int N, int B, unsigned o) {
  auto term = [&](int k) {
    int q = idx[(size_t)k * M + o];
    q = q < 0 ? 0 : (q >= N ? N - 1 : q);
    return __dmul_rn(as_double(column[(size_t)q * B]), w[(size_t)k * M + o]);
  };
  double acc = term(0);
#pragma unroll 4
  for (int k = 1; k < P; ++k) acc = __dadd_rn(acc, term(k));
  return acc;
}

}  // namespace dsen2
