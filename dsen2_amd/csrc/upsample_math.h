// The arithmetic of ONE output of the mirror-bilinear up-sampler (interp_patches, utils/patches.py:11-16; the derivation is
// written out above upsample_kernel in patch_ops.hip), as device functions: every kernel that up-samples — upsample_kernel,
// upsample_window_kernel (patch_ops.hip) and corpus_batch_kernel (corpus_batch.hip) — calls these and nothing else, so they cannot
// drift apart: the same operations on the same values, the same bits.  Each function switches contraction off for itself; the
// library is built with -ffp-contract=off as well.
#pragma once
#include <hip/hip_runtime.h>

namespace dsen2 {

// neighbours are folded back by mirroring WITHOUT repeating the edge sample (skimage mode='reflect' of warp())
__device__ __forceinline__ int mirror_index(int i, int dim) {
  if (dim == 1) return 0;
  const int cmax = dim - 1;
  if (i < 0) {
    const int k = -i;
    return ((k / cmax) & 1) ? cmax - (k % cmax) : (k % cmax);
  }
  if (i > cmax) return ((i / cmax) & 1) ? cmax - (i % cmax) : (i % cmax);
  return i;
}

// mirror_index for an index at most one image away (-cmax <= i <= 2 * cmax: one reflection, no division, no branch) —
// every tap of an up-sampler's window; images of one or two pixels (several reflections) take the general form.
__device__ __forceinline__ int mirror_index_near(int i, int dim) {
  const int cmax = dim - 1;
  int j = i < 0 ? -i : i;
  j = j > cmax ? 2 * cmax - j : j;
  if (__builtin_expect((unsigned)j > (unsigned)cmax, 0)) j = mirror_index(i, dim);
  return j;
}

// Source coordinate of output index o along one axis: src = scale * o + offset in float32, a multiply and an add rounded
// separately.  *lo / *hi: floor and ceil of it, NOT yet mirrored into the image; returns the float32 fraction src - floor(src).
__device__ __forceinline__ float up_coord(float scale, float offset, int o, int* lo, int* hi) {
#pragma clang fp contract(off)
  const float c = __fadd_rn(__fmul_rn(scale, (float)o), offset);
  const float cf = floorf(c);
  *lo = (int)cf;
  *hi = (int)ceilf(c);
  return __fsub_rn(c, cf);
}

// a source sample as the blends see it: skimage's x / 30000 in float32
__device__ __forceinline__ float up_quotient(float v) { return __fdiv_rn(v, 30000.0f); }

// horizontal blend of the two quotients q0 (left tap) and q1 (right tap) of one source row: the left product in double, the right
// one a float32 multiply (patch_ops.hip: skimage's compiled bilinear_interpolation, operation by operation)
__device__ __forceinline__ double up_hblend(float dcf, float q0, float q1) {
#pragma clang fp contract(off)
  return (1.0 - (double)dcf) * (double)q0 + (double)__fmul_rn(dcf, q1);
}

// vertical blend of the two row blends, back to the data's range, and the folded `/= SCALE` (post_div 1: exact no-op)
__device__ __forceinline__ float up_vblend(float drf, double top, double bot, float post_div) {
#pragma clang fp contract(off)
  const double dr = (double)drf;
  const float v = __fmul_rn((float)((1.0 - dr) * top + dr * bot), 30000.0f);
  return post_div == 1.0f ? v : __fdiv_rn(v, post_div);
}

}  // namespace dsen2
