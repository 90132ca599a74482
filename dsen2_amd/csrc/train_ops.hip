// train_ops.hip — the memory-bound kernels of the training step (capi_train.hip): loss and dL/dout, ReLU-gradient masks,
// the Nadam update and the device weight repack.  Every reduction runs in a fixed order (no float atomics): the same
// inputs give the same bits on every run.
#include "dsen2_internal.h"

namespace dsen2 {

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kLossThreads = 256;
constexpr int kLossMaxBlocks = 1024;

// fixed-shape tree over one block's values (blockDim.x = kLossThreads)
__device__ void block_sum2(double* s, double a, double b, double* out) {
  const int tid = threadIdx.x;
  s[tid] = a;
  s[kLossThreads + tid] = b;
  __syncthreads();
  for (int k = kLossThreads / 2; k > 0; k >>= 1) {
    if (tid < k) {
      s[tid] += s[tid + k];
      s[kLossThreads + tid] += s[kLossThreads + tid + k];
    }
    __syncthreads();
  }
  if (tid == 0) {
    out[0] = s[0];
    out[1] = s[kLossThreads];
  }
}

// e = out - y over NCHW [n][c][hw]; dL/dout = sign(e) * inv_count written as NHWC16 [n*hw][16] (channels >= c zero);
// partial[block] = (sum |e|, sum e^2) of the block's pixels (grid-stride, fixed grid)
__global__ __launch_bounds__(kLossThreads) void mae_loss_grad_kernel(const float* __restrict__ out, const float* __restrict__ y,
                                                                   float* __restrict__ gpad, double* __restrict__ partial,
                                                                   size_t pixels, int hw, int c, float inv_count) {
  __shared__ double s[2 * kLossThreads];
  double sa = 0.0, sq = 0.0;
  for (size_t pix = (size_t)blockIdx.x * kLossThreads + threadIdx.x; pix < pixels; pix += (size_t)gridDim.x * kLossThreads) {
    const size_t img = pix / hw, q = pix % hw;
    float gv[16];
#pragma unroll
    for (int ch = 0; ch < 16; ++ch) {
      gv[ch] = 0.f;
      if (ch < c) {
        const size_t idx = (img * c + ch) * hw + q;
        const float e = out[idx] - y[idx];
        gv[ch] = e > 0.f ? inv_count : (e < 0.f ? -inv_count : 0.f);     // TensorFlow's Abs gradient: sign(0) = 0
        sa += (double)fabsf(e);
        sq += (double)e * (double)e;
      }
    }
    f32x4* dst = reinterpret_cast<f32x4*>(gpad + pix * 16);
#pragma unroll
    for (int k = 0; k < 4; ++k) dst[k] = f32x4{gv[4 * k], gv[4 * k + 1], gv[4 * k + 2], gv[4 * k + 3]};
  }
  block_sum2(s, sa, sq, partial + 2 * (size_t)blockIdx.x);
}

__global__ __launch_bounds__(kLossThreads) void mae_loss_final_kernel(const double* __restrict__ partial, int blocks, double count,
                                                                    float* __restrict__ loss2) {
  __shared__ double s[2 * kLossThreads];
  double sa = 0.0, sq = 0.0;
  for (int i = threadIdx.x; i < blocks; i += kLossThreads) {
    sa += partial[2 * i];
    sq += partial[2 * i + 1];
  }
  __shared__ double tot[2];
  block_sum2(s, sa, sq, tot);
  __syncthreads();
  if (threadIdx.x == 0) {
    loss2[0] = (float)(tot[0] / count);
    loss2[1] = (float)(tot[1] / count);
  }
}

// v = m > 0 ? v : 0, in place (the ReLU gradient through a saved ReLU output m)
__global__ __launch_bounds__(256) void relu_mask_kernel(float* __restrict__ v, const float* __restrict__ m, size_t n4) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n4) return;
  f32x4 a = reinterpret_cast<f32x4*>(v)[i];
  const f32x4 b = reinterpret_cast<const f32x4*>(m)[i];
#pragma unroll
  for (int e = 0; e < 4; ++e) a[e] = b[e] > 0.f ? a[e] : 0.f;
  reinterpret_cast<f32x4*>(v)[i] = a;
}

// keras 2.2 Nadam on one parameter; the per-step scalars come from the host (computed there in double)
__global__ __launch_bounds__(256) void nadam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                  float* __restrict__ v, size_t count, float lr, float b1, float b2, float eps,
                                                  float mc_t, float mc_t1, float ms_new, float ms_next, float b2_pow_t) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  const double gi = g[i];
  const double gp = gi / (1.0 - (double)ms_new);
  const float mt = (float)((double)b1 * m[i] + (1.0 - (double)b1) * gi);
  const float vt = (float)((double)b2 * v[i] + (1.0 - (double)b2) * gi * gi);
  const double mp = (double)mt / (1.0 - (double)ms_next);
  const double vp = (double)vt / (1.0 - (double)b2_pow_t);
  const double mbar = (1.0 - (double)mc_t) * gp + (double)mc_t1 * mp;
  p[i] = (float)((double)p[i] - (double)lr * mbar / (sqrt(vp) + (double)eps));
  m[i] = mt;
  v[i] = vt;
}

// dst[i] = src[map[i] - 1], 0 where map[i] == 0 (padding)
__global__ __launch_bounds__(256) void gather_kernel(float* __restrict__ dst, const float* __restrict__ src, const int* __restrict__ map,
                                                   size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int k = map[i];
  dst[i] = k > 0 ? src[k - 1] : 0.f;
}

// the inverse: flat[map[i] - 1] = packed[i].  Where a flat element appears more than once in the packed buffer every copy
// holds the same value, so the order of the writes does not matter.
__global__ __launch_bounds__(256) void scatter_kernel(float* __restrict__ flat, const float* __restrict__ packed,
                                                    const int* __restrict__ map, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int k = map[i];
  if (k > 0) flat[k - 1] = packed[i];
}

unsigned blocks_for(size_t n, unsigned per) { return (unsigned)((n + per - 1) / per); }

}  // namespace

size_t mae_loss_partial_doubles(size_t pixels) {
  size_t b = (pixels + kLossThreads - 1) / kLossThreads;
  if (b > (size_t)kLossMaxBlocks) b = kLossMaxBlocks;
  if (b < 1) b = 1;
  return 2 * b;
}

hipError_t launch_mae_loss_grad(const float* out, const float* y, float* gpad, double* partial, float* loss2, int n, int c, int h,
                                int w, hipStream_t stream) {
  if (c < 1 || c > 16) return hipErrorInvalidValue;
  const size_t pixels = (size_t)n * h * w;
  const int blocks = (int)(mae_loss_partial_doubles(pixels) / 2);
  const double count = (double)pixels * c;
  hipLaunchKernelGGL(mae_loss_grad_kernel, dim3(blocks), dim3(kLossThreads), 0, stream, out, y, gpad, partial, pixels, h * w, c,
                     (float)(1.0 / count));
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(mae_loss_final_kernel, dim3(1), dim3(kLossThreads), 0, stream, partial, blocks, count, loss2);
  return hipGetLastError();
}

hipError_t launch_relu_mask(float* v, const float* m, size_t count, hipStream_t stream) {
  if (count % 4 != 0) return hipErrorInvalidValue;
  if (count == 0) return hipSuccess;
  hipLaunchKernelGGL(relu_mask_kernel, dim3(blocks_for(count / 4, 256)), dim3(256), 0, stream, v, m, count / 4);
  return hipGetLastError();
}

hipError_t launch_nadam(float* p, const float* g, float* m, float* v, size_t count, float lr, float b1, float b2, float eps,
                        float mc_t, float mc_t1, float ms_new, float ms_next, float b2_pow_t, hipStream_t stream) {
  if (count == 0) return hipSuccess;
  hipLaunchKernelGGL(nadam_kernel, dim3(blocks_for(count, 256)), dim3(256), 0, stream, p, g, m, v, count, lr, b1, b2, eps, mc_t,
                     mc_t1, ms_new, ms_next, b2_pow_t);
  return hipGetLastError();
}

hipError_t launch_gather(float* dst, const float* src, const int* map, size_t n, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(gather_kernel, dim3(blocks_for(n, 256)), dim3(256), 0, stream, dst, src, map, n);
  return hipGetLastError();
}

hipError_t launch_scatter(float* flat, const float* packed, const int* map, size_t n, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(scatter_kernel, dim3(blocks_for(n, 256)), dim3(256), 0, stream, flat, packed, map, n);
  return hipGetLastError();
}

}  // namespace dsen2
