// The pieces of every float64 sum whose order the element count alone fixes (no atomics, the same bits on every
// run, and a restatement in numpy gives them too — tests/fixed_sum_restatement.py): the tree over a workgroup's 256 threads, the
// strided sum over the workgroups' partials, the one-block finish kernel made of those two, and the wave-then-four-waves sum of
// the tiled metrics.  Every addition is a __dadd_rn under `fp contract(off)` of its own, whatever the includer's state.
// Needs the HIP runtime alone.
#pragma once
#include <hip/hip_runtime.h>

namespace dsen2 {

constexpr int kQThreads = 256;                     // threads of every workgroup that sums
constexpr int kQWaves = kQThreads / 64;
constexpr int kQMaxBands = 64;
constexpr int kQMaxBlocks = 4096;                  // partial pairs per band: the workspace is kQMaxBlocks * C * 2 doubles

static size_t sum_work_bytes(int C) { return (size_t)kQMaxBlocks * C * 2 * sizeof(double); }

// v[k] = the sum over the workgroup's kQThreads threads of their v[k], k = 0 .. N - 1, each on its own: LDS [N][256], a barrier,
// then tid += tid + half for half = 128 .. 1.  Valid in thread 0 alone.  Every thread of the workgroup must call it.  It may be
// called again without a barrier in between: after the last barrier thread 0 reads only its own slots.
template <int N>
__device__ __forceinline__ void block_tree(double (&v)[N]) {
#pragma clang fp contract(off)
  __shared__ double s[N][kQThreads];
  const int tid = threadIdx.x;
#pragma unroll
  for (int k = 0; k < N; ++k) s[k][tid] = v[k];
  __syncthreads();
  for (int half = kQThreads / 2; half > 0; half >>= 1) {
    if (tid < half) {
#pragma unroll
      for (int k = 0; k < N; ++k) s[k][tid] = __dadd_rn(s[k][tid], s[k][tid + half]);
    }
    __syncthreads();
  }
  if (tid == 0) {
#pragma unroll
    for (int k = 0; k < N; ++k) v[k] = s[k][0];
  }
}

// v[k] = 0.0 + partials[blk * stride + k] for blk = tid, tid + 256, ... below `blocks`, in that order: what a thread of a
// one-block kernel brings to block_tree
template <int N>
__device__ __forceinline__ void strided_partials(const double* __restrict__ partials, int blocks, size_t stride, double (&v)[N]) {
#pragma clang fp contract(off)
#pragma unroll
  for (int k = 0; k < N; ++k) v[k] = 0.0;
  for (int blk = threadIdx.x; blk < blocks; blk += kQThreads) {
#pragma unroll
    for (int k = 0; k < N; ++k) v[k] = __dadd_rn(v[k], partials[(size_t)blk * stride + k]);
  }
}

// one block: out[c * out_stride + 0 .. 1] = the sums over all blocks of partials[block][c][0 .. 1]; out_stride 3 (dsen2_band_errors)
// also stores `third` at out[c * 3 + 2]
static __global__ __launch_bounds__(kQThreads) void fixed_sum_finish_kernel(const double* __restrict__ partials, int blocks, int C,
                                                                            int out_stride, double third, double* __restrict__ out) {
  for (int c = 0; c < C; ++c) {
    double v[2];
    strided_partials<2>(partials + c * 2, blocks, (size_t)C * 2, v);
    block_tree<2>(v);
    if (threadIdx.x == 0) {
      out[c * out_stride + 0] = v[0];
      out[c * out_stride + 1] = v[1];
      if (out_stride == 3) out[c * 3 + 2] = third;
    }
  }
}

static hipError_t launch_finish(const double* partials, int blocks, int C, int out_stride, double third, double* out, hipStream_t stream) {
  hipLaunchKernelGGL(fixed_sum_finish_kernel, dim3(1), dim3(kQThreads), 0, stream, partials, blocks, C, out_stride, third, out);
  return hipGetLastError();
}

// The sum of the workgroup's 256 values of v: a fixed shuffle tree per wave, then (w0 + w1) + (w2 + w3).  Valid in thread 0 alone.
// It holds one barrier; another one must lie between two calls (the tiled metrics have two per band).
__device__ __forceinline__ double wave_then_block_sum(double v) {
#pragma clang fp contract(off)
  __shared__ double s_wave[kQWaves];
  const int tid = threadIdx.x;
  for (int off = 32; off > 0; off >>= 1) v = __dadd_rn(v, __shfl_down(v, off));
  if ((tid & 63) == 0) s_wave[tid >> 6] = v;
  __syncthreads();
  return tid == 0 ? __dadd_rn(__dadd_rn(s_wave[0], s_wave[1]), __dadd_rn(s_wave[2], s_wave[3])) : 0.0;
}

}  // namespace dsen2
