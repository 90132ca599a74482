// optimizer_step.hip — the optimiser step with options (include/dsen2_hip.h, dsen2_optimizer_step): the global norm of the mean
// gradient in a fixed order, and one kernel template for keras 2.2 Nadam, Adam and SGD with gradient clipping (by global norm, by
// value) and decoupled weight decay.  Every operation on a parameter is done in double and rounded on its own: the file is
// compiled with contraction off and says so again below, so no v_fma_f64 joins two of them; double sqrt and divide are correctly
// rounded.  No atomics: the same inputs give the same bits on every run and on every rank of a data-parallel group.
#include "optimizer_step.h"
#include "fixed_sum.h"

#pragma clang fp contract(off)

namespace dsen2 {

namespace {

constexpr int kSqsumPerThread = 8;             // elements per thread the grid aims at (error_sums.hip's rule)
constexpr int kStepWide = 4;                   // floats per access of optimizer_step_kernel's wide form
constexpr size_t kStepMaxBlocks = (size_t)1 << 30;

// nadam_shards_kernel's mean of element i: rows in order, a row whose count is 0 never read
__device__ __forceinline__ float mean_of_rows(const float* __restrict__ g, size_t stride, int shards, const ShardCounts& counts, double total,
                                              size_t i) {
  double acc = 0.0;
  for (int r = 0; r < shards; ++r) {
    const int c = counts.n[r];
    if (c > 0) acc = acc + (double)c * (double)g[(size_t)r * stride + i];
  }
  return (float)(acc / total);
}

// partials[block] = the sum of (double)g * (double)g over the block's elements of the mean gradient g, which is written to g_mean
// where that is given.  loss_sums_kernel's order: the grid is a function of count alone (sqsum_blocks), a thread adds its elements
// i = block * 256 + thread, + blocks * 256, ... in index order, block_tree adds the 256 threads.  Consecutive threads read
// consecutive floats of every row: a wave's access is 256 contiguous bytes.
__global__ __launch_bounds__(kQThreads) void grad_mean_sqsum_kernel(const float* __restrict__ g, size_t stride, int shards, ShardCounts counts,
                                                                    double total, float* __restrict__ g_mean, size_t count,
                                                                    double* __restrict__ partials) {
  const size_t step = (size_t)gridDim.x * kQThreads;
  double v[1] = {0.0};
  for (size_t i = (size_t)blockIdx.x * kQThreads + threadIdx.x; i < count; i += step) {
    const float gm = mean_of_rows(g, stride, shards, counts, total, i);
    if (g_mean) g_mean[i] = gm;
    v[0] = __dadd_rn(v[0], __dmul_rn((double)gm, (double)gm));
  }
  block_tree<1>(v);
  if (threadIdx.x == 0) partials[blockIdx.x] = v[0];
}

// one block: *sqsum = the sum of the blocks' partials (strided_partials, block_tree), *norm (or NULL) = sqrt(*sqsum)
__global__ __launch_bounds__(kQThreads) void sqsum_finish_kernel(const double* __restrict__ partials, int blocks, double* __restrict__ sqsum,
                                                                 double* __restrict__ norm) {
  double v[1];
  strided_partials<1>(partials, blocks, 1, v);
  block_tree<1>(v);
  if (threadIdx.x == 0) {
    *sqsum = v[0];
    if (norm) *norm = sqrt(v[0]);
  }
}

// The update of one parameter from its mean gradient gm.  CLIP & 1: g = (float)((double)g * scale), scale = c / n where the global
// norm n >= c, else 1.0 (keras 2.2 get_gradients / clip_norm).  CLIP & 2: g clamped to [-cv, cv] (a NaN passes: both comparisons
// are false).  Then the step of kind OPT; then, where DECAY and `decayed`, p = (float)((double)p - lr * wd * p_old).
template <int OPT, int CLIP, bool DECAY>
__device__ __forceinline__ void step_one(float gm, float& p, float& m, float& v, const OptimizerScalars& s, double scale, bool decayed) {
  float g = gm;
  if (CLIP & 1) g = (float)((double)g * scale);
  if (CLIP & 2) {
    const float cv = s.clipvalue;
    g = g < -cv ? -cv : (g > cv ? cv : g);
  }
  const float p_old = p;
  const double gi = (double)g, lr = (double)s.nadam.lr;
  if (OPT == kOptNadam) {
    nadam_one(gi, p, m, v, s.nadam);
  } else if (OPT == kOptAdam) {
    const double b1 = (double)s.nadam.b1, b2 = (double)s.nadam.b2;
    const float mt = (float)(b1 * (double)m + (1.0 - b1) * gi);
    const float vt = (float)(b2 * (double)v + (1.0 - b2) * gi * gi);
    p = (float)((double)p - (double)s.lr_t * (double)mt / (sqrt((double)vt) + (double)s.nadam.eps));
    m = mt;
    v = vt;
  } else {
    const double mu = (double)s.momentum;
    const float vel = (float)(mu * (double)m - lr * gi);
    p = s.nesterov ? (float)((double)p + mu * (double)vel - lr * gi) : (float)((double)p + (double)vel);
    m = vel;
  }
  if (DECAY && decayed) p = (float)((double)p - lr * (double)s.weight_decay * (double)p_old);
}

// the first range whose end lies behind element e (n: none), by bisection of the sorted ends in LDS
__device__ __forceinline__ int first_range_behind(const unsigned* s_hi, int n, size_t e) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if ((size_t)s_hi[mid] > e) hi = mid; else lo = mid + 1;
  }
  return lo;
}

// One template for every kind and option, as loss_grad_kernel<KIND, MASK> is for the losses.  W floats per access (W = 4: 16 bytes)
// on elements [0, W * units), the last count % W elements by the first threads of block 0; W = 1: one element per unit, for
// pointers or a stride off the 16-byte grid: the same bits.  One unit per thread, as nadam_shards_kernel (a grid capped at 2048
// blocks ran 10 % slower there); the loop's stride is a guard.  shards == 0: g is the mean already.  SGD (OPT 2) neither reads nor
// writes v.  DECAY: the block copies the ranges into LDS once; a thread bisects for its first element and walks on from there.
template <int OPT, int CLIP, bool DECAY, int W>
__global__ __launch_bounds__(256) void optimizer_step_kernel(float* __restrict__ p, const float* __restrict__ g, size_t stride, int shards,
                                                           ShardCounts counts, double total, float* __restrict__ g_mean,
                                                           float* __restrict__ m, float* __restrict__ v, size_t count, OptimizerScalars s,
                                                           const double* __restrict__ sqsum, DecayRanges ranges) {
  typedef float vec __attribute__((ext_vector_type(W)));
  __shared__ unsigned s_lo[DECAY ? kMaxDecayRanges : 1], s_hi[DECAY ? kMaxDecayRanges : 1];
  const int nr = DECAY ? ranges.n : 0;
  if (DECAY) {
    if ((int)threadIdx.x < nr) {
      s_lo[threadIdx.x] = ranges.lo[threadIdx.x];
      s_hi[threadIdx.x] = ranges.hi[threadIdx.x];
    }
    __syncthreads();
  }
  double scale = 1.0;
  if (CLIP & 1) {
    const double n = sqrt(*sqsum), c = (double)s.clipnorm;
    scale = n >= c ? c / n : 1.0;
  }
  const size_t units = count / W;
  for (size_t u = (size_t)blockIdx.x * blockDim.x + threadIdx.x; u < units; u += (size_t)gridDim.x * blockDim.x) {
    vec gm;
    if (shards == 0) {
      gm = reinterpret_cast<const vec*>(g)[u];
    } else {
      double acc[W];
#pragma unroll
      for (int e = 0; e < W; ++e) acc[e] = 0.0;
      for (int r = 0; r < shards; ++r) {
        const int c = counts.n[r];
        if (c <= 0) continue;
        const vec a = reinterpret_cast<const vec*>(g + (size_t)r * stride)[u];
#pragma unroll
        for (int e = 0; e < W; ++e) acc[e] = acc[e] + (double)c * (double)a[e];
      }
#pragma unroll
      for (int e = 0; e < W; ++e) gm[e] = (float)(acc[e] / total);
    }
    vec pv = reinterpret_cast<vec*>(p)[u], mv = reinterpret_cast<vec*>(m)[u], vv;
    if (OPT != kOptSgd) vv = reinterpret_cast<vec*>(v)[u];
    int at = DECAY ? first_range_behind(s_hi, nr, u * W) : 0;
#pragma unroll
    for (int e = 0; e < W; ++e) {
      bool decayed = false;
      if (DECAY) {
        const size_t i = u * W + e;
        while (at < nr && (size_t)s_hi[at] <= i) ++at;
        decayed = at < nr && (size_t)s_lo[at] <= i;
      }
      float pe = pv[e], me = mv[e], ve = OPT != kOptSgd ? vv[e] : 0.f;
      step_one<OPT, CLIP, DECAY>(gm[e], pe, me, ve, s, scale, decayed);
      pv[e] = pe; mv[e] = me;
      if (OPT != kOptSgd) vv[e] = ve;
    }
    if (g_mean) reinterpret_cast<vec*>(g_mean)[u] = gm;
    reinterpret_cast<vec*>(p)[u] = pv;
    reinterpret_cast<vec*>(m)[u] = mv;
    if (OPT != kOptSgd) reinterpret_cast<vec*>(v)[u] = vv;
  }
  if (W > 1 && blockIdx.x == 0 && units * W + threadIdx.x < count) {
    const size_t i = units * W + threadIdx.x;
    const float gm = shards == 0 ? g[i] : mean_of_rows(g, stride, shards, counts, total, i);
    if (g_mean) g_mean[i] = gm;
    bool decayed = false;
    if (DECAY) {
      const int at = first_range_behind(s_hi, nr, i);
      decayed = at < nr && (size_t)s_lo[at] <= i;
    }
    float ve = OPT != kOptSgd ? v[i] : 0.f;
    step_one<OPT, CLIP, DECAY>(gm, p[i], m[i], ve, s, scale, decayed);
    if (OPT != kOptSgd) v[i] = ve;
  }
}

template <int OPT, int CLIP, bool DECAY>
void launch_step_as(bool wide, unsigned blocks, hipStream_t stream, float* p, const float* g, size_t stride, int shards,
                    const ShardCounts& counts, double total, float* g_mean, float* m, float* v, size_t count, const OptimizerScalars& s,
                    const double* sqsum, const DecayRanges& ranges) {
  if (wide)
    hipLaunchKernelGGL((optimizer_step_kernel<OPT, CLIP, DECAY, kStepWide>), dim3(blocks), dim3(256), 0, stream, p, g, stride, shards, counts,
                       total, g_mean, m, v, count, s, sqsum, ranges);
  else
    hipLaunchKernelGGL((optimizer_step_kernel<OPT, CLIP, DECAY, 1>), dim3(blocks), dim3(256), 0, stream, p, g, stride, shards, counts, total,
                       g_mean, m, v, count, s, sqsum, ranges);
}

template <int OPT, int CLIP, typename... A>
void with_decay(bool decay, A&&... a) {
  if (decay) launch_step_as<OPT, CLIP, true>(a...); else launch_step_as<OPT, CLIP, false>(a...);
}
template <int OPT, typename... A>
void with_clip(int clip, bool decay, A&&... a) {
  switch (clip) {
    case 0: with_decay<OPT, 0>(decay, a...); break;
    case 1: with_decay<OPT, 1>(decay, a...); break;
    case 2: with_decay<OPT, 2>(decay, a...); break;
    default: with_decay<OPT, 3>(decay, a...); break;
  }
}

}  // namespace

int sqsum_blocks(size_t count) {
  const size_t per = (size_t)kQThreads * kSqsumPerThread;
  const size_t want = (count + per - 1) / per;
  return (int)(want < 1 ? 1 : (want > (size_t)kQMaxBlocks ? (size_t)kQMaxBlocks : want));
}

size_t sqsum_partial_doubles() { return kQMaxBlocks; }

hipError_t launch_grad_mean_sqsum(const float* g_shards, size_t shard_stride, int shards, const ShardCounts& counts, float* g_mean,
                                  size_t count, double* partials, double* sqsum, double* norm, hipStream_t stream) {
  long long total = 0;
  for (int r = 0; r < shards; ++r) total += counts.n[r];
  const int blocks = sqsum_blocks(count);
  hipLaunchKernelGGL(grad_mean_sqsum_kernel, dim3(blocks), dim3(kQThreads), 0, stream, g_shards, shard_stride, shards, counts, (double)total,
                     g_mean, count, partials);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(sqsum_finish_kernel, dim3(1), dim3(kQThreads), 0, stream, partials, blocks, sqsum, norm);
  return hipGetLastError();
}

hipError_t launch_optimizer_step(const OptimizerScalars& s, float* p, const float* g_shards, size_t shard_stride, int shards,
                                 const ShardCounts& counts, float* g_mean, float* m, float* v, size_t count, const double* sqsum,
                                 const DecayRanges& ranges, hipStream_t stream) {
  if (count == 0) return hipSuccess;
  long long total = 0;
  for (int r = 0; r < shards; ++r) total += counts.n[r];
  // 16-byte accesses need every vector's start on a 16-byte boundary: the bases and, for several rows, the stride
  const uintptr_t bases = (uintptr_t)p | (uintptr_t)g_shards | (uintptr_t)g_mean | (uintptr_t)m | (uintptr_t)v;
  const bool wide = bases % 16 == 0 && (shards <= 1 || shard_stride % 4 == 0) && count >= (size_t)kStepWide;
  const size_t units = wide ? count / kStepWide : count;
  const size_t want = (units + 255) / 256;
  const unsigned blocks = (unsigned)(want > kStepMaxBlocks ? kStepMaxBlocks : want);
  const int clip = (s.clipnorm > 0.f ? 1 : 0) | (s.clipvalue > 0.f ? 2 : 0);
  const bool decay = s.weight_decay > 0.f && ranges.n > 0;
  const double tot = (double)total;
  switch (s.kind) {
    case kOptNadam: with_clip<kOptNadam>(clip, decay, wide, blocks, stream, p, g_shards, shard_stride, shards, counts, tot, g_mean, m, v, count, s, sqsum, ranges); break;
    case kOptAdam: with_clip<kOptAdam>(clip, decay, wide, blocks, stream, p, g_shards, shard_stride, shards, counts, tot, g_mean, m, v, count, s, sqsum, ranges); break;
    case kOptSgd: with_clip<kOptSgd>(clip, decay, wide, blocks, stream, p, g_shards, shard_stride, shards, counts, tot, g_mean, m, v, count, s, sqsum, ranges); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

}  // namespace dsen2
