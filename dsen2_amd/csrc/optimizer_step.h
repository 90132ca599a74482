// The optimiser step with options (optimizer_step.hip; include/dsen2_hip.h, dsen2_optimizer_step): what travels into the launches
// and the launchers capi_train.hip calls.  Nothing is checked here: dsen2_optimizer_step has checked every argument.
#pragma once
#include "dsen2_internal.h"
#include "nadam_math.h"

namespace dsen2 {

enum { kOptNadam = 0, kOptAdam = 1, kOptSgd = 2, kOptKinds = 3 };

// the scalars of one step, as floats (the kernel widens them): nadam.lr / b1 / b2 / eps serve Adam, nadam.lr serves SGD
struct OptimizerScalars {
  int kind;
  NadamScalars nadam;
  float lr_t, momentum;
  int nesterov;
  float clipnorm, clipvalue, weight_decay;     // 0 = off
};

// the parameters decoupled weight decay applies to: n half-open index ranges [lo, hi), sorted and disjoint, by value in the launch
constexpr int kMaxDecayRanges = 128;
struct DecayRanges {
  int n;
  unsigned lo[kMaxDecayRanges], hi[kMaxDecayRanges];
};

// partial sums grad_mean_sqsum's blocks write (the grid of error_sums.hip: one block per 2048 elements, kQMaxBlocks at the most)
size_t sqsum_partial_doubles();
int sqsum_blocks(size_t count);

// g_mean[i] (where g_mean is given) = the count-weighted mean of the shard rows, launch_nadam_shards' arithmetic;
// *sqsum = the fixed-order float64 sum of (double)g * (double)g; *norm (or NULL) = sqrt(*sqsum)
hipError_t launch_grad_mean_sqsum(const float* g_shards, size_t shard_stride, int shards, const ShardCounts& counts, float* g_mean,
                                  size_t count, double* partials, double* sqsum, double* norm, hipStream_t stream);

// One step of kind s.kind on p, m (, v).  shards >= 1: the gradient is the count-weighted mean of the rows, formed here as
// launch_nadam_shards forms it, and g_mean (or NULL) receives it; shards == 0: g_shards is that mean already.  sqsum (device;
// read when s.clipnorm > 0) is launch_grad_mean_sqsum's.  ranges are read when s.weight_decay > 0 and ranges.n > 0.
hipError_t launch_optimizer_step(const OptimizerScalars& s, float* p, const float* g_shards, size_t shard_stride, int shards,
                                 const ShardCounts& counts, float* g_mean, float* m, float* v, size_t count, const double* sqsum,
                                 const DecayRanges& ranges, hipStream_t stream);

}  // namespace dsen2
