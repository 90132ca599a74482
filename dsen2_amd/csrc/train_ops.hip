// train_ops.hip — the memory-bound kernels of the training step (capi_train.hip): loss and dL/dout, ReLU-gradient masks
// (fp32, and with the bf16x3 / bf16 operand tensor of du written in the same pass), the Nadam update and the device weight
// repack, and the count-weighted sum of sharded gradients with Nadam in one pass.  Every reduction runs in a fixed order (no
// float atomics): the same inputs give the same bits on every run.
#include "dsen2_internal.h"
#include "fixed_sum.h"
#include "loss_terms.h"
#include "nadam_math.h"

namespace dsen2 {

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kLossMaxBlocks = 1024;

// The loss of kind KIND (loss_terms.h) over NCHW [n][c][hw]: e = out - y in float32, d = (double)e, dL/dout = (float)(rho'(d) *
// (double)inv_count) written as NHWC16 [n*hw][16] (channels >= c zero), partial[block] = (sum rho(d), sum d^2) of the block's
// pixels (grid-stride, fixed grid; fixed_sum.h's tree).  MASK: a pixel whose target is 0 (or -0) in all c bands adds nothing to
// either sum and gets a zero gradient in every band; the thread owns all bands of its pixel, so the test costs no second pass.
// The default pair is the <kLossMae, false> instance: sign(e) * inv_count, TensorFlow's Abs gradient with sign(0) = 0.
template <int KIND, bool MASK>
__global__ __launch_bounds__(kQThreads) void loss_grad_kernel(const float* __restrict__ out, const float* __restrict__ y,
                                                              float* __restrict__ gpad, double* __restrict__ partial, size_t pixels,
                                                              int hw, int c, float inv_count, float param) {
  const double p = (double)param, inv = (double)inv_count;
  double sa = 0.0, sq = 0.0;
  for (size_t pix = (size_t)blockIdx.x * kQThreads + threadIdx.x; pix < pixels; pix += (size_t)gridDim.x * kQThreads) {
    const size_t img = pix / hw, q = pix % hw;
    float ev[16];
    bool valid = !MASK;
#pragma unroll
    for (int ch = 0; ch < 16; ++ch) {
      ev[ch] = 0.f;
      if (ch < c) {
        const size_t idx = (img * c + ch) * hw + q;
        const float yv = y[idx];
        ev[ch] = out[idx] - yv;
        if (MASK) valid |= yv != 0.f;          // -0.0 compares equal to 0: no data; NaN and negative values are data
      }
    }
    float gv[16];
#pragma unroll
    for (int ch = 0; ch < 16; ++ch) {
      gv[ch] = 0.f;
      if (ch < c && valid) {
        const double d = (double)ev[ch];
        double rho, slope;
        loss_terms<KIND>(d, p, rho, slope);
        gv[ch] = (float)__dmul_rn(slope, inv);
        sa = __dadd_rn(sa, rho);
        sq = __dadd_rn(sq, __dmul_rn(d, d));
      }
    }
    f32x4* dst = reinterpret_cast<f32x4*>(gpad + pix * 16);
#pragma unroll
    for (int k = 0; k < 4; ++k) dst[k] = f32x4{gv[4 * k], gv[4 * k + 1], gv[4 * k + 2], gv[4 * k + 3]};
  }
  double v[2] = {sa, sq};
  block_tree<2>(v);
  if (threadIdx.x == 0) {
    partial[2 * (size_t)blockIdx.x + 0] = v[0];
    partial[2 * (size_t)blockIdx.x + 1] = v[1];
  }
}

// one block: loss2 = ((float)(sum rho / count), (float)(sum d^2 / count)) from the blocks' partial pairs, in a fixed order
// ssim_sums (or NULL): { sum (1 - q), Nw } of the SSIM term (ssim_loss.hip), added as tscale * sum, tscale = weight / Nw, in double
__global__ __launch_bounds__(kQThreads) void loss_final_kernel(const double* __restrict__ partial, int blocks, double count,
                                                               float* __restrict__ loss2, const double* __restrict__ ssim_sums,
                                                               double tscale) {
  double v[2];
  strided_partials<2>(partial, blocks, 2, v);
  block_tree<2>(v);
  if (threadIdx.x == 0) {
    loss2[0] = ssim_sums ? (float)__dadd_rn(v[0] / count, __dmul_rn(tscale, ssim_sums[0])) : (float)(v[0] / count);
    loss2[1] = (float)(v[1] / count);
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

// (nadam_one, nadam_kernel's arithmetic on one parameter for a gradient already held in double: nadam_math.h)

// The count-weighted mean of `shards` gradient vectors, added in shard order in double, and the Nadam update on it, one pass
// (launch_nadam_shards).  A shard whose count is 0 is never read.  count * g is exact in double (count < 2^24), so an FMA and a
// multiply followed by an add round alike.  W floats per access (W = 4: 16 bytes) on elements [0, W * units), the last count % W
// elements by the first threads of block 0; W = 1: one element per unit.  One unit per thread: a grid capped at 2048 blocks ran
// 10 % slower at VDSen2's 37.8 M parameters, the uncapped one at nadam_kernel's rate (profiles/train_data_parallel.md).  The
// stride of the loop is a guard only: it keeps a count beyond kShardsMaxBlocks * 256 units (2^38) inside the grid's range.
template <int W>
__global__ __launch_bounds__(256) void nadam_shards_kernel(float* __restrict__ p, const float* __restrict__ g, size_t stride, int shards,
                                                         ShardCounts counts, double total, float* __restrict__ g_mean,
                                                         float* __restrict__ m, float* __restrict__ v, size_t count, NadamScalars s) {
  typedef float vec __attribute__((ext_vector_type(W)));
  const size_t units = count / W;
  for (size_t u = (size_t)blockIdx.x * blockDim.x + threadIdx.x; u < units; u += (size_t)gridDim.x * blockDim.x) {
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
    vec pv = reinterpret_cast<vec*>(p)[u], mv = reinterpret_cast<vec*>(m)[u], vv = reinterpret_cast<vec*>(v)[u], gm;
#pragma unroll
    for (int e = 0; e < W; ++e) {
      gm[e] = (float)(acc[e] / total);
      float pe = pv[e], me = mv[e], ve = vv[e];
      nadam_one((double)gm[e], pe, me, ve, s);
      pv[e] = pe; mv[e] = me; vv[e] = ve;
    }
    if (g_mean) reinterpret_cast<vec*>(g_mean)[u] = gm;
    reinterpret_cast<vec*>(p)[u] = pv;
    reinterpret_cast<vec*>(m)[u] = mv;
    reinterpret_cast<vec*>(v)[u] = vv;
  }
  if (W > 1 && blockIdx.x == 0 && units * W + threadIdx.x < count) {
    const size_t i = units * W + threadIdx.x;
    double acc = 0.0;
    for (int r = 0; r < shards; ++r) {
      const int c = counts.n[r];
      if (c > 0) acc = acc + (double)c * (double)g[(size_t)r * stride + i];
    }
    const float gm = (float)(acc / total);
    if (g_mean) g_mean[i] = gm;
    nadam_one((double)gm, p[i], m[i], v[i], s);
  }
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

// ---- precision 2 (bf16x3) ----
// f32_to_bf16_rne (dsen2_internal.h) on the device: the host packers' rounding, the same integer arithmetic
__device__ __forceinline__ unsigned bf16_rne(float f) {
  unsigned u = __builtin_bit_cast(unsigned, f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (u >> 16) | 0x40u;
  u += 0x7fffu + ((u >> 16) & 1u);
  return u >> 16;
}
__device__ __forceinline__ float bf16_value(unsigned h16) { return __builtin_bit_cast(float, h16 << 16); }
// element e (0..7) of a 16-byte pixel of a blocked 16-bit tensor
__device__ __forceinline__ unsigned half_of(const uint4& v, int e) {
  const unsigned d = e < 2 ? v.x : e < 4 ? v.y : e < 6 ? v.z : v.w;
  return (e & 1) ? d >> 16 : d & 0xffffu;
}
__device__ __forceinline__ uint4 pack_halves(const unsigned* h) {
  return make_uint4(h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16));
}

// One thread per (pixel, 8-channel block), the block fastest: the fp32 side is read / written in contiguous 32-byte pieces.
// hx [n][2][nblk][img_pix] pixels of 8 x 16 bit (plane 0 = hi, the ties-away rounding of the bit pattern), lo [n][nblk][img_pix]:
// value bits = ((hi - (lo >> 15)) << 16) | lo, the inverse of split3_kernel (conv3x3_body16w.hip)
__global__ __launch_bounds__(256) void join3_kernel(const uint4* __restrict__ hx, const uint4* __restrict__ lo, float* __restrict__ out,
                                                  size_t total, int img_pix, int nblk) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int blk = (int)(i % nblk);
  const size_t pix = i / nblk, img = pix / img_pix, px = pix % img_pix;
  const uint4 h = hx[((img * 2) * nblk + blk) * img_pix + px];
  const uint4 l = lo[(img * nblk + blk) * img_pix + px];
  float v[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const unsigned le = half_of(l, e);
    const unsigned top = (half_of(h, e) - (le >> 15)) & 0xffffu;
    v[e] = __builtin_bit_cast(float, (top << 16) | le);
  }
  f32x4* dst = reinterpret_cast<f32x4*>(out + (pix * nblk + blk) * 8);
  dst[0] = f32x4{v[0], v[1], v[2], v[3]};
  dst[1] = f32x4{v[4], v[5], v[6], v[7]};
}

// du = t > 0 ? v : 0 as (hi | lo) planes; v fp32 NHWC, t and du [n][2][nblk][img_pix] pixels of 8 bf16
__global__ __launch_bounds__(256) void mask_split3_kernel(const float* __restrict__ v_nhwc, const uint4* __restrict__ t, uint4* __restrict__ du,
                                                        size_t total, int img_pix, int nblk) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int blk = (int)(i % nblk);
  const size_t pix = i / nblk, img = pix / img_pix, px = pix % img_pix;
  const size_t hi_at = ((img * 2) * nblk + blk) * img_pix + px, lo_at = hi_at + (size_t)nblk * img_pix;
  const uint4 th = t[hi_at], tl = t[lo_at];
  const f32x4* src = reinterpret_cast<const f32x4*>(v_nhwc + (pix * nblk + blk) * 8);
  const f32x4 a = src[0], b = src[1];
  const float v[8] = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
  unsigned h[8], l[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const float tv = bf16_value(half_of(th, e)) + bf16_value(half_of(tl, e));
    const float x = tv > 0.f ? v[e] : 0.f;
    h[e] = bf16_rne(x);
    l[e] = bf16_rne(x - bf16_value(h[e]));
  }
  du[hi_at] = pack_halves(h);
  du[lo_at] = pack_halves(l);
}

// du = bf16_rne(t > 0 ? v : 0) as one plane; v fp32 NHWC, t and du [n][nblk][img_pix] pixels of 8 bf16 (launch_mask_round16)
__global__ __launch_bounds__(256) void mask_round16_kernel(const float* __restrict__ v_nhwc, const uint4* __restrict__ t, uint4* __restrict__ du,
                                                         size_t total, int img_pix, int nblk) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int blk = (int)(i % nblk);
  const size_t pix = i / nblk, img = pix / img_pix, px = pix % img_pix;
  const size_t at = (img * nblk + blk) * img_pix + px;
  const uint4 tv = t[at];
  const f32x4* src = reinterpret_cast<const f32x4*>(v_nhwc + (pix * nblk + blk) * 8);
  const f32x4 a = src[0], b = src[1];
  const float v[8] = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
  unsigned h[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) h[e] = bf16_rne(bf16_value(half_of(tv, e)) > 0.f ? v[e] : 0.f);
  du[at] = pack_halves(h);
}

// one 32-bit word of a packed precision-2 buffer from the keras-flat values (launch_gather16)
__device__ __forceinline__ unsigned gather16_half(const float* __restrict__ src, int entry) {
  if (entry == 0) return 0u;
  const float w = src[(entry >> 2) - 1];
  const int kind = entry & 3;
  const unsigned hi = bf16_rne(w);
  if (kind == kGatherHi) return hi;
  if (kind == kGatherLo) return bf16_rne(w - bf16_value(hi));
  const unsigned u = __builtin_bit_cast(unsigned, w);
  return kind == kGatherF32Low ? u & 0xffffu : u >> 16;
}
__global__ __launch_bounds__(256) void gather16_kernel(unsigned* __restrict__ dst, const float* __restrict__ src, const int* __restrict__ map,
                                                     size_t words, size_t dst_stride, size_t src_stride) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= words) return;
  const float* s = src + (size_t)blockIdx.y * src_stride;
  dst[(size_t)blockIdx.y * dst_stride + i] = gather16_half(s, map[2 * i]) | (gather16_half(s, map[2 * i + 1]) << 16);
}

unsigned blocks_for(size_t n, unsigned per) { return (unsigned)((n + per - 1) / per); }
constexpr int kShardsWide = 4;                      // floats per access of nadam_shards_kernel's wide form
constexpr size_t kShardsMaxBlocks = (size_t)1 << 30;

}  // namespace

size_t loss_partial_doubles(size_t pixels) {
  size_t b = (pixels + kQThreads - 1) / kQThreads;
  if (b > (size_t)kLossMaxBlocks) b = kLossMaxBlocks;
  if (b < 1) b = 1;
  return 2 * b;
}

hipError_t launch_loss_grad(const float* out, const float* y, float* gpad, double* partial, float* loss2, int n, int c, int h, int w,
                            int kind, float param, int mask, hipStream_t stream, const SsimLossTerm* ssim, double* ssim_work) {
  if (c < 1 || c > 16 || kind < 0 || kind >= kLossKinds || mask < 0 || mask >= kMaskModes) return hipErrorInvalidValue;
  if (ssim && (!ssim_work || !(ssim->weight > 0.f))) return hipErrorInvalidValue;
  const size_t pixels = (size_t)n * h * w;
  const int blocks = (int)(loss_partial_doubles(pixels) / 2);
  const double count = (double)pixels * c;
  const float inv = (float)(1.0 / count);
  with_loss(kind, mask, [&](auto k, auto m) {
    hipLaunchKernelGGL((loss_grad_kernel<decltype(k)::value, decltype(m)::value>), dim3(blocks), dim3(kQThreads), 0, stream, out, y, gpad,
                       partial, pixels, h * w, c, inv, param);
  });
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const double* ssim_sums = nullptr;
  double tscale = 0.0;
  if (ssim) {
    e = launch_ssim_loss(out, y, n, c, h, w, *ssim, mask, gpad, ssim_work, false, stream);
    if (e != hipSuccess) return e;
    ssim_sums = ssim_work + ssim_loss_work_doubles() - 3;
    tscale = (double)ssim->weight / ((double)n * c * (h - ssim->win + 1) * (double)(w - ssim->win + 1));
  }
  hipLaunchKernelGGL(loss_final_kernel, dim3(1), dim3(kQThreads), 0, stream, partial, blocks, count, loss2, ssim_sums, tscale);
  return hipGetLastError();
}

hipError_t launch_relu_mask(float* v, const float* m, size_t count, hipStream_t stream) {
  if (count % 4 != 0) return hipErrorInvalidValue;
  if (count == 0) return hipSuccess;
  hipLaunchKernelGGL(relu_mask_kernel, dim3(blocks_for(count / 4, 256)), dim3(256), 0, stream, v, m, count / 4);
  return hipGetLastError();
}

hipError_t launch_join3_f32(const void* hx, const void* lo, float* out_nhwc, int n, int h, int w, int c, hipStream_t stream) {
  if (n <= 0 || h <= 0 || w <= 0 || c <= 0 || c % 8 != 0 || c > 512) return hipErrorInvalidValue;
  const size_t total = (size_t)n * h * w * (c / 8);
  hipLaunchKernelGGL(join3_kernel, dim3(blocks_for(total, 256)), dim3(256), 0, stream, reinterpret_cast<const uint4*>(hx),
                     reinterpret_cast<const uint4*>(lo), out_nhwc, total, h * w, c / 8);
  return hipGetLastError();
}

hipError_t launch_mask_split3(const float* v_nhwc, const void* t_planes, void* du_planes, int n, int h, int w, int c, hipStream_t stream) {
  if (n <= 0 || h <= 0 || w <= 0 || c <= 0 || c % 8 != 0 || c > 512) return hipErrorInvalidValue;
  const size_t total = (size_t)n * h * w * (c / 8);
  hipLaunchKernelGGL(mask_split3_kernel, dim3(blocks_for(total, 256)), dim3(256), 0, stream, v_nhwc,
                     reinterpret_cast<const uint4*>(t_planes), reinterpret_cast<uint4*>(du_planes), total, h * w, c / 8);
  return hipGetLastError();
}

hipError_t launch_mask_round16(const float* v_nhwc, const void* t_plane, void* du_plane, int n, int h, int w, int c, hipStream_t stream) {
  if (n <= 0 || h <= 0 || w <= 0 || c <= 0 || c % 8 != 0 || c > 512) return hipErrorInvalidValue;
  const size_t total = (size_t)n * h * w * (c / 8);
  hipLaunchKernelGGL(mask_round16_kernel, dim3(blocks_for(total, 256)), dim3(256), 0, stream, v_nhwc,
                     reinterpret_cast<const uint4*>(t_plane), reinterpret_cast<uint4*>(du_plane), total, h * w, c / 8);
  return hipGetLastError();
}

hipError_t launch_gather16(void* dst, const float* src, const int* map, size_t words, int layers, size_t dst_stride, size_t src_stride,
                           hipStream_t stream) {
  if (words == 0 || layers <= 0) return hipSuccess;
  if (layers > 65535) return hipErrorInvalidValue;
  hipLaunchKernelGGL(gather16_kernel, dim3(blocks_for(words, 256), (unsigned)layers), dim3(256), 0, stream,
                     reinterpret_cast<unsigned*>(dst), src, map, words, dst_stride, src_stride);
  return hipGetLastError();
}

hipError_t launch_nadam(float* p, const float* g, float* m, float* v, size_t count, float lr, float b1, float b2, float eps,
                        float mc_t, float mc_t1, float ms_new, float ms_next, float b2_pow_t, hipStream_t stream) {
  if (count == 0) return hipSuccess;
  hipLaunchKernelGGL(nadam_kernel, dim3(blocks_for(count, 256)), dim3(256), 0, stream, p, g, m, v, count, lr, b1, b2, eps, mc_t,
                     mc_t1, ms_new, ms_next, b2_pow_t);
  return hipGetLastError();
}

hipError_t launch_nadam_shards(float* p, const float* g_shards, size_t shard_stride, int shards, const ShardCounts& counts, float* g_mean,
                               float* m, float* v, size_t count, float lr, float b1, float b2, float eps, float mc_t, float mc_t1,
                               float ms_new, float ms_next, float b2_pow_t, hipStream_t stream) {
  long long total = 0;
  for (int r = 0; r < shards; ++r) total += counts.n[r];
  if (count == 0) return hipSuccess;
  const NadamScalars s{lr, b1, b2, eps, mc_t, mc_t1, ms_new, ms_next, b2_pow_t};
  // 16-byte accesses need every vector's start on a 16-byte boundary: the bases and, for the shards, the stride
  const uintptr_t bases = (uintptr_t)p | (uintptr_t)g_shards | (uintptr_t)g_mean | (uintptr_t)m | (uintptr_t)v;
  const bool wide = bases % 16 == 0 && (shards == 1 || shard_stride % 4 == 0) && count >= (size_t)kShardsWide;
  const size_t units = wide ? count / kShardsWide : count;
  const size_t want = (units + 255) / 256;
  const unsigned blocks = (unsigned)(want > kShardsMaxBlocks ? kShardsMaxBlocks : want);
  if (wide)
    hipLaunchKernelGGL(nadam_shards_kernel<kShardsWide>, dim3(blocks), dim3(256), 0, stream, p, g_shards, shard_stride, shards, counts,
                       (double)total, g_mean, m, v, count, s);
  else
    hipLaunchKernelGGL(nadam_shards_kernel<1>, dim3(blocks), dim3(256), 0, stream, p, g_shards, shard_stride, shards, counts,
                       (double)total, g_mean, m, v, count, s);
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
