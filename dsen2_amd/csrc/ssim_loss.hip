// ssim_loss.hip — the SSIM term of the training loss (include/dsen2_hip.h, "the SSIM loss term") and its gradient:
//     T = weight * (1/Nw) * sum over unmasked windows of (1 - q),   dT/dout = -(weight/Nw) * G,   Nw = n*c*(h-P+1)*(w-P+1),
// with q the SSIM of csrc/ssim.hip (its separable filter over valid windows, its operation order, float32 inputs promoted to
// float64) per window of every (sample, band) plane of an NCHW pair x = out, y = target.  All arithmetic is float64 with every
// product and every sum rounded on its own (__dmul_rn / __dadd_rn, contraction off); the only fused operations are inside the
// IEEE divisions.  tests/ssim_loss_restatement.py and losses.ssim_term state every operation in numpy in this order.
//
// PER WINDOW (mx, my, exx, eyy, exy the five filtered fields, ssim.hip's row pass then column pass, taps k = 0 .. P-1 in order):
//     m11 = mx*mx  m22 = my*my  m12 = mx*my  s1 = exx - m11  s2 = eyy - m22  s12 = exy - m12
//     A1 = 2*m12 + c1   A2 = 2*s12 + c2   B1 = (m11 + m22) + c1   B2 = (s1 + s2) + c2   den = B1*B2   q = (A1*A2) / den
//     a = ((2*my)*(A2 - A1)) / den - (((2*mx)*q)*(B2 - B1)) / den          (dq/dmx)
//     b = (-q) / B2                                                          (dq/dexx)
//     d = (2*A1) / den                                                       (dq/dexy)
// A window that holds a masked pixel (mask mode 1: the target is 0 in all c bands of that pixel of the sample) adds nothing to
// the sum and has a = b = d = 0.  Nw counts ALL windows in every mask mode.
// PER PIXEL u: the transposed ("full") filter of the three maps, zero outside the map: the column pass t[u_r][p_c] = g[0]*m[u_r][p_c],
// then t = t + g[k]*m[u_r - k][p_c] for k = 1 .. P-1 in order, the row pass the same sum over t[u_r][u_c - k]; then
//     G = (Gt a + (2*x)*Gt b) + y*Gt d        gpad[pixel][band] = (float)((double)gpad[pixel][band] + scale*G),  scale = -(double)weight/Nw.
//
// TILE.  An item is (sample, band, tile); a workgroup of 256 threads takes the items block, block + grid, ... in order.  A tile
// stages S x S samples of x and y (S = 32 for P >= 9, else 28; float32 in LDS, promoted on every read, zeros outside the image)
// starting at (ty*T, tx*T), T = S - 2 (P-1), and holds the RW x RW windows whose origin lies there, RW = S - P + 1; the number of
// tiles along a side of length L is 1 + ceil(max(L - S, 0) / T).  Every window that touches a pixel the tile owns lies in the
// tile: it owns the staged pixels P-1 .. S-P of each axis, and also 0 .. P-2 where it is the first tile of that axis and S-P+1 ..
// where it is the last.  A 32 x 32 plane with P = 11 is one tile of 22 x 22 windows.  A window's (1 - q) is added by the one tile
// that owns its origin: local origins 0 .. T-1 of each axis, all of them in the last tile.
// Phases per item, a barrier between each: stage (and, masked, the pixel-validity plane from all c bands of the target) | row
// pass of the five fields [5][S][RW] (and the row OR of the validity plane) | column pass, the formula, (1 - q) and a, b, d
// [3][RW][RW] | block_tree of { sum (1 - q), unmasked windows } | transposed column pass [3][S][RW] over the row-pass buffer |
// transposed row pass and the read-modify-write of the band's lane of the NHWC16 gradient.  Lanes run along the column in
// every phase.  LDS: 8*(5*S*RW + 3*RW*RW) + 8*S*S + S*S + S*RW bytes, 48.5 KB at P = 11 and at most 53.3 KB (P = 9).
// SUMS: a thread adds its windows i = tid, tid + 256, ... of the tile in index order, block_tree (fixed_sum.h) adds the threads,
// thread 0 adds the block's items in order, one partial pair per block, and one block adds the partials (strided_partials,
// block_tree).  grid = min(items, 4096): a function of the shape alone, no atomics, the same bits on every run.
#include "capi_internal.h"

#include <cmath>

#pragma clang fp contract(off)

#include "fixed_sum.h"

namespace dsen2 {

namespace {

struct SsimLossArgs {
  const float *x, *y;
  float* g;
  double* partials;
  int n, c, h, w, P, S, tiles_x, tiles_y;
  long long items;
  double c1, c2, scale;
  double win[kSsimLossMaxWin];
};

int stage_side(int P) { return P >= 9 ? 32 : 28; }
int tiles_along(int L, int S, int T) { return L <= S ? 1 : 1 + (L - S + T - 1) / T; }
size_t lds_bytes(int P) {
  const size_t S = stage_side(P), RW = S - P + 1;
  return 8 * (5 * S * RW + 3 * RW * RW) + 8 * S * S + S * S + S * RW;
}

template <bool GRAD, bool MASK>
__global__ __launch_bounds__(kQThreads) void ssim_loss_kernel(SsimLossArgs A) {
  extern __shared__ double smem[];
  __shared__ double s_w[kSsimLossMaxWin], s_acc[2];
  const int P = A.P, S = A.S, RW = S - P + 1, T = S - 2 * (P - 1);
  double* const hs = smem;                          // [5][S][RW]: row pass of x, y, x*x, y*y, x*y; then [3][S][RW]: Gt's column pass
  double* const am = hs + 5 * S * RW;               // [RW][RW] each: a, b, d
  double* const bm = am + RW * RW;
  double* const dm = bm + RW * RW;
  float* const xs = reinterpret_cast<float*>(dm + RW * RW);      // [S][S]
  float* const ys = xs + S * S;
  unsigned char* const inv = reinterpret_cast<unsigned char*>(ys + S * S);      // [S][S]: the pixel carries no ground truth
  unsigned char* const rinv = inv + S * S;                                       // [S][RW]: its OR along the window's row
  const int tid = threadIdx.x, H = A.h, W = A.w, OH = H - P + 1, OW = W - P + 1, tiles = A.tiles_x * A.tiles_y;
  const size_t hw = (size_t)H * W;
  if (tid < kSsimLossMaxWin) s_w[tid] = tid < P ? A.win[tid] : 0.0;
  if (tid < 2) s_acc[tid] = 0.0;
  for (long long it = blockIdx.x; it < A.items; it += gridDim.x) {
    const int t = (int)(it % tiles);
    const size_t plane = (size_t)(it / tiles);      // sample * c + band
    const int band = (int)(plane % A.c);
    const size_t smp = plane / A.c;
    const int ty = t / A.tiles_x, tx = t - ty * A.tiles_x;
    const int r0 = ty * T, c0 = tx * T;
    const bool last_y = ty == A.tiles_y - 1, last_x = tx == A.tiles_x - 1;
    const float* const px = A.x + plane * hw;
    const float* const py = A.y + plane * hw;
    const float* const pall = A.y + smp * A.c * hw;
    for (int i = tid; i < S * S; i += kQThreads) {
      const int r = i / S, gr = r0 + r, gc = c0 + (i - r * S);
      const bool in = gr < H && gc < W;
      const size_t o = (size_t)gr * W + gc;
      xs[i] = in ? px[o] : 0.f;
      ys[i] = in ? py[o] : 0.f;
      if (MASK) {
        bool data = !in;
        if (in)
          for (int ch = 0; ch < A.c; ++ch) data |= pall[ch * hw + o] != 0.f;      // -0.0 is 0; NaN and negative values are data
        inv[i] = data ? 0 : 1;
      }
    }
    __syncthreads();                                // also orders s_w and s_acc before their first use
    for (int i = tid; i < S * RW; i += kQThreads) {
      const int r = i / RW, c = i - r * RW;
      const float *qx = xs + r * S + c, *qy = ys + r * S + c;
      double wk = s_w[0], a = (double)qx[0], b = (double)qy[0];
      double fx = __dmul_rn(wk, a), fy = __dmul_rn(wk, b);
      double fxx = __dmul_rn(wk, __dmul_rn(a, a)), fyy = __dmul_rn(wk, __dmul_rn(b, b)), fxy = __dmul_rn(wk, __dmul_rn(a, b));
      for (int k = 1; k < P; ++k) {
        wk = s_w[k];
        a = (double)qx[k];
        b = (double)qy[k];
        fx = __dadd_rn(fx, __dmul_rn(wk, a));
        fy = __dadd_rn(fy, __dmul_rn(wk, b));
        fxx = __dadd_rn(fxx, __dmul_rn(wk, __dmul_rn(a, a)));
        fyy = __dadd_rn(fyy, __dmul_rn(wk, __dmul_rn(b, b)));
        fxy = __dadd_rn(fxy, __dmul_rn(wk, __dmul_rn(a, b)));
      }
      hs[i] = fx;
      hs[S * RW + i] = fy;
      hs[2 * S * RW + i] = fxx;
      hs[3 * S * RW + i] = fyy;
      hs[4 * S * RW + i] = fxy;
      if (MASK) {
        unsigned char any = 0;
        for (int k = 0; k < P; ++k) any |= inv[r * S + c + k];
        rinv[i] = any;
      }
    }
    __syncthreads();
    double v[2] = {0.0, 0.0};
    for (int i = tid; i < RW * RW; i += kQThreads) {
      const int wr = i / RW, wc = i - wr * RW, plane5 = S * RW;
      const double* p = hs + i;                     // window (wr, wc): rows wr .. wr + P - 1 of its column
      double wk = s_w[0];
      double mx = __dmul_rn(wk, p[0]), my = __dmul_rn(wk, p[plane5]);
      double exx = __dmul_rn(wk, p[2 * plane5]), eyy = __dmul_rn(wk, p[3 * plane5]), exy = __dmul_rn(wk, p[4 * plane5]);
      for (int k = 1; k < P; ++k) {
        p += RW;
        wk = s_w[k];
        mx = __dadd_rn(mx, __dmul_rn(wk, p[0]));
        my = __dadd_rn(my, __dmul_rn(wk, p[plane5]));
        exx = __dadd_rn(exx, __dmul_rn(wk, p[2 * plane5]));
        eyy = __dadd_rn(eyy, __dmul_rn(wk, p[3 * plane5]));
        exy = __dadd_rn(exy, __dmul_rn(wk, p[4 * plane5]));
      }
      const double m11 = __dmul_rn(mx, mx), m22 = __dmul_rn(my, my), m12 = __dmul_rn(mx, my);
      const double s1 = __dadd_rn(exx, -m11), s2 = __dadd_rn(eyy, -m22), s12 = __dadd_rn(exy, -m12);
      const double A1 = __dadd_rn(__dmul_rn(2.0, m12), A.c1), A2 = __dadd_rn(__dmul_rn(2.0, s12), A.c2);
      const double B1 = __dadd_rn(__dadd_rn(m11, m22), A.c1), B2 = __dadd_rn(__dadd_rn(s1, s2), A.c2);
      const double den = __dmul_rn(B1, B2);
      const double q = __dmul_rn(A1, A2) / den;
      bool live = r0 + wr < OH && c0 + wc < OW;
      if (MASK) {
        unsigned char any = 0;
        for (int k = 0; k < P; ++k) any |= rinv[(wr + k) * RW + wc];
        live = live && !any;
      }
      if (live && (last_y || wr < T) && (last_x || wc < T)) {
        v[0] = __dadd_rn(v[0], __dadd_rn(1.0, -q));
        v[1] = __dadd_rn(v[1], 1.0);
      }
      if (GRAD) {
        double a = 0.0, b = 0.0, d = 0.0;
        if (live) {
          const double t1 = __dmul_rn(__dmul_rn(2.0, my), __dadd_rn(A2, -A1)) / den;
          const double t2 = __dmul_rn(__dmul_rn(__dmul_rn(2.0, mx), q), __dadd_rn(B2, -B1)) / den;
          a = __dadd_rn(t1, -t2);
          b = -q / B2;
          d = __dmul_rn(2.0, A1) / den;
        }
        am[i] = a;
        bm[i] = b;
        dm[i] = d;
      }
    }
    block_tree<2>(v);                               // its barriers also order a, b, d and end every read of the row pass
    if (tid == 0) {
      s_acc[0] = __dadd_rn(s_acc[0], v[0]);
      s_acc[1] = __dadd_rn(s_acc[1], v[1]);
    }
    if (GRAD) {
      for (int i = tid; i < S * RW; i += kQThreads) {
        const int ur = i / RW, pc = i - ur * RW;
        double ta = __dmul_rn(s_w[0], ur < RW ? am[ur * RW + pc] : 0.0);
        double tb = __dmul_rn(s_w[0], ur < RW ? bm[ur * RW + pc] : 0.0);
        double td = __dmul_rn(s_w[0], ur < RW ? dm[ur * RW + pc] : 0.0);
        for (int k = 1; k < P; ++k) {
          const int r = ur - k;
          const bool in = r >= 0 && r < RW;
          const int o = in ? r * RW + pc : 0;
          const double wk = s_w[k];
          ta = __dadd_rn(ta, __dmul_rn(wk, in ? am[o] : 0.0));
          tb = __dadd_rn(tb, __dmul_rn(wk, in ? bm[o] : 0.0));
          td = __dadd_rn(td, __dmul_rn(wk, in ? dm[o] : 0.0));
        }
        hs[i] = ta;
        hs[S * RW + i] = tb;
        hs[2 * S * RW + i] = td;
      }
      __syncthreads();
      const int lo_r = ty == 0 ? 0 : P - 1, hi_r = last_y ? S : S - (P - 1);
      const int lo_c = tx == 0 ? 0 : P - 1, hi_c = last_x ? S : S - (P - 1);
      for (int i = tid; i < S * S; i += kQThreads) {
        const int ur = i / S, uc = i - ur * S, gr = r0 + ur, gc = c0 + uc;
        if (gr >= H || gc >= W || ur < lo_r || ur >= hi_r || uc < lo_c || uc >= hi_c) continue;
        const double* row = hs + ur * RW;
        double ga = __dmul_rn(s_w[0], uc < RW ? row[uc] : 0.0);
        double gb = __dmul_rn(s_w[0], uc < RW ? row[S * RW + uc] : 0.0);
        double gd = __dmul_rn(s_w[0], uc < RW ? row[2 * S * RW + uc] : 0.0);
        for (int k = 1; k < P; ++k) {
          const int cc = uc - k;
          const bool in = cc >= 0 && cc < RW;
          const int o = in ? cc : 0;
          const double wk = s_w[k];
          ga = __dadd_rn(ga, __dmul_rn(wk, in ? row[o] : 0.0));
          gb = __dadd_rn(gb, __dmul_rn(wk, in ? row[S * RW + o] : 0.0));
          gd = __dadd_rn(gd, __dmul_rn(wk, in ? row[2 * S * RW + o] : 0.0));
        }
        const double xv = (double)xs[i], yv = (double)ys[i];
        const double G = __dadd_rn(__dadd_rn(ga, __dmul_rn(__dmul_rn(2.0, xv), gb)), __dmul_rn(yv, gd));
        float* const dst = A.g + ((smp * H + gr) * W + gc) * 16 + band;
        *dst = (float)__dadd_rn((double)*dst, __dmul_rn(A.scale, G));
      }
      __syncthreads();                              // the next item stages over xs and ys
    }
  }
  if (tid == 0) {
    A.partials[2 * (size_t)blockIdx.x + 0] = s_acc[0];
    A.partials[2 * (size_t)blockIdx.x + 1] = s_acc[1];
  }
}

// one block: out = { sum (1 - q), Nw [, unmasked windows] } from the blocks' partial pairs
__global__ __launch_bounds__(kQThreads) void ssim_loss_finish_kernel(const double* __restrict__ partials, int blocks, double nw, int three,
                                                                     double* __restrict__ out) {
  double v[2];
  strided_partials<2>(partials, blocks, 2, v);
  block_tree<2>(v);
  if (threadIdx.x == 0) {
    out[0] = v[0];
    out[1] = nw;
    if (three) out[2] = v[1];
  }
}

int check_pair(const char* who, const void* out, const void* target, int n, int c, int h, int w, int mask_mode) {
  if (!out || !target) return fail(DSEN2_ERR_INVALID, "%s: NULL argument", who);
  if (n <= 0 || h <= 0 || w <= 0 || c < 1 || c > 15) return fail(DSEN2_ERR_INVALID, "%s: bad shape n=%d c=%d h=%d w=%d (c in 1..15)", who, n, c, h, w);
  if ((size_t)n * h * w * 16 >= ((size_t)1 << 31)) return fail(DSEN2_ERR_INVALID, "%s: %d x %d x %d pixels exceed one launch", who, n, h, w);
  if (mask_mode < 0 || mask_mode >= kMaskModes) return fail(DSEN2_ERR_INVALID, "%s: mask mode %d unknown (0 none, 1 no-data)", who, mask_mode);
  return DSEN2_OK;
}

}  // namespace

size_t ssim_loss_work_doubles() { return 2 * (size_t)kQMaxBlocks + 3; }

hipError_t launch_ssim_loss(const float* out, const float* y, int n, int c, int h, int w, const SsimLossTerm& term, int mask, float* gpad,
                            double* work, bool three, hipStream_t stream) {
  const int P = term.win;
  if (n <= 0 || c < 1 || c > 16 || P < kSsimLossMinWin || P > kSsimLossMaxWin || P % 2 == 0 || h < P || w < P || mask < 0 || mask >= kMaskModes)
    return hipErrorInvalidValue;
  SsimLossArgs A{};
  A.x = out; A.y = y; A.g = gpad; A.partials = work;
  A.n = n; A.c = c; A.h = h; A.w = w; A.P = P; A.S = stage_side(P);
  const int T = A.S - 2 * (P - 1);
  A.tiles_x = tiles_along(w, A.S, T);
  A.tiles_y = tiles_along(h, A.S, T);
  A.items = (long long)n * c * A.tiles_x * A.tiles_y;
  const double nw = (double)n * c * (h - P + 1) * (double)(w - P + 1);
  A.c1 = term.c1; A.c2 = term.c2;
  A.scale = -(double)term.weight / nw;
  for (int i = 0; i < kSsimLossMaxWin; ++i) A.win[i] = i < P ? term.w[i] : 0.0;
  const int grid = A.items < kQMaxBlocks ? (int)A.items : kQMaxBlocks;
  const size_t lds = lds_bytes(P);
  auto go = [&](auto kernel) { hipLaunchKernelGGL(kernel, dim3(grid), dim3(kQThreads), lds, stream, A); };
  if (gpad) mask ? go(ssim_loss_kernel<true, true>) : go(ssim_loss_kernel<true, false>);
  else mask ? go(ssim_loss_kernel<false, true>) : go(ssim_loss_kernel<false, false>);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(ssim_loss_finish_kernel, dim3(1), dim3(kQThreads), 0, stream, work, grid, nw, three ? 1 : 0, work + 2 * (size_t)kQMaxBlocks);
  return hipGetLastError();
}

}  // namespace dsen2

using namespace dsen2;

extern "C" int dsen2_ssim_loss_grad(const float* dev_out, const float* dev_target, int n, int c, int h, int w, float weight,
                                    const double* host_window, int win, double c1, double c2, int mask_mode, float* dev_g_nhwc16,
                                    double* dev_sums2, void* stream) {
  return guarded([&]() -> int {
    const char* who = "ssim_loss_grad";
    if (!dev_g_nhwc16 || !dev_sums2) return fail(DSEN2_ERR_INVALID, "%s: NULL argument", who);
    if (int rc = check_pair(who, dev_out, dev_target, n, c, h, w, mask_mode)) return rc;
    SsimLossTerm term;
    if (int rc = check_ssim_loss_term(who, weight, host_window, win, c1, c2, &term)) return rc;
    if (h < win || w < win) return fail(DSEN2_ERR_INVALID, "%s: a plane of %d x %d is smaller than the %d x %d window", who, h, w, win, win);
    hipStream_t s = (hipStream_t)stream;
    return launch_once_with_temp(who, nullptr, ssim_loss_work_doubles() * sizeof(double), s, [&](char* dev) {
      double* work = reinterpret_cast<double*>(dev);
      hipError_t e = launch_ssim_loss(dev_out, dev_target, n, c, h, w, term, mask_mode, dev_g_nhwc16, work, false, s);
      if (e != hipSuccess) return e;
      return hipMemcpyAsync(dev_sums2, work + 2 * (size_t)kQMaxBlocks, 2 * sizeof(double), hipMemcpyDeviceToDevice, s);
    });
  });
}

extern "C" int dsen2_ssim_loss_sums_workspace_bytes(size_t* bytes) {
  if (!bytes) return fail(DSEN2_ERR_INVALID, "ssim_loss_sums_workspace_bytes: NULL argument");
  *bytes = ssim_loss_work_doubles() * sizeof(double);
  return DSEN2_OK;
}

extern "C" int dsen2_ssim_loss_sums(const float* dev_pred, const float* dev_target, int n, int c, int h, int w, const double* host_window,
                                    int win, double c1, double c2, int mask_mode, void* dev_work, size_t work_bytes, double* dev_out3,
                                    void* stream) {
  return guarded([&]() -> int {
    const char* who = "ssim_loss_sums";
    if (!dev_work || !dev_out3) return fail(DSEN2_ERR_INVALID, "%s: NULL argument", who);
    if (int rc = check_pair(who, dev_pred, dev_target, n, c, h, w, mask_mode)) return rc;
    SsimLossTerm term;
    if (int rc = check_ssim_loss_term(who, 1.f, host_window, win, c1, c2, &term)) return rc;
    if (h < win || w < win) return fail(DSEN2_ERR_INVALID, "%s: a plane of %d x %d is smaller than the %d x %d window", who, h, w, win, win);
    const size_t need = ssim_loss_work_doubles() * sizeof(double);
    if (work_bytes < need)
      return fail(DSEN2_ERR_WORKSPACE, "%s: workspace of %zu bytes, dsen2_ssim_loss_sums_workspace_bytes asks for %zu", who, work_bytes, need);
    hipStream_t s = (hipStream_t)stream;
    double* work = static_cast<double*>(dev_work);
    hipError_t e = launch_ssim_loss(dev_pred, dev_target, n, c, h, w, term, mask_mode, nullptr, work, true, s);
    if (e != hipSuccess) return fail(DSEN2_ERR_HIP, "%s launch: %s", who, hipGetErrorString(e));
    HIP_TRY(hipMemcpyAsync(dev_out3, work + 2 * (size_t)kQMaxBlocks, 3 * sizeof(double), hipMemcpyDeviceToDevice, s));
    return DSEN2_OK;
  });
}
