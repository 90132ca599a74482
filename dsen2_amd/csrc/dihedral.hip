// dihedral.hip — the 8 flips and rotations of NCHW float32 planes (the dihedral group of the square), for the geometric
// self-ensemble at prediction time and for flip / rotate augmentation while fine-tuning.
//
// Convention (include/dsen2_hip.h, "dihedral"): op = k + 4 f, D_op(a) = rot90(f ? a[..., ::-1] : a, k) counter-clockwise.  Every
// op is an index map out[i][j] = in[sy][sx] that is affine in (i, j), plain or transposing (odd k: H and W swap):
//     plain:       sy = ry ? ih - 1 - i : i,   sx = rx ? iw - 1 - j : j
//     transposing: sy = ry ? ih - 1 - j : j,   sx = rx ? iw - 1 - i : i
// and the inverse of an op is again one of the eight: a rotation's is the opposite rotation, a reflection (f = 1) is its own.
// So ONE gather serves D and D^-1 alike.
//
// One workgroup moves one 32 x 32 tile of one OUTPUT plane through LDS: it reads the tile's source pixels along the source's
// rows (consecutive lanes = consecutive, ascending or descending, source columns: coalesced for all 8 ops), and writes along the
// output's rows; a transposing op reads LDS by columns, which the row stride of 33 floats spreads over all 32 banks.  Ragged
// edges are bounds on (i, j); pure data movement in store mode (any bit pattern survives), one fp32 add — and one correctly
// rounded divide — per element in the accumulating modes.  No atomics: every output element has exactly one writer.
#include "dsen2_internal.h"

namespace dsen2 {

namespace {

constexpr int kDTile = 32;               // tile edge
constexpr int kDStride = kDTile + 1;     // LDS row stride in floats: column reads hit 32 different banks
constexpr int kDRows = 8;                // rows of the tile a pass of the 256 threads covers

typedef float f32x4 __attribute__((ext_vector_type(4)));

// (dihedral_bits: the (transposing, ry, rx) bits of an op, dsen2_internal.h)
__host__ __device__ __forceinline__ int dihedral_inverse(int op) {
  op &= 7;
  return (op & 4) ? op : ((4 - op) & 3);
}

enum : int { kDStore = 0, kDAdd = 1, kDAddFinish = 2 };

// in: planes of ih x iw; out: planes of oh x ow ((iw, ih) for a transposing op).  grid.x = planes * tiles_i * tiles_j.
// dev_ops != NULL (store mode, ih == iw): plane p belongs to sample p / c and takes dev_ops[p / c] & 7 (its inverse when
// `inverse`), else `op` as given (the caller has already inverted it).
template <int MODE, bool WIDE>
__global__ __launch_bounds__(256) void dihedral_kernel(const float* __restrict__ in, float* out, int ih, int iw, int oh, int ow,
                                                       int tiles_i, int tiles_j, int op, const int* __restrict__ dev_ops, int c,
                                                       int inverse, float count) {
  __shared__ float tile[kDTile * kDStride];
  const unsigned tiles = (unsigned)tiles_i * (unsigned)tiles_j;
  const unsigned p = blockIdx.x / tiles, t = blockIdx.x - p * tiles;
  const int i0 = (int)(t / (unsigned)tiles_j) * kDTile, j0 = (int)(t % (unsigned)tiles_j) * kDTile;
  if (dev_ops) {
    op = dev_ops[p / (unsigned)c] & 7;
    if (inverse) op = dihedral_inverse(op);
  }
  const int bits = dihedral_bits(op);
  const bool tr = bits & 4, ry = bits & 2, rx = bits & 1;
  const float* const src = in + (size_t)p * ih * iw;
  float* const dst = out + (size_t)p * oh * ow;
  const int tid = threadIdx.x;

  // tile[a][b]: b runs along the source's rows.  plain: (i, j) = (i0 + a, j0 + b); transposing: (i, j) = (i0 + b, j0 + a).
  if constexpr (WIDE) {
    // iw % 4 == 0 and 16-byte aligned planes: a lane reads the 4 source columns of output columns / rows 4 q .. 4 q + 3 as ONE
    // 16-byte access (the run is aligned in the source because its length and the plane's width are multiples of 4)
    const int q = tid & 7, a = tid >> 3;         // 8 lanes per row of the tile, all 32 rows in one pass
    const int i = tr ? i0 + 4 * q : i0 + a, j = tr ? j0 + a : j0 + 4 * q;
    if (i < oh && j < ow) {               // (the extent along b is iw, a multiple of 4: the four are in or out together)
      const int sy = tr ? (ry ? ih - 1 - j : j) : (ry ? ih - 1 - i : i);
      const int b_first = tr ? i : j;
      const int sx = rx ? iw - 4 - b_first : b_first;
      const f32x4 v = *reinterpret_cast<const f32x4*>(src + (size_t)sy * iw + sx);
      float* const row = tile + a * kDStride + 4 * q;
      row[0] = rx ? v.w : v.x; row[1] = rx ? v.z : v.y; row[2] = rx ? v.y : v.z; row[3] = rx ? v.x : v.w;
    }
  } else {
    const int b = tid & 31;
    for (int a = tid >> 5; a < kDTile; a += kDRows) {
      const int i = tr ? i0 + b : i0 + a, j = tr ? j0 + a : j0 + b;
      if (i < oh && j < ow) {
        const int sy = tr ? (ry ? ih - 1 - j : j) : (ry ? ih - 1 - i : i);
        const int sx = tr ? (rx ? iw - 1 - i : i) : (rx ? iw - 1 - j : j);
        tile[a * kDStride + b] = src[(size_t)sy * iw + sx];
      }
    }
  }
  __syncthreads();
  {
    const int lj = tid & 31;
    for (int li = tid >> 5; li < kDTile; li += kDRows) {
      const int i = i0 + li, j = j0 + lj;
      if (i < oh && j < ow) {
        float v = tr ? tile[lj * kDStride + li] : tile[li * kDStride + lj];
        float* const o = dst + (size_t)i * ow + j;
        if constexpr (MODE != kDStore) v = *o + v;
        if constexpr (MODE == kDAddFinish) v = __fdiv_rn(v, count);
        *o = v;
      }
    }
  }
}

template <int MODE>
hipError_t launch_mode(const float* in, float* out, int planes, int c, int ih, int iw, int op, const int* dev_ops, int inverse,
                       float count, hipStream_t stream) {
  const bool tr = dihedral_bits(op) & 4;                       // (dev_ops: square planes, either way the same shape)
  const int oh = tr ? iw : ih, ow = tr ? ih : iw;
  const int tiles_i = (oh + kDTile - 1) / kDTile, tiles_j = (ow + kDTile - 1) / kDTile;
  const size_t blocks = (size_t)planes * tiles_i * tiles_j;
  if (blocks == 0) return hipSuccess;
  if (blocks >= ((size_t)1 << 31)) return hipErrorInvalidValue;
  // the 16-byte reads: every source row starts 16-byte aligned, and so does every run of 4 (iw % 4 == 0, base aligned)
  const bool wide = iw % 4 == 0 && reinterpret_cast<uintptr_t>(in) % 16 == 0;
  const dim3 grid((unsigned)blocks), block(256);
  if (wide)
    hipLaunchKernelGGL((dihedral_kernel<MODE, true>), grid, block, 0, stream, in, out, ih, iw, oh, ow, tiles_i, tiles_j, op, dev_ops, c,
                       inverse, count);
  else
    hipLaunchKernelGGL((dihedral_kernel<MODE, false>), grid, block, 0, stream, in, out, ih, iw, oh, ow, tiles_i, tiles_j, op, dev_ops, c,
                       inverse, count);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_dihedral(const float* in, float* out, int n, int c, int ih, int iw, int op, const int* dev_ops, bool inverse,
                           hipStream_t stream) {
  return launch_mode<kDStore>(in, out, n * c, c, ih, iw, inverse ? dihedral_inverse(op) : (op & 7), dev_ops, inverse ? 1 : 0, 1.f, stream);
}

hipError_t launch_dihedral_accumulate(const float* in, float* acc, int n, int c, int h, int w, int op, int count, hipStream_t stream) {
  // in = D_op of something shaped like acc: (w, h) planes for a transposing op
  const bool tr = dihedral_bits(op) & 4;
  const int ih = tr ? w : h, iw = tr ? h : w;
  const int inv = dihedral_inverse(op);
  if (count > 0) return launch_mode<kDAddFinish>(in, acc, n * c, c, ih, iw, inv, nullptr, 0, (float)count, stream);
  return launch_mode<kDAdd>(in, acc, n * c, c, ih, iw, inv, nullptr, 0, 1.f, stream);
}

}  // namespace dsen2
