"""numpy restatement of what the training step's input-gradient path does outside its convolution kernels
(dsen2_amd/csrc/capi_train.hip, train_ops.hip), the yardstick of tests/test_dgrad_host.py, tests/test_gpu_dgrad.py and
tests/test_gpu_backward_chain.py.  Written from the definitions in the file comment of capi_train.hip, not from the kernels:

  flip_hwio      the kernel of a dgrad convolution: W'[ky, kx, c, o] = W[2 - ky, 2 - kx, o, c] (HWIO in, HWIO out, the roles of
                 the two channel axes exchanged); pad_in=16: the output layer's form, whose `co` real gradient channels are
                 zero-padded to the 16 input lanes of the 16 -> F tile kernel
  mask_split3    du of the bf16x3 step: x = (t_hi + t_lo > 0) ? v : 0, h = bf16_rne(x), l = bf16_rne(x - h).  NOT split3_f32's
                 split, whose hi plane is (u + 0x8000) >> 16 (ties away)
  mask_round16   du of the mixed-precision step: bf16_rne((t > 0) ? v : 0)
  to_blocked / from_blocked / planes_to_values / values_to_planes
                 between NHWC arrays and the blocked 16-bit layouts [n, (2,) c/8, h, w, 8] of the bf16 kernels

bf16 numbers travel as uint16 bit patterns.  The product must never import this file."""
import numpy as np

from amp_bf16_restatement import bf16_rne_bits


def flip_hwio(k, pad_in=None):
    """(3, 3, ci, co) -> (3, 3, co, ci): W'[ky, kx, c, o] = W[2 - ky, 2 - kx, o, c].  pad_in: the `co` input channels of the result
    zero-padded to pad_in lanes, (3, 3, pad_in, ci)."""
    k = np.asarray(k)
    assert k.ndim == 4 and k.shape[:2] == (3, 3), k.shape
    ci, co = k.shape[2:]
    lanes = co if pad_in is None else int(pad_in)
    assert lanes >= co, (lanes, co)
    out = np.zeros((3, 3, lanes, ci), k.dtype)
    for ky in range(3):
        for kx in range(3):
            out[ky, kx, :co, :] = k[2 - ky, 2 - kx].T
    return out


def bf16_value(bits):
    """uint16 bf16 bit patterns -> their float32 values."""
    return (np.asarray(bits, np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def _f32_bits(x):
    x = np.ascontiguousarray(x)
    assert x.dtype == np.float32, x.dtype
    return x.view(np.uint32)


def mask_split3(v, t_hi, t_lo):
    """v: float32 values; t_hi, t_lo: float32 VALUES of the two bf16 planes of t (same shape).  Returns the (hi, lo) planes of du as
    uint16 bit patterns: x = v where t_hi + t_lo > 0 (a float32 sum), else +0; hi = bf16_rne(x); lo = bf16_rne(x - hi) (the
    float32 difference, which is exact)."""
    v, t_hi, t_lo = (np.asarray(a, np.float32) for a in (v, t_hi, t_lo))
    x = np.where((t_hi + t_lo) > np.float32(0), v, np.float32(0)).astype(np.float32)
    h = bf16_rne_bits(_f32_bits(x))
    rest = (x - bf16_value(h)).astype(np.float32)
    return h, bf16_rne_bits(_f32_bits(rest))


def mask_round16(v, t):
    """v: float32 values; t: float32 VALUES of the bf16 tensor t.  Returns bf16_rne(v where t > 0 else +0) as uint16 bit patterns."""
    v, t = np.asarray(v, np.float32), np.asarray(t, np.float32)
    return bf16_rne_bits(_f32_bits(np.where(t > np.float32(0), v, np.float32(0)).astype(np.float32)))


# ---- layouts ----
def to_blocked(x_nhwc):
    """[n, h, w, c] -> [n, c/8, h, w, 8] (any dtype)."""
    x = np.asarray(x_nhwc)
    n, h, w, c = x.shape
    assert c % 8 == 0, c
    return np.ascontiguousarray(x.reshape(n, h, w, c // 8, 8).transpose(0, 3, 1, 2, 4))


def from_blocked(x_blk):
    """[n, c/8, h, w, 8] -> [n, h, w, c]."""
    x = np.asarray(x_blk)
    n, b, h, w, e = x.shape
    assert e == 8, e
    return np.ascontiguousarray(x.transpose(0, 2, 3, 1, 4).reshape(n, h, w, b * 8))


def planes_to_values(planes):
    """A blocked 16-bit tensor (int16 / uint16 bit patterns) -> float32 NHWC values: [n, c/8, h, w, 8] gives one array,
    [n, 2, c/8, h, w, 8] the pair (plane 0, plane 1)."""
    p = np.ascontiguousarray(planes).view(np.uint16)
    if p.ndim == 5:
        return bf16_value(from_blocked(p))
    assert p.ndim == 6 and p.shape[1] == 2, p.shape
    return bf16_value(from_blocked(p[:, 0])), bf16_value(from_blocked(p[:, 1]))


def values_to_planes(hi_bits, lo_bits=None):
    """uint16 NHWC bit patterns -> the blocked int16 tensor: [n, c/8, h, w, 8], or with lo_bits [n, 2, c/8, h, w, 8]."""
    hi = to_blocked(np.asarray(hi_bits, np.uint16))
    if lo_bits is None:
        return hi.view(np.int16)
    lo = to_blocked(np.asarray(lo_bits, np.uint16))
    return np.ascontiguousarray(np.stack([hi, lo], axis=1)).view(np.int16)
