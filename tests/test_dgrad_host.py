"""tests/dgrad_restatement.py against statements that owe nothing to this project (no GPU): the flipped, transposed dgrad kernel
against torch autograd in float64; the two mask-and-round definitions against torch's own bfloat16 conversion, on values that
tell round-to-nearest-even from the ties-away rounding of a residual stream's hi plane; the layout helpers against each other.
This is what lets tests/test_gpu_dgrad.py and tests/test_gpu_backward_chain.py trust a flip written in the tests."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import dgrad_restatement as R  # noqa: E402

conv2d = torch.nn.functional.conv2d


def _oihw(k_hwio):
    return torch.from_numpy(np.ascontiguousarray(k_hwio)).permute(3, 2, 0, 1).contiguous()


# (ci, co, pad_in): the body layers of both feature sizes; the output layer at every kind of Cout (6, 2: the Sentinel-2 models; 1
# and 15: the ends of what a model may have), its gradient zero-padded to the 16 lanes of the 16 -> F kernel
FLIP_CASES = [(128, 128, None), (256, 256, None), (128, 6, 16), (128, 2, 16), (128, 1, 16), (128, 15, 16)]


@pytest.mark.parametrize('ci,co,pad_in', FLIP_CASES)
def test_conv_with_the_flipped_kernel_is_autograds_input_gradient(ci, co, pad_in):
    """float64, a ragged 5 x 7 image, zero padding: conv2d(g, flip_hwio(W)) == d/dx <conv2d(x, W), g>, to 1e-12 relative."""
    rng = np.random.default_rng(ci + co)
    n, h, w = 2, 5, 7
    k = rng.standard_normal((3, 3, ci, co))
    x = torch.from_numpy(rng.standard_normal((n, ci, h, w))).requires_grad_(True)
    g = rng.standard_normal((n, co, h, w))
    y = conv2d(x, _oihw(k), padding=1)
    want, = torch.autograd.grad(y, x, torch.from_numpy(g))
    kf = R.flip_hwio(k, pad_in=pad_in)
    lanes = co if pad_in is None else pad_in
    assert kf.shape == (3, 3, lanes, ci) and kf.dtype == k.dtype
    gp = np.zeros((n, lanes, h, w))
    gp[:, :co] = g
    got = conv2d(torch.from_numpy(gp), _oihw(kf), padding=1)
    err = float((got - want).abs().max() / want.abs().max())
    print('flip %d -> %d (pad_in %r): max |error| / max |gradient| = %.2e' % (ci, co, pad_in, err))
    assert got.shape == want.shape and err <= 1e-12


@pytest.mark.parametrize('ci,co,pad_in', FLIP_CASES)
def test_the_flip_is_its_own_inverse(ci, co, pad_in):
    """flip_hwio(flip_hwio(k)) == k; the padded form gives k back in its first `co` lanes and zeros above; the padding lanes of
    the flipped kernel itself are zero."""
    k = np.random.default_rng(3).standard_normal((3, 3, ci, co)).astype(np.float32)
    kf = R.flip_hwio(k, pad_in=pad_in)
    back = R.flip_hwio(kf)
    assert np.array_equal(back[..., :co], k)
    assert not back[..., co:].any() and not kf[:, :, co:, :].any()
    assert back.shape == (3, 3, ci, co if pad_in is None else pad_in)
    # every element of k appears exactly once, where the definition says
    for ky, kx, c, o in ((0, 0, 0, 0), (0, 2, co - 1, 0), (2, 1, 0, ci - 1), (1, 1, co // 2, ci // 3), (1, 0, co - 1, ci - 1)):
        assert kf[ky, kx, c, o] == k[2 - ky, 2 - kx, o, c]


def _interesting_values(shape, seed):
    """float32 values over many binades, with exact bf16 ties (low half 0x8000: even and odd neighbours), exact bf16 numbers, zeros
    and -0.0 among them."""
    rng = np.random.default_rng(seed)
    v = (rng.standard_normal(shape) * np.exp(rng.uniform(-8, 8, shape))).astype(np.float32)
    u = v.view(np.uint32).ravel()
    u[0::7] = (u[0::7] & np.uint32(0xffff0000)) | np.uint32(0x8000)      # ties
    u[1::7] = u[1::7] & np.uint32(0xffff0000)                            # exact bf16
    u[2::91] = 0
    u[3::91] = 0x80000000
    return v


def _torch_rne_bits(x):
    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)


def test_mask_round16_is_torchs_bfloat16_of_the_masked_value():
    shape = (2, 3, 5, 16)
    v = _interesting_values(shape, 1)
    t = R.bf16_value(_torch_rne_bits(np.random.default_rng(2).standard_normal(shape).clip(-1, 1)))
    t.ravel()[::5] = 0.0
    t.ravel()[1::17] = -0.0
    got = R.mask_round16(v, t)
    want = _torch_rne_bits(np.where(t > 0, v, np.float32(0)))
    assert got.dtype == np.uint16 and np.array_equal(got, want)
    assert not got[t <= 0].any()                                        # +0 where masked, never -0
    ties = (v.view(np.uint32) & np.uint32(0xffff)) == 0x8000
    from amp_bf16_restatement import bf16_hi_bits
    assert (got[ties & (t > 0)] != bf16_hi_bits(v.view(np.uint32))[ties & (t > 0)]).any(), 'no tie tells the two roundings apart'


def test_mask_split3_is_two_torch_roundings_and_not_the_streams_split():
    shape = (2, 3, 5, 16)
    v = _interesting_values(shape, 4)
    rng = np.random.default_rng(5)
    t_hi = R.bf16_value(_torch_rne_bits(np.maximum(rng.standard_normal(shape), 0)))
    t_lo = R.bf16_value(_torch_rne_bits(rng.standard_normal(shape) * 2.0 ** -9 * t_hi))
    h, l = R.mask_split3(v, t_hi, t_lo)
    x = np.where((t_hi + t_lo) > 0, v, np.float32(0)).astype(np.float32)
    assert np.array_equal(h, _torch_rne_bits(x))
    assert np.array_equal(l, _torch_rne_bits(x - R.bf16_value(h)))
    active = x != 0
    assert 0.2 < active.mean() < 0.8
    # hi + lo carries 16 significant bits of x
    rel = np.abs(R.bf16_value(h)[active].astype(np.float64) + R.bf16_value(l)[active] - x[active]) / np.abs(x[active])
    assert rel.max() <= 2.0 ** -16
    from amp_bf16_restatement import bf16_hi_bits
    assert (h != bf16_hi_bits(x.view(np.uint32))).any(), 'no tie tells the two roundings apart'


def test_layout_helpers_round_trip_and_agree_with_the_definition():
    rng = np.random.default_rng(6)
    a = rng.integers(0, 1 << 16, (2, 3, 5, 24), dtype=np.uint16)
    b = rng.integers(0, 1 << 16, (2, 3, 5, 24), dtype=np.uint16)
    blk = R.to_blocked(a)
    assert blk.shape == (2, 3, 3, 5, 8)
    assert blk[1, 2, 1, 4, 3] == a[1, 1, 4, 2 * 8 + 3]
    assert np.array_equal(R.from_blocked(blk), a)
    one = R.values_to_planes(a)
    two = R.values_to_planes(a, b)
    assert one.dtype == np.int16 and one.shape == (2, 3, 3, 5, 8) and two.shape == (2, 2, 3, 3, 5, 8)
    assert np.array_equal(two[:, 0], one) and np.array_equal(two[:, 1], R.values_to_planes(b))
    # (compared as bit patterns: a NaN pattern must survive too)
    assert np.array_equal(R.planes_to_values(one).view(np.uint32), a.astype(np.uint32) << 16)
    va, vb = R.planes_to_values(two)
    assert np.array_equal(va.view(np.uint32), a.astype(np.uint32) << 16) and np.array_equal(vb.view(np.uint32), b.astype(np.uint32) << 16)
