"""csrc/dihedral.hip through the C ABI (dsen2_dihedral_nchw, dsen2_dihedral_accumulate) against tests/dihedral_restatement.py, bit
for bit.  Store mode is pure data movement: its data are random uint32 bit patterns viewed as float32 (NaN payloads, denormals,
infinities), compared through integer views.  Shapes: ragged edges narrower and wider than the 32 x 32 tile, one exact tile,
several tiles in both directions, widths that take the 16-byte reads (multiples of 4) and widths that cannot, more than one plane,
and a pointer offset by one float (which takes the 4-byte reads at a width that would otherwise take the wide ones)."""
import ctypes

import numpy as np
import pytest
import torch

import dihedral_restatement as dr
from dsen2_amd import _lib
from dsen2_amd.DSen2Net import _ptr, _stream_ptr, dihedral

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda', 0)
SHAPES = [(3, 5, 7, 9), (2, 1, 1, 5), (2, 3, 32, 32), (1, 2, 31, 33), (1, 2, 33, 65), (1, 1, 64, 96)]


def _bits(shape, seed):
    """Random 32-bit patterns as float32."""
    return np.random.default_rng(seed).integers(0, 2 ** 32, size=shape, dtype=np.uint32).view(np.float32)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _same_bits(got, want):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32, (got.shape, want.shape)
    return np.array_equal(got.view(np.uint32), np.ascontiguousarray(want).view(np.uint32))


@pytest.mark.parametrize('inverse', [False, True], ids=['forward', 'inverse'])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_all_eight_ops_equal_the_restatement(shape, inverse):
    a = _bits(shape, sum(shape))
    x = _dev(a)
    for op in dr.OPS:
        want = dr.inverse(a, op) if inverse else dr.forward(a, op)
        assert _same_bits(dihedral(x, op=op, inverse=inverse), want), (shape, op, inverse)


@pytest.mark.parametrize('shape', [(2, 3, 32, 32), (1, 2, 12, 20)], ids=lambda s: 'x'.join(map(str, s)))
def test_a_view_offset_by_one_float(shape):
    """Input and output both start one float past an allocation's alignment: no 16-byte access may be taken for granted."""
    n, c, h, w = shape
    a = _bits(shape, 11)
    count = a.size
    for op in dr.OPS:
        for inverse in (False, True):
            src = torch.zeros(count + 1, dtype=torch.float32, device=DEV)
            dst = torch.zeros(count + 1, dtype=torch.float32, device=DEV)
            x = src[1:].view(shape)
            x.copy_(_dev(a))
            out_shape = (n, c, w, h) if op & 1 else shape
            out = dst[1:].view(out_shape)
            assert x.data_ptr() % 16 == 4 and out.data_ptr() % 16 == 4 and x.is_contiguous()
            dihedral(x, op=op, inverse=inverse, out=out)
            assert _same_bits(out, dr.inverse(a, op) if inverse else dr.forward(a, op)), (op, inverse)
            assert float(dst[0]) == 0.0 and _same_bits(x, a)


@pytest.mark.parametrize('shape', [(2, 3, 7, 9), (1, 2, 33, 65), (2, 1, 32, 32)], ids=lambda s: 'x'.join(map(str, s)))
def test_inverse_of_forward_is_the_identity(shape):
    a = _bits(shape, 5)
    x = _dev(a)
    for op in dr.OPS:
        assert _same_bits(dihedral(dihedral(x, op=op), op=op, inverse=True), a), op
        assert _same_bits(dihedral(dihedral(x, op=op, inverse=True), op=op), a), op


@pytest.mark.parametrize('p', [5, 32])
def test_per_sample_ops(p):
    n = 9
    a = _bits((n, 3, p, p), p)
    ops = np.array([5, 0, 7, 2, 1, 6, 3, 4, 5], np.int32)
    assert set(ops.tolist()) == set(range(8))
    x = _dev(a)
    turned = dihedral(x, ops=ops)
    assert _same_bits(turned, dr.per_sample(a, ops))
    assert _same_bits(dihedral(x, ops=ops, inverse=True), dr.per_sample(a, ops, inv=True))
    assert _same_bits(dihedral(turned, ops=_dev(ops), inverse=True), a)
    # only the low three bits of a device op are read
    assert _same_bits(dihedral(x, ops=_dev((ops + 8 * np.arange(n)).astype(np.int32))), dr.per_sample(a, ops))


@pytest.mark.parametrize('shape', [(3, 5, 7, 9), (1, 2, 33, 65), (2, 3, 32, 32)], ids=lambda s: 'x'.join(map(str, s)))
def test_add_and_add_and_finish_equal_numpy_float32(shape):
    """acc = acc + D^-1(in), and (acc + D^-1(in)) / count with a correctly rounded fp32 divide: numpy's float32 arithmetic."""
    n, c, h, w = shape
    rng = np.random.default_rng(h * w)
    acc0 = (rng.standard_normal(shape) * np.exp(rng.uniform(-4, 4, shape))).astype(np.float32)
    for op in dr.OPS:
        turned_shape = (n, c, w, h) if op & 1 else shape
        b = (rng.standard_normal(turned_shape) * np.exp(rng.uniform(-4, 4, turned_shape))).astype(np.float32)
        bd = _dev(b)
        for count in (0, 1, 3, 8):
            acc = _dev(acc0)
            with torch.cuda.device(DEV):
                _lib.call('dsen2_dihedral_accumulate', _ptr(bd), _ptr(acc), n, c, h, w, op, count, _stream_ptr(DEV))
            want = (acc0 + dr.inverse(b, op)).astype(np.float32)
            if count:
                want = (want / np.float32(count)).astype(np.float32)
            assert _same_bits(acc, want), (op, count)


def test_refusals_return_the_error_and_leave_the_output_untouched():
    n, c, h, w = 2, 3, 6, 10
    x = _dev(_bits((n, c, h, w), 1))
    sentinel = np.float32(-123.25)
    out = torch.full((n, c, h, w), float(sentinel), dtype=torch.float32, device=DEV)
    ops = _dev(np.zeros(n, np.int32))
    NULL = ctypes.c_void_p(0)
    lib = _lib.load()
    s = _stream_ptr(DEV)

    def refused(code):
        torch.cuda.synchronize()
        assert code == _lib.ERR_INVALID, code
        assert lib.dsen2_last_error()
        assert bool((out == float(sentinel)).all())

    with torch.cuda.device(DEV):
        for op in (-1, 8, 255):
            refused(lib.dsen2_dihedral_nchw(_ptr(x), _ptr(out), n, c, h, w, op, NULL, 0, s))
            refused(lib.dsen2_dihedral_accumulate(_ptr(x), _ptr(out), n, c, h, w, op, 0, s))
        refused(lib.dsen2_dihedral_nchw(_ptr(x), _ptr(out), n, c, h, w, 0, _ptr(ops), 0, s))            # per-sample ops, h != w
        refused(lib.dsen2_dihedral_nchw(NULL, _ptr(out), n, c, h, w, 1, NULL, 0, s))
        refused(lib.dsen2_dihedral_nchw(_ptr(x), NULL, n, c, h, w, 1, NULL, 0, s))
        refused(lib.dsen2_dihedral_accumulate(NULL, _ptr(out), n, c, h, w, 1, 0, s))
        refused(lib.dsen2_dihedral_accumulate(_ptr(x), NULL, n, c, h, w, 1, 0, s))
        refused(lib.dsen2_dihedral_accumulate(_ptr(x), _ptr(out), n, c, h, w, 1, -1, s))
        refused(lib.dsen2_dihedral_nchw(_ptr(x), _ptr(out), 1, 1, 1 << 16, 1 << 15, 1, NULL, 0, s))      # 2^31 elements
        refused(lib.dsen2_dihedral_accumulate(_ptr(x), _ptr(out), 1 << 11, 1 << 10, 1 << 5, 1 << 5, 1, 0, s))
        refused(lib.dsen2_dihedral_nchw(_ptr(x), _ptr(out), n, 0, h, w, 1, NULL, 0, s))
        # the output aliases the input: the same pointer, and a range that overlaps it
        before = out.clone()
        for op in (0, 1, 4):
            assert lib.dsen2_dihedral_nchw(_ptr(out), _ptr(out), n, c, h, w, op, NULL, 0, s) == _lib.ERR_INVALID
            assert lib.dsen2_dihedral_accumulate(_ptr(out), _ptr(out), n, c, h, w, op, 0, s) == _lib.ERR_INVALID
        flat = out.view(-1)
        assert lib.dsen2_dihedral_nchw(_ptr(flat[:h * w * c]), _ptr(flat[h * w:]), 1, c, h, w, 2, NULL, 0, s) == _lib.ERR_INVALID
        torch.cuda.synchronize()
        assert torch.equal(out, before)
        # an empty batch is not an error and launches nothing
        assert lib.dsen2_dihedral_nchw(_ptr(x), _ptr(out), 0, c, h, w, 3, NULL, 0, s) == _lib.OK
        assert lib.dsen2_dihedral_accumulate(_ptr(x), _ptr(out), 0, c, h, w, 3, 8, s) == _lib.OK
        torch.cuda.synchronize()
        assert torch.equal(out, before)
    with pytest.raises(ValueError):
        dihedral(x, op=8)
    with pytest.raises(ValueError):
        dihedral(x, ops=[0, 9])
    with pytest.raises(ValueError):
        dihedral(x, ops=[0, 1])                              # h != w
    with pytest.raises(ValueError):
        dihedral(x)
