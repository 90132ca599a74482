"""The memory contract (tests/guarded.py: run_three_ways) of the three launching entry points of the dihedral family:
dsen2_dihedral_nchw, dsen2_dihedral_accumulate and dsen2_model_forward_ensemble.  Guard bands around every tensor, outputs and
the ensemble's workspace poisoned, the workspace passed with exactly the byte count of the library's own size function; every
comparison is on bits.  Shapes: ragged edges on both sides of the 32 x 32 tile, a 1 x 1 image, widths that take the 16-byte
reads and widths that do not."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import dihedral_restatement as dr
from dsen2_amd import _lib, weights
from dsen2_amd.DSen2Net import _ptr, _stream_ptr, s2model
from guarded import run_three_ways

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
F32 = torch.float32
NULL = ctypes.c_void_p(0)
SHAPES = [(1, 1, 1, 1), (2, 3, 7, 9), (1, 2, 33, 65), (2, 1, 36, 32)]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _run(what, call, inputs, outputs, inplace=(), scratch=()):
    def on_device(*tensors):
        with torch.cuda.device(DEV):
            call(*tensors)
    return run_three_ways(on_device, inputs, outputs, inplace, scratch, device=DEV, what=what)


def _lib_call(name, *args):
    _lib.call(name, *(args + (_stream_ptr(DEV),)))


@pytest.mark.parametrize('inverse', [0, 1])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_dihedral_nchw(shape, inverse):
    n, c, h, w = shape
    a = np.random.default_rng(h * w).standard_normal(shape).astype(np.float32)
    for op in dr.OPS:
        out_shape = (n, c, w, h) if op & 1 else shape
        (got,), _ = _run('dihedral op %d inverse %d %r' % (op, inverse, shape), lambda inp, out, _, __: _lib_call(
            'dsen2_dihedral_nchw', _ptr(inp[0]), _ptr(out[0]), n, c, h, w, op, NULL, inverse), [_dev(a)], [(out_shape, F32)])
        assert np.array_equal(got.cpu().numpy(), dr.inverse(a, op) if inverse else dr.forward(a, op))


@pytest.mark.parametrize('p', [5, 33])
def test_dihedral_nchw_per_sample_ops(p):
    n, c = 9, 2
    a = np.random.default_rng(p).standard_normal((n, c, p, p)).astype(np.float32)
    ops = np.array([5, 0, 7, 2, 1, 6, 3, 4, 5], np.int32)
    for inverse in (0, 1):
        (got,), _ = _run('dihedral per-sample ops %d inverse %d' % (p, inverse), lambda inp, out, _, __: _lib_call(
            'dsen2_dihedral_nchw', _ptr(inp[0]), _ptr(out[0]), n, c, p, p, 0, _ptr(inp[1]), inverse), [_dev(a), _dev(ops)],
            [((n, c, p, p), F32)])
        assert np.array_equal(got.cpu().numpy(), dr.per_sample(a, ops, inv=bool(inverse)))


@pytest.mark.parametrize('count', [0, 8])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_dihedral_accumulate(shape, count):
    n, c, h, w = shape
    rng = np.random.default_rng(h + w)
    acc = rng.standard_normal(shape).astype(np.float32)
    for op in dr.OPS:
        b = rng.standard_normal((n, c, w, h) if op & 1 else shape).astype(np.float32)
        _, (got,) = _run('accumulate op %d count %d %r' % (op, count, shape), lambda inp, _, io, __: _lib_call(
            'dsen2_dihedral_accumulate', _ptr(inp[0]), _ptr(io[0]), n, c, h, w, op, count), [_dev(b)], [], inplace=[_dev(acc)])
        want = acc + dr.inverse(b, op)
        assert np.array_equal(got.cpu().numpy(), want / np.float32(count) if count else want)


NETS = [((4, 6), 2, 128), ((4, 6, 2), 1, 256)]


@functools.lru_cache(maxsize=None)
def _model(bands, d, feat, precision):
    m = s2model(tuple((c, None, None) for c in bands), num_layers=d, feature_size=feat, device=DEV, precision=precision)
    m.set_weights_flat(weights.random_he_uniform(sum(bands), bands[-1], d, feat, seed=1, bias_scale=0.05))
    return m


@pytest.mark.parametrize('mask', [255, 0x11, 8, 1])
@pytest.mark.parametrize('n,h,w', [(1, 1, 1), (3, 21, 37), (2, 32, 32)])
@pytest.mark.parametrize('bands,d,feat', NETS)
@pytest.mark.parametrize('precision', ['fp32', 'bf16', 'bf16x3'])
def test_forward_ensemble(precision, bands, d, feat, n, h, w, mask):
    m = _model(bands, d, feat, precision)
    rng = np.random.default_rng([n, h, w])
    xs = [_dev(rng.uniform(0.0, 0.5, (n, c, h, w)).astype(np.float32)) for c in bands]
    size = ctypes.c_size_t(0)
    _lib.call('dsen2_model_ensemble_workspace_bytes', m._handle, n, h, w, mask, ctypes.byref(size))

    def call(inp, out, _, scr):
        _lib_call('dsen2_model_forward_ensemble', m._handle, _ptr(inp[0]), _ptr(inp[1]), _ptr(inp[2]), _ptr(out[0]), n, h, w, mask,
                  _ptr(scr[0]), scr[0].numel())
    _run('ensemble %s %r d=%d F=%d %dx%dx%d mask %#x' % (precision, bands, d, feat, n, h, w, mask), call,
         xs + [None] * (3 - len(xs)), [((n, m.cout, h, w), F32)], scratch=[size.value])
