"""The bicubic resampler, host side (no GPU): the tap builder against the reference's recorded taps bit for bit, the numpy
restatement against the reference's recorded images, the pass order, the refusals, the C ABI's new symbols and their argument
checks, and the un-fused float64 arithmetic in the ISA."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import imresize_fixtures as ifx  # noqa: E402
import imresize_restatement as rs  # noqa: E402

from dsen2_amd import imresize as ir  # noqa: E402
from dsen2_amd import patches  # noqa: E402


def test_tap_builder_equals_the_reference_taps_bit_for_bit():
    rec = np.load(os.path.join(ifx.GOLDEN, 'imresize_contributions.npz'))
    assert len(rec.files) == 2 * len(ifx.CONTRIB_CASES)
    for n, (in_len, out_len, scale) in enumerate(ifx.CONTRIB_CASES):
        w, i = ir.contributions(in_len, out_len, scale)
        want_w, want_i = rec['w%d' % n], rec['i%d' % n]
        assert w.dtype == np.float64 and i.dtype == np.int32 and w.shape == want_w.shape == i.shape == (out_len, want_w.shape[1]), (in_len, out_len, scale)
        assert w.tobytes() == want_w.tobytes() and np.array_equal(i, want_i), (in_len, out_len, scale)
        assert i.min() >= 0 and i.max() < in_len
    # an image shorter than the taps: indices fold through [0 1 2 2 1 0] more than once
    w, i = ir.contributions(3, 1, 1.0 / 3)
    assert w.shape[1] > 6 and set(i.ravel().tolist()) == {0, 1, 2}


@pytest.mark.parametrize('key', [c[0] for c in ifx.IMAGE_CASES])
def test_restatement_equals_the_reference_images(key):
    _, shape, dtype, scalar_scale, output_shape = [c for c in ifx.IMAGE_CASES if c[0] == key][0]
    want = np.load(os.path.join(ifx.GOLDEN, 'imresize_images.npz'))[key]
    x = ifx.image(key)
    assert x.shape == shape and x.dtype == dtype
    got, bound = rs.imresize(x, scalar_scale, output_shape, with_bound=True)
    assert got.dtype == np.float64 and got.shape == want.shape and got.ndim == x.ndim
    if rs.is_sequential_in_numpy(shape, scalar_scale, output_shape):
        assert got.tobytes() == want.tobytes(), np.abs(got - want).max()
    else:
        # a single band with 8 taps or more: numpy adds them pairwise.  |diff| <= 2 P 2^-53 sum |w x| per pass
        assert rs.max_taps(shape, scalar_scale, output_shape) >= 8
        assert (np.abs(got - want) <= bound).all(), (np.abs(got - want).max(), bound.max())
        assert bound.max() < 1e-9 * max(1.0, np.abs(want).max())


def test_the_pass_with_the_smaller_scale_runs_first():
    assert ir.plan((10, 12, 3), output_shape=(25, 18)) == ([25, 18], [2.5, 1.5], (1, 0))
    assert ir.plan((8, 20, 2), output_shape=(16, 10))[2] == (1, 0)
    assert ir.plan((12, 12, 2), output_shape=(6, 30))[2] == (0, 1)
    assert ir.plan((7, 9), scalar_scale=6) == ([42, 54], [6.0, 6.0], (0, 1))          # equal scales: axis 0 first
    assert ir.plan((9, 8), scalar_scale=1.5)[0] == [14, 12]                            # ceil
    # the bits depend on the order: the recorded case is not what axis 0 first gives
    x = ifx.image('hwc_f32_shape')
    want = np.load(os.path.join(ifx.GOLDEN, 'imresize_images.npz'))['hwc_f32_shape']
    w0, i0 = ir.contributions(10, 25, 2.5)
    w1, i1 = ir.contributions(12, 18, 1.5)
    other = rs.resize_axis(rs.resize_axis(x, 0, w0, i0)[0], 1, w1, i1)[0]
    right = rs.resize_axis(rs.resize_axis(x, 1, w1, i1)[0], 0, w0, i0)[0]
    assert right.tobytes() == want.tobytes() and other.tobytes() != want.tobytes()
    assert np.abs(other - want).max() < 1e-8


def test_refusals_come_before_the_gpu(monkeypatch):
    def no_gpu():
        raise AssertionError('the GPU was asked for')
    monkeypatch.setattr(patches, 'default_device', no_gpu)
    with pytest.raises(TypeError, match='uint8'):
        ir.imresize(np.zeros((8, 8, 3), np.uint8), 2)
    with pytest.raises(TypeError):
        ir.imresize(np.zeros((8, 8, 3), np.int32), 2)
    with pytest.raises(ValueError, match='dimensions'):
        ir.imresize(np.zeros((2, 8, 8, 3), np.float32), 2)
    with pytest.raises(ValueError, match='dimensions'):
        ir.imresize(np.zeros(8, np.float32), 2)
    with pytest.raises(ValueError, match='scalar_scale OR output_shape'):
        ir.imresize(np.zeros((8, 8, 3), np.float32))


def test_c_abi_declares_exports_and_checks_the_new_entries():
    from dsen2_amd import _lib, build
    build.build()
    lib = _lib.load()
    header = open(os.path.join(ROOT, 'include', 'dsen2_hip.h')).read()
    for name in ('dsen2_imresize_axis', 'dsen2_band_errors', 'dsen2_imresize_band_errors', 'dsen2_band_errors_workspace_bytes'):
        assert re.search(r'\bint %s\s*\(' % name, header) and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert re.search(r'#define DSEN2_DTYPE_F64 (\d)', header).group(1) == str(_lib.DTYPE_F64)
    a, b, c, d = (ctypes.c_void_p(0x1000 * k) for k in (1, 2, 3, 4))       # never dereferenced: every call below is refused first

    def refused(fn, *args):
        assert fn(*args) in (_lib.ERR_INVALID, _lib.ERR_WORKSPACE)
        return lib.dsen2_last_error().decode()
    f = lib.dsen2_imresize_axis
    assert 'not supported' in refused(f, a, 3, 8, 8, 3, 0, 16, b, c, 4, d, None)             # uint8 has no code: any other dtype
    assert 'axis 2' in refused(f, a, _lib.DTYPE_F32, 8, 8, 3, 2, 16, b, c, 4, d, None)
    assert 'taps' in refused(f, a, _lib.DTYPE_F32, 8, 8, 3, 0, 16, b, c, 0, d, None)
    assert 'taps' in refused(f, a, _lib.DTYPE_F32, 8, 8, 3, 0, 16, b, c, 257, d, None)
    assert 'too large' in refused(f, a, _lib.DTYPE_U16, 8, 70000, 13, 0, 4000, b, c, 4, d, None)
    refused(f, None, _lib.DTYPE_F32, 8, 8, 3, 0, 16, b, c, 4, d, None)
    refused(f, a, _lib.DTYPE_F32, 8, 8, 3, 0, 16, b, c, 4, None, None)
    n = ctypes.c_size_t(0)
    assert lib.dsen2_band_errors_workspace_bytes(6, ctypes.byref(n)) == _lib.OK and n.value >= 6 * 16
    assert lib.dsen2_band_errors_workspace_bytes(65, ctypes.byref(n)) == _lib.ERR_INVALID
    g = lib.dsen2_band_errors
    assert 'bands' in refused(g, a, _lib.DTYPE_F32, b, _lib.DTYPE_F32, 8, 8, 65, c, 1 << 30, d, None)
    assert 'not supported' in refused(g, a, _lib.DTYPE_U16, b, _lib.DTYPE_F32, 8, 8, 6, c, 1 << 30, d, None)
    assert 'workspace' in refused(g, a, _lib.DTYPE_F32, b, _lib.DTYPE_F64, 8, 8, 6, c, 16, d, None)
    h = lib.dsen2_imresize_band_errors
    assert 'not supported' in refused(h, a, _lib.DTYPE_F64, 8, 8, 3, 1, 16, b, c, 4, d, _lib.DTYPE_U16, c, 1 << 30, d, None)
    assert 'workspace' in refused(h, a, _lib.DTYPE_F64, 8, 8, 3, 1, 16, b, c, 4, d, _lib.DTYPE_F32, c, 0, d, None)


def test_tap_sums_are_not_contracted_in_the_isa(tmp_path):
    """numpy rounds each product and each sum; an FMA rounds once.  This file has no float64 division either, so it may hold no
    v_fma_f64 at all; and nothing may spill."""
    from dsen2_amd import asm_contract, build
    out = str(tmp_path / 'imresize.s')
    subprocess.check_call([build.HIPCC] + [f for f in build.FLAGS if f != '-fPIC'] + ['-S', '--cuda-device-only',
                          os.path.join(build.CSRC, 'imresize.hip'), '-o', out], stderr=subprocess.DEVNULL)
    kernels = asm_contract._kernels(open(out).read())
    assert len([k for k in kernels if 'imresize_axis_kernel' in k]) == 9          # {uint16, float32, float64} x {store, fused x {float32, float64}}
    assert len([k for k in kernels if 'band_errors_kernel' in k]) == 4
    assert len([k for k in kernels if 'fixed_sum_finish_kernel' in k]) == 1
    for name, body in kernels.items():
        assert not any(ln.startswith('v_fma_f64') or ln.startswith('v_fmac_f64') for ln in body), name
        assert not any('scratch_' in ln for ln in body), name
        if 'finish' not in name:
            assert any(ln.startswith('v_mul_f64') for ln in body) and any(ln.startswith('v_add_f64') for ln in body), name


def test_the_product_does_not_import_the_tests_restatement():
    for base, _, files in os.walk(os.path.join(ROOT, 'dsen2_amd')):
        for f in files:
            if f.endswith('.py'):
                text = open(os.path.join(base, f)).read()
                assert 'imresize_restatement' not in text and 'imresize_fixtures' not in text, f
