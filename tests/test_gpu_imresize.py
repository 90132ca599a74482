"""The bicubic resampler on the GPU: the kernel against the reference's recorded outputs and against the numpy restatement —
EQUALITY of float64 bits wherever the arithmetic is specified operation by operation (every enlargement, every image with two
or more bands), and the derived summation-order bound for single-band reductions with 8 taps or more, where numpy itself adds
pairwise.  Nothing here reads the reference tree: its outputs are the fixtures of tests/golden/make_golden_imresize.py."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import imresize_fixtures as ifx  # noqa: E402
import imresize_restatement as rs  # noqa: E402

from dsen2_amd import patches  # noqa: E402
from dsen2_amd.imresize import imresize, imresize_device  # noqa: E402

pytestmark = pytest.mark.gpu


def _same(got, want, what):
    """float64 arrays equal in their BITS (tests/bits.py is the float32 form of this)."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype == np.float64 and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    bad = got.view(np.uint64) != want.view(np.uint64)
    if bad.any():
        first = tuple(np.argwhere(bad)[0])
        raise AssertionError('%s: %d of %d values differ in their bits, first at %s: %r != %r (max |diff| %g)' % (
            what, int(bad.sum()), bad.size, list(first), got[first], want[first], np.abs(got - want).max()))


@pytest.mark.parametrize('key', [c[0] for c in ifx.IMAGE_CASES])
def test_kernel_equals_the_reference_images(key):
    _, shape, dtype, scalar_scale, output_shape = [c for c in ifx.IMAGE_CASES if c[0] == key][0]
    want = np.load(os.path.join(ifx.GOLDEN, 'imresize_images.npz'))[key]
    x = ifx.image(key)
    got = imresize(x, scalar_scale=scalar_scale, output_shape=output_shape)
    assert got.ndim == x.ndim                                            # 2-D in -> 2-D out
    mine, bound = rs.imresize(x, scalar_scale, output_shape, with_bound=True)
    _same(got, mine, key + ' (restatement)')                             # the kernel adds sequentially whatever the shape
    if rs.is_sequential_in_numpy(shape, scalar_scale, output_shape):
        _same(got, want, key)
    else:
        diff = np.abs(got - want)
        print('%s: max |diff| %.3g, smallest bound %.3g' % (key, diff.max(), bound.min()))
        assert (diff <= bound).all(), (key, diff.max(), bound.max())


@pytest.mark.parametrize('tile', ifx.TILES)
def test_kernel_equals_the_reference_on_the_bundled_tiles(tile):
    rec = np.load(os.path.join(ifx.GOLDEN, 'imresize_tile_%s.npz' % tile))
    for key, x, scale in ifx.tile_cases(tile):
        out = imresize(x, scale)
        assert out.shape == (600, 600, x.shape[2])
        for part, v in ifx.edge_views(out).items():
            _same(v, rec['%s_%s' % (key, part)], '%s %s %s' % (tile, key, part))
        _same(out, rs.imresize(x, scale), '%s %s whole (restatement)' % (tile, key))
        # the same from float32 and float64 copies of the raster: uint16 converts exactly
        _same(imresize(x.astype(np.float32), scale), out, '%s %s float32' % (tile, key))
        _same(imresize(x.astype(np.float64), scale), out, '%s %s float64' % (tile, key))


@pytest.mark.parametrize('shape, dtype, kwargs', [
    ((40, 52, 1), np.float32, {'scalar_scale': 2}), ((40, 52, 6), np.uint16, {'scalar_scale': 2}), ((23, 31, 13), np.float32, {'scalar_scale': 6}),
    ((3, 5), np.float64, {'scalar_scale': 2}), ((3, 5, 2), np.uint16, {'scalar_scale': 6}), ((3, 5, 4), np.float32, {'scalar_scale': 1.0 / 3}),
    ((33, 20, 6), np.float32, {'scalar_scale': 1.5}), ((33, 20), np.uint16, {'scalar_scale': 1.5}),
    ((30, 44, 3), np.float64, {'output_shape': (75, 66)}), ((30, 44, 5), np.uint16, {'output_shape': (90, 22)}),
    ((64, 48, 2), np.float32, {'output_shape': (16, 96)}), ((120, 90, 13), np.uint16, {'scalar_scale': 0.5}),
    ((96, 60, 1), np.float32, {'scalar_scale': 1.0 / 6}), ((300, 7, 6), np.float32, {'scalar_scale': 2}), ((7, 300, 6), np.float64, {'scalar_scale': 6})])
def test_kernel_equals_the_restatement_at_other_shapes(shape, dtype, kwargs):
    """1, 6 and 13 channels, a 3 x 5 image (taps that reflect more than once), scale 1.5, one scale per axis in both pass orders,
    reductions, uint16 input, images far narrower than a workgroup.  Sequential sums on both sides: equality, whatever the shape."""
    rng = np.random.RandomState(shape[0] * 131 + shape[1])
    x = rng.randint(0, 65536, size=shape).astype(dtype)
    if dtype != np.uint16:
        x += rng.random_sample(shape).astype(dtype)
    _same(imresize(x, **kwargs), rs.imresize(x, **kwargs), '%r %s %r' % (shape, np.dtype(dtype).name, kwargs))


def test_device_entry_dtypes_and_refusals():
    x = np.random.RandomState(4).randint(0, 9000, size=(20, 24, 4)).astype(np.uint16)
    t, dt = patches.upload_raster(x)
    out = imresize_device(t, 2)
    assert out.is_cuda and out.dtype == torch.float64 and tuple(out.shape) == (40, 48, 4)
    _same(out.cpu().numpy(), rs.imresize(x, 2), 'device uint16')
    band = imresize_device(torch.from_numpy(x[:, :, 0].astype(np.float32)).cuda(), output_shape=(30, 30))
    assert tuple(band.shape) == (30, 30)
    _same(band.cpu().numpy(), rs.imresize(x[:, :, 0].astype(np.float32), output_shape=(30, 30)), 'device 2-D')
    # a non-contiguous view is resampled as the image it shows
    view = torch.from_numpy(x.astype(np.float32)).cuda()[::2, 1::3]
    _same(imresize_device(view, 2).cpu().numpy(), rs.imresize(x.astype(np.float32)[::2, 1::3], 2), 'view')
    with pytest.raises(TypeError, match='uint8'):
        imresize_device(torch.zeros((8, 8, 3), dtype=torch.uint8, device='cuda'), 2)
    with pytest.raises(TypeError):
        imresize_device(torch.zeros((8, 8, 3), dtype=torch.int32, device='cuda'), 2)
    with pytest.raises(ValueError):
        imresize_device(torch.zeros((8, 8, 3), device='cuda'))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        imresize_device(torch.zeros((8, 8, 3)), 2)


def test_kernel_at_full_tile_size_is_deterministic_and_right():
    """The six 20 m bands of a whole tile, 5490 x 5490 x 6 float32, enlarged by 2: two runs give the same bits, and three windows
    (a corner on the image border, the interior, the opposite corner) equal the restatement.  At scale 2 the taps of an output do
    not depend on where a crop starts (u = x / 2 + 0.25 is exact), so a crop with a margin is resampled to the same bits."""
    n, scale = 5490, 2
    g = torch.Generator(device='cuda').manual_seed(20170725)
    img = torch.randint(0, 12000, (n, n, 6), device='cuda', generator=g).to(torch.float32)
    a = imresize_device(img, scale)
    b = imresize_device(img, scale)
    assert tuple(a.shape) == (n * scale, n * scale, 6) and a.dtype == torch.float64 and torch.equal(a, b)
    del b
    on, m, k = n * scale, 8, 48                          # m: output pixels of margin that hide the crop's own reflection
    for oy, ox in ((0, 0), (on // 2 - 6, on // 3 + 4), (on - k, on - k)):
        y0, y1, x0, x1 = max(oy - m, 0), min(oy + k + m, on), max(ox - m, 0), min(ox + k + m, on)
        assert y0 % scale == 0 and y1 % scale == 0 and x0 % scale == 0 and x1 % scale == 0
        crop = img[y0 // scale:y1 // scale, x0 // scale:x1 // scale].cpu().numpy()
        want = rs.imresize(crop, scale)[oy - y0:oy - y0 + k, ox - x0:ox - x0 + k]
        _same(a[oy:oy + k, ox:ox + k].cpu().numpy(), np.ascontiguousarray(want), 'window (%d, %d)' % (oy, ox))
