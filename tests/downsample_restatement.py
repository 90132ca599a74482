"""Plain-numpy restatement of the reference's downPixelAggr (utils/patches.py:353-371) — the checker of the GPU kernel.

scipy.ndimage.gaussian_filter(band, 1 / SCALE) + skimage.measure.block_reduce(band, (SCALE, SCALE), np.mean), written out
operation by operation (scipy 1.7.1's symmetric correlate1d, `reflect` boundary, output in the INPUT's dtype after each axis).
tests/golden/make_golden_trainset.py asserts at generation time that this equals the reference's own function in every value on
both bundled tiles (uint16 and float32, SCALE 2 and 6).  Nothing under dsen2_amd/ imports this file.

numpy's exp differs in the last bit between builds (AVX-512 kernel or libm), so `gaussian_weights` is only the reference's
weights under the reference's numpy; the tests hand down_pixel_aggr the RECORDED weights (golden/trainset_weights.npz).
"""
import numpy as np


def gaussian_weights(scale):
    """(weights float64 [2 * radius + 1], radius) of scipy's gaussian_filter1d(sigma=1/scale, truncate=4.0)."""
    sigma = 1.0 / scale
    radius = int(4.0 * sigma + 0.5)
    x = np.arange(-radius, radius + 1)
    w = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    return w / w.sum(), radius


def _filter_axis0(a, w, radius):
    """Symmetric correlate1d along axis 0 of `a`, float64 arithmetic in scipy's order, cast to a.dtype (uint16: truncation)."""
    n = a.shape[0]
    p = np.pad(a, [(radius, radius)] + [(0, 0)] * (a.ndim - 1), mode='symmetric').astype(np.float64)
    tmp = p[radius:radius + n] * w[radius]
    for ii in range(-radius, 0):
        tmp = tmp + (p[radius + ii:radius + ii + n] + p[radius - ii:radius - ii + n]) * w[ii + radius]
    return tmp.astype(a.dtype)


def recorded_weights(scale):
    """The weights scipy built when the fixtures were recorded (SCALE 2 and 6)."""
    import os
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'trainset_weights.npz'))
    return z['s%d' % scale], (z['s%d' % scale].shape[0] - 1) // 2


def down_pixel_aggr(img, scale=2, weights=None):
    """float64 [H/scale, W/scale(, C)], squeezed like the reference's.  weights: (w, radius), default gaussian_weights(scale)."""
    img = np.asarray(img)
    if img.ndim == 2:
        img = img[:, :, None]
    h, w_, c = img.shape
    if h % scale or w_ % scale:
        raise ValueError('image %d x %d is not a multiple of the scale %d' % (h, w_, scale))
    w, radius = weights if weights is not None else gaussian_weights(scale)
    if radius > min(h, w_):
        raise ValueError('radius larger than the image')
    v = _filter_axis0(img, w, radius)
    v = _filter_axis0(v.transpose(1, 0, 2), w, radius).transpose(1, 0, 2)
    blocks = v.astype(np.float64).reshape(h // scale, scale, w_ // scale, scale, c)
    total = np.zeros((h // scale, w_ // scale, c))
    for dy in range(scale):                      # row-major inside a block, as the kernel adds
        for dx in range(scale):
            total = total + blocks[:, dy, :, dx, :]
    return np.squeeze(total / float(scale * scale))
