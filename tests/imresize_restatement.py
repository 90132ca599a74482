"""Plain-numpy restatement of the reference's imresize (utils/imresize.py) — the checker of the GPU resampler.

Two passes, one per image axis, the axis with the smaller scale first (stable argsort); per output the taps are multiplied and
added SEQUENTIALLY in float64, in the order of the tap table, starting from the first product; the value between the passes and
the result stay float64.  Vectorised over everything but the taps, so a whole 600 x 600 x 6 image takes milliseconds where the
reference's double Python loop takes seconds.  tests/golden/make_golden_imresize.py asserts at generation time that this equals
the reference's own function bit for bit wherever numpy adds an output's taps sequentially (fewer than 8 taps, or two or more
bands), and within `bound` elsewhere.  Nothing under dsen2_amd/ imports this file; the taps come from dsen2_amd.imresize's host
builder, which the fixtures pin separately.
"""
import numpy as np

from dsen2_amd.imresize import contributions, plan

EPS = 2.0 ** -53


def resize_axis(x, axis, weights, indices, err=None):
    """x [H, W, C] (any dtype) -> (float64 result, sum_k |w_k x_k| per output, propagated error bound or None)."""
    x = np.moveaxis(np.asarray(x), axis, 0)
    col = lambda k: weights[:, k].reshape((-1,) + (1,) * (x.ndim - 1))      # noqa: E731
    acc = x[indices[:, 0]].astype(np.float64) * col(0)
    mag = np.abs(acc)
    for k in range(1, weights.shape[1]):
        term = x[indices[:, k]].astype(np.float64) * col(k)
        acc = acc + term
        mag = mag + np.abs(term)
    out_err = None
    if err is not None:
        e = np.moveaxis(err, axis, 0)
        out_err = sum(np.abs(col(k)) * e[indices[:, k]] for k in range(weights.shape[1]))
        out_err = np.moveaxis(out_err, 0, axis)
    return np.moveaxis(acc, 0, axis), np.moveaxis(mag, 0, axis), out_err


def imresize(img, scalar_scale=None, output_shape=None, with_bound=False):
    """float64 result shaped like the reference's (2-D in -> 2-D out).  with_bound: (result, bound) where bound is, per element, how
    far another summation ORDER of the same taps may land: 2 P 2^-53 sum_k |w_k x_k| for each pass (two orders of the same P
    terms differ by at most (P - 1) 2^-53 sum |terms| each from the exact sum, to first order), the first pass's bound carried
    through the second pass's |weights|."""
    img = np.asarray(img)
    flat = img.ndim == 2
    x = img[:, :, None] if flat else img
    size, scale, order = plan(x.shape, scalar_scale, output_shape)
    err = np.zeros(x.shape)
    for axis in order:
        w, i = contributions(x.shape[axis], size[axis], scale[axis])
        x, mag, err = resize_axis(x, axis, w, i, err)
        err = err + 2 * w.shape[1] * EPS * mag
    x = x[:, :, 0] if flat else x
    err = err[:, :, 0] if flat else err
    return (x, err) if with_bound else x


def max_taps(in_shape, scalar_scale=None, output_shape=None):
    size, scale, _ = plan(in_shape, scalar_scale, output_shape)
    return max(contributions(in_shape[k], size[k], scale[k])[0].shape[1] for k in range(2))


def is_sequential_in_numpy(in_shape, scalar_scale=None, output_shape=None):
    """Whether the reference's np.sum adds an output's taps in table order: below 8 taps always; from 8 on only when the reduced
    axis is not the contiguous one, i.e. with two or more bands."""
    bands = in_shape[2] if len(in_shape) == 3 else 1
    return bands >= 2 or max_taps(in_shape, scalar_scale, output_shape) < 8
