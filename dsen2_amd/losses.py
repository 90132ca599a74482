"""The losses a compiled S2Model minimises and the no-data mask (include/dsen2_hip.h, "losses and the no-data mask"), as the host
states them: the names compile() and train.py accept, the (kind, param, mask_mode) triple of dsen2_model_set_loss, and ONE float64
numpy statement of the loss table, which evaluate(), the sharded evaluation and fit's host-array validation all use.

    kind          rho(d)                                rho'(d)
    MAE           |d|                                   sign(d), sign(0) = 0
    MSE           d*d                                   2*d
    Huber(delta)  |d| <= delta: 0.5*(d*d)               d
                  otherwise:    delta*(|d| - 0.5*delta) delta*sign(d)
    Charbonnier   s = sqrt(d*d + eps*eps)               d / s

The mask: a pixel (sample, y, x) whose target is exactly 0 in every band carries no ground truth ((y != 0).any(axis=1): -0.0 is 0,
NaN and negative values are data).  It adds nothing to either sum; the denominator stays the number of ALL elements.
"""
import numpy as np

MAE, MSE, HUBER, CHARBONNIER = 0, 1, 2, 3
KINDS = {'mean_absolute_error': MAE, 'mae': MAE, 'mean_squared_error': MSE, 'mse': MSE, 'huber': HUBER, 'charbonnier': CHARBONNIER}
SHORT = {MAE: 'mae', MSE: 'mse', HUBER: 'huber', CHARBONNIER: 'charbonnier'}
MASK_NONE, MASK_NODATA = 0, 1
DEFAULT = (MAE, 0.0, MASK_NONE)


def parse(loss, loss_param=None, mask_nodata=False):
    """(kind, param, mask_mode) of compile(loss=, loss_param=, mask_nodata=); ValueError for anything it does not accept.  param is
    the float32 value that crosses the C ABI (0.0 for the kinds without one)."""
    kind = KINDS.get(loss) if isinstance(loss, str) else None
    if kind is None:
        raise ValueError("loss must be one of %s, got %r" % (', '.join(repr(k) for k in KINDS), loss))
    if kind in (HUBER, CHARBONNIER):
        if loss_param is None:
            raise ValueError('loss=%r needs loss_param (%s): errors live in the reflectance / 2000 domain, where no default fits'
                             % (loss, 'delta' if kind == HUBER else 'epsilon'))
        param = float(np.float32(loss_param))
        if not np.isfinite(param) or not param > 0.0:
            raise ValueError('loss_param must be a finite float32 > 0, got %r' % (loss_param,))
    else:
        if loss_param is not None:
            raise ValueError('loss=%r takes no loss_param (got %r)' % (loss, loss_param))
        param = 0.0
    return kind, param, MASK_NODATA if mask_nodata else MASK_NONE


def describe(setting):
    kind, param, mask = setting
    return SHORT[kind] + ('(%g)' % param if kind in (HUBER, CHARBONNIER) else '') + (', no-data pixels masked' if mask else '')


def rho(d, kind, param):
    """rho of the table above on a float64 array of errors, every operation rounded on its own (numpy has no FMA)."""
    d = np.asarray(d, np.float64)
    p = float(np.float32(param))
    if kind == MAE:
        return np.abs(d)
    if kind == MSE:
        return d * d
    if kind == HUBER:
        a = np.abs(d)
        return np.where(a <= p, 0.5 * (d * d), p * (a - 0.5 * p))
    if kind == CHARBONNIER:
        return np.sqrt(d * d + p * p)
    raise ValueError('loss kind %r unknown' % (kind,))


def slope(d, kind, param):
    """rho' of the table above on a float64 array of errors."""
    d = np.asarray(d, np.float64)
    p = float(np.float32(param))
    sgn = (d > 0).astype(np.float64) - (d < 0).astype(np.float64)
    if kind == MAE:
        return sgn
    if kind == MSE:
        return 2.0 * d
    if kind == HUBER:
        return np.where(np.abs(d) <= p, d, p * sgn)
    if kind == CHARBONNIER:
        return d / np.sqrt(d * d + p * p)
    raise ValueError('loss kind %r unknown' % (kind,))


def valid_pixels(y):
    """[n, 1, h, w] bool: the pixels of an NCHW target that carry ground truth."""
    return (np.asarray(y) != 0).any(axis=1, keepdims=True)


def terms(pred, y, setting):
    """(rho, d*d) per element of an NCHW pair in float64, masked elements 0.0: d = float64(pred) - float64(y)."""
    kind, param, mask = setting
    d = np.asarray(pred).astype(np.float64) - np.asarray(y).astype(np.float64)
    r, q = rho(d, kind, param), d * d
    if mask == MASK_NODATA:
        v = valid_pixels(y)
        r, q = np.where(v, r, 0.0), np.where(v, q, 0.0)
    return r, q


# ---- the summation order of dsen2_loss_sums, for the settings that are not the default -------------------------------------------
# The default (MAE, unmasked) keeps np.mean / np.sum: the bits every earlier run has.  Any other setting is summed in the order
# the device validation pass uses (csrc/error_sums.hip: blocks = clamp(ceil(count / 2048), 1, 4096) workgroups of 256 threads, a
# thread adds its elements i, i + blocks * 256, ... in index order, a halving tree per workgroup, the partials added the same
# way by one workgroup), so that validating a chunk from host arrays and on the device gives one number, not two that differ
# in the last place.  Every term is >= +0.0, so the zeros of masked elements and of the padding change no bit.
_THREADS, _PER_THREAD, _MAX_BLOCKS = 256, 8, 4096


def _tree(s):
    s = s.copy()
    half = _THREADS // 2
    while half > 0:
        s[:, :half] = s[:, :half] + s[:, half:2 * half]
        half //= 2
    return s[:, 0]


def _strided(values, lanes):
    v = np.concatenate([values, np.zeros(-values.size % lanes)]).reshape(-1, lanes)
    acc = np.zeros(lanes)
    for row in v:
        acc = acc + row
    return acc


def fixed_order_sum(values):
    values = np.asarray(values, np.float64).ravel()
    blocks = min(max(-(-values.size // (_THREADS * _PER_THREAD)), 1), _MAX_BLOCKS)
    partials = _tree(_strided(values, blocks * _THREADS).reshape(blocks, _THREADS))
    return float(_tree(_strided(partials, _THREADS).reshape(1, _THREADS))[0])


def host_sums(pred, y, setting=DEFAULT):
    """(sum rho, sum d*d, elements) in float64 over an NCHW pair; `elements` counts masked ones too (the denominator)."""
    r, q = terms(pred, y, setting)
    if tuple(setting) == DEFAULT:
        return float(np.sum(r)), float(np.sum(q)), float(r.size)
    return fixed_order_sum(r), fixed_order_sum(q), float(r.size)


def host_loss(pred, y, setting=DEFAULT):
    """[loss, mean_squared_error] over an NCHW pair."""
    if tuple(setting) == DEFAULT:
        r, q = terms(pred, y, setting)
        return [float(np.mean(r)), float(np.mean(q))]
    sr, sq, cnt = host_sums(pred, y, setting)
    return [float(sr / cnt), float(sq / cnt)]
