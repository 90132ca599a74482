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

The SSIM term (compile(ssim_weight=...); include/dsen2_hip.h, "the SSIM loss term"): weight * the mean over ALL windows of (1 - SSIM),
added to the loss above.  With it the setting is (kind, param, mask_mode, (weight, win, sigma, data_range)); without it (weight 0, the
default) the triple as it always was.  Its float64 numpy statement, in the device's operation and summation order, is at the end.
"""
import numpy as np

MAE, MSE, HUBER, CHARBONNIER = 0, 1, 2, 3
KINDS = {'mean_absolute_error': MAE, 'mae': MAE, 'mean_squared_error': MSE, 'mse': MSE, 'huber': HUBER, 'charbonnier': CHARBONNIER}
SHORT = {MAE: 'mae', MSE: 'mse', HUBER: 'huber', CHARBONNIER: 'charbonnier'}
MASK_NONE, MASK_NODATA = 0, 1
SSIM_MIN_WIN, SSIM_MAX_WIN = 3, 11
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


def parse_ssim(setting, ssim_weight=0.0, ssim_win=11, ssim_sigma=1.5, ssim_data_range=5.0):
    """compile(ssim_weight=, ssim_win=, ssim_sigma=, ssim_data_range=) on top of parse()'s triple.  Weight 0 (the default): the triple
    itself, today's object.  Else (kind, param, mask_mode, (weight, win, sigma, data_range)), the weight as the float32 that crosses
    the C ABI; ValueError for anything dsen2_model_set_loss_ssim would refuse (the window is odd, 3..11: 13 and 15 are the
    metrics' alone)."""
    try:
        weight = float(np.float32(ssim_weight))
    except (TypeError, ValueError):
        raise ValueError('ssim_weight must be a finite float32 >= 0, got %r' % (ssim_weight,))
    if not np.isfinite(weight) or weight < 0.0:
        raise ValueError('ssim_weight must be a finite float32 >= 0, got %r' % (ssim_weight,))
    if isinstance(ssim_win, bool) or int(ssim_win) != ssim_win or int(ssim_win) % 2 == 0 or not SSIM_MIN_WIN <= ssim_win <= SSIM_MAX_WIN:
        raise ValueError('ssim_win must be odd and in %d..%d, got %r' % (SSIM_MIN_WIN, SSIM_MAX_WIN, ssim_win))
    sigma, L = float(ssim_sigma), float(ssim_data_range)
    if not (np.isfinite(sigma) and sigma > 0.0):
        raise ValueError('ssim_sigma must be finite and > 0, got %r' % (ssim_sigma,))
    if not (np.isfinite(L) and L > 0.0):
        raise ValueError('ssim_data_range must be finite and > 0, got %r' % (ssim_data_range,))
    ssim = (weight, int(ssim_win), sigma, L)
    window, c1, c2 = ssim_constants(ssim)
    if not (np.isfinite(window).all() and np.isfinite(c1) and np.isfinite(c2) and c1 > 0.0 and c2 > 0.0):
        raise ValueError('ssim_sigma = %r and ssim_data_range = %r do not give a finite window and finite, positive constants'
                         % (ssim_sigma, ssim_data_range))
    return tuple(setting) if weight == 0.0 else tuple(setting[:3]) + (ssim,)


def pointwise(setting):
    """The (kind, param, mask_mode) triple of a setting."""
    return tuple(setting[:3])


def ssim_part(setting):
    """(weight, win, sigma, data_range) of a setting with the SSIM term, else None."""
    return setting[3] if len(setting) > 3 else None


def ssim_constants(ssim):
    """(window float64 [win], c1, c2) of an SSIM part: metrics.ssim_window, c1 = (0.01 L)^2, c2 = (0.03 L)^2."""
    from .metrics import ssim_window
    _, win, sigma, L = ssim
    return ssim_window(win, sigma), (0.01 * L) ** 2, (0.03 * L) ** 2


def describe(setting):
    kind, param, mask = setting[:3]
    text = SHORT[kind] + ('(%g)' % param if kind in (HUBER, CHARBONNIER) else '')
    if ssim_part(setting):
        weight, win, sigma, L = ssim_part(setting)
        text += ' + %g x (1 - SSIM), window %d, sigma %g, data range %g' % (weight, win, sigma, L)
    return text + (', no-data pixels masked' if mask else '')


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
    kind, param, mask = setting[:3]
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
    """(sum rho, sum d*d, elements) in float64 over an NCHW pair; `elements` counts masked ones too (the denominator).  With the
    SSIM term the first is sum rho + ssim_fold * sum (1 - q), so that it over `elements` is the total the optimiser minimises and
    every consumer of the triple (shards, ranks, epoch sums) stays as it is."""
    r, q = terms(pred, y, setting)
    if tuple(setting) == DEFAULT:
        return float(np.sum(r)), float(np.sum(q)), float(r.size)
    sr = fixed_order_sum(r)
    if ssim_part(setting) and r.size:          # (an empty shard has no window)
        sr = float(sr + ssim_sums(pred, y, setting)[0] * ssim_fold(setting, r.shape))
    return sr, fixed_order_sum(q), float(r.size)


def host_loss(pred, y, setting=DEFAULT):
    """[loss, mean_squared_error] over an NCHW pair."""
    if tuple(setting) == DEFAULT:
        r, q = terms(pred, y, setting)
        return [float(np.mean(r)), float(np.mean(q))]
    sr, sq, cnt = host_sums(pred, y, setting)
    return [float(sr / cnt), float(sq / cnt)]


# ---- the SSIM term (include/dsen2_hip.h, "the SSIM loss term"; csrc/ssim_loss.hip) --------------------------------------------------
# T = weight * (1/Nw) * sum over the unmasked windows of (1 - q), Nw = n*c*(h-P+1)*(w-P+1) in every mask mode.  The statements
# below are float64 numpy in the device's operation order (numpy rounds every product and sum on its own) and, for the sum, in
# its summation order: an item is (plane = sample*c + band, tile); a tile stages S x S samples from (ty*T, tx*T), S = 32 for P >=
# 9 else 28, T = S - 2 (P-1), holds the RW x RW windows starting there, RW = S - P + 1, and adds those whose local origin is
# below T on each axis (all of them in the last tile of the axis); thread i % 256 of 256 adds the tile's windows i = wr*RW + wc in
# index order, a halving tree adds the threads, block b of min(items, 4096) adds its items b, b + blocks, ... in order, and
# one workgroup adds the blocks' partials (lane j the partials j, j + 256, ...; the tree).  A skipped window is a +0.0 term here:
# x + 0.0 == x for every x a sum started at +0.0 can hold.
def _ssim_stage(P):
    S = 32 if P >= 9 else 28
    return S, S - P + 1, S - 2 * (P - 1)


def _ssim_filter(f, g):
    """ssim.hip's separable filter over valid windows along the last two axes: the row pass, then the column pass, taps in order."""
    P = len(g)
    H, W = f.shape[-2:]
    r = g[0] * f[..., :, 0:W - P + 1]
    for k in range(1, P):
        r = r + g[k] * f[..., :, k:W - P + 1 + k]
    t = g[0] * r[..., 0:H - P + 1, :]
    for k in range(1, P):
        t = t + g[k] * r[..., k:H - P + 1 + k, :]
    return t


def ssim_window_terms(pred, y, window, c1, c2, mask):
    """(1 - q [n, c, OH, OW] float64, live [n, c, OH, OW] bool): every window's term and whether it counts (it holds no masked pixel)."""
    x = np.asarray(pred).astype(np.float64)
    t = np.asarray(y).astype(np.float64)
    g = np.asarray(window, np.float64)
    P = len(g)
    mx, my, exx, eyy, exy = (_ssim_filter(f, g) for f in (x, t, x * x, t * t, x * t))
    m11, m22, m12 = mx * mx, my * my, mx * my
    s1, s2, s12 = exx - m11, eyy - m22, exy - m12
    q = ((2.0 * m12 + c1) * (2.0 * s12 + c2)) / (((m11 + m22) + c1) * ((s1 + s2) + c2))
    live = np.ones(q.shape, bool)
    if mask == MASK_NODATA:
        blank = ~valid_pixels(y)
        holds = np.lib.stride_tricks.sliding_window_view(blank, (P, P), axis=(2, 3)).any(axis=(-1, -2))
        live = np.broadcast_to(~holds, q.shape).copy()
    return 1.0 - q, live


def ssim_tiled_sum(values, P):
    """The device's sum of values [planes, OH, OW] (0.0 where a window does not count) in its fixed order."""
    values = np.asarray(values, np.float64)
    planes, OH, OW = values.shape
    S, RW, T = _ssim_stage(P)
    ny = 1 if OH + P - 1 <= S else 1 + -(-(OH + P - 1 - S) // T)
    nx = 1 if OW + P - 1 <= S else 1 + -(-(OW + P - 1 - S) // T)
    pad = np.zeros((planes, (ny - 1) * T + RW, (nx - 1) * T + RW))
    pad[:, :OH, :OW] = values
    tiles = []
    for ty in range(ny):
        for tx in range(nx):
            loc = pad[:, ty * T:ty * T + RW, tx * T:tx * T + RW].copy()
            if ty < ny - 1:
                loc[:, T:, :] = 0.0
            if tx < nx - 1:
                loc[:, :, T:] = 0.0
            tiles.append(loc.reshape(planes, RW * RW))
    items = np.stack(tiles, axis=1).reshape(planes * ny * nx, RW * RW)
    items = np.concatenate([items, np.zeros((items.shape[0], -items.shape[1] % _THREADS))], axis=1).reshape(items.shape[0], -1, _THREADS)
    acc = np.zeros((items.shape[0], _THREADS))
    for j in range(items.shape[1]):
        acc = acc + items[:, j, :]
    sums = _tree(acc)
    blocks = min(sums.size, _MAX_BLOCKS)
    partials = _strided(sums, blocks)
    return float(_tree(_strided(partials, _THREADS).reshape(1, _THREADS))[0])


def ssim_sums(pred, y, setting):
    """(sum (1 - q) over the unmasked windows, Nw, unmasked windows) of an NCHW pair: dsen2_ssim_loss_sums' three numbers."""
    window, c1, c2 = ssim_constants(ssim_part(setting))
    P = len(window)
    n, c, h, w = np.asarray(y).shape
    if h < P or w < P:
        raise ValueError('a patch of %d x %d is smaller than the %d x %d window of the SSIM term' % (h, w, P, P))
    total, count = [], 0.0
    for i0 in range(0, n, 64):      # a chunk of samples at a time: the five fields of a large validation set need not coexist
        t, live = ssim_window_terms(np.asarray(pred)[i0:i0 + 64], np.asarray(y)[i0:i0 + 64], window, c1, c2, setting[2])
        total.append(np.where(live, t, 0.0).reshape(-1, h - P + 1, w - P + 1))
        count += float(live.sum())
    return ssim_tiled_sum(np.concatenate(total), P), float(n * c * (h - P + 1) * (w - P + 1)), count


def ssim_fold(setting, shape):
    """weight * N / Nw for an NCHW shape: what sum (1 - q) is multiplied by before it joins sum rho, whose denominator is N."""
    n, c, h, w = shape
    weight, P = ssim_part(setting)[:2]
    return weight * float(n * c * h * w) / float(n * c * (h - P + 1) * (w - P + 1))
