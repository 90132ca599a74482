"""numpy float64 restatement of dsen2_optimizer_step (include/dsen2_hip.h, "the optimiser step with options"), operation by
operation: numpy rounds every operation once, to nearest even, as the device does with contraction off; np.sqrt and the division
are correctly rounded on both sides.  The sum of squares takes its order from tests/fixed_sum_restatement.py.  The scalars reach
the kernel as floats and are widened there, so every one goes through float32 here."""
import numpy as np

from fixed_sum_restatement import THREADS, PER_THREAD, MAX_BLOCKS, fixed_order_sum

NADAM, ADAM, SGD = 0, 1, 2
NADAM_NAMES = ('lr', 'b1', 'b2', 'eps', 'mc_t', 'mc_t1', 'ms_new', 'ms_next', 'b2_pow_t')


def _w(x):
    """A float of the descriptor as the kernel sees it."""
    return np.float64(np.float32(x))


def sqsum_grid(count):
    """(blocks, the most elements one thread adds) of the sum of squares: the header's grid rule."""
    blocks = min(max(-(-count // (THREADS * PER_THREAD)), 1), MAX_BLOCKS)
    return blocks, -(-count // (blocks * THREADS))


def mean_gradient(g_rows, counts):
    """dsen2_nadam_step_shards' mean: rows in order onto 0.0 in double, a row whose count is 0 never read."""
    acc = np.zeros(g_rows[0].shape, np.float64)
    for c, g in zip(counts, g_rows):
        if c > 0:
            acc = acc + np.float64(c) * g.astype(np.float64)
    return (acc / np.float64(sum(counts))).astype(np.float32)


def global_norm(g_mean):
    gd = g_mean.astype(np.float64)
    return np.sqrt(np.float64(fixed_order_sum(gd * gd)))


def clip_scale(norm, clipnorm):
    c = _w(clipnorm)
    with np.errstate(invalid='ignore', divide='ignore'):
        return c / norm if norm >= c else np.float64(1.0)


def decay_mask(count, ranges):
    mask = np.zeros(count, bool)
    for lo, hi in ranges:
        mask[lo:hi] = True
    return mask


def restate(desc, p, g_rows, counts, m, v, ranges=()):
    """desc: a dict with kind, lr and the kind's scalars (Nadam: NADAM_NAMES; Adam: b1, b2, eps, lr_t; SGD: momentum, nesterov) and
    the options clipnorm, clipvalue, weight_decay (0 or absent: off).  Returns dict(g_mean, norm, scale, g, p, m, v): the unclipped
    mean, its global norm, the clipnorm scale, the gradient the update saw, and the new p, m, v (v None for SGD)."""
    kind = desc['kind']
    g_mean = mean_gradient(g_rows, counts)
    norm = global_norm(g_mean)
    g = g_mean
    scale = np.float64(1.0)
    if desc.get('clipnorm', 0) > 0:
        scale = clip_scale(norm, desc['clipnorm'])
        g = (g.astype(np.float64) * scale).astype(np.float32)
    if desc.get('clipvalue', 0) > 0:
        cv = np.float32(desc['clipvalue'])
        g = np.where(g < -cv, -cv, np.where(g > cv, cv, g)).astype(np.float32)          # a NaN passes: both comparisons are false
    gi, pd, md = g.astype(np.float64), p.astype(np.float64), m.astype(np.float64)
    lr = _w(desc['lr'])
    vt = None
    if kind == NADAM:
        _, b1, b2, eps, mc_t, mc_t1, ms_new, ms_next, b2_pow_t = (_w(desc[k]) for k in NADAM_NAMES)
        gp = gi / (1.0 - ms_new)
        mt = (b1 * md + (1.0 - b1) * gi).astype(np.float32)
        vt = (b2 * v.astype(np.float64) + (1.0 - b2) * gi * gi).astype(np.float32)
        mp = mt.astype(np.float64) / (1.0 - ms_next)
        vp = vt.astype(np.float64) / (1.0 - b2_pow_t)
        mbar = (1.0 - mc_t) * gp + mc_t1 * mp
        pt = (pd - lr * mbar / (np.sqrt(vp) + eps)).astype(np.float32)
    elif kind == ADAM:
        b1, b2, eps, lr_t = (_w(desc[k]) for k in ('b1', 'b2', 'eps', 'lr_t'))
        mt = (b1 * md + (1.0 - b1) * gi).astype(np.float32)
        vt = (b2 * v.astype(np.float64) + (1.0 - b2) * gi * gi).astype(np.float32)
        pt = (pd - lr_t * mt.astype(np.float64) / (np.sqrt(vt.astype(np.float64)) + eps)).astype(np.float32)
    elif kind == SGD:
        mu = _w(desc['momentum'])
        mt = (mu * md - lr * gi).astype(np.float32)
        if desc.get('nesterov'):
            pt = (pd + mu * mt.astype(np.float64) - lr * gi).astype(np.float32)
        else:
            pt = (pd + mt.astype(np.float64)).astype(np.float32)
    else:
        raise ValueError(kind)
    if desc.get('weight_decay', 0) > 0 and len(ranges):
        mask = decay_mask(p.size, ranges)
        decayed = (pt.astype(np.float64) - lr * _w(desc['weight_decay']) * pd).astype(np.float32)
        pt = np.where(mask, decayed, pt)
    return dict(g_mean=g_mean, norm=norm, scale=scale, g=g, p=pt, m=mt, v=vt)


def adam_scalars(lr, beta_1, beta_2, epsilon, t):
    """keras 2.2 Adam's step t (1-based), in double."""
    return dict(lr=lr, b1=beta_1, b2=beta_2, eps=epsilon, lr_t=lr * np.sqrt(1.0 - beta_2 ** t) / (1.0 - beta_1 ** t))
