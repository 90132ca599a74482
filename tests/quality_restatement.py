"""numpy restatement of the two quality metrics of csrc/quality_metrics.hip, the yardstick of their tests: the universal image
quality index (Wang & Bovik 2002, img_qi.m) and the spectral angle mapper.  float64 throughout; numpy rounds every product and
every sum on its own, and every sum below is written out sequentially, so the kernel's quality map can equal this one bit for
bit.  The product must never import this file (tests/test_quality_metrics_host.py checks that)."""
import numpy as np


def box(a, B):
    """Valid B x B window sums: horizontal first, then vertical, each sequential (left to right, top to bottom).  NOT a sliding
    add-the-new, subtract-the-old sum: that rounds differently."""
    H, W = a.shape
    s = a[:, 0:W - B + 1]
    for k in range(1, B):
        s = s + a[:, k:W - B + 1 + k]
    t = s[0:H - B + 1]
    for k in range(1, B):
        t = t + s[k:H - B + 1 + k]
    return t


def uiq_map_band(x, y, B=8, branches=None):
    """The quality map [H - B + 1, W - B + 1] of one band.  branches (a dict): the number of windows each special case took."""
    x = np.asarray(x).astype(np.float64)
    y = np.asarray(y).astype(np.float64)
    N = float(B * B)
    sx, sy, sxx, syy, sxy = box(x, B), box(y, B), box(x * x, B), box(y * y, B), box(x * y, B)
    s12 = sx * sy
    q12 = sx * sx + sy * sy
    num = (4.0 * (N * sxy - s12)) * s12
    den1 = N * (sxx + syy) - q12
    den = den1 * q12
    q = np.ones_like(den)                                  # a window where both images are all zero scores 1
    flat = (den1 == 0) & (q12 != 0)
    q[flat] = (2.0 * s12[flat]) / q12[flat]
    usual = den != 0
    q[usual] = num[usual] / den[usual]                     # applied last, as in img_qi.m
    if branches is not None:
        branches['flat'] = branches.get('flat', 0) + int((flat & ~usual).sum())
        branches['one'] = branches.get('one', 0) + int((~flat & ~usual).sum())
    return q


def uiq_map(x, y, B=8, branches=None):
    """[H - B + 1, W - B + 1, C] of two [H, W, C] images ([H, W] -> 2-D)."""
    x, y = np.asarray(x), np.asarray(y)
    if x.ndim == 2:
        return uiq_map_band(x, y, B, branches)
    return np.stack([uiq_map_band(x[:, :, c], y[:, :, c], B, branches) for c in range(x.shape[2])], axis=2)


def uiq(x, y, B=8):
    """(UIQ per band [C], their mean): the mean of each band's map."""
    q = uiq_map(x, y, B)
    if q.ndim == 2:
        q = q[:, :, None]
    band = np.array([q[:, :, c].mean() for c in range(q.shape[2])])
    return band, float(band.mean())


def sam_angles(x, y):
    """(angles in degrees of the pixels that count, in row-major order; the mask of those pixels [H, W])."""
    x = np.asarray(x).astype(np.float64)
    y = np.asarray(y).astype(np.float64)
    if x.ndim == 2:
        x, y = x[:, :, None], y[:, :, None]
    d = x[..., 0] * y[..., 0]
    nx = x[..., 0] * x[..., 0]
    ny = y[..., 0] * y[..., 0]
    for c in range(1, x.shape[-1]):
        d = d + x[..., c] * y[..., c]
        nx = nx + x[..., c] * x[..., c]
        ny = ny + y[..., c] * y[..., c]
    den = np.sqrt(nx) * np.sqrt(ny)
    ok = den != 0
    cs = np.minimum(1.0, np.maximum(-1.0, d[ok] / den[ok]))
    return np.arccos(cs) * (180.0 / np.pi), ok


def sam_sums(x, y):
    """(sum of the angles in degrees, pixels counted); SAM is their quotient."""
    angles, ok = sam_angles(x, y)
    return float(angles.sum()), int(ok.sum())


def planted(seed=0, shape=(40, 37)):
    """The image pair of the issue's check: a flat region (constant, different, non-zero in both) and an all-zero region."""
    r = np.random.RandomState(seed)
    gt = r.randint(1, 4000, shape).astype(np.uint16)
    x = (gt + r.normal(0, 30, shape)).astype(np.float32)
    gt[5:20, 3:18] = 1234
    x[5:20, 3:18] = 1200.0
    gt[22:34, 20:33] = 0
    x[22:34, 20:33] = 0.0
    return x, gt
