"""numpy restatement of the SSIM of csrc/ssim.hip, the yardstick of its tests: Wang, Bovik, Sheikh & Simoncelli 2004 (ssim_index.m
without its automatic down-sampling) per band, a Gaussian window over valid windows only, the biased (population) covariance.
float64 throughout; numpy rounds every product and every sum on its own, and every sum below is written out sequentially, so the
kernel's map can equal this one bit for bit.  The window is the product's (metrics.ssim_window): the one function both sides use.
The product must never import this file (tests/test_ssim_host.py checks that)."""
import numpy as np

from dsen2_amd.metrics import ssim_window


def filt(f, w):
    """The separable filter over valid windows: the row pass r[y][c] = w[0] f[y][c], then r = r + w[k] f[y][c + k] for k = 1 .. P - 1
    in order; the column pass the same sequential sum over r[y + k][c].  [H, W] -> [H - P + 1, W - P + 1]."""
    H, W = f.shape
    P = len(w)
    r = w[0] * f[:, 0:W - P + 1]
    for k in range(1, P):
        r = r + w[k] * f[:, k:W - P + 1 + k]
    t = w[0] * r[0:H - P + 1]
    for k in range(1, P):
        t = t + w[k] * r[k:H - P + 1 + k]
    return t


def ssim_map_band(x, y, data_range, win_size=11, sigma=1.5, k1=0.01, k2=0.03):
    """The SSIM map [H - P + 1, W - P + 1] of one band."""
    x = np.asarray(x).astype(np.float64)
    y = np.asarray(y).astype(np.float64)
    w = ssim_window(win_size, sigma)
    C1 = (float(k1) * float(data_range)) ** 2
    C2 = (float(k2) * float(data_range)) ** 2
    mx, my, exx, eyy, exy = filt(x, w), filt(y, w), filt(x * x, w), filt(y * y, w), filt(x * y, w)
    m11 = mx * mx
    m22 = my * my
    m12 = mx * my
    s1 = exx - m11
    s2 = eyy - m22
    s12 = exy - m12
    num = (2.0 * m12 + C1) * (2.0 * s12 + C2)
    den = (m11 + m22 + C1) * (s1 + s2 + C2)
    return num / den


def ssim_map(x, y, data_range, win_size=11, sigma=1.5, k1=0.01, k2=0.03):
    """[H - P + 1, W - P + 1, C] of two [H, W, C] images ([H, W] -> 2-D)."""
    x, y = np.asarray(x), np.asarray(y)
    if x.ndim == 2:
        return ssim_map_band(x, y, data_range, win_size, sigma, k1, k2)
    return np.stack([ssim_map_band(x[:, :, c], y[:, :, c], data_range, win_size, sigma, k1, k2) for c in range(x.shape[2])], axis=2)


def ssim(x, y, data_range, win_size=11, sigma=1.5, k1=0.01, k2=0.03):
    """(SSIM per band [C], their mean): the mean of each band's map."""
    q = ssim_map(x, y, data_range, win_size, sigma, k1, k2)
    if q.ndim == 2:
        q = q[:, :, None]
    band = np.array([q[:, :, c].mean() for c in range(q.shape[2])])
    return band, float(band.mean())


def window_2d(win_size=11, sigma=1.5):
    """fspecial('gaussian', P, sigma) as ssim_index.m builds it: the 2-D Gaussian divided by its sum (an independent statement of
    the window, for the host test against the 2-D form)."""
    d = np.arange(win_size, dtype=np.float64) - (win_size - 1) / 2.0
    g = np.exp(-(d[:, None] ** 2 + d[None, :] ** 2) / (2.0 * sigma * sigma))
    return g / g.sum()

