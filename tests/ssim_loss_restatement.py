"""numpy restatement of the SSIM loss term of csrc/ssim_loss.hip (include/dsen2_hip.h, "the SSIM loss term"), the yardstick of its
tests: the term, G, the float32 accumulation into the NHWC16 gradient and the summation order, operation by operation.  float64
throughout; numpy rounds every product and every sum on its own, and every sum below is written out sequentially.  This is not a
test, and the product never imports it.

    mx, my, exx, eyy, exy = ssim.hip's filter of x, y, x*x, y*y, x*y        (row pass, then column pass, taps k = 0 .. P-1 in order)
    m11 = mx*mx  m22 = my*my  m12 = mx*my  s1 = exx - m11  s2 = eyy - m22  s12 = exy - m12
    A1 = 2*m12 + c1   A2 = 2*s12 + c2   B1 = (m11 + m22) + c1   B2 = (s1 + s2) + c2   den = B1*B2   q = (A1*A2) / den
    a = ((2*my)*(A2 - A1)) / den - (((2*mx)*q)*(B2 - B1)) / den      b = (-q) / B2      d = (2*A1) / den
    a = b = d = 0 in a window that holds a masked pixel
    Gt m: zero outside the map; column pass t[ur][pc] = g[0]*m[ur][pc], t = t + g[k]*m[ur-k][pc]; row pass the same over t[ur][uc-k]
    G = (Gt a + (2*x)*Gt b) + y*Gt d
    g16[pixel][band] = float32(float64(g16[pixel][band]) + scale*G),   scale = -float64(float32(weight)) / Nw
"""
import numpy as np

from fixed_sum_restatement import THREADS, MAX_BLOCKS, strided, tree


def filt(f, g):
    """[..., H, W] -> [..., H - P + 1, W - P + 1]: tests/ssim_restatement.filt along the last two axes."""
    H, W = f.shape[-2:]
    P = len(g)
    r = g[0] * f[..., :, 0:W - P + 1]
    for k in range(1, P):
        r = r + g[k] * f[..., :, k:W - P + 1 + k]
    t = g[0] * r[..., 0:H - P + 1, :]
    for k in range(1, P):
        t = t + g[k] * r[..., k:H - P + 1 + k, :]
    return t


def filt_transposed(m, g):
    """[..., OH, OW] -> [..., OH + P - 1, OW + P - 1]: the full filter, zeros outside the map, the column pass first."""
    P = len(g)
    OH, OW = m.shape[-2:]
    z = np.zeros(m.shape[:-2] + (OH + 2 * (P - 1), OW))
    z[..., P - 1:P - 1 + OH, :] = m
    H = OH + P - 1                                     # t[ur] reads m[ur - k] = z[ur - k + P - 1]
    t = g[0] * z[..., P - 1:P - 1 + H, :]
    for k in range(1, P):
        t = t + g[k] * z[..., P - 1 - k:P - 1 - k + H, :]
    z = np.zeros(t.shape[:-1] + (OW + 2 * (P - 1),))
    z[..., P - 1:P - 1 + OW] = t
    W = OW + P - 1
    r = g[0] * z[..., P - 1:P - 1 + W]
    for k in range(1, P):
        r = r + g[k] * z[..., P - 1 - k:P - 1 - k + W]
    return r


def valid_pixels(y):
    """[n, 1, h, w] bool: the target is not 0 (or -0) in at least one band."""
    return (np.asarray(y) != 0).any(axis=1, keepdims=True)


def live_windows(y, P, mask):
    """[n, 1, OH, OW] bool: the window holds no masked pixel."""
    n, c, h, w = y.shape
    live = np.ones((n, 1, h - P + 1, w - P + 1), bool)
    if mask:
        blank = ~valid_pixels(y)
        for r in range(P):
            for s in range(P):
                live &= ~blank[:, :, r:r + h - P + 1, s:s + w - P + 1]
    return live


def maps(out, y, window, c1, c2, mask):
    """(q, a, b, d [n, c, OH, OW] float64; live [n, c, OH, OW] bool) of an NCHW float32 pair; a, b, d are 0 where not live."""
    x = np.asarray(out).astype(np.float64)
    t = np.asarray(y).astype(np.float64)
    g = np.asarray(window, np.float64)
    mx, my, exx, eyy, exy = filt(x, g), filt(t, g), filt(x * x, g), filt(t * t, g), filt(x * t, g)
    m11 = mx * mx
    m22 = my * my
    m12 = mx * my
    s1 = exx - m11
    s2 = eyy - m22
    s12 = exy - m12
    A1 = 2.0 * m12 + c1
    A2 = 2.0 * s12 + c2
    B1 = (m11 + m22) + c1
    B2 = (s1 + s2) + c2
    den = B1 * B2
    q = (A1 * A2) / den
    a = ((2.0 * my) * (A2 - A1)) / den - (((2.0 * mx) * q) * (B2 - B1)) / den
    b = (-q) / B2
    d = (2.0 * A1) / den
    live = np.broadcast_to(live_windows(np.asarray(y), len(g), mask), q.shape)
    return q, np.where(live, a, 0.0), np.where(live, b, 0.0), np.where(live, d, 0.0), live


def big_g(out, y, window, c1, c2, mask):
    """G [n, c, h, w] float64: dT/dout = scale * G."""
    x = np.asarray(out).astype(np.float64)
    t = np.asarray(y).astype(np.float64)
    g = np.asarray(window, np.float64)
    _, a, b, d, _ = maps(out, y, window, c1, c2, mask)
    return (filt_transposed(a, g) + (2.0 * x) * filt_transposed(b, g)) + t * filt_transposed(d, g)


def windows(shape, P):
    n, c, h, w = shape
    return float(n * c * (h - P + 1) * (w - P + 1))


def stage(P):
    """(S, RW, T): the staged side, the windows per side and the step of a tile."""
    S = 32 if P >= 9 else 28
    return S, S - P + 1, S - 2 * (P - 1)


def tiles_along(L, P):
    S, _, T = stage(P)
    return 1 if L <= S else 1 + -(-(L - S) // T)


def tiled_sum(values, h, w, P):
    """The kernel's sum of values [planes, OH, OW], window by window through its items (plane, tile), threads, blocks and finish."""
    S, RW, T = stage(P)
    planes, OH, OW = values.shape
    ny, nx = tiles_along(h, P), tiles_along(w, P)
    wr, wc = np.divmod(np.arange(RW * RW), RW)                 # window i of a tile is (i / RW, i % RW)
    rows = -(-RW * RW // THREADS)
    item_sums = []
    for p in range(planes):
        for ty in range(ny):
            for tx in range(nx):
                gr, gc = ty * T + wr, tx * T + wc
                mine = (gr < OH) & (gc < OW) & ((ty == ny - 1) | (wr < T)) & ((tx == nx - 1) | (wc < T))
                local = np.zeros(rows * THREADS)               # thread i % 256 adds window i; one it does not add is a +0.0 term
                local[:RW * RW][mine] = values[p, gr[mine], gc[mine]]
                lanes = np.zeros(THREADS)
                for row in local.reshape(rows, THREADS):       # i = tid, tid + 256, ... in index order
                    lanes = lanes + row
                item_sums.append(tree(lanes.reshape(1, THREADS))[0])
    item_sums = np.array(item_sums)
    blocks = min(item_sums.size, MAX_BLOCKS)
    return float(tree(strided(strided(item_sums, blocks), THREADS).reshape(1, THREADS))[0])


def sums(out, y, window, c1, c2, mask):
    """float64 [3]: { sum (1 - q) over the unmasked windows, Nw, unmasked windows } (dsen2_ssim_loss_sums; dsen2_ssim_loss_grad gives
    the first two).  A window that does not count is a +0.0 term: x + 0.0 == x for every x that a sum started at +0.0 can hold."""
    n, c, h, w = np.asarray(y).shape
    P = len(window)
    q, _, _, _, live = maps(out, y, window, c1, c2, mask)
    terms = np.where(live, 1.0 - q, 0.0).reshape(n * c, h - P + 1, w - P + 1)
    return np.array([tiled_sum(terms, h, w, P), windows((n, c, h, w), P), float(live.sum())])


def accumulate(g16, out, y, weight, window, c1, c2, mask):
    """The NHWC16 float32 gradient [n*h*w, 16] after the term was added to g16: one rounding per lane, lanes >= c as they were."""
    n, c, h, w = np.asarray(y).shape
    scale = -float(np.float32(weight)) / windows((n, c, h, w), len(window))
    G = big_g(out, y, window, c1, c2, mask).transpose(0, 2, 3, 1).reshape(n * h * w, c)
    res = np.array(g16, dtype=np.float32, copy=True)
    res[:, :c] = (res[:, :c].astype(np.float64) + scale * G).astype(np.float32)
    return res


def term(out, y, weight, window, c1, c2, mask):
    """T in float64: (weight / Nw) * sum."""
    s = sums(out, y, window, c1, c2, mask)
    return (float(np.float32(weight)) / s[1]) * s[0]
