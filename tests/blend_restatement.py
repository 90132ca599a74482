"""numpy restatement of the feathered recomposition of include/dsen2_hip.h ("feathered recomposition"), for
tests/test_blend_host.py and tests/test_gpu_blend.py.  Written from the definition: float64, a loop over the patches in
ascending (ty, tx) order, every patch laid over the pixels it covers — not from the kernel, which gathers per pixel."""
from math import ceil

import numpy as np


def grid(H, W, inner):
    return int(ceil(W / float(inner))), int(ceil(H / float(inner)))          # x_tiles, y_tiles


def origins(extent, inner):
    """Where the tiles of one axis start: t * inner, the last one clamped to extent - inner."""
    n = int(ceil(extent / float(inner)))
    return [extent - inner if t == n - 1 else t * inner for t in range(n)]


def weight_1d(P, border, feather):
    """int64 [P]: w(u) = clamp(min(u + 1, P - u) - (border - feather), 0, 2 * feather)."""
    u = np.arange(P, dtype=np.int64)
    return np.clip(np.minimum(u + 1, P - u) - (border - feather), 0, 2 * feather)


def axis_weights(L, P, border, feather):
    """int64 [tiles, L]: the 1-D weight of every tile of an axis at every image coordinate (0 where the patch does not reach;
    what a patch covers outside [0, L) is padding and is dropped)."""
    inner = P - 2 * border
    w1 = weight_1d(P, border, feather)
    starts = origins(L, inner)
    out = np.zeros((len(starts), L), np.int64)
    for t, s in enumerate(starts):
        lo, hi = max(0, s - border), min(L, s - border + P)
        out[t, lo:hi] = w1[lo - (s - border):hi - (s - border)]
    return out


def row_support(ty, H, inner, feather):
    """Image rows [r0, r1) on which tile row ty carries weight: [s - feather, s + inner + feather) cut to the image."""
    s = origins(H, inner)[ty]
    return max(0, s - feather), min(H, s + inner + feather)


def blend(patches, border, feather, H, W, scale, slots=None, valid=None):
    """float32 [H, W, C] from patches [n, C, P, P]: out = float32(sum_k w_k p_k / sum_k w_k) * float32(scale), the sums over the
    patches with w_k > 0 in ascending (ty, tx) order as a left fold that starts at its first term, in float64.  slots (patch
    index -> index in `patches`, anything outside [0, n) = the patch carries no weight) and valid (bool [H, W], False = the
    pixel is 0), both or neither; a pixel without any weighted patch is 0."""
    assert (slots is None) == (valid is None)
    n, C, P, _ = patches.shape
    inner = P - 2 * border
    x_tiles, y_tiles = grid(H, W, inner)
    w1 = weight_1d(P, border, feather)
    num = np.zeros((H, W, C), np.float64)
    den = np.zeros((H, W), np.int64)
    for ty, ys in enumerate(origins(H, inner)):
        for tx, xs in enumerate(origins(W, inner)):
            k = ty * x_tiles + tx
            s = k if slots is None else int(slots[k])
            if not 0 <= s < n:
                continue
            y0, y1 = max(0, ys - border), min(H, ys - border + P)
            x0, x1 = max(0, xs - border), min(W, xs - border + P)
            uy, ux = y0 - (ys - border), x0 - (xs - border)
            w = np.outer(w1[uy:uy + y1 - y0], w1[ux:ux + x1 - x0])
            p = patches[s, :, uy:uy + y1 - y0, ux:ux + x1 - x0].astype(np.float64).transpose(1, 2, 0)
            m = w > 0
            term = w[m][:, None] * p[m]                                # exact: an integer below 2^14 times a float32
            first = den[y0:y1, x0:x1][m] == 0
            acc = num[y0:y1, x0:x1][m]
            num[y0:y1, x0:x1][m] = np.where(first[:, None], term, acc + term)
            den[y0:y1, x0:x1] += w
    ok = den > 0
    if valid is not None:
        ok &= np.asarray(valid, bool)
    out = np.zeros((H, W, C), np.float32)
    out[ok] = (num[ok] / den[ok][:, None].astype(np.float64)).astype(np.float32) * np.float32(scale)
    return out


def weighted_patch_count(H, W, P, border, feather):
    """int [H, W]: how many patches carry weight at each pixel."""
    cy = (axis_weights(H, P, border, feather) > 0).sum(axis=0)
    cx = (axis_weights(W, P, border, feather) > 0).sum(axis=0)
    return np.outer(cy, cx)


def cut_patches(image, P, border):
    """[n, C, P, P] float32: every patch of the grid cut from image [H, W, C], zero outside it."""
    H, W, C = image.shape
    inner = P - 2 * border
    out = []
    for ys in origins(H, inner):
        for xs in origins(W, inner):
            p = np.zeros((P, P, C), np.float32)
            y0, y1 = max(0, ys - border), min(H, ys - border + P)
            x0, x1 = max(0, xs - border), min(W, xs - border + P)
            p[y0 - (ys - border):y1 - (ys - border), x0 - (xs - border):x1 - (xs - border)] = image[y0:y1, x0:x1]
            out.append(p.transpose(2, 0, 1))
    return np.ascontiguousarray(np.stack(out))
