"""numpy restatement of the no-data definitions of include/dsen2_hip.h ("tile no-data"), for tests/test_nodata_host.py and
tests/test_gpu_nodata.py.  Written from the definitions, with loops over pixels' owners — not from the kernels."""
from math import ceil

import numpy as np


def grid(H, W, inner):
    return int(ceil(W / float(inner))), int(ceil(H / float(inner)))          # x_tiles, y_tiles


def origins(extent, inner):
    """Where the tiles of one axis start: t * inner, the last one clamped to extent - inner."""
    n = int(ceil(extent / float(inner)))
    return [extent - inner if t == n - 1 else t * inner for t in range(n)]


def owner_map(H, W, inner):
    """int [H, W]: the row-major index of the patch each pixel takes its value from — the tiles are laid down in order, each
    overwriting what lies under its inner x inner square, as the reference's recompose_images does."""
    x_tiles, _ = grid(H, W, inner)
    own = np.full((H, W), -1, np.int64)
    for ty, ys in enumerate(origins(H, inner)):
        for tx, xs in enumerate(origins(W, inner)):
            own[ys:ys + inner, xs:xs + inner] = ty * x_tiles + tx
    assert (own >= 0).all()
    return own


def owned_rectangle(ty, tx, H, W, inner):
    """(y0, y1, x0, x1) of the definition in the header."""
    x_tiles, y_tiles = grid(H, W, inner)

    def interval(t, n, extent):
        return (extent - inner, extent) if t == n - 1 else (t * inner, min((t + 1) * inner, extent - inner))
    return interval(ty, y_tiles, H) + interval(tx, x_tiles, W)


def valid_pixels(img10):
    """bool [H, W]: a pixel holds data unless every band is exactly 0 (-0.0 == 0; NaN != 0 and a negative value are data)."""
    return (np.asarray(img10) != 0).any(axis=2)


def patch_empty(valid, inner):
    H, W = valid.shape
    x_tiles, y_tiles = grid(H, W, inner)
    own = owner_map(H, W, inner)
    has = np.zeros(x_tiles * y_tiles, bool)
    has[np.unique(own[valid])] = True
    return (~has).astype(np.uint8)


def pack_bits(valid):
    """uint32 [H, ceil(W / 32)]: pixel x is bit x & 31 of word x >> 5; the bits at x >= W are 0."""
    H, W = valid.shape
    words = (W + 31) // 32
    padded = np.zeros((H, words * 32), np.uint64)
    padded[:, :W] = valid
    weights = np.uint64(1) << (np.arange(words * 32, dtype=np.uint64) % np.uint64(32))
    return (padded * weights).reshape(H, words, 32).sum(axis=2).astype(np.uint32)


def slot_map(empty):
    kept = [k for k, e in enumerate(np.asarray(empty).reshape(-1)) if not e]
    slots = np.full(len(np.asarray(empty).reshape(-1)), -1, np.int32)
    for j, k in enumerate(kept):
        slots[k] = j
    return np.array(kept, np.int64), slots


def recompose(patches, slots, valid, border, scale):
    """float32 [H, W, C] from a compact buffer [n, C, P, P]: a pixel without data, or whose owner has no slot in [0, n), is 0."""
    H, W = valid.shape
    n, C, P, _ = patches.shape
    inner = P - 2 * border
    x_tiles, _ = grid(H, W, inner)
    own = owner_map(H, W, inner)
    ys, xs = origins(H, inner), origins(W, inner)
    img = np.zeros((H, W, C), np.float32)
    for y in range(H):
        for x in range(W):
            k = own[y, x]
            s = slots[k]
            if valid[y, x] and 0 <= s < n:
                ty, tx = divmod(int(k), x_tiles)
                img[y, x] = patches[s, :, border + y - ys[ty], border + x - xs[tx]] * np.float32(scale)
    return img


def final_rows(slots, slots_done, per, H, W, inner):
    """bool per tile row: every patch of the row is empty or among the first `slots_done` slots of its shard of `per`."""
    x_tiles, y_tiles = grid(H, W, inner)
    out = []
    for ty in range(y_tiles):
        row = slots[ty * x_tiles:(ty + 1) * x_tiles]
        out.append(all(s < 0 or (per > 0 and s % per < slots_done) for s in row))
    return np.array(out, bool)


def tile_row_rows(ty, H, inner):
    """Image rows [r0, r1) that tile row ty decides."""
    y_tiles = int(ceil(H / float(inner)))
    return (H - inner, H) if ty == y_tiles - 1 else (ty * inner, min((ty + 1) * inner, H - inner))
