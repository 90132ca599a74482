"""numpy restatements for the tests of drawing crops with origin masks and of validating on the device: the valid-origin map of
dsen2_corpus_origin_mask from its definitions (include/dsen2_hip.h, "corpus origin mask"), the redraw rule of
corpus.CorpusSampler(masks=) with plain loops, and the summation order of dsen2_abs_sq_error_sums."""
import numpy as np

from fixed_sum_restatement import fixed_order_sum as _fixed_order_sum      # the entries' order of addition

CROP = 16


def blank_cells(d10, grid, footprint):
    """bool [grid_h, grid_w]: a band-0 sample of the cell's footprint x footprint samples fails v >= 1 (a NaN fails it)."""
    gh, gw = grid
    band0 = np.asarray(d10)[:, :, 0]
    assert band0.shape == (gh * footprint, gw * footprint)
    with np.errstate(invalid='ignore'):
        bad = ~(band0 >= 1)
    return bad.reshape(gh, footprint, gw, footprint).any(axis=(1, 3))


def covered_cells(grid, holdout, margin):
    gh, gw = grid
    cells = np.zeros((gh, gw), bool)
    for vy, vx in np.asarray(holdout, np.int64).reshape(-1, 2).tolist():
        cells[max(vy - margin, 0):max(vy + CROP + margin, 0), max(vx - margin, 0):max(vx + CROP + margin, 0)] = True
    return cells


def valid_origins(cells):
    """bool [grid_h - 15, grid_w - 15] from the cell map (True = blank or covered): no such cell in the origin's 16 x 16 window."""
    gh, gw = cells.shape
    valid = np.zeros((gh - CROP + 1, gw - CROP + 1), bool)
    for oy in range(valid.shape[0]):
        for ox in range(valid.shape[1]):
            valid[oy, ox] = not cells[oy:oy + CROP, ox:ox + CROP].any()
    return valid


def origin_mask(d10, grid, footprint, holdout=(), margin=0):
    """(packed bitmap, count, cell map as uint8) as the entry writes them."""
    cells = blank_cells(d10, grid, footprint) | covered_cells(grid, holdout, margin)
    valid = valid_origins(cells)
    return np.packbits(valid, axis=1, bitorder='little'), int(valid.sum()), cells.astype(np.uint8)


def pack(valid):
    return np.packbits(np.asarray(valid, bool), axis=1, bitorder='little')


def draw_with_masks(rng, extents, valid, n, augment, max_rounds=10000):
    """One draw(n) of a sampler with masks, from scratch: today's draws, then the redraw rounds.  valid: bool maps per tile."""
    ext = np.asarray(extents, np.int64)
    table = np.zeros((n, 4), np.int32)
    tiles = rng.integers(0, len(extents), size=n)
    table[:, 0] = tiles
    table[:, 1] = rng.integers(0, ext[tiles, 0] - CROP)
    table[:, 2] = rng.integers(0, ext[tiles, 1] - CROP)
    if augment:
        table[:, 3] = rng.integers(0, 8, size=n)
    return redraw(rng, table, ext, valid, max_rounds)


def redraw(rng, table, ext, valid, max_rounds=10000):
    for _ in range(max_rounds + 1):
        bad = [k for k in range(table.shape[0]) if not valid[table[k, 0]][table[k, 1], table[k, 2]]]      # ascending
        if not bad:
            return table
        rows = rng.integers(0, np.asarray([ext[table[k, 0], 0] - CROP for k in bad]))
        cols = rng.integers(0, np.asarray([ext[table[k, 0], 1] - CROP for k in bad]))
        for k, oy, ox in zip(bad, rows, cols):
            table[k, 1], table[k, 2] = oy, ox
    raise AssertionError('the restatement did not end')


def validation_table(extents, crops_per_tile, seed, stream, valid=None):
    """corpus.validation_table from its documented order: per tile m row origins, then m column origins; then the redraws."""
    rng = np.random.default_rng(np.random.SeedSequence([int(seed), stream]))
    m = crops_per_tile
    table = np.zeros((len(extents) * m, 4), np.int32)
    for i, (eh, ew) in enumerate(extents):
        table[i * m:(i + 1) * m, 0] = i
        table[i * m:(i + 1) * m, 1] = rng.integers(0, eh - CROP, size=m)
        table[i * m:(i + 1) * m, 2] = rng.integers(0, ew - CROP, size=m)
    if valid is not None:
        redraw(rng, table, np.asarray(extents, np.int64), valid)
    return table


# ---- dsen2_abs_sq_error_sums ---------------------------------------------------------------------------------------------------------
def abs_sq_error_sums(pred, target):
    """(sum |p - t|, sum (p - t)^2) in the entry's order: float64 throughout, every operation rounded on its own."""
    d = np.asarray(pred, np.float32).astype(np.float64).ravel() - np.asarray(target, np.float32).astype(np.float64).ravel()
    return _fixed_order_sum(np.abs(d)), _fixed_order_sum(d * d)


def sums_bound(count):
    """Relative bound between two summation orders of `count` non-negative float64 terms: each order is within (count - 1) * 2^-53
    of the exact sum, relative to it."""
    return 2.0 * (count - 1) * 2.0 ** -53
