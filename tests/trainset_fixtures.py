"""Helpers shared by tests/golden/make_golden_trainset.py (which records the reference's outputs) and the tests that read them."""
import glob
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
TILES = ('T33UUB', 'T49JGM')
EDGE = 6                      # rows / columns of each border strip of a recorded downsampler output
SEED_20, SEED_60, SEED_VAL = 20170527, 20171022, 38
NR_CROP_20, NR_CROP_60 = 16, 8
VAL_SIZE, VAL_RATIO = 200, 0.1


def load_tile(name):
    z = np.load(os.path.join(GOLDEN, 'tile_%s_600.npz' % name))
    return z['d10'], z['d20'], z['d60']


def down_cases(name):
    """(key, input array, scale) of every recorded downsampler case of one tile: the three resolutions, uint16 and float32,
    SCALE 2 and 6 (the 100 x 100 60 m image is cropped to 96 x 96 for SCALE 6: downPixelAggr refuses an indivisible size), plus
    one 2-D single-band input."""
    d10, d20, d60 = load_tile(name)
    out = []
    for res, a in (('d10', d10), ('d20', d20), ('d60', d60)):
        for dt in (np.uint16, np.float32):
            for scale in (2, 6):
                x = a[:96, :96] if (res == 'd60' and scale == 6) else a
                out.append(('%s_%s_s%d' % (res, np.dtype(dt).name, scale), np.ascontiguousarray(x.astype(dt)), scale))
    out.append(('band_uint16_s2', np.ascontiguousarray(d10[:, :, 0]), 2))
    return out


def edge_views(out):
    """The parts of a downsampler output that are recorded: strips along all four image borders (they pin the reflect boundary)
    and a strided sample of the interior."""
    return {'top': out[:EDGE], 'bottom': out[-EDGE:], 'left': out[:, :EDGE], 'right': out[:, -EDGE:], 'sub': out[3::7, 2::5]}


def mosaic_60(d10, d20, d60):
    """A 1152 x 1152 (10 m) image from the 576 x 576 corner of a bundled tile, mirrored to the right and downwards: the 600 x 600
    tile itself is 16 pixels at 1/36 resolution, and save_random_patches60 needs more than its 16 x 16 patch."""
    def grow(a, n):
        a = a[:n, :n]
        return np.ascontiguousarray(np.pad(a, ((0, n), (0, n), (0, 0)), mode='symmetric'))
    return grow(d10, 576), grow(d20, 288), grow(d60, 96)


def save_split(stem, arrays, limit=900 * 1024):
    """np.savez_compressed of each array on its own, cut along axis 0 into as many files as it takes to stay below `limit` bytes
    each: GOLDEN/<stem>.<key>.<i>.npz."""
    for old in glob.glob(os.path.join(GOLDEN, stem + '.*.npz')):
        os.remove(old)
    for key, a in arrays.items():
        a = np.asarray(a)
        parts = 1
        while True:
            pieces = np.array_split(a, parts, axis=0) if a.ndim else [a]
            paths = []
            for i, piece in enumerate(pieces):
                path = os.path.join(GOLDEN, '%s.%s.%d.npz' % (stem, key, i))
                np.savez_compressed(path, a=piece)
                paths.append(path)
            if all(os.path.getsize(p) <= limit for p in paths):
                break
            for p in paths:
                os.remove(p)
            parts += 1


def load_split(stem, key):
    paths = sorted(glob.glob(os.path.join(GOLDEN, '%s.%s.*.npz' % (stem, key))), key=lambda p: int(p.split('.')[-2]))
    assert paths, 'no fixture %s.%s' % (stem, key)
    pieces = [np.load(p)['a'] for p in paths]
    return pieces[0] if pieces[0].ndim == 0 else np.concatenate(pieces, axis=0)
