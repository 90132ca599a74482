"""Helpers shared by tests/golden/make_golden_imresize.py (which records the reference's outputs) and the tests that read them."""
import json
import os

import numpy as np

import trainset_fixtures as fx

GOLDEN = fx.GOLDEN
TILES = fx.TILES
EDGE = 3                      # rows / columns of each border strip of a recorded enlargement
SCALE = 2000                  # training/supres_train.py

# (in_length, out_length, scale) of every recorded contributions() call.  in_length 3: the taps reflect more than once.
CONTRIB_CASES = [(10, 20, 2.0), (10, 60, 6.0), (10, 15, 1.5), (10, 5, 0.5), (12, 2, 1.0 / 6), (300, 600, 2.0), (100, 600, 6.0),
                 (3, 6, 2.0), (3, 18, 6.0), (3, 1, 1.0 / 3), (3, 2, 0.5),
                 (10, 25, 25.0 / 10), (12, 18, 18.0 / 12)]          # output_shape (25, 18) of a 10 x 12 image: one scale per axis

# (key, shape, dtype, scalar_scale, output_shape) of every imresize() call recorded whole
IMAGE_CASES = [
    ('hwc_f32_x2', (12, 10, 3), np.float32, 2, None),
    ('hwc_u16_x6', (7, 9, 2), np.uint16, 6, None),
    ('hwc_f64_x1p5', (9, 8, 4), np.float64, 1.5, None),
    ('hwc_u16_half', (16, 14, 3), np.uint16, 0.5, None),
    ('hwc_f32_sixth', (24, 30, 2), np.float32, 1.0 / 6, None),
    ('hwc_f64_third', (18, 21, 6), np.float64, 1.0 / 3, None),
    ('band_f32_x2', (11, 13), np.float32, 2, None),
    ('band_u16_x6', (5, 6), np.uint16, 6, None),
    ('band_f64_x1p5', (9, 7), np.float64, 1.5, None),
    ('band_f64_half', (16, 18), np.float64, 0.5, None),          # single band, 8 taps or more: numpy adds them pairwise
    ('band_u16_sixth', (36, 30), np.uint16, 1.0 / 6, None),
    ('band_f32_third', (18, 21), np.float32, 1.0 / 3, None),
    ('one_f32_half', (16, 18, 1), np.float32, 0.5, None),
    ('hwc_f32_shape', (10, 12, 3), np.float32, None, (25, 18)),     # scales 2.5 and 1.5: axis 1 runs first
    ('hwc_u16_shape_down_up', (12, 12, 2), np.uint16, None, (6, 30)),
    ('hwc_f64_shape_up_down', (8, 20, 2), np.float64, None, (16, 10)),  # scales 2 and 0.5: axis 1 runs first
    ('tiny_u16_x2', (3, 5, 2), np.uint16, 2, None),
    ('tiny_u16_x6', (3, 5, 2), np.uint16, 6, None),
    ('tiny_f32_third', (3, 5, 2), np.float32, 1.0 / 3, None),
]


def image(key):
    """The seeded integer-valued input of one IMAGE_CASES entry (numpy's frozen legacy generator: the same on every numpy)."""
    for n, (k, shape, dtype, _, _) in enumerate(IMAGE_CASES):
        if k == key:
            return np.random.RandomState(1000 + n).randint(0, 10000, size=shape).astype(dtype)
    raise KeyError(key)


def edge_views(out):
    """The recorded parts of an enlarged tile: strips along all four borders (they pin the symmetric boundary) and a strided
    sample of the interior."""
    return {'top': out[:EDGE], 'bottom': out[-EDGE:], 'left': out[:, :EDGE], 'right': out[:, -EDGE:], 'sub': out[3::11, 2::7]}


def tile_cases(name):
    """(key, input, scale): the 20 m bands x 2 and the 60 m bands x 6 of one bundled tile."""
    _, d20, d60 = fx.load_tile(name)
    return [('d20_x2', d20, 2), ('d60_x6', d60, 6)]


def opendata_dir(path, run_60):
    """The tiny test directory OpenDataFilesTest is recorded on: data10 / data20 (/ data60) patches and roi.json."""
    rng = np.random.RandomState(77)
    os.makedirs(path, exist_ok=True)
    np.save(os.path.join(path, 'data10.npy'), rng.randint(0, 9000, size=(3, 4, 8, 8)).astype(np.float32))
    np.save(os.path.join(path, 'data20.npy'), rng.randint(0, 9000, size=(3, 6, 8, 8)).astype(np.float32))
    if run_60:
        np.save(os.path.join(path, 'data60.npy'), rng.randint(0, 9000, size=(3, 2, 8, 8)).astype(np.float32))
    with open(os.path.join(path, 'roi.json'), 'w') as f:
        json.dump([6, 12, 48, 30], f)


def rmse_regions(name):
    """(key, ground truth, scale) of the recorded bicubic baselines of one tile: the 20 m bands of the whole
    tile (what `create_patches --test_data` keeps without a region), the 60 m bands of its 576 x 576 corner (the largest region
    whose 60 m image SCALE 6 divides) and, for T33UUB, of the mirrored mosaic the --run_60 flow is tested on."""
    d10, d20, d60 = fx.load_tile(name)
    out = [('d20_x2', d20, 2), ('d60_x6', np.ascontiguousarray(d60[:96, :96]), 6)]
    if name == 'T33UUB':
        out.append(('mosaic_d60_x6', fx.mosaic_60(d10, d20, d60)[2], 6))
    return out
