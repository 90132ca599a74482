#!/opt/conda/bin/python3.9
"""Generate tests/golden/trainset_*.npz by RUNNING THE REFERENCE'S OWN utils/patches.py and training/create_random.py.

Run in the build container only (the reference never travels to the GPU box):
    /opt/conda/bin/python3.9 tests/golden/make_golden_trainset.py
Environment at capture time: numpy 1.26.4, scipy 1.7.1, scikit-image 0.18.3.

The files hold DATA only — what the reference's functions returned for the two bundled tiles (tile_*_600.npz):
  trainset_down_<tile>.npz      downPixelAggr of the whole d10 / d20 / d60 as uint16 and as float32, SCALE 2 and 6, and of one 2-D
                                band: strips along all four image borders and a strided interior sample (tests/trainset_fixtures.py)
  trainset_weights.npz          the Gaussian weights scipy builds for sigma = 1/2 and 1/6
  trainset_random20.*.npz       save_random_patches (NR_CROP 16) on the downsampled T33UUB tile under random.seed(SEED_20): the
                                three .npy outputs and the origins drawn
  trainset_random60.*.npz       save_random_patches60 (NR_CROP 8) under random.seed(SEED_60), on the mirrored mosaic of T33UUB
                                (trainset_fixtures.mosaic_60: the tile itself is smaller than one patch at 1/36 resolution)
  trainset_val_index.npz        the loop of training/create_random.py at size 200 under random.seed(SEED_VAL)
It also ASSERTS that tests/downsample_restatement.py equals the reference's downPixelAggr in every value on the whole tiles.
"""
import contextlib
import io
import os
import random
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, '/root/reference')
from utils.patches import downPixelAggr, save_random_patches, save_random_patches60  # noqa: E402
import downsample_restatement as rs  # noqa: E402
import trainset_fixtures as fx  # noqa: E402


def scipy_weights(scale):
    from scipy.ndimage.filters import _gaussian_kernel1d
    sigma = 1.0 / scale
    radius = int(4.0 * sigma + 0.5)
    return _gaussian_kernel1d(sigma, 0, radius)[::-1]


def case_down(name):
    out = {}
    for key, x, scale in fx.down_cases(name):
        ref = downPixelAggr(x, SCALE=scale)
        assert ref.dtype == np.float64
        mine = rs.down_pixel_aggr(x, scale)
        assert mine.shape == ref.shape and np.array_equal(mine, ref), (name, key, np.abs(mine - ref).max())
        for part, v in fx.edge_views(ref).items():
            out['%s_%s' % (key, part)] = v
        print(name, key, ref.shape, 'restatement == reference')
    np.savez_compressed(os.path.join(HERE, 'trainset_down_%s.npz' % name), **out)
    # downPixelAggr refuses sizes that SCALE does not divide
    try:
        downPixelAggr(fx.load_tile(name)[2], SCALE=6)
    except ValueError:
        pass
    else:
        raise AssertionError('the reference accepted 100 x 100 at SCALE 6')


def run_random(fn, seed, *dsets, **kw):
    """The reference's function under random.seed(seed), and the origins it drew (the same seed replayed)."""
    with tempfile.TemporaryDirectory() as tmp:
        random.seed(seed)
        with contextlib.redirect_stdout(io.StringIO()):
            fn(*dsets, tmp + '/', **kw)
        return {f[:-4]: np.load(os.path.join(tmp, f)) for f in sorted(os.listdir(tmp))}


def drawn(seed, lr_shape, patch, n):
    random.seed(seed)
    return np.array([(random.randrange(0, lr_shape[0] - patch), random.randrange(0, lr_shape[1] - patch)) for _ in range(n)], np.int32)


def case_random():
    d10, d20, d60 = fx.load_tile('T33UUB')
    d10_lr, d20_lr = downPixelAggr(d10, SCALE=2), downPixelAggr(d20, SCALE=2)
    got = run_random(save_random_patches, fx.SEED_20, d20, d10_lr, d20_lr, NR_CROP=fx.NR_CROP_20)
    assert sorted(got) == ['data10', 'data20', 'data20_gt'] and all(v.dtype == np.float32 for v in got.values())
    got['origins'] = drawn(fx.SEED_20, d20_lr.shape, 16, fx.NR_CROP_20)
    o = got['origins'][3]
    assert np.array_equal(got['data20_gt'][3], np.rollaxis(d20[2 * o[0]:2 * o[0] + 32, 2 * o[1]:2 * o[1] + 32], 2))
    fx.save_split('trainset_random20', got)
    print('random20', {k: v.shape for k, v in got.items()})

    m10, m20, m60 = fx.mosaic_60(d10, d20, d60)
    lr = [downPixelAggr(a, SCALE=6) for a in (m10, m20, m60)]
    got = run_random(save_random_patches60, fx.SEED_60, m60, lr[0], lr[1], lr[2], NR_CROP=fx.NR_CROP_60)
    assert sorted(got) == ['data10', 'data20', 'data60', 'data60_gt']
    got['origins'] = drawn(fx.SEED_60, lr[2].shape, 16, fx.NR_CROP_60)
    o = got['origins'][5]
    assert np.array_equal(got['data60_gt'][5], np.rollaxis(m60[6 * o[0]:6 * o[0] + 96, 6 * o[1]:6 * o[1] + 96], 2))
    fx.save_split('trainset_random60', got)
    print('random60', {k: v.shape for k, v in got.items()})


def case_val_index():
    """training/create_random.py is a script with its size and path written in: its own text is executed with the size and the
    path replaced (and numpy's removed aliases np.bool / np.int spelled bool / int)."""
    src = open('/root/reference/training/create_random.py').read()
    with tempfile.TemporaryDirectory() as tmp:
        src = src.replace('size = 45*8000', 'size = %d' % fx.VAL_SIZE).replace("path = '../data/train/'", 'path = %r' % (tmp + '/'))
        src = src.replace('ratio = .1', 'ratio = %r' % fx.VAL_RATIO).replace('np.bool', 'bool').replace('np.int', 'int')
        assert 'size = %d' % fx.VAL_SIZE in src and tmp in src
        random.seed(fx.SEED_VAL)
        scope = {}
        with contextlib.redirect_stdout(io.StringIO()):
            exec(compile(src, 'create_random.py', 'exec'), scope)
        index = np.load(os.path.join(tmp, 'val_index.npy'))
    assert index.dtype == np.bool_ and index.sum() == int(fx.VAL_SIZE * fx.VAL_RATIO)
    np.savez_compressed(os.path.join(HERE, 'trainset_val_index.npz'), index=index, iterations=scope['i'], size=fx.VAL_SIZE,
                        ratio=fx.VAL_RATIO, seed=fx.SEED_VAL)
    print('val_index', index.shape, int(index.sum()), scope['i'])


if __name__ == '__main__':
    w = {}
    for scale in (2, 6):
        mine, radius = rs.gaussian_weights(scale)
        ref = scipy_weights(scale)
        assert np.array_equal(mine, ref)
        # the package pins these two sets (dsen2_amd/patches.py; read as text: this interpreter has no torch to import it with)
        import ast
        import re
        text = open(os.path.join(os.path.dirname(os.path.dirname(HERE)), 'dsen2_amd', 'patches.py')).read()
        table = ast.literal_eval(re.search(r'_REFERENCE_WEIGHTS = (\{.*?\n\})', text, re.S).group(1))
        assert [float.fromhex(v) for v in table[scale]] == ref.tolist()
        w['s%d' % scale] = ref
    np.savez_compressed(os.path.join(HERE, 'trainset_weights.npz'), **w)
    for name in fx.TILES:
        case_down(name)
    case_random()
    case_val_index()
