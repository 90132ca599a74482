#!/opt/conda/bin/python3.9
"""Generate tests/golden/imresize_*.npz / .json by RUNNING THE REFERENCE'S OWN utils/imresize.py, utils/patches.py and the RMSE of
testing/demoDSen2.py.

Run in the build container only (the reference never travels to the GPU box):
    /opt/conda/bin/python3.9 tests/golden/make_golden_imresize.py
Environment at capture time: numpy 1.26.4, scipy 1.7.1, scikit-image 0.18.3.

The files hold DATA only (tests/imresize_fixtures.py lists the cases):
  imresize_contributions.npz   weights and indices of contributions() for every CONTRIB_CASES entry
  imresize_images.npz          imresize() of every IMAGE_CASES entry, whole (small seeded integer-valued images: float32, float64,
                               uint16; HWC and 2-D; enlargements, reductions, output_shape with one scale per axis)
  imresize_tile_<tile>.npz     imresize(d20, 2) and imresize(d60, 6) of the bundled tiles: the strips along all four borders and a
                               strided interior sample
  imresize_opendata.npz/.json  OpenDataFilesTest on a tiny test directory: the arrays and image_size it returns, the lines it prints
  imresize_rmse.json           the demo's bicubic baseline RMSE(imresize(downPixelAggr(gt), s), gt) on the regions create_patches
                               keeps: 'f64' with the downsampled image as downPixelAggr returns it, 'f32' with its float32 cast
                               (what create_patches stores in no_tiling/ and an evaluation therefore reads)
It also ASSERTS that tests/imresize_restatement.py equals the reference's imresize on every whole image and on the whole tiles:
bit for bit where numpy adds the taps sequentially, within the restatement's bound elsewhere.
"""
import ast
import contextlib
import io
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, '/root/reference')
from utils import imresize as ref  # noqa: E402
from utils.patches import OpenDataFilesTest, downPixelAggr  # noqa: E402
import imresize_fixtures as ifx  # noqa: E402
import imresize_restatement as rs  # noqa: E402


def demo_rmse():
    """RMSE of testing/demoDSen2.py (a script that imports h5py and the networks at the top: only that function is taken)."""
    tree = ast.parse(open('/root/reference/testing/demoDSen2.py').read())
    fn = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == 'RMSE'][0]
    scope = {'np': np}
    exec(compile(ast.Module(body=[fn], type_ignores=[]), 'demoDSen2.py', 'exec'), scope)
    return scope['RMSE']


def check_restatement(what, x, want, scalar_scale=None, output_shape=None):
    mine, bound = rs.imresize(x, scalar_scale, output_shape, with_bound=True)
    assert mine.dtype == want.dtype == np.float64 and mine.shape == want.shape, (what, mine.shape, want.shape)
    if rs.is_sequential_in_numpy(x.shape, scalar_scale, output_shape):
        assert mine.tobytes() == want.tobytes(), (what, np.abs(mine - want).max())
        print(what, want.shape, 'restatement == reference')
    else:
        assert (np.abs(mine - want) <= bound).all(), (what, np.abs(mine - want).max(), bound.min())
        print(what, want.shape, 'restatement within the bound: max |diff| %.3g, %d of %d values differ' % (
            np.abs(mine - want).max(), int((mine != want).sum()), mine.size))


def case_contributions():
    out = {}
    for n, (in_len, out_len, scale) in enumerate(ifx.CONTRIB_CASES):
        w, i = ref.contributions(in_len, out_len, scale, ref.cubic, 4.0)
        out['w%d' % n], out['i%d' % n] = np.squeeze(w, axis=1), np.squeeze(i, axis=1)
        assert out['w%d' % n].dtype == np.float64 and out['i%d' % n].dtype == np.int32
    np.savez_compressed(os.path.join(HERE, 'imresize_contributions.npz'), **out)


def case_images():
    out = {}
    for key, shape, dtype, scalar_scale, output_shape in ifx.IMAGE_CASES:
        x = ifx.image(key)
        want = ref.imresize(x, scalar_scale=scalar_scale, output_shape=output_shape)
        assert want.ndim == x.ndim
        check_restatement(key, x, want, scalar_scale, output_shape)
        out[key] = want
    np.savez_compressed(os.path.join(HERE, 'imresize_images.npz'), **out)


def case_tiles():
    for name in ifx.TILES:
        out = {}
        for key, x, scale in ifx.tile_cases(name):
            want = ref.imresize(x, scale)
            check_restatement('%s %s' % (name, key), x, want, scale)
            for part, v in ifx.edge_views(want).items():
                out['%s_%s' % (key, part)] = v
        np.savez_compressed(os.path.join(HERE, 'imresize_tile_%s.npz' % name), **out)
    # a crop of a tile in another dtype
    x = ifx.tile_cases('T33UUB')[0][1][:120, :120].astype(np.float32)
    check_restatement('T33UUB 120 x 120 float32', x, ref.imresize(x, 2), 2)


def case_opendata():
    arrays, record = {}, {}
    for run_60, true_scale in ((False, False), (True, True)):
        with tempfile.TemporaryDirectory() as tmp:
            ifx.opendata_dir(tmp, run_60)
            buf = io.StringIO()
            with contextlib.redirect_stdout(buf):
                train, image_size = OpenDataFilesTest(tmp, run_60, ifx.SCALE, true_scale)
        tag = 'run60' if run_60 else 'run20'
        for n, a in enumerate(train):
            arrays['%s_%d' % (tag, n)] = a
        record[tag] = {'image_size': image_size, 'printed': buf.getvalue().splitlines(), 'arrays': len(train)}
    np.savez_compressed(os.path.join(HERE, 'imresize_opendata.npz'), **arrays)
    with open(os.path.join(HERE, 'imresize_opendata.json'), 'w') as f:
        json.dump(record, f, indent=1, sort_keys=True)
        f.write('\n')


def case_rmse():
    rmse = demo_rmse()
    record = {}
    for name in ifx.TILES:
        for key, gt, scale in ifx.rmse_regions(name):
            lr = downPixelAggr(gt, SCALE=scale)
            with contextlib.redirect_stdout(io.StringIO()):
                v64 = rmse(ref.imresize(lr, scale), gt)
                v32 = rmse(ref.imresize(lr.astype(np.float32), scale), gt)
            record['%s_%s' % (name, key)] = {'f64': float(v64), 'f32': float(v32), 'shape': list(gt.shape), 'scale': scale}
            print(name, key, gt.shape, v64, v32)
    with open(os.path.join(HERE, 'imresize_rmse.json'), 'w') as f:
        json.dump(record, f, indent=1, sort_keys=True)
        f.write('\n')


if __name__ == '__main__':
    case_contributions()
    case_images()
    case_opendata()
    case_tiles()
    case_rmse()
