"""The evaluation step on the GPU: the per-band error sums (alone and fused into the second resampling pass) against numpy's
float64, and create_patches --test_data -> train --predict -> evaluate end to end, with the bicubic baseline against the values the
reference computed (tests/golden/imresize_rmse.json).

Tolerance of the reductions: the sums add non-negative float64 terms in another order than numpy's pairwise one; either order is
within about log2(n) 2^-53 ~ 3e-15 of the exact sum, relatively.  1e-12 covers that with margin (and nothing else)."""
import contextlib
import io
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import downsample_restatement as ds  # noqa: E402
import imresize_fixtures as ifx  # noqa: E402
import imresize_restatement as rs  # noqa: E402
import trainset_fixtures as fx  # noqa: E402

from dsen2_amd import metrics, patches, weights  # noqa: E402
from dsen2_amd.imresize import imresize_device  # noqa: E402

pytestmark = pytest.mark.gpu
RTOL = 1e-12
RMSE_GATE_NORMALISED = 1e-4                 # BASELINE.md §2 (fp32, normalised domain)


def _quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def _numpy_scores(x, gt):
    diff = x.astype(np.float64) - gt.astype(np.float64)
    if diff.ndim == 2:
        diff, gt = diff[:, :, None], gt[:, :, None]
    mse = np.array([np.mean(np.power(diff[:, :, c], 2)) for c in range(diff.shape[2])])
    mean_gt = np.array([np.mean(gt[:, :, c].astype(np.float64)) for c in range(diff.shape[2])])
    return np.sqrt(mse), 10 * np.log10(mean_gt ** 2 / mse), np.sqrt(np.mean(np.power(diff, 2)))


@pytest.mark.parametrize('shape, dx, dg', [((300, 300, 6), np.float32, np.float32), ((257, 129, 6), np.float64, np.float32),
                                           ((64, 100, 2), np.float32, np.float64), ((91, 37, 13), np.float64, np.float64),
                                           ((50, 70), np.float32, np.float32), ((5, 3, 1), np.float32, np.float32),
                                           ((1200, 1100, 6), np.float32, np.uint16)])
def test_band_errors_agree_with_numpy_and_repeat_their_bits(shape, dx, dg, capsys):
    rng = np.random.RandomState(shape[0] + shape[1])
    gt = rng.randint(1, 12000, size=shape).astype(dg)
    x = (gt.astype(np.float64) + rng.normal(0, 80, size=shape)).astype(dx)
    rmse, sre, total = _numpy_scores(x, gt)
    got_rmse, got_sre = metrics.band_errors(x, gt)
    print('band_errors %r: max relative difference rmse %.3g, sre %.3g' % (shape, np.abs(got_rmse / rmse - 1).max(), np.abs(got_sre / sre - 1).max()))
    np.testing.assert_allclose(got_rmse, rmse, rtol=RTOL, atol=0)
    np.testing.assert_allclose(got_sre, sre, rtol=RTOL, atol=0)
    a, b = metrics.error_sums(x, gt), metrics.error_sums(x, gt)
    assert a.dtype == np.float64 and a.shape == (rmse.size, 3) and a.tobytes() == b.tobytes()
    assert (a[:, 2] == shape[0] * shape[1]).all()
    np.testing.assert_allclose(a[:, 1], gt.astype(np.float64).reshape(-1, rmse.size).sum(axis=0), rtol=RTOL)
    # device tensors give the same bits as host arrays
    tx = torch.from_numpy(x).cuda()
    c = metrics.error_sums(tx, gt)
    assert c.tobytes() == a.tobytes()
    capsys.readouterr()
    value = metrics.RMSE(x, gt)
    assert capsys.readouterr().out == 'RMSE: {:.4f}\n'.format(total)
    assert abs(value - total) <= RTOL * total


@pytest.mark.parametrize('shape, dtype, scale', [((150, 150, 6), np.float32, 2), ((40, 33, 2), np.float64, 6), ((64, 48, 13), np.float32, 2),
                                                 ((31, 57), np.float32, 2), ((90, 120, 6), np.uint16, 2), ((120, 96, 3), np.float32, 0.5)])
def test_fused_bicubic_errors_agree_with_resize_then_reduce(shape, dtype, scale):
    rng = np.random.RandomState(shape[0] * 7 + shape[1])
    lr = rng.randint(1, 12000, size=shape).astype(dtype)
    up = rs.imresize(lr, scale)
    gt = (up + rng.normal(0, 60, size=up.shape)).astype(np.float32)
    rmse, sre, _ = _numpy_scores(up, gt)
    fused = metrics.bicubic_error_sums(lr, gt, scale)
    assert fused.tobytes() == metrics.bicubic_error_sums(lr, gt, scale).tobytes()              # the same bits on every run
    got_rmse, got_sre, _ = metrics.scores(fused)
    np.testing.assert_allclose(got_rmse, rmse, rtol=RTOL, atol=0)
    np.testing.assert_allclose(got_sre, sre, rtol=RTOL, atol=0)
    # resize, store, then reduce: the same terms in another order
    t = torch.from_numpy(lr.view(np.int16) if dtype == np.uint16 else lr).cuda()
    stored = imresize_device(t, scale)
    two_step = metrics.error_sums(stored if stored.dim() == 3 else stored[:, :, None], gt if gt.ndim == 3 else gt[:, :, None])
    np.testing.assert_allclose(fused, two_step, rtol=RTOL, atol=0)
    r2, s2 = metrics.bicubic_errors(lr, gt, scale)
    assert r2.tobytes() == got_rmse.tobytes() and s2.tobytes() == got_sre.tobytes()
    with pytest.raises(ValueError, match='ground truth of shape'):
        metrics.bicubic_error_sums(lr, gt[:-1], scale)


@pytest.mark.parametrize('tile', fx.TILES)
def test_bicubic_baseline_equals_the_reference_values(tile):
    """RMSE(imresize(downPixelAggr(gt), s), gt) as testing/demoDSen2.py prints it, on the regions create_patches keeps."""
    rec = json.load(open(os.path.join(ifx.GOLDEN, 'imresize_rmse.json')))
    for key, gt, scale in ifx.rmse_regions(tile):
        want = rec['%s_%s' % (tile, key)]
        assert want['shape'] == list(gt.shape) and want['scale'] == scale
        lr64 = patches.downPixelAggr(gt, SCALE=scale)
        for kind, lr in (('f64', lr64), ('f32', lr64.astype(np.float32))):
            total = metrics.scores(metrics.bicubic_error_sums(lr, gt, scale))[2]
            print('%s %s %s: %.17g (reference %.17g)' % (tile, key, kind, total, want[kind]))
            assert abs(total - want[kind]) <= RTOL * want[kind], (tile, key, kind)
            assert '{:.4f}'.format(total) == '{:.4f}'.format(want[kind])


def _run(args, timeout):
    r = subprocess.run([sys.executable, '-m'] + args, cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, ' '.join(args) + '\n' + r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


def _oracle_prediction(lr, flat, run_60):
    """The float64 oracle pipeline on the downsampled images: oracle tiling + up-sampling, / 2000, C oracle CNN, oracle
    recomposition, * 2000 (as conftest.oracle_dsen2_tile does for the inference entry, with the test set's patch geometry)."""
    from oracle import c_oracle, patches_oracle as po
    if run_60:
        p, border = po.get_test_patches60(lr[0], lr[1], lr[2], patchSize=192, border=12, f32_coords=True), 12
    else:
        p, border = po.get_test_patches(lr[0], lr[1], patchSize=128, border=4, f32_coords=True), 4
    pred = c_oracle.forward([a / np.float32(2000) for a in p], flat, 6, 128)
    img = _quiet(po.recompose_images, pred, border=border, size=lr[0].shape)
    return img.astype(np.float64) * 2000


def _flow(tmp_path, tile_file, images, run_60, rmse_key, roi=None):
    """create_patches --test_data -> train --predict -> evaluate in tmp_path; returns (prediction, evaluate's JSON record)."""
    from dsen2_amd import train
    from dsen2_amd.DSen2Net import s2model
    prefix = str(tmp_path / 'data') + '/'
    flags = ['--run_60'] if run_60 else []
    out = _run(['dsen2_amd.create_patches', tile_file, '--save_prefix', prefix, '--test_data'] + flags + (['--roi_x_y', roi] if roi else []), 300)
    assert out.splitlines()[-1] == 'Success.'
    folder = 'test60' if run_60 else 'test'
    name = os.path.splitext(os.path.basename(tile_file))[0] + '.SAFE'
    d = os.path.join(prefix, folder, name)
    bands = ((4, None, None), (6, None, None), (2, None, None)) if run_60 else ((4, None, None), (6, None, None))
    cin, cout = (12, 2) if run_60 else (10, 6)
    flat = weights.random_he_uniform(cin, cout, 6, 128, seed=5)
    ckpt = str(tmp_path / 's2_999_lr_1e-04.npy')
    np.save(ckpt, flat)
    out = _run(['dsen2_amd.train', '--predict', ckpt, '--path', prefix] + flags, 600)
    for line in ('Changing the model number to: s2_999_', 'Timer started.', 'Predicting: %s.' % name, 'Writing to file...'):
        assert line in out.splitlines(), line
    assert 'Elapsed time: ' in out
    written = np.load(os.path.join(d, 's2_999_-predict.npy'))

    # exactly what the reference's predict branch computes from the same files
    model = s2model(bands, num_layers=6, feature_size=128)
    model.set_weights_flat(flat)
    train_x, image_size = _quiet(patches.OpenDataFilesTest, d, run_60, train.SCALE)
    size = (image_size[1], image_size[0])
    want = _quiet(patches.recompose_images, model.predict(train_x, batch_size=8), border=12 if run_60 else 4, size=size) * train.SCALE
    assert written.dtype == want.dtype == np.float32 and written.shape == want.shape and written.tobytes() == want.tobytes()
    gt = np.load(os.path.join(d, 'no_tiling', ('data60' if run_60 else 'data20') + '_gt.npy'))
    assert written.shape == gt.shape and np.isfinite(written).all()

    if images is not None:
        # the float64 oracle pipeline, from the restatement of the downsampler
        scale = 6 if run_60 else 2
        lr = [ds.down_pixel_aggr(a, scale, ds.recorded_weights(scale)).astype(np.float32) for a in images]
        from oracle import dsen2_oracle as do
        err = do.rmse(written, _oracle_prediction(lr, flat, run_60)) / 2000
        print('%s predict: normalised rmse against the float64 oracle %.3e' % (folder, err))
        assert err < RMSE_GATE_NORMALISED

    out_json = str(tmp_path / 'scores.json')
    out = _run(['dsen2_amd.evaluate', '--path', prefix, '--model_nr', 's2_999_', '--json', out_json] + flags, 300).splitlines()
    rec = json.load(open(out_json))
    r = rec['tiles'][name]
    i = out.index(name)
    assert out[i:i + 5] == [name, 'DSen2:', 'RMSE: {:.4f}'.format(r['dsen2']['rmse']), 'Bicubic:', 'RMSE: {:.4f}'.format(r['bicubic']['rmse'])]
    # the DSen2 line is the demo's RMSE of the written prediction
    diff = written.astype(np.float64) - gt.astype(np.float64)
    assert abs(r['dsen2']['rmse'] - np.sqrt(np.mean(np.power(diff, 2)))) <= RTOL * r['dsen2']['rmse']
    if rmse_key:
        ref = json.load(open(os.path.join(ifx.GOLDEN, 'imresize_rmse.json')))[rmse_key]['f32']       # no_tiling/ holds float32
        print('%s bicubic: %.17g (reference %.17g)' % (folder, r['bicubic']['rmse'], ref))
        assert out[i + 4] == 'RMSE: {:.4f}'.format(ref)
        assert abs(r['bicubic']['rmse'] - ref) <= RTOL * ref
    # without a prediction file the baseline is still printed
    os.remove(os.path.join(d, 's2_999_-predict.npy'))
    out = _run(['dsen2_amd.evaluate', '--path', prefix, '--model_nr', 's2_999_'] + flags, 300).splitlines()
    i = out.index(name)
    assert out[i:i + 3] == [name, 'Bicubic:', 'RMSE: {:.4f}'.format(r['bicubic']['rmse'])] and 'DSen2:' not in out
    return written, rec


def test_create_predict_evaluate_end_to_end(tmp_path):
    tile = os.path.join(fx.GOLDEN, 'tile_T33UUB_600.npz')
    d10, d20, _ = fx.load_tile('T33UUB')
    written, rec = _flow(tmp_path, tile, (d10, d20), False, 'T33UUB_d20_x2')
    assert written.shape == (300, 300, 6)
    r = rec['tiles']['tile_T33UUB_600.SAFE']
    assert len(r['bicubic']['band_rmse']) == 6 and len(r['dsen2']['band_sre']) == 6 and rec['mean']['bicubic']['tiles'] == 1


def test_a_non_square_region_predicts_to_the_ground_truths_shape(tmp_path):
    """--roi_x_y 0,72,575,359 (snapped to 36: 576 wide, 288 high): roi.json gives [width, height] = [288, 144]; the prediction is
    144 rows x 288 columns like no_tiling/data20_gt.npy."""
    tile = os.path.join(fx.GOLDEN, 'tile_T33UUB_600.npz')
    written, rec = _flow(tmp_path, tile, None, False, None, roi='0,72,575,359')
    assert written.shape == (144, 288, 6)


def test_the_same_flow_at_60_m_on_the_mirrored_mosaic(tmp_path):
    m10, m20, m60 = fx.mosaic_60(*fx.load_tile('T33UUB'))
    tile = str(tmp_path / 'mosaic_T33UUB.npz')
    np.savez(tile, data10=m10, data20=m20, data60=m60)
    written, rec = _flow(tmp_path, tile, (m10, m20, m60), True, 'T33UUB_mosaic_d60_x6')
    assert written.shape == (192, 192, 2)
