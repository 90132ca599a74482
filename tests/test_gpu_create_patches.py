"""Training-set creation on the GPU: the downPixelAggr kernel against the reference's recorded outputs and against the numpy
restatement (EQUALITY, not a tolerance: the arithmetic is specified operation by operation), the random / test patch writers
against the reference's recorded files, and create_patches -> create_random -> train end to end.  Nothing here reads the
reference tree: its outputs are the fixtures of tests/golden/make_golden_trainset.py."""
import contextlib
import io
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import downsample_restatement as rs  # noqa: E402
import trainset_fixtures as fx  # noqa: E402

from dsen2_amd import patches  # noqa: E402

pytestmark = pytest.mark.gpu


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    if got.tobytes() != want.tobytes():
        bad = np.argwhere(got != want)
        raise AssertionError('%s: %d of %d values differ, first at %s: %r != %r (max |diff| %g)' % (
            what, len(bad), got.size, bad[0].tolist(), got[tuple(bad[0])], want[tuple(bad[0])],
            np.abs(got.astype(np.float64) - want.astype(np.float64)).max()))


def _device_f32(x, scale):
    t, dt = patches.upload_raster(x)
    return patches.down_pixel_aggr_device(t, scale, dt).cpu().numpy()


@pytest.mark.parametrize('tile', fx.TILES)
def test_kernel_equals_the_reference_fixtures_bit_for_bit(tile):
    rec = np.load(os.path.join(fx.GOLDEN, 'trainset_down_%s.npz' % tile))
    for key, x, scale in fx.down_cases(tile):
        out = patches.downPixelAggr(x, SCALE=scale)
        assert out.dtype == np.float64 and out.ndim == x.ndim          # squeezed like the reference's: a 2-D band stays 2-D
        for part, v in fx.edge_views(out).items():
            _same(v, rec['%s_%s' % (key, part)], '%s %s %s' % (tile, key, part))


@pytest.mark.parametrize('tile', fx.TILES)
def test_kernel_equals_the_restatement_on_the_whole_tiles(tile):
    """All three resolutions, uint16 and float32, SCALE 2 and 6, float64 and float32 output."""
    for key, x, scale in fx.down_cases(tile):
        want = rs.down_pixel_aggr(x, scale, rs.recorded_weights(scale))
        _same(patches.downPixelAggr(x, SCALE=scale), want, '%s %s float64' % (tile, key))
        got32 = _device_f32(x, scale)
        _same(got32.reshape(want.shape), want.astype(np.float32), '%s %s float32' % (tile, key))


@pytest.mark.parametrize('shape, scale, dtype', [((30, 42, 5), 3, np.uint16), ((30, 42, 5), 3, np.float32), ((24, 20, 11), 1, np.uint16),
                                                 ((20, 36, 19), 4, np.float32), ((12, 18, 4), 6, np.uint16), ((8, 8, 1), 2, np.float32),
                                                 ((96, 64, 3), 32, np.uint16)])
def test_kernel_at_other_scales_channel_counts_and_tiny_images(shape, scale, dtype):
    """The run-time form of the kernel (any scale <= 32, radius <= 8), channel chunks (C > 8), images smaller than a tile."""
    rng = np.random.default_rng(scale * 1000 + shape[2])
    x = rng.integers(0, 65536, shape).astype(dtype)
    if dtype == np.float32:
        x += rng.random(shape, dtype=np.float32)
    weights = patches.gaussian_weights(scale)
    want = rs.down_pixel_aggr(x, scale, weights)
    _same(patches.downPixelAggr(x, SCALE=scale), want, 'float64')
    _same(_device_f32(x, scale).reshape(want.shape), want.astype(np.float32), 'float32')


def test_kernel_at_full_tile_size_is_deterministic_and_right():
    """One synthetic 10980 x 10980 x 4 uint16 image: two runs give the same bits, and three windows (a corner on the image border,
    the interior, the opposite corner) equal the restatement."""
    n = 10980
    g = torch.Generator(device='cuda').manual_seed(20170527)
    img = torch.randint(-32768, 32768, (n, n, 4), dtype=torch.int16, device='cuda', generator=g)      # uint16 bits
    for scale in (2, 6):
        a = patches.down_pixel_aggr_device(img, scale, np.uint16)
        b = patches.down_pixel_aggr_device(img, scale, np.uint16)
        assert a.shape == (n // scale, n // scale, 4) and torch.equal(a, b)
        on, m, k = n // scale, 4, 48                         # m: output pixels of margin that hide the crop's own reflection
        for oy, ox in ((0, 0), (on // 2 - 7, on // 3 + 5), (on - k, on - k)):
            y0, y1, x0, x1 = max(oy - m, 0), min(oy + k + m, on), max(ox - m, 0), min(ox + k + m, on)
            crop = img[y0 * scale:y1 * scale, x0 * scale:x1 * scale].cpu().numpy().view(np.uint16)
            want = rs.down_pixel_aggr(crop, scale, rs.recorded_weights(scale)).astype(np.float32)
            want = want[oy - y0:oy - y0 + k, ox - x0:ox - x0 + k]
            _same(a[oy:oy + k, ox:ox + k].cpu().numpy(), want, 'scale %d window (%d, %d)' % (scale, oy, ox))
        del a, b


def _quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def test_random_patches_equal_the_reference_files(tmp_path):
    d10, d20, _ = fx.load_tile('T33UUB')
    t10, t20 = patches.upload_raster(d10), patches.upload_raster(d20)
    lr10, lr20 = (patches.down_pixel_aggr_device(t, 2, dt) for t, dt in (t10, t20))
    out = str(tmp_path) + '/'
    _quiet(patches.save_random_patches, d20, lr10, lr20, out, NR_CROP=fx.NR_CROP_20, seed=fx.SEED_20)
    assert sorted(os.listdir(out)) == ['data10.npy', 'data20.npy', 'data20_gt.npy']
    for key in ('data10', 'data20_gt', 'data20'):
        _same(np.load(out + key + '.npy'), fx.load_split('trainset_random20', key), key)
    # the same from the reference's float64 host arrays and explicit origins
    out2 = str(tmp_path / 'b') + '/'
    os.makedirs(out2)
    _quiet(patches.save_random_patches, d20, patches.downPixelAggr(d10), patches.downPixelAggr(d20), out2, NR_CROP=fx.NR_CROP_20,
           origins=fx.load_split('trainset_random20', 'origins'))
    for key in ('data10', 'data20_gt', 'data20'):
        _same(np.load(out2 + key + '.npy'), fx.load_split('trainset_random20', key), key + ' (host arrays)')


def test_random_patches60_equal_the_reference_files(tmp_path):
    m10, m20, m60 = fx.mosaic_60(*fx.load_tile('T33UUB'))
    lr = [patches.down_pixel_aggr_device(patches.upload_raster(a)[0], 6, np.uint16) for a in (m10, m20, m60)]
    out = str(tmp_path) + '/'
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        patches.save_random_patches60(m60, lr[0], lr[1], lr[2], out, NR_CROP=fx.NR_CROP_60, seed=fx.SEED_60)
    assert buf.getvalue().splitlines() == ['(8, 2, 96, 96)', '(8, 4, 96, 96)', '(8, 6, 48, 48)', '(8, 2, 16, 16)', 'Done!']
    assert sorted(os.listdir(out)) == ['data10.npy', 'data20.npy', 'data60.npy', 'data60_gt.npy']
    for key in ('data10', 'data60_gt', 'data20', 'data60'):
        _same(np.load(out + key + '.npy'), fx.load_split('trainset_random60', key), key)


def test_test_patches_equal_tiling_the_restatement(tmp_path):
    d10, d20, d60 = fx.load_tile('T49JGM')
    w2 = rs.recorded_weights(2)
    r10, r20 = (rs.down_pixel_aggr(a, 2, w2).astype(np.float32) for a in (d10, d20))
    out = str(tmp_path) + '/'
    _quiet(patches.save_test_patches, _device_f32(d10, 2), _device_f32(d20, 2), out)
    want = patches.get_test_patches(r10, r20, patchSize=128, border=4)
    for key, w in zip(('data10', 'data20'), want):
        _same(np.load(out + key + '.npy'), w, key)
    m10, m20, m60 = fx.mosaic_60(d10, d20, d60)
    w6 = rs.recorded_weights(6)
    r = [rs.down_pixel_aggr(a, 6, w6).astype(np.float32) for a in (m10, m20, m60)]
    out = str(tmp_path / '60') + '/'
    os.makedirs(out)
    _quiet(patches.save_test_patches60, _device_f32(m10, 6), _device_f32(m20, 6), _device_f32(m60, 6), out)
    want = patches.get_test_patches60(r[0], r[1], r[2], patchSize=192, border=12)
    for key, w in zip(('data10', 'data20', 'data60'), want):
        _same(np.load(out + key + '.npy'), w, key + ' (60)')


def test_unsupported_dtype_and_indivisible_device_images_are_refused():
    with pytest.raises(TypeError, match='uint16 or float32'):
        patches.downPixelAggr(np.zeros((8, 8, 1), np.float64))
    t = torch.zeros((8, 8, 2), dtype=torch.float32, device='cuda')
    with pytest.raises(ValueError, match='not a multiple of SCALE = 2'):
        patches.down_pixel_aggr_device(t[:7], 2)
    with pytest.raises(TypeError):
        patches.down_pixel_aggr_device(t, 2, np.uint16)
    # the library itself refuses what the Python layer would let through
    import ctypes
    from dsen2_amd import _lib
    out = torch.empty((4, 4, 2), dtype=torch.float32, device='cuda')
    w = (ctypes.c_double * 5)(*patches.gaussian_weights(2)[0])
    rc = _lib.load().dsen2_down_pixel_aggr(ctypes.c_void_p(t.data_ptr()), _lib.DTYPE_F32, 8, 7, 2, 2, w, 2, ctypes.c_void_p(out.data_ptr()), 0, None)
    assert rc == _lib.ERR_INVALID


def _run(args, timeout):
    r = subprocess.run([sys.executable, '-m'] + args, cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, ' '.join(args) + '\n' + r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


def test_create_patches_create_random_train_end_to_end(tmp_path):
    """tile in -> training set -> validation split -> two epochs of fine-tuning -> a checkpoint DSen2_20 loads."""
    prefix = str(tmp_path / 'data') + '/'
    tile = os.path.join(fx.GOLDEN, 'tile_T33UUB_600.npz')
    out = _run(['dsen2_amd.create_patches', tile, '--save_prefix', prefix, '--nr_crop', '96', '--seed', '11'], 300)
    assert out.splitlines()[-1] == 'Success.'
    d = os.path.join(prefix, 'train', 'tile_T33UUB_600.SAFE')
    shapes = {k: np.load(os.path.join(d, k + '.npy')).shape for k in ('data10', 'data20', 'data20_gt')}
    assert shapes == {'data10': (96, 4, 32, 32), 'data20': (96, 6, 32, 32), 'data20_gt': (96, 6, 32, 32)}
    # the crops are the ones the seed draws, cut from what the restatement computes
    d10, d20, _ = fx.load_tile('T33UUB')
    org = patches.random_origins((150, 150), 16, 96, 11)
    lr10 = rs.down_pixel_aggr(d10, 2, rs.recorded_weights(2)).astype(np.float32)
    y, x = 2 * org[17]
    _same(np.load(os.path.join(d, 'data10.npy'))[17], np.ascontiguousarray(lr10[y:y + 32, x:x + 32].transpose(2, 0, 1)), 'patch 17 of data10')
    _same(np.load(os.path.join(d, 'data20_gt.npy'))[17], np.ascontiguousarray(d20[y:y + 32, x:x + 32].transpose(2, 0, 1)).astype(np.float32),
          'patch 17 of data20_gt')

    out = _run(['dsen2_amd.create_random', '--path', prefix, '--seed', '5'], 120)
    assert 'Full no of samples: 96' in out and 'Validation samples: 9' in out
    models = tmp_path / 'models'
    out = _run(['dsen2_amd.train', '--path', prefix, '--epochs', '2', '--batch_size', '16', '--out', str(models), '--seed', '0'], 600)
    log = (models / 's2_038__lr_1.0e-04.txt').read_text().splitlines()
    assert len(log) == 2
    for line in log:
        loss, val = float(line.split('loss ')[1].split(',')[0]), float(line.split('valid: ')[1].split(',')[0])
        assert np.isfinite(loss) and np.isfinite(val), line

    # DSen2_20 picks the .npy up in place of the .hdf5 of the same name
    os.replace(str(models / 's2_038_lr_1e-04.npy'), str(models / 's2_032_lr_1e-04.npy'))
    from dsen2_amd import supres
    keep = supres.MDL_PATH
    try:
        supres.MDL_PATH = str(models) + '/'
        supres.clear_model_cache()
        sr = _quiet(supres.DSen2_20, d10, d20)
    finally:
        supres.MDL_PATH = keep
        supres.clear_model_cache()
    assert sr.shape == (600, 600, 6) and np.isfinite(sr).all()
