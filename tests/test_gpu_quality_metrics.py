"""UIQ and SAM on the GPU (csrc/quality_metrics.hip) against the numpy restatement (tests/quality_restatement.py): the quality map
bit for bit, the fused sums within the bound of two summation orders, the repeatability of their bits, the fused bicubic forms
against resize, store, then measure (the same bits), and create_patches -> train --predict -> evaluate --uiq --sam end to end.

Bounds.  uiq_sums: the kernel and numpy add the same n numbers q in two orders; each order is within n 2^-53 sum |q| of the exact
sum to first order, so the two differ by at most 2 n 2^-53 sum |q|.  sam_sums: the cosine is bit-identical by construction; 16
half-ulps cover two acos implementations and the conversion to degrees, n the order of n non-negative terms: (n + 16) 2^-53
relative.  Neither figure was measured."""
import functools
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import imresize_restatement as rs  # noqa: E402
import quality_restatement as qr  # noqa: E402
import trainset_fixtures as fx  # noqa: E402

from dsen2_amd import imresize as ir  # noqa: E402
from dsen2_amd import metrics, weights  # noqa: E402

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -53
TH, TW = (int(v) for v in re.search(r'constexpr int kUiqTileH = (\d+), kUiqTileW = (\d+);',
                                    open(os.path.join(ROOT, 'dsen2_amd', 'csrc', 'quality_metrics.hip')).read()).groups())
SHAPES = [(8, 8, 1), (9, 23, 2), (64, 100, 13), (300, 257, 6), (TH + 7, TW + 7, 6), (TH + 8, TW + 6, 6), (2 * TH + 8, TW + 8, 1)]
DTYPES = [(np.float32, np.float32), (np.float64, np.float32), (np.float32, np.float64), (np.float32, np.uint16)]
MANY_TILES = (1100, 2100, 1)          # 69 x 66 tiles of windows: more than the 4096 workgroups of a launch, so a workgroup walks two


@functools.lru_cache(maxsize=None)
def _pair(shape, dx, dg):
    rng = np.random.RandomState(shape[0] * 31 + shape[1] + len(shape))
    gt = rng.randint(1, 12000, size=shape).astype(dg)
    x = (gt.astype(np.float64) + rng.normal(0, 80, size=shape)).astype(dx)
    x.setflags(write=False)
    gt.setflags(write=False)
    return x, gt


@functools.lru_cache(maxsize=None)
def _reference_map(shape, dx, dg, block):
    q = qr.uiq_map(*_pair(shape, dx, dg), B=block)
    q.setflags(write=False)
    return q


def test_the_tile_the_shapes_are_built_around():
    assert (TH, TW) == (16, 32)


@pytest.mark.parametrize('dx, dg', DTYPES)
@pytest.mark.parametrize('shape, block', [(s, 8) for s in SHAPES] + [((64, 100, 13), 3), ((40, 50, 2), 16), ((9, 23, 2), 2)])
def test_uiq_map_equals_the_restatement_bit_for_bit(shape, block, dx, dg):
    x, gt = _pair(shape, dx, dg)
    want = _reference_map(shape, dx, dg, block)
    got = metrics.uiq_map(x, gt, block)
    assert got.dtype == np.float64 and got.shape == want.shape == (shape[0] - block + 1, shape[1] - block + 1, shape[2])
    assert got.tobytes() == want.tobytes(), np.abs(got - want).max()


def test_flat_and_all_zero_windows_take_their_branches_on_the_gpu():
    x, gt = qr.planted()
    taken = {}
    want = qr.uiq_map(x, gt, 8, taken)
    assert taken == {'flat': 64, 'one': 30}
    got = metrics.uiq_map(x, gt)
    assert got.shape == (33, 30) and got.tobytes() == want.tobytes()
    assert (got[22:27, 20:26] == 1.0).all() and got[5, 3] == want[5, 3] != 1.0
    sums = metrics.uiq_sums(x, gt)
    assert sums.shape == (1, 2) and sums[0, 1] == 33 * 30
    assert abs(sums[0, 0] - want.sum()) <= 2 * want.size * EPS * np.abs(want).sum()
    band, mean = metrics.UIQ(x, gt)
    assert band.shape == (1,) and band[0] == sums[0, 0] / sums[0, 1] == mean


@pytest.mark.parametrize('shape, dx, dg, block', [((9, 23, 2), np.float32, np.float32, 8), ((64, 100, 13), np.float64, np.float32, 8),
                                                  ((300, 257, 6), np.float32, np.uint16, 8), ((2 * TH + 8, TW + 8, 1), np.float32, np.float64, 8),
                                                  ((64, 100, 13), np.float32, np.float32, 3), (MANY_TILES, np.float32, np.float32, 8)])
def test_uiq_sums_are_within_the_bound_and_repeat_their_bits(shape, dx, dg, block):
    x, gt = _pair(shape, dx, dg)
    q = _reference_map(shape, dx, dg, block)
    n = q.shape[0] * q.shape[1]
    a = metrics.uiq_sums(x, gt, block)
    assert a.dtype == np.float64 and a.shape == (shape[2], 2)
    assert (a[:, 1] == n).all()
    for c in range(shape[2]):
        want, bound = q[:, :, c].sum(), 2 * n * EPS * np.abs(q[:, :, c]).sum()
        print('uiq_sums %r band %d: |difference| %.3g, bound %.3g' % (shape, c, abs(a[c, 0] - want), bound))
        assert abs(a[c, 0] - want) <= bound
    assert metrics.uiq_sums(x, gt, block).tobytes() == a.tobytes()                            # the same bits on every run
    tx = torch.from_numpy(np.array(x)).cuda()
    assert metrics.uiq_sums(tx, gt, block).tobytes() == a.tobytes()                           # device tensor or host array
    band, mean = metrics.UIQ(x, gt, block)
    assert band.tobytes() == (a[:, 0] / a[:, 1]).tobytes() and mean == float(np.mean(band))
    if shape == MANY_TILES:          # the workgroups' second tiles, in the map as well
        assert metrics.uiq_map(x, gt, block).tobytes() == q.tobytes()


@pytest.mark.parametrize('shape, dx, dg, zeros', [((5, 3, 1), np.float32, np.float32, 0), ((50, 70, 6), np.float32, np.uint16, 2),
                                                  ((257, 129, 13), np.float64, np.float32, 0), ((50, 70, 6), np.float32, np.float64, 0)])
def test_sam_sums_count_exactly_and_agree_with_the_restatement(shape, dx, dg, zeros):
    x, gt = (np.array(a) for a in _pair(shape, dx, dg))
    if zeros:
        gt[7, 11] = 0
        x[31, 69] = 0
    want, n = qr.sam_sums(x, gt)
    assert n == shape[0] * shape[1] - zeros
    a = metrics.sam_sums(x, gt)
    assert a.dtype == np.float64 and a.shape == (2,) and a[1] == n
    print('sam_sums %r: relative difference %.3g, allowance %.3g' % (shape, abs(a[0] - want) / want if want else 0.0, (n + 16) * EPS))
    assert abs(a[0] - want) <= (n + 16) * EPS * want
    assert metrics.sam_sums(x, gt).tobytes() == a.tobytes()
    assert metrics.sam_sums(torch.from_numpy(x).cuda(), gt).tobytes() == a.tobytes()
    assert metrics.SAM(x, gt) == a[0] / a[1]


def _stored(lr, scale):
    t = torch.from_numpy(lr.view(np.int16) if lr.dtype == np.uint16 else lr).cuda()
    up = ir.imresize_device(t, scale)
    return up if up.dim() == 3 else up[:, :, None]


@pytest.mark.parametrize('shape, dtype, scale', [((40, 33, 2), np.float64, 6), ((90, 120, 6), np.uint16, 2), ((31, 57), np.float32, 2)])
def test_fused_bicubic_sums_are_the_bits_of_resize_store_measure(shape, dtype, scale):
    rng = np.random.RandomState(shape[0] * 7 + shape[1])
    lr = rng.randint(1, 12000, size=shape).astype(dtype)
    up = rs.imresize(lr, scale)
    gt = (up + rng.normal(0, 60, size=up.shape)).astype(np.float32)
    gt3 = gt if gt.ndim == 3 else gt[:, :, None]
    stored = _stored(lr, scale)
    assert stored.cpu().numpy().tobytes() == up.tobytes()                  # enlargements: the resampler is bit-exact
    for block in (8, 5):
        fused = metrics.bicubic_uiq_sums(lr, gt, scale, block)
        assert fused.tobytes() == metrics.uiq_sums(stored, gt3, block).tobytes()
        assert fused.tobytes() == metrics.bicubic_uiq_sums(lr, gt, scale, block).tobytes()
        assert (fused[:, 1] == (up.shape[0] - block + 1) * (up.shape[1] - block + 1)).all()
    fused = metrics.bicubic_sam_sums(lr, gt, scale)
    assert fused.tobytes() == metrics.sam_sums(stored, gt3).tobytes() and fused[1] == up.shape[0] * up.shape[1]
    band, mean = metrics.bicubic_UIQ(lr, gt, scale)
    assert band.tobytes() == metrics.UIQ(stored, gt3)[0].tobytes() and metrics.bicubic_SAM(lr, gt, scale) == metrics.SAM(stored, gt3)
    want, n = qr.sam_sums(up, gt)
    assert abs(fused[0] - want) <= (n + 16) * EPS * want


def test_the_fused_loader_resamples_along_rows_as_well():
    """The baseline's second pass runs along the columns (equal scales: axis 0 first); a pass along the rows goes through the
    loader's other branch."""
    rng = np.random.RandomState(9)
    mid = torch.from_numpy(rng.randint(1, 12000, size=(21, 45, 3)).astype(np.float64)).cuda()
    taps = ir.device_taps(21, 42, 2.0, mid.device)
    stored = ir.resize_axis_device(mid, 0, 42, taps)
    gt = (stored + 50 * torch.randn(stored.shape, dtype=torch.float64, device=mid.device, generator=torch.Generator(mid.device).manual_seed(2))).to(torch.float32)
    a = metrics.resample_quality_sums_device(mid, 0, 42, taps, gt, 8)
    assert a.cpu().numpy().tobytes() == metrics.uiq_sums_device(stored, gt, 8).cpu().numpy().tobytes()
    b = metrics.resample_quality_sums_device(mid, 0, 42, taps, gt)
    assert b.cpu().numpy().tobytes() == metrics.sam_sums_device(stored, gt).cpu().numpy().tobytes()


def _run(args, timeout):
    r = subprocess.run([sys.executable, '-m'] + args, cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, ' '.join(args) + '\n' + r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


def test_create_predict_evaluate_with_uiq_and_sam(tmp_path):
    tile = os.path.join(fx.GOLDEN, 'tile_T33UUB_600.npz')
    prefix = str(tmp_path / 'data') + '/'
    out = _run(['dsen2_amd.create_patches', tile, '--save_prefix', prefix, '--test_data', '--roi_x_y', '0,72,575,359'], 300)
    assert out.splitlines()[-1] == 'Success.'
    name = 'tile_T33UUB_600.SAFE'
    d = os.path.join(prefix, 'test', name)
    ckpt = str(tmp_path / 's2_999_lr_1e-04.npy')
    np.save(ckpt, weights.random_he_uniform(10, 6, 6, 128, seed=5))
    _run(['dsen2_amd.train', '--predict', ckpt, '--path', prefix], 600)
    out_json = str(tmp_path / 'scores.json')
    out = _run(['dsen2_amd.evaluate', '--path', prefix, '--model_nr', 's2_999_', '--json', out_json, '--uiq', '--sam'], 300)
    rec = json.load(open(out_json))
    r = rec['tiles'][name]
    pred = np.load(os.path.join(d, 's2_999_-predict.npy'))
    gt = np.load(os.path.join(d, 'no_tiling', 'data20_gt.npy'))
    lr = np.load(os.path.join(d, 'no_tiling', 'data20.npy'))
    assert pred.shape == gt.shape == (144, 288, 6)
    band, mean = metrics.UIQ(pred, gt)
    assert r['dsen2']['band_uiq'] == band.tolist() and r['dsen2']['uiq'] == mean
    s = metrics.sam_sums(pred, gt)
    assert r['dsen2']['sam'] == metrics.SAM(pred, gt) == s[0] / s[1] and r['dsen2']['sam_pixels'] == int(s[1])
    band, mean = metrics.bicubic_UIQ(lr, gt, 2)
    assert r['bicubic']['band_uiq'] == band.tolist() and r['bicubic']['uiq'] == mean
    assert r['bicubic']['sam'] == metrics.bicubic_SAM(lr, gt, 2)
    assert rec['mean']['bicubic']['uiq'] == mean and rec['mean']['dsen2']['sam'] == r['dsen2']['sam']
    assert np.isfinite(r['dsen2']['band_uiq']).all() and 0 < r['bicubic']['uiq'] <= 1 and 0 <= r['bicubic']['sam'] < 90
    lines = out.splitlines()
    assert 'DSen2 SAM [deg]: {:.4f}'.format(r['dsen2']['sam']) in lines and 'Bicubic SAM [deg]: {:.4f}'.format(r['bicubic']['sam']) in lines
    assert [ln.split() for ln in lines if 'UIQ' in ln] == [['RMSE', 'SRE', '[dB]', 'UIQ'] * 2] * 2
    # the values every run printed before are the same, and without the flags nothing of this is printed
    plain_json = str(tmp_path / 'plain.json')
    plain = _run(['dsen2_amd.evaluate', '--path', prefix, '--model_nr', 's2_999_', '--json', plain_json], 300)
    assert 'UIQ' not in plain and 'SAM' not in plain
    p = json.load(open(plain_json))['tiles'][name]
    for k in ('dsen2', 'bicubic'):
        assert sorted(p[k]) == ['band_rmse', 'band_sre', 'rmse'] and all(p[k][key] == r[k][key] for key in p[k])
