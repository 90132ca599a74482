"""SSIM on the GPU (csrc/ssim.hip) against the numpy restatement (tests/ssim_restatement.py): the map bit for bit, the fused sums
within the bound of a summation order, the repeatability and the symmetry of their bits, the fused bicubic form against resize,
store, then measure (the same bits), ERGAS / PSNR / SSIM from host arrays and device tensors, `evaluate --ssim --ergas --psnr` end
to end, and the refusals through Python.

Bound of ssim_sums: the kernel adds the n numbers q of a band in an order of its own; any order of n - 1 additions is within
n 2^-53 sum |q| of the exact sum, which math.fsum of the restatement's map gives (for n = 1 the kernel's sum is q itself).  The
bound comes from the number format alone; each test prints the difference it found before it asserts."""
import functools
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import imresize_restatement as rs  # noqa: E402
import ssim_restatement as sr  # noqa: E402

from dsen2_amd import imresize as ir  # noqa: E402
from dsen2_amd import metrics  # noqa: E402

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -53
L = 1e4
# one window; exactly one tile of 16 x 32 windows; one window into the next tile both ways; ragged; seven tile columns and one row
# of two windows; and the smallest and largest window
CASES = [((11, 11, 1), 11), ((26, 42, 6), 11), ((27, 43, 2), 11), ((40, 70, 3), 11), ((12, 200, 1), 11), ((33, 47, 2), 3), ((33, 47, 2), 15)]
DTYPES = [(np.float32, np.float32), (np.float32, np.float64), (np.float64, np.float32)]


@functools.lru_cache(maxsize=None)
def _pair(shape, dx, dy, kind='noisy'):
    """Integer-valued reflectance-like values 35..13109; anti: y = L - x, so that negative q occurs; constant: two flat images."""
    rng = np.random.RandomState(shape[0] * 31 + shape[1] + shape[2])
    y = rng.randint(35, 13110, size=shape).astype(np.float64)
    if kind == 'noisy':
        x = np.clip(y + np.rint(rng.normal(0, 300, size=shape)), 35, 13109)
    elif kind == 'anti':
        x, y = y, L - y
    else:
        x, y = np.full(shape, 4321.0), np.full(shape, 4000.0)
    x, y = x.astype(dx), y.astype(dy)
    x.setflags(write=False)
    y.setflags(write=False)
    return x, y


@functools.lru_cache(maxsize=None)
def _reference_map(shape, dx, dy, win, kind='noisy'):
    q = sr.ssim_map(*_pair(shape, dx, dy, kind), data_range=L, win_size=win)
    q.setflags(write=False)
    return q


@pytest.mark.parametrize('dx, dy', DTYPES)
@pytest.mark.parametrize('shape, win', CASES)
def test_ssim_map_equals_the_restatement_bit_for_bit(shape, win, dx, dy):
    x, y = _pair(shape, dx, dy)
    want = _reference_map(shape, dx, dy, win)
    got = metrics.ssim_map(x, y, L, win)
    assert got.dtype == np.float64 and got.shape == want.shape == (shape[0] - win + 1, shape[1] - win + 1, shape[2])
    assert got.tobytes() == want.tobytes(), np.abs(got - want).max()


@pytest.mark.parametrize('kind', ['anti', 'constant'])
@pytest.mark.parametrize('shape, win', [((27, 43, 2), 11), ((40, 70, 3), 11), ((33, 47, 2), 15)])
def test_anti_correlated_and_constant_pairs(shape, win, kind):
    x, y = _pair(shape, np.float32, np.float32, kind)
    want = _reference_map(shape, np.float32, np.float32, win, kind)
    got = metrics.ssim_map(x, y, L, win)
    assert got.tobytes() == want.tobytes(), np.abs(got - want).max()
    if kind == 'anti':
        assert got.min() < 0
    else:
        # flat images: q is the luminance term times (2 s12 + C2) / (s1 + s2 + C2), where s1, s2, s12 are the rounding left of
        # exx - mx^2 (a few ulps of 1.9e7, below 1e-6) against C2 = 9e4: well within 1e-9 of 1
        lum = (2 * 4321.0 * 4000.0 + 1e4) / (4321.0 ** 2 + 4000.0 ** 2 + 1e4)
        assert np.abs(got - lum).max() <= 1e-9
    sums = metrics.ssim_sums(x, y, L, win)
    n = want.shape[0] * want.shape[1]
    for c in range(shape[2]):
        assert sums[c, 1] == n and abs(sums[c, 0] - math.fsum(want[:, :, c].ravel())) <= n * EPS * np.abs(want[:, :, c]).sum()


@pytest.mark.parametrize('dx, dy', DTYPES)
@pytest.mark.parametrize('shape, win', CASES)
def test_ssim_sums_are_within_the_bound_repeat_their_bits_and_are_symmetric(shape, win, dx, dy):
    x, y = _pair(shape, dx, dy)
    q = _reference_map(shape, dx, dy, win)
    n = q.shape[0] * q.shape[1]
    a = metrics.ssim_sums(x, y, L, win)
    assert a.dtype == np.float64 and a.shape == (shape[2], 2)
    assert n == (shape[0] - win + 1) * (shape[1] - win + 1) and (a[:, 1] == n).all()
    for c in range(shape[2]):
        want, bound = math.fsum(q[:, :, c].ravel()), n * EPS * np.abs(q[:, :, c]).sum()
        print('ssim_sums %r win %d band %d: |difference| %.3g, bound %.3g' % (shape, win, c, abs(a[c, 0] - want), bound))
        assert abs(a[c, 0] - want) <= bound
    assert metrics.ssim_sums(x, y, L, win).tobytes() == a.tobytes()                     # the same bits on every run
    assert metrics.ssim_sums(y, x, L, win).tobytes() == a.tobytes()                     # symmetric operation by operation
    band, mean = metrics.SSIM(x, y, L, win)
    assert band.tobytes() == (a[:, 0] / a[:, 1]).tobytes() and mean == float(np.mean(band))
    assert metrics.ssim_scores(a)[0].tobytes() == band.tobytes()


def _stored(lr, scale):
    t = torch.from_numpy(lr.view(np.int16) if lr.dtype == np.uint16 else lr).cuda()
    up = ir.imresize_device(t, scale)
    return up if up.dim() == 3 else up[:, :, None]


@pytest.mark.parametrize('gt_dtype', [np.float32, np.float64])
@pytest.mark.parametrize('shape, dtype, scale', [((14, 22, 6), np.float32, 2), ((14, 22, 6), np.uint16, 2), ((5, 8, 2), np.float32, 6)])
def test_fused_bicubic_sums_are_the_bits_of_resize_store_measure(shape, dtype, scale, gt_dtype):
    rng = np.random.RandomState(shape[0] * 7 + shape[1])
    lr = rng.randint(35, 13110, size=shape).astype(dtype)
    up = rs.imresize(lr, scale)
    gt = np.clip(np.rint(up + rng.normal(0, 200, size=up.shape)), 35, 13109).astype(gt_dtype)
    stored = _stored(lr, scale)
    assert stored.cpu().numpy().tobytes() == up.tobytes()                  # enlargements: the resampler is bit-exact
    for win in (11, 5):
        fused = metrics.bicubic_ssim_sums(lr, gt, scale, L, win)
        assert fused.tobytes() == metrics.ssim_sums(stored, gt, L, win).tobytes()
        assert fused.tobytes() == metrics.bicubic_ssim_sums(lr, gt, scale, L, win).tobytes()
        assert (fused[:, 1] == (up.shape[0] - win + 1) * (up.shape[1] - win + 1)).all()
        q = sr.ssim_map(up, gt, L, win)
        for c in range(shape[2]):
            assert abs(fused[c, 0] - math.fsum(q[:, :, c].ravel())) <= q.shape[0] * q.shape[1] * EPS * np.abs(q[:, :, c]).sum()
    band, mean = metrics.bicubic_SSIM(lr, gt, scale, L)
    want = metrics.SSIM(stored, gt, L)
    assert band.tobytes() == want[0].tobytes() and mean == want[1]
    # both axes of the loader: the second pass of the baseline runs along the columns; here each pass is fused in turn
    mid0 = torch.from_numpy(np.ascontiguousarray(lr.astype(np.float64))).cuda()
    for axis in (0, 1):
        out_len = shape[axis] * scale
        taps = ir.device_taps(shape[axis], out_len, float(scale), mid0.device)
        passed = ir.resize_axis_device(mid0, axis, out_len, taps)
        ref = torch.clamp(torch.round(passed + 150 * torch.randn(passed.shape, dtype=torch.float64, device=mid0.device,
                                                                 generator=torch.Generator(mid0.device).manual_seed(3))), 35, 13109)
        ref = ref.to(torch.float32 if gt_dtype == np.float32 else torch.float64)
        win = 5 if min(passed.shape[:2]) < 11 else 11
        a = metrics.resample_ssim_sums_device(mid0, axis, out_len, taps, ref, L, win)
        assert a.cpu().numpy().tobytes() == metrics.ssim_sums_device(passed, ref, L, win).cpu().numpy().tobytes()


def test_numpy_arrays_and_device_tensors_agree():
    x, y = _pair((40, 70, 3), np.float32, np.float32)
    tx, ty = torch.from_numpy(np.array(x)).cuda(), torch.from_numpy(np.array(y)).cuda()
    band, mean = metrics.SSIM(x, y, L)
    for a, b in ((tx, ty), (tx, y), (x, ty)):
        got = metrics.SSIM(a, b, L)
        assert got[0].tobytes() == band.tobytes() and got[1] == mean
    assert metrics.ssim_map(tx, ty, L).tobytes() == _reference_map((40, 70, 3), np.float32, np.float32, 11).tobytes()
    assert metrics.ssim_map(x[:, :, 0], y[:, :, 0], L).shape == (30, 60)
    x64, y64 = x.astype(np.float64), y.astype(np.float64)
    mse = np.array([np.mean((x64[:, :, c] - y64[:, :, c]) ** 2) for c in range(3)])
    mean_gt = np.array([np.mean(y64[:, :, c]) for c in range(3)])
    for a, b in ((x, y), (tx, ty), (tx, y)):
        e = metrics.ERGAS(a, b, 2)
        assert e == metrics.ERGAS(x, y, 2) and abs(e - 50 * np.sqrt(np.mean(mse / mean_gt ** 2))) <= 1e-12 * e
        pb, pt = metrics.PSNR(a, b, L)
        assert pb.tobytes() == metrics.PSNR(x, y, L)[0].tobytes() and pt == metrics.PSNR(x, y, L)[1]
        np.testing.assert_allclose(pb, 10 * np.log10(L * L / mse), rtol=1e-12, atol=0)
        assert abs(pt - 10 * np.log10(L * L / np.mean((x64 - y64) ** 2))) <= 1e-12 * pt
    assert metrics.ERGAS(x, y, 6) == metrics.ergas_score(metrics.error_sums(x, y), 6)
    # the bicubic forms: the formulas over bicubic_error_sums
    lr = np.ascontiguousarray(y[::2, ::2])
    sums = metrics.bicubic_error_sums(lr, y, 2)
    assert metrics.bicubic_ERGAS(lr, y, 2) == metrics.ergas_score(sums, 2) == metrics.bicubic_ERGAS(torch.from_numpy(lr).cuda(), ty, 2)
    pb, pt = metrics.bicubic_PSNR(lr, y, 2, L)
    assert pb.tobytes() == metrics.psnr_scores(sums, L)[0].tobytes() and pt == metrics.psnr_scores(sums, L)[1]
    up = rs.imresize(lr, 2)
    assert abs(pt - 10 * np.log10(L * L / np.mean((up - y64) ** 2))) <= 1e-12 * pt


def _run(args, timeout):
    r = subprocess.run([sys.executable, '-m'] + args, cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, ' '.join(args) + '\n' + r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


def test_evaluate_with_ssim_ergas_and_psnr(tmp_path):
    """Two tiny tiles laid out as create_patches --test_data writes them; the JSON against the API on the same files."""
    rng = np.random.RandomState(11)
    files = {}
    for name, shape in (('A.SAFE', (24, 36, 3)), ('B.SAFE', (30, 26, 3))):
        d = tmp_path / 'test' / name / 'no_tiling'
        os.makedirs(str(d))
        gt = rng.randint(35, 13110, size=shape).astype(np.uint16)
        lr = rs.imresize(gt.astype(np.float64), 0.5).astype(np.float32)
        pred = (gt + np.rint(rng.normal(0, 150, size=shape))).astype(np.float32)
        np.save(str(d / 'data20_gt.npy'), gt)
        np.save(str(d / 'data20.npy'), lr)
        np.save(str(tmp_path / 'test' / name / 's2_999_-predict.npy'), pred)
        files[name] = (pred, gt, lr)
    out_json = str(tmp_path / 'scores.json')
    base = ['dsen2_amd.evaluate', '--path', str(tmp_path), '--model_nr', 's2_999_']
    out = _run(base + ['--json', out_json, '--ssim', '--ergas', '--psnr'], 300).splitlines()
    rec = json.load(open(out_json))
    assert rec['data_range'] == 10000.0
    for name, (pred, gt, lr) in files.items():
        r = rec['tiles'][name]
        band, mean = metrics.SSIM(pred, gt, L)
        assert r['dsen2']['band_ssim'] == band.tolist() and r['dsen2']['ssim'] == mean
        band, mean = metrics.bicubic_SSIM(lr, gt, 2, L)
        assert r['bicubic']['band_ssim'] == band.tolist() and r['bicubic']['ssim'] == mean
        assert r['dsen2']['ergas'] == metrics.ERGAS(pred, gt, 2) and r['bicubic']['ergas'] == metrics.bicubic_ERGAS(lr, gt, 2)
        band, total = metrics.PSNR(pred, gt, L)
        assert r['dsen2']['band_psnr'] == band.tolist() and r['dsen2']['psnr'] == total
        band, total = metrics.bicubic_PSNR(lr, gt, 2, L)
        assert r['bicubic']['band_psnr'] == band.tolist() and r['bicubic']['psnr'] == total
        q = sr.ssim_map(pred, gt, L)
        n = q.shape[0] * q.shape[1]
        for c in range(3):
            assert abs(r['dsen2']['band_ssim'][c] * n - math.fsum(q[:, :, c].ravel())) <= (n + 2) * EPS * np.abs(q[:, :, c]).sum()      # the quotient and its product: two roundings more
        assert -1 <= r['bicubic']['ssim'] <= 1 and r['dsen2']['psnr'] > 20 and r['dsen2']['ergas'] > 0
    a, b = rec['tiles']['A.SAFE'], rec['tiles']['B.SAFE']
    for k in ('dsen2', 'bicubic'):
        assert rec['mean'][k]['tiles'] == 2
        for key in ('ssim', 'ergas', 'psnr'):
            assert rec['mean'][k][key] == float(np.mean([a[k][key], b[k][key]]))
        for key in ('band_ssim', 'band_psnr'):
            assert rec['mean'][k][key] == np.mean([a[k][key], b[k][key]], axis=0).tolist()
    assert [ln.split() for ln in out if 'SSIM' in ln] == [['RMSE', 'SRE', '[dB]', 'SSIM', 'PSNR', '[dB]'] * 2] * 3
    means = [ln.split() for ln in out if ln.startswith('mean ')]
    assert means == [['mean', '%.4f' % t['dsen2']['ssim'], '%.4f' % t['bicubic']['ssim']] for t in (a, b, rec['mean'])]
    rows = [ln.split() for ln in out if ln.startswith('0 ')]
    assert len(rows) == 3 and rows[0] == ['0'] + ['%.4f' % a[k][key][0] for k in ('dsen2', 'bicubic')
                                                   for key in ('band_rmse', 'band_sre', 'band_ssim', 'band_psnr')]
    for label, k in (('DSen2', 'dsen2'), ('Bicubic', 'bicubic')):
        for t in (a, b, rec['mean']):
            assert '{} PSNR [dB]: {:.4f}'.format(label, t[k]['psnr']) in out and '{} ERGAS: {:.4f}'.format(label, t[k]['ergas']) in out
    # without the flags none of this is printed, and the values every run printed before are the same
    plain_json = str(tmp_path / 'plain.json')
    plain = _run(base + ['--json', plain_json], 300)
    assert 'SSIM' not in plain and 'PSNR' not in plain and 'ERGAS' not in plain
    p = json.load(open(plain_json))
    assert sorted(p) == ['folder', 'mean', 'model_nr', 'tiles']
    for name in files:
        for k in ('dsen2', 'bicubic'):
            assert sorted(p['tiles'][name][k]) == ['band_rmse', 'band_sre', 'rmse']
            assert all(p['tiles'][name][k][key] == rec['tiles'][name][k][key] for key in p['tiles'][name][k])


def test_refusals_through_python_raise_value_error():
    x = torch.zeros((10, 30, 2), dtype=torch.float32, device='cuda')
    big = torch.zeros((20, 30, 2), dtype=torch.float32, device='cuda')
    for call in (lambda: metrics.SSIM(x, x, L), lambda: metrics.ssim_map_device(x, x, L), lambda: metrics.ssim_sums_device(x, x, L),
                 lambda: metrics.bicubic_SSIM(x[:5, :4], torch.zeros((10, 8, 2), device='cuda'), 2, L)):
        with pytest.raises(ValueError, match='smaller than the'):
            call()
    for call in (lambda: metrics.SSIM(big, big, L, win_size=8), lambda: metrics.ssim_map_device(big, big, L, 10),
                 lambda: metrics.ssim_sums_device(big, big, L, win_size=17)):
        with pytest.raises(ValueError, match='win_size'):
            call()
    for bad in (0, -1.0):
        for call in (lambda: metrics.SSIM(big, big, bad), lambda: metrics.ssim_map_device(big, big, bad), lambda: metrics.PSNR(big, big, bad),
                     lambda: metrics.ssim_sums_device(big, big, bad), lambda: metrics.bicubic_SSIM(x[:, :15], big, 2, bad)):
            with pytest.raises(ValueError, match='data_range'):
                call()
    assert metrics.SSIM(big, big, L)[1] == 1.0                      # and what is not refused runs: an image against itself
