"""SSIM, ERGAS and PSNR, host side (no GPU): the numpy restatement (tests/ssim_restatement.py) against the 2-D-window form and
against the maps scikit-image computed (tests/golden/ssim_skimage.npz); the window; ERGAS and PSNR against a direct computation;
the C ABI's new symbols and their argument checks; the refusals that come before the GPU; the command line's new flags.

Gate of the two independent statements: 1e-12 absolute on a map whose values are below 1.  The separable form and the 2-D form
add 121 terms of magnitude up to 1e8 in two orders, sums that then cancel to variances of about 1e4 .. 1e6 and are divided by
about as much.  On the committed fixture (values 418 .. 5746, a perturbation of standard deviation 120) the differences are
2.9e-13 against the 2-D window and 2.1e-13 against scikit-image; each test prints its own."""
import ctypes
import json
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ssim_restatement as sr  # noqa: E402

from dsen2_amd import evaluate, metrics, patches  # noqa: E402

ENTRIES = ('dsen2_ssim_map', 'dsen2_ssim_sums', 'dsen2_imresize_ssim_sums')
GATE = 1e-12
L = 1e4


def _golden():
    z = np.load(os.path.join(ROOT, 'tests', 'golden', 'ssim_skimage.npz'))
    return z['x'], z['gt'], z['ssim_map'], float(z['data_range'])


def _two_d(x, y, data_range, win_size=11, sigma=1.5):
    """ssim_index.m with the 2-D window: five 'valid' correlations with fspecial-style weights."""
    from scipy.signal import correlate2d
    x, y = x.astype(np.float64), y.astype(np.float64)
    g = sr.window_2d(win_size, sigma)
    C1, C2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    mx, my = correlate2d(x, g, 'valid'), correlate2d(y, g, 'valid')
    sxx = correlate2d(x * x, g, 'valid') - mx * mx
    syy = correlate2d(y * y, g, 'valid') - my * my
    sxy = correlate2d(x * y, g, 'valid') - mx * my
    return ((2 * mx * my + C1) * (2 * sxy + C2)) / ((mx * mx + my * my + C1) * (sxx + syy + C2))


def test_restatement_equals_the_two_d_window_form():
    x, gt, _, data_range = _golden()
    assert x.shape == gt.shape == (48, 64, 2) and data_range == L
    for c in range(2):
        q = sr.ssim_map_band(x[:, :, c], gt[:, :, c], L)
        assert q.shape == (38, 54) and q.dtype == np.float64
        d = np.abs(q - _two_d(x[:, :, c], gt[:, :, c], L)).max()
        print('band %d: restatement against the 2-D window, max abs difference %.3g' % (c, d))
        assert d <= GATE
    # another window, a ragged crop, an anti-correlated pair (negative values occur) and an image against itself
    a, b = x[:33, :47, 0], gt[:33, :47, 0]
    for win, sigma in ((3, 0.8), (15, 2.5)):
        assert np.abs(sr.ssim_map_band(a, b, L, win, sigma) - _two_d(a, b, L, win, sigma)).max() <= GATE
    q = sr.ssim_map_band(a, L - a.astype(np.float64), L)
    assert q.min() < 0 and np.abs(q - _two_d(a, L - a.astype(np.float64), L)).max() <= GATE
    assert np.abs(sr.ssim_map_band(a, a, L) - 1).max() <= GATE


def test_restatement_equals_the_committed_scikit_image_maps():
    x, gt, want, data_range = _golden()
    q = sr.ssim_map(x, gt, data_range)
    assert q.shape == want.shape == (38, 54, 2)
    d = np.abs(q - want).max()
    print('restatement against scikit-image: max abs difference %.3g' % d)
    assert d <= GATE
    band, mean = sr.ssim(x, gt, data_range)
    assert band.shape == (2,) and band[0] == q[:, :, 0].mean() and mean == band.mean() and 0.9 < mean < 1
    assert os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'ssim_skimage.npz')) < 100 * 1024


def test_the_window_sums_to_one_and_is_symmetric():
    for win, sigma in ((11, 1.5), (3, 1.5), (15, 1.5), (7, 0.5), (11, 4.0)):
        w = metrics.ssim_window(win, sigma)
        assert w.dtype == np.float64 and w.shape == (win,)
        assert abs(w.sum() - 1.0) <= 2.0 ** -52
        assert w.tobytes() == w[::-1].tobytes()
        assert w.argmax() == win // 2 and (w > 0).all()
    assert metrics.ssim_window().tobytes() == metrics.ssim_window(11, 1.5).tobytes()
    d = np.arange(11) - 5.0
    g = np.exp(-d * d / 4.5)
    assert np.abs(metrics.ssim_window() - g / g.sum()).max() <= 2.0 ** -52
    assert np.abs(np.outer(metrics.ssim_window(), metrics.ssim_window()) - sr.window_2d()).max() <= 1e-17
    for bad in (2, 4, 1, 17, 5.5):
        with pytest.raises(ValueError, match='win_size'):
            metrics.ssim_window(bad)
    for bad in (0, -1.0, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='sigma'):
            metrics.ssim_window(11, bad)


def _sums(x, gt):
    x, gt = x.astype(np.float64), gt.astype(np.float64)
    return np.stack([((x - gt) ** 2).sum(axis=(0, 1)), gt.sum(axis=(0, 1)), np.full(gt.shape[2], gt.shape[0] * gt.shape[1], np.float64)], axis=1)


def test_ergas_and_psnr_against_a_direct_computation():
    x, gt, _, _ = _golden()
    x, gt = x.astype(np.float64), gt.astype(np.float64)
    sums = _sums(x, gt)
    mse = np.array([np.mean((x[:, :, c] - gt[:, :, c]) ** 2) for c in range(2)])
    mean = np.array([np.mean(gt[:, :, c]) for c in range(2)])
    for scale in (2, 6):
        want = 100.0 / scale * np.sqrt(np.mean(mse / mean ** 2))
        got = metrics.ergas_score(sums, scale)
        assert isinstance(got, float) and abs(got - want) <= 1e-13 * want
    band, total = metrics.psnr_scores(sums, L)
    np.testing.assert_allclose(band, 10 * np.log10(L * L / mse), rtol=1e-13, atol=0)
    assert isinstance(total, float) and abs(total - 10 * np.log10(L * L / np.mean((x - gt) ** 2))) <= 1e-13 * total
    assert 20 < total < 60 and 0 < metrics.ergas_score(sums, 2) < 10
    # a zero band mean and a zero error give numpy's inf
    zero = np.array([[5.0, 0.0, 10.0], [0.0, 30.0, 10.0]])
    assert metrics.ergas_score(zero, 2) == np.inf
    band, total = metrics.psnr_scores(zero, L)
    assert np.isfinite(band[0]) and band[1] == np.inf and np.isfinite(total)
    assert metrics.psnr_scores(zero[1:], L)[1] == np.inf
    for bad in (0, -1.0, float('nan')):
        with pytest.raises(ValueError, match='data_range'):
            metrics.psnr_scores(sums, bad)


def test_refusals_come_before_the_gpu(monkeypatch):
    def no_gpu():
        raise AssertionError('the GPU was asked for')
    monkeypatch.setattr(patches, 'default_device', no_gpu)
    a = np.zeros((12, 20, 2), np.float32)
    for call in (lambda: metrics.ssim_map(a, a[:, :, :1], L), lambda: metrics.SSIM(a, a[:11], L), lambda: metrics.ssim_sums(a, a[:, :19], L)):
        with pytest.raises(ValueError, match='images of shape'):
            call()
    for call in (lambda: metrics.ssim_map(a[:10], a[:10], L), lambda: metrics.SSIM(a[:, :10], a[:, :10], L), lambda: metrics.ssim_sums(a, a, L, 13),
                 lambda: metrics.bicubic_ssim_sums(a[:5, :9], np.zeros((10, 18, 2), np.float32), 2, L),
                 lambda: metrics.bicubic_SSIM(a[:6], np.zeros((12, 40, 2), np.float32), 2, L, win_size=13)):
        with pytest.raises(ValueError, match='smaller than the'):
            call()
    for size in (10, 2, 17, 4.5):
        with pytest.raises(ValueError, match='win_size'):
            metrics.SSIM(a, a, L, win_size=size)
    for bad in (0, -5.0, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='data_range'):
            metrics.SSIM(a, a, bad)
        with pytest.raises(ValueError, match='data_range'):
            metrics.bicubic_SSIM(a, np.zeros((24, 40, 2), np.float32), 2, bad)
    with pytest.raises(ValueError, match='sigma'):
        metrics.ssim_map(a, a, L, sigma=0)
    with pytest.raises(ValueError, match='constants'):
        metrics.SSIM(a, a, L, k1=0)
    with pytest.raises(ValueError, match='ground truth of shape'):
        metrics.bicubic_ssim_sums(a, np.zeros((24, 41, 2), np.float32), 2, L)
    with pytest.raises(TypeError):
        metrics.SSIM(a, a)                                  # data_range has no default


def test_c_abi_declares_exports_and_checks_the_new_entries():
    from dsen2_amd import _lib, build
    build.build()
    lib = _lib.load()
    header = open(os.path.join(ROOT, 'include', 'dsen2_hip.h')).read()
    for name in ENTRIES:
        assert re.search(r'\bint %s\s*\(' % name, header) and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert 'ssim.hip' in build.SOURCES and 'quality_metrics.hip' in build.SOURCES
    a, b, c, d = (ctypes.c_void_p(0x1000 * k) for k in (1, 2, 3, 4))       # never dereferenced: every call below is refused first
    F32, F64, U16, big = _lib.DTYPE_F32, _lib.DTYPE_F64, _lib.DTYPE_U16, 1 << 30
    c1, c2 = (0.01 * L) ** 2, (0.03 * L) ** 2
    nan, inf = float('nan'), float('inf')

    def window(win, poison=None):
        w = [1.0 / win] * win
        if poison is not None:
            w[win // 2] = poison
        return (ctypes.c_double * win)(*w)

    def refused(code, fn, *args):
        assert fn(*args) == code
        return lib.dsen2_last_error().decode()
    INVALID, WORKSPACE = _lib.ERR_INVALID, _lib.ERR_WORKSPACE
    w11 = window(11)
    m = lib.dsen2_ssim_map
    for win in (10, 2, 1, 17, 16, 0, -3):
        assert 'window size' in refused(INVALID, m, a, F32, b, F32, 40, 40, 2, window(max(win, 1)), win, c1, c2, d, None)
    assert 'smaller' in refused(INVALID, m, a, F32, b, F32, 10, 40, 2, w11, 11, c1, c2, d, None)
    assert 'smaller' in refused(INVALID, m, a, F32, b, F32, 40, 10, 2, w11, 11, c1, c2, d, None)
    assert 'bands' in refused(INVALID, m, a, F32, b, F32, 40, 40, 65, w11, 11, c1, c2, d, None)
    assert 'bands' in refused(INVALID, m, a, F32, b, F32, 40, 40, 0, w11, 11, c1, c2, d, None)
    assert 'not supported' in refused(INVALID, m, a, U16, b, F32, 40, 40, 2, w11, 11, c1, c2, d, None)
    assert 'not supported' in refused(INVALID, m, a, F64, b, 3, 40, 40, 2, w11, 11, c1, c2, d, None)
    assert 'too large' in refused(INVALID, m, a, F32, b, F32, 40000, 40000, 2, w11, 11, c1, c2, d, None)
    for k1, k2 in ((0.0, c2), (c1, 0.0), (-1.0, c2), (c1, -c2), (nan, c2), (c1, nan), (inf, c2), (c1, inf)):
        assert 'finite and positive' in refused(INVALID, m, a, F32, b, F32, 40, 40, 2, w11, 11, k1, k2, d, None)
    for poison in (nan, inf, -inf):
        assert 'not finite' in refused(INVALID, m, a, F32, b, F32, 40, 40, 2, window(11, poison), 11, c1, c2, d, None)
    refused(INVALID, m, None, F32, b, F32, 40, 40, 2, w11, 11, c1, c2, d, None)
    refused(INVALID, m, a, F32, None, F32, 40, 40, 2, w11, 11, c1, c2, d, None)
    refused(INVALID, m, a, F32, b, F32, 40, 40, 2, None, 11, c1, c2, d, None)
    refused(INVALID, m, a, F32, b, F32, 40, 40, 2, w11, 11, c1, c2, None, None)
    s = lib.dsen2_ssim_sums
    assert 'workspace' in refused(WORKSPACE, s, a, F32, b, F64, 40, 40, 6, w11, 11, c1, c2, c, 16, d, None)
    assert 'smaller' in refused(INVALID, s, a, F32, b, F64, 40, 10, 6, w11, 11, c1, c2, c, big, d, None)
    assert 'window size' in refused(INVALID, s, a, F32, b, F64, 40, 40, 6, w11, 8, c1, c2, c, big, d, None)
    assert 'bands' in refused(INVALID, s, a, F32, b, F64, 40, 40, 65, w11, 11, c1, c2, c, big, d, None)
    assert 'not supported' in refused(INVALID, s, a, U16, b, F64, 40, 40, 6, w11, 11, c1, c2, c, big, d, None)
    assert 'too large' in refused(INVALID, s, a, F32, b, F64, 40000, 40000, 2, w11, 11, c1, c2, c, big, d, None)
    assert 'finite and positive' in refused(INVALID, s, a, F32, b, F64, 40, 40, 6, w11, 11, c1, 0.0, c, big, d, None)
    assert 'not finite' in refused(INVALID, s, a, F32, b, F64, 40, 40, 6, window(11, nan), 11, c1, c2, c, big, d, None)
    refused(INVALID, s, a, F32, b, F64, 40, 40, 6, w11, 11, c1, c2, None, big, d, None)
    refused(INVALID, s, a, F32, b, F64, 40, 40, 6, w11, 11, c1, c2, c, big, None, None)
    refused(INVALID, s, a, F32, b, F64, 40, 40, 6, None, 11, c1, c2, c, big, d, None)
    u = lib.dsen2_imresize_ssim_sums
    assert 'smaller' in refused(INVALID, u, a, F64, 5, 40, 2, 0, 10, b, c, 4, d, F32, w11, 11, c1, c2, c, big, d, None)     # the OUTPUT is 10 x 40
    assert 'smaller' in refused(INVALID, u, a, F64, 40, 5, 2, 1, 10, b, c, 4, d, F32, w11, 11, c1, c2, c, big, d, None)
    assert 'window size' in refused(INVALID, u, a, F64, 20, 20, 2, 1, 40, b, c, 4, d, F32, w11, 12, c1, c2, c, big, d, None)
    assert 'not supported' in refused(INVALID, u, a, 3, 20, 20, 2, 1, 40, b, c, 4, d, F32, w11, 11, c1, c2, c, big, d, None)
    assert 'not supported' in refused(INVALID, u, a, F64, 20, 20, 2, 1, 40, b, c, 4, d, U16, w11, 11, c1, c2, c, big, d, None)
    assert 'bands' in refused(INVALID, u, a, F64, 20, 20, 65, 1, 40, b, c, 4, d, F32, w11, 11, c1, c2, c, big, d, None)
    assert 'axis 2' in refused(INVALID, u, a, F64, 20, 20, 2, 2, 40, b, c, 4, d, F32, w11, 11, c1, c2, c, big, d, None)
    assert 'taps' in refused(INVALID, u, a, F64, 20, 20, 2, 1, 40, b, c, 257, d, F32, w11, 11, c1, c2, c, big, d, None)
    assert 'too large' in refused(INVALID, u, a, F64, 20, 70000, 13, 0, 4000, b, c, 4, d, F32, w11, 11, c1, c2, c, big, d, None)
    assert 'finite and positive' in refused(INVALID, u, a, U16, 20, 20, 2, 1, 40, b, c, 4, d, F32, w11, 11, nan, c2, c, big, d, None)
    assert 'not finite' in refused(INVALID, u, a, U16, 20, 20, 2, 1, 40, b, c, 4, d, F32, window(11, inf), 11, c1, c2, c, big, d, None)
    assert 'workspace' in refused(WORKSPACE, u, a, U16, 20, 20, 2, 1, 40, b, c, 4, d, F64, w11, 11, c1, c2, c, 8, d, None)
    refused(INVALID, u, None, F64, 20, 20, 2, 1, 40, b, c, 4, d, F32, w11, 11, c1, c2, c, big, d, None)
    refused(INVALID, u, a, F64, 20, 20, 2, 1, 40, None, c, 4, d, F32, w11, 11, c1, c2, c, big, d, None)
    refused(INVALID, u, a, F64, 20, 20, 2, 1, 40, b, None, 4, d, F32, w11, 11, c1, c2, c, big, d, None)
    refused(INVALID, u, a, F64, 20, 20, 2, 1, 40, b, c, 4, None, F32, w11, 11, c1, c2, c, big, d, None)
    refused(INVALID, u, a, F64, 20, 20, 2, 1, 40, b, c, 4, d, F32, None, 11, c1, c2, c, big, d, None)
    refused(INVALID, u, a, F64, 20, 20, 2, 1, 40, b, c, 4, d, F32, w11, 11, c1, c2, None, big, d, None)
    refused(INVALID, u, a, F64, 20, 20, 2, 1, 40, b, c, 4, d, F32, w11, 11, c1, c2, c, big, None, None)


def test_evaluate_accepts_the_new_flags_and_defaults_them_to_off():
    a = evaluate.parse_args([])
    assert (a.ssim, a.ergas, a.psnr, a.data_range, a.win_size, a.sigma) == (False, False, False, 10000.0, 11, 1.5)
    assert (a.uiq, a.sam, a.block_size, a.path, a.run_60, a.model_nr, a.json) == (False, False, 8, '../data/', False, 's2_038_', None)
    a = evaluate.parse_args(['--ssim', '--ergas', '--psnr', '--data_range', '2000', '--win_size', '7', '--sigma', '1.0'])
    assert (a.ssim, a.ergas, a.psnr, a.data_range, a.win_size, a.sigma) == (True, True, True, 2000.0, 7, 1.0)
    a = evaluate.parse_args(['--psnr'])
    assert (a.ssim, a.ergas, a.psnr, a.uiq, a.sam) == (False, False, True, False, False)


class _OnHost(np.ndarray):
    device = None                 # stands in for the device tensor evaluate uploads once per image


def test_evaluate_prints_ssim_ergas_and_psnr_only_when_asked(tmp_path, monkeypatch, capsys):
    """The command line's plumbing with the GPU sums replaced by the restatement: the columns, the lines, the JSON keys, and
    unchanged text and JSON without the flags."""
    def up(lr, scale):
        return np.repeat(np.repeat(np.asarray(lr), scale, 0), scale, 1)

    def ssim_sums(x, gt, data_range, win_size=11, sigma=1.5, k1=0.01, k2=0.03):
        q = sr.ssim_map(np.asarray(x), np.asarray(gt), data_range, win_size, sigma, k1, k2)
        return np.stack([q.sum(axis=(0, 1)), np.full(q.shape[2], q.shape[0] * q.shape[1], np.float64)], axis=1)
    uploads = []

    def upload(a, device=None):
        uploads.append(np.shape(a))
        return np.asarray(a).view(_OnHost)
    monkeypatch.setattr(metrics, '_device_image', upload)
    monkeypatch.setattr(metrics, 'error_sums', lambda x, gt: _sums(np.asarray(x), np.asarray(gt)))
    monkeypatch.setattr(metrics, 'bicubic_error_sums', lambda lr, gt, scale: _sums(up(lr, scale), np.asarray(gt)))
    monkeypatch.setattr(metrics, 'ssim_sums', ssim_sums)
    monkeypatch.setattr(metrics, 'bicubic_ssim_sums', lambda lr, gt, scale, data_range, *a: ssim_sums(up(lr, scale), gt, data_range, *a))
    rng = np.random.RandomState(5)
    data = {}
    for name in ('A.SAFE', 'B.SAFE'):
        d = tmp_path / 'test' / name / 'no_tiling'
        os.makedirs(str(d))
        gt = rng.randint(100, 9000, size=(12, 14, 3)).astype(np.float32)
        lr = gt[::2, ::2] + 3
        pred = gt + rng.randint(-50, 60, size=gt.shape).astype(np.float32)
        np.save(str(d / 'data20_gt.npy'), gt)
        np.save(str(d / 'data20.npy'), lr)
        np.save(str(tmp_path / 'test' / name / 's2_999_-predict.npy'), pred)
        data[name] = (pred, gt, lr)
    plain_json, out_json = str(tmp_path / 'plain.json'), str(tmp_path / 'scores.json')
    base = ['--path', str(tmp_path), '--model_nr', 's2_999_']
    assert evaluate.main(base + ['--json', plain_json]) == 0
    plain = capsys.readouterr().out
    assert 'SSIM' not in plain and 'PSNR' not in plain and 'ERGAS' not in plain and 'mean ' not in plain and uploads == []
    assert evaluate.main(base + ['--json', out_json, '--ssim', '--ergas', '--psnr', '--win_size', '5', '--sigma', '1.0', '--data_range', '8000']) == 0
    out = capsys.readouterr().out.splitlines()
    assert sorted(uploads) == sorted([(12, 14, 3), (6, 7, 3), (12, 14, 3)] * 2)           # one upload of each image per tile
    rec = json.load(open(out_json))
    assert rec['data_range'] == 8000.0
    for name, (pred, gt, lr) in data.items():
        e = rec['tiles'][name]
        band, mean = sr.ssim(pred, gt, 8000.0, 5, 1.0)
        np.testing.assert_allclose(e['dsen2']['band_ssim'], band, rtol=1e-14)             # the stand-in adds the map up in another order
        assert abs(e['dsen2']['ssim'] - mean) <= 1e-14 and e['dsen2']['ssim'] == float(np.mean(e['dsen2']['band_ssim']))
        np.testing.assert_allclose(e['bicubic']['band_ssim'], sr.ssim(up(lr, 2), gt, 8000.0, 5, 1.0)[0], rtol=1e-14)
        assert e['dsen2']['ergas'] == metrics.ergas_score(_sums(pred, gt), 2) and e['bicubic']['ergas'] == metrics.ergas_score(_sums(up(lr, 2), gt), 2)
        band, total = metrics.psnr_scores(_sums(pred, gt), 8000.0)
        assert e['dsen2']['band_psnr'] == band.tolist() and e['dsen2']['psnr'] == total
    a, b = rec['tiles']['A.SAFE'], rec['tiles']['B.SAFE']
    for k in ('dsen2', 'bicubic'):
        for key in ('ssim', 'ergas', 'psnr'):
            assert rec['mean'][k][key] == float(np.mean([a[k][key], b[k][key]]))
        for key in ('band_ssim', 'band_psnr'):
            assert rec['mean'][k][key] == np.mean([a[k][key], b[k][key]], axis=0).tolist()
    header = [ln for ln in out if ln.lstrip().startswith('RMSE') and 'SSIM' in ln]
    assert len(header) == 3 and header[0].split() == ['RMSE', 'SRE', '[dB]', 'SSIM', 'PSNR', '[dB]'] * 2
    row = [ln for ln in out if ln.startswith('0 ')][0].split()
    assert len(row) == 9 and row[3] == '%.4f' % a['dsen2']['band_ssim'][0] and row[4] == '%.4f' % a['dsen2']['band_psnr'][0]
    means = [ln.split() for ln in out if ln.startswith('mean ')]
    assert len(means) == 3 and means[0] == ['mean', '%.4f' % a['dsen2']['ssim'], '%.4f' % a['bicubic']['ssim']]
    for label, k in (('DSen2', 'dsen2'), ('Bicubic', 'bicubic')):
        assert '{} PSNR [dB]: {:.4f}'.format(label, a[k]['psnr']) in out and '{} ERGAS: {:.4f}'.format(label, b[k]['ergas']) in out
        assert '{} ERGAS: {:.4f}'.format(label, rec['mean'][k]['ergas']) in out
    # the values every run printed before are the same; one flag alone adds only its own values and needs no upload
    p = json.load(open(plain_json))
    assert 'data_range' not in p
    for name in data:
        for k in ('dsen2', 'bicubic'):
            assert sorted(p['tiles'][name][k]) == ['band_rmse', 'band_sre', 'rmse']
            assert all(p['tiles'][name][k][key] == rec['tiles'][name][k][key] for key in p['tiles'][name][k])
    del uploads[:]
    assert evaluate.main(base + ['--json', out_json, '--ergas']) == 0
    text = capsys.readouterr().out
    assert 'SSIM' not in text and 'PSNR' not in text and text.count('ERGAS') == 6 and uploads == []
    rec = json.load(open(out_json))
    e = rec['tiles']['A.SAFE']['dsen2']
    assert 'ergas' in e and 'ssim' not in e and 'psnr' not in e and 'data_range' not in rec
    # the text without the new flags is the old text: what --ergas printed minus its lines
    assert [ln for ln in text.splitlines() if 'ERGAS' not in ln] == plain.splitlines()


def test_the_product_does_not_import_the_tests_restatement():
    for base, _, files in os.walk(os.path.join(ROOT, 'dsen2_amd')):
        for f in files:
            if f.endswith('.py'):
                assert 'ssim_restatement' not in open(os.path.join(base, f)).read(), f
