"""UIQ and SAM, host side (no GPU): the numpy restatement (tests/quality_restatement.py) against a naive per-window computation
with means, variances and covariance; its SAM on a zero spectrum; the refusals that come before the GPU; the C ABI's new symbols
and their argument checks; the command line's new flags."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import quality_restatement as qr  # noqa: E402

from dsen2_amd import evaluate, metrics, patches  # noqa: E402

ENTRIES = ('dsen2_quality_workspace_bytes', 'dsen2_uiq_map', 'dsen2_uiq_sums', 'dsen2_sam_sums', 'dsen2_imresize_uiq_sums',
           'dsen2_imresize_sam_sums')


def _naive(x, y, B=8):
    """img_qi.m's definition window by window: q = 4 cov mx my / ((vx + vy) (mx^2 + my^2)) with its two special cases."""
    x, y = x.astype(np.float64), y.astype(np.float64)
    H, W = x.shape
    out = np.ones((H - B + 1, W - B + 1))
    for i in range(H - B + 1):
        for j in range(W - B + 1):
            a, b = x[i:i + B, j:j + B], y[i:i + B, j:j + B]
            ma, mb, va, vb = a.mean(), b.mean(), a.var(ddof=1), b.var(ddof=1)
            cov = ((a - ma) * (b - mb)).sum() / (B * B - 1)
            d = (va + vb) * (ma * ma + mb * mb)
            if d != 0:
                out[i, j] = 4 * cov * ma * mb / d
            elif va + vb == 0 and ma * ma + mb * mb != 0:
                out[i, j] = 2 * ma * mb / (ma * ma + mb * mb)
    return out


def test_restatement_equals_the_naive_windows_and_takes_both_special_branches():
    x, gt = qr.planted()
    assert x.shape == (40, 37)
    taken = {}
    q = qr.uiq_map(x, gt, 8, taken)
    assert q.shape == (33, 30) and q.dtype == np.float64
    assert np.abs(q - _naive(x, gt)).max() <= 1e-12
    assert taken == {'flat': 64, 'one': 30}               # 15 x 15 flat pixels: 8 x 8 windows; 12 x 13 zero pixels: 5 x 6 windows
    flat = 2.0 * 1234 * 1200 / (1234.0 ** 2 + 1200.0 ** 2)
    assert abs(q[5, 3] - flat) <= 1e-15 and q[22, 20] == 1.0
    band, mean = qr.uiq(np.stack([x, x], 2), np.stack([gt, gt], 2))
    assert band.shape == (2,) and band[0] == band[1] == q.mean() and mean == band.mean()
    # another block size, and an image equal to itself scores 1 wherever it is not constant
    assert np.abs(qr.uiq_map(x, gt, 3) - _naive(x, gt, 3)).max() <= 1e-12
    assert np.abs(qr.uiq_map(x, x, 8) - 1).max() <= 1e-12


def test_restatements_sam_skips_a_zero_spectrum():
    r = np.random.RandomState(1)
    x = (r.rand(6, 5, 4) * 4000).astype(np.float32)
    y = (x + r.normal(0, 30, x.shape)).astype(np.float32)
    y[3, 4] = 0
    x[0, 0] = 0
    total, n = qr.sam_sums(x, y)
    assert n == 6 * 5 - 2
    want = 0.0
    for i in range(6):
        for j in range(5):
            a, b = x[i, j].astype(np.float64), y[i, j].astype(np.float64)
            if np.linalg.norm(a) * np.linalg.norm(b) != 0:
                want += np.degrees(np.arccos(min(1.0, np.dot(a, b) / (np.linalg.norm(a) * np.linalg.norm(b)))))
    assert abs(total - want) <= 1e-9 * want
    assert qr.sam_sums(x[1:3], x[1:3] * 2)[0] <= 1e-4 * 10          # parallel spectra: angle 0 up to the rounding of the cosine
    assert qr.sam_sums(np.zeros((3, 3, 2)), np.ones((3, 3, 2))) == (0.0, 0)


def test_refusals_come_before_the_gpu(monkeypatch):
    def no_gpu():
        raise AssertionError('the GPU was asked for')
    monkeypatch.setattr(patches, 'default_device', no_gpu)
    a = np.zeros((9, 12, 2), np.float32)
    for call in (lambda: metrics.uiq_map(a, a[:, :, :1]), lambda: metrics.UIQ(a, a[:8]), lambda: metrics.uiq_sums(a, a[:, :11]),
                 lambda: metrics.SAM(a, a[:8]), lambda: metrics.sam_sums(a, a[:, :, 0])):
        with pytest.raises(ValueError, match='images of shape'):
            call()
    for call in (lambda: metrics.uiq_map(a[:7], a[:7]), lambda: metrics.UIQ(a[:, :7], a[:, :7]), lambda: metrics.uiq_sums(a, a, 10),
                 lambda: metrics.bicubic_uiq_sums(a[:3, :5], np.zeros((6, 10, 2), np.float32), 2),
                 lambda: metrics.bicubic_UIQ(a[:4], np.zeros((8, 24, 2), np.float32), 2, block_size=9)):
        with pytest.raises(ValueError, match='smaller than the'):
            call()
    for size in (1, 17, 2.5):
        with pytest.raises(ValueError, match='block_size'):
            metrics.UIQ(a, a, block_size=size)
    for call in (lambda: metrics.bicubic_uiq_sums(a, np.zeros((18, 25, 2), np.float32), 2), lambda: metrics.bicubic_SAM(a, a, 2),
                 lambda: metrics.bicubic_sam_sums(a, np.zeros((18, 24, 3), np.float32), 2)):
        with pytest.raises(ValueError, match='ground truth of shape'):
            call()
    with pytest.raises(ValueError, match='dimensions'):
        metrics.SAM(np.zeros((2, 9, 9, 2), np.float32), np.zeros((2, 9, 9, 2), np.float32))


def test_c_abi_declares_exports_and_checks_the_new_entries():
    from dsen2_amd import _lib, build
    build.build()
    lib = _lib.load()
    header = open(os.path.join(ROOT, 'include', 'dsen2_hip.h')).read()
    for name in ENTRIES:
        assert re.search(r'\bint %s\s*\(' % name, header) and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert 'quality_metrics.hip' in build.SOURCES
    a, b, c, d = (ctypes.c_void_p(0x1000 * k) for k in (1, 2, 3, 4))       # never dereferenced: every call below is refused first
    F32, F64, U16, big = _lib.DTYPE_F32, _lib.DTYPE_F64, _lib.DTYPE_U16, 1 << 30

    def refused(fn, *args):
        assert fn(*args) in (_lib.ERR_INVALID, _lib.ERR_WORKSPACE)
        return lib.dsen2_last_error().decode()
    n = ctypes.c_size_t(0)
    assert lib.dsen2_quality_workspace_bytes(6, ctypes.byref(n)) == _lib.OK and n.value >= 6 * 16
    assert lib.dsen2_quality_workspace_bytes(65, ctypes.byref(n)) == _lib.ERR_INVALID
    assert lib.dsen2_quality_workspace_bytes(0, ctypes.byref(n)) == _lib.ERR_INVALID
    m = lib.dsen2_uiq_map
    assert 'smaller' in refused(m, a, F32, b, F32, 7, 9, 2, 8, d, None)
    assert 'smaller' in refused(m, a, F32, b, F32, 9, 7, 2, 8, d, None)
    assert 'block size' in refused(m, a, F32, b, F32, 40, 40, 2, 1, d, None)
    assert 'block size' in refused(m, a, F32, b, F32, 40, 40, 2, 17, d, None)
    assert 'bands' in refused(m, a, F32, b, F32, 40, 40, 65, 8, d, None)
    assert 'bands' in refused(m, a, F32, b, F32, 40, 40, 0, 8, d, None)
    assert 'not supported' in refused(m, a, U16, b, F32, 40, 40, 2, 8, d, None)
    assert 'not supported' in refused(m, a, F64, b, 3, 40, 40, 2, 8, d, None)
    assert 'too large' in refused(m, a, F32, b, F32, 40000, 40000, 2, 8, d, None)
    refused(m, None, F32, b, F32, 40, 40, 2, 8, d, None)
    refused(m, a, F32, None, F32, 40, 40, 2, 8, d, None)
    refused(m, a, F32, b, F32, 40, 40, 2, 8, None, None)
    s = lib.dsen2_uiq_sums
    assert 'workspace' in refused(s, a, F32, b, F64, 40, 40, 6, 8, c, 16, d, None)
    assert 'smaller' in refused(s, a, F32, b, F64, 40, 7, 6, 8, c, big, d, None)
    assert 'block size' in refused(s, a, F32, b, F64, 40, 40, 6, 0, c, big, d, None)
    assert 'not supported' in refused(s, a, U16, b, F64, 40, 40, 6, 8, c, big, d, None)
    refused(s, a, F32, b, F64, 40, 40, 6, 8, None, big, d, None)
    refused(s, a, F32, b, F64, 40, 40, 6, 8, c, big, None, None)
    g = lib.dsen2_sam_sums
    assert 'bands' in refused(g, a, F32, b, F32, 8, 8, 65, c, big, d, None)
    assert 'not supported' in refused(g, a, F32, b, U16, 8, 8, 6, c, big, d, None)
    assert 'workspace' in refused(g, a, F32, b, F32, 8, 8, 6, c, 0, d, None)
    refused(g, None, F32, b, F32, 8, 8, 6, c, big, d, None)
    u = lib.dsen2_imresize_uiq_sums
    assert 'smaller' in refused(u, a, F64, 3, 8, 2, 0, 6, b, c, 4, d, F32, 8, c, big, d, None)          # the OUTPUT is 6 x 8
    assert 'block size' in refused(u, a, F64, 8, 8, 2, 1, 16, b, c, 4, d, F32, 17, c, big, d, None)
    assert 'not supported' in refused(u, a, 3, 8, 8, 2, 1, 16, b, c, 4, d, F32, 8, c, big, d, None)
    assert 'not supported' in refused(u, a, F64, 8, 8, 2, 1, 16, b, c, 4, d, U16, 8, c, big, d, None)
    assert 'axis 2' in refused(u, a, F64, 8, 8, 2, 2, 16, b, c, 4, d, F32, 8, c, big, d, None)
    assert 'taps' in refused(u, a, F64, 8, 8, 2, 1, 16, b, c, 257, d, F32, 8, c, big, d, None)
    assert 'workspace' in refused(u, a, F64, 8, 8, 2, 1, 16, b, c, 4, d, F32, 8, c, 0, d, None)
    assert 'too large' in refused(u, a, F64, 8, 70000, 13, 0, 4000, b, c, 4, d, F32, 8, c, big, d, None)
    refused(u, a, F64, 8, 8, 2, 1, 16, None, c, 4, d, F32, 8, c, big, d, None)
    v = lib.dsen2_imresize_sam_sums
    assert 'bands' in refused(v, a, F64, 8, 8, 65, 1, 16, b, c, 4, d, F32, c, big, d, None)
    assert 'taps' in refused(v, a, F64, 8, 8, 2, 1, 16, b, c, 0, d, F32, c, big, d, None)
    assert 'workspace' in refused(v, a, U16, 8, 8, 2, 1, 16, b, c, 4, d, F64, c, 8, d, None)
    refused(v, a, F64, 8, 8, 2, 1, 16, b, c, 4, None, F32, c, big, d, None)


def test_evaluate_accepts_the_new_flags_and_defaults_them_to_off():
    a = evaluate.parse_args([])
    assert (a.uiq, a.sam, a.block_size) == (False, False, 8)
    assert (a.path, a.run_60, a.model_nr, a.json) == ('../data/', False, 's2_038_', None)
    a = evaluate.parse_args(['--uiq', '--sam', '--block_size', '4', '--path', 'p'])
    assert (a.uiq, a.sam, a.block_size, a.path) == (True, True, 4, 'p')
    assert evaluate.parse_args(['--sam']).uiq is False and evaluate.parse_args(['--uiq']).sam is False


def _host_error_sums(x, gt):
    x, gt = np.asarray(x, np.float64), np.asarray(gt, np.float64)
    return np.stack([((x - gt) ** 2).sum(axis=(0, 1)), gt.sum(axis=(0, 1)), np.full(gt.shape[2], gt.shape[0] * gt.shape[1], np.float64)], axis=1)


class _OnHost(np.ndarray):
    device = None                 # stands in for the device tensor evaluate uploads once per image


def test_evaluate_prints_uiq_and_sam_only_when_asked(tmp_path, monkeypatch, capsys):
    """The command line's plumbing with the GPU sums replaced by the restatement: the UIQ column, the SAM lines, the JSON keys."""
    import json

    def up(lr, scale):
        return np.repeat(np.repeat(np.asarray(lr), scale, 0), scale, 1)

    def uiq_sums(x, gt, block_size=8):
        q = qr.uiq_map(np.asarray(x), np.asarray(gt), block_size)
        return np.stack([q.sum(axis=(0, 1)), np.full(q.shape[2], q.shape[0] * q.shape[1], np.float64)], axis=1)
    monkeypatch.setattr(metrics, '_device_image', lambda a, device=None: np.asarray(a).view(_OnHost))
    monkeypatch.setattr(metrics, 'error_sums', _host_error_sums)
    monkeypatch.setattr(metrics, 'bicubic_error_sums', lambda lr, gt, scale: _host_error_sums(up(lr, scale), gt))
    monkeypatch.setattr(metrics, 'uiq_sums', uiq_sums)
    monkeypatch.setattr(metrics, 'sam_sums', lambda x, gt: np.array(qr.sam_sums(np.asarray(x), np.asarray(gt)), np.float64))
    monkeypatch.setattr(metrics, 'bicubic_uiq_sums', lambda lr, gt, scale, block_size=8: uiq_sums(up(lr, scale), gt, block_size))
    monkeypatch.setattr(metrics, 'bicubic_sam_sums', lambda lr, gt, scale: np.array(qr.sam_sums(up(lr, scale), np.asarray(gt)), np.float64))
    rng = np.random.RandomState(5)
    d = tmp_path / 'test' / 'A.SAFE' / 'no_tiling'
    os.makedirs(str(d))
    gt = rng.randint(100, 9000, size=(10, 12, 3)).astype(np.float32)
    gt[0, 0] = 0
    lr = gt[::2, ::2] + 3
    pred = gt + rng.randint(-50, 60, size=gt.shape).astype(np.float32)
    np.save(str(d / 'data20_gt.npy'), gt)
    np.save(str(d / 'data20.npy'), lr)
    np.save(str(tmp_path / 'test' / 'A.SAFE' / 's2_999_-predict.npy'), pred)
    out_json = str(tmp_path / 'scores.json')
    assert evaluate.main(['--path', str(tmp_path), '--model_nr', 's2_999_']) == 0
    plain = capsys.readouterr().out
    assert 'UIQ' not in plain and 'SAM' not in plain
    assert evaluate.main(['--path', str(tmp_path), '--model_nr', 's2_999_', '--json', out_json, '--uiq', '--sam', '--block_size', '4']) == 0
    out = capsys.readouterr().out.splitlines()
    rec = json.load(open(out_json))
    e = rec['tiles']['A.SAFE']
    band, mean = qr.uiq(pred, gt, 4)
    np.testing.assert_allclose(e['dsen2']['band_uiq'], band, rtol=1e-14)
    assert abs(e['dsen2']['uiq'] - mean) <= 1e-14
    total, n = qr.sam_sums(pred, gt)
    assert e['dsen2']['sam'] == total / n and e['dsen2']['sam_pixels'] == n == 10 * 12 - 1
    np.testing.assert_allclose(e['bicubic']['band_uiq'], qr.uiq(up(lr, 2), gt, 4)[0], rtol=1e-14)
    assert e['bicubic']['sam_pixels'] == n
    assert rec['mean']['dsen2']['uiq'] == e['dsen2']['uiq'] and rec['mean']['bicubic']['sam'] == e['bicubic']['sam']
    header = [ln for ln in out if ln.lstrip().startswith('RMSE') and 'UIQ' in ln]
    assert len(header) == 2 and header[0].split() == ['RMSE', 'SRE', '[dB]', 'UIQ'] * 2
    row = [ln for ln in out if ln.startswith('0 ')][0].split()
    assert row[3] == '%.4f' % band[0] and len(row) == 7
    assert out.count('DSen2 SAM [deg]: %.4f' % (total / n)) == 2 and len([ln for ln in out if ln.startswith('Bicubic SAM [deg]: ')]) == 2
    # one flag alone adds only its own values
    assert evaluate.main(['--path', str(tmp_path), '--model_nr', 's2_999_', '--json', out_json, '--sam']) == 0
    assert 'UIQ' not in capsys.readouterr().out
    e = json.load(open(out_json))['tiles']['A.SAFE']['dsen2']
    assert 'sam' in e and 'uiq' not in e and 'band_uiq' not in e


def test_the_product_does_not_import_the_tests_restatement():
    for base, _, files in os.walk(os.path.join(ROOT, 'dsen2_amd')):
        for f in files:
            if f.endswith('.py'):
                assert 'quality_restatement' not in open(os.path.join(base, f)).read(), f
