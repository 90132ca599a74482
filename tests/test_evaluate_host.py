"""The evaluation step, host side (no GPU): OpenDataFilesTest against the reference's recorded return value and printed lines, the
command lines' arguments, the predict branch's file layout and (rows, columns) decision, the evaluation's printed block and JSON
with the GPU sums replaced by host stand-ins, and the metrics' refusal to compute without a device."""
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
import imresize_fixtures as ifx  # noqa: E402

from dsen2_amd import evaluate, metrics, patches, train  # noqa: E402


@pytest.mark.parametrize('run_60, true_scale, tag', [(False, False, 'run20'), (True, True, 'run60')])
def test_open_data_files_test_equals_the_reference(tmp_path, capsys, run_60, true_scale, tag):
    rec = json.load(open(os.path.join(ifx.GOLDEN, 'imresize_opendata.json')))[tag]
    arrays = np.load(os.path.join(ifx.GOLDEN, 'imresize_opendata.npz'))
    ifx.opendata_dir(str(tmp_path), run_60)
    got, image_size = patches.OpenDataFilesTest(str(tmp_path), run_60, ifx.SCALE, true_scale)
    assert capsys.readouterr().out.splitlines() == rec['printed']
    assert image_size == rec['image_size'] == [42, 18]                      # [width, height], as the reference returns it
    assert len(got) == rec['arrays'] == (3 if run_60 else 2)
    for n, a in enumerate(got):
        want = arrays['%s_%d' % (tag, n)]
        assert a.dtype == want.dtype == np.float32 and a.shape == want.shape and a.tobytes() == want.tobytes()
    # SCALE = 0 / None: no division
    got, _ = patches.OpenDataFilesTest(str(tmp_path), run_60, 0)
    assert np.array_equal(got[0], np.load(str(tmp_path / 'data10.npy')))
    assert 'The SCALE is: 1' in capsys.readouterr().out


def test_command_lines_list_their_arguments():
    r = subprocess.run([sys.executable, '-m', 'dsen2_amd.train', '--help'], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and '--predict' in r.stdout and '--true' in r.stdout and '--resume' in r.stdout
    r = subprocess.run([sys.executable, '-m', 'dsen2_amd.evaluate', '--help'], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0
    for flag in ('--path', '--run_60', '--model_nr', '--json'):
        assert flag in r.stdout
    a = train.parse_args(['--predict', 'm/s2_999_lr_1e-04.npy', '--true', '--path', 'p'])
    assert (a.predict_file, a.true, a.run_60, a.deep, a.path, a.resume_file) == ('m/s2_999_lr_1e-04.npy', True, False, False, 'p', None)
    assert train.model_number(a.predict_file) == 's2_999_' and train.model_number('x/s2_032_lr_1e-04.hdf5') == 's2_032_'
    a = evaluate.parse_args([])
    assert (a.path, a.run_60, a.model_nr, a.json) == ('../data/', False, 's2_038_', None)


class FakeModel(object):
    def __init__(self):
        self.calls = []

    def load_weights(self, path):
        self.calls.append(('load', path))

    def predict(self, x, batch_size=None, verbose=0):
        self.calls.append(('predict', [a.shape for a in x], batch_size, float(x[0].max())))
        return np.ones((x[0].shape[0], 6) + x[0].shape[2:], np.float32)


@pytest.mark.parametrize('flags, folder, border', [([], 'test/', 4), (['--run_60'], 'test60/', 12), (['--true', '--run_60'], 'true/', 12)])
def test_predict_branch_layout_and_rows_columns(tmp_path, monkeypatch, capsys, flags, folder, border):
    """Every *SAFE directory in sorted order; <model_nr>-predict.npy = recompose * SCALE; recompose_images gets (rows, columns)
    = (height, width) although image_size is [width, height]."""
    seen = []

    def recompose(a, border, size=None):
        seen.append((a.shape, border, tuple(size)))
        return np.full((size[0], size[1], a.shape[1]), 0.5, np.float32)
    monkeypatch.setattr(patches, 'recompose_images', recompose)
    for name in ('B.SAFE', 'A.SAFE', 'ignored'):
        ifx.opendata_dir(str(tmp_path / folder / name), '--run_60' in flags)
    args = train.parse_args(['--predict', str(tmp_path / 's2_999_lr_1e-04.npy'), '--path', str(tmp_path)] + flags)
    model = FakeModel()
    assert train.predict(model, args, str(tmp_path) + '/') == 0
    out = capsys.readouterr().out.splitlines()
    assert out[0] == 'Changing the model number to: s2_999_' and out[1].startswith('Predicting using file: ')
    assert [ln for ln in out if ln.startswith('Predicting: ')] == ['Predicting: A.SAFE.', 'Predicting: B.SAFE.']
    assert out.count('Timer started.') == 2 and out.count('Writing to file...') == 2 and len([ln for ln in out if ln.startswith('Elapsed time: ')]) == 2
    assert 'The true_scale is: %s' % ('--true' in flags) in out
    assert model.calls[0] == ('load', args.predict_file)
    n_in = 3 if '--run_60' in flags else 2
    assert [c[1:3] for c in model.calls[1:]] == [([(3, 4, 8, 8), (3, 6, 8, 8), (3, 2, 8, 8)][:n_in], 8)] * 2
    assert all(c[3] < 9000 / 2000.0 for c in model.calls[1:])                 # the inputs were divided by SCALE
    assert seen == [((3, 6, 8, 8), border, (18, 42))] * 2                     # roi.json [6, 12, 48, 30]: 42 wide, 18 high
    for name in ('A.SAFE', 'B.SAFE'):
        img = np.load(str(tmp_path / folder / name / 's2_999_-predict.npy'))
        assert img.shape == (18, 42, 6) and img.dtype == np.float32 and (img == 1000).all()
    assert not os.path.exists(str(tmp_path / folder / 'ignored' / 's2_999_-predict.npy'))


def _host_sums(x, gt):
    x, gt = np.asarray(x, np.float64), np.asarray(gt, np.float64)
    return np.stack([((x - gt) ** 2).sum(axis=(0, 1)), gt.sum(axis=(0, 1)), np.full(gt.shape[2], gt.shape[0] * gt.shape[1], np.float64)], axis=1)


def test_evaluate_prints_the_demo_block_and_writes_json(tmp_path, monkeypatch, capsys):
    rng = np.random.RandomState(3)
    monkeypatch.setattr(metrics, 'error_sums', _host_sums)
    monkeypatch.setattr(metrics, 'bicubic_error_sums', lambda lr, gt, scale: _host_sums(np.repeat(np.repeat(lr, scale, 0), scale, 1), gt))
    want = {}
    for name, with_pred in (('A.SAFE', True), ('B.SAFE', False)):
        d = tmp_path / 'test' / name / 'no_tiling'
        os.makedirs(str(d))
        gt = rng.randint(100, 9000, size=(8, 12, 6)).astype(np.float32)
        lr = gt[::2, ::2] + 3
        np.save(str(d / 'data20_gt.npy'), gt)
        np.save(str(d / 'data20.npy'), lr)
        want[name] = {'bicubic': float(np.sqrt(np.mean((np.repeat(np.repeat(lr, 2, 0), 2, 1).astype(np.float64) - gt) ** 2)))}
        if with_pred:
            pred = gt + rng.randint(-5, 6, size=gt.shape).astype(np.float32)
            np.save(str(tmp_path / 'test' / name / 's2_999_-predict.npy'), pred)
            want[name]['dsen2'] = float(np.sqrt(np.mean((pred.astype(np.float64) - gt) ** 2)))
            want[name]['band'] = np.sqrt(np.mean((pred.astype(np.float64) - gt) ** 2, axis=(0, 1)))
            want[name]['sre'] = 10 * np.log10(gt.astype(np.float64).mean(axis=(0, 1)) ** 2 / np.mean((pred.astype(np.float64) - gt) ** 2, axis=(0, 1)))
    os.makedirs(str(tmp_path / 'test' / 'not_a_test_set'))
    out_json = str(tmp_path / 'scores.json')
    assert evaluate.main(['--path', str(tmp_path), '--model_nr', 's2_999_', '--json', out_json]) == 0
    out = capsys.readouterr().out.splitlines()
    i = out.index('A.SAFE')
    assert out[i:i + 5] == ['A.SAFE', 'DSen2:', 'RMSE: {:.4f}'.format(want['A.SAFE']['dsen2']), 'Bicubic:', 'RMSE: {:.4f}'.format(want['A.SAFE']['bicubic'])]
    j = out.index('B.SAFE')
    assert out[j:j + 3] == ['B.SAFE', 'Bicubic:', 'RMSE: {:.4f}'.format(want['B.SAFE']['bicubic'])]          # no prediction: the baseline alone
    assert 'Mean over 2 tile(s)' in out and 'not_a_test_set' not in out
    rec = json.load(open(out_json))
    assert sorted(rec['tiles']) == ['A.SAFE', 'B.SAFE'] and 'dsen2' not in rec['tiles']['B.SAFE']
    a = rec['tiles']['A.SAFE']
    assert abs(a['dsen2']['rmse'] - want['A.SAFE']['dsen2']) <= 1e-12 * want['A.SAFE']['dsen2']
    np.testing.assert_allclose(a['dsen2']['band_rmse'], want['A.SAFE']['band'], rtol=1e-12)
    np.testing.assert_allclose(a['dsen2']['band_sre'], want['A.SAFE']['sre'], rtol=1e-12)
    assert rec['mean']['dsen2']['tiles'] == 1 and rec['mean']['bicubic']['tiles'] == 2
    assert abs(rec['mean']['bicubic']['rmse'] - (want['A.SAFE']['bicubic'] + want['B.SAFE']['bicubic']) / 2) < 1e-9
    # nothing to score
    assert evaluate.main(['--path', str(tmp_path / 'nowhere')]) == 2


def test_metrics_have_no_host_fallback(monkeypatch):
    """numpy inputs without a GPU: the package's usual error, never a silent host computation."""
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    x = np.ones((4, 4, 2), np.float32)
    for call in (lambda: metrics.RMSE(x, x), lambda: metrics.band_errors(x, x), lambda: metrics.bicubic_errors(x[:2, :2], x, 2),
                 lambda: metrics.RMSE(torch.ones(4, 4, 2), x)):
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            with contextlib.redirect_stdout(io.StringIO()):
                call()
    # the arithmetic above the sums is the host's: RMSE, SRE and the all-band RMSE of given sums
    sums = np.array([[8.0, 40.0, 4.0], [0.0, 4.0, 4.0]])
    rmse, sre, total = metrics.scores(sums)
    assert rmse.tolist() == [np.sqrt(2.0), 0.0] and total == 1.0
    assert abs(sre[0] - 10 * np.log10(100.0 / 2.0)) < 1e-12 and np.isinf(sre[1])
