"""Fine-tuning, host side (no GPU): the Nadam scalar schedule, ReduceLROnPlateau, the data loader, save_weights -> load_flat,
the training CLI's flags, and the weight-gradient kernels' geometry query (tiles, split count, workspace)."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from dsen2_amd import training, weights  # noqa: E402


def test_nadam_scalar_schedule_matches_keras_formula():
    opt = training.Nadam(lr=1e-4, beta_1=0.9, beta_2=0.999, epsilon=1e-8, schedule_decay=0.004)
    m_schedule = 1.0
    for t in range(1, 6):
        s = opt.next_step()
        mc_t = 0.9 * (1.0 - 0.5 * np.power(0.96, t * 0.004, dtype=np.float64))
        mc_t1 = 0.9 * (1.0 - 0.5 * np.power(0.96, (t + 1) * 0.004, dtype=np.float64))
        ms_new = m_schedule * mc_t
        ms_next = ms_new * mc_t1
        m_schedule = ms_new
        assert s['t'] == t and opt.iterations == t
        for k, want in (('mc_t', mc_t), ('mc_t1', mc_t1), ('ms_new', ms_new), ('ms_next', ms_next),
                        ('b2_pow_t', 0.999 ** t)):
            assert s[k] == pytest.approx(want, rel=1e-15, abs=0), (t, k)
    opt.reset()
    assert opt.iterations == 0 and opt.m_schedule == 1.0
    assert opt.next_step()['ms_new'] == pytest.approx(0.9 * (1 - 0.5 * 0.96 ** 0.004), rel=1e-15)


def test_reduce_lr_on_plateau_patience_cooldown_and_min_lr():
    cb = training.ReduceLROnPlateau(factor=0.5, patience=2, min_delta=1e-6, cooldown=3, min_lr=0.3)
    lr = 1.0
    # improves twice, then stalls: two epochs without an improvement of more than min_delta -> halve; cooldown 3: the
    # counter reaches 0 on the third epoch after, which counts again (keras), one more stall -> halve again, clamped to
    # min_lr; at min_lr it never changes again
    series = [1.0, 0.9, 0.9 - 1e-7, 0.95, 0.9, 0.9, 0.9, 0.9, 0.9, 0.9, 0.9, 0.9, 0.9, 0.9]
    lrs = []
    for v in series:
        lr = cb.step(v, lr)
        lrs.append(lr)
    assert lrs == [1.0, 1.0, 1.0, 0.5, 0.5, 0.5, 0.5, 0.3, 0.3, 0.3, 0.3, 0.3, 0.3, 0.3]
    assert cb.best == 0.9
    # an improvement during the cooldown still resets the best value
    cb = training.ReduceLROnPlateau(factor=0.5, patience=1, min_delta=0.0, cooldown=2, min_lr=0.0)
    assert [cb.step(v, 1.0) for v in (1.0, 1.0)] == [1.0, 0.5]
    assert cb.step(0.5, 0.5) == 0.5 and cb.best == 0.5 and cb.cooldown_counter == 1


def test_reduce_lr_callback_sets_optimizer_lr():
    class M(object):
        optimizer = training.Nadam(lr=1e-4)
    cb = training.ReduceLROnPlateau(factor=0.5, patience=5, min_delta=1e-6, cooldown=20, min_lr=1e-5)
    cb.set_model(M())
    for epoch in range(6):
        cb.on_epoch_end(epoch, {'val_loss': 1.0})
    assert M.optimizer.lr == pytest.approx(5e-5)
    assert cb.cooldown_counter == 20


def _write_safe(d, n, rng, run_60):
    os.makedirs(d)
    arrays = {'data10': rng.uniform(0, 4000, (n, 4, 8, 8)), 'data20': rng.uniform(0, 4000, (n, 6, 8, 8))}
    if run_60:
        arrays['data60'] = rng.uniform(0, 4000, (n, 2, 8, 8))
        arrays['data60_gt'] = rng.uniform(0, 4000, (n, 2, 8, 8))
    else:
        arrays['data20_gt'] = rng.uniform(0, 4000, (n, 6, 8, 8))
    for k, a in arrays.items():
        np.save(os.path.join(d, k + '.npy'), a.astype(np.float32))
    return arrays


@pytest.mark.parametrize('run_60', [False, True])
def test_load_training_data_splits_by_val_index_and_scales(tmp_path, run_60):
    rng = np.random.default_rng(0)
    train_dir = tmp_path / ('train60' if run_60 else 'train')
    a = _write_safe(str(train_dir / 'S2B_B.SAFE'), 5, rng, run_60)
    b = _write_safe(str(train_dir / 'S2A_A.SAFE'), 4, rng, run_60)      # sorted first
    os.makedirs(str(train_dir / 'notes'))                               # not a *SAFE directory: ignored
    val = np.zeros(9, bool)
    val[[1, 6]] = True
    np.save(str(train_dir / 'val_index.npy'), val)
    train, label, val_tr, val_lb = training.load_training_data(str(tmp_path), run_60=run_60)
    names = ['data10', 'data20'] + (['data60'] if run_60 else [])
    gt = 'data60_gt' if run_60 else 'data20_gt'
    assert len(train) == len(val_tr) == len(names)
    for k, tr, va in zip(names, train, val_tr):
        full = np.concatenate([b[k], a[k]]).astype(np.float32) / np.float32(2000)
        assert tr.dtype == np.float32
        np.testing.assert_array_equal(tr, full[~val])
        np.testing.assert_array_equal(va, full[val])
    full = np.concatenate([b[gt], a[gt]]).astype(np.float32) / np.float32(2000)
    np.testing.assert_array_equal(label, full[~val])
    np.testing.assert_array_equal(val_lb, full[val])


def test_load_training_data_without_tiles_raises(tmp_path):
    with pytest.raises(OSError):
        training.load_training_data(str(tmp_path))


def test_save_weights_file_round_trips_through_load_flat(tmp_path):
    """S2Model.save_weights writes np.save of the flat vector: load_flat reads it back, also under the .hdf5 name the
    inference path asks for (the .npy fallback)."""
    from dsen2_amd.DSen2Net import S2Model
    flat = weights.random_he_uniform(10, 6, 1, 128, seed=4, bias_scale=0.1)

    class Fake(object):
        def get_weights_flat(self):
            return flat
    path = str(tmp_path / 's2_032_lr_1e-04.npy')
    S2Model.save_weights(Fake(), path)
    back = weights.load_flat(path, 10, 6, 1, 128)
    np.testing.assert_array_equal(back, flat)
    back = weights.load_flat(str(tmp_path / 's2_032_lr_1e-04.hdf5'), 10, 6, 1, 128)
    np.testing.assert_array_equal(back, flat)


def test_model_checkpoint_saves_only_improvements(tmp_path):
    saved = []

    class M(object):
        def save_weights(self, path):
            saved.append(path)
    cb = training.ModelCheckpoint(str(tmp_path / 'w.npy'))
    cb.set_model(M())
    for epoch, v in enumerate([1.0, 0.8, 0.9, 0.8, 0.7]):
        cb.on_epoch_end(epoch, {'val_loss': v})
    assert len(saved) == 3 and cb.best == 0.7


def test_train_cli_help_lists_reference_flags():
    r = subprocess.run([sys.executable, '-m', 'dsen2_amd.train', '--help'], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    for flag in ('--path', '--resume', '--run_60', '--deep', '--epochs', '--lr', '--batch_size', '--out'):
        assert flag in r.stdout, flag


def test_train_cli_model_number_like_reference():
    from dsen2_amd import train
    assert train.model_number('../models/s2_032_lr_1e-04.hdf5') == 's2_032_'
    assert train.model_number('/x/s2_034_lr_1e-04.npy') == 's2_034_'
    assert '../models/s2_032_lr_1e-04.hdf5'[-20:-13] == 's2_032_'      # training/supres_train.py's slice


def test_train_cli_refuses_data_parallel():
    env = dict(os.environ, WORLD_SIZE='2')
    r = subprocess.run([sys.executable, '-m', 'dsen2_amd.train', '--epochs', '1'], cwd=ROOT, capture_output=True, text=True,
                       timeout=120, env=env)
    assert r.returncode != 0 and 'WORLD_SIZE' in r.stderr


# ---- dsen2_conv3x3_wgrad_geometry: the split-K geometry of the three weight-gradient kernels, without a device ----
def test_wgrad_geometry_is_declared_exported_and_refuses_bad_arguments():
    from dsen2_amd import _lib, build
    build.build()
    lib = _lib.load()
    header = open(os.path.join(ROOT, 'include', 'dsen2_hip.h')).read()
    name = 'dsen2_conv3x3_wgrad_geometry'
    assert re.search(r'\bint %s\s*\(' % name, header) and name in _lib.SIGNATURES and hasattr(lib, name)
    tiles, splits, floats = ctypes.c_longlong(0), ctypes.c_int(0), ctypes.c_size_t(0)
    out = [ctypes.byref(tiles), ctypes.byref(splits), ctypes.byref(floats)]

    def refused(*args):
        assert lib.dsen2_conv3x3_wgrad_geometry(*args) == _lib.ERR_INVALID
        return lib.dsen2_last_error().decode()
    for k in range(3):
        args = list(out)
        args[k] = None
        assert 'NULL' in refused(0, 2, 16, 16, 128, 128, *args)
    assert 'kind' in refused(3, 2, 16, 16, 128, 128, *out)
    assert 'kind' in refused(-1, 2, 16, 16, 128, 128, *out)
    assert 'bad shape' in refused(0, 0, 16, 16, 128, 128, *out)
    assert 'bad shape' in refused(1, 2, 16, -1, 128, 128, *out)
    assert 'no wgrad kernel' in refused(0, 2, 16, 16, 128, 64, *out)       # the fp32 kernel: cg % 128 == 0, or cg <= 32 with ca % 128 == 0
    assert 'no wgrad kernel' in refused(0, 2, 16, 16, 16, 16, *out)
    for kind in (1, 2):
        assert 'unsupported' in refused(kind, 2, 16, 16, 64, 64, *out)
        assert 'unsupported' in refused(kind, 2, 16, 16, 128, 256, *out)
        assert 'unsupported' in refused(kind, 2, 16, 16, 16, 128, *out)     # the first layer stays on the fp32 kernel


# (kind, ca, cg, cip, cop) -> the split count once there are enough tiles: 256 / the number of (co, ci) blocks.  The fp32
# kernel's block is 128 co x 32 ci (body, first layer) or 32 co x 128 ci (output layer), the bf16 kernels' 128 co x 32 ci.
WGRAD_SPLITS = [
    ('fp32', 128, 128, 128, 128, 64), ('fp32', 256, 256, 256, 256, 16),         # body
    ('fp32', 16, 128, 32, 128, 256), ('fp32', 16, 256, 32, 256, 128),           # first layer (NHWC16 input)
    ('fp32', 128, 16, 128, 32, 256), ('fp32', 256, 16, 256, 32, 128),           # output layer (dL/dout padded to 16)
    ('bf16x3', 128, 128, 128, 128, 64), ('bf16x3', 256, 256, 256, 256, 16),
    ('bf16', 128, 128, 128, 128, 64), ('bf16', 256, 256, 256, 256, 16),
]


@pytest.mark.parametrize('kind,ca,cg,cip,cop,splits', WGRAD_SPLITS)
def test_wgrad_geometry_pins_tiles_splits_and_workspace(kind, ca, cg, cip, cop, splits):
    from dsen2_amd import build
    from dsen2_amd.DSen2Net import conv3x3_wgrad_geometry
    build.build()
    # the timed shapes (32 x 32 patches, batch 128 and 8), ragged ones, one image wider than it is high, fewer tiles than splits
    for n, h, w in ((128, 32, 32), (8, 32, 32), (9, 32, 32), (7, 21, 37), (19, 21, 37), (40, 32, 32), (2, 21, 37), (1, 8, 600),
                    (3, 20, 28), (1, 1, 1), (1, 4, 16), (1, 5, 17)):
        want_tiles = n * ((h + 3) // 4) * ((w + 15) // 16)
        got_tiles, got_splits, floats = conv3x3_wgrad_geometry(kind, n, h, w, ca, cg)
        assert got_tiles == want_tiles, (n, h, w)
        assert got_splits == min(splits, want_tiles), (n, h, w)
        assert floats == got_splits * (9 * cip * cop + 2 * cop), (n, h, w)
    assert conv3x3_wgrad_geometry(kind, 128, 32, 32, ca, cg)[:2] == (2048, splits)      # DSen2, batch 128
    assert conv3x3_wgrad_geometry(kind, 8, 32, 32, ca, cg)[:2] == (128, min(splits, 128))

