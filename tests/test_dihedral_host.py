"""Host side of the self-ensemble and of the training augmentation (no GPU): the restatement's own properties, the op
generator, the command-line flags, and the loud failure without a device."""
import numpy as np
import pytest
import torch

import dihedral_restatement as dr
from dsen2_amd import DSen2Net, training


def _plane(h, w, seed=0):
    return np.random.default_rng(seed).standard_normal((2, 3, h, w)).astype(np.float32)


# ---- the restatement ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('h,w', [(3, 3), (2, 5)])
def test_the_eight_ops_are_distinct_and_swap_the_shape_for_odd_turns(h, w):
    a = _plane(h, w)
    outs = [dr.forward(a, op) for op in dr.OPS]
    for op, b in enumerate(outs):
        assert b.shape == ((2, 3, w, h) if op & 1 else (2, 3, h, w)), op
        assert b.flags['C_CONTIGUOUS']
    for i in dr.OPS:
        for j in dr.OPS:
            if i < j and outs[i].shape == outs[j].shape:
                assert not np.array_equal(outs[i], outs[j]), (i, j)
    assert np.array_equal(outs[0], a)
    assert np.array_equal(outs[4], a[..., ::-1])                                  # the flip alone
    assert np.array_equal(outs[1][0, 0], np.rot90(a[0, 0]))                       # one quarter turn, counter-clockwise


@pytest.mark.parametrize('h,w', [(4, 4), (3, 7)])
def test_inverse_undoes_forward_and_is_itself_one_of_the_eight(h, w):
    a = _plane(h, w, 1)
    for op in dr.OPS:
        b = dr.forward(a, op)
        assert np.array_equal(dr.inverse(b, op), a), op
        assert np.array_equal(dr.forward(dr.inverse(a, op), op), a), op
        # a rotation's inverse is the opposite rotation, a reflection (f = 1) is its own: what lets one gather serve both
        inv = op if op & 4 else (4 - op) & 3
        assert np.array_equal(dr.inverse(b, op), dr.forward(b, inv)), op


def test_per_sample_and_ensemble_restatements():
    a = _plane(5, 5, 2)
    ops = np.array([7, 2], np.int32)
    t = dr.per_sample(a, ops)
    assert np.array_equal(t[0], dr.forward(a[0], 7)) and np.array_equal(t[1], dr.forward(a[1], 2))
    assert np.array_equal(dr.per_sample(t, ops, inv=True), a)
    assert dr.members(True) == list(range(8)) and dr.members([4, 0, 4]) == [0, 4]
    # a predictor that commutes with every op: the ensemble is the plain prediction, up to the rounding of sum and divide
    ident = lambda xs: xs[0] * np.float32(2)                                      # noqa: E731
    assert np.array_equal(dr.ensemble(ident, [a], [3]), ident([a]))
    e8 = dr.ensemble(ident, [a])
    assert e8.dtype == np.float32 and np.allclose(e8, ident([a]), rtol=1e-6)
    # one that does not (it reads its upper-left neighbourhood): the ensemble differs from the plain prediction
    shift = lambda xs: np.roll(xs[0], 1, axis=-1)                                 # noqa: E731
    assert not np.allclose(dr.ensemble(shift, [a]), shift([a]))
    assert np.allclose(dr.ensemble_f64(shift, [a]), dr.ensemble(shift, [a]), atol=1e-6)


# ---- the ops of a training step -----------------------------------------------------------------------------------------------
def test_augment_ops_are_a_function_of_the_seed_on_a_stream_of_their_own():
    a, b = training.AugmentOps(7), training.AugmentOps(7)
    d1 = [a.draw(n) for n in (5, 5, 2)]
    d2 = [b.draw(n) for n in (5, 5, 2)]
    for x, y in zip(d1, d2):
        assert x.dtype == np.int32 and np.array_equal(x, y)
    assert d1[0].shape == (5,) and d1[2].shape == (2,)
    big = training.AugmentOps(7).draw(4000)
    assert big.min() == 0 and big.max() == 7 and set(np.unique(big)) == set(range(8))
    assert abs(np.bincount(big, minlength=8) / 4000.0 - 0.125).max() < 0.03
    assert not np.array_equal(training.AugmentOps(8).draw(64), training.AugmentOps(7).draw(64))
    # drawing ops does not touch the shuffle's generator, and is not the shuffle's stream
    rng = np.random.default_rng(7)
    first = rng.permutation(12)
    assert np.array_equal(first, np.random.default_rng(7).permutation(12))
    assert not np.array_equal(training.AugmentOps(7).draw(64), np.random.default_rng(7).integers(0, 8, size=64, dtype=np.int32))
    assert training.AugmentOps(None).draw(3).shape == (3,)


def test_ensemble_mask():
    em = DSen2Net.ensemble_mask
    assert em(False) == 0 and em(None) == 0 and em(True) == 255
    assert em(range(8)) == 255 and em([0]) == 1 and em([0, 4]) == 0x11 and em({3}) == 8
    for bad in ([], [8], [-1], [1.5]):
        with pytest.raises(ValueError):
            em(bad)


# ---- command lines ------------------------------------------------------------------------------------------------------------
def test_train_flags_and_the_augment_predict_refusal(capsys):
    from dsen2_amd import train
    a = train.parse_args([])
    assert a.augment is False and a.self_ensemble is False
    assert train.parse_args(['--augment']).augment is True
    a = train.parse_args(['--predict', 'm/s2_999_lr_1e-04.npy', '--self_ensemble'])
    assert a.self_ensemble is True and a.augment is False
    with pytest.raises(SystemExit):
        train.parse_args(['--predict', 'm/s2_999_lr_1e-04.npy', '--augment'])
    assert '--augment' in capsys.readouterr().err
    with pytest.raises(SystemExit):
        train.parse_args(['--self_ensemble'])                                     # an option of --predict


def test_cli_self_ensemble_sets_the_module_switch(tmp_path, monkeypatch):
    from dsen2_amd import cli, supres
    seen = []

    def fake20(d10, d20, deep=False):
        seen.append(supres.SELF_ENSEMBLE)
        return np.repeat(np.repeat(np.asarray(d20, np.float32), 2, 0), 2, 1)
    monkeypatch.setattr(supres, 'DSen2_20', fake20)
    monkeypatch.setattr(supres, 'SELF_ENSEMBLE', False)
    src = str(tmp_path / 'tile.npz')
    np.savez(src, data10=np.zeros((12, 12, 4), np.uint16), data20=np.ones((6, 6, 6), np.uint16))
    assert cli.main([src, str(tmp_path / 'plain.npz')]) == 0
    assert cli.main([src, str(tmp_path / 'ens.npz'), '--self_ensemble']) == 0
    assert seen == [False, True]


def test_the_environment_switch_is_read_at_import_and_off_by_default():
    """DSEN2_SELF_ENSEMBLE is read when dsen2_amd.supres is imported (the idiom of DSEN2_PRECISION): off here, on in a process
    started with it."""
    import os
    import subprocess
    import sys
    from dsen2_amd import supres
    if os.environ.get('DSEN2_SELF_ENSEMBLE', '0') in ('', '0'):
        assert supres.SELF_ENSEMBLE is False
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, '-c', 'import dsen2_amd.supres as s; print(int(s.SELF_ENSEMBLE is True))'], cwd=root,
                         env=dict(os.environ, DSEN2_SELF_ENSEMBLE='1'), capture_output=True, text=True, check=True).stdout
    assert out.strip().splitlines()[-1] == '1', out


# ---- no device, no fallback ---------------------------------------------------------------------------------------------------
@pytest.mark.skipif(torch.cuda.is_available(), reason='CPU-box behaviour')
def test_new_entry_points_fail_loudly_without_a_gpu():
    x = torch.zeros((1, 2, 4, 4), dtype=torch.float32)
    with pytest.raises(RuntimeError):
        DSen2Net.dihedral(x, op=1)
    with pytest.raises(RuntimeError):
        DSen2Net.dihedral(x, ops=[3])
    with pytest.raises(RuntimeError):                                             # the model the ensemble and the augmented step hang on
        DSen2Net.s2model(((4, None, None), (6, None, None)), num_layers=2, feature_size=128).forward_device_ensemble([x, x])
    from dsen2_amd import supres
    old = supres.SELF_ENSEMBLE
    supres.SELF_ENSEMBLE = True
    try:
        with pytest.raises(RuntimeError):
            supres.DSen2_20(np.zeros((240, 240, 4), np.float32), np.zeros((120, 120, 6), np.float32))
    finally:
        supres.SELF_ENSEMBLE = old
