"""Flip / rotate augmentation of the fine-tuning step: the inputs and the target of every sample are turned by its own op on the
device after the upload.  Everything here is an identity on bits: a step with augment_ops equals the step on numpy-turned data
(tests/dihedral_restatement.py), a fit(augment=True) equals the host loop that draws the same permutations and the same
training.AugmentOps, and its data-parallel restatement equals the loop with shards."""
import numpy as np
import pytest
import torch

import dihedral_restatement as dr
from dsen2_amd import training, weights
from dsen2_amd.DSen2Net import s2model

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
BANDS, D, F = (4, 6), 2, 128
MODES = {'fp32': ('fp32', None), 'fp32-amp': ('fp32', 'bf16'), 'bf16x3': ('bf16x3', None)}
OPS7 = np.array([5, 0, 3, 6, 1, 7, 2], np.int32)              # every op but the plain flip, op 0 among them


def _data(n, p, seed):
    rng = np.random.default_rng(seed)
    x = [rng.uniform(0.0, 0.5, (n, c, p, p)).astype(np.float32) for c in BANDS]
    return x, rng.uniform(0.0, 0.5, (n, BANDS[-1], p, p)).astype(np.float32)


def _model(mode='fp32', seed=1):
    precision, mixed = MODES[mode]
    m = s2model(tuple((c, None, None) for c in BANDS), num_layers=D, feature_size=F, device=DEV, precision=precision)
    m.set_weights_flat(weights.random_he_uniform(sum(BANDS), BANDS[-1], D, F, seed=seed, bias_scale=0.05))
    m.compile(training.Nadam(lr=1e-3), mixed_precision=mixed)
    return m


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


@pytest.mark.parametrize('shards', [None, 3], ids=['plain', 'shards3'])
@pytest.mark.parametrize('mode', list(MODES))
def test_an_augmented_step_is_the_step_on_turned_data(mode, shards):
    """7 samples of 9 x 9 (a ragged tile); shards=3 cuts them 3 + 2 + 2, so every shard takes its own slice of the ops."""
    x, y = _data(7, 9, 21)
    a, b, plain = _model(mode), _model(mode), _model(mode)
    la = a.train_on_batch(x, y, shards=shards, augment_ops=OPS7)
    lb = b.train_on_batch([dr.per_sample(t, OPS7) for t in x], dr.per_sample(y, OPS7), shards=shards)
    assert la == lb
    wa, wb = a.get_weights_flat(), b.get_weights_flat()
    assert _same_bits(wa, wb)
    plain.train_on_batch(x, y, shards=shards)
    assert not np.array_equal(wa, plain.get_weights_flat())       # the ops did something
    # all-zero ops are no augmentation at all
    c = _model(mode)
    assert c.train_on_batch(x, y, shards=shards, augment_ops=np.zeros(7, np.int32)) is not None
    assert _same_bits(c.get_weights_flat(), plain.get_weights_flat())


def test_augment_ops_are_checked_before_anything_runs():
    m = _model()
    x, y = _data(3, 8, 4)
    before = m.get_weights_flat()
    for bad in ([0, 1], [0, 1, 8], [0, -1, 2]):
        with pytest.raises(ValueError):
            m.train_on_batch(x, y, augment_ops=bad)
    xr = [t[:, :, :, :6].copy() for t in x]
    with pytest.raises(ValueError):                                 # an odd rotation needs square patches
        m.train_on_batch(xr, y[:, :, :, :6].copy(), augment_ops=[0, 1, 2])
    assert m.optimizer.iterations == 0 and _same_bits(m.get_weights_flat(), before)


def _loop(model, x, y, seed, epochs, batch, shards=None, augment=True):
    """fit's schedule restated on the host: default_rng(seed) permutations, AugmentOps(seed) ops, one train_on_batch per batch."""
    rng = np.random.default_rng(seed)
    aug = training.AugmentOps(seed)
    for _ in range(epochs):
        order = rng.permutation(y.shape[0])
        for i0 in range(0, y.shape[0], batch):
            idx = order[i0:i0 + batch]
            ops = aug.draw(len(idx)) if augment else None
            model.train_on_batch([a[idx] for a in x], y[idx], shards=shards, augment_ops=ops)
    return model.get_weights_flat()


@pytest.fixture(scope='module')
def fit_data():
    return _data(12, 8, 55)             # 12 samples, batch 5: batches of 5, 5 and 2


def test_fit_with_augmentation_equals_the_host_loop(fit_data):
    x, y = fit_data
    m = _model()
    h = m.fit(x, y, batch_size=5, epochs=2, verbose=0, seed=9, augment=True, validation_data=(x, y))
    want = _loop(_model(), x, y, 9, 2, 5)
    assert _same_bits(m.get_weights_flat(), want)
    assert len(h.history['val_loss']) == 2
    # validation is never augmented: val_loss is evaluate() on the data as given
    assert h.history['val_loss'][-1] == m.evaluate(x, y, batch_size=5)[0]
    # ... and the augmentation is not a no-op
    assert not np.array_equal(want, _loop(_model(), x, y, 9, 2, 5, augment=False))


def test_data_parallel_restatement_equals_the_loop_with_shards(fit_data):
    x, y = fit_data
    m = _model()
    m.fit(x, y, batch_size=5, epochs=2, verbose=0, seed=9, augment=True, data_parallel=True, emulate_world=2)
    assert _same_bits(m.get_weights_flat(), _loop(_model(), x, y, 9, 2, 5, shards=2))


def test_fit_without_augmentation_is_unchanged_run_to_run(fit_data):
    x, y = fit_data
    runs = []
    for _ in range(2):
        m = _model()
        m.fit(x, y, batch_size=5, epochs=2, verbose=0, seed=9)
        runs.append(m.get_weights_flat())
    assert _same_bits(runs[0], runs[1])
    assert _same_bits(runs[0], _loop(_model(), x, y, 9, 2, 5, augment=False))       # the permutations of the augmented fit
    m = _model()
    m.fit(x, y, batch_size=5, epochs=2, verbose=0, seed=9, augment=False)
    assert _same_bits(m.get_weights_flat(), runs[0])
