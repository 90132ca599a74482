"""The geometric self-ensemble (dsen2_model_forward_ensemble; S2Model.forward_device_ensemble, predict(ensemble=...), the tile
path's SELF_ENSEMBLE switch).

Pinned bit for bit against tests/dihedral_restatement.py built on the model's OWN predict of numpy-turned inputs: members in
ascending op order, fp32 sum, one fp32 divide.  The accuracy gate is against the float64 oracle's ensemble, which differs from
the oracle's plain forward by four orders of magnitude more than the gate, so a plain forward cannot pass it."""
import contextlib
import functools
import io
import os

import numpy as np
import pytest
import torch

import dihedral_restatement as dr

pytestmark = pytest.mark.gpu

from oracle import c_oracle
from oracle import dsen2_oracle as do

RMSE_GATE = 1e-4                    # the project's fp32 gate in the network's normalised domain
D, F, N = 2, 128, 3
NETS = [(4, 6), (4, 6, 2)]
SIZES = [(16, 24), (32, 32)]
PRECISIONS = ['fp32', 'bf16', 'bf16x3']
MASKS = [True, (0, 4), (3,)]


def _same_bits(a, b):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else a
    return a.shape == b.shape and a.dtype == b.dtype == np.float32 and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@functools.lru_cache(maxsize=None)
def _model(bands, precision):
    from dsen2_amd.DSen2Net import s2model
    m = s2model(tuple((b, None, None) for b in bands), num_layers=D, feature_size=F, precision=precision)
    m.set_weights_flat(do.he_uniform_weights(sum(bands), bands[-1], D, F, seed=1))
    return m


def _inputs(bands, h, w, n=N):
    return do.synthetic_inputs(n, h, w, bands, seed=0)


@pytest.mark.parametrize('h,w', SIZES)
@pytest.mark.parametrize('bands', NETS, ids=['20m', '60m'])
@pytest.mark.parametrize('precision', PRECISIONS)
def test_ensemble_equals_its_restatement_bit_for_bit(precision, bands, h, w):
    m = _model(bands, precision)
    xs = _inputs(bands, h, w)
    dev = [torch.from_numpy(a).to(m.device) for a in xs]
    plain = m.predict(xs)
    for ops in MASKS:
        want = dr.ensemble(m.predict, xs, ops)
        members = range(8) if ops is True else ops
        got_dev = m.forward_device_ensemble(dev, ops=members)
        assert _same_bits(got_dev, want), (precision, bands, h, w, ops, 'forward_device_ensemble')
        assert _same_bits(m.predict(xs, ensemble=ops), want), (precision, bands, h, w, ops, 'predict')
        for a, d in zip(xs, dev):                                   # the inputs are only read
            assert _same_bits(d, a)
        if ops is True:
            assert not np.array_equal(want, plain)                  # (the network is not equivariant: the ensemble is not a no-op)
    # an `out` of the caller's is written in place
    out = torch.empty((N, bands[-1], h, w), dtype=torch.float32, device=m.device)
    assert m.forward_device_ensemble(dev, out=out) is out
    assert _same_bits(out, dr.ensemble(m.predict, xs, True))


@pytest.mark.parametrize('precision', PRECISIONS)
def test_member_zero_alone_is_the_plain_forward(precision):
    for bands in NETS:
        for h, w in SIZES:
            m = _model(bands, precision)
            xs = _inputs(bands, h, w)
            plain = m.predict(xs)
            assert _same_bits(m.predict(xs, ensemble=[0]), plain)
            dev = [torch.from_numpy(a).to(m.device) for a in xs]
            assert _same_bits(m.forward_device_ensemble(dev, ops=[0]), plain)
            # ... with the plain forward's workspace
            assert m.workspace_bytes(N, h, w, ensemble=[0]) == m.workspace_bytes(N, h, w) < m.workspace_bytes(N, h, w, ensemble=True)
            assert _same_bits(m.predict(xs, ensemble=False), plain)


@pytest.mark.parametrize('precision', PRECISIONS)
def test_batching_is_invisible(precision):
    m = _model((4, 6), precision)
    for h, w in SIZES:
        xs = _inputs((4, 6), h, w)
        assert _same_bits(m.predict(xs, ensemble=True, batch_size=2), m.predict(xs, ensemble=True))
        assert m.batch_limit(h, w, ensemble=True) <= m.batch_limit(h, w)
        assert 1 <= m.preferred_batch(h, w, ensemble=True) <= m.batch_limit(h, w, ensemble=True)
    empty = [np.zeros((0, c, 16, 24), np.float32) for c in (4, 6)]
    assert m.predict(empty, ensemble=True).shape == (0, 6, 16, 24)


def test_fp32_ensemble_against_the_float64_oracle():
    """c_oracle.forward on the 8 turned inputs, turned back and averaged in float64.  Weights seed 1, inputs seed 0, 2 x 16 x 24."""
    bands, h, w = (4, 6), 16, 24
    flat = do.he_uniform_weights(10, 6, D, F, seed=1)
    xs = _inputs(bands, h, w, n=2)
    oracle = lambda turned: c_oracle.forward(turned, flat, D, F)    # noqa: E731
    ref = dr.ensemble_f64(oracle, xs)
    plain = np.asarray(oracle(xs), np.float64)
    gap = do.rmse(ref, plain)
    print('oracle: ensemble vs plain forward rmse', gap)
    assert gap > 1000 * RMSE_GATE                                   # a plain forward cannot pass for the ensemble
    got = _model(bands, 'fp32').predict(xs, ensemble=True)
    err = do.rmse(got, ref)
    print('fp32 self-ensemble rmse vs float64 oracle', err)
    assert err < RMSE_GATE
    for precision, bound in (('bf16x3', RMSE_GATE),):
        e = do.rmse(_model(bands, precision).predict(xs, ensemble=True), ref)
        print('%s self-ensemble rmse vs float64 oracle' % precision, e)
        assert e < bound


def test_refusals_launch_nothing():
    import ctypes
    from dsen2_amd import _lib
    from dsen2_amd.DSen2Net import _ptr, _stream_ptr
    m = _model((4, 6), 'fp32')
    n, h, w = 2, 16, 24
    dev = [torch.from_numpy(a).to(m.device) for a in _inputs((4, 6), h, w, n=n)]
    out = torch.full((n, 6, h, w), -7.5, dtype=torch.float32, device=m.device)
    need = m.workspace_bytes(n, h, w, ensemble=True)
    ws = torch.zeros(need, dtype=torch.uint8, device=m.device)
    lib, NULL, s = _lib.load(), ctypes.c_void_p(0), _stream_ptr(m.device)

    def call(x10=dev[0], x20=dev[1], x60=None, o=out, hh=h, ww=w, mask=255, wsp=ws, nbytes=need, nn=n):
        with torch.cuda.device(m.device):
            code = lib.dsen2_model_forward_ensemble(m._handle, _ptr(x10), _ptr(x20), _ptr(x60), _ptr(o), nn, hh, ww, mask, _ptr(wsp), nbytes, s)
        torch.cuda.synchronize()
        return code

    for kw in (dict(mask=0), dict(mask=256), dict(mask=-1), dict(x10=None), dict(x20=None), dict(o=None), dict(wsp=None),
               dict(x60=dev[1]), dict(hh=1 << 13, ww=1 << 13), dict(nn=-1)):
        assert call(**kw) == _lib.ERR_INVALID, kw
    assert call(nbytes=need - 1) == _lib.ERR_WORKSPACE
    assert call(mask=2, nbytes=m.workspace_bytes(n, h, w)) == _lib.ERR_WORKSPACE         # the plain forward's is too short for a turned member
    assert bool((out == -7.5).all()) and not bool(ws.any())
    assert call(o=dev[1], mask=1) == _lib.ERR_INVALID                                    # out aliases an input
    assert call(nn=0) == _lib.OK and bool((out == -7.5).all())
    size = ctypes.c_size_t(0)
    for mask in (0, 256):
        assert lib.dsen2_model_ensemble_workspace_bytes(m._handle, n, h, w, mask, ctypes.byref(size)) == _lib.ERR_INVALID
    assert call() == _lib.OK and not bool((out == -7.5).any())
    with pytest.raises(ValueError):
        m.predict([a.cpu().numpy() for a in dev], ensemble=[8])
    with pytest.raises(ValueError):
        m.forward_device_ensemble(dev, ops=[])


# ---- the tile path ------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def tile_model(tmp_path, monkeypatch):
    from dsen2_amd import supres
    flat = do.he_uniform_weights(10, 6, 6, 128, seed=11, bias_scale=0.02)
    np.save(str(tmp_path / 's2_032_lr_1e-04.npy'), flat)
    monkeypatch.setattr(supres, 'MDL_PATH', str(tmp_path) + os.sep)
    monkeypatch.setattr(supres, 'PRECISION', 'fp32')
    supres.clear_model_cache()
    yield supres
    supres.clear_model_cache()


def _quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def _restated_tile(supres, d10, d20, patch, border, ensemble):
    """The tile path from its pieces: the package's tiling and up-sampling, /2000, predict on the used patches, the existing
    recomposition with its x 2000."""
    from dsen2_amd import patches
    p10, p20 = patches.get_test_patches(d10, d20, patchSize=patch, border=border)
    x_tiles, y_tiles = patches.recompose_grid(d10.shape, patch, border)
    used = x_tiles * y_tiles
    xs = [p10[:used] / np.float32(supres.SCALE), p20[:used] / np.float32(supres.SCALE)]
    model = _quiet(supres._get_model, ((4, None, None), (6, None, None)), False, False)
    pred = model.predict(xs, ensemble=ensemble)
    assert used > 1
    img = patches.recompose_device(torch.from_numpy(pred).to(model.device), border, d10.shape[:2], scale=supres.SCALE)
    return img.cpu().numpy()


@pytest.mark.parametrize('geometry', ['40x46 patches of 16', 'DSen2_20 136x150'])
def test_tile_path_honours_the_switch(tile_model, monkeypatch, geometry):
    """40 x 46 is below DSen2_20's patch of 128 (which rejects it), so that size runs DSen2_20's own body, supres._run, with the
    geometry scaled to patches of 16 with a border of 2: 4 x 4 patches, the last row and column clamped.  DSen2_20 itself runs on
    the smallest image that gives it 2 x 2 patches."""
    supres = tile_model
    rng = np.random.default_rng(3)
    if geometry.startswith('40x46'):
        H, W, patch, border = 40, 46, 16, 2
        run = lambda a, b: supres._run([a, b], [2, 1], patch=patch, border=border, deep=False, run_60=False)   # noqa: E731
    else:
        H, W, patch, border = 136, 150, 128, 8
        run = lambda a, b: supres.DSen2_20(a, b)                                                                   # noqa: E731
    d10 = rng.integers(35, 6000, size=(H, W, 4)).astype(np.float32)
    d20 = rng.integers(35, 6000, size=(H // 2, W // 2, 6)).astype(np.float32)
    monkeypatch.setattr(supres, 'SELF_ENSEMBLE', False)
    off = _quiet(run, d10, d20)
    assert _same_bits(off, _restated_tile(supres, d10, d20, patch, border, False))           # today's result
    monkeypatch.setattr(supres, 'SELF_ENSEMBLE', True)
    on = _quiet(run, d10, d20)
    assert on.shape == (H, W, 6)
    assert _same_bits(on, _restated_tile(supres, d10, d20, patch, border, True))
    assert not np.array_equal(on, off)
    # _predict (the reference's own entry) honours it too
    xs = do.synthetic_inputs(2, 16, 16, (4, 6), seed=5)
    model = _quiet(supres._get_model, ((4, None, None), (6, None, None)), False, False)
    assert _same_bits(_quiet(supres._predict, xs, ((4, None, None), (6, None, None))), model.predict(xs, ensemble=True))
    monkeypatch.setattr(supres, 'SELF_ENSEMBLE', False)
    assert _same_bits(_quiet(supres._predict, xs, ((4, None, None), (6, None, None))), model.predict(xs))
