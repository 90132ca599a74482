"""Losses and the no-data mask, host side (no GPU): the float64 restatement (tests/loss_restatement.py) against
torch.nn.functional in float64, with and without a mask applied by hand; the product's one host statement (dsen2_amd/losses.py)
against the restatement; compile()'s and train.py's acceptances and refusals; the four new C entries are declared, exported,
listed, and refuse bad arguments before touching a device."""
import ctypes
import inspect
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import loss_restatement as R  # noqa: E402

DELTA, EPS = 0.03, 0.01
PARAM = {R.MAE: 0.0, R.MSE: 0.0, R.HUBER: DELTA, R.CHARBONNIER: EPS}


def _pair(seed=0, shape=(3, 6, 5, 7)):
    """(out, y) float32 NCHW with |e| in 0.01 .. 0.06, exact zeros among the errors, a rectangle of blank pixels, pixels blank in
    some bands only, a -0.0 pixel and a negative one."""
    rng = np.random.default_rng(seed)
    out = rng.uniform(0.1, 0.5, shape).astype(np.float32)
    s = np.where(rng.uniform(size=shape) < 0.5, -1.0, 1.0)
    y = (out + s * (0.01 + rng.uniform(0.0, 0.05, shape))).astype(np.float32)
    y.ravel()[::11] = out.ravel()[::11]
    y[:, :, :2, :3] = 0.0
    y[0, :, 4, 6] = -0.0
    y[1, ::2, 3, 3] = 0.0
    y[2, :, 4, 0] = -0.25
    return out, y


def _torch_loss(e, kind):
    zero = torch.zeros_like(e)
    F = torch.nn.functional
    if kind == R.MAE:
        return F.l1_loss(e, zero, reduction='none')
    if kind == R.MSE:
        return F.mse_loss(e, zero, reduction='none')
    if kind == R.HUBER:
        return F.huber_loss(e, zero, reduction='none', delta=float(np.float32(DELTA)))
    return torch.sqrt(e * e + float(np.float32(EPS)) ** 2)


@pytest.mark.parametrize('mask', [0, 1])
@pytest.mark.parametrize('kind', R.KINDS)
def test_restatement_against_torch_float64(kind, mask):
    out, y = _pair()
    d = (out - y).astype(np.float64)
    v = R.valid(y, mask)
    assert (not mask) or (0 < int(v.sum()) < v.size and not v[:, :, :2, :3].any() and not v[0, 0, 4, 6] and v[1, 0, 3, 3] and v[2, 0, 4, 0])
    e = torch.tensor(d, requires_grad=True)
    per = _torch_loss(e, kind) * torch.tensor(np.broadcast_to(v, d.shape).astype(np.float64))       # the mask, by hand
    per.sum().backward()
    want_rho, want_slope = per.detach().numpy(), e.grad.numpy()
    got_rho = np.where(v, R.rho(d, kind, PARAM[kind]), 0.0)
    got_slope = np.where(v, R.slope(d, kind, PARAM[kind]), 0.0)
    np.testing.assert_allclose(got_rho, want_rho, rtol=1e-14, atol=0)
    np.testing.assert_allclose(got_slope, want_slope, rtol=1e-14, atol=0)
    assert (got_slope[d == 0] == 0).all() and (d == 0).sum() > 10
    # dL/dout and the pair as dsen2_loss_grad writes them
    g16, (loss, mse) = R.loss_grad(out, y, kind, PARAM[kind], mask)
    n, c, h, w = out.shape
    assert g16.shape == (n * h * w, 16) and g16.dtype == np.float32 and not g16[:, c:].any()
    inv = float(np.float32(1.0 / out.size))
    np.testing.assert_allclose(g16[:, :c].reshape(n, h, w, c).transpose(0, 3, 1, 2), want_slope * inv, rtol=2.0 ** -23, atol=0)
    assert loss == pytest.approx(want_rho.sum() / out.size, rel=1e-12) and mse == pytest.approx((np.where(v, d * d, 0)).sum() / out.size, rel=1e-12)
    sums = R.loss_sums(out, y, kind, PARAM[kind], mask)
    d2 = out.astype(np.float64) - y.astype(np.float64)
    assert sums[0] == pytest.approx(np.where(v, R.rho(d2, kind, PARAM[kind]), 0).sum(), rel=1e-12)
    assert sums[2] == float(np.broadcast_to(v, d.shape).sum())


def test_huber_delta_puts_a_quarter_of_the_elements_on_each_branch():
    out, y = _pair()
    a = np.abs((out - y).astype(np.float64))
    assert (a <= float(np.float32(DELTA))).mean() >= 0.25 and (a > float(np.float32(DELTA))).mean() >= 0.25


def test_product_statement_is_the_restatement():
    from dsen2_amd import losses
    out, y = _pair(seed=2)
    d = out.astype(np.float64) - y.astype(np.float64)
    for kind in R.KINDS:
        assert np.array_equal(losses.rho(d, kind, PARAM[kind]), R.rho(d, kind, PARAM[kind]))
        assert np.array_equal(losses.slope(d, kind, PARAM[kind]), R.slope(d, kind, PARAM[kind]))
        for mask in (0, 1):
            setting = (kind, PARAM[kind], mask)
            sums = R.loss_sums(out, y, kind, PARAM[kind], mask)
            got = losses.host_sums(out, y, setting)
            if setting == losses.DEFAULT:          # the statement evaluate() always was
                assert got == (float(np.sum(np.abs(d))), float(np.sum(d * d)), float(d.size))
                assert losses.host_loss(out, y, setting) == [float(np.mean(np.abs(d))), float(np.mean(d * d))]
            else:                                  # dsen2_loss_sums' order; the denominator counts masked elements too
                assert got == (sums[0], sums[1], float(d.size))
                assert losses.host_loss(out, y, setting) == [sums[0] / d.size, sums[1] / d.size]
    assert np.array_equal(losses.valid_pixels(y), R.valid(y, 1))
    mse = losses.host_loss(out, y, (R.MSE, 0.0, 1))
    assert mse[0] == mse[1]


def test_parse_accepts_and_refuses():
    from dsen2_amd import losses
    assert losses.parse('mean_absolute_error') == losses.parse('mae') == losses.DEFAULT == (0, 0.0, 0)
    assert losses.parse('mean_squared_error') == losses.parse('mse') == (1, 0.0, 0)
    assert losses.parse('huber', 0.03, True) == (2, float(np.float32(0.03)), 1)
    assert losses.parse('charbonnier', loss_param=0.01) == (3, float(np.float32(0.01)), 0)
    for bad in (dict(loss='huber'), dict(loss='charbonnier'), dict(loss='mae', loss_param=1.0), dict(loss='mse', loss_param=0.1),
                dict(loss='huber', loss_param=0.0), dict(loss='huber', loss_param=-1.0), dict(loss='huber', loss_param=float('nan')),
                dict(loss='charbonnier', loss_param=float('inf')), dict(loss='charbonnier', loss_param=1e-60),
                dict(loss='logcosh'), dict(loss=None), dict(loss='MSE')):
        with pytest.raises(ValueError):
            losses.parse(**bad)


def test_compile_signature_keeps_the_new_arguments_keyword_only():
    from dsen2_amd.DSen2Net import S2Model
    sig = inspect.signature(S2Model.compile)
    assert sig.parameters['loss_param'].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters['loss_param'].default is None
    assert sig.parameters['mask_nodata'].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters['mask_nodata'].default is False
    assert sig.parameters['loss'].default == 'mean_absolute_error'
    assert 'min_delta' in S2Model.compile.__doc__


def test_compile_refuses_before_it_touches_the_handle():
    """compile() on an object that has no handle: every refusal comes before the first library call."""
    from dsen2_amd.DSen2Net import S2Model
    m = S2Model.__new__(S2Model)
    m.precision, m._handle = 'fp32', None
    for kw in (dict(loss='logcosh'), dict(loss='huber'), dict(loss='mse', loss_param=0.1), dict(loss='charbonnier', loss_param=0.0)):
        with pytest.raises(ValueError):
            m.compile(**kw)
    assert getattr(m, 'optimizer', None) is None and not hasattr(m, 'loss_setting')


def test_train_cli_flags():
    from dsen2_amd import train
    a = train.parse_args([])
    assert (a.loss, a.loss_param, a.mask_nodata) == (None, None, False)
    a = train.parse_args(['--loss', 'charbonnier', '--loss_param', '0.01', '--mask_nodata', '--data_parallel', '--emulate_world', '2'])
    assert (a.loss, a.loss_param, a.mask_nodata) == ('charbonnier', 0.01, True)
    assert train.parse_args(['--loss', 'mse', '--tiles', 'a.npz', '--mixed_precision', 'bf16']).loss == 'mse'
    assert train.parse_args(['--mask_nodata', '--precision', 'bf16x3']).mask_nodata is True
    for bad in (['--loss', 'huber'], ['--loss', 'charbonnier'], ['--loss_param', '0.1'], ['--loss', 'mse', '--loss_param', '0.1'],
                ['--loss', 'huber', '--loss_param', '0'], ['--loss', 'huber', '--loss_param', '-1'], ['--loss', 'huber', '--loss_param', 'nan'],
                ['--loss', 'huber', '--loss_param', 'inf'], ['--loss', 'logcosh'], ['--loss', 'mse', '--predict', 'w.npy'],
                ['--mask_nodata', '--predict', 'w.npy']):
        with pytest.raises(SystemExit):
            train.parse_args(bad)
    assert '--loss' in train.__doc__ and '--mask_nodata' in train.__doc__


def test_c_abi_declares_exports_and_checks_the_new_entries():
    from dsen2_amd import _lib, build
    build.build()
    lib = _lib.load()
    header = open(os.path.join(ROOT, 'include', 'dsen2_hip.h')).read()
    for name in ('dsen2_model_set_loss', 'dsen2_loss_grad', 'dsen2_loss_sums_workspace_bytes', 'dsen2_loss_sums'):
        assert re.search(r'\bint %s\s*\(' % name, header) and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert 'loss_terms.h' in ' '.join(build.HEADERS)
    a, b, c, d = (ctypes.c_void_p(0x1000 * k) for k in (1, 2, 3, 4))       # never dereferenced: every call below is refused first

    def refused(fn, *args, code=_lib.ERR_INVALID):
        assert fn(*args) == code
        return lib.dsen2_last_error().decode()
    assert 'NULL' in refused(lib.dsen2_model_set_loss, None, 1, 0.0, 0)
    f = lib.dsen2_loss_grad
    for k in range(4):
        ptrs = [a, b, c, d]
        ptrs[k] = None
        assert 'NULL' in refused(f, ptrs[0], ptrs[1], 1, 6, 4, 4, 0, 0.0, 0, ptrs[2], ptrs[3], None)
    for shape in ((0, 6, 4, 4), (1, 0, 4, 4), (1, 16, 4, 4), (1, 6, 0, 4), (1, 6, 4, -1)):
        assert 'bad shape' in refused(f, a, b, *shape, 0, 0.0, 0, c, d, None)
    assert 'kind 4' in refused(f, a, b, 1, 6, 4, 4, 4, 0.0, 0, c, d, None)
    assert 'kind -1' in refused(f, a, b, 1, 6, 4, 4, -1, 0.0, 0, c, d, None)
    assert 'mask mode 2' in refused(f, a, b, 1, 6, 4, 4, 1, 0.0, 2, c, d, None)
    for kind in (2, 3):
        for param in (0.0, -0.5, float('nan'), float('inf')):
            assert 'parameter' in refused(f, a, b, 1, 6, 4, 4, kind, param, 0, c, d, None)
    need = ctypes.c_size_t(0)
    assert lib.dsen2_loss_sums_workspace_bytes(ctypes.byref(need)) == _lib.OK and need.value == 4096 * 2 * 2 * 8 + 32
    assert 'NULL' in refused(lib.dsen2_loss_sums_workspace_bytes, None)
    s = lib.dsen2_loss_sums
    for k in range(4):
        ptrs = [a, b, c, d]
        ptrs[k] = None
        assert 'NULL' in refused(s, ptrs[0], ptrs[1], 1, 6, 16, 0, 0.0, 0, ptrs[2], need.value, ptrs[3], None)
    for n, ch, hw in ((0, 6, 16), (1, 0, 16), (1, 6, 0), (1, 6, -4)):
        assert 'bad shape' in refused(s, a, b, n, ch, hw, 0, 0.0, 0, c, need.value, d, None)
    assert 'outside 1..2^31 - 1' in refused(s, a, b, 2, 1, 1 << 30, 0, 0.0, 0, c, need.value, d, None)
    assert 'outside 1..2^31 - 1' in refused(s, a, b, 1 << 20, 1 << 12, 1 << 40, 0, 0.0, 0, c, need.value, d, None)
    assert 'kind 7' in refused(s, a, b, 1, 6, 16, 7, 0.0, 0, c, need.value, d, None)
    assert 'mask mode -1' in refused(s, a, b, 1, 6, 16, 0, 0.0, -1, c, need.value, d, None)
    assert 'parameter' in refused(s, a, b, 1, 6, 16, 2, 0.0, 0, c, need.value, d, None)
    assert 'workspace' in refused(s, a, b, 1, 6, 16, 1, 0.0, 1, c, need.value - 1, d, None, code=_lib.ERR_WORKSPACE)


def test_the_product_does_not_import_the_restatement():
    for dirpath, _, files in os.walk(os.path.join(ROOT, 'dsen2_amd')):
        for name in files:
            if name.endswith('.py'):
                assert 'loss_restatement' not in open(os.path.join(dirpath, name)).read(), name
