"""The SSIM loss term, host side (no GPU): the float64 restatement (tests/ssim_loss_restatement.py) against the SSIM restatement of
the metric and against a torch float64 autograd of T, with and without the mask; the product's host statement (dsen2_amd/losses.py)
against the restatement, bit for bit; compile()'s and train.py's acceptances and refusals; weight 0 keeps today's objects; the four
new C entries are declared, exported, listed, and refuse bad arguments before they touch a device."""
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

import ssim_loss_restatement as S  # noqa: E402
import ssim_restatement as Q  # noqa: E402

from dsen2_amd import losses  # noqa: E402
from dsen2_amd.metrics import ssim_window  # noqa: E402

L = 5.0
C1, C2 = (0.01 * L) ** 2, (0.03 * L) ** 2


def _pair(shape=(2, 2, 37, 45), seed=0):
    """(out, y) float32 NCHW in the normalised reflectance domain (0.1 .. 2.5, errors of a few percent); in y a 4 x 13 rectangle of
    blank pixels in sample 0, one blank pixel in sample 1, a pixel blank in one band only (data) and a -0.0 pixel (blank)."""
    n, c, h, w = shape
    rng = np.random.default_rng(seed)
    y = rng.uniform(0.1, 2.5, shape).astype(np.float32)
    out = (y + rng.normal(0.0, 0.05, shape)).astype(np.float32)
    y[0, :, 5:9, 7:20] = 0.0
    y[n - 1, :, h - 3, w - 2] = 0.0
    y[n - 1, 0, 2, 2] = 0.0
    if c > 1:
        assert y[n - 1, 1, 2, 2] != 0
    y[n - 1, :, h - 1, 0] = -0.0
    return out, y


def test_the_q_map_is_the_metric_restatement_bit_for_bit():
    out, y = _pair()
    for P in (11, 7, 3):
        q = S.maps(out, y, ssim_window(P, 1.5), C1, C2, 0)[0]
        for s in range(out.shape[0]):
            for b in range(out.shape[1]):
                want = Q.ssim_map_band(out[s, b], y[s, b], L, win_size=P, sigma=1.5)
                assert q[s, b].tobytes() == want.tobytes(), (P, s, b)


def _torch_term(out, y, g, mask):
    """T with weight 1 by torch float64 autograd: conv2d with the outer product of the window, the mask applied by hand."""
    x = torch.tensor(out.astype(np.float64), requires_grad=True)
    t = torch.tensor(y.astype(np.float64))
    n, c, h, w = x.shape
    P = len(g)
    k = torch.tensor(np.outer(g, g))[None, None]

    def f(v):
        return torch.nn.functional.conv2d(v.reshape(n * c, 1, h, w), k).reshape(n, c, h - P + 1, w - P + 1)
    mx, my, exx, eyy, exy = f(x), f(t), f(x * x), f(t * t), f(x * t)
    q = ((2 * mx * my + C1) * (2 * (exy - mx * my) + C2)) / ((mx * mx + my * my + C1) * ((exx - mx * mx) + (eyy - my * my) + C2))
    live = torch.ones_like(q)
    if mask:
        blank = torch.tensor((~S.valid_pixels(y)).astype(np.float64))
        live = (torch.nn.functional.conv2d(blank, torch.ones(1, 1, P, P, dtype=torch.float64)) == 0).to(torch.float64).expand_as(q)
    T = ((1 - q) * live).sum() / q.numel()
    T.backward()
    return float(T.detach()), x.grad.numpy(), live.numpy().astype(bool)


@pytest.mark.parametrize('mask', [0, 1])
@pytest.mark.parametrize('P', [11, 7, 3])
def test_the_gradient_matches_a_float64_autograd(P, mask):
    """Relative L2 <= 1e-10: the formula alone is at 1e-15; the cancellation in exx - mx^2 can amplify double round-off by about
    mean^2 / c2 = 2e3; a wrong or missing term shows at 1e-3 or worse."""
    out, y = _pair()
    g = ssim_window(P, 1.5)
    T64, grad64, live64 = _torch_term(out, y, g, mask)
    live = S.maps(out, y, g, C1, C2, mask)[4]
    assert np.array_equal(live, live64)
    if mask:
        share = 1.0 - live.mean()
        print('P %d: %.1f %% of the windows are masked' % (P, 100 * share))
        assert 0 < share <= 0.75
        assert live[1, 1, 0, 0] and not live[1, 0, out.shape[2] - P, 0]         # one band blank: data; -0.0: blank
    Nw = S.windows(out.shape, P)
    grad = -S.big_g(out, y, g, C1, C2, mask) / Nw
    err = float(np.linalg.norm(grad - grad64) / np.linalg.norm(grad64))
    T = S.term(out, y, 1.0, g, C1, C2, mask)
    print('P %d mask %d: gradient rel. L2 %.2e, T %.6e against %.6e' % (P, mask, err, T, T64))
    assert err <= 1e-10
    assert abs(T - T64) <= 1e-12 * abs(T64)
    if mask:                                                                    # a masked pixel's SSIM gradient is exactly 0
        blank = np.broadcast_to(~S.valid_pixels(y), out.shape)
        assert blank.any() and not grad[blank].any()


def test_the_float32_accumulation_rounds_once_and_leaves_the_other_lanes():
    out, y = _pair((1, 3, 12, 13))
    g = ssim_window(7, 1.5)
    g16 = np.random.default_rng(1).uniform(-1e-3, 1e-3, (12 * 13, 16)).astype(np.float32)
    res = S.accumulate(g16, out, y, 0.2, g, C1, C2, 0)
    assert res.dtype == np.float32 and np.array_equal(res[:, 3:], g16[:, 3:]) and not np.array_equal(res[:, :3], g16[:, :3])
    G = S.big_g(out, y, g, C1, C2, 0).transpose(0, 2, 3, 1).reshape(-1, 3)
    want = (g16[:, :3].astype(np.float64) + (-float(np.float32(0.2)) / S.windows(out.shape, 7)) * G).astype(np.float32)
    assert res[:, :3].tobytes() == want.tobytes()


@pytest.mark.parametrize('shape,P', [((1, 1, 11, 11), 11), ((3, 6, 32, 32), 11), ((2, 2, 37, 45), 11), ((1, 3, 40, 33), 7),
                                     ((1, 15, 16, 16), 3)])
def test_the_product_statement_is_the_restatement_bit_for_bit(shape, P):
    rng = np.random.default_rng(5)
    y = rng.uniform(0.1, 2.5, shape).astype(np.float32)
    out = (y + rng.normal(0.0, 0.05, shape)).astype(np.float32)
    if shape[2] > P:
        y[0, :, 1, 2] = 0.0
    for mask in (0, 1):
        setting = losses.parse_ssim(losses.parse('mae', None, bool(mask)), 0.25, P, 1.5, L)
        window, c1, c2 = losses.ssim_constants(losses.ssim_part(setting))
        assert window.tobytes() == ssim_window(P, 1.5).tobytes() and (c1, c2) == (C1, C2)
        got = np.array(losses.ssim_sums(out, y, setting))
        want = S.sums(out, y, window, c1, c2, mask)
        assert got.tobytes() == want.tobytes(), (got, want)
        # every window is summed by exactly one tile
        t, live = losses.ssim_window_terms(out, y, window, c1, c2, mask)
        assert got[2] == live.sum() and abs(got[0] - np.where(live, t, 0.0).sum()) <= 1e-12 * abs(got[0])


def test_host_loss_with_the_term():
    out, y = _pair()
    for name, param, mask in (('mae', None, False), ('huber', 0.03, True)):
        base = losses.parse(name, param, mask)
        setting = losses.parse_ssim(base, 0.2, 11, 1.5, L)
        plain = losses.host_sums(out, y, base)
        sr, sq, cnt = losses.host_sums(out, y, setting)
        s = losses.ssim_sums(out, y, setting)
        fixed = losses.fixed_order_sum(losses.terms(out, y, base)[0])
        assert sr == fixed + s[0] * losses.ssim_fold(setting, out.shape) and cnt == out.size and sq == losses.fixed_order_sum(losses.terms(out, y, base)[1])
        total, mse = losses.host_loss(out, y, setting)
        assert total == sr / cnt and mse == sq / cnt
        T = S.term(out, y, 0.2, ssim_window(11, 1.5), C1, C2, int(mask))
        assert total == pytest.approx(fixed / cnt + T, rel=1e-14) and T > 0 and total > plain[0] / cnt
        text = losses.describe(setting)
        assert '0.2 x (1 - SSIM), window 11' in text and text.startswith(name) and text.endswith('masked') == mask
    with pytest.raises(ValueError):
        losses.host_loss(out[:, :, :8, :8], y[:, :, :8, :8], setting)


def test_weight_zero_keeps_todays_objects_and_bits():
    out, y = _pair()
    for args in (('mae', None, False), ('mse', None, True), ('charbonnier', 0.01, False)):
        base = losses.parse(*args)
        for w in (0.0, 0, -0.0, np.float32(0)):
            assert losses.parse_ssim(base, w) == base and len(losses.parse_ssim(base, w)) == 3
        assert losses.ssim_part(base) is None and losses.pointwise(base) == base
    assert losses.parse_ssim(losses.DEFAULT) == losses.DEFAULT == (0, 0.0, 0)
    r, q = losses.terms(out, y, losses.DEFAULT)
    assert losses.host_loss(out, y) == [float(np.mean(r)), float(np.mean(q))]
    assert losses.host_sums(out, y) == (float(np.sum(r)), float(np.sum(q)), float(r.size))
    assert losses.describe(losses.parse('huber', 0.03, True)) == 'huber(0.03), no-data pixels masked'


def test_parse_refusals():
    base = losses.DEFAULT
    assert losses.parse_ssim(base, 0.2) == (0, 0.0, 0, (float(np.float32(0.2)), 11, 1.5, 5.0))
    for kw in (dict(ssim_weight=-0.1), dict(ssim_weight=float('nan')), dict(ssim_weight=float('inf')), dict(ssim_weight='much'),
               dict(ssim_weight=0.2, ssim_win=10), dict(ssim_weight=0.2, ssim_win=13), dict(ssim_weight=0.2, ssim_win=1),
               dict(ssim_weight=0.2, ssim_win=7.5), dict(ssim_weight=0.2, ssim_sigma=0.0), dict(ssim_weight=0.2, ssim_sigma=float('nan')),
               dict(ssim_weight=0.2, ssim_data_range=0.0), dict(ssim_weight=0.2, ssim_data_range=float('inf')),
               dict(ssim_weight=0.0, ssim_win=4)):
        with pytest.raises(ValueError):
            losses.parse_ssim(base, **kw)


def test_compile_signature_and_refusals_before_it_touches_the_handle():
    from dsen2_amd.DSen2Net import S2Model
    sig = inspect.signature(S2Model.compile)
    for name, default in (('ssim_weight', 0.0), ('ssim_win', 11), ('ssim_sigma', 1.5), ('ssim_data_range', 5.0)):
        assert sig.parameters[name].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters[name].default == default
    m = S2Model.__new__(S2Model)
    m.precision, m._handle = 'fp32', None
    for kw in (dict(ssim_weight=-1.0), dict(ssim_weight=0.2, ssim_win=12), dict(ssim_weight=0.2, ssim_win=15),
               dict(ssim_weight=0.2, ssim_data_range=-5.0), dict(ssim_weight=float('nan'))):
        with pytest.raises(ValueError):
            m.compile(**kw)
    assert getattr(m, 'optimizer', None) is None and not hasattr(m, 'loss_setting')
    b = S2Model.__new__(S2Model)
    b.precision, b._handle = 'bf16', None
    with pytest.raises(ValueError):
        b.compile(ssim_weight=0.2)


def test_train_cli_flags():
    from dsen2_amd import train
    a = train.parse_args([])
    assert (a.ssim_weight, a.ssim_win, a.ssim_sigma, a.ssim_data_range) == (0.0, 11, 1.5, 5.0)
    a = train.parse_args(['--ssim_weight', '0.2', '--ssim_win', '7', '--ssim_sigma', '1.0', '--ssim_data_range', '2.5', '--mask_nodata'])
    assert (a.ssim_weight, a.ssim_win, a.ssim_sigma, a.ssim_data_range, a.mask_nodata) == (0.2, 7, 1.0, 2.5, True)
    for bad in (['--ssim_weight', '-1'], ['--ssim_weight', 'nan'], ['--ssim_weight', '0.2', '--ssim_win', '8'],
                ['--ssim_weight', '0.2', '--ssim_win', '13'], ['--ssim_weight', '0.2', '--ssim_sigma', '0'],
                ['--ssim_weight', '0.2', '--predict', 'w.npy']):
        with pytest.raises(SystemExit):
            train.parse_args(bad)
    assert '--ssim_weight' in train.__doc__


def test_c_abi_declares_exports_and_checks_the_new_entries():
    from dsen2_amd import _lib, build
    build.build()
    lib = _lib.load()
    header = open(os.path.join(ROOT, 'include', 'dsen2_hip.h')).read()
    for name in ('dsen2_model_set_loss_ssim', 'dsen2_ssim_loss_grad', 'dsen2_ssim_loss_sums_workspace_bytes', 'dsen2_ssim_loss_sums'):
        assert re.search(r'\bint %s\s*\(' % name, header) and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert 'ssim_loss.hip' in build.SOURCES
    a, b, c, d = (ctypes.c_void_p(0x1000 * k) for k in (1, 2, 3, 4))       # never dereferenced: every call below is refused first
    win = (ctypes.c_double * 11)(*ssim_window(11, 1.5).tolist())

    def refused(fn, *args, code=_lib.ERR_INVALID):
        assert fn(*args) == code
        return lib.dsen2_last_error().decode()
    assert 'NULL' in refused(lib.dsen2_model_set_loss_ssim, None, 0.2, win, 11, C1, C2)
    f = lib.dsen2_ssim_loss_grad
    for k in range(4):
        ptrs = [a, b, c, d]
        ptrs[k] = None
        assert 'NULL' in refused(f, ptrs[0], ptrs[1], 1, 6, 32, 32, 0.2, win, 11, C1, C2, 0, ptrs[2], ptrs[3], None)
    for shape in ((0, 6, 32, 32), (1, 0, 32, 32), (1, 16, 32, 32), (1, 6, 0, 32), (1, 6, 32, -1)):
        assert 'bad shape' in refused(f, a, b, *shape, 0.2, win, 11, C1, C2, 0, c, d, None)
    assert 'mask mode 2' in refused(f, a, b, 1, 6, 32, 32, 0.2, win, 11, C1, C2, 2, c, d, None)
    for weight in (-0.5, float('nan'), float('inf')):
        assert 'weight' in refused(f, a, b, 1, 6, 32, 32, weight, win, 11, C1, C2, 0, c, d, None)
    for P in (10, 1, 13, 15, -3):
        assert 'window size' in refused(f, a, b, 1, 6, 32, 32, 0.2, win, P, C1, C2, 0, c, d, None)
    assert 'NULL window' in refused(f, a, b, 1, 6, 32, 32, 0.2, None, 11, C1, C2, 0, c, d, None)
    bad_win = (ctypes.c_double * 11)(*([0.1] * 10 + [float('nan')]))
    assert 'not finite' in refused(f, a, b, 1, 6, 32, 32, 0.2, bad_win, 11, C1, C2, 0, c, d, None)
    for c1, c2 in ((0.0, C2), (C1, -1.0), (float('nan'), C2), (C1, float('inf'))):
        assert 'constants' in refused(f, a, b, 1, 6, 32, 32, 0.2, win, 11, c1, c2, 0, c, d, None)
    for h, w in ((10, 32), (32, 10)):
        assert 'smaller than' in refused(f, a, b, 1, 6, h, w, 0.2, win, 11, C1, C2, 0, c, d, None)
    need = ctypes.c_size_t(0)
    assert lib.dsen2_ssim_loss_sums_workspace_bytes(ctypes.byref(need)) == _lib.OK and need.value == (4096 * 2 + 3) * 8
    assert 'NULL' in refused(lib.dsen2_ssim_loss_sums_workspace_bytes, None)
    s = lib.dsen2_ssim_loss_sums
    for k in range(4):
        ptrs = [a, b, c, d]
        ptrs[k] = None
        assert 'NULL' in refused(s, ptrs[0], ptrs[1], 1, 6, 32, 32, win, 11, C1, C2, 0, ptrs[2], need.value, ptrs[3], None)
    assert 'bad shape' in refused(s, a, b, 1, 16, 32, 32, win, 11, C1, C2, 0, c, need.value, d, None)
    assert 'window size' in refused(s, a, b, 1, 6, 32, 32, win, 12, C1, C2, 0, c, need.value, d, None)
    assert 'smaller than' in refused(s, a, b, 1, 6, 8, 32, win, 11, C1, C2, 0, c, need.value, d, None)
    assert 'workspace' in refused(s, a, b, 1, 6, 32, 32, win, 11, C1, C2, 0, c, need.value - 8, d, None, code=_lib.ERR_WORKSPACE)
