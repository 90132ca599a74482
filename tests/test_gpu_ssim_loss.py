"""The SSIM loss term on the GPU (include/dsen2_hip.h, "the SSIM loss term"): dsen2_ssim_loss_grad and dsen2_ssim_loss_sums bit for
bit against the float64 restatement (tests/ssim_loss_restatement.py) inside guard bands, onto a non-zero gradient, with and without
the mask; the mask cases; identities that need no gate; the sums against dsen2_ssim_sums; whole-step gradients with MAE plus the
term against a float64 torch autograd of graph and loss; train_on_batch, fit, fit_corpus validating on the device against host
arrays; two gloo ranks against the one-process restatement; refusals."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import ssim_loss_restatement as S  # noqa: E402
import test_gpu_train as T  # noqa: E402            (the graph, the cases and the target construction of the fp32 step's tests)
import test_gpu_train_bf16x3 as X  # noqa: E402     (the margin and a safe case of the bf16x3 step's tests)
import test_gpu_train_parallel as P  # noqa: E402   (ranks against the one-process restatement)
from guarded import run_three_ways  # noqa: E402

from dsen2_amd import _lib, corpus, losses, metrics, training, weights  # noqa: E402
from dsen2_amd.DSen2Net import _ptr, _stream_ptr, s2model  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)

L = 5.0
C1, C2 = (0.01 * L) ** 2, (0.03 * L) ** 2
WEIGHT = 0.2
# (n, c, h, w), P: one window; the training shape, one tile; several tiles, ragged, window ownership across tile seams; the 60 m
# shape; the most lanes and the smallest window; a middle window (tiles of another size)
SHAPES = [((1, 1, 11, 11), 11), ((3, 6, 32, 32), 11), ((2, 2, 37, 45), 11), ((2, 2, 96, 96), 11), ((1, 15, 16, 16), 3), ((1, 3, 40, 33), 7)]
# 4200 items (sample, band, tile) > the grid's cap of 4096 workgroups: the first 104 take a second item; sample 0 is wholly masked
ABOVE_THE_GRID_CAP = ((300, 14, 11, 11), 11)


def _cwin(window):
    return (ctypes.c_double * len(window))(*np.asarray(window).tolist())


@functools.lru_cache(maxsize=None)
def _pair(shape, P):
    """(out, y, g16) computed once and never modified: a float32 NCHW pair in the normalised reflectance domain, y with a blank
    rectangle and one blank pixel where the plane has room for them, and a non-zero NHWC16 starting gradient, all 16 lanes."""
    n, c, h, w = shape
    rng = np.random.default_rng(n * 1000 + c * 100 + h)
    y = rng.uniform(0.1, 2.5, shape).astype(np.float32)
    out = (y + rng.normal(0.0, 0.05, shape)).astype(np.float32)
    if h > 2 * P:
        y[0, :, 5:9, 7:20] = 0.0
        y[n - 1, :, h - 3, w - 2] = 0.0
    elif h > P:
        y[0, :, 0, 1] = 0.0
    elif n > 1:
        y[0, :, h // 2, w // 2] = 0.0
    g16 = rng.uniform(-1e-4, 1e-4, (n * h * w, 16)).astype(np.float32)
    for a in (out, y, g16):
        a.setflags(write=False)
    return out, y, g16


@functools.lru_cache(maxsize=None)
def _want(shape, P, mask):
    out, y, g16 = _pair(shape, P)
    window = metrics.ssim_window(P, 1.5)
    return S.accumulate(g16, out, y, WEIGHT, window, C1, C2, mask), S.sums(out, y, window, C1, C2, mask)


def _grad_call(out, y, P, mask, g16, weight=WEIGHT, c1=C1, c2=C2):
    """dsen2_ssim_loss_grad on device tensors; returns (gradient, sums2) as numpy."""
    n, c, h, w = out.shape
    sums2 = torch.zeros(2, dtype=torch.float64, device=DEV)
    with torch.cuda.device(DEV):
        _lib.call('dsen2_ssim_loss_grad', _ptr(out), _ptr(y), n, c, h, w, weight, _cwin(metrics.ssim_window(P, 1.5)), P, c1, c2, mask,
                  _ptr(g16), _ptr(sums2), _stream_ptr(DEV))
    return g16.cpu().numpy(), sums2.cpu().numpy()


def _sums_need():
    need = ctypes.c_size_t(0)
    _lib.call('dsen2_ssim_loss_sums_workspace_bytes', ctypes.byref(need))
    return int(need.value)


# ---- (a) the two entries against the restatement, inside guard bands ----------------------------------------------------------------
@pytest.mark.parametrize('mask', [0, 1])
@pytest.mark.parametrize('shape,P', SHAPES + [ABOVE_THE_GRID_CAP])
def test_ssim_loss_grad_equals_the_restatement_bit_for_bit(shape, P, mask):
    out, y, g16 = _pair(shape, P)
    n, c, h, w = shape
    want_g, want_s = _want(shape, P, mask)
    if mask and (h > P or n > 1):
        assert 0 < want_s[2] < want_s[1]
    inp = [torch.from_numpy(out.copy()).to(DEV), torch.from_numpy(y.copy()).to(DEV)]
    window = _cwin(metrics.ssim_window(P, 1.5))

    def call(i, o, inplace, _scratch):
        with torch.cuda.device(DEV):
            _lib.call('dsen2_ssim_loss_grad', _ptr(i[0]), _ptr(i[1]), n, c, h, w, WEIGHT, window, P, C1, C2, mask, _ptr(inplace[0]),
                      _ptr(o[0]), _stream_ptr(DEV))
    (sums2,), (g,) = run_three_ways(call, inp, [((2,), torch.float64)], inplace=[torch.from_numpy(g16.copy()).to(DEV)], device=DEV,
                                    what='ssim_loss_grad %r P %d mask %d' % (shape, P, mask))
    g, sums2 = g.cpu().numpy(), sums2.cpu().numpy()
    bad = g.view(np.uint32) != want_g.view(np.uint32)
    print('ssim_loss_grad %r P %d mask %d: %d of %d lanes differ; sums %r, restatement %r' % (shape, P, mask, int(bad.sum()), bad.size,
                                                                                              sums2.tolist(), want_s[:2].tolist()))
    assert not bad.any(), np.argwhere(bad)[:8]
    assert np.array_equal(g[:, c:].view(np.uint32), g16[:, c:].view(np.uint32))             # lanes >= c: what was there
    assert not np.array_equal(g[:, :c], g16[:, :c])
    assert sums2.tobytes() == want_s[:2].tobytes()


@pytest.mark.parametrize('mask', [0, 1])
@pytest.mark.parametrize('shape,P', SHAPES + [ABOVE_THE_GRID_CAP])
def test_ssim_loss_sums_equal_the_restatement_bit_for_bit(shape, P, mask):
    out, y, _ = _pair(shape, P)
    n, c, h, w = shape
    want = _want(shape, P, mask)[1]
    inp = [torch.from_numpy(out.copy()).to(DEV), torch.from_numpy(y.copy()).to(DEV)]
    window = _cwin(metrics.ssim_window(P, 1.5))

    def call(i, o, _inplace, scratch):
        with torch.cuda.device(DEV):
            _lib.call('dsen2_ssim_loss_sums', _ptr(i[0]), _ptr(i[1]), n, c, h, w, window, P, C1, C2, mask, _ptr(scratch[0]),
                      scratch[0].numel(), _ptr(o[0]), _stream_ptr(DEV))
    (got,), _ = run_three_ways(call, inp, [((3,), torch.float64)], scratch=[_sums_need()], device=DEV,
                               what='ssim_loss_sums %r P %d mask %d' % (shape, P, mask))
    got = got.cpu().numpy()
    print('ssim_loss_sums %r P %d mask %d: kernel %r restatement %r' % (shape, P, mask, got.tolist(), want.tolist()))
    assert got.tobytes() == want.tobytes()
    setting = losses.parse_ssim(losses.parse('mae', None, bool(mask)), WEIGHT, P, 1.5, L)
    assert np.array(losses.ssim_sums(out, y, setting)).tobytes() == got.tobytes()              # the product's host statement too


# ---- (b) the mask cases --------------------------------------------------------------------------------------------------------------
def _mask_case(name):
    shape, P = ((2, 2, 37, 45), 11)
    out, y, _ = _pair(shape, P)
    y = y.copy()
    y[0, :, 5:9, 7:20] = np.float32(1.0) + y[1, :, 5:9, 7:20]          # undo _pair's own blanks
    y[1, :, 34, 43] = 1.5
    assert S.valid_pixels(y).all()
    if name == 'rectangle':
        y[0, :, 5:9, 7:20] = 0.0
    elif name == 'rectangle and pixel':
        y[0, :, 5:9, 7:20] = 0.0
        y[1, :, 20, 30] = 0.0
    elif name == 'one pixel':
        y[1, :, 20, 30] = 0.0
    elif name == 'some bands only':          # blank in band 0 alone: data; next to one truly blank pixel
        y[0, 0, 10, 10] = 0.0
        y[1, :, 3, 40] = 0.0
    elif name == 'minus zero':
        y[1, :, 36, 0] = -0.0
    elif name == 'blank sample':
        y[0] = 0.0
    return out, y, shape, P


@pytest.mark.parametrize('name', ['rectangle', 'rectangle and pixel', 'one pixel', 'some bands only', 'minus zero', 'blank sample'])
def test_mask_cases(name):
    out, y, shape, P = _mask_case(name)
    n, c, h, w = shape
    window = metrics.ssim_window(P, 1.5)
    live = S.maps(out, y, window, C1, C2, 1)[4]
    share = 1.0 - live.mean()
    print('%s: %.1f %% of the windows are masked' % (name, 100 * share))
    assert 0 < share <= 0.75                       # the mask masks something and leaves at least a quarter of the windows
    if name == 'some bands only':
        assert live[0, 0, 5, 5] and live[0, 1, 5, 5]
    if name == 'minus zero':
        assert not live[1, 0, 26, 0] and np.signbit(y[1, :, 36, 0]).all()
    g0 = np.zeros((n * h * w, 16), np.float32)
    got_g, got_s = _grad_call(torch.from_numpy(out.copy()).to(DEV), torch.from_numpy(y).to(DEV), P, 1, torch.from_numpy(g0).to(DEV))
    want_g, want_s = S.accumulate(g0, out, y, WEIGHT, window, C1, C2, 1), S.sums(out, y, window, C1, C2, 1)
    assert got_g.view(np.uint32).tobytes() == want_g.view(np.uint32).tobytes()
    assert got_s.tobytes() == want_s[:2].tobytes() and want_s[2] == live.sum()
    blank = np.broadcast_to(~S.valid_pixels(y), shape).transpose(0, 2, 3, 1).reshape(n * h * w, c)
    assert blank.any() and not got_g[:, :c][blank].any()                   # a masked pixel's SSIM gradient is 0
    # and the mask is not a no-op
    off_g, off_s = _grad_call(torch.from_numpy(out.copy()).to(DEV), torch.from_numpy(y).to(DEV), P, 0, torch.from_numpy(g0).to(DEV))
    assert off_s[0] != got_s[0] and not np.array_equal(off_g, got_g)


# ---- (c) identities that need no gate ------------------------------------------------------------------------------------------------
def _bits(t):
    return (t.cpu().numpy() if isinstance(t, torch.Tensor) else t).view(np.uint32)


def test_kernel_identities():
    shape, P = SHAPES[2]
    out, y, _ = _pair(shape, P)
    n, c, h, w = shape
    zeros = lambda: torch.zeros((n * h * w, 16), device=DEV)        # noqa: E731
    o, t = torch.from_numpy(out.copy()).to(DEV), torch.from_numpy(y.copy()).to(DEV)
    # out == target: every q is exactly 1
    _, s_same = _grad_call(t, t, P, 0, zeros())
    assert s_same[0] == 0.0 and not np.signbit(s_same[0]) and s_same[1] == S.windows(shape, P)
    # twice the weight from a zero buffer: exactly twice the bits (a power of two commutes with both roundings)
    g1, s1 = _grad_call(o, t, P, 1, zeros(), weight=0.25)
    g2, s2 = _grad_call(o, t, P, 1, zeros(), weight=0.5)
    assert np.array_equal(_bits(g2), _bits(2.0 * g1)) and s1.tobytes() == s2.tobytes() and np.abs(g1).max() > 0
    # the mask without blank pixels is no mask
    dense = np.where(np.broadcast_to(S.valid_pixels(y), shape), y, np.float32(0.125)).astype(np.float32)
    assert S.valid_pixels(dense).all() and not S.valid_pixels(y).all()
    d = torch.from_numpy(dense).to(DEV)
    ga, sa = _grad_call(o, d, P, 1, zeros())
    gb, sb = _grad_call(o, d, P, 0, zeros())
    assert np.array_equal(_bits(ga), _bits(gb)) and sa.tobytes() == sb.tobytes()
    # two runs: the same bits
    gc, sc = _grad_call(o, d, P, 1, zeros())
    assert np.array_equal(_bits(ga), _bits(gc)) and sa.tobytes() == sc.tobytes()


FORMATS = {'fp32': dict(precision='fp32'), 'bf16x3': dict(precision='bf16x3'), 'mixed': dict(precision='fp32', mixed_precision='bf16')}
ID_BANDS, ID_D, ID_F, ID_SHAPE = (4, 6), 1, 128, (2, 16, 16)


@functools.lru_cache(maxsize=None)
def _step_case(bands, d, F, n, h, w, seed, scale=1.0):
    """(inputs, target with a blank rectangle, flat weights, min |ReLU input|): test_gpu_loss's construction, computed once.
    scale: the errors of test_gpu_train's target construction (|e| in 0.01 .. 0.06) times this."""
    flat = weights.random_he_uniform(sum(bands), bands[-1], d, F, seed=1, bias_scale=0.05)
    xs = T._inputs(bands, n, h, w, seed=seed)
    with torch.no_grad():
        pre = []
        out64 = T._forward64([torch.tensor(a, dtype=torch.float64) for a in xs], T._unflatten(flat.astype(np.float64), bands, d, F), d, pre)
    y = T._target(out64.numpy(), seed=3)
    if scale != 1.0:
        y = (out64.numpy() + scale * (y.astype(np.float64) - out64.numpy())).astype(np.float32)
    y[:, :, :h // 4, :w // 4] = 0.0
    return xs, y, flat, min(float(t.abs().min()) for t in pre)


@pytest.mark.parametrize('fmt', sorted(FORMATS))
def test_weight_zero_is_compile_today(fmt):
    kw = dict(FORMATS[fmt])
    m, _ = T._model(ID_BANDS, ID_D, ID_F, precision=kw.pop('precision'))
    n, h, w = ID_SHAPE
    xs, y, _, _ = _step_case(ID_BANDS, ID_D, ID_F, n, h, w, 2)
    xs_d, y_d = T._dev(xs), T._dev([y])[0]
    m.compile(mask_nodata=True, **kw)
    g_plain, l_plain = T._gradients(m, xs_d, y_d)
    m.compile(mask_nodata=True, ssim_weight=0.2, ssim_win=7, **kw)
    g_on, l_on = T._gradients(m, xs_d, y_d)
    assert not np.array_equal(_bits(g_on), _bits(g_plain)) and float(l_on[0]) > float(l_plain[0])
    assert np.array_equal(_bits(l_on[1:]), _bits(l_plain[1:]))                         # the MSE metric is untouched
    m.compile(mask_nodata=True, ssim_weight=0.0, ssim_win=7, **kw)
    assert m.loss_setting == losses.parse('mae', None, True)
    g_zero, l_zero = T._gradients(m, xs_d, y_d)
    assert np.array_equal(_bits(g_zero), _bits(g_plain)) and np.array_equal(_bits(l_zero), _bits(l_plain))


# ---- (d) the new sums against the metric's ------------------------------------------------------------------------------------------
def test_sums_against_dsen2_ssim_sums():
    """A band [h, w] through dsen2_ssim_loss_sums is windows - dsen2_ssim_sums of that plane WITHIN 1 ULP OF THE SUM OF q (not to
    the last bit of a restated subtraction order): the metric adds q in its own tiles of 16 x 32 windows and subtracts once, the
    term adds (1 - q) in tiles of 22 x 22; the two orders differ, and each sum of N terms is itself only good to a few ulp.  The
    bound is 1 ulp of the metric's sum (about N), which dwarfs the rounding of either order at these sizes."""
    shape, P = SHAPES[2]
    out, y, _ = _pair(shape, P)
    n, c, h, w = shape
    window = metrics.ssim_window(P, 1.5)
    o, t = torch.from_numpy(out.copy()).to(DEV), torch.from_numpy(y.copy()).to(DEV)
    for s in range(n):
        for b in range(c):
            po, pt = o[s:s + 1, b:b + 1].contiguous(), t[s:s + 1, b:b + 1].contiguous()
            work = torch.zeros(_sums_need(), dtype=torch.uint8, device=DEV)
            got = torch.zeros(3, dtype=torch.float64, device=DEV)
            with torch.cuda.device(DEV):
                _lib.call('dsen2_ssim_loss_sums', _ptr(po), _ptr(pt), 1, 1, h, w, _cwin(window), P, C1, C2, 0, _ptr(work), work.numel(),
                          _ptr(got), _stream_ptr(DEV))
            got = got.cpu().numpy()
            ref = metrics.ssim_sums_device(po.reshape(h, w, 1), pt.reshape(h, w, 1), L, win_size=P, sigma=1.5).cpu().numpy()
            assert got[1] == ref[0, 1] == got[2] == (h - P + 1) * (w - P + 1)
            print('plane (%d, %d): sum (1 - q) %r, windows - sum q %r' % (s, b, got[0], ref[0, 1] - ref[0, 0]))
            assert abs(got[0] - (ref[0, 1] - ref[0, 0])) <= np.spacing(ref[0, 0])


def test_one_window_is_one_minus_the_ssim_map():
    """q is formed as ssim_kernel forms it: an 11 x 11 plane has one window, and sum (1 - q) of it is 1 - dsen2_ssim_map bit for bit."""
    shape, P = SHAPES[0]
    out, y, _ = _pair(shape, P)
    o, t = torch.from_numpy(out.copy()).to(DEV), torch.from_numpy(y.copy()).to(DEV)
    _, s2 = _grad_call(o, t, P, 0, torch.zeros((121, 16), device=DEV))
    q = metrics.ssim_map_device(o.reshape(11, 11, 1), t.reshape(11, 11, 1), L, win_size=P, sigma=1.5).cpu().numpy()
    assert q.shape == (1, 1, 1) and 0 < q[0, 0, 0] < 1 and s2[0] == 1.0 - q[0, 0, 0]


# ---- (e) whole-step gradients against a float64 autograd ----------------------------------------------------------------------------
def _torch_total(out, y64, P, weight, mask):
    """MAE + weight * T of a float64 torch output against the float64 target, the masks applied by hand; (total, mse)."""
    n, c, h, w = out.shape
    g = metrics.ssim_window(P, 1.5)
    k = torch.tensor(np.outer(g, g))[None, None]
    t = torch.tensor(y64)
    valid = torch.tensor(np.broadcast_to(S.valid_pixels(y64) if mask else np.ones((n, 1, h, w), bool), out.shape).astype(np.float64))

    def f(v):
        return torch.nn.functional.conv2d(v.reshape(n * c, 1, h, w), k).reshape(n, c, h - P + 1, w - P + 1)
    mx, my, exx, eyy, exy = f(out), f(t), f(out * out), f(t * t), f(out * t)
    q = ((2 * mx * my + C1) * (2 * (exy - mx * my) + C2)) / ((mx * mx + my * my + C1) * ((exx - mx * mx) + (eyy - my * my) + C2))
    live = torch.tensor(np.broadcast_to(S.live_windows(y64, P, mask), q.shape).astype(np.float64))
    e = out - t
    total = (e.abs() * valid).sum() / e.numel() + weight * ((1 - q) * live).sum() / q.numel()
    return total, ((e * e) * valid).sum() / e.numel()


def _whole_step(m, case, P, tensor_gate, loss_gate, what, scale=1.0, **kw):
    bands, d, F = case[:3]
    xs, y, flat, _ = _step_case(*case, scale)
    for mask in (0, 1):
        ps = T._unflatten(flat.astype(np.float64), bands, d, F)
        out = T._forward64([torch.tensor(a, dtype=torch.float64) for a in xs], ps, d)
        total, mse = _torch_total(out, y.astype(np.float64), P, float(np.float32(WEIGHT)), mask)
        plain = float(_torch_total(out.detach(), y.astype(np.float64), P, 0.0, mask)[0])
        total.backward()
        g64 = [(p.grad.permute(2, 3, 1, 0) if i % 2 == 0 else p.grad).contiguous().numpy().ravel() for i, p in enumerate(ps)]
        m.compile(mask_nodata=bool(mask), ssim_weight=WEIGHT, ssim_win=P, **kw)
        grad, loss2 = T._gradients(m, T._dev(xs), T._dev([y])[0])
        parts = T._split(grad.cpu().numpy().astype(np.float64), bands, d, F)
        errs = [float(np.linalg.norm(a - ref) / np.linalg.norm(ref)) for a, ref in zip(parts, g64)]
        l2 = loss2.cpu().numpy().astype(np.float64)
        total, mse = float(total.detach()), float(mse.detach())
        print('%s mask %d %r: worst per-tensor rel. L2 error %.2e, loss %.4e (rel %.1e; the term is %.3f of it), mse rel %.1e'
              % (what, mask, case, max(errs), l2[0], abs(l2[0] - total) / total, (total - plain) / total, abs(l2[1] - mse) / mse))
        assert (total - plain) / total >= 0.05                      # the term carries weight in this case
        for i, err in enumerate(errs):
            assert err <= tensor_gate, (mask, i, err)
        assert abs(l2[0] - total) <= loss_gate * total and abs(l2[1] - mse) <= loss_gate * mse


@pytest.mark.parametrize('bands,d,F,n,h,w', T.CASES[:2])
def test_fp32_step_gradients_match_float64_autograd(bands, d, F, n, h, w):
    m, _ = T._model(bands, d, F)
    _whole_step(m, (bands, d, F, n, h, w, 2), 7, 1e-4, 1e-6, 'fp32 step')


def test_bf16x3_step_gradients_match_float64_autograd():
    """The bf16x3 step at the gates of tests/test_gpu_loss.py, on its case and for its reason: the term's dL/dout is a function of
    out - target like the MSE's, so the forward's own error (about 5e-6 per output) reaches it as (error of out) / |e| whatever the
    backward pass does, and a gate of 1e-4 says something about the backward pass only where |e| is well above 0.05: the errors of
    test_gpu_train's target construction times 10 (|e| in 0.1 .. 0.6)."""
    case = X.SAFE_CASES[0]
    margin = _step_case(*case)[3]
    assert margin >= X.MARGIN, 'input seed %d: a ReLU input lies %.2e from zero' % (case[6], margin)
    m, _ = X._model(*case[:3])
    _whole_step(m, case, 5, 1e-4, 1e-5, 'bf16x3 step', scale=10.0)      # 8 x 8: 4 x 4 windows of 5 x 5, 4 of them masked


# ---- (f) train_on_batch, fit -----------------------------------------------------------------------------------------------------------
def test_train_on_batch_one_shard_is_the_plain_step_and_follows_the_setting():
    bands, d, F = (4, 6), 1, 128
    xs, y, flat, _ = _step_case(bands, d, F, 2, 16, 16, 2)
    runs = []
    for kw in ({}, dict(shards=1)):
        m, _ = T._model(bands, d, F)
        m.compile(training.Nadam(lr=1e-3), mask_nodata=True, ssim_weight=WEIGHT, ssim_win=7)
        runs.append((m.train_on_batch(xs, y, **kw), m.get_weights_flat()))
    (la, wa), (lb, wb) = runs
    assert la == lb and wa.tobytes() == wb.tobytes() and not np.array_equal(wa, flat)
    ref, _ = T._model(bands, d, F)
    ref.compile(training.Nadam(lr=1e-3), mask_nodata=True, ssim_weight=WEIGHT, ssim_win=7)
    want = ref.evaluate(xs, y)                       # losses.host_loss of predict(): the total from the host statement
    assert la[0] == pytest.approx(want[0], rel=1e-6) and la[1] == pytest.approx(want[1], rel=1e-6)
    ref.compile(training.Nadam(lr=1e-3), mask_nodata=True)
    assert want[0] > ref.evaluate(xs, y)[0]


def test_fit_lowers_the_total_loss():
    bands, d, F = (4, 6), 1, 128
    teacher, tflat = T._model(bands, d, F, seed=3)
    xs = T._inputs(bands, 8, 16, 16, seed=14)
    y = teacher.predict(xs)
    student, _ = T._model(bands, d, F)
    student.set_weights_flat((tflat + np.random.default_rng(0).uniform(-0.15, 0.15, tflat.shape)).astype(np.float32))
    student.compile(training.Nadam(lr=1e-3), ssim_weight=WEIGHT, ssim_win=7)
    first = student.evaluate(xs, y)
    h = student.fit(xs, y, batch_size=8, epochs=6, verbose=0, validation_data=(xs, y), seed=5)
    last = student.evaluate(xs, y)
    print('fit with the SSIM term: total loss %.4e -> %.4e; epochs %r' % (first[0], last[0], h.history['loss']))
    assert h.history['loss'][0] == pytest.approx(first[0], rel=1e-5)
    assert last[0] < first[0] and h.history['loss'][-1] < h.history['loss'][0]
    assert h.history['val_loss'][-1] == last[0]


# ---- (g) fit_corpus: validation on the device = validation from host arrays ---------------------------------------------------------
def test_fit_corpus_validates_on_the_device_as_from_host_arrays():
    import test_gpu_loss as GL
    bands, d, F = (4, 6), 1, 128
    c = corpus.TileCorpus(GL._tiles_with_a_blank_corner(), device=DEV)
    table = c.validation_table(2, 17)
    arrays = c.validation_arrays(2, 17)
    v = S.valid_pixels(arrays[1])
    assert 0 < int(v.sum()) < v.size
    runs = []
    for how in ('device', 'host'):
        m = s2model(tuple((k, None, None) for k in bands), num_layers=d, feature_size=F, device=DEV)
        m.set_weights_flat(weights.random_he_uniform(sum(bands), bands[-1], d, F, seed=5, bias_scale=0.05))
        m.compile(training.Nadam(lr=1e-3), mask_nodata=True, ssim_weight=WEIGHT, ssim_win=7)
        assert m._validation_chunk(c) >= table.shape[0]                         # one chunk: one summation order on both sides
        kw = dict(validation_crops=table) if how == 'device' else dict(validation_data=arrays)
        h = m.fit_corpus(c, 4, 3, epochs=2, seed=17, augment=True, verbose=0, **kw)
        runs.append((m.get_weights_flat(), h.history))
    (wa, ha), (wb, hb) = runs
    print('val_loss device %r host %r' % (ha['val_loss'], hb['val_loss']))
    assert wa.tobytes() == wb.tobytes()
    assert ha['loss'] == hb['loss'] and ha['mean_squared_error'] == hb['mean_squared_error']
    assert np.asarray(ha['val_loss']).tobytes() == np.asarray(hb['val_loss']).tobytes()
    assert np.asarray(ha['val_mean_squared_error']).tobytes() == np.asarray(hb['val_mean_squared_error']).tobytes()
    # the term reached the validation loss
    m.compile(training.Nadam(lr=1e-3), mask_nodata=True)
    assert hb['val_loss'][1] > m.evaluate(*arrays)[0]


# ---- (h) two ranks = the one-process restatement -----------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def blank_corner_data(tmp_path_factory):
    """test_gpu_train_parallel's tiny set (7 training and 3 validation patches of 8 x 8), a corner of every target without data."""
    root = tmp_path_factory.mktemp('dp_ssim')
    rng = np.random.default_rng(41)
    train_dir = root / 'data' / 'train'
    for name, n in (('S2A_A.SAFE', 6), ('S2B_B.SAFE', 4)):
        d = train_dir / name
        os.makedirs(str(d))
        d20 = rng.uniform(0, 3000, (n, 6, 8, 8)).astype(np.float32)
        gt = (d20 + rng.uniform(-50, 50, d20.shape)).astype(np.float32)
        gt[:, :, :1, :1] = 0.0
        np.save(str(d / 'data10.npy'), rng.uniform(0, 3000, (n, 4, 8, 8)).astype(np.float32))
        np.save(str(d / 'data20.npy'), d20)
        np.save(str(d / 'data20_gt.npy'), gt)
    val = np.zeros(10, bool)
    val[[1, 4, 8]] = True
    np.save(str(train_dir / 'val_index.npy'), val)
    return root


def test_two_ranks_equal_the_one_process_restatement(blank_corner_data, capfd):
    extra = ('--ssim_weight', '0.2', '--ssim_win', '5', '--mask_nodata')
    ckpt, log = P._ranks_against_restatement(blank_corner_data, 2, extra)
    assert 'Loss: mae + 0.2 x (1 - SSIM), window 5, sigma 1.5, data range 5, no-data pixels masked.' in capfd.readouterr().out
    # the term reached the run: without it the same data gives another checkpoint
    from dsen2_amd import train
    out = blank_corner_data / 'one_without'
    assert train.main(P._train_args(blank_corner_data, out, ('--mask_nodata',)) + ['--emulate_world', '2']) == 0
    assert P._files(out)[0] != ckpt


# ---- (i) refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals_return_invalid_and_launch_nothing():
    lib = _lib.load()
    m, _ = T._model((4, 6), 1, 128)
    m.compile()
    win11, win7 = _cwin(metrics.ssim_window(11, 1.5)), _cwin(metrics.ssim_window(7, 1.5))
    with torch.cuda.device(DEV):
        assert lib.dsen2_model_set_loss_ssim(m._handle, 0.2, win7, 7, C1, C2) == _lib.OK
        for args, text in (((-0.5, win11, 11, C1, C2), b'weight'), ((float('nan'), win11, 11, C1, C2), b'weight'),
                           ((0.2, win11, 10, C1, C2), b'window size'), ((0.2, win11, 13, C1, C2), b'window size'),
                           ((0.2, _cwin([0.5, float('inf'), 0.5]), 3, C1, C2), b'not finite'), ((0.2, win11, 11, 0.0, C2), b'constants'),
                           ((0.2, win11, 11, C1, float('nan')), b'constants')):
            assert lib.dsen2_model_set_loss_ssim(m._handle, *args) == _lib.ERR_INVALID
            assert text in lib.dsen2_last_error()
        bf, _ = T._model((4, 6), 1, 128, precision='bf16')
        assert lib.dsen2_model_set_loss_ssim(bf._handle, 0.2, win11, 11, C1, C2) == _lib.ERR_INVALID
        assert b'fp32' in lib.dsen2_last_error()
    # nothing changed: the handle still holds (0.2, window 7), so a 6 x 6 patch is refused and an 8 x 8 one is not
    n, h, w = 1, 6, 6
    xs_d = T._dev(T._inputs((4, 6), n, h, w, seed=1))
    y_d = torch.full((n, 6, h, w), 0.25, device=DEV)
    grad = torch.full((m.count_params(),), -7.0, device=DEV)
    loss2 = torch.full((2,), -7.0, device=DEV)
    ws = torch.zeros(m.train_workspace_bytes(n, h, w), dtype=torch.uint8, device=DEV)
    with torch.cuda.device(DEV):
        rc = lib.dsen2_model_gradients(m._handle, _ptr(xs_d[0]), _ptr(xs_d[1]), None, _ptr(y_d), None, _ptr(grad), _ptr(loss2), n, h, w,
                                       _ptr(ws), ws.numel(), _stream_ptr(DEV))
    assert rc == _lib.ERR_INVALID and b'smaller than' in lib.dsen2_last_error()
    torch.cuda.synchronize()
    assert (grad.cpu().numpy() == -7.0).all() and (loss2.cpu().numpy() == -7.0).all() and not ws.any()
    with pytest.raises(Exception, match='smaller than'):
        m.train_on_batch(T._inputs((4, 6), 1, 6, 6, seed=1), np.full((1, 6, 6, 6), 0.25, np.float32))
    xs8 = T._inputs((4, 6), 1, 8, 8, seed=1)
    assert np.isfinite(m.train_on_batch(xs8, np.full((1, 6, 8, 8), 0.25, np.float32))).all()
    # the kernel entry: h < win
    o = torch.zeros((1, 1, 10, 12), device=DEV)
    g = torch.full((120, 16), -7.0, device=DEV)
    s2 = torch.full((2,), -7.0, dtype=torch.float64, device=DEV)
    with torch.cuda.device(DEV):
        assert lib.dsen2_ssim_loss_grad(_ptr(o), _ptr(o), 1, 1, 10, 12, 0.2, win11, 11, C1, C2, 0, _ptr(g), _ptr(s2), _stream_ptr(DEV)) == _lib.ERR_INVALID
    torch.cuda.synchronize()
    assert (g.cpu().numpy() == -7.0).all() and (s2.cpu().numpy() == -7.0).all()
