"""Losses and the no-data mask on the GPU (include/dsen2_hip.h, "losses and the no-data mask"): dsen2_loss_grad and dsen2_loss_sums
bit for bit against the float64 restatement (tests/loss_restatement.py) inside guard bands; whole-step gradients against a
float64 torch autograd of the same graph with each loss, masked and unmasked; identities between the losses that need no gate,
in all three step formats; train_on_batch, fit and learning per kind; fit_corpus validating on the device against host arrays;
and two gloo ranks against the one-process restatement."""
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

import loss_restatement as R  # noqa: E402
import test_gpu_train as T  # noqa: E402            (the graph, the cases and the target construction of the fp32 step's tests)
import test_gpu_train_bf16x3 as X  # noqa: E402     (the margin and a safe case of the bf16x3 step's tests)
import test_gpu_train_parallel as P  # noqa: E402   (ranks against the one-process restatement)
from guarded import run_three_ways  # noqa: E402

from dsen2_amd import _lib, corpus, training, weights  # noqa: E402
from dsen2_amd.DSen2Net import _ptr, _stream_ptr, s2model  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)

DELTA, EPS = 0.03, 0.01
PARAM = {R.MAE: 0.0, R.MSE: 0.0, R.HUBER: DELTA, R.CHARBONNIER: EPS}
NAME = {R.MAE: 'mae', R.MSE: 'mse', R.HUBER: 'huber', R.CHARBONNIER: 'charbonnier'}
# (n, c, h, w): the smallest; ragged, less than one block; ragged; the widest cout; 269 120 pixels > 1024 blocks x 256 threads, so
# the grid-stride loop of the step's kernel takes a second pass
SHAPES = [(1, 1, 1, 1), (3, 6, 5, 7), (2, 2, 9, 21), (2, 15, 4, 4), (5, 6, 232, 232)]
# dsen2_loss_sums alone: 8 392 609 elements > 4096 blocks x 2048, the cap of its grid, so every thread takes a ninth pass
ABOVE_THE_SUMS_GRID_CAP = (1, 1, 2897, 2897)


def _compile(m, kind, mask=0, scale=1.0, **kw):
    extra = dict(loss_param=scale * PARAM[kind]) if kind in (R.HUBER, R.CHARBONNIER) else {}
    m.compile(kw.pop('optimizer', 'nadam'), loss=NAME[kind], mask_nodata=bool(mask), **extra, **kw)
    return m


@functools.lru_cache(maxsize=None)
def _pair(shape):
    """(out, y) float32 NCHW, computed once and never modified: |e| in 0.01 .. 0.06 (test_gpu_train's _target construction), and
    in y a rectangle of all-zero pixels, a pixel that is zero in every band but the last and one that is zero in every band but the
    first (both valid), a -0.0 pixel (masked), a negative pixel (valid), and every 7th element equal to out (e == 0 exactly).  The one-pixel shape holds an all-zero target."""
    n, c, h, w = shape
    rng = np.random.default_rng(n * 1000 + c * 100 + h)
    out = rng.uniform(0.1, 0.5, shape).astype(np.float32)
    y = T._target(out.astype(np.float64), seed=3)
    y.ravel()[::7] = out.ravel()[::7]
    if h * w == 1:
        y[...] = 0.0
    else:
        assert h >= 4 and w >= 4
        y[:, :, :max(1, h // 3), :max(1, w // 3)] = 0.0
        y[n - 1, :c - 1, h - 1, w - 1] = 0.0
        y[n - 1, 1:, h - 2, w - 1] = 0.0
        y[n - 1, c - 1, h - 1, w - 1] = y[n - 1, 0, h - 2, w - 1] = 0.375
        y[0, :, h - 1, 0] = -0.0
        y[0, :, h - 1, w // 2] = -0.25
    out.setflags(write=False)
    y.setflags(write=False)
    return out, y


def _check_pair(shape):
    """What the data must hold for the cases to bite, asserted from the float64 side alone."""
    out, y = _pair(shape)
    n, c, h, w = shape
    v = R.valid(y, 1)
    d = (out - y).astype(np.float64)
    if h * w == 1:
        assert not v.any()
        return
    assert 0 < int(v.sum()) < v.size and not v[:, :, :max(1, h // 3), :max(1, w // 3)].any()
    assert not v[0, 0, h - 1, 0] and np.signbit(y[0, :, h - 1, 0]).all()                 # -0.0: masked
    assert v[0, 0, h - 1, w // 2] and (y[0, :, h - 1, w // 2] < 0).all()                   # negative: data
    assert v[n - 1, 0, h - 1, w - 1] and v[n - 1, 0, h - 2, w - 1]                          # one band with data: valid
    assert c == 1 or (not y[n - 1, :c - 1, h - 1, w - 1].any() and not y[n - 1, 1:, h - 2, w - 1].any())
    assert (d == 0).sum() >= 1 and not np.isnan(y).any()
    a, delta = np.abs(d), float(np.float32(DELTA))
    assert (a <= delta).mean() >= 0.25 and (a > delta).mean() >= 0.25                      # both Huber branches, a quarter each


# ---- (a) dsen2_loss_grad ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', R.KINDS)
@pytest.mark.parametrize('shape', SHAPES)
def test_loss_grad_equals_the_restatement_bit_for_bit(shape, kind):
    _check_pair(shape)
    out, y = _pair(shape)
    n, c, h, w = shape
    inp = [torch.from_numpy(out.copy()).to(DEV), torch.from_numpy(y.copy()).to(DEV)]
    for mask in (0, 1):
        def call(i, o, _inplace, _scratch):
            with torch.cuda.device(DEV):
                _lib.call('dsen2_loss_grad', _ptr(i[0]), _ptr(i[1]), n, c, h, w, kind, PARAM[kind], mask, _ptr(o[0]), _ptr(o[1]),
                          _stream_ptr(DEV))
        (g, loss2), _ = run_three_ways(call, inp, [((n * h * w, 16), torch.float32), ((2,), torch.float32)], device=DEV,
                                       what='loss_grad %r %s mask %d' % (shape, NAME[kind], mask))
        want_g, want_l = R.loss_grad(out, y, kind, PARAM[kind], mask)
        g, loss2 = g.cpu().numpy(), loss2.cpu().numpy().astype(np.float64)
        bad = (g.view(np.uint32) != want_g.view(np.uint32))
        print('loss_grad %r %s mask %d: %d of %d lanes differ; loss2 %r, float64 %r' % (shape, NAME[kind], mask, int(bad.sum()), bad.size,
                                                                                      loss2.tolist(), want_l))
        assert not bad.any(), np.argwhere(bad)[:8]
        assert not g[:, c:].any()
        if mask:
            masked = ~np.broadcast_to(R.valid(y, 1), (n, c, h, w)).transpose(0, 2, 3, 1).reshape(n * h * w, c)
            assert masked.any() and not g[:, :c][masked].any()
        for got, ref in zip(loss2, want_l):
            assert abs(got - ref) <= 1e-6 * ref
        if kind == R.MSE:
            assert loss2[0] == loss2[1]


# ---- (b) dsen2_loss_sums ------------------------------------------------------------------------------------------------------------
def _sums_need():
    need = ctypes.c_size_t(0)
    _lib.call('dsen2_loss_sums_workspace_bytes', ctypes.byref(need))
    return int(need.value)


@pytest.mark.parametrize('kind', R.KINDS)
@pytest.mark.parametrize('shape', SHAPES + [ABOVE_THE_SUMS_GRID_CAP])
def test_loss_sums_equal_the_restatement_bit_for_bit(shape, kind):
    out, y = _pair(shape)
    n, c, h, w = shape
    inp = [torch.from_numpy(out.copy()).to(DEV), torch.from_numpy(y.copy()).to(DEV)]
    need = _sums_need()
    for mask in (0, 1):
        def call(i, o, _inplace, scratch):
            with torch.cuda.device(DEV):
                _lib.call('dsen2_loss_sums', _ptr(i[0]), _ptr(i[1]), n, c, h * w, kind, PARAM[kind], mask, _ptr(scratch[0]),
                          scratch[0].numel(), _ptr(o[0]), _stream_ptr(DEV))
        (got,), _ = run_three_ways(call, inp, [((3,), torch.float64)], scratch=[need], device=DEV,
                                   what='loss_sums %r %s mask %d' % (shape, NAME[kind], mask))
        got = got.cpu().numpy()
        want = R.loss_sums(out, y, kind, PARAM[kind], mask)
        print('loss_sums %r %s mask %d: kernel %r restatement %r' % (shape, NAME[kind], mask, got.tolist(), want.tolist()))
        assert got.tobytes() == want.tobytes()
        assert got[2] == float(np.broadcast_to(R.valid(y, mask), out.shape).sum())
        if kind == R.MAE and not mask:
            pair = torch.zeros(2, dtype=torch.float64, device=DEV)
            work = torch.zeros(need, dtype=torch.uint8, device=DEV)
            with torch.cuda.device(DEV):
                _lib.call('dsen2_abs_sq_error_sums', _ptr(inp[0]), _ptr(inp[1]), out.size, _ptr(work), work.numel(), _ptr(pair),
                          _stream_ptr(DEV))
            assert pair.cpu().numpy().tobytes() == got[:2].tobytes()


def test_loss_sums_refusals_and_the_wrapper():
    lib = _lib.load()
    out, y = _pair(SHAPES[1])
    n, c, h, w = SHAPES[1]
    p, t = torch.from_numpy(out.copy()).to(DEV), torch.from_numpy(y.copy()).to(DEV)
    need = _sums_need()
    work = torch.zeros(need, dtype=torch.uint8, device=DEV)
    out3 = torch.full((3,), -1.0, dtype=torch.float64, device=DEV)
    with torch.cuda.device(DEV):
        for args, code, text in (((n, c, h * w, 4, 0.0, 0, _ptr(work), need), _lib.ERR_INVALID, b'kind 4'),
                                 ((n, c, h * w, 2, 0.0, 0, _ptr(work), need), _lib.ERR_INVALID, b'parameter'),
                                 ((n, c, h * w, 0, 0.0, 3, _ptr(work), need), _lib.ERR_INVALID, b'mask mode 3'),
                                 ((n, c, 0, 0, 0.0, 0, _ptr(work), need), _lib.ERR_INVALID, b'bad shape'),
                                 ((n, c, h * w, 1, 0.0, 1, _ptr(work), need - 8), _lib.ERR_WORKSPACE, b'workspace'),
                                 ((n, c, h * w, 1, 0.0, 1, None, need), _lib.ERR_INVALID, b'NULL')):
            assert lib.dsen2_loss_sums(_ptr(p), _ptr(t), *args, _ptr(out3), _stream_ptr(DEV)) == code
            assert text in lib.dsen2_last_error()
    torch.cuda.synchronize()
    assert (out3.cpu().numpy() == -1.0).all()                                      # a refused call writes nothing
    # S2Model.loss_sums_device: the compiled loss's first two sums; the default setting is abs_sq_error_sums_device
    m, _ = T._model((4, 6), 1, 128)
    for kind, mask in ((R.HUBER, 1), (R.MAE, 0)):
        _compile(m, kind, mask)
        got = m.loss_sums_device(p, t, torch.empty(2, dtype=torch.float64, device=DEV)).cpu().numpy()
        assert got.tobytes() == R.loss_sums(out, y, kind, PARAM[kind], mask)[:2].tobytes()


# ---- (c) whole-step gradients against a float64 autograd ---------------------------------------------------------------------------
def _torch_rho(e, kind, scale=1.0):
    zero, F = torch.zeros_like(e), torch.nn.functional
    if kind == R.MAE:
        return F.l1_loss(e, zero, reduction='none')
    if kind == R.MSE:
        return F.mse_loss(e, zero, reduction='none')
    if kind == R.HUBER:
        return F.huber_loss(e, zero, reduction='none', delta=float(np.float32(scale * DELTA)))
    return torch.sqrt(e * e + float(np.float32(scale * EPS)) ** 2)


def _grads64(xs, y, flat, bands, d, F, kind, mask, scale=1.0):
    """(gradients per tensor, loss, mse) of the float64 graph with the loss `kind`; the mask applied by hand, the mean over ALL elements."""
    ps = T._unflatten(flat.astype(np.float64), bands, d, F)
    out = T._forward64([torch.tensor(a, dtype=torch.float64) for a in xs], ps, d)
    e = out - torch.tensor(y, dtype=torch.float64)
    v = torch.tensor(np.broadcast_to(R.valid(y, mask), y.shape).astype(np.float64))
    loss = (_torch_rho(e, kind, scale) * v).sum() / e.numel()
    loss.backward()
    grads = [(p.grad.permute(2, 3, 1, 0) if i % 2 == 0 else p.grad).contiguous().numpy().ravel() for i, p in enumerate(ps)]
    return grads, float(loss.detach()), float(((e * e) * v).sum().detach() / e.numel())


@functools.lru_cache(maxsize=None)
def _step_case(bands, d, F, n, h, w, seed, scale=1.0):
    """(inputs, target with a blank rectangle and a pixel blank in every band but the last, flat weights, min |ReLU input|) of a whole-step
    case: computed once.  scale: the errors of test_gpu_train's target construction (|e| in 0.01 .. 0.06) times this."""
    flat = weights.random_he_uniform(sum(bands), bands[-1], d, F, seed=1, bias_scale=0.05)
    xs = T._inputs(bands, n, h, w, seed=seed)
    with torch.no_grad():
        pre = []
        out64 = T._forward64([torch.tensor(a, dtype=torch.float64) for a in xs], T._unflatten(flat.astype(np.float64), bands, d, F), d, pre)
    y = T._target(out64.numpy(), seed=3)
    if scale != 1.0:
        y = (out64.numpy() + scale * (y.astype(np.float64) - out64.numpy())).astype(np.float32)
    y[:, :, :h // 3, :w // 2] = 0.0
    y[0, :-1, h - 1, w - 1] = 0.0                   # data in the last band alone: valid
    v = R.valid(y, 1)
    assert 0 < int(v.sum()) < v.size and v[0, 0, h - 1, w - 1] and y[0, -1, h - 1, w - 1] != 0
    return xs, y, flat, min(float(t.abs().min()) for t in pre)


def _out64(case):
    bands, d, F = case[:3]
    xs, _, flat, _ = _step_case(*case)
    with torch.no_grad():
        return T._forward64([torch.tensor(a, dtype=torch.float64) for a in xs], T._unflatten(flat.astype(np.float64), bands, d, F), d).numpy()


def _whole_step(m, case, kind, tensor_gate, loss_gate, what, scale=1.0):
    bands, d, F = case[:3]
    xs, y, flat, _ = _step_case(*case, scale)
    if kind == R.HUBER:         # both branches, a quarter of the elements each, by the float64 side alone
        a = np.abs(_out64(case) - y.astype(np.float64))
        assert (a <= scale * DELTA).mean() >= 0.25 and (a > scale * DELTA).mean() >= 0.25
    for mask in (0, 1):
        g64, loss64, mse64 = _grads64(xs, y, flat, bands, d, F, kind, mask, scale)
        _compile(m, kind, mask, scale)
        grad, loss2 = T._gradients(m, T._dev(xs), T._dev([y])[0])
        parts = T._split(grad.cpu().numpy().astype(np.float64), bands, d, F)
        errs = [float(np.linalg.norm(g - ref) / np.linalg.norm(ref)) for g, ref in zip(parts, g64)]
        l2 = loss2.cpu().numpy().astype(np.float64)
        print('%s %s mask %d %r: worst per-tensor rel. L2 error %.2e, loss %.4e (rel %.1e), mse rel %.1e'
              % (what, NAME[kind], mask, case, max(errs), l2[0], abs(l2[0] - loss64) / loss64, abs(l2[1] - mse64) / mse64))
        for i, err in enumerate(errs):
            assert err <= tensor_gate, (mask, i, err)
        assert abs(l2[0] - loss64) <= loss_gate * loss64 and abs(l2[1] - mse64) <= loss_gate * mse64


@pytest.mark.parametrize('kind', R.KINDS)
@pytest.mark.parametrize('bands,d,F,n,h,w', T.CASES[:2])
def test_fp32_step_gradients_match_float64_autograd(bands, d, F, n, h, w, kind):
    assert T.CASES[:2] == [((4, 6), 2, 128, 2, 16, 16), ((4, 6, 2), 1, 128, 2, 16, 16)]
    m, _ = T._model(bands, d, F)
    _whole_step(m, (bands, d, F, n, h, w, 2), kind, 1e-4, 1e-6, 'fp32 step')


BF16X3_CASE = X.SAFE_CASES[0]          # ((4, 6), 1, 128, 1, 8, 8, seed): an input seed found on the CPU from the float64 forward
BF16X3_ERROR_SCALE = 10.0


@pytest.mark.parametrize('kind', R.KINDS)
def test_bf16x3_step_gradients_match_float64_autograd(kind):
    """The bf16x3 step at the gates of tests/test_gpu_train_bf16x3.py (1e-4 per tensor, 1e-5 on the losses), on one of that
    file's cases whose ReLU masks cannot flip.
    The size of the errors is chosen for the kinds whose dL/dout is proportional to e = out - y (MSE, Huber below delta,
    Charbonnier near epsilon): the forward's own error reaches such a gradient as (error of out) / |e|, whatever the backward
    pass does.  A bf16x3 forward is good to about 5e-6 per output (MARGIN above is ten times that), so a gate of
    1e-4 on the gradient says something about the backward pass only where |e| is well above 5e-6 / 1e-4 = 0.05.  The case
    therefore takes test_gpu_train's target construction with its errors times 10 (|e| in 0.1 .. 0.6) and delta = 0.3, epsilon
    = 0.1, which puts the same shares of the elements on each branch.  At the unscaled construction (|e| in 0.01 .. 0.06) the
    masked MSE gradient of this case is 1.3e-4 from the float64 one in its worst tensor (Huber 1.0e-4): the forward's error
    over |e|, as profiles/train_losses.md records.  The MAE's gradient does not depend on |e| and passes at either scale."""
    margin = _step_case(*BF16X3_CASE)[3]
    assert margin >= X.MARGIN, 'input seed %d: a ReLU input lies %.2e from zero' % (BF16X3_CASE[6], margin)
    m, _ = X._model(*BF16X3_CASE[:3])
    _whole_step(m, BF16X3_CASE, kind, 1e-4, 1e-5, 'bf16x3 step', scale=BF16X3_ERROR_SCALE)


# ---- (d) identities that need no gate, in every step format ---------------------------------------------------------------------------
FORMATS = {'fp32': dict(precision='fp32'), 'bf16x3': dict(precision='bf16x3'), 'mixed': dict(precision='fp32', mixed_precision='bf16')}
ID_BANDS, ID_D, ID_F, ID_SHAPE = (4, 6), 1, 128, (2, 16, 16)


def _bits(t):
    return t.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize('fmt', sorted(FORMATS))
def test_identities_between_the_losses(fmt):
    kw = dict(FORMATS[fmt])
    m, flat = T._model(ID_BANDS, ID_D, ID_F, precision=kw.pop('precision'))
    n, h, w = ID_SHAPE
    xs, y, _, _ = _step_case(ID_BANDS, ID_D, ID_F, n, h, w, 2)          # y has blank pixels
    xs_d = T._dev(xs)

    def run(kind, target, mask=0, param=None, default=False):
        if default:
            m.compile(**kw)
        elif param is not None:
            m.compile(loss=NAME[kind], loss_param=param, mask_nodata=bool(mask), **kw)
        else:
            _compile(m, kind, mask, **kw)
        out = torch.empty((n, ID_BANDS[-1], h, w), dtype=torch.float32, device=DEV)
        grad, loss2 = T._gradients(m, xs_d, T._dev([target])[0], out=out)
        return grad, loss2, out.cpu().numpy()

    g_mae, l_mae, out = run(R.MAE, y)
    assert float(g_mae.abs().max()) > 0
    # MSE = 2 x Huber(1024): rho' = 2d against d, and a power of two commutes with every rounding of the linear backward pass
    g_mse, _, _ = run(R.MSE, y)
    g_hub, _, _ = run(R.HUBER, y, param=1024.0)
    assert np.array_equal(_bits(g_mse), _bits(2.0 * g_hub)), int((_bits(g_mse) != _bits(2.0 * g_hub)).sum())
    # Huber(2^-10) below every |e| = 2^-10 x MAE (on a target that is 0.02 away from the step's own output where y is blank:
    # the output itself comes arbitrarily close to 0)
    masked = np.broadcast_to(~R.valid(y, 1), y.shape)
    y_far = np.where(masked, out + np.float32(0.02), y).astype(np.float32)
    assert np.abs(out - y_far).min() > 2.0 ** -10
    g_far, _, _ = run(R.MAE, y_far)
    g_small, _, _ = run(R.HUBER, y_far, param=2.0 ** -10)
    assert np.array_equal(_bits(g_small), _bits(2.0 ** -10 * g_far)), int((_bits(g_small) != _bits(2.0 ** -10 * g_far)).sum())
    y_filled = np.where(masked, out, y).astype(np.float32)                  # e == 0 where there is no ground truth
    y_dense = np.where(masked, np.float32(0.125), y).astype(np.float32)     # no all-zero pixel
    assert masked.any() and R.valid(y_dense, 1).all()
    for kind in R.KINDS:
        # the mask = an error of exactly zero there: every rho'(0) is 0
        g_on, _, out_on = run(kind, y, mask=1)
        g_off, _, _ = run(kind, y_filled, mask=0)
        assert np.array_equal(out_on, out)
        assert np.array_equal(_bits(g_on), _bits(g_off)), (NAME[kind], int((_bits(g_on) != _bits(g_off)).sum()))
        assert not np.array_equal(_bits(g_on), _bits(run(kind, y, mask=0)[0]))          # and it is not a no-op on this target
        # nothing to mask: the mask changes no bit
        g1, l1, _ = run(kind, y_dense, mask=1)
        g0, l0, _ = run(kind, y_dense, mask=0)
        assert np.array_equal(_bits(g1), _bits(g0)) and np.array_equal(_bits(l1), _bits(l0)), NAME[kind]
    # compile() is compile(loss='mae')
    g_def, l_def, _ = run(R.MAE, y, default=True)
    assert np.array_equal(_bits(g_def), _bits(g_mae)) and np.array_equal(_bits(l_def), _bits(l_mae))


# ---- (e) train_on_batch, fit, learning -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', R.KINDS)
def test_train_on_batch_takes_the_nadam_step_of_that_loss(kind):
    bands, d, F = (4, 6), 1, 128
    xs, y, flat, _ = _step_case(bands, d, F, 2, 16, 16, 2)
    a, _ = T._model(bands, d, F)
    b, _ = T._model(bands, d, F)
    _compile(a, kind, 1, optimizer=training.Nadam(lr=1e-3))
    _compile(b, kind, 1, optimizer=training.Nadam(lr=1e-3))
    la = a.train_on_batch(xs, y)
    grad, loss2 = T._gradients(b, T._dev(xs), T._dev([y])[0])
    count = b.count_params()
    pb, mb, vb = torch.from_numpy(flat.copy()).to(DEV), torch.zeros(count, device=DEV), torch.zeros(count, device=DEV)
    s = training.Nadam(lr=1e-3).next_step()
    with torch.cuda.device(DEV):
        _lib.call('dsen2_nadam_step', _ptr(pb), _ptr(grad), _ptr(mb), _ptr(vb), count, s['lr'], s['b1'], s['b2'], s['eps'], s['mc_t'],
                  s['mc_t1'], s['ms_new'], s['ms_next'], s['b2_pow_t'], _stream_ptr(DEV))
    assert la == [float(v) for v in loss2.cpu().numpy()]
    got = a.get_weights_flat()
    assert got.tobytes() == pb.cpu().numpy().tobytes() and not np.array_equal(got, flat)
    want = R.loss_grad(b.predict(xs), y, kind, PARAM[kind], 1)[1]             # b still holds the weights the step started from
    assert la[0] == pytest.approx(want[0], rel=1e-6) and la[1] == pytest.approx(want[1], rel=1e-6)


def test_fit_with_mse_logs_the_loss_as_the_metric():
    bands, d, F = (4, 6), 1, 128
    xs, y, _, _ = _step_case(bands, d, F, 2, 16, 16, 2)
    xs6, y6 = [np.concatenate([a, a[::-1], a]) for a in xs], np.concatenate([y, y[::-1], y])
    for mask in (0, 1):
        m, _ = T._model(bands, d, F)
        _compile(m, R.MSE, mask, optimizer=training.Nadam(lr=1e-3))
        h = m.fit(xs6, y6, batch_size=4, epochs=2, verbose=0, validation_data=(xs, y), seed=5)
        assert len(h.history['loss']) == 2 and h.history['loss'] == h.history['mean_squared_error']
        assert h.history['val_loss'] == h.history['val_mean_squared_error']
        assert h.history['loss'][1] != h.history['loss'][0]
        assert m.evaluate(xs, y)[0] == h.history['val_loss'][1]


@pytest.mark.parametrize('kind', R.KINDS)
def test_thirty_steps_halve_the_loss(kind):
    bands, d, F = (4, 6), 1, 128
    teacher, tflat = T._model(bands, d, F, seed=3)
    xs = T._inputs(bands, 8, 16, 16, seed=14)
    y = teacher.predict(xs)
    student, _ = T._model(bands, d, F)
    student.set_weights_flat((tflat + np.random.default_rng(0).uniform(-0.15, 0.15, tflat.shape)).astype(np.float32))
    _compile(student, kind, 0, optimizer=training.Nadam(lr=1e-3))
    first = student.evaluate(xs, y)
    losses = [student.train_on_batch(xs, y)[0] for _ in range(30)]
    last = student.evaluate(xs, y)
    print('learning %s: loss %.4e -> %.4e (%.3f of the start)' % (NAME[kind], first[0], last[0], last[0] / first[0]))
    assert losses[0] == pytest.approx(first[0], rel=1e-5)
    assert last[0] < 0.5 * first[0]


# ---- (f) fit_corpus: validation on the device = validation from host arrays -----------------------------------------------------------
def _tiles_with_a_blank_corner():
    """Two 20 m tiles (grids 24 x 40 uint16 and 33 x 17 float32, as the corpus tests use) whose top-left part is fill: 0 in every
    band of both rasters."""
    rng = np.random.default_rng(1)
    tiles = []
    for (gh, gw), dtype, (bh, bw) in (((24, 40), np.uint16, (12, 20)), ((33, 17), np.float32, (20, 17))):
        t = [rng.integers(200, 12000, (gh * f, gw * f, c)).astype(dtype) for f, c in ((4, 4), (2, 6))]
        t[0][:bh * 4, :bw * 4, :] = 0
        t[1][:bh * 2, :bw * 2, :] = 0
        tiles.append(tuple(t))
    return tiles


def test_fit_corpus_validates_on_the_device_as_from_host_arrays():
    bands, d, F = (4, 6), 1, 128
    c = corpus.TileCorpus(_tiles_with_a_blank_corner(), device=DEV)
    table = c.validation_table(2, 17)
    arrays = c.validation_arrays(2, 17)
    v = R.valid(arrays[1], 1)
    assert 0 < int(v.sum()) < v.size                                            # blank and valid pixels among the validation crops
    runs = []
    for how in ('device', 'host'):
        m = s2model(tuple((k, None, None) for k in bands), num_layers=d, feature_size=F, device=DEV)
        m.set_weights_flat(weights.random_he_uniform(sum(bands), bands[-1], d, F, seed=5, bias_scale=0.05))
        m.compile(training.Nadam(lr=1e-3), loss='huber', loss_param=DELTA, mask_nodata=True)
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
    assert len(ha['val_loss']) == 2 and ha['val_loss'][0] != ha['val_loss'][1]
    # and the mask is not a no-op on these crops
    pred = m.predict(arrays[0])
    sums_on, sums_off = R.loss_sums(pred, arrays[1], R.HUBER, DELTA, 1), R.loss_sums(pred, arrays[1], R.HUBER, DELTA, 0)
    assert sums_on[0] < sums_off[0] and hb['val_loss'][1] == sums_on[0] / pred.size


# ---- (g) two ranks = the one-process restatement -----------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def blank_corner_data(tmp_path_factory):
    """test_gpu_train_parallel's tiny set (7 training and 3 validation patches of 8 x 8), a corner of every target without data."""
    root = tmp_path_factory.mktemp('dp_loss')
    rng = np.random.default_rng(41)
    train_dir = root / 'data' / 'train'
    for name, n in (('S2A_A.SAFE', 6), ('S2B_B.SAFE', 4)):
        d = train_dir / name
        os.makedirs(str(d))
        d20 = rng.uniform(0, 3000, (n, 6, 8, 8)).astype(np.float32)
        gt = (d20 + rng.uniform(-50, 50, d20.shape)).astype(np.float32)
        gt[:, :, :3, :4] = 0.0
        np.save(str(d / 'data10.npy'), rng.uniform(0, 3000, (n, 4, 8, 8)).astype(np.float32))
        np.save(str(d / 'data20.npy'), d20)
        np.save(str(d / 'data20_gt.npy'), gt)
    val = np.zeros(10, bool)
    val[[1, 4, 8]] = True
    np.save(str(train_dir / 'val_index.npy'), val)
    return root


def test_two_ranks_equal_the_one_process_restatement(blank_corner_data, capfd):
    extra = ('--loss', 'charbonnier', '--loss_param', '0.01', '--mask_nodata')
    ckpt, log = P._ranks_against_restatement(blank_corner_data, 2, extra)
    assert 'Loss: charbonnier(0.01), no-data pixels masked.' in capfd.readouterr().out
    # the mask reached the run: without it the same data gives another checkpoint
    from dsen2_amd import train
    out = blank_corner_data / 'one_unmasked'
    assert train.main(P._train_args(blank_corner_data, out, extra[:4]) + ['--emulate_world', '2']) == 0
    assert P._files(out)[0] != ckpt
