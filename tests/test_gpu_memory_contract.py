"""The memory contract of the C ABI ("memory contract"), entry point by entry point: guard bands around every device
tensor and poisoned outputs and scratch (tests/guarded.py: run_three_ways).

The parity tests compare what a call wrote with a reference.  These rows check what they cannot see: that nothing is written
outside the caller's buffers (the convolution kernels mask by pushing an offset out of range of a per-image buffer descriptor:
a descriptor one plane, slab or image too long strays only behind the LAST image), that the result does not depend on what
the workspace held on entry, that nothing outside the input tensors feeds the arithmetic, and that every output element is
written.  Every comparison is on bits; there is no tolerance in this file.  Shapes are the smallest at which the addressing can
still go wrong: 1 x 1, ragged images narrower and wider than a tile, more than one image.  Scratch is passed with exactly the
byte count of the library's own size function, so a size function that is too small shows as a changed tail guard."""
import ctypes
import functools
import os
import re
import sys
from math import ceil

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from dsen2_amd import _lib, training, weights  # noqa: E402
from dsen2_amd import imresize as ir  # noqa: E402
from dsen2_amd import metrics, patches as gp  # noqa: E402
from dsen2_amd.DSen2Net import _ptr, _stream_ptr, s2model, split3_f32, split_f32  # noqa: E402
from guarded import run_three_ways  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda', 0)
NULL = ctypes.c_void_p(0)
I16, F32, F64 = torch.int16, torch.float32, torch.float64


def _rng(*key):
    return np.random.default_rng([abs(int(k)) for k in key])


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _run(what, call, inputs, outputs, inplace=(), scratch=()):
    def on_device(*tensors):
        with torch.cuda.device(DEV):
            call(*tensors)
    return run_three_ways(on_device, inputs, outputs, inplace, scratch, device=DEV, what=what)


def _lib_call(name, *args):
    _lib.call(name, *(args + (_stream_ptr(DEV),)))


def _size(name, *args):
    out = ctypes.c_size_t(0)
    _lib.call(name, *(args + (ctypes.byref(out),)))
    return out.value


def _host(a):
    a = np.ascontiguousarray(a, np.float32)
    return a, a.ctypes.data_as(_lib.c_float_p)


def _he(rng, cin, cout):
    """he-normal HWIO kernel and a bias (tests/test_gpu_conv.py)."""
    return ((rng.standard_normal((3, 3, cin, cout)) * np.sqrt(2.0 / (9 * cin))).astype(np.float32),
            (rng.standard_normal(cout) * 0.1).astype(np.float32))


# ---- the harness sees a real kernel's writes ----------------------------------------------------------------------------------
def test_the_harness_reports_a_kernel_that_covers_one_image_too_many_or_too_few():
    """tests/test_guarded_host.py shows run_three_ways failing on CPU stand-ins; here on device memory under a real launch.
    dsen2_split_f32 is asked for n + 1 images where the harness was told n (the extra image of input exists; the extra output
    lands in the tail guards, which are allocated memory at least as large as the tensor), then for n - 1."""
    n, h, w, c = 2, 7, 9, 128
    x = _dev(_rng(1).standard_normal((n + 1, h, w, c)).astype(np.float32))
    planes = (n, c // 8, h, w, 8)
    for images, expect in ((n + 1, 'tail guard'), (n - 1, 'never written')):
        with pytest.raises(AssertionError) as e:
            _run('split_f32 told %d images' % images, lambda inp, out, _, __: _lib_call(
                # (the plain run's outputs have no guard behind them: it gets the true n)
                'dsen2_split_f32', _ptr(inp[0]), _ptr(out[0]), _ptr(out[1]), images if out[0].storage_offset() else n, h, w, c),
                [x], [(planes, I16), (planes, I16)])
        assert expect in str(e.value) and 'output 0' in str(e.value), str(e.value)
        if images > n:
            lo, hi = (int(v) for v in re.search(r'bytes (\d+)\.\.(\d+) past the last element', str(e.value)).groups())
            assert lo < 16 and h * w * c * 2 - 16 <= hi < h * w * c * 2       # one image of int16 (a data byte may equal the poison)


# ---- whole network: dsen2_model_forward -------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=3)
def _model(bands, d, feat, precision, train_precision=0):
    m = s2model(tuple((c, None, None) for c in bands), num_layers=d, feature_size=feat, device=DEV, precision=precision)
    m.set_weights_flat(weights.random_he_uniform(sum(bands), bands[-1], d, feat, seed=1, bias_scale=0.05))
    if train_precision:
        with torch.cuda.device(DEV):
            _lib.call('dsen2_model_set_train_precision', m._handle, train_precision)
    return m


def _inputs(bands, n, h, w, seed):
    """tests/test_gpu_train.py's inputs: U[0, 0.5)."""
    rng = _rng(seed, n, h, w)
    return [_dev(rng.uniform(0.0, 0.5, (n, c, h, w)).astype(np.float32)) for c in bands]


def _forward_row(what, m, xs, n, h, w):
    ws_bytes = _size('dsen2_model_workspace_bytes', m._handle, n, h, w)

    def call(inp, out, _, scr):
        _lib_call('dsen2_model_forward', m._handle, _ptr(inp[0]), _ptr(inp[1]), _ptr(inp[2]), _ptr(out[0]), n, h, w, _ptr(scr[0]),
                  scr[0].numel())
    return _run(what, call, list(xs) + [None] * (3 - len(xs)), [((n, m.cout, h, w), F32)], scratch=[ws_bytes])


NETS = [((4, 6), 2, 128), ((4, 6, 2), 1, 256)]
NHW = [(1, 1, 1), (3, 21, 37), (2, 16, 33)]
FORWARD = [(p, bands, d, feat, n, h, w) for p in ('fp32', 'bf16', 'bf16x3') for bands, d, feat in NETS for n, h, w in NHW] + \
    [(p, (3, 5), 1, 128, 2, 16, 16) for p in ('fp32', 'bf16', 'bf16x3')]        # no Sentinel-2 band group: the generic first layer


@pytest.mark.parametrize('precision,bands,d,feat,n,h,w', FORWARD)
def test_forward(precision, bands, d, feat, n, h, w):
    m = _model(bands, d, feat, precision)
    _forward_row('forward %s %r d=%d F=%d %dx%dx%d' % (precision, bands, d, feat, n, h, w), m, _inputs(bands, n, h, w, 1), n, h, w)


@pytest.mark.parametrize('precision', ['bf16', 'bf16x3'])
@pytest.mark.parametrize('feat,d,n,h,w', [(128, 2, 301, 16, 32), (256, 2, 511, 16, 32)])
def test_forward_chain_kernel(precision, feat, d, n, h, w):
    """The persistent chain launch (one launch for all 2 d residual-block convolutions): the tail workgroup owns a single item per
    layer.  The hundreds of MB of workspace are poisoned like every other."""
    m = _model((4, 6), d, feat, precision)
    assert m.body_launches(n, h, w) == 1
    rng = np.random.Generator(np.random.PCG64(n + h))
    xs = [_dev(rng.random((n, c, h, w), dtype=np.float32) * np.float32(5.0)) for c in (4, 6)]
    _forward_row('chain %s F=%d d=%d %dx%dx%d' % (precision, feat, d, n, h, w), m, xs, n, h, w)


@pytest.mark.parametrize('precision', ['fp32', 'bf16', 'bf16x3'])
def test_forward_device_reuses_its_workspace_across_shapes(precision):
    """S2Model keeps one workspace per stream: the short last batch runs in what the big one left behind."""
    used, fresh = (_model.__wrapped__((4, 6), 2, 128, precision) for _ in range(2))
    used.forward_device(_inputs((4, 6), 8, 32, 32, 2))
    xs = _inputs((4, 6), 5, 21, 37, 3)
    got, want = used.forward_device(xs), fresh.forward_device(xs)
    torch.cuda.synchronize()
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))


# ---- training step: dsen2_model_gradients, dsen2_nadam_step, the flat weight vector -------------------------------------------
TRAIN_MODES = {'fp32': ('fp32', 0), 'bf16x3': ('bf16x3', 0), 'fp32-amp': ('fp32', 1)}
TRAIN_NETS = [((4, 6), 2, 128, 3, 21, 37), ((4, 6, 2), 1, 256, 1, 9, 21), ((4, 6), 1, 128, 2, 1, 1), ((4, 6), 0, 128, 2, 5, 7)]


@pytest.mark.parametrize('with_loss2', [True, False], ids=['loss2', 'loss2-null'])
@pytest.mark.parametrize('with_out', [True, False], ids=['out', 'out-null'])
@pytest.mark.parametrize('bands,d,feat,n,h,w', TRAIN_NETS)
@pytest.mark.parametrize('mode', list(TRAIN_MODES))
def test_gradients(mode, bands, d, feat, n, h, w, with_out, with_loss2):
    precision, train_precision = TRAIN_MODES[mode]
    m = _model(bands, d, feat, precision, train_precision)
    ws_bytes = _size('dsen2_model_train_workspace_bytes', m._handle, n, h, w)
    xs = _inputs(bands, n, h, w, 5)
    y = _dev(_rng(6, n, h, w).uniform(0, 0.5, (n, bands[-1], h, w)).astype(np.float32))
    outputs = [((m.count_params(),), F32)] + [((n, m.cout, h, w), F32)] * with_out + [((2,), F32)] * with_loss2

    def call(inp, out, _, scr):
        o = out[1] if with_out else None
        l2 = out[-1] if with_loss2 else None
        _lib_call('dsen2_model_gradients', m._handle, _ptr(inp[0]), _ptr(inp[1]), _ptr(inp[2]), _ptr(inp[3]), _ptr(o), _ptr(out[0]),
                  _ptr(l2), n, h, w, _ptr(scr[0]), scr[0].numel())
    _run('gradients %s %r d=%d F=%d %dx%dx%d' % (mode, bands, d, feat, n, h, w), call,
         list(xs) + [None] * (3 - len(xs)) + [y], outputs, scratch=[ws_bytes])


@pytest.mark.parametrize('mode', list(TRAIN_MODES))
def test_gradients_device_reuses_its_workspace_across_shapes(mode):
    """gradients_device keeps one workspace too: the short last batch of an epoch steps in what the full one left behind."""
    precision, train_precision = TRAIN_MODES[mode]
    used, fresh = (_model.__wrapped__((4, 6), 2, 128, precision, train_precision) for _ in range(2))

    def step(m, n, h, w, seed):
        grad = torch.empty(m.count_params(), dtype=F32, device=DEV)
        loss2 = torch.empty(2, dtype=F32, device=DEV)
        y = _dev(_rng(seed, 9).uniform(0, 0.5, (n, 6, h, w)).astype(np.float32))
        out = m.gradients_device(_inputs((4, 6), n, h, w, seed), y, grad, loss2, out=torch.empty((n, 6, h, w), dtype=F32, device=DEV))
        torch.cuda.synchronize()
        return [t.view(torch.int32) for t in (grad, loss2, out)]
    used._train = {}                        # where a compiled model keeps the buffer (S2Model.gradients_device)
    step(used, 8, 32, 32, 2)
    kept = used._train['ws']
    got, want = step(used, 5, 21, 37, 3), step(fresh, 5, 21, 37, 3)
    assert used._train['ws'] is kept
    for a, b in zip(got, want):
        assert torch.equal(a, b)


@pytest.mark.parametrize('count', [10007, 1])
def test_nadam_step(count):
    rng = _rng(11, count)
    p, g, m = (_dev(rng.uniform(-1, 1, count).astype(np.float32)) for _ in range(3))
    v = _dev(rng.uniform(0, 1, count).astype(np.float32))
    s = training.Nadam(lr=1e-3).next_step()

    def call(inp, _, inplace, __):
        _lib_call('dsen2_nadam_step', _ptr(inplace[0]), _ptr(inp[0]), _ptr(inplace[1]), _ptr(inplace[2]), count, s['lr'], s['b1'], s['b2'],
                  s['eps'], s['mc_t'], s['mc_t1'], s['ms_new'], s['ms_next'], s['b2_pow_t'])
    _run('nadam %d' % count, call, [g], [], inplace=[p, m, v])


@pytest.mark.parametrize('precision,bands,d,feat', [('fp32', (4, 6), 2, 128), ('bf16x3', (4, 6, 2), 1, 256)])
def test_flat_weight_vector(precision, bands, d, feat):
    m = _model.__wrapped__(bands, d, feat, precision)
    count = m.count_params()
    _run('get_weights %s' % precision, lambda _, out, __, ___: _lib_call('dsen2_model_get_weights', m._handle, _ptr(out[0])),
         [], [((count,), F32)])
    new = _dev(weights.random_he_uniform(sum(bands), bands[-1], d, feat, seed=9, bias_scale=0.1))

    def call(inp, out, _, __):
        _lib_call('dsen2_model_set_weights_device', m._handle, _ptr(inp[0]))
        _lib_call('dsen2_model_get_weights', m._handle, _ptr(out[0]))
    back, _ = _run('set_weights_device %s' % precision, call, [new], [((count,), F32)])
    assert torch.equal(back[0].view(torch.int32), new.view(torch.int32))


# ---- convolutions at kernel level ---------------------------------------------------------------------------------------------
CONV_SHAPES = [(1, 1, 1), (2, 21, 37), (1, 16, 33)]
# cin, cout, epilogue; (16, 256, 1) is the geometry of the output layer's input gradient; (128, 7, 2) the vector-unit kernel
CONV_LAYERS = [(16, 128, 0), (128, 128, 0), (128, 128, 1), (256, 256, 1), (16, 256, 1), (128, 6, 2), (256, 2, 2), (128, 7, 2)]
CONV = [(cin, cout, epi, n, h, w, False) for cin, cout, epi in CONV_LAYERS for n, h, w in CONV_SHAPES + [(1, 9, 230)] * (epi == 2)] + \
    [(128, 128, 1, n, h, w, True) for n, h, w in CONV_SHAPES]


@pytest.mark.parametrize('entry', ['dsen2_conv3x3_nhwc', 'dsen2_conv3x3_nhwc_ref'])
@pytest.mark.parametrize('cin,cout,epilogue,n,h,w,in_place', CONV)
def test_conv3x3_nhwc(entry, cin, cout, epilogue, n, h, w, in_place):
    rng = _rng(cin, cout, epilogue, h, w)
    x = _dev(rng.standard_normal((n, h, w, cin)).astype(np.float32))
    (k, kp), (b, bp) = (_host(a) for a in _he(rng, cin, cout))
    out_shape = (n, cout, h, w) if epilogue == 2 else (n, h, w, cout)
    aux = _dev(rng.standard_normal(out_shape).astype(np.float32)) if epilogue else None
    what = '%s %d->%d epilogue %d %dx%dx%d%s' % (entry, cin, cout, epilogue, n, h, w, ' in place' if in_place else '')
    if in_place:
        _run(what, lambda inp, _, io, __: _lib_call(entry, _ptr(inp[0]), kp, bp, _ptr(io[0]), _ptr(io[0]), n, h, w, cin, cout, epilogue,
                                                   0.1), [x], [], inplace=[aux])
    else:
        _run(what, lambda inp, out, _, __: _lib_call(entry, _ptr(inp[0]), kp, bp, _ptr(inp[1]), _ptr(out[0]), n, h, w, cin, cout,
                                                    epilogue, 0.1), [x, aux], [(out_shape, F32)])


@pytest.mark.parametrize('n,h,w', [(1, 1, 1), (2, 21, 37), (3, 5, 70)])
@pytest.mark.parametrize('epilogue', [0, 1, 3])
@pytest.mark.parametrize('feat', [128, 256])
@pytest.mark.parametrize('x3', [False, True], ids=['bf16', 'bf16x3'])
def test_conv3x3_body_16bit(x3, feat, epilogue, n, h, w):
    """dsen2_conv3x3_body_bf16 / _bf16x3: epilogue 0 writes the operand tensor of the next layer, 1 updates the stream's planes in
    place, 3 writes fp32 and leaves the planes alone."""
    entry = 'dsen2_conv3x3_body_bf16x3' if x3 else 'dsen2_conv3x3_body_bf16'
    rng = _rng(feat, epilogue, h, w, x3)
    (k, kp), (b, bp) = (_host(a) for a in _he(rng, feat, feat))
    t = _dev(rng.standard_normal((n, h, w, feat)).astype(np.float32))
    s = _dev(rng.standard_normal((n, h, w, feat)).astype(np.float32))
    x = split3_f32(t)[0] if x3 else split_f32(t)[0]               # the operand: two planes (hi | xl) or one
    s0, s1 = split3_f32(s) if x3 else split_f32(s)                # the residual stream's tensors
    what = '%s F=%d epilogue %d %dx%dx%d' % (entry, feat, epilogue, n, h, w)
    if epilogue == 0:
        _run(what, lambda inp, out, _, __: _lib_call(entry, _ptr(inp[0]), kp, bp, NULL, NULL, _ptr(out[0]), n, h, w, feat, 0, 0.1),
             [x], [(tuple(x.shape), I16)])
    elif epilogue == 1:
        _run(what, lambda inp, _, io, __: _lib_call(entry, _ptr(inp[0]), kp, bp, _ptr(io[0]), _ptr(io[1]), NULL, n, h, w, feat, 1, 0.1),
             [x], [], inplace=[s0, s1])
    else:
        _run(what, lambda inp, out, _, __: _lib_call(entry, _ptr(inp[0]), kp, bp, _ptr(inp[1]), _ptr(inp[2]), _ptr(out[0]), n, h, w, feat,
                                                    3, 0.1), [x, s0, s1], [((n, h, w, feat), F32)])


@pytest.mark.parametrize('n,h,w', [(1, 1, 1), (3, 21, 37)])
@pytest.mark.parametrize('feat', [128, 256])
@pytest.mark.parametrize('bands', [(4, 6), (4, 6, 2)])
@pytest.mark.parametrize('precision', [1, 2])
def test_conv3x3_first_planes(precision, bands, feat, n, h, w):
    rng = _rng(precision, feat, h, len(bands))
    xs = [_dev(rng.random((n, c, h, w), dtype=np.float32) * np.float32(5.0)) for c in bands]      # tests/test_gpu_first16.py
    cin = sum(bands)
    k, kp = _host(rng.uniform(-1, 1, (3, 3, cin, feat)) * np.sqrt(6.0 / (9 * cin)))
    b, bp = _host(rng.standard_normal(feat) * 0.1)
    planes = (n, feat // 8, h, w, 8)
    c60 = bands[2] if len(bands) == 3 else 0

    def call(inp, out, _, __):
        _lib_call('dsen2_conv3x3_first_planes', _ptr(inp[0]), _ptr(inp[1]), _ptr(inp[2]), 4, 6, c60, kp, bp, feat, precision, _ptr(out[0]),
                  _ptr(out[1]), n, h, w)
    _run('first_planes precision %d %r F=%d %dx%dx%d' % (precision, bands, feat, n, h, w), call, xs + [None] * (3 - len(xs)),
         [((n, 2) + planes[1:] if precision == 2 else planes, I16), (planes, I16)])


@pytest.mark.parametrize('n,h,w', [(3, 7, 9), (1, 1, 33)])
@pytest.mark.parametrize('c', [8, 128, 512])
@pytest.mark.parametrize('entry', ['dsen2_split_f32', 'dsen2_join_f32', 'dsen2_split3_f32', 'dsen2_join3_f32'])
def test_split_and_join(entry, c, n, h, w):
    rng = _rng(c, n, h, w)
    planes = (n, c // 8, h, w, 8)
    first = (n, 2) + planes[1:] if entry.endswith('3_f32') else planes
    what = '%s c=%d %dx%dx%d' % (entry, c, n, h, w)
    if 'split' in entry:
        x = _dev((rng.standard_normal((n, h, w, c)) * np.exp(rng.uniform(-6, 6, (n, h, w, c)))).astype(np.float32))
        _run(what, lambda inp, out, _, __: _lib_call(entry, _ptr(inp[0]), _ptr(out[0]), _ptr(out[1]), n, h, w, c), [x],
             [(first, I16), (planes, I16)])
    else:                                   # every bit pattern joins
        a, b = (_dev(rng.integers(-32768, 32768, shape).astype(np.int16)) for shape in (first, planes))
        _run(what, lambda inp, out, _, __: _lib_call(entry, _ptr(inp[0]), _ptr(inp[1]), _ptr(out[0]), n, h, w, c), [a, b],
             [((n, h, w, c), F32)])


# tests/test_gpu_train.py's first-layer, output-layer and 1 x 1 cases; shape B of tests/test_gpu_wgrad_runs.py (several tiles per
# split-K run); F = 256 ragged: n, h, w, ca, cg, ci, co
WGRAD_FP32 = [(3, 5, 7, 16, 128, 10, 128), (2, 12, 12, 16, 256, 12, 256), (2, 11, 13, 128, 16, 128, 6), (1, 1, 1, 256, 16, 256, 2),
              (1, 1, 1, 128, 128, 128, 128), (7, 21, 37, 128, 128, 128, 128), (1, 9, 21, 256, 256, 256, 256)]
WGRAD = [('fp32',) + c for c in WGRAD_FP32] + [(kind,) + c for kind in ('bf16x3', 'bf16') for c in WGRAD_FP32[4:]]


@pytest.mark.parametrize('kind,n,h,w,ca,cg,ci,co', WGRAD)
def test_conv3x3_wgrad(kind, n, h, w, ca, cg, ci, co):
    rng = np.random.default_rng(n * 1000 + h * 10 + w)
    a = rng.uniform(-1, 1, (n, h, w, ca)).astype(np.float32)
    g = rng.uniform(-1, 1, (n, h, w, cg)).astype(np.float32)
    a[..., ci:] = 0
    g[..., co:] = 0
    ad, gd = _dev(a), _dev(g)
    if kind == 'fp32':
        def call(inp, out, _, __):
            _lib_call('dsen2_conv3x3_wgrad', _ptr(inp[0]), _ptr(inp[1]), _ptr(out[0]), _ptr(out[1]), n, h, w, ca, cg, ci, co, 0.5)
    else:
        entry = 'dsen2_conv3x3_wgrad_' + kind
        ad, gd = (split3_f32(t)[0] if kind == 'bf16x3' else split_f32(t)[0] for t in (ad, gd))

        def call(inp, out, _, __):
            _lib_call(entry, _ptr(inp[0]), _ptr(inp[1]), _ptr(out[0]), _ptr(out[1]), n, h, w, ca, 0.5)
    _run('wgrad %s %dx%dx%d %d->%d' % (kind, n, h, w, ci, co), call, [ad, gd], [((3, 3, ci, co), F32), ((co,), F32)])


# ---- tiling, up-sampling, training-set creation -------------------------------------------------------------------------------
# H, W, C, P, border: the last row and column of patches are clamped; one patch
TILINGS = [(70, 53, 3, 32, 4), (24, 24, 3, 32, 4)]


@pytest.mark.parametrize('H,W,C,P,border', TILINGS)
def test_tile_gather(H, W, C, P, border):
    img = _dev(_rng(H, W).uniform(0, 12000, (H, W, C)).astype(np.float32))
    org, _ = gp.tile_origins((H, W), P, border)
    count = org.shape[0]
    assert count == (9 if H == 70 else 1)
    _run('tile_gather %dx%dx%d' % (H, W, C), lambda inp, out, _, __: _lib_call(
        'dsen2_tile_gather', _ptr(inp[0]), H, W, C, border, _ptr(inp[1]), count, P, 2000.0, _ptr(out[0])),
        [img, _dev(org)], [((count, C, P, P), F32)])


@pytest.mark.parametrize('H,W,C,P,border', TILINGS)
def test_recompose(H, W, C, P, border):
    x_tiles, y_tiles = gp.recompose_grid((H, W), P, border)
    count = x_tiles * y_tiles
    a = _dev(_rng(H, W, 1).uniform(0, 6, (count, C, P, P)).astype(np.float32))
    _run('recompose %dx%dx%d' % (H, W, C), lambda inp, out, _, __: _lib_call(
        'dsen2_recompose', _ptr(inp[0]), count, C, P, border, _ptr(out[0]), H, W, 2000.0), [a], [((H, W, C), F32)])
    # rows [row0, row1) only: the other rows of the image are the caller's and stay what they were
    img = _dev(_rng(H, W, 2).uniform(0, 6, (H, W, C)).astype(np.float32))
    for row0, row1 in ((0, H), (H // 3, H - 5), (H - 1, H)):
        (_, (got,)) = _run('recompose_rows %dx%dx%d [%d, %d)' % (H, W, C, row0, row1), lambda inp, _, io, __: _lib_call(
            'dsen2_recompose_rows', _ptr(inp[0]), count, C, P, border, _ptr(io[0]), H, W, 2000.0, row0, row1), [a], [], inplace=[img])
        keep = torch.ones(H, dtype=torch.bool, device=DEV)
        keep[row0:row1] = False
        assert torch.equal(got[keep].view(torch.int32), img[keep].view(torch.int32))


@pytest.mark.parametrize('entry', ['dsen2_upsample_mirror_bilinear', 'dsen2_upsample_mirror_bilinear_ref'])
@pytest.mark.parametrize('n,c,h,w,oh,ow', [(2, 3, 1, 1, 2, 2), (1, 2, 10, 10, 27, 27), (1, 2, 37, 53, 74, 106)])
def test_upsample(entry, n, c, h, w, oh, ow):
    x = _dev((_rng(h, w, oh).random((n, c, h, w), dtype=np.float32) * 12000).astype(np.float32))
    _run('%s %dx%d -> %dx%d' % (entry, h, w, oh, ow), lambda inp, out, _, __: _lib_call(
        entry, _ptr(inp[0]), _ptr(out[0]), n * c, h, w, oh, ow, 2000.0), [x], [((n, c, oh, ow), F32)])


@pytest.mark.parametrize('out_f64', [0, 1], ids=['f32-out', 'f64-out'])
@pytest.mark.parametrize('H,W,C,scale,u16', [(30, 42, 5, 3, True), (12, 18, 4, 6, True), (8, 8, 1, 2, False), (20, 36, 19, 4, False)])
def test_down_pixel_aggr(H, W, C, scale, u16, out_f64):
    rng = _rng(H, W, C, scale)
    if u16:
        img = _dev(rng.integers(0, 65536, (H, W, C)).astype(np.uint16).view(np.int16))
    else:
        img = _dev(rng.uniform(0, 12000, (H, W, C)).astype(np.float32))
    wts, radius = gp.gaussian_weights(scale)
    host_w = (ctypes.c_double * len(wts))(*wts)
    _run('down_pixel_aggr %dx%dx%d / %d' % (H, W, C, scale), lambda inp, out, _, __: _lib_call(
        'dsen2_down_pixel_aggr', _ptr(inp[0]), _lib.DTYPE_U16 if u16 else _lib.DTYPE_F32, H, W, C, scale, host_w, radius, _ptr(out[0]),
        out_f64), [img], [((H // scale, W // scale, C), F64 if out_f64 else F32)])


# ---- evaluation ---------------------------------------------------------------------------------------------------------------
def _image(rng, shape, dtype):
    if dtype == 'u16':
        return _dev(rng.integers(0, 65536, shape).astype(np.uint16).view(np.int16)), _lib.DTYPE_U16
    if dtype == 'f32':
        return _dev(rng.uniform(0, 12000, shape).astype(np.float32)), _lib.DTYPE_F32
    return _dev(rng.uniform(0, 12000, shape)), _lib.DTYPE_F64


@pytest.mark.parametrize('H,W,C', [(3, 5, 2), (23, 31, 13)])
@pytest.mark.parametrize('scale', [2.0, 1.0 / 3.0], ids=['x2', 'x1/3'])
@pytest.mark.parametrize('dtype', ['u16', 'f32', 'f64'])
@pytest.mark.parametrize('axis', [0, 1])
def test_imresize_axis(axis, dtype, scale, H, W, C):
    img, code = _image(_rng(H, W, axis), (H, W, C), dtype)
    in_len = (H, W)[axis]
    out_len = int(ceil(scale * in_len))
    wts, idx, taps = ir.device_taps(in_len, out_len, scale, DEV)
    shape = (out_len, W, C) if axis == 0 else (H, out_len, C)
    _run('imresize_axis %d %s x%g %dx%dx%d' % (axis, dtype, scale, H, W, C), lambda inp, out, _, __: _lib_call(
        'dsen2_imresize_axis', _ptr(inp[0]), code, H, W, C, axis, out_len, _ptr(inp[1]), _ptr(inp[2]), taps, _ptr(out[0])),
        [img, wts, idx], [(shape, F64)])


def _pair(H, W, C):
    rng = _rng(H, W, C)
    gt = rng.uniform(100, 12000, (H, W, C))
    x = (gt + rng.normal(0, 300, (H, W, C))).astype(np.float32)
    return _dev(x), _lib.DTYPE_F32, _dev(gt), _lib.DTYPE_F64


def _ssim_args(H, W):
    win = 11 if min(H, W) >= 11 else 7
    w = metrics.ssim_window(win, 1.5)
    return (ctypes.c_double * win)(*w.tolist()), win, (0.01 * 12000.0) ** 2, (0.03 * 12000.0) ** 2


@pytest.mark.parametrize('H,W,C', [(9, 23, 2), (64, 100, 13)])
@pytest.mark.parametrize('entry', ['dsen2_band_errors', 'dsen2_uiq_sums', 'dsen2_sam_sums', 'dsen2_ssim_sums', 'dsen2_uiq_map',
                                   'dsen2_ssim_map'])
def test_evaluation_sums_and_maps(entry, H, W, C):
    x, xd, gt, gd = _pair(H, W, C)
    block = 8
    window, win, c1, c2 = _ssim_args(H, W)
    head = lambda inp: (_ptr(inp[0]), xd, _ptr(inp[1]), gd, H, W, C)      # noqa: E731
    work = [_size('dsen2_band_errors_workspace_bytes' if entry == 'dsen2_band_errors' else 'dsen2_quality_workspace_bytes', C)]
    what = '%s %dx%dx%d' % (entry, H, W, C)
    if entry == 'dsen2_uiq_map':
        _run(what, lambda inp, out, _, __: _lib_call(entry, *(head(inp) + (block, _ptr(out[0])))), [x, gt],
             [((H - block + 1, W - block + 1, C), F64)])
    elif entry == 'dsen2_ssim_map':
        _run(what, lambda inp, out, _, __: _lib_call(entry, *(head(inp) + (window, win, c1, c2, _ptr(out[0])))), [x, gt],
             [((H - win + 1, W - win + 1, C), F64)])
    else:
        extra = {'dsen2_band_errors': (), 'dsen2_uiq_sums': (block,), 'dsen2_sam_sums': (), 'dsen2_ssim_sums': (window, win, c1, c2)}[entry]
        shape = {'dsen2_band_errors': (C, 3), 'dsen2_uiq_sums': (C, 2), 'dsen2_sam_sums': (2,), 'dsen2_ssim_sums': (C, 2)}[entry]
        _run(what, lambda inp, out, _, scr: _lib_call(entry, *(head(inp) + extra + (_ptr(scr[0]), scr[0].numel(), _ptr(out[0])))),
             [x, gt], [(shape, F64)], scratch=work)


@pytest.mark.parametrize('axis', [0, 1])
@pytest.mark.parametrize('entry', ['dsen2_imresize_band_errors', 'dsen2_imresize_uiq_sums', 'dsen2_imresize_sam_sums',
                                   'dsen2_imresize_ssim_sums'])
def test_fused_resample_and_sums(entry, axis):
    """The second pass of the bicubic baseline fused into the reduction: the weight and index tables and dev_gt are inputs."""
    H, W, C = 14, 22, 6
    rng = _rng(H, W, axis, 7)
    mid = _dev(rng.uniform(100, 12000, (H, W, C)))
    in_len = (H, W)[axis]
    out_len = 2 * in_len
    shape = (out_len, W, C) if axis == 0 else (H, out_len, C)
    gt = _dev(rng.uniform(100, 12000, shape).astype(np.float32))
    wts, idx, taps = ir.device_taps(in_len, out_len, 2.0, DEV)
    window, win, c1, c2 = _ssim_args(shape[0], shape[1])
    extra = {'dsen2_imresize_band_errors': (), 'dsen2_imresize_uiq_sums': (8,), 'dsen2_imresize_sam_sums': (),
             'dsen2_imresize_ssim_sums': (window, win, c1, c2)}[entry]
    out_shape = {'dsen2_imresize_band_errors': (C, 3), 'dsen2_imresize_uiq_sums': (C, 2), 'dsen2_imresize_sam_sums': (2,),
                 'dsen2_imresize_ssim_sums': (C, 2)}[entry]
    work = [_size('dsen2_band_errors_workspace_bytes' if entry == 'dsen2_imresize_band_errors' else 'dsen2_quality_workspace_bytes', C)]
    _run('%s axis %d' % (entry, axis), lambda inp, out, _, scr: _lib_call(
        entry, *((_ptr(inp[0]), _lib.DTYPE_F64, H, W, C, axis, out_len, _ptr(inp[1]), _ptr(inp[2]), taps, _ptr(inp[3]), _lib.DTYPE_F32) +
                 extra + (_ptr(scr[0]), scr[0].numel(), _ptr(out[0])))), [mid, wts, idx, gt], [(out_shape, F64)], scratch=work)
