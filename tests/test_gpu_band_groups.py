"""Every band grouping dsen2_model_create accepts, forward and training (include/dsen2_hip.h: c10 >= 1, c20 >= 1, c60 >= 0,
c10 + c20 + c60 <= 16, so 1 .. 15 output channels).

The rest of the suite builds (4, 6) and (4, 6, 2) networks, which run the direct first-layer kernels (conv3x3_first.hip,
conv3x3_first16.hip) and the matrix-core output kernel at Cout 6 / 2.  Any other grouping runs the code this file is about:
launch_pack_inputs + the generic tile kernel as first layer (its CREAL form for 10 or 12 input channels whatever the groups,
its kEpiReluSplit epilogue in a 'bf16' model, kEpiRelu + launch_split3_f32 in a 'bf16x3' one), the output layer on
out_mfma<F, 1> (Cout 1 .. 2), out_mfma<F, 3> (3 .. 6), the vector-unit kernel (7 .. 8) or the tile kernel's kEpiSkipNCHW instance
(9 .. 15), and the loss, weight-gradient, dgrad and gather kernels of the training step at those channel counts.

 1. forward against the float64 C oracle at the suite's own gates, plus a maximum-error gate in fp32;
 2. identities that need no tolerance: regrouped inputs, zero padding lanes, delta kernels through the whole model, zero weights;
 3. (tests/test_gpu_conv.py: the output convolution alone at Cout 1, 4, 8, 9, 15, 16, 32)
 4. training: gradients against float64 autograd in the three training modes, the weight-gradient kernel at the channel edges bit
    for bit, one step end to end, the flat weight vector;
 5. the memory contract of forward and gradients (tests/guarded.py);
 6. what dsen2_model_create and dsen2_conv3x3_first_planes refuse.
`python -m pytest tests/test_gpu_band_groups.py -m gpu -s` prints every figure; profiles/band_groups_parity.txt holds a run."""
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

import test_gpu_memory_contract as MC  # noqa: E402    run_three_ways rows of forward and gradients
import test_gpu_train as T32  # noqa: E402              the float64 autograd restatement of the training graph
import test_gpu_train_amp as TA  # noqa: E402           mixed bf16: the comparison with tests/amp_bf16_restatement.py
import test_gpu_train_bf16x3 as T3  # noqa: E402        _reference: a cached float64 case with its ReLU margin
import test_gpu_wgrad_runs as WR  # noqa: E402          the exact small-integer method of the weight-gradient kernels
from dsen2_amd import _lib, training, weights  # noqa: E402
from dsen2_amd.DSen2Net import _ptr, _stream_ptr, conv3x3_first_planes, conv3x3_nhwc, s2model  # noqa: E402
from oracle import c_oracle  # noqa: E402                checker only
from oracle import dsen2_oracle as do  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda', 0)
PRECISIONS = ('fp32', 'bf16', 'bf16x3')

# bands -> what the grouping reaches that the others do not
GROUPS = {
    (1, 1): 'tile first layer, 14 zero lanes; out_mfma<F,1> with one output',
    (6, 4): 'CREAL 10 with other offsets than 4 + 6; out_mfma<F,3>, Cout not a multiple of 3',
    (5, 5, 2): 'CREAL 12, three inputs regrouped',
    (3, 7, 2): 'the concatenation of (4, 6, 2)',
    (2, 7): 'vector-unit output kernel',
    (8, 8): 'all 16 input lanes real; Cout 8',
    (1, 12): 'output layer on the tile kernel (kEpiSkipNCHW, cout_pad 32)',
    (1, 15): 'the largest Cout of a model',
    (4, 6, 1): 'Sentinel-2 prefix, but not a Sentinel-2 grouping',
}


def _shape(bands):
    return tuple((c, None, None) for c in bands)


@functools.lru_cache(maxsize=6)
def _net(bands, d, feat, precision):
    """One inference model per (network, precision); the tests load the weights they need."""
    return s2model(_shape(bands), num_layers=d, feature_size=feat, device=DEV, precision=precision)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- 1. forward against the float64 oracle ------------------------------------------------------------------------------------------
# bands, F, d, n, h, w: every grouping at a ragged two-image shape (9 x 21: one tile row, a second ragged tile column) and at one
# pixel; F = 256; the full DSen2 depth; and networks without residual blocks, which the plan makes fp32 in every precision.
FORWARD = [(b, 128, 2) + nhw for b in GROUPS for nhw in ((2, 9, 21), (1, 1, 1))] + \
    [(b, 256, 1, 1, 21, 37) for b in ((6, 4), (1, 15), (3, 7, 2))] + \
    [((5, 5, 2), 128, 6, 1, 8, 8)] + \
    [(b, 128, 0, 2, 9, 21) for b in ((1, 15), (6, 4))]
FP32_RMSE_GATE = 5e-6                    # tests/test_gpu_forward.py::test_forward_matches_golden_fixture
FP32_MAX_GATE = 10 * FP32_RMSE_GATE      # no single pixel or channel hides inside an rms
BF16X3_RMSE_GATE = 1e-4                  # tests/test_gpu_bf16x3.py
BF16_REL_GATE = 5e-3                     # tests/test_gpu_bf16.py: rmse / rms of the reference


@functools.lru_cache(maxsize=None)
def _forward_case(bands, feat, d, n, h, w):
    """(weights, inputs, float64 oracle output): computed once, never modified."""
    flat = do.he_uniform_weights(sum(bands), bands[-1], d, feat, seed=1, bias_scale=0.05)
    xs = do.synthetic_inputs(n, h, w, bands, seed=10 * h + w + d)
    ref = c_oracle.forward(xs, flat, d, feat)
    for a in [flat, ref] + xs:
        a.setflags(write=False)
    return flat, xs, ref


def _gate_forward(y, ref, precision, what):
    e, mx = do.rmse(y, ref), float(np.abs(y.astype(np.float64) - ref).max())
    rms = float(np.sqrt(np.mean(np.asarray(ref, np.float64) ** 2)))
    print('forward %-6s %s: rmse %.3e  max %.3e  rmse / rms(ref) %.3e' % (precision, what, e, mx, e / rms))
    assert y.dtype == np.float32 and y.shape == ref.shape and np.isfinite(y).all()
    if precision == 'fp32':
        assert e < FP32_RMSE_GATE, (what, e)
        assert mx < FP32_MAX_GATE, (what, mx)
    elif precision == 'bf16x3':
        assert e < BF16X3_RMSE_GATE, (what, e)
    else:
        assert e / rms < BF16_REL_GATE, (what, e / rms)


@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('bands,feat,d,n,h,w', FORWARD)
def test_forward_matches_float64_oracle(bands, feat, d, n, h, w, precision):
    flat, xs, ref = _forward_case(bands, feat, d, n, h, w)
    m = _net(bands, d, feat, precision)
    assert m.count_params() == flat.size and m.cout == bands[-1]
    m.set_weights_flat(flat)
    _gate_forward(m.predict(xs), ref, precision, '%-9r F=%d d=%d %dx%dx%d' % (bands, feat, d, n, h, w))


@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('bands', [(1, 1), (6, 4), (2, 7), (1, 15)])
def test_batching_is_invisible(bands, precision):
    """predict cut into batches of 2 (the last one short) gives the bits of one batch of 5."""
    flat = do.he_uniform_weights(sum(bands), bands[-1], 1, 128, seed=3, bias_scale=0.05)
    xs = do.synthetic_inputs(5, 9, 21, bands, seed=2)
    m = _net(bands, 1, 128, precision)
    m.set_weights_flat(flat)
    assert np.array_equal(_bits(m.predict(xs)), _bits(m.predict(xs, batch_size=2)))


# ---- 2. identities that need no tolerance ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('feat,n,h,w', [(128, 3, 21, 37), (256, 1, 16, 16)])
def test_regrouped_inputs_are_the_same_function(feat, n, h, w, precision):
    """(3, 7, 2) and (9, 1, 2) models with the weights of a (4, 6, 2) model, fed the same twelve planes cut at other boundaries.
    fp32: the bits of the Sentinel-2 model (its direct first kernel gives the generic kernel's bits:
    test_first_layer_without_padding_mfmas_gives_the_same_bits; CREAL 12 drops terms that are exactly zero).  In the 16-bit modes
    the Sentinel-2 model's first convolution runs on bf16 operands (conv3x3_first16.hip) and the regrouped ones' in fp32, by
    design: there the outputs are compared with each other at the gates of section 1."""
    d = 2
    flat = do.he_uniform_weights(12, 2, d, feat, seed=4, bias_scale=0.05)
    xs = do.synthetic_inputs(n, h, w, (4, 6, 2), seed=7)
    planes = np.concatenate(xs, axis=1)
    s2 = _net((4, 6, 2), d, feat, precision)
    s2.set_weights_flat(flat)
    y0 = s2.predict(xs)
    for bands in ((3, 7, 2), (9, 1, 2)):
        parts = [np.ascontiguousarray(a) for a in np.split(planes, np.cumsum(bands)[:-1], axis=1)]
        assert [a.shape[1] for a in parts] == list(bands) and np.array_equal(parts[-1], xs[-1])
        m = _net(bands, d, feat, precision)
        m.set_weights_flat(flat)
        y = m.predict(parts)
        if precision == 'fp32':
            assert np.array_equal(_bits(y), _bits(y0)), (bands, int((_bits(y) != _bits(y0)).sum()))
        else:
            _gate_forward(y, y0.astype(np.float64), precision, '%r against (4, 6, 2), F=%d %dx%dx%d' % (bands, feat, n, h, w))


def _zero_body(d, feat):
    """All-zero parameters of d residual blocks: each block is then the identity, exactly, in every precision (t = relu(0) = 0,
    x + 0.1 * 0 = x; the 16-bit modes keep the residual stream as an exact fp32 value)."""
    return np.zeros(d * 2 * (9 * feat * feat + feat), np.float32)


def _poison_workspace(m, n, h, w):
    """The model's workspace of the current stream, every byte 0xFF (NaN as fp32 and as bf16): what a padding lane that the pack
    did not write would hold.  NaN times a zero weight is NaN, which the ReLU (fmaxf(v, 0)) turns into 0 at EVERY pixel of every
    feature channel: nothing like the expected activations.  (A finite poison times a zero weight would vanish;
    tests/guarded.py's rows below run both.)"""
    m._get_workspace(m.workspace_bytes(n, h, w)).fill_(0xFF)


# a network without blocks is fp32 in every precision (the issue's case); one all-zero block puts the first layer's kEpiReluSplit
# epilogue ('bf16') and kEpiRelu + launch_split3_f32 ('bf16x3') between the generic first convolution and the output
FIRST_LAYER_MODES = [('fp32', 0), ('bf16', 0), ('bf16x3', 0), ('bf16', 1), ('bf16x3', 1)]


@pytest.mark.parametrize('precision,d', FIRST_LAYER_MODES)
@pytest.mark.parametrize('bands', [(1, 1), (4, 6, 1)])
def test_padding_lanes_of_the_generic_first_layer_are_zero(bands, precision, d):
    """The model's first layer (launch_pack_inputs into a poisoned workspace + the tile kernel) against dsen2_conv3x3_nhwc on the
    same data packed HERE into 16 channels with zeros, the kernel zero-padded likewise.  The activations cannot be read from a
    model, so the output kernel is a one-hot copy of feature channel f: out = a[f] + skip, one fp32 addition.  Equal bits."""
    feat, n, h, w = 128, 2, 9, 21
    cin, cout = sum(bands), bands[-1]
    (k0, b0), _ = do.split_weights(do.he_uniform_weights(cin, cout, 0, feat, seed=8, bias_scale=0.05), cin, cout, 0, feat)
    dev = [torch.from_numpy(a).to(DEV) for a in do.synthetic_inputs(n, h, w, bands, seed=8)]
    x16 = torch.zeros((n, h, w, 16), device=DEV)
    x16[..., :cin] = torch.cat(dev, dim=1).permute(0, 2, 3, 1)
    k16 = np.zeros((3, 3, 16, feat), np.float32)
    k16[:, :, :cin] = k0
    a = conv3x3_nhwc(x16, k16, b0, epilogue=0)
    assert float(a.min()) >= 0 and float(a.max()) > 0
    m = _net(bands, d, feat, precision)
    for f in (0, 77, feat - 1):
        k1 = np.zeros((3, 3, feat, cout), np.float32)
        k1[1, 1, f, 0] = 1
        m.set_weights_flat(np.concatenate([k0.ravel(), b0, _zero_body(d, feat), k1.ravel(), np.zeros(cout, np.float32)]))
        _poison_workspace(m, n, h, w)
        y = m.forward_device(dev)
        want = (a[..., f] + dev[-1][:, 0]).unsqueeze(1)
        assert torch.equal(y.view(torch.int32), want.view(torch.int32)), (bands, precision, d, f)


def _shifted(x, dy, dx):
    """out[..., y, x] = x[..., y + dy - 1, x + dx - 1], zero outside: what tap (dy, dx) of a 3 x 3 'same' cross-correlation reads."""
    h, w = x.shape[-2:]
    out = torch.zeros_like(x)
    ys = slice(max(0, 1 - dy), min(h, h + 1 - dy))
    xs = slice(max(0, 1 - dx), min(w, w + 1 - dx))
    out[..., ys, xs] = x[..., ys.start + dy - 1:ys.stop + dy - 1, xs.start + dx - 1:xs.stop + dx - 1]
    return out


@pytest.mark.parametrize('precision,d', FIRST_LAYER_MODES)
@pytest.mark.parametrize('bands', [(1, 15), (6, 4), (5, 5, 2)])
def test_delta_kernels_through_the_whole_model(bands, precision, d):
    """First-layer kernel one-hot at (tap, ci, f), output kernel one-hot at (centre, f, co), all biases zero, positive inputs (the
    ReLU is the identity): output channel co = shift(x[ci]) + skip[co] and every other channel = its skip input, bit for bit.
    Inputs are multiples of 1 / 64 below 2 (7 significant bits: exact in bf16, their sums exact in fp32).  Pins the concatenation
    order and every channel offset of pack, first layer and the three output kernels: every (ci, co) pair without blocks, and
    with one all-zero block every ci and every co."""
    feat, n, h, w = 128, 2, 17, 19
    cin, cout = sum(bands), bands[-1]
    rng = np.random.default_rng([cin, cout, len(bands)])
    dev = [torch.from_numpy((rng.integers(1, 128, (n, c, h, w)) / 64.0).astype(np.float32)).to(DEV) for c in bands]
    cat, skip = torch.cat(dev, dim=1), dev[-1]
    if d == 0:
        pairs = [(ci, co) for ci in range(cin) for co in range(cout)]
    else:
        pairs = sorted({(ci, (7 * ci + 3) % cout) for ci in range(cin)} | {((5 * co + 1) % cin, co) for co in range(cout)})
    assert {p[0] for p in pairs} == set(range(cin)) and {p[1] for p in pairs} == set(range(cout))
    m = _net(bands, d, feat, precision)
    flat = np.zeros(m.count_params(), np.float32)
    out_off = 9 * cin * feat + feat + _zero_body(d, feat).size
    assert out_off + 9 * feat * cout + cout == flat.size
    _poison_workspace(m, n, h, w)
    for ci, co in pairs:
        for dy, dx in ((0, 0), (1, 1)):                    # a corner tap and the centre tap
            f = (13 * ci + 29 * co + 3 * dy) % feat
            i0 = ((dy * 3 + dx) * cin + ci) * feat + f
            i1 = out_off + (4 * feat + f) * cout + co
            flat[i0] = flat[i1] = 1
            m.set_weights_flat(flat)
            flat[i0] = flat[i1] = 0
            y = m.forward_device(dev)
            want = skip.clone()
            want[:, co] += _shifted(cat[:, ci], dy, dx)
            assert torch.equal(y.view(torch.int32), want.view(torch.int32)), (bands, precision, d, ci, co, dy, dx, f)


@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('bands', [(1, 15), (2, 7)])
def test_zero_weights_return_the_skip_input_exactly(bands, precision):
    xs = do.synthetic_inputs(3, 9, 21, bands, seed=4)
    m = _net(bands, 2, 128, precision)
    m.set_weights_flat(np.zeros(do.num_params(sum(bands), bands[-1], 2, 128), np.float32))
    assert np.array_equal(_bits(m.predict(xs)), _bits(xs[-1]))


# ---- 4. training -----------------------------------------------------------------------------------------------------------------------------
def _tensor_names(d):
    return ['first.kernel', 'first.bias'] + ['block%d.conv%s.%s' % (l, ab, kb) for l in range(d) for ab in 'AB' for kb in ('kernel', 'bias')] + \
        ['out.kernel', 'out.bias']


def _print_tensors(title, names, errs):
    print(title)
    for name, err in zip(names, errs):
        print('   %-20s rel. L2 error %.2e' % (name, err))


# bands, d, F, n, h, w -> input seed.  As for test_gpu_train.py's MULTI_RUN cases, every float64 ReLU input must lie at least
# MULTI_RUN_MARGIN = 8e-7 from zero (the error of an fp32 forward is ~1e-7; ONE flipped mask moves a bias gradient by ~1e-3 of
# its norm), which is asserted; seed 2 is that file's, 3 where seed 2 has a ReLU input 4.8e-7 from zero (found on the CPU from the
# float64 reference alone).
TRAIN_FP32 = {((1, 1), 1, 128, 2, 16, 16): 2, ((6, 4), 1, 128, 2, 16, 16): 3, ((8, 8), 1, 128, 2, 16, 16): 2,
              ((1, 15), 1, 128, 2, 16, 16): 2, ((5, 5, 2), 1, 128, 2, 16, 16): 2, ((1, 15), 1, 256, 1, 9, 21): 2}


@pytest.mark.parametrize('bands,d,F,n,h,w', list(TRAIN_FP32))
def test_gradients_match_float64_autograd(bands, d, F, n, h, w):
    """tests/test_gpu_train.py::test_gradients_match_float64_autograd, its method and gates: per-tensor relative L2 <= 1e-4, loss
    and mse <= 1e-6 relative.  The first and the output layer's tensors are the ones these cases are about."""
    seed, pre = TRAIN_FP32[(bands, d, F, n, h, w)], []
    m, flat = T32._model(bands, d, F)
    xs = T32._inputs(bands, n, h, w, seed=seed)
    with torch.no_grad():
        out64 = T32._forward64([torch.tensor(a, dtype=torch.float64) for a in xs], T32._unflatten(flat.astype(np.float64), bands, d, F), d, pre)
    margin = min(float(v.abs().min()) for v in pre)
    assert margin >= T32.MULTI_RUN_MARGIN, 'input seed %d: a ReLU input lies %.2e from zero' % (seed, margin)
    y = T32._target(out64.numpy(), seed=3)
    _, g64, loss64, mse64 = T32._grads64(xs, y, flat, bands, d, F)
    m.compile()
    grad, loss2 = T32._gradients(m, T32._dev(xs), T32._dev([y])[0])
    parts = T32._split(grad.cpu().numpy().astype(np.float64), bands, d, F)
    errs = [float(np.linalg.norm(g - ref) / np.linalg.norm(ref)) for g, ref in zip(parts, g64)]
    l2 = loss2.cpu().numpy().astype(np.float64)
    _print_tensors('gradients fp32 %r d=%d F=%d n=%d %dx%d (margin %.1e): loss rel %.1e, mse rel %.1e'
                   % (bands, d, F, n, h, w, margin, abs(l2[0] - loss64) / loss64, abs(l2[1] - mse64) / mse64), _tensor_names(d), errs)
    assert torch.isfinite(grad).all()
    for i, err in enumerate(errs):
        assert err <= 1e-4, (i, err)
    assert abs(l2[0] - loss64) <= 1e-6 * loss64
    assert abs(l2[1] - mse64) <= 1e-6 * mse64


# bf16x3: input seeds for which every float64 ReLU input lies at least T3.MARGIN = 5e-5 from zero, found on the CPU from the
# float64 reference alone (seeds 100 .. of T3._inputs, the first three that hold), as test_gpu_train_bf16x3.py's SAFE_CASES were
SAFE_X3 = [((6, 4), 1, 128, 1, 8, 8, s) for s in (111, 117)] + [((1, 15), 1, 128, 1, 8, 8, s) for s in (109, 121)]


@pytest.mark.parametrize('bands,d,F,n,h,w,seed', SAFE_X3)
def test_bf16x3_gradients_where_no_mask_can_flip(bands, d, F, n, h, w, seed):
    """tests/test_gpu_train_bf16x3.py::test_gradients_match_float64_autograd_where_no_mask_can_flip, its reference and gates."""
    xs, y, g64, loss64, mse64, margin = T3._reference(bands, d, F, n, h, w, seed)
    assert margin >= T3.MARGIN, 'input seed %d: a ReLU input lies %.2e from zero' % (seed, margin)
    m, _ = T3._model(bands, d, F)
    m.compile()
    grad, loss2 = T3._gradients(m, T3._dev(xs), T3._dev([y])[0])
    parts = T3._split(grad.cpu().numpy().astype(np.float64), bands, d, F)
    errs = [T3._rel(g, ref) for g, ref in zip(parts, g64)]
    l2 = loss2.cpu().numpy().astype(np.float64)
    _print_tensors('gradients bf16x3 %r d=%d F=%d n=%d %dx%d seed %d (margin %.1e): loss rel %.1e, mse rel %.1e'
                   % (bands, d, F, n, h, w, seed, margin, abs(l2[0] - loss64) / loss64, abs(l2[1] - mse64) / mse64), _tensor_names(d), errs)
    for i, err in enumerate(errs):
        assert err <= 1e-4, (i, err)
    assert abs(l2[0] - loss64) <= 1e-5 * loss64
    assert abs(l2[1] - mse64) <= 1e-5 * mse64


@pytest.mark.parametrize('bands', [(6, 4), (1, 15)])
def test_mixed_bf16_gradients_against_the_restatement_and_float64(bands):
    """tests/test_gpu_train_amp.py::test_gradients_against_the_restatement_and_float64 itself at these band groups: R.case's
    weights put every ReLU input near +-1 and its targets 0.01 away from the output, and R.check_preconditions asserts both."""
    TA.test_gradients_against_the_restatement_and_float64(bands, 1, 128, 1, 8, 8)


# role, F, the channel count at the edge: ca = 16 with ci real lanes (first layer), cg = 16 with co real lanes (output layer)
WGRAD_EDGES = [('first', F, ci) for F in (128, 256) for ci in (1, 2, 13, 16)] + [('output', F, co) for F in (128, 256) for co in (1, 4, 15, 16)]


@pytest.mark.parametrize('n,h,w', [(2, 11, 13), (1, 1, 1)])
@pytest.mark.parametrize('role,F,edge', WGRAD_EDGES)
def test_wgrad_kernel_at_the_channel_edges(role, F, edge, n, h, w):
    """The exact small-integer method of tests/test_gpu_wgrad_runs.py (integers -3 .. 3: every product and every partial sum in
    any order is exact in fp32), so dW and db are compared bit for bit.  include/dsen2_hip.h (dsen2_conv3x3_wgrad): lanes ci .. of
    dev_a and co .. of dev_g may hold anything; each element of dW takes one lane of each operand.  So the call is repeated with
    those lanes filled with non-zero values, which must not change dW or db."""
    ca, cg, ci, co = (16, F, edge, F) if role == 'first' else (F, 16, F, edge)
    rng = np.random.default_rng([n, h, w, ca, cg, ci, co])
    a = rng.integers(-3, 4, (n, h, w, ca)).astype(np.float32)
    g = rng.integers(-3, 4, (n, h, w, cg)).astype(np.float32)
    ref_w, ref_b = WR._wgrad64(a[..., :ci], g[..., :co])
    assert 9 * n * h * w < 2 ** 24
    zeroed, filled = (a.copy(), g.copy()), (a.copy(), g.copy())
    zeroed[0][..., ci:] = 0
    zeroed[1][..., co:] = 0
    filled[0][..., ci:] = rng.choice([-3.0, -2.0, -1.0, 1.0, 2.0, 3.0], (n, h, w, ca - ci))
    filled[1][..., co:] = rng.choice([-3.0, -2.0, -1.0, 1.0, 2.0, 3.0], (n, h, w, cg - co))
    for lanes, (ah, gh) in (('zero', zeroed), ('non-zero', filled)):
        ops = WR._operands('fp32', ah, gh)
        for scale in (1.0, 0.5):
            dw, db, _ = WR._launch('fp32', ops, (n, h, w, ca, cg), ci, co, scale)
            what = 'wgrad %s layer F=%d n=%d %dx%d %d->%d scale %g, %s padding lanes' % (role, F, n, h, w, ci, co, scale, lanes)
            WR._assert_exact(dw, ref_w * scale, what + ' dW')
            WR._assert_exact(db, ref_b * scale, what + ' db')


@pytest.mark.parametrize('precision', ['fp32', 'bf16x3'])
def test_train_on_batch_of_a_1_15_model_is_gradients_nadam_repack(precision):
    """tests/test_gpu_train.py::test_train_on_batch_is_gradients_nadam_repack at 16 input and 15 output channels: byte for byte."""
    bands, d, F = (1, 15), 1, 128
    xs = T32._inputs(bands, 2, 16, 16, seed=12)
    y = np.random.default_rng(13).uniform(0, 0.5, (2, 15, 16, 16)).astype(np.float32)
    a, flat = T32._model(bands, d, F, precision=precision)
    b, _ = T32._model(bands, d, F, precision=precision)
    a.compile(training.Nadam(lr=1e-3))
    b.compile(training.Nadam(lr=1e-3))
    count = b.count_params()
    pb = torch.from_numpy(flat.copy()).to(DEV)
    mb = torch.zeros(count, device=DEV)
    vb = torch.zeros(count, device=DEV)
    opt = training.Nadam(lr=1e-3)
    xs_d, y_d = T32._dev(xs), T32._dev([y])[0]
    for _ in range(2):
        la = a.train_on_batch(xs, y)
        grad, loss2 = T32._gradients(b, xs_d, y_d)
        s = opt.next_step()
        with torch.cuda.device(DEV):
            _lib.call('dsen2_nadam_step', _ptr(pb), _ptr(grad), _ptr(mb), _ptr(vb), count, s['lr'], s['b1'], s['b2'], s['eps'],
                      s['mc_t'], s['mc_t1'], s['ms_new'], s['ms_next'], s['b2_pow_t'], _stream_ptr(DEV))
        b.set_weights_device(pb)
        assert la == [float(x) for x in loss2.cpu().numpy()]
    stepped = a.get_weights_flat()
    assert np.array_equal(_bits(stepped), _bits(pb.cpu().numpy())) and not np.array_equal(stepped, flat)
    fresh, _ = T32._model(bands, d, F, precision=precision)
    fresh.set_weights_flat(stepped)
    assert np.array_equal(_bits(a.predict(xs)), _bits(fresh.predict(xs)))


@pytest.mark.parametrize('precision', ['fp32', 'bf16x3'])
@pytest.mark.parametrize('bands', [(1, 1), (1, 15)])
def test_flat_weights_survive_the_device_repack(bands, precision):
    """dsen2_model_get_weights after dsen2_model_set_weights_device returns the same floats, and the repacked model is the
    host-packed one: the gather maps of the first and the output layer at 2 and 16 input, 1 and 15 output channels."""
    d, F = 1, 128
    m, _ = T32._model(bands, d, F, precision=precision)
    new = weights.random_he_uniform(sum(bands), bands[-1], d, F, seed=9, bias_scale=0.1)
    m.set_weights_device(torch.from_numpy(new).to(DEV))
    back = torch.empty(m.count_params(), dtype=torch.float32, device=DEV)
    with torch.cuda.device(DEV):
        _lib.call('dsen2_model_get_weights', m._handle, _ptr(back), _stream_ptr(DEV))
    assert np.array_equal(_bits(back.cpu().numpy()), _bits(new))
    fresh, _ = T32._model(bands, d, F, precision=precision)
    fresh.set_weights_flat(new)
    xs_d = T32._dev(T32._inputs(bands, 2, 9, 21, seed=7))
    assert torch.equal(m.forward_device(xs_d), fresh.forward_device(xs_d))


# ---- 5. memory contract --------------------------------------------------------------------------------------------------------------------
# The NHWC16 pack with 14 padding lanes over poisoned scratch, and 15 output channels behind a 32-wide tile: guards intact, inputs
# unchanged, the same bits over zeroed, 0xFF and 0x7F surroundings, the workspace exactly the size function's byte count.
@pytest.mark.parametrize('n,h,w', [(2, 5, 7), (1, 1, 1)])
@pytest.mark.parametrize('bands', [(1, 1), (1, 15)])
@pytest.mark.parametrize('precision', PRECISIONS)
def test_memory_contract_of_forward(precision, bands, n, h, w):
    m = MC._model(bands, 1, 128, precision)
    MC._forward_row('forward %s %r d=1 F=128 %dx%dx%d' % (precision, bands, n, h, w), m, MC._inputs(bands, n, h, w, 1), n, h, w)


@pytest.mark.parametrize('n,h,w', [(2, 5, 7), (1, 1, 1)])
@pytest.mark.parametrize('bands', [(1, 1), (1, 15)])
@pytest.mark.parametrize('mode', list(MC.TRAIN_MODES))
def test_memory_contract_of_gradients(mode, bands, n, h, w):
    MC.test_gradients(mode, bands, 1, 128, n, h, w, True, True)


# ---- 6. the boundary --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c10,c20,c60,feat', [(0, 6, 0, 128), (4, 0, 0, 128), (4, 6, -1, 128), (1, 16, 0, 128), (8, 8, 1, 128), (15, 1, 1, 128),
                                              (4, 6, 0, 64), (4, 6, 0, 384)])
def test_model_create_refuses(c10, c20, c60, feat):
    lib = _lib.load()
    handle = ctypes.c_void_p(1)
    with torch.cuda.device(DEV):
        rc = lib.dsen2_model_create(ctypes.byref(handle), c10, c20, c60, 1, feat, 0)
    assert rc == _lib.ERR_INVALID and len(lib.dsen2_last_error()) > 0 and not handle.value
    if c60 >= 0:
        bands = (c10, c20) + ((c60,) if c60 else ())
        with pytest.raises(_lib.DSen2Error) as e:
            s2model(_shape(bands), num_layers=1, feature_size=feat, device=DEV)
        assert e.value.code == _lib.ERR_INVALID


@pytest.mark.parametrize('bands', list(GROUPS))
def test_model_create_accepts(bands):
    m = _net(bands, 1, 128, 'fp32')
    cin, cout = sum(bands), bands[-1]
    assert (m.cin, m.cout) == (cin, cout) and m.count_params() == do.num_params(cin, cout, 1, 128)


@pytest.mark.parametrize('precision', [1, 2])
@pytest.mark.parametrize('bands', [(6, 4), (4, 6, 1)])
def test_first_planes_entry_refuses_other_band_groups(bands, precision):
    xs = [torch.zeros((1, c, 8, 8), device=DEV) for c in bands]
    with pytest.raises(_lib.DSen2Error) as e:
        conv3x3_first_planes(xs, np.zeros((3, 3, sum(bands), 128), np.float32), np.zeros(128, np.float32), precision)
    assert e.value.code == _lib.ERR_INVALID and 'band groups' in str(e.value)
