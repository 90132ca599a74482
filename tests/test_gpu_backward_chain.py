"""dsen2_model_gradients against the same step strung together from the kernel-level entry points: the same BITS, in every step
format (fp32, bf16x3, and an fp32 model under compile(mixed_precision='bf16')).

The forward is pinned this way already (test_precision1/2_forward_is_the_chain_of_its_kernel_level_operations,
test_first_layer_without_padding_mfmas_gives_the_same_bits).  The backward pass was checked against float64 autograd at a
per-tensor relative L2 error of 1e-4 only — about a thousand fp32 roundings, room enough for a few wrong pixels, a small share of
wrong ReLU masks, or a stale dgrad weight buffer.  Here one helper per format follows the file comment of
dsen2_amd/csrc/capi_train.hip line by line, using only

  conv3x3_nhwc, conv3x3_body_bf16x3, conv3x3_body_bf16, conv3x3_first_planes, split_f32 / join_f32, split3_f32 / join3_f32,
  dsen2_conv3x3_wgrad, conv3x3_wgrad_bf16x3, conv3x3_wgrad_bf16, dsen2_loss_grad         (each tested on its own),
  tests/dgrad_restatement.py (the flipped kernels and the two mask-and-round definitions; tests/test_dgrad_host.py proves them
  against torch) and torch.where / zeros for the fp32 masks and the memsets,

and returns (out, grad, loss2), which must be torch.equal to what gradients_device writes.  What that reaches and nothing else
does: the dgrad weight buffers behind the gather maps (flip, transposition, the per-layer stride, the bf16 digit encoding), the
16 -> F residual convolution, where the 0.1 goes, the zeroed buffers, the splits and joins of g round the block loop, one
weight-gradient workspace for three layer kinds, the loss settings of the owner reaching the companion's step — and whether
the dgrad weights follow the weights (the last test).

Where the step does what no public entry does, the helper says so:
  * the training step calls its fp32 dgrad convolutions in place; DSen2Net.conv3x3_nhwc always allocates its output, so the
    helpers call the same C entry (dsen2_conv3x3_nhwc) through test_gpu_dgrad.conv_into with out = aux;
  * a model of the bands 4 + 6 (+ 2) runs its fp32 first convolution on the direct kernel; the helper runs conv3x3_nhwc on the
    16 padded channels, which test_first_layer_without_padding_mfmas_gives_the_same_bits shows to be the same bits;
  * a network without residual blocks is planned in fp32 in every precision and trains in the fp32 format, so the d = 0 case of
    every format is the fp32 helper;
  * mixed precision with a band grouping other than 4 + 6 (+ 2): the companion's generic first convolution writes the stream's two
    planes itself (kEpiReluSplit), for which there is no kernel-level entry; that case is left out of the mixed format only."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import dgrad_restatement as R  # noqa: E402
from test_gpu_dgrad import conv_into  # noqa: E402
from dsen2_amd import _lib, losses, training  # noqa: E402
from dsen2_amd.DSen2Net import (_ptr, _stream_ptr, conv3x3_body_bf16, conv3x3_body_bf16x3, conv3x3_first_planes, conv3x3_nhwc,  # noqa: E402
                                conv3x3_wgrad_bf16, conv3x3_wgrad_bf16x3, from_blocked, join3_f32, join_f32, s2model, split3_f32,
                                split_f32, to_blocked)
from oracle import dsen2_oracle as do  # noqa: E402      weights and their layout only

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda', 0)
SENTINEL2 = ((4, 6), (4, 6, 2))


# ---- pieces shared by the three helpers ----------------------------------------------------------------------------------------
def _offsets(bands, d, F):
    """[(offset of the kernel, offset of the bias, ci, co)] of every layer in the keras-flat vector."""
    out, off = [], 0
    for ci, co in do.layer_shapes(sum(bands), bands[-1], d, F):
        out.append((off, off + 9 * ci * co, ci, co))
        off += 9 * ci * co + co
    return out


def _wgrad32(grad, where, a, g, scale):
    """dsen2_conv3x3_wgrad straight into the layer's place in the flat gradient, as the step writes it."""
    off, boff, ci, co = where
    n, h, w, ca = a.shape
    cg = g.shape[3]
    assert a.is_contiguous() and g.is_contiguous() and tuple(g.shape[:3]) == (n, h, w)
    with torch.cuda.device(DEV):
        _lib.call('dsen2_conv3x3_wgrad', _ptr(a), _ptr(g), _ptr(grad[off:]), _ptr(grad[boff:]), n, h, w, ca, cg, ci, co, float(scale),
                  _stream_ptr(DEV))


def _put(grad, where, dw, db):
    off, boff, ci, co = where
    grad[off:boff] = dw.reshape(-1)
    grad[boff:boff + co] = db


def _pack16(xs):
    """launch_pack_inputs: the concatenated inputs as NHWC16, the lanes above the real channels zero."""
    n, _, h, w = xs[0].shape
    cin = sum(x.shape[1] for x in xs)
    x16 = torch.zeros((n, h, w, 16), dtype=torch.float32, device=DEV)
    x16[..., :cin] = torch.cat(xs, dim=1).permute(0, 2, 3, 1)
    return x16


def _first_fp32(x16, layers, F):
    """The fp32 first convolution on the 16 padded channels (the model's own bits: tests/test_gpu_forward.py)."""
    k0, b0 = layers[0]
    k16 = np.zeros((3, 3, 16, F), np.float32)
    k16[:, :, :k0.shape[2]] = k0
    return conv3x3_nhwc(x16, k16, b0, epilogue=0)


def _loss_and_output_layer(xd, xs, y, setting, layers, offs, grad, F):
    """Output convolution, loss, the output layer's weight gradient, and its input gradient onto a zeroed g: fp32 kernels on fp32
    tensors in every format.  Returns (out, loss2, g)."""
    n, h, w, _ = xd.shape
    ko, bo = layers[-1]
    cout = ko.shape[3]
    out = conv3x3_nhwc(xd, ko, bo, epilogue=2, aux=xs[-1])
    gpad = torch.full((n, h, w, 16), float('nan'), dtype=torch.float32, device=DEV)     # the kernel owes all 16 lanes
    loss2 = torch.empty(2, dtype=torch.float32, device=DEV)
    kind, param, mask = setting
    with torch.cuda.device(DEV):
        _lib.call('dsen2_loss_grad', _ptr(out), _ptr(y), n, cout, h, w, int(kind), float(param), int(mask), _ptr(gpad), _ptr(loss2),
                  _stream_ptr(DEV))
    _wgrad32(grad, offs[-1], xd, gpad, 1.0)
    g = torch.zeros((n, h, w, F), dtype=torch.float32, device=DEV)
    conv_into(gpad, R.flip_hwio(ko, pad_in=16), np.zeros(F, np.float32), 1, g, g, 1.0)
    return out, loss2, g


def _first_layer_gradient(g, x0f, x16, offs, grad):
    """[x_0 > 0] * g, then the first layer's weight gradient on the NHWC16 input (fp32 kernels in every format)."""
    g = torch.where(x0f > 0, g, torch.zeros_like(g))
    _wgrad32(grad, offs[0], x16, g, 1.0)


def _new_grad(bands, d, F):
    return torch.full((do.num_params(sum(bands), bands[-1], d, F),), float('nan'), dtype=torch.float32, device=DEV)


# ---- the three step formats ------------------------------------------------------------------------------------------------------
def chain_fp32(flat, xs, y, setting, bands, d, F):
    """planes 0: fp32 tensors, g updated in place, du zeroed for every block."""
    layers, offs, grad = do.split_weights(np.asarray(flat), sum(bands), bands[-1], d, F), _offsets(bands, d, F), _new_grad(bands, d, F)
    zero = np.zeros(F, np.float32)
    x16 = _pack16(xs)
    x, t = [_first_fp32(x16, layers, F)], []
    for l in range(1, d + 1):
        (ka, ba), (kb, bb) = layers[2 * l - 1], layers[2 * l]
        t.append(conv3x3_nhwc(x[-1], ka, ba, epilogue=0))
        x.append(conv3x3_nhwc(t[-1], kb, bb, epilogue=1, aux=x[-1], res_scale=0.1))
    out, loss2, g = _loss_and_output_layer(x[d], xs, y, setting, layers, offs, grad, F)
    for l in range(d, 0, -1):
        (ka, _), (kb, _) = layers[2 * l - 1], layers[2 * l]
        _wgrad32(grad, offs[2 * l], t[l - 1], g, 0.1)                                    # dWB = 0.1 * wgrad(t_l, g)
        du = torch.zeros_like(g)
        conv_into(g, R.flip_hwio(kb), zero, 1, du, du, 0.1)                              # 0 + 0.1 * dgradB(g)
        du = torch.where(t[l - 1] > 0, du, torch.zeros_like(du))                         # the ReLU mask of t_l
        _wgrad32(grad, offs[2 * l - 1], x[l - 1], du, 1.0)                               # dWA = wgrad(x_{l-1}, du)
        conv_into(du, R.flip_hwio(ka), zero, 1, g, g, 1.0)                               # g <- g + dgradA(du)
    _first_layer_gradient(g, x[0], x16, offs, grad)
    return out, grad, loss2


def chain_bf16x3(flat, xs, y, setting, bands, d, F):
    """planes 2: the forward's bf16x3 kernels on planes; g as a precision-2 stream (hx = hi | xl, lo16) round the block loop."""
    if d == 0:
        return chain_fp32(flat, xs, y, setting, bands, d, F)
    layers, offs, grad = do.split_weights(np.asarray(flat), sum(bands), bands[-1], d, F), _offsets(bands, d, F), _new_grad(bands, d, F)
    zero = np.zeros(F, np.float32)
    x16 = _pack16(xs)
    if tuple(bands) in SENTINEL2:
        hx, lo = conv3x3_first_planes(xs, layers[0][0], layers[0][1], precision=2)
    else:                                     # the generic first layer: fp32, then launch_split3_f32
        hx, lo = split3_f32(_first_fp32(x16, layers, F))
    x0f = join3_f32(hx, lo)
    xkeep, tkeep = [], []
    for l in range(1, d + 1):
        (ka, ba), (kb, bb) = layers[2 * l - 1], layers[2 * l]
        xkeep.append(hx.clone())
        tkeep.append(conv3x3_body_bf16x3(hx, ka, ba, epilogue=0))
        if l < d:
            conv3x3_body_bf16x3(tkeep[-1], kb, bb, epilogue=1, res_hx=hx, res_lo=lo, res_scale=0.1)
        else:
            xd = conv3x3_body_bf16x3(tkeep[-1], kb, bb, epilogue=3, res_hx=hx, res_lo=lo, res_scale=0.1)
    out, loss2, g = _loss_and_output_layer(xd, xs, y, setting, layers, offs, grad, F)
    gs0, gs1 = split3_f32(g)
    zs0, zs1 = torch.zeros_like(gs0), torch.zeros_like(gs1)
    for l in range(d, 0, -1):
        (ka, _), (kb, _) = layers[2 * l - 1], layers[2 * l]
        _put(grad, offs[2 * l], *conv3x3_wgrad_bf16x3(tkeep[l - 1], gs0, scale=0.1))
        v = conv3x3_body_bf16x3(gs0, R.flip_hwio(kb), zero, epilogue=3, res_hx=zs0, res_lo=zs1, res_scale=0.1)
        t_hi, t_lo = R.planes_to_values(tkeep[l - 1].cpu().numpy())
        du = torch.from_numpy(R.values_to_planes(*R.mask_split3(v.cpu().numpy(), t_hi, t_lo))).to(DEV)
        _put(grad, offs[2 * l - 1], *conv3x3_wgrad_bf16x3(xkeep[l - 1], du, scale=1.0))
        conv3x3_body_bf16x3(du, R.flip_hwio(ka), zero, epilogue=1, res_hx=gs0, res_lo=gs1, res_scale=1.0)
    g = join3_f32(gs0, gs1)
    assert not zs0.any() and not zs1.any(), 'the fp32 epilogue wrote the zero stream'
    _first_layer_gradient(g, x0f, x16, offs, grad)
    return out, grad, loss2


def chain_amp(flat, xs, y, setting, bands, d, F):
    """planes 1: the one-plane analogue on a precision-1 plan of the same weights; the first and output layers' gradients on fp32
    kernels.  g is a precision-1 stream (hi, lo) = exact fp32; t_l bf16; du = bf16_rne of the masked value."""
    if d == 0:
        return chain_fp32(flat, xs, y, setting, bands, d, F)
    assert tuple(bands) in SENTINEL2, 'no kernel-level entry for the generic first convolution of a precision-1 plan'
    layers, offs, grad = do.split_weights(np.asarray(flat), sum(bands), bands[-1], d, F), _offsets(bands, d, F), _new_grad(bands, d, F)
    zero = np.zeros(F, np.float32)
    bf16 = torch.bfloat16
    x16 = _pack16(xs)
    hi, lo = conv3x3_first_planes(xs, layers[0][0], layers[0][1], precision=1)
    x0f = join_f32(hi, lo)
    xkeep, tkeep = [], []
    for l in range(1, d + 1):
        (ka, ba), (kb, bb) = layers[2 * l - 1], layers[2 * l]
        xkeep.append(hi.clone())
        tkeep.append(conv3x3_body_bf16(from_blocked(hi.view(bf16)), ka, ba, epilogue=0))              # bf16 NHWC
        if l < d:
            conv3x3_body_bf16(tkeep[-1], kb, bb, epilogue=1, res_hi=hi, res_lo=lo, res_scale=0.1)
        else:
            xd = conv3x3_body_bf16(tkeep[-1], kb, bb, epilogue=3, res_hi=hi, res_lo=lo, res_scale=0.1)
    out, loss2, g = _loss_and_output_layer(xd, xs, y, setting, layers, offs, grad, F)
    gs0, gs1 = split_f32(g)
    zs0, zs1 = torch.zeros_like(gs0), torch.zeros_like(gs1)
    for l in range(d, 0, -1):
        (ka, _), (kb, _) = layers[2 * l - 1], layers[2 * l]
        _put(grad, offs[2 * l], *conv3x3_wgrad_bf16(to_blocked(tkeep[l - 1]), gs0, scale=0.1))
        v = conv3x3_body_bf16(from_blocked(gs0.view(bf16)), R.flip_hwio(kb), zero, epilogue=3, res_hi=zs0, res_lo=zs1, res_scale=0.1)
        bits = R.mask_round16(v.cpu().numpy(), tkeep[l - 1].float().cpu().numpy())
        du = torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).to(DEV).view(bf16)            # bf16 NHWC
        _put(grad, offs[2 * l - 1], *conv3x3_wgrad_bf16(xkeep[l - 1], to_blocked(du), scale=1.0))
        conv3x3_body_bf16(du, R.flip_hwio(ka), zero, epilogue=1, res_hi=gs0, res_lo=gs1, res_scale=1.0)
    g = join_f32(gs0, gs1)
    assert not zs0.any() and not zs1.any(), 'the fp32 epilogue wrote the zero stream'
    _first_layer_gradient(g, x0f, x16, offs, grad)
    return out, grad, loss2


# format -> (model precision, compile(mixed_precision=), helper)
FORMATS = {'fp32': ('fp32', None, chain_fp32), 'bf16x3': ('bf16x3', None, chain_bf16x3), 'amp': ('fp32', 'bf16', chain_amp)}


# ---- cases ------------------------------------------------------------------------------------------------------------------------
def _weights(bands, d, F, seed, bias_scale=0.05):
    return do.he_uniform_weights(sum(bands), bands[-1], d, F, seed=seed, bias_scale=bias_scale)


def _data(bands, n, h, w, seed, blank=False):
    """Inputs and a target in the normalised reflectance range; blank: a rectangle of no-data pixels (target exactly 0 in every
    band) and a pixel that is 0 in some bands only, which is data."""
    rng = np.random.default_rng(seed)
    xs = [rng.uniform(0.0, 0.5, (n, c, h, w)).astype(np.float32) for c in bands]
    y = rng.uniform(0.0, 0.5, (n, bands[-1], h, w)).astype(np.float32)
    if blank:
        y[:, :, :h // 2, :w // 3] = 0.0
        y[0, ::2, h - 1, w - 1] = 0.0
    return [torch.from_numpy(a).to(DEV) for a in xs], torch.from_numpy(y).to(DEV), xs, y


def _model(fmt, bands, d, F, optimizer='nadam', **loss):
    precision, mixed, _ = FORMATS[fmt]
    m = s2model(tuple((c, None, None) for c in bands), num_layers=d, feature_size=F, device=DEV, precision=precision)
    m.compile(optimizer, mixed_precision=mixed, **loss)
    return m


def _step(m, xs, y):
    grad = torch.full((m.count_params(),), float('nan'), dtype=torch.float32, device=DEV)
    loss2 = torch.full((2,), float('nan'), dtype=torch.float32, device=DEV)
    out = m.gradients_device(xs, y, grad, loss2, out=torch.empty_like(y))
    torch.cuda.synchronize()
    return out, grad, loss2


def _names(d):
    return ['the first layer'] + [s % l for l in range(1, d + 1) for s in ('conv-A of block %d', 'conv-B of block %d')] + ['the output layer']


def _assert_same(step, chain, bands, d, F, what):
    """out, loss2, then the flat gradient tensor by tensor in the order the step forms it — the output layer first, the first layer
    last — so that the message names the first link that differs."""
    assert torch.equal(step[0], chain[0]), '%s: the forward output differs' % what
    assert torch.equal(step[2], chain[2]), '%s: loss2 differs: %r / %r' % (what, step[2].tolist(), chain[2].tolist())
    assert not torch.isnan(step[1]).any() and not torch.isnan(chain[1]).any(), '%s: a gradient was not written' % what
    names = _names(d)
    for li in reversed(range(len(names))):
        off, boff, ci, co = _offsets(bands, d, F)[li]
        for part, a, b in (('kernel', off, boff), ('bias', boff, boff + co)):
            s, c = step[1][a:b], chain[1][a:b]
            if not torch.equal(s, c):
                bad = int((s != c).sum())
                raise AssertionError('%s: the %s gradient of %s is the first to differ, %d of %d values, max |diff| %.3e'
                                     % (what, part, names[li], bad, s.numel(), float((s - c).abs().max())))
    assert torch.equal(step[1], chain[1])


# bands, d, F, n, h, w
CASES = [((4, 6), 2, 128, 2, 16, 16),        # one tile per image, two blocks: the per-layer stride of the dgrad buffer
         ((4, 6, 2), 1, 128, 1, 21, 37),     # ragged tiles, 12 input and 2 output channels
         ((4, 6), 1, 256, 2, 19, 16),        # two output slabs
         ((4, 6), 0, 128, 1, 7, 31)]         # no block: output dgrad, mask, first wgrad only
# a grouping whose first layer takes the generic path (launch_pack_inputs + the tile kernel) and whose 15 output channels fill
# 15 of gpad's 16 lanes (tests/test_gpu_band_groups.py)
GENERIC_FIRST = ((1, 15), 1, 128, 2, 9, 21)
PER_FORMAT = [(f,) + c for f in FORMATS for c in CASES] + [(f,) + GENERIC_FIRST for f in ('fp32', 'bf16x3')]


@pytest.mark.parametrize('fmt,bands,d,F,n,h,w', PER_FORMAT)
def test_the_step_is_the_chain_of_its_kernel_level_operations(fmt, bands, d, F, n, h, w):
    """The default loss (MAE, no mask).  (The generic-first-layer grouping is left out of the mixed format: see the file comment.)"""
    flat = _weights(bands, d, F, seed=d + F)
    xs, y, _, _ = _data(bands, n, h, w, seed=h + w)
    m = _model(fmt, bands, d, F)
    m.set_weights_flat(flat)
    step = _step(m, xs, y)
    chain = FORMATS[fmt][2](flat, xs, y, losses.DEFAULT, bands, d, F)
    _assert_same(step, chain, bands, d, F, '%s %r d=%d F=%d %dx%dx%d' % (fmt, bands, d, F, n, h, w))
    assert float(step[2][0]) > 0 and bool((step[1] != 0).any())


@pytest.mark.parametrize('fmt', list(FORMATS))
def test_the_step_follows_the_compiled_loss_and_mask(fmt):
    """loss='mse' with the no-data mask on the first case.  Under mixed precision the settings live on the owner and the step runs
    on its companion: the chain, which hands them to dsen2_loss_grad itself, shows that they arrive."""
    bands, d, F, n, h, w = CASES[0]
    flat = _weights(bands, d, F, seed=3)
    xs, y, _, _ = _data(bands, n, h, w, seed=11, blank=True)
    m = _model(fmt, bands, d, F, loss='mse', mask_nodata=True)
    m.set_weights_flat(flat)
    step = _step(m, xs, y)
    setting = losses.parse('mse', None, True)
    assert setting != losses.DEFAULT
    chain = FORMATS[fmt][2](flat, xs, y, setting, bands, d, F)
    _assert_same(step, chain, bands, d, F, '%s mse, masked' % fmt)
    default = FORMATS[fmt][2](flat, xs, y, losses.DEFAULT, bands, d, F)
    assert not torch.equal(default[1], step[1]) and not torch.equal(default[2], step[2])      # the settings matter on this data


def _every_layer_differs(a, b, bands, d, F):
    return all((a[off:boff] != b[off:boff]).any() and (a[boff:boff + co] != b[boff:boff + co]).any() for off, boff, _, co in _offsets(bands, d, F))


@pytest.mark.parametrize('fmt', list(FORMATS))
def test_the_dgrad_weights_follow_the_weights(fmt):
    """A stale dgrad buffer still trains, on the wrong gradient.  After each way the weights can change, the step must be the chain
    on get_weights_flat() — and must NOT be the chain on the weights before the change, or the check could not fail:
     1. set_weights_flat on a freshly compiled model (dsen2_model_load_weights, then the training state built from it);
     2. one train_on_batch (Nadam, then repack_from_master on the device);
     3. set_weights_flat on that model (dsen2_model_load_weights with a training state: train_state_after_load);
     4. set_weights_device (dsen2_model_set_weights_device)."""
    bands, d, F, n, h, w = CASES[0]
    helper = FORMATS[fmt][2]
    xs, y, xs_host, y_host = _data(bands, n, h, w, seed=21)
    m = _model(fmt, bands, d, F, optimizer=training.Nadam(lr=1e-3))

    def check(what, old):
        now = m.get_weights_flat()
        assert _every_layer_differs(now, old, bands, d, F), '%s: a layer kept its weights' % what
        step = _step(m, xs, y)
        _assert_same(step, helper(now, xs, y, losses.DEFAULT, bands, d, F), bands, d, F, '%s after %s' % (fmt, what))
        stale = helper(old, xs, y, losses.DEFAULT, bands, d, F)
        assert not torch.equal(stale[1], step[1]), '%s: the chain on the old weights gives the same gradient' % what
        return now

    w1 = _weights(bands, d, F, seed=1)
    m.set_weights_flat(w1)
    np.testing.assert_array_equal(m.get_weights_flat(), w1)
    w1 = check('set_weights_flat on a fresh model', _weights(bands, d, F, seed=2))
    m.train_on_batch(xs_host, y_host)
    w2 = check('train_on_batch', w1)
    w3 = _weights(bands, d, F, seed=7, bias_scale=0.1)
    m.set_weights_flat(w3)
    np.testing.assert_array_equal(m.get_weights_flat(), w3)
    check('set_weights_flat on a stepped model', w2)
    w4 = _weights(bands, d, F, seed=8, bias_scale=0.02)
    m.set_weights_device(torch.from_numpy(w4).to(DEV))
    np.testing.assert_array_equal(m.get_weights_flat(), w4)
    check('set_weights_device', w3)
