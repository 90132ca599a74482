"""The convolution the training step runs and the forward never does: the output layer's input gradient (ConvRole::DgradOutput),
16 -> F on the tile kernel with kc = 16 and the RESIDUAL epilogue, called as the step calls it —
conv3x3_nhwc(g16, W', 0, epilogue=1, aux=..., res_scale=1.0) with g16 = dL/dout in NHWC16 and W' = flip_hwio(W_out, pad_in=16).
(The forward's 16 -> F instance has the ReLU epilogue; every residual test of tests/test_gpu_conv.py is F -> F.)

 1. against the float64 C oracle, at that file's gate for the same kernel family and contraction length 9 * 16
    (RMS_GATE['relu'][16], MAX_GATE_FACTOR, imported): the residual epilogue adds one rounding of a sum of rms ~1.7, ~1e-7, inside
    the gate's margin over the 2.1e-7 recorded there.  `python -m pytest tests/test_gpu_dgrad.py -m gpu -s` prints every figure
    (measured on an MI355X: rmse 2.7e-8 .. 3.0e-7 and max 1.1e-7 .. 3.1e-6 over the 40 cases, against gates of 2e-6 and 2.4e-5);
 2. in place (aux is out), as the step runs it: the bits of the out-of-place call;
 3. known answers: a one-hot W' copies one shifted gradient lane into one output channel bit for bit, on top of aux;
 4. dsen2_conv3x3_nhwc_ref on the same cases: the same bits."""
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

from test_gpu_conv import MAX_GATE_FACTOR, RMS_GATE  # noqa: E402      the gates of the same kernel family: imported, not copied
from oracle import c_oracle  # noqa: E402                              checker only
from oracle import dsen2_oracle as do  # noqa: E402

pytestmark = pytest.mark.gpu

# one pixel; one full tile per image; ragged tiles in both directions; a ragged column of tiles over three images
SHAPES = [(1, 1, 1), (2, 16, 16), (1, 21, 37), (3, 5, 70)]
# real gradient channels: the Sentinel-2 models' 6 and 2, the ends of what a model may have (1, 15), and all 16 lanes
REAL = [6, 2, 1, 15, 16]
CASES = [(feat, real) + nhw for feat in (128, 256) for nhw in SHAPES for real in REAL]


def conv_into(x, kernel_hwio, bias, epilogue, aux, out, res_scale, ref=False):
    """dsen2_conv3x3_nhwc(_ref) writing into a tensor the caller chooses (DSen2Net.conv3x3_nhwc always allocates its output):
    out may be aux itself, which is how the training step calls its dgrad convolutions."""
    from dsen2_amd import _lib
    n, h, w, cin = x.shape
    kernel_hwio = np.ascontiguousarray(kernel_hwio, np.float32)
    bias = np.ascontiguousarray(bias, np.float32)
    cout = kernel_hwio.shape[3]
    assert kernel_hwio.shape == (3, 3, cin, cout) and bias.shape == (cout,)
    for t in (x, aux, out):
        assert t.is_contiguous() and t.dtype == torch.float32 and t.is_cuda
    assert tuple(out.shape) == (n, h, w, cout) and tuple(aux.shape) == (n, h, w, cout)
    with torch.cuda.device(x.device):
        _lib.call('dsen2_conv3x3_nhwc_ref' if ref else 'dsen2_conv3x3_nhwc', ctypes.c_void_p(x.data_ptr()),
                  kernel_hwio.ctypes.data_as(_lib.c_float_p), bias.ctypes.data_as(_lib.c_float_p), ctypes.c_void_p(aux.data_ptr()),
                  ctypes.c_void_p(out.data_ptr()), n, h, w, cin, cout, int(epilogue), float(res_scale),
                  ctypes.c_void_p(torch.cuda.current_stream(x.device).cuda_stream))
    return out


@functools.lru_cache(maxsize=None)
def _case(feat, real, n, h, w):
    """(g16 NCHW, W' HWIO, aux NCHW, the float64 oracle's result, the kernel's result on the device): computed once, never
    modified.  Operands as in tests/test_gpu_conv.py: inputs N(0, 1), a he-normal kernel for the fan 9 * 16, aux N(0, 1); the
    lanes above the real count are zero in g16 and in W', as dL/dout's padding and flip_hwio(pad_in=16)'s are."""
    from dsen2_amd.DSen2Net import conv3x3_nhwc
    rng = np.random.default_rng(1000 * feat + 100 * real + 10 * h + w)
    g = rng.standard_normal((n, 16, h, w)).astype(np.float32)
    k = (rng.standard_normal((3, 3, 16, feat)) * np.sqrt(2.0 / (9 * 16))).astype(np.float32)
    aux = rng.standard_normal((n, feat, h, w)).astype(np.float32)
    g[:, real:] = 0
    k[:, :, real:] = 0
    ref = c_oracle.conv3x3(g, k, np.zeros(feat, np.float32), relu=False) + aux
    for a in (g, k, aux, ref):
        a.setflags(write=False)
    y = conv3x3_nhwc(_nhwc(g), k, np.zeros(feat, np.float32), epilogue=1, aux=_nhwc(aux), res_scale=1.0)
    return g, k, aux, ref, y


def _nhwc(x_nchw):
    return torch.from_numpy(np.array(np.asarray(x_nchw).transpose(0, 2, 3, 1), order='C')).cuda()      # (always a writable copy)


@pytest.mark.parametrize('feat,real,n,h,w', CASES)
def test_dgrad_output_matches_the_oracle(feat, real, n, h, w):
    g, k, aux, ref, y = _case(feat, real, n, h, w)
    y = y.cpu().numpy().transpose(0, 3, 1, 2)
    e, mx = do.rmse(y, ref), float(np.abs(y - ref).max())
    gate = RMS_GATE['relu'][16]
    print('dgrad-out F %3d real %2d %dx%dx%d: rmse %.3e (gate %.1e)  max %.3e (gate %.1e)  output rms %.3f'
          % (feat, real, n, h, w, e, gate, mx, MAX_GATE_FACTOR * gate, float(np.sqrt(np.mean(ref * ref)))))
    assert y.shape == ref.shape and np.isfinite(y).all()
    assert e < gate, (feat, real, n, h, w, e)
    assert mx < MAX_GATE_FACTOR * gate, (feat, real, n, h, w, mx)


@pytest.mark.parametrize('feat,real,n,h,w', CASES)
def test_dgrad_output_in_place_gives_the_same_bits(feat, real, n, h, w):
    """aux is out: every workgroup reads aux and writes out at its own pixels only, so nothing may change."""
    g, k, aux, _, y = _case(feat, real, n, h, w)
    buf = _nhwc(aux)
    conv_into(_nhwc(g), k, np.zeros(feat, np.float32), 1, buf, buf, 1.0)
    assert torch.equal(buf, y)


@pytest.mark.parametrize('feat,real,n,h,w', CASES)
def test_dgrad_output_reference_entry_gives_the_same_bits(feat, real, n, h, w):
    """dsen2_conv3x3_nhwc_ref accepts this shape and epilogue (its plan for a 16 -> F residual convolution is the tile kernel too,
    whatever the tuning: the check is that the two entries agree, not an independent structure); out of place and in place."""
    g, k, aux, _, y = _case(feat, real, n, h, w)
    out = torch.full_like(y, float('nan'))
    conv_into(_nhwc(g), k, np.zeros(feat, np.float32), 1, _nhwc(aux), out, 1.0, ref=True)
    assert torch.equal(out, y)
    buf = _nhwc(aux)
    conv_into(_nhwc(g), k, np.zeros(feat, np.float32), 1, buf, buf, 1.0, ref=True)
    assert torch.equal(buf, y)


@pytest.mark.parametrize('feat', [128, 256])
@pytest.mark.parametrize('n,h,w', [(1, 20, 40), (2, 7, 31)])
def test_dgrad_output_delta_kernels_shift_exactly(feat, n, h, w):
    """Known answer (the pattern of test_gpu_conv.py::test_delta_kernel_shifts_exactly): W' one-hot at (tap, lane, channel) for
    every one of the nine taps, the input lanes 0, 5 and 15 and the output channels 0, 31, 32, F/2 and F - 1 (the pair boundary of
    the fp32 packing, both slabs at F = 256).  That channel is aux plus the shifted lane — zero outside the image, one fp32
    addition, so bit for bit — and every other channel is aux exactly.  In place, as the step runs it."""
    rng = np.random.default_rng(feat + h + w)
    g = torch.from_numpy(rng.standard_normal((n, h, w, 16)).astype(np.float32)).cuda()
    aux = torch.from_numpy(rng.standard_normal((n, h, w, feat)).astype(np.float32)).cuda()
    padded = torch.nn.functional.pad(g, (0, 0, 1, 1, 1, 1))            # [n, h + 2, w + 2, 16]
    zero = np.zeros(feat, np.float32)
    for dy in range(3):
        for dx in range(3):
            for lane in (0, 5, 15):
                shifted = padded[:, dy:dy + h, dx:dx + w, lane]
                for co in (0, 31, 32, feat // 2, feat - 1):
                    k = np.zeros((3, 3, 16, feat), np.float32)
                    k[dy, dx, lane, co] = 1
                    want = aux.clone()
                    want[..., co] += shifted
                    buf = aux.clone()
                    conv_into(g, k, zero, 1, buf, buf, 1.0)
                    assert torch.equal(buf, want), (dy, dx, lane, co)
