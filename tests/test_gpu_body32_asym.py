"""conv3x3_body32.hip where waves 0-3 issue every DMA (Body32Form::DeferAsym): bit for bit the one-tile-per-workgroup kernel.

The shapes are the smallest at which the form can go wrong: one masked pixel, one tile, ragged tiles (zero padding written by
out-of-range lanes of the two-group input rounds), two slabs, and — the only small shapes with a deferred epilogue, a weight
stream that crosses an item boundary and set_stage_item for a second item — a few more items than the device has compute units,
so that some workgroups own two.  A wrong wait count shows as wrong bits.  Every case runs both epilogues."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

MAX_PATCHES = 80


def _rand(rng, shape, scale=1.0):
    return torch.from_numpy((rng.standard_normal(shape) * scale).astype(np.float32))


def _two_item_batch(feat):
    """Patches of 32 x 32 that give a few more items (16 x 16 tile x 128-channel slab) than the device has compute units."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    per_patch = 4 * (feat // 128)
    n = cus // per_patch + 1
    if n > MAX_PATCHES:
        pytest.skip('%d compute units: %d patches needed for a second item' % (cus, n))
    assert cus < n * per_patch < 2 * cus
    return n


def _operands(feat, n, h, w):
    rng = np.random.default_rng(1000 * feat + 37 * n + h)
    x = _rand(rng, (n, h, w, feat)).cuda()
    res = _rand(rng, (n, h, w, feat)).cuda()
    k = _rand(rng, (3, 3, feat, feat), np.sqrt(2.0 / (9 * feat))).numpy()
    b = _rand(rng, (feat,), 0.1).numpy()
    return x, res, k, b


def _check_both_epilogues(feat, n, h, w):
    from dsen2_amd.DSen2Net import conv3x3_nhwc
    x, res, k, b = _operands(feat, n, h, w)
    for epi, aux in ((0, None), (1, res)):
        a = conv3x3_nhwc(x, k, b, epilogue=epi, aux=aux)
        r = conv3x3_nhwc(x, k, b, epilogue=epi, aux=aux, ref=True)
        assert torch.equal(a, r), (feat, n, h, w, epi, int((a != r).sum()))
        assert bool(a.any())


@pytest.mark.parametrize('feat,n,h,w', [
    (128, 1, 1, 1),         # one item, the last-item epilogue only, 255 of 256 pixels masked
    (128, 1, 16, 16),       # one full tile
    (128, 3, 21, 37),       # ragged right and bottom tiles
    (256, 1, 19, 16),       # two slabs, 8 input chunks
])
def test_small_shapes_are_bit_identical_to_the_reference_structure(feat, n, h, w):
    _check_both_epilogues(feat, n, h, w)


@pytest.mark.parametrize('feat', [128, 256])
def test_workgroups_with_two_items_are_bit_identical_to_the_reference_structure(feat):
    _check_both_epilogues(feat, _two_item_batch(feat), 32, 32)


def _residual_into(x, k, b, aux, out):
    """conv3x3_nhwc's call with the caller's output tensor (which may be `aux` itself)."""
    from dsen2_amd import _lib
    from dsen2_amd.DSen2Net import RES_SCALE, _ptr, _stream_ptr
    n, h, w, cin = x.shape
    with torch.cuda.device(x.device):
        _lib.call('dsen2_conv3x3_nhwc', _ptr(x), k.ctypes.data_as(_lib.c_float_p), b.ctypes.data_as(_lib.c_float_p), _ptr(aux),
                  _ptr(out), n, h, w, cin, k.shape[3], 1, float(RES_SCALE), _stream_ptr(x.device))
    return out


def test_residual_epilogue_in_place_and_twice_the_same_bits():
    """aux is out: a piece's residual quad is read before the piece is stored, by the same lane.  And a second call on the same
    operands gives the same bits as the first."""
    from dsen2_amd.DSen2Net import conv3x3_nhwc
    feat = 128
    n = _two_item_batch(feat)
    x, res, k, b = _operands(feat, n, 32, 32)
    r = conv3x3_nhwc(x, k, b, epilogue=1, aux=res, ref=True)
    first = conv3x3_nhwc(x, k, b, epilogue=1, aux=res)
    second = conv3x3_nhwc(x, k, b, epilogue=1, aux=res)
    assert torch.equal(first, r)
    assert torch.equal(second, first)
    stream = res.clone()
    _residual_into(x, k, b, stream, stream)
    assert torch.equal(stream, r)
