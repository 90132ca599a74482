"""Class masks on the GPU: dsen2_class_valid_bits, dsen2_tile_flags_from_bits, dsen2_raster_apply_valid and
dsen2_cells_from_valid_bits bit for bit against the numpy restatement (tests/valid_mask_restatement.py) and inside guard bands
(tests/guarded.py).  Everything is an equality: no tolerance anywhere."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nodata_restatement as nr  # noqa: E402
import valid_mask_restatement as vr  # noqa: E402
from guarded import run_three_ways  # noqa: E402

from dsen2_amd import _lib, masks, patches  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
CLASSES = masks.SCL_INVALID
TABLE = masks.lut(CLASSES)

# (Hs, Ws, up, down, H, W, dilations): the smallest shapes where the kernels can go wrong
CASES = [
    (40, 50, 2, 1, 79, 99, (0, 1, 7, 32)),        # odd target, partial last source row, 4 words with padding bits
    (33, 70, 1, 1, 33, 70, (3,)),
    (120, 130, 1, 3, 40, 43, (2,)),               # block OR, surplus source columns
    (20, 20, 6, 1, 115, 118, (5,)),
    (150, 300, 1, 1, 150, 300, (31, 32)),         # more than one workgroup tile (64 rows x 256 pixels) on both axes
]
IDS = ['%dx%d_up%d_down%d_to_%dx%d' % c[:6] for c in CASES]


def class_raster(case, d, seed):
    """uint8 [Hs, Ws] of valid classes (2, 4, 5, 6, 7, 11) with few enough invalid pixels that the mask dilated by d leaves both
    kinds of pixel: scattered ones and a block for a small d, the two opposite corners (and the centre of a large image) else."""
    Hs, Ws, up, down, H, W, _ = case
    rng = np.random.default_rng(seed)
    cls = rng.choice(np.array([2, 4, 5, 6, 7, 11], np.uint8), size=(Hs, Ws))
    if d >= 8:
        cls[0, 0], cls[Hs - 1, Ws - 1] = 3, 10
        if min(H, W) >= 140:
            cls[Hs // 2, Ws // 2] = 0
        return cls
    n = max(2, int(0.25 * H * W / (2 * d + up + 1) ** 2))
    cls[rng.integers(0, Hs, n), rng.integers(0, Ws, n)] = rng.choice(np.array(CLASSES, np.uint8), size=n)
    if d <= 3:
        cls[Hs // 3:Hs // 3 + 4, Ws // 2:Ws // 2 + 9] = 9
    return cls


def lone_pixels(H, W):
    """Single invalid pixels at the image corners, on the edges of the 64-row x 256-pixel workgroup tiles and on word boundaries."""
    ys = sorted({0, H - 1} | {y for y in (31, 32, 63, 64, 65, 127, 128) if y < H})
    xs = sorted({0, W - 1} | {x for x in (31, 32, 33, 63, 64, 255, 256, 257, 287, 288) if x < W})
    return [(y, x) for y in ys for x in xs]


def run_bits(cls, up, down, H, W, d, table=TABLE, and_bits=None, inplace=False):
    """dsen2_class_valid_bits inside guard bands -> uint32 [H, ceil(W / 32)] on the host."""
    Hs, Ws = cls.shape
    wpr = (W + 31) // 32
    cls_dev = torch.from_numpy(cls).to(DEV)
    table = np.ascontiguousarray(table, dtype=np.uint8)

    def call(inputs, outputs, inplace_t, scratch):
        and_t = inputs[1] if len(inputs) > 1 else (inplace_t[0] if inplace_t else None)
        out = inplace_t[0] if inplace_t else outputs[0]
        _lib.call('dsen2_class_valid_bits', patches._ptr(inputs[0]), Hs, Ws, table.ctypes.data, up, down, H, W, d,
                  patches._ptr(and_t) if and_t is not None else None, patches._ptr(out), patches._stream(DEV))
    what = 'dsen2_class_valid_bits %r up=%d down=%d -> %dx%d dilate=%d' % (cls.shape, up, down, H, W, d)
    if inplace:
        _, (bits,) = run_three_ways(call, [cls_dev], [], inplace=[torch.from_numpy(and_bits.view(np.int32)).to(DEV)], what=what)
    elif and_bits is not None:
        (bits,), _ = run_three_ways(call, [cls_dev, torch.from_numpy(and_bits.view(np.int32)).to(DEV)], [((H, wpr), torch.int32)], what=what)
    else:
        (bits,), _ = run_three_ways(call, [cls_dev], [((H, wpr), torch.int32)], what=what)
    return bits.cpu().numpy().view(np.uint32)


# ---- dsen2_class_valid_bits ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_bits_equal_the_restatement(case):
    Hs, Ws, up, down, H, W, dilations = case
    assert masks.ratio((Hs, Ws), (H, W)) == (up, down)
    for d in dilations:
        cls = class_raster(case, d, seed=Hs + Ws)
        want = vr.valid_bits(cls, TABLE, up, down, H, W, d)
        got = run_bits(cls, up, down, H, W, d)
        assert got.shape == want.shape and np.array_equal(got, want), (case, d, np.argwhere(got != want)[:5].tolist())
        assert 0 < vr.unpack_bits(got, W).mean() < 1                     # the case holds both kinds of pixel
        # masks.valid_bits_device derives up / down itself and gives the same words
        mine = masks.valid_bits_device(cls, (H, W), CLASSES, d, device=DEV)
        assert mine.dtype == torch.int32 and np.array_equal(mine.cpu().numpy().view(np.uint32), want)


@pytest.mark.parametrize('d', [31, 32])
def test_lone_pixels_at_corners_tile_edges_and_word_boundaries(d):
    H, W = 150, 300
    pixels = lone_pixels(H, W)
    assert (0, 0) in pixels and (H - 1, W - 1) in pixels and (64, 256) in pixels and (63, 255) in pixels and (0, 32) in pixels
    all_at_once = np.full((H, W), 4, np.uint8)
    for i, (y, x) in enumerate(pixels):
        all_at_once[y, x] = 3
        if i % 7 == 0:                                                   # each of these alone in the image
            cls = np.full((H, W), 4, np.uint8)
            cls[y, x] = 3
            got = masks.valid_bits_device(cls, (H, W), CLASSES, d, device=DEV).cpu().numpy().view(np.uint32)
            want = np.ones((H, W), bool)
            want[max(0, y - d):y + d + 1, max(0, x - d):x + d + 1] = False
            assert np.array_equal(got, vr.pack_bits(want)), (y, x, d)
    want = vr.valid_bits(all_at_once, TABLE, 1, 1, H, W, d)
    assert np.array_equal(run_bits(all_at_once, 1, 1, H, W, d), want)


@pytest.mark.parametrize('d', [0, 5])
def test_all_valid_and_all_invalid(d):
    for (Hs, Ws, up, down, H, W, _) in CASES[:3]:
        wpr = (W + 31) // 32
        got = run_bits(np.full((Hs, Ws), 4, np.uint8), up, down, H, W, d)
        assert np.array_equal(got, vr.pack_bits(np.ones((H, W), bool)))
        if W % 32:
            assert (got[:, wpr - 1] == np.uint32((1 << (W % 32)) - 1)).all()          # padding bits are 0
        got = run_bits(np.full((Hs, Ws), 9, np.uint8), up, down, H, W, d)
        assert not got.any()


@pytest.mark.parametrize('d', [0, 7])
def test_and_bits_also_in_place(d):
    Hs, Ws, up, down, H, W, _ = CASES[0]
    cls = class_raster(CASES[0], d, seed=5)
    rng = np.random.default_rng(d)
    other = vr.pack_bits(rng.random((H, W)) < 0.7)
    want = vr.valid_bits(cls, TABLE, up, down, H, W, d, and_bits=other)
    assert np.array_equal(want, vr.pack_bits(vr.valid_pixels(cls, TABLE, up, down, H, W, d) & vr.unpack_bits(other, W)))
    assert np.array_equal(run_bits(cls, up, down, H, W, d, and_bits=other), want)
    assert np.array_equal(run_bits(cls, up, down, H, W, d, and_bits=other, inplace=True), want)
    both = torch.from_numpy(other.view(np.int32)).to(DEV)
    assert masks.valid_bits_device(cls, (H, W), CLASSES, d, and_bits=both, out=both) is both
    assert np.array_equal(both.cpu().numpy().view(np.uint32), want)


def test_a_table_as_a_probability_threshold():
    Hs, Ws, up, down, H, W, _ = CASES[1]
    prob = np.random.default_rng(8).integers(0, 256, size=(Hs, Ws), dtype=np.uint8)
    prob[0, 0], prob[1, 1], prob[2, 2] = 59, 60, 255
    table = masks.lut(range(60, 256))
    for d in (0, 1):
        got = run_bits(prob, up, down, H, W, d, table=table)
        assert np.array_equal(got, vr.pack_bits(~vr.dilate(prob >= 60, d)))
    table2 = (np.arange(256) >= 60).astype(np.uint8) * 200                # any non-zero entry means invalid
    assert np.array_equal(run_bits(prob, up, down, H, W, 0, table=table2), vr.pack_bits(prob < 60))


# ---- dsen2_tile_flags_from_bits --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('H,W', [(24, 64), (31, 65), (50, 130)])
def test_flags_from_bits_are_tile_nodatas_own_flags(H, W):
    P, border = 16, 2
    rng = np.random.default_rng(H + W)
    img = rng.uniform(1.0, 9.0, size=(H, W, 4)).astype(np.float32)
    img[np.kron(rng.random((H // 6 + 1, W // 6 + 1)) < 0.6, np.ones((6, 6), bool))[:H, :W]] = 0.0
    empty, bits = patches.nodata_device(torch.from_numpy(img).to(DEV), P, border)
    assert 0 < int(empty.sum()) < empty.numel()
    x_tiles, y_tiles, words = patches.nodata_geometry((H, W), P, border)

    def call(inputs, outputs, inplace, scratch):
        _lib.call('dsen2_tile_flags_from_bits', patches._ptr(inputs[0]), H, W, P, border, patches._ptr(outputs[0]), patches._stream(DEV))
    (got,), _ = run_three_ways(call, [bits], [((x_tiles * y_tiles,), torch.uint8)], what='dsen2_tile_flags_from_bits')
    assert torch.equal(got, empty)
    assert torch.equal(masks.tile_flags_device(bits, (H, W), P, border), empty)
    # and for a bitmap that no raster wrote
    valid = rng.random((H, W)) < 0.01
    mine = torch.from_numpy(vr.pack_bits(valid).view(np.int32)).to(DEV)
    assert np.array_equal(masks.tile_flags_device(mine, (H, W), P, border).cpu().numpy(), nr.patch_empty(valid, P - 2 * border))


# ---- dsen2_raster_apply_valid ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('C', [6, 2])
@pytest.mark.parametrize('dtype', ['uint16', 'float32'])
@pytest.mark.parametrize('H,W', [(33, 70), (40, 64)])
def test_apply_valid_zeroes_the_masked_pixels_and_nothing_else(H, W, dtype, C):
    rng = np.random.default_rng(H + C)
    valid = rng.random((H, W)) < 0.6
    valid[0, 0], valid[H - 1, W - 1], valid[0, W - 1] = False, False, True
    if dtype == 'uint16':
        img = rng.integers(1, 65536, size=(H, W, C), dtype=np.uint16)
        img_dev = torch.from_numpy(img.view(np.int16)).to(DEV)
    else:
        img = rng.standard_normal((H, W, C)).astype(np.float32)
        img[1, 1], img[2, 2, 0] = np.nan, -0.0
        img_dev = torch.from_numpy(img).to(DEV)
    bits = torch.from_numpy(vr.pack_bits(valid).view(np.int32)).to(DEV)
    code = _lib.DTYPE_U16 if dtype == 'uint16' else _lib.DTYPE_F32

    def call(inputs, outputs, inplace, scratch):
        _lib.call('dsen2_raster_apply_valid', patches._ptr(inplace[0]), code, H, W, C, patches._ptr(inputs[0]), patches._stream(DEV))
    _, (got,) = run_three_ways(call, [bits], [], inplace=[img_dev], what='dsen2_raster_apply_valid %s C=%d' % (dtype, C))
    got = got.cpu().numpy().view(img.dtype)
    want = vr.apply_valid(img, valid)
    assert got.tobytes() == want.tobytes()                                # byte for byte: valid pixels untouched, +0.0 elsewhere
    assert not got[~valid].view(np.uint8).any() and got[valid].tobytes() == img[valid].tobytes()
    mine = masks.raster_apply_valid_device(img_dev.clone(), bits)
    assert mine.cpu().numpy().view(img.dtype).tobytes() == want.tobytes()


# ---- dsen2_cells_from_valid_bits -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('accumulate', [False, True])
@pytest.mark.parametrize('S,H,W', [(2, 34, 70), (6, 36, 102)])
def test_cells_from_bits(S, H, W, accumulate):
    rng = np.random.default_rng(S + H)
    valid = rng.random((H, W)) < 0.97
    valid[H - 1, W - 1] = False
    valid[:S, :S] = True
    bits = torch.from_numpy(vr.pack_bits(valid).view(np.int32)).to(DEV)
    prior = (rng.random((H // S, W // S)) < 0.2).astype(np.uint8) * 3
    prior[0, 0] = 7

    def call(inputs, outputs, inplace, scratch):
        out = inplace[0] if accumulate else outputs[0]
        _lib.call('dsen2_cells_from_valid_bits', patches._ptr(inputs[0]), H, W, S, int(accumulate), patches._ptr(out), patches._stream(DEV))
    if accumulate:
        _, (got,) = run_three_ways(call, [bits], [], inplace=[torch.from_numpy(prior).to(DEV)], what='dsen2_cells_from_valid_bits')
        want = vr.cells(valid, S, prior)
        assert want[0, 0] == 7
        cells = torch.from_numpy(prior).to(DEV)
        assert masks.cells_from_bits_device(bits, (H, W), S, cells=cells) is cells and np.array_equal(cells.cpu().numpy(), want)
    else:
        (got,), _ = run_three_ways(call, [bits], [((H // S, W // S), torch.uint8)], what='dsen2_cells_from_valid_bits')
        want = vr.cells(valid, S)
        assert want[0, 0] == 0 and want[-1, -1] == 1 and 0 < want.mean() < 1
        assert np.array_equal(masks.cells_from_bits_device(bits, (H, W), S).cpu().numpy(), want)
    assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want)
