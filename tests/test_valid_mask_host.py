"""Class masks — what can be checked without a GPU: the numpy restatement against scipy's binary dilation, masks.lut and the
shape-ratio rule, the four C-ABI symbols and every refusal (all of which come before any launch), the command-line flags, and the
refusal of a masked ground truth by a model that was not compiled with mask_nodata."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import valid_mask_restatement as vr  # noqa: E402

from dsen2_amd import _lib, masks  # noqa: E402

FAKE = ctypes.c_void_p(0x1000)           # never dereferenced: every refusal below comes before a launch
NAMES = ('dsen2_class_valid_bits', 'dsen2_tile_flags_from_bits', 'dsen2_raster_apply_valid', 'dsen2_cells_from_valid_bits')


# ---- the restatement itself ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('d', [0, 1, 2, 7, 32])
def test_restated_dilation_is_scipys_binary_dilation_with_a_square(d):
    ndimage = pytest.importorskip('scipy.ndimage')
    rng = np.random.default_rng(d)
    for H, W in ((1, 1), (5, 70), (40, 43), (33, 9)):
        inv = rng.random((H, W)) < 0.03
        inv[0, 0] = inv[H - 1, W - 1] = True
        want = ndimage.binary_dilation(inv, structure=np.ones((2 * d + 1, 2 * d + 1), bool)) if d else inv
        assert np.array_equal(vr.dilate(inv, d), want), (H, W, d)


def test_restated_raw_and_bits():
    table = vr.lut([3, 9])
    cls = np.array([[0, 3], [9, 1]], np.uint8)
    assert vr.raw_invalid(cls, table, 2, 1, 3, 4).tolist() == [[False, False, True, True], [False, False, True, True],
                                                                [True, True, False, False]]
    fine = np.zeros((6, 7), np.uint8)
    fine[5, 2] = 3                                   # block (1, 0) of a 3 x 3 tiling; column 6 is surplus
    fine[0, 6] = 9
    assert vr.raw_invalid(fine, table, 1, 3, 2, 2).tolist() == [[False, False], [True, False]]
    bits = vr.pack_bits(np.ones((1, 33), bool))
    assert bits.dtype == np.uint32 and bits.tolist() == [[0xFFFFFFFF, 1]]
    assert vr.unpack_bits(bits, 33).all()
    valid = np.ones((4, 4), bool)
    valid[3, 0] = False
    assert vr.cells(valid, 2).tolist() == [[0, 0], [1, 0]]
    assert vr.cells(valid, 2, np.array([[7, 0], [0, 0]], np.uint8)).tolist() == [[7, 0], [1, 0]]


# ---- masks.py ------------------------------------------------------------------------------------------------------------------
def test_lut_and_scl_classes():
    assert masks.SCL_INVALID == (0, 1, 3, 8, 9, 10)
    table = masks.lut(masks.SCL_INVALID)
    assert table.dtype == np.uint8 and table.shape == (256,) and np.nonzero(table)[0].tolist() == [0, 1, 3, 8, 9, 10]
    assert np.array_equal(masks.lut(None), table) and np.array_equal(table, vr.lut(masks.SCL_INVALID))
    assert np.nonzero(masks.lut(range(60, 256)))[0].tolist() == list(range(60, 256))     # a probability threshold
    assert not masks.lut(()).any()
    for bad in ((256,), (-1,), (1.5,), (True,)):
        with pytest.raises(ValueError):
            masks.lut(bad)
    assert masks.parse_classes('0, 1,3') == (0, 1, 3) and masks.parse_classes(None) is None and masks.parse_classes('') is None
    for bad in ('a,b', '1,300'):
        with pytest.raises(ValueError):
            masks.parse_classes(bad)


def test_shape_ratio_derivation():
    assert masks.ratio((40, 50), (79, 99)) == (2, 1)
    assert masks.ratio((33, 70), (33, 70)) == (1, 1)
    assert masks.ratio((120, 130), (40, 43)) == (1, 3)
    assert masks.ratio((20, 20), (115, 118)) == (6, 1)
    assert masks.ratio((5490, 5490), (10980, 10980)) == (2, 1) and masks.ratio((1830, 1830), (10980, 10980)) == (6, 1)
    assert masks.ratio((10980, 10980), (1830, 1830)) == (1, 6)
    assert masks.ratio((35, 71), (33, 70)) == (1, 1)                  # surplus rows and columns
    assert masks.ratio((10, 10), (80, 80)) == (8, 1) and masks.ratio((80, 80), (10, 10)) == (1, 8)
    for src, dst in (((10, 10), (81, 81)), ((90, 90), (10, 10)), ((40, 50), (79, 150)), ((40, 150), (79, 50)), ((0, 5), (4, 4)),
                     ((4, 4), (0, 4))):
        with pytest.raises(ValueError) as e:
            masks.ratio(src, dst)
        assert repr(src) in str(e.value) and repr(dst) in str(e.value)


def test_valid_bits_device_refuses_before_it_needs_a_gpu():
    cls = np.zeros((10, 10), np.uint8)
    with pytest.raises(ValueError) as e:
        masks.valid_bits_device(cls, (81, 81))
    assert '(10, 10)' in str(e.value) and '(81, 81)' in str(e.value)
    with pytest.raises(ValueError):
        masks.valid_bits_device(np.zeros((10, 10, 1), np.uint8), (10, 10))
    with pytest.raises(ValueError):
        masks.valid_bits_device(cls, (20, 20), dilate=33)
    with pytest.raises(ValueError):
        masks.valid_bits_device(cls, (20, 20), classes=(300,))


# ---- the C ABI: symbols, and the refusals that come before the GPU ---------------------------------------------------------------
def test_header_declares_the_entries():
    header = open(os.path.join(ROOT, 'include', 'dsen2_hip.h')).read()
    lib = _lib.load()
    for name in NAMES:
        assert re.search(r'\bint %s\s*\(' % name, header) and name in _lib.SIGNATURES and hasattr(lib, name), name
        decl = re.search(r'\bint %s\s*\(([^)]*)\)' % name, header).group(1)
        assert len(decl.split(',')) == len(_lib.SIGNATURES[name][1]), name


def _refused(code):
    assert code == _lib.ERR_INVALID, code
    assert _lib.load().dsen2_last_error().decode()


LUT = np.zeros(256, np.uint8)


def test_class_valid_bits_refuses_before_it_launches():
    lib = _lib.load()

    def bits(cls=FAKE, Hs=40, Ws=50, lut=LUT.ctypes.data, up=2, down=1, H=79, W=99, dilate=0, and_bits=None, out=FAKE):
        return lib.dsen2_class_valid_bits(cls, Hs, Ws, lut, up, down, H, W, dilate, and_bits, out, None)
    for kw in (dict(cls=None), dict(lut=None), dict(out=None),
               dict(up=0), dict(down=0), dict(up=9, H=79, W=99, Hs=40, Ws=50), dict(up=1, down=9, H=4, W=5), dict(up=2, down=2),
               dict(up=-1), dict(down=-3),
               dict(H=81), dict(W=101), dict(Hs=39), dict(Ws=49),                                   # (H-1)/up < Hs broken
               dict(up=1, down=3, Hs=120, Ws=130, H=41, W=43), dict(up=1, down=3, Hs=120, Ws=130, H=40, W=44),   # H*down <= Hs broken
               dict(up=1, H=41, W=50), dict(up=1, H=40, W=51),
               dict(dilate=-1), dict(dilate=33),
               dict(H=0), dict(W=0), dict(H=-5), dict(up=1, Hs=1 << 16, Ws=50, H=(1 << 15) + 1, W=50),
               dict(up=1, Hs=40, Ws=1 << 16, H=40, W=(1 << 15) + 1), dict(Hs=0), dict(Ws=0)):
        _refused(bits(**kw))


def test_flags_apply_and_cells_refuse_before_they_launch():
    lib = _lib.load()

    def flags(bits=FAKE, H=24, W=64, P=16, border=2, empty=FAKE):
        return lib.dsen2_tile_flags_from_bits(bits, H, W, P, border, empty, None)
    for kw in (dict(bits=None), dict(empty=None), dict(border=8), dict(border=9), dict(H=11), dict(W=11), dict(H=0), dict(P=0),
               dict(border=-1)):                                   # dsen2_tile_nodata's own
        _refused(flags(**kw))

    def apply(img=FAKE, dtype=_lib.DTYPE_F32, H=24, W=64, C=6, bits=FAKE):
        return lib.dsen2_raster_apply_valid(img, dtype, H, W, C, bits, None)
    for kw in (dict(img=None), dict(bits=None), dict(dtype=_lib.DTYPE_F64), dict(dtype=-1), dict(dtype=_lib.MASK_BLANK_MAP), dict(C=0),
               dict(C=-2), dict(H=0), dict(W=0), dict(H=(1 << 15) + 1), dict(W=(1 << 15) + 1)):
        _refused(apply(**kw))

    def cells(bits=FAKE, H=24, W=60, S=6, accumulate=0, out=FAKE):
        return lib.dsen2_cells_from_valid_bits(bits, H, W, S, accumulate, out, None)
    for kw in (dict(bits=None), dict(out=None), dict(S=0), dict(S=9), dict(S=-1), dict(S=5), dict(H=25), dict(W=61), dict(H=0), dict(W=0),
               dict(H=(1 << 15) + 6, S=2), dict(W=(1 << 15) + 6, S=2)):
        _refused(cells(**kw))


# ---- command lines ---------------------------------------------------------------------------------------------------------------
def test_cli_hands_the_mask_to_the_drop_in_functions(tmp_path, monkeypatch, capsys):
    from dsen2_amd import cli, supres
    seen = []

    def fake20(d10, d20, deep=False, **kw):
        seen.append(kw)
        return np.repeat(np.repeat(np.asarray(d20, np.float32), 2, 0), 2, 1)
    monkeypatch.setattr(supres, 'DSen2_20', fake20)
    scl = (np.arange(36, dtype=np.uint8) % 12).reshape(6, 6)
    src = str(tmp_path / 'tile.npz')
    np.savez(src, data10=np.ones((12, 12, 4), np.uint16), data20=np.ones((6, 6, 6), np.uint16), scl=scl)
    np.save(str(tmp_path / 'scl10.npy'), np.repeat(np.repeat(scl, 2, 0), 2, 1))
    out = str(tmp_path / 'o.npz')
    assert cli.main([src, out]) == 0
    assert cli.main([src, out, '--mask', 'scl']) == 0
    assert cli.main([src, out, '--mask', str(tmp_path / 'scl10.npy'), '--mask_classes', '8,9', '--mask_dilate', '3']) == 0
    assert seen[0] == {}                                                         # without the flag: the call as it always was
    assert set(seen[1]) == {'mask', 'mask_classes', 'mask_dilate'} and np.array_equal(seen[1]['mask'], scl)
    assert seen[1]['mask_classes'] is None and seen[1]['mask_dilate'] == 0
    assert seen[2]['mask'].shape == (12, 12) and seen[2]['mask_classes'] == (8, 9) and seen[2]['mask_dilate'] == 3
    assert cli.main([src, out, '--mask', 'nosuchkey']) == 2
    assert 'nosuchkey' in capsys.readouterr().out
    for bad in (['--mask_classes', '1'], ['--mask_dilate', '2'], ['--mask', 'scl', '--mask_dilate', '33'],
                ['--mask', 'scl', '--mask_classes', '1,x']):
        with pytest.raises(SystemExit):
            cli.main([src, out] + bad)


def test_cli_crops_the_mask_with_the_region():
    from dsen2_amd import cli
    m20 = np.arange(60 * 60, dtype=np.uint16).reshape(60, 60)
    assert np.array_equal(cli.crop_mask(m20, (120, 120), 12, 24, 47, 83), m20[12:42, 6:24])
    m10 = np.arange(120 * 120).reshape(120, 120)
    assert np.array_equal(cli.crop_mask(m10, (120, 120), 12, 24, 47, 83), m10[24:84, 12:48])
    m60 = np.arange(20 * 20).reshape(20, 20)
    assert np.array_equal(cli.crop_mask(m60, (120, 120), 12, 24, 47, 83), m60[4:14, 2:8])


def test_train_flags():
    from dsen2_amd import train
    a = train.parse_args(['--tiles', 'a.npz', 'b.npz', '--mask_key', 'scl'])
    assert a.mask_key == 'scl' and a.mask_classes is None and a.mask_dilate is None and a.skip_masked is False and a.mask_nodata is False
    a = train.parse_args(['--tiles', 'a.npz', '--mask_key', 'scl', '--mask_classes', '3,8,9', '--mask_dilate', '4', '--skip_masked'])
    assert a.mask_classes == (3, 8, 9) and a.mask_dilate == 4 and a.skip_masked is True
    a = train.parse_args(['--predict', 's2_032_lr_1e-04.npy', '--mask', 'scl.npy', '--mask_classes', '9', '--mask_dilate', '32'])
    assert a.mask == 'scl.npy' and a.mask_classes == (9,) and a.mask_dilate == 32
    plain = train.parse_args([])
    assert plain.mask_key is None and plain.mask is None and plain.skip_masked is False
    for bad in (['--mask_key', 'scl'], ['--tiles', 'a.npz', '--skip_masked'], ['--tiles', 'a.npz', '--mask_classes', '1'],
                ['--tiles', 'a.npz', '--mask_dilate', '1'], ['--tiles', 'a.npz', '--mask_key', 'scl', '--mask_dilate', '33'],
                ['--tiles', 'a.npz', '--mask_key', 'scl', '--mask_classes', '256'], ['--mask', 'scl.npy'],
                ['--tiles', 'a.npz', '--mask', 'scl.npy']):
        with pytest.raises(SystemExit):
            train.parse_args(bad)


def test_tile_class_mask_reads_the_key_of_the_npz(tmp_path):
    from dsen2_amd import train
    f = str(tmp_path / 't.npz')
    np.savez(f, data10=np.zeros((2, 2, 4)), scl=np.full((1, 1), 9, np.uint8))
    assert train.tile_class_mask(f, 'scl').tolist() == [[9]]
    assert train.tile_class_mask(f, 'other') is None and train.tile_class_mask(str(tmp_path / 't.mat'), 'scl') is None


# ---- a masked ground truth and a loss that would not ignore it ---------------------------------------------------------------------
def test_a_masked_target_needs_mask_nodata():
    from dsen2_amd import losses, training
    from dsen2_amd.DSen2Net import S2Model
    plain, masked = losses.parse('mean_absolute_error'), losses.parse('mse', None, True)
    training.check_masked_target(plain, False, 'fit')
    training.check_masked_target(masked, True, 'fit')
    training.check_masked_target(losses.parse_ssim(masked, 0.5), True, 'fit')
    with pytest.raises(ValueError) as e:
        training.check_masked_target(plain, True, 'fit_corpus')
    assert 'mask_nodata' in str(e.value)
    with pytest.raises(ValueError):
        training.check_masked_target(losses.parse_ssim(plain, 0.5), True, 'fit')

    class Model(object):                     # the first thing fit and fit_corpus do, before they look at anything else
        def _loss_setting(self):
            return plain

    class Corpus(object):
        class_masked = True
    with pytest.raises(ValueError) as e:
        S2Model.fit_corpus(Model(), Corpus(), 4, 2)
    assert 'mask_nodata' in str(e.value)
    y = np.zeros((2, 6, 4, 4), np.float32).view(training.MaskedTarget)
    assert y[:1].class_masked and isinstance(y[1:], training.MaskedTarget) and not hasattr(np.asarray(y), 'class_masked')
    with pytest.raises(ValueError):
        S2Model.fit(Model(), [np.zeros((2, 4, 4, 4), np.float32)], y)
    with pytest.raises(ValueError):
        S2Model.fit(Model(), [np.zeros((2, 4, 4, 4), np.float32)], np.asarray(y), validation_data=([], y))


def test_corpus_refuses_bad_class_masks_before_any_upload():
    from dsen2_amd.corpus import TileCorpus
    tile = (np.ones((64, 64, 4), np.uint16), np.ones((32, 32, 6), np.uint16))
    ok = np.zeros((32, 32), np.uint8)
    for kw in (dict(class_masks=[ok, ok]), dict(class_masks=[ok.astype(np.int32)]), dict(class_masks=[ok[None]]),
               dict(class_masks=[ok], mask_dilate=33), dict(class_masks=[ok], mask_dilate=-1), dict(class_masks=[ok], mask_classes=(256,)),
               dict(skip_masked=True), dict(class_masks=[None], skip_masked=True)):
        with pytest.raises(ValueError):
            TileCorpus([tile], **kw)
