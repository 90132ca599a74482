"""Training-set creation, host side (no GPU): the Gaussian weights, the random origins, the validation split, the command lines'
arguments / directory layout / roi.json / ROI snapping, the refusals, and the C ABI's new symbol and its argument checks."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import trainset_fixtures as fx  # noqa: E402

from dsen2_amd import cli, create_patches, create_random, patches  # noqa: E402


def test_gaussian_weights_equal_the_recorded_ones_bit_for_bit():
    rec = np.load(os.path.join(fx.GOLDEN, 'trainset_weights.npz'))
    for scale, radius in ((2, 2), (6, 1)):
        w, r = patches.gaussian_weights(scale)
        assert r == radius and w.dtype == np.float64
        assert w.tobytes() == rec['s%d' % scale].tobytes()
    # any other scale: scipy's formula with the numpy at hand
    w, r = patches.gaussian_weights(3)
    assert r == 1 and w.shape == (3,) and abs(w.sum() - 1) < 1e-15 and w[0] == w[2]
    w, r = patches.gaussian_weights(1)
    assert r == 4 and w.shape == (9,)


def test_random_origins_equal_the_reference_draws():
    assert np.array_equal(patches.random_origins((150, 150, 6), 16, fx.NR_CROP_20, fx.SEED_20), fx.load_split('trainset_random20', 'origins'))
    assert np.array_equal(patches.random_origins((32, 32, 2), 16, fx.NR_CROP_60, fx.SEED_60), fx.load_split('trainset_random60', 'origins'))
    # seed=None: the module's global generator, as the reference uses it
    import random
    random.seed(fx.SEED_20)
    assert np.array_equal(patches.random_origins((150, 150, 6), 16, fx.NR_CROP_20), fx.load_split('trainset_random20', 'origins'))
    with pytest.raises(ValueError):
        patches.random_origins((16, 40, 2), 16, 4, 0)          # the reference: randrange(0, 0)


def test_create_random_equals_the_recorded_mask(tmp_path, capsys):
    rec = np.load(os.path.join(fx.GOLDEN, 'trainset_val_index.npz'))
    index, draws = create_random.make_index(int(rec['size']), float(rec['ratio']), int(rec['seed']))
    assert index.dtype == np.bool_ and np.array_equal(index, rec['index']) and draws == int(rec['iterations'])
    # the command line counts the patches it finds and writes the mask next to them
    for name, n in (('A.SAFE', 120), ('B.SAFE', 80)):
        os.makedirs(str(tmp_path / 'train' / name))
        np.save(str(tmp_path / 'train' / name / 'data10.npy'), np.zeros((n, 4, 2, 2), np.float32))
    assert create_random.main(['--path', str(tmp_path), '--seed', str(int(rec['seed']))]) == 0
    written = np.load(str(tmp_path / 'train' / 'val_index.npy'))
    assert written.dtype == np.bool_ and np.array_equal(written, rec['index'])
    out = capsys.readouterr().out.splitlines()
    assert out == ['Full no of samples: 200', 'Validation samples: 20', 'Number of iterations: %d' % int(rec['iterations'])]
    os.makedirs(str(tmp_path / 'train60' / 'A.SAFE'))
    np.save(str(tmp_path / 'train60' / 'A.SAFE' / 'data10.npy'), np.zeros((30, 4, 2, 2), np.float32))
    assert create_random.main(['--path', str(tmp_path), '--run_60', '--ratio', '0.2', '--size', '50', '--seed', '1']) == 0
    v = np.load(str(tmp_path / 'train60' / 'val_index.npy'))
    assert v.shape == (50,) and v.sum() == 10
    with pytest.raises(OSError):
        create_random.count_patches(str(tmp_path / 'nothing'))


def test_arguments_mirror_the_reference():
    a = create_patches.parse_args(['tile.npz'])
    assert (a.data_file, a.roi_x_y, a.test_data, a.run_60, a.true_data, a.write_images, a.save_prefix) == \
        ('tile.npz', '', False, False, False, False, '../data/')
    assert a.seed is None and a.nr_crop is None and a.name is None
    a = create_patches.parse_args(['p/', '--roi_x_y', '0,0,100,100', '--test_data', '--run_60', '--save_prefix', 'o/', '--seed', '3',
                                   '--nr_crop', '12', '--name', 'X.SAFE'])
    assert (a.roi_x_y, a.test_data, a.run_60, a.save_prefix, a.seed, a.nr_crop, a.name) == ('0,0,100,100', True, True, 'o/', 3, 12, 'X.SAFE')
    assert create_patches.product_name('/d/S2A_X.SAFE/') == 'S2A_X.SAFE' and create_patches.product_name('/d/S2A_X.SAFE') == 'S2A_X.SAFE'


@pytest.mark.parametrize('roi, size', [((2000, 2000, 3200, 3200), 10980), ((10, 50, 575, 599), 600), ((700, 0, 20, 90), 600),
                                       ((0, 0, 30, 30), 600)])
def test_roi_is_snapped_to_multiples_of_36(roi, size):
    x1, y1, x2, y2 = roi
    # training/create_patches.py:63-71
    xmin, xmax = max(min(x1, x2, size - 1), 0), min(max(x1, x2, 0), size - 1)
    ymin, ymax = max(min(y1, y2, size - 1), 0), min(max(y1, y2, 0), size - 1)
    want = (int(xmin / 36) * 36, int(ymin / 36) * 36, int((xmax + 1) / 36) * 36 - 1, int((ymax + 1) / 36) * 36 - 1)
    got = cli.snap_roi(x1, y1, x2, y2, size, size, 36)
    assert got == want
    if got[2] >= got[0] and got[3] >= got[1]:
        assert (got[2] - got[0] + 1) % 36 == 0 and got[0] % 36 == 0
    assert cli.snap_roi(x1, y1, x2, y2, size, size) == cli.snap_roi(x1, y1, x2, y2, size, size, 6)      # the inference default


@pytest.fixture
def fake_gpu(monkeypatch):
    """The GPU steps of create_patches replaced by host stand-ins that record what they were given: the plumbing under test is
    the host's (directory layout, roi.json, no_tiling, which image goes where)."""
    calls = []
    monkeypatch.setattr(patches, 'default_device', lambda: torch.device('cpu'))

    def upload(img, device=None):
        a = np.ascontiguousarray(img)
        calls.append(('upload', a.dtype.name, a.shape))
        return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a), a.dtype.type
    monkeypatch.setattr(patches, 'upload_raster', upload)

    def down(t, scale, np_dtype=None):
        calls.append(('down', str(t.dtype), tuple(t.shape), scale, np.dtype(np_dtype).name))
        return t[::scale, ::scale].to(torch.float32)
    monkeypatch.setattr(patches, 'down_pixel_aggr_device', down)

    def saver(kind, names):
        def fn(*a, **kw):
            file = [x for x in a if isinstance(x, str)][0]
            calls.append((kind, [tuple(x.shape) for x in a if not isinstance(x, str)], kw))
            for n in names:
                np.save(file + n, np.zeros(1, np.float32))
        return fn
    monkeypatch.setattr(patches, 'save_random_patches', saver('random', ['data10', 'data20_gt', 'data20']))
    monkeypatch.setattr(patches, 'save_random_patches60', saver('random60', ['data10', 'data60_gt', 'data20', 'data60']))
    monkeypatch.setattr(patches, 'save_test_patches', saver('test', ['data10', 'data20']))
    monkeypatch.setattr(patches, 'save_test_patches60', saver('test60', ['data10', 'data20', 'data60']))
    return calls


def _tile(tmp_path, n=648):
    rng = np.random.default_rng(5)
    path = str(tmp_path / 'S2A_TILE.npz')
    np.savez(path, data10=rng.integers(1, 9000, (n, n, 4)).astype(np.uint16), data20=rng.integers(1, 9000, (n // 2, n // 2, 6)).astype(np.uint16),
             data60=rng.integers(1, 9000, (n // 6, n // 6, 2)).astype(np.uint16))
    return path


def test_train_mode_layout_and_what_is_uploaded(fake_gpu, tmp_path, capsys):
    path, prefix = _tile(tmp_path), str(tmp_path / 'data') + '/'
    assert create_patches.main([path, '--save_prefix', prefix, '--seed', '7', '--nr_crop', '5']) == 0
    d = tmp_path / 'data' / 'train' / 'S2A_TILE.SAFE'                # the training loader's *SAFE pattern finds it
    assert sorted(os.listdir(str(d))) == ['data10.npy', 'data20.npy', 'data20_gt.npy']
    # the rasters went up as uint16, not widened; the 60 m image is not touched without --run_60
    assert [c for c in fake_gpu if c[0] == 'upload'] == [('upload', 'uint16', (648, 648, 4)), ('upload', 'uint16', (324, 324, 6))]
    assert [c[1:] for c in fake_gpu if c[0] == 'down'] == [('torch.int16', (648, 648, 4), 2, 'uint16'), ('torch.int16', (324, 324, 6), 2, 'uint16')]
    kind, shapes, kw = [c for c in fake_gpu if c[0] == 'random'][0]
    assert shapes == [(324, 324, 6), (324, 324, 4), (162, 162, 6)] and kw == {'NR_CROP': 5, 'seed': 7}
    out = capsys.readouterr().out.splitlines()
    assert out[0] == 'I will proceed with file ' + path
    assert out[1:5] == ['Selected UTM Zone:', 'Selected pixel region: xmin=0, ymin=0, xmax=647, ymax=647:',
                        'Selected pixel region: tmxmin=0, tmymin=0, tmxmax=647, tmymax=647:', 'Image size: width=648 x height=648']
    assert out[5:8] == ['Selected 10m bands: B4 B3 B2 B8', 'Selected 20m bands: B5 B6 B7 B8A B11 B12', 'Selected 60m bands:']
    assert 'Writing files for training to:' + str(d) + '/' in out and out[-1] == 'Success.'
    # defaults of the reference: 8000 crops, 500 at 60 m
    assert create_patches.main([path, '--save_prefix', prefix, '--run_60', '--name', 'other']) == 0
    kind, shapes, kw = [c for c in fake_gpu if c[0] == 'random60'][0]
    assert shapes == [(108, 108, 2), (108, 108, 4), (54, 54, 6), (18, 18, 2)] and kw == {'NR_CROP': 500, 'seed': None}
    assert sorted(os.listdir(str(tmp_path / 'data' / 'train60' / 'other'))) == ['data10.npy', 'data20.npy', 'data60.npy', 'data60_gt.npy']


def test_test_and_true_mode_layout_and_roi_json(fake_gpu, tmp_path, capsys):
    path, prefix = _tile(tmp_path), str(tmp_path / 'data') + '/'
    assert create_patches.main([path, '--save_prefix', prefix, '--test_data', '--roi_x_y', '40,80,300,400']) == 0
    d = tmp_path / 'data' / 'test' / 'S2A_TILE.SAFE'
    # snapped to 36: x 36..287, y 72..395
    assert json.load(open(str(d / 'roi.json'))) == [36 // 2, 72 // 2, 288 // 2, 396 // 2]
    assert sorted(os.listdir(str(d))) == ['data10.npy', 'data20.npy', 'no_tiling', 'roi.json']
    assert sorted(os.listdir(str(d / 'no_tiling'))) == ['data10.npy', 'data20.npy', 'data20_gt.npy']
    z = np.load(path)
    gt = np.load(str(d / 'no_tiling' / 'data20_gt.npy'))
    assert gt.dtype == np.float32 and np.array_equal(gt, z['data20'][36:198, 18:144].astype(np.float32))
    lr10 = np.load(str(d / 'no_tiling' / 'data10.npy'))
    assert lr10.dtype == np.float32 and lr10.shape == (162, 126, 4)
    assert 'Selected pixel region: tmxmin=36, tmymin=72, tmxmax=287, tmymax=395:' in capsys.readouterr().out

    assert create_patches.main([path, '--save_prefix', prefix, '--test_data', '--run_60']) == 0
    d = tmp_path / 'data' / 'test60' / 'S2A_TILE.SAFE'
    assert json.load(open(str(d / 'roi.json'))) == [0, 0, 108, 108]
    assert sorted(os.listdir(str(d / 'no_tiling'))) == ['data10.npy', 'data20.npy', 'data60.npy', 'data60_gt.npy']
    assert [c[3] for c in fake_gpu if c[0] == 'down'][-3:] == [6, 6, 6]

    n_down = len([c for c in fake_gpu if c[0] == 'down'])
    assert create_patches.main([path, '--save_prefix', prefix, '--true_data']) == 0
    d = tmp_path / 'data' / 'true' / 'S2A_TILE.SAFE'
    assert json.load(open(str(d / 'roi.json'))) == [0, 0, 648, 648]
    assert sorted(os.listdir(str(d / 'no_tiling'))) == ['data10.npy', 'data20.npy', 'data60.npy']
    assert len([c for c in fake_gpu if c[0] == 'down']) == n_down              # the image itself: nothing is downsampled
    kind, shapes, kw = [c for c in fake_gpu if c[0] == 'test60'][-1]
    assert shapes == [(648, 648, 4), (324, 324, 6), (108, 108, 2)] and kw == {'patchSize': 384, 'border': 12}
    # a region smaller than one 36-pixel cell
    assert create_patches.main([path, '--save_prefix', prefix, '--roi_x_y', '0,0,20,20']) == 0
    assert 'Invalid region of interest / UTM Zone combination' in capsys.readouterr().out


def test_write_images_is_refused_and_nothing_is_opened(tmp_path, capsys):
    assert create_patches.main([str(tmp_path / 'does_not_exist.npz'), '--write_images', '--save_prefix', str(tmp_path) + '/']) == 2
    assert capsys.readouterr().out.strip() == create_patches.NO_IMAGES
    assert os.listdir(str(tmp_path)) == []


def test_indivisible_sizes_fail_before_the_gpu(tmp_path, capsys, monkeypatch):
    def no_gpu():
        raise AssertionError('the GPU was asked for')
    monkeypatch.setattr(patches, 'default_device', no_gpu)
    with pytest.raises(ValueError, match='not a multiple of SCALE = 2'):
        patches.downPixelAggr(np.zeros((7, 8, 2), np.uint16), SCALE=2)
    with pytest.raises(ValueError, match='not a multiple of SCALE = 6'):
        patches.downPixelAggr(np.zeros((12, 100), np.float32), SCALE=6)


def test_c_abi_declares_exports_and_checks_down_pixel_aggr():
    import ctypes
    from dsen2_amd import _lib, build
    build.build()
    lib = _lib.load()
    header = open(os.path.join(ROOT, 'include', 'dsen2_hip.h')).read()
    assert re.search(r'\bint dsen2_down_pixel_aggr\s*\(', header) and 'dsen2_down_pixel_aggr' in _lib.SIGNATURES
    m = re.findall(r'#define DSEN2_DTYPE_(U16|F32) (\d)', header)
    assert dict(m) == {'U16': str(_lib.DTYPE_U16), 'F32': str(_lib.DTYPE_F32)}
    fn = lib.dsen2_down_pixel_aggr
    w = (ctypes.c_double * 17)(*([1.0 / 17] * 17))
    img, out = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x2000)        # never dereferenced: every call below is refused first

    def refused(*args):
        assert fn(*args) == _lib.ERR_INVALID
        return lib.dsen2_last_error().decode()
    assert 'not a multiple' in refused(img, _lib.DTYPE_U16, 7, 8, 4, 2, w, 2, out, 0, None)
    assert 'not a multiple' in refused(img, _lib.DTYPE_F32, 12, 100, 1, 6, w, 1, out, 1, None)
    assert 'radius 9' in refused(img, _lib.DTYPE_U16, 64, 64, 4, 2, w, 9, out, 0, None)
    assert 'larger than the image' in refused(img, _lib.DTYPE_U16, 2, 64, 4, 2, w, 4, out, 0, None)
    assert 'dtype 7' in refused(img, 7, 64, 64, 4, 2, w, 2, out, 0, None)
    assert 'scale' in refused(img, _lib.DTYPE_U16, 64, 64, 4, 0, w, 2, out, 0, None)
    refused(None, _lib.DTYPE_U16, 64, 64, 4, 2, w, 2, out, 0, None)
    refused(img, _lib.DTYPE_U16, 64, 64, 4, 2, None, 2, out, 0, None)


def test_filter_sums_are_not_contracted_in_the_isa(tmp_path):
    """scipy rounds the product and the sum separately; an FMA would round once and the truncation to uint16 then differs near
    integer boundaries.  The only v_fma_f64 the kernels may hold are the refinement steps of the IEEE division sum / SCALE^2, which
    sit between that division's v_rcp_f64 and its v_div_fixup_f64."""
    from dsen2_amd import asm_contract, build
    out = str(tmp_path / 'down.s')
    subprocess.check_call([build.HIPCC] + [f for f in build.FLAGS if f != '-fPIC'] + ['-S', '--cuda-device-only',
                          os.path.join(build.CSRC, 'down_pixel_aggr.hip'), '-o', out], stderr=subprocess.DEVNULL)
    kernels = {k: v for k, v in asm_contract._kernels(open(out).read()).items() if 'down_pixel_aggr_kernel' in k}
    assert len(kernels) == 12                                    # {uint16, float32} x {float32, float64} x {2/2, 6/1, run time}
    for name, body in kernels.items():
        assert not any('scratch_' in ln for ln in body), name
        assert sum(ln.startswith('v_mul_f64') for ln in body) >= 2 and sum(ln.startswith('v_add_f64') for ln in body) >= 2, name
        in_division = False
        for ln in body:
            if ln.startswith('v_rcp_f64'):
                in_division = True
            elif ln.startswith('v_div_fixup_f64'):
                in_division = False
            elif ln.startswith('v_fma_f64'):
                assert in_division, '%s: fused multiply-add outside a division: %s' % (name, ln)


def test_the_product_does_not_import_the_tests_restatement():
    for base, _, files in os.walk(os.path.join(ROOT, 'dsen2_amd')):
        for f in files:
            if f.endswith('.py'):
                text = open(os.path.join(base, f)).read()
                assert 'downsample_restatement' not in text and 'trainset_fixtures' not in text, f


def test_gdal_branch_reuses_the_command_lines_product_code(fake_gpu, tmp_path, capsys, monkeypatch):
    """A product GDAL opens: cli.GdalProduct with the ROI snapped to 36, the reference's printed lines, bands by name (B10 never)."""
    import types
    from fake_gdal import arrays, fake_gdal
    d10, d20, d60 = arrays(144)
    gdal = fake_gdal(d10, d20, d60)
    osgeo = types.ModuleType('osgeo')
    osgeo.gdal = gdal
    monkeypatch.setitem(sys.modules, 'osgeo', osgeo)
    monkeypatch.setitem(sys.modules, 'osgeo.gdal', gdal)
    prefix = str(tmp_path / 'data') + '/'
    assert create_patches.main(['S2A.zip', '--save_prefix', prefix, '--run_60', '--test_data', '--roi_x_y', '40,30,120,130']) == 0
    out = capsys.readouterr().out
    assert 'Selected pixel region: tmxmin=36, tmymin=0, tmxmax=107, tmymax=107:' in out and 'Image size: width=72 x height=108' in out
    assert 'Selected 10m bands: B4 B3 B2 B8' in out and 'Selected 60m bands: B1 B9' in out
    d = tmp_path / 'data' / 'test60' / 'S2A.zip'                     # the product's own name, as in the reference
    assert json.load(open(str(d / 'roi.json'))) == [6, 0, 18, 18]
    assert [c for c in fake_gpu if c[0] == 'upload'] == [('upload', 'uint16', (108, 72, 4)), ('upload', 'uint16', (54, 36, 6)),
                                                         ('upload', 'uint16', (18, 12, 2))]
    assert np.array_equal(np.load(str(d / 'no_tiling' / 'data60_gt.npy')), d60[0:18, 6:18, :2].astype(np.float32))
    # without GDAL the command says what to do instead
    monkeypatch.setitem(sys.modules, 'osgeo', None)
    assert create_patches.main(['S2A.zip', '--save_prefix', prefix]) == 2
    assert 'GDAL (osgeo) is not importable' in capsys.readouterr().out
