"""Adjustable overlap and feathered blending on the GPU: dsen2_recompose_rows_blend bit for bit against the numpy restatement
(tests/blend_restatement.py) and inside guard bands; DSen2_20 / DSen2_60 with border= and feather= against the restatement
applied to model.predict of the library's own patches, for every precision, ending and batch size; two gloo ranks; and the
seams against the float64 oracle's forward of the untiled image.  Everything but that last comparison is an equality."""
import contextlib
import io
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import blend_restatement as br  # noqa: E402
import nodata_restatement as nr  # noqa: E402
from guarded import run_three_ways  # noqa: E402

from dsen2_amd import _lib, patches, weights  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
P, BORDER, INNER = 16, 4, 8
SHAPES = [(8, 20), (19, 27), (24, 32), (33, 70)]        # one tile row; three patches per axis; exact division; ragged
RMSE_GATE_NORMALISED = 1e-4     # the project's fp32 gate, in the network's normalised (/2000) domain (tests/test_gpu_supres.py)


def _bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    if isinstance(a, np.ndarray):
        return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.int32), b.view(np.int32))
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def blend_call(a_dev, C, patch, border, feather, H, W, slots=None, bits=None, scale=2000.0, what='dsen2_recompose_rows_blend'):
    """The entry point inside guard bands, three ways (tests/guarded.py); returns the image of the plain run."""
    def call(inputs, outputs, inplace, scratch):
        _lib.call('dsen2_recompose_rows_blend', patches._ptr(inputs[0]) if inputs[0].shape[0] else None, inputs[0].shape[0], C, patch,
                  border, feather, None if inputs[1] is None else patches._ptr(inputs[1]), None if inputs[2] is None else patches._ptr(inputs[2]),
                  patches._ptr(outputs[0]), H, W, scale, 0, H, patches._stream(DEV))
    (out,), _ = run_three_ways(call, [a_dev, slots, bits], [((H, W, C), torch.float32)], device=DEV, what=what)
    return out


# ---- kernel level ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('F', [1, 3, 4])
@pytest.mark.parametrize('H,W', SHAPES)
def test_kernel_equals_the_restatement_bit_for_bit(H, W, F):
    x_tiles, y_tiles = br.grid(H, W, INNER)
    n = x_tiles * y_tiles
    single = br.weighted_patch_count(H, W, P, BORDER, F) == 1
    for C in (1, 2, 6, 7):
        rng = np.random.default_rng(H * 1000 + W * 10 + C + F)
        a = rng.standard_normal((n + 1, C, P, P)).astype(np.float32)           # one patch more than the grid: never read
        a[n] = np.nan
        a_dev = torch.from_numpy(a).to(DEV)
        got = blend_call(a_dev, C, P, BORDER, F, H, W)
        want = br.blend(a[:n], BORDER, F, H, W, 2000.0)
        assert same_bits(got.cpu().numpy(), want), (C, np.argwhere(got.cpu().numpy() != want)[:4])
        # any split of [0, H) into row bands gives the whole-image bits, and touches no other row
        for step in (1, 3, INNER):
            img = torch.full((H, W, C), -7.0, device=DEV)
            for r0 in range(0, H, step):
                r1 = min(H, r0 + step)
                patches.recompose_rows_device(a_dev, BORDER, img, r0, r1, scale=2000.0, feather=F)
                assert bool((img[r1:] == -7.0).all())
            assert same_bits(img, got), (C, step)
        # whole patches with (b, F) == crops of side inner + 2 F with (F, F)
        crop = BORDER - F
        cropped = a_dev[:, :, crop:P - crop, crop:P - crop].contiguous()
        assert same_bits(patches.recompose_device(cropped, F, (H, W), scale=2000.0, feather=F), got), C
        # pixels with a single weighted patch are dsen2_recompose_rows' pixels
        hard = patches.recompose_device(a_dev, BORDER, (H, W), scale=2000.0)
        m = torch.from_numpy(single).to(DEV)
        assert bool(m.any()) and same_bits(got[m], hard[m]) and not torch.equal(got[~m], hard[~m])
        # patches gathered from one image return that image
        image = rng.standard_normal((H, W, C)).astype(np.float32)
        back = patches.recompose_device(torch.from_numpy(br.cut_patches(image, P, BORDER)).to(DEV), BORDER, (H, W), feather=F)
        assert same_bits(back.cpu().numpy(), image), C
    assert same_bits(patches.recompose_device(a_dev, BORDER, (H, W), scale=2000.0, feather=True),
                     patches.recompose_device(a_dev, BORDER, (H, W), scale=2000.0, feather=BORDER))


@pytest.mark.parametrize('patch,border,feather,C,H,W,most', [(128, 8, 8, 6, 232, 300, 6), (192, 12, 12, 2, 342, 396, 6), (128, 16, 4, 6, 200, 300, 4)])
def test_the_real_geometries(patch, border, feather, C, H, W, most):
    inner = patch - 2 * border
    x_tiles, y_tiles = br.grid(H, W, inner)
    assert br.weighted_patch_count(H, W, patch, border, feather).max() == most              # 6: three patches on the row axis
    rng = np.random.default_rng(H + W)
    a = rng.standard_normal((x_tiles * y_tiles, C, patch, patch)).astype(np.float32)
    got = blend_call(torch.from_numpy(a).to(DEV), C, patch, border, feather, H, W).cpu().numpy()
    assert same_bits(got, br.blend(a, border, feather, H, W, 2000.0))


def test_an_image_above_the_grid_cap():
    """1032 x 1040 pixels > 4096 blocks x 256 threads: the grid-stride loop takes a second pass."""
    H, W, C, F = 1032, 1040, 1, 4
    assert H * W > 4096 * 256
    x_tiles, y_tiles = br.grid(H, W, INNER)
    rng = np.random.default_rng(1)
    a = rng.standard_normal((x_tiles * y_tiles, C, P, P)).astype(np.float32)
    got = patches.recompose_device(torch.from_numpy(a).to(DEV), BORDER, (H, W), scale=2000.0, feather=F).cpu().numpy()
    assert same_bits(got, br.blend(a, BORDER, F, H, W, 2000.0))


def _valid_masks(H, W, seed):
    rng = np.random.default_rng(seed)
    mixed = rng.random((H, W)) < 0.7
    blocks = rng.random((H // 5 + 1, W // 7 + 1)) < 0.5
    mixed &= ~np.kron(blocks, np.ones((5, 7), bool))[:H, :W]
    mixed[:INNER, :2 * INNER] = False                        # two empty patches for certain
    lone = np.zeros((H, W), bool)
    lone[H - 3, W - 2] = True                                # a lone data pixel, where the clamped last tiles overlap their neighbours
    return {'mixed': mixed, 'lone': lone, 'all': np.ones((H, W), bool), 'none': np.zeros((H, W), bool)}


@pytest.mark.parametrize('F', [1, 4])
@pytest.mark.parametrize('H,W', [(19, 27), (33, 70)])
def test_kernel_with_slot_map_and_bitmap(H, W, F):
    C = 6
    x_tiles, y_tiles = br.grid(H, W, INNER)
    n = x_tiles * y_tiles
    rng = np.random.default_rng(H + W + F)
    full = rng.standard_normal((n, C, P, P)).astype(np.float32)
    for name, valid in _valid_masks(H, W, H * W).items():
        empty = nr.patch_empty(valid, INNER)
        kept, slots = patches.slot_map(empty)
        compact = np.full((len(kept) + 2, C, P, P), np.nan, np.float32)         # the unused tail holds NaN
        compact[:len(kept)] = full[kept]
        bits = torch.from_numpy(nr.pack_bits(valid).view(np.int32)).to(DEV)
        c_dev = torch.from_numpy(compact).to(DEV)
        got = blend_call(c_dev, C, P, BORDER, F, H, W, torch.from_numpy(slots).to(DEV), bits, what='blend with maps, ' + name).cpu().numpy()
        want = br.blend(compact, BORDER, F, H, W, 2000.0, slots=slots, valid=valid)
        assert same_bits(got, want) and np.isfinite(got).all(), name
        assert not got[~valid].any()
        if name == 'all':
            assert same_bits(got, br.blend(full, BORDER, F, H, W, 2000.0))
        if name == 'lone':
            assert len(kept) == 1 and np.count_nonzero(got.any(axis=2)) == 1
        # the host wrapper in row bands
        img = torch.full((H, W, C), -7.0, device=DEV)
        for r0 in range(0, H, 5):
            patches.recompose_rows_device(c_dev, BORDER, img, r0, min(H, r0 + 5), scale=2000.0, slots=torch.from_numpy(slots).to(DEV),
                                          valid_bits=bits, feather=F)
        assert same_bits(img.cpu().numpy(), want), name
        if name == 'mixed':
            # slots that are out of range — one past the end, far beyond, negative — count as no slot and read nothing
            assert 2 <= len(kept) < n
            bad = slots.copy()
            bad[kept[0]], bad[kept[1]] = len(compact), 10 ** 6
            bad[np.nonzero(slots < 0)[0][0]] = -5
            want_slots = slots.copy()
            want_slots[[kept[0], kept[1]]] = -1
            got = blend_call(c_dev, C, P, BORDER, F, H, W, torch.from_numpy(bad).to(DEV), bits, what='blend with out-of-range slots').cpu().numpy()
            assert same_bits(got, br.blend(compact, BORDER, F, H, W, 2000.0, slots=want_slots, valid=valid)) and np.isfinite(got).all()
            # slots == 0: every pixel is 0 and the patch buffer may be NULL
            zero = blend_call(c_dev[:0], C, P, BORDER, F, H, W, torch.from_numpy(slots).to(DEV), bits, what='blend with no slots')
            assert not bool(zero.any())


# ---- end to end --------------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def model_dir(tmp_path, monkeypatch):
    """A MDL_PATH holding synthetic checkpoints under the reference's file names (as .npy), as tests/test_gpu_nodata.py's."""
    from dsen2_amd import supres
    np.save(str(tmp_path / 's2_032_lr_1e-04.npy'), weights.random_he_uniform(10, 6, 6, 128, seed=11))
    np.save(str(tmp_path / 's2_030_lr_1e-05.npy'), weights.random_he_uniform(12, 2, 6, 128, seed=12))
    monkeypatch.setattr(supres, 'MDL_PATH', str(tmp_path) + os.sep)
    for name, value in (('BORDER_20', 8), ('BORDER_60', 12), ('FEATHER', None), ('SKIP_NODATA', False), ('SELF_ENSEMBLE', False)):
        monkeypatch.setattr(supres, name, value)
    supres.clear_model_cache()
    yield str(tmp_path)
    supres.clear_model_cache()


def quiet(fn, *a, **k):
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        out = fn(*a, **k)
    return out, buf.getvalue()


CASES = {'20_300x412': (False, 300, 412), '20_224x336': (False, 224, 336), '60_396x540': (True, 396, 540)}
SETTINGS = [('20_300x412', 8, 8), ('20_300x412', 16, None), ('20_300x412', 16, 4), ('20_224x336', 8, 8), ('20_224x336', 16, None),
            ('20_224x336', 16, 4), ('60_396x540', 12, 12), ('60_396x540', 18, None)]


def case_inputs(name, nodata=False):
    """(function name, [d10, d20(, d60)] uint16, patch): the image sizes of tests/test_gpu_nodata.py; nodata: the lower right of
    the 10 m image holds none, but for a lone pixel."""
    run_60, H, W = CASES[name]
    rng = np.random.default_rng(H + W)
    d10 = rng.integers(35, 9000, size=(H, W, 4), dtype=np.uint16)
    if nodata:
        y, x = np.mgrid[0:H, 0:W]
        nod = x / float(W) + y / float(H) >= 0.9
        nod[H - 3, W - 2] = False
        d10[nod] = 0
    args = [d10, rng.integers(35, 9000, size=(H // 2, W // 2, 6), dtype=np.uint16)]
    if run_60:
        args.append(rng.integers(35, 9000, size=(H // 6, W // 6, 2), dtype=np.uint16))
    return ('DSen2_60' if run_60 else 'DSen2_20'), args, (192 if run_60 else 128)


_WANT = {}


def restated(name, border, feather, precision='fp32', ensemble=False, nodata=False):
    """The restatement applied to model.predict of the library's own patches (get_test_patches{,60} with border=), as
    testing/supres.py chains them: /= SCALE, predict, recompose, *= SCALE.  Computed once per key."""
    from dsen2_amd import supres
    key = (name, border, feather, precision, ensemble, nodata)
    if key not in _WANT:
        fn_name, args, patch = case_inputs(name, nodata)
        H, W = args[0].shape[:2]
        get = patches.get_test_patches60 if len(args) == 3 else patches.get_test_patches
        xs = [p / np.float32(supres.SCALE) for p in get(*args, patchSize=patch, border=border)]
        inner = patch - 2 * border
        x_tiles, y_tiles = br.grid(H, W, inner)
        used = x_tiles * y_tiles
        model, _ = quiet(supres._get_model, tuple((int(a.shape[2]), None, None) for a in args), False, len(args) == 3)
        pred = model.predict([x[:used] for x in xs], ensemble=True) if ensemble else model.predict([x[:used] for x in xs])
        F = patches.feather_width(feather, border)
        slots, valid = np.arange(used, dtype=np.int32), np.ones((H, W), bool)
        if nodata:
            valid = nr.valid_pixels(args[0])
            empty = nr.patch_empty(valid, inner)
            assert 2 <= (empty != 0).sum() < used
            slots = np.where(empty != 0, -1, slots).astype(np.int32)
        if F:
            _WANT[key] = br.blend(pred, border, F, H, W, float(supres.SCALE), slots=slots, valid=valid)
        else:
            _WANT[key] = nr.recompose(pred, slots, valid, border, float(supres.SCALE))
    return _WANT[key]


def run_case(name, border, feather, **kw):
    from dsen2_amd import supres
    fn_name, args, patch = case_inputs(name, kw.pop('nodata', False))
    out, printed = quiet(getattr(supres, fn_name), *args, deep=False, border=border, feather=feather, **kw)
    assert out.dtype == np.float32 and out.shape == args[0].shape[:2] + (2 if len(args) == 3 else 6,)
    assert printed.count('(%d, %d, %d)' % (out.shape[2], out.shape[0], out.shape[1])) == 1
    return out


@pytest.mark.parametrize('precision', ['fp32', 'bf16', 'bf16x3'])
@pytest.mark.parametrize('name,border,feather', SETTINGS)
def test_border_and_feather_equal_the_restatement_of_predict(model_dir, monkeypatch, name, border, feather, precision):
    from dsen2_amd import supres
    monkeypatch.setattr(supres, 'PRECISION', precision)
    want = restated(name, border, feather, precision)
    got = run_case(name, border, feather)
    assert same_bits(got, want), (name, border, feather, precision, int((got != want).sum()))
    inner = (192 if name.startswith('60') else 128) - 2 * border
    x_tiles, y_tiles = br.grid(got.shape[0], got.shape[1], inner)
    assert supres.last_run_stats() == {'patches': x_tiles * y_tiles, 'kept': x_tiles * y_tiles, 'skipped': 0}


@pytest.mark.parametrize('ending', ['banded', 'one_shot', 'pageable'])
@pytest.mark.parametrize('limit', [1, 5])
@pytest.mark.parametrize('name,border,feather', [('20_300x412', 16, 4), ('20_224x336', 8, 8), ('60_396x540', 12, 12), ('60_396x540', 18, None)])
def test_every_ending_and_batch_size(model_dir, monkeypatch, name, border, feather, limit, ending):
    from dsen2_amd import supres
    from dsen2_amd.DSen2Net import S2Model
    want = restated(name, border, feather)
    monkeypatch.setattr(supres, 'PINNED_OUTPUT_MIN_BYTES', 0)
    monkeypatch.delenv('DSEN2_BANDED_OUTPUT', raising=False)
    monkeypatch.delenv('DSEN2_PINNED_OUTPUT', raising=False)
    if ending == 'one_shot':
        monkeypatch.setenv('DSEN2_BANDED_OUTPUT', '0')
    if ending == 'pageable':
        monkeypatch.setenv('DSEN2_PINNED_OUTPUT', '0')
    monkeypatch.setattr(S2Model, 'batch_limit', lambda self, hh, ww: limit)
    assert same_bits(run_case(name, border, feather), want), (name, ending, limit)


@pytest.mark.parametrize('name,border,feather', [('20_300x412', 16, 4), ('60_396x540', 12, 12)])
def test_self_ensemble_and_the_module_switches(model_dir, monkeypatch, name, border, feather):
    from dsen2_amd import supres
    monkeypatch.setattr(supres, 'SELF_ENSEMBLE', True)
    got = run_case(name, border, feather)
    assert same_bits(got, restated(name, border, feather, ensemble=True))
    monkeypatch.setattr(supres, 'BORDER_60' if name.startswith('60') else 'BORDER_20', border)
    monkeypatch.setattr(supres, 'FEATHER', feather)
    assert same_bits(run_case(name, None, None), got)                     # None reads the module switches


@pytest.mark.parametrize('name,border,feather', [('20_300x412', 8, 8), ('20_300x412', 16, 4), ('20_224x336', 16, None), ('60_396x540', 12, 12)])
def test_skip_nodata_equals_the_restatement_with_the_slot_map(model_dir, name, border, feather):
    from dsen2_amd import supres
    want = restated(name, border, feather, nodata=True)
    got = run_case(name, border, feather, skip_nodata=True, nodata=True)
    assert same_bits(got, want), (name, int((got != want).sum()))
    assert supres.last_run_stats()['skipped'] >= 2 and not got[~nr.valid_pixels(case_inputs(name, True)[1][0])].any()


@pytest.mark.parametrize('name', list(CASES))
def test_with_both_knobs_off_the_image_and_the_prints_are_the_reference_pipeline(model_dir, monkeypatch, name):
    """border=None, feather=None and no environment switch: the hard cut at 8 / 12 of the unchanged path — the reference chain
    restated on predict — and the printed lines of before."""
    from dsen2_amd import supres
    for var in ('DSEN2_BORDER_20', 'DSEN2_BORDER_60', 'DSEN2_FEATHER'):
        assert os.environ.get(var, '') == ''
    fn_name, args, patch = case_inputs(name)
    border = 12 if patch == 192 else 8
    out, printed = quiet(getattr(supres, fn_name), *args, deep=False)
    assert same_bits(out, restated(name, border, None))
    stem = 's2_030_lr_1e-05' if patch == 192 else 's2_032_lr_1e-04'
    assert printed == 'Symbolic Model Created.\nPredicting using file: %s%s.hdf5\n(%d, %d, %d)\n' % (supres.MDL_PATH, stem, out.shape[2], out.shape[0], out.shape[1])
    again, printed_again = quiet(getattr(supres, fn_name), *args, deep=False, border=border, feather=0)
    assert same_bits(again, out) and printed_again == printed


def test_recompose_images_with_feather():
    rng = np.random.default_rng(3)
    a = rng.standard_normal((12, 6, P, P)).astype(np.float32)
    got, printed = quiet(patches.recompose_images, a, BORDER, size=(19, 27), feather=3)
    assert printed == '(6, 19, 27)\n' and same_bits(got, br.blend(a, BORDER, 3, 19, 27, 1.0))
    one, _ = quiet(patches.recompose_images, a[:1], BORDER, size=(8, 8), feather=3)          # the single-patch shortcut stays
    assert np.array_equal(one, a[0].transpose(1, 2, 0))


# ---- two gloo ranks sharing the GPU ------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return str(p)


@pytest.mark.parametrize('chunked', [False, True])
def test_two_ranks_equal_the_single_rank_image(chunked):
    """tools/bench_seam_blend.py under two gloo ranks on a 600^2 tile: (8, 8), (16, hard cut), (16, 4) and (8, 8) with skip_nodata on
    a half-empty tile.  The ranks send crops of side inner + 2 F; rank 0's images equal the single-rank ones bit for bit."""
    env = dict(os.environ)
    env.pop('DSEN2_CHUNKED_GATHER', None)
    if chunked:
        env['DSEN2_CHUNKED_GATHER'] = '1'
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2', '--master-addr', '127.0.0.1',
           '--master-port', _free_port(), os.path.join(ROOT, 'tools', 'bench_seam_blend.py'), '--size', '600', '--backend', 'gloo', '--check']
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    assert p.returncode == 0, p.stderr[-2000:]
    r = json.loads([line for line in p.stdout.splitlines() if line.startswith('{')][0])
    assert r['n_gpus'] == 2 and r['chunked_gather'] is chunked and r['jobs'] == 4
    assert r['matches_single_rank'] is True


# ---- exact seams -------------------------------------------------------------------------------------------------------------------
def _untiled_forward(args, flat):
    """The float64 oracle on the untiled inputs: the whole low-resolution images up-sampled in one piece at exact (float64)
    sample positions — the mathematical definition; skimage's float32 coordinates round differently for every origin, so no
    whole-image evaluation of them is what any patch computes (that reading moves the 60 m figures below from 2.9e-6 to 5.6e-6
    for every border alike) — then one forward over the whole image.  (The network pads with zeros, the tiling with a mirror:
    both reach 15 / 17 pixels into the image — the receptive-field radius 14 plus the up-sampler's 1 / 3 — so pixels 32 from
    the edge see neither.)"""
    from oracle import c_oracle
    from oracle import patches_oracle as po
    H, W = args[0].shape[:2]
    xs = [args[0].astype(np.float32).transpose(2, 0, 1)[None]]
    for lr in args[1:]:
        xs.append(po.interp_patches(lr.astype(np.float32).transpose(2, 0, 1)[None], (1, lr.shape[2], H, W), f32_coords=False))
    xs = [x / np.float32(2000) for x in xs]
    return c_oracle.forward(xs, flat, 6, 128)[0].transpose(1, 2, 0) * 2000.0


@pytest.mark.parametrize('name,wide,narrow', [('20_300x412', 16, 8), ('60_396x540', 18, 12)])
def test_a_border_beyond_the_receptive_field_removes_the_seams(model_dir, name, wide, narrow):
    """fp32, hard cut, against the untiled float64 forward on the pixels at least 32 from the image edge: with a border of 16 /
    18 no kept pixel sees a patch edge (it can depend on what lies 15 / 17 pixels inside it) and only the fp32 arithmetic and
    the up-sampler's float32 coordinates are left — inside the project's gate of 1e-4 — and the figure is smaller than at 8 / 12.
    Measured on an MI355X, normalised rmse (synthetic He-uniform weights, uniform random rasters):
        DSen2_20   border 16: 1.18e-06    border  8: 1.39e-05
        DSen2_60   border 18: 2.85e-06    border 12: 2.94e-06    (6: 4.8e-04, 24: 2.96e-06, 30: 3.06e-06)
    8 and 12 pass the gate as well; the inequality is kept.  On the 60 m path it is narrow: what a border of 12 lets through
    (depth 13 .. 17 of a patch, through at least 13 convolutions and the residual scaling of 0.1) is smaller than the error
    floor of the x3 / x6 up-sampling at float32 coordinates, which every border shares."""
    from dsen2_amd import supres
    fn_name, args, patch = case_inputs(name)
    flat = np.load(os.path.join(model_dir, 's2_030_lr_1e-05.npy' if patch == 192 else 's2_032_lr_1e-04.npy'))
    ref = _untiled_forward(args, flat)[32:-32, 32:-32]
    err = {}
    for border in (wide, narrow):
        out, _ = quiet(getattr(supres, fn_name), *args, deep=False, border=border)
        d = out[32:-32, 32:-32].astype(np.float64) - ref
        err[border] = float(np.sqrt(np.mean(d * d))) / 2000.0
        print('%s border %d: normalised rmse to the untiled forward %.3e' % (fn_name, border, err[border]))
    assert err[wide] < RMSE_GATE_NORMALISED, err
    assert err[wide] < err[narrow], err
