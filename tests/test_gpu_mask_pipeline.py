"""Class masks end to end on the GPU.  Prediction: DSen2_20 / DSen2_60 with mask= against where(valid, the image without a mask, 0),
valid by the numpy restatement (tests/valid_mask_restatement.py), for every precision, with skip_nodata, feather and self-ensemble,
and over two gloo ranks.  Training: fit_corpus on a corpus with class masks against the same run on a corpus whose ground truth
numpy zeroed with the restated mask; skip_masked against the restated origin bitmap.  Everything is an equality."""
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
import corpus_mask_restatement as cm  # noqa: E402
import nodata_restatement as nr  # noqa: E402
import valid_mask_restatement as vr  # noqa: E402

from dsen2_amd import corpus, masks, training, weights  # noqa: E402
from dsen2_amd.DSen2Net import s2model  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
TABLE = masks.lut(masks.SCL_INVALID)


# ---- prediction ------------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def model_dir(tmp_path, monkeypatch):
    """A MDL_PATH holding synthetic checkpoints under the reference's file names (as .npy), as tests/test_gpu_nodata.py's."""
    from dsen2_amd import supres
    np.save(str(tmp_path / 's2_032_lr_1e-04.npy'), weights.random_he_uniform(10, 6, 6, 128, seed=11))
    np.save(str(tmp_path / 's2_030_lr_1e-05.npy'), weights.random_he_uniform(12, 2, 6, 128, seed=12))
    monkeypatch.setattr(supres, 'MDL_PATH', str(tmp_path) + os.sep)
    supres.clear_model_cache()
    yield str(tmp_path)
    supres.clear_model_cache()


def quiet(fn, *a, **k):
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        out = fn(*a, **k)
    return out, buf.getvalue()


# name -> (run_60, H, W, ratio of the class raster's grid to the 10 m grid): the smallest tiles with more than one patch per axis
# (2 x 3 patches, exactly; 300 x 412: 3 x 4 with a clamped last row and column) and a class raster at 20, 60, 10 and 60 m
CASES = {'20_224x336_scl20': (False, 224, 336, 2), '60_336x504_scl60': (True, 336, 504, 6), '20_300x412_scl10': (False, 300, 412, 1),
         '20_300x412_scl60': (False, 300, 412, 6)}


def class_raster(H, W, ratio, inner):
    """uint8 [ceil(H / ratio), ceil(W / ratio)] of SCL classes: cloud (9) over the whole owned rectangle of patch (0, 0) and 12 to 24
    pixels beyond it — more than any feather width used here, so that no valid pixel takes weight from the skipped patch — a
    shadow band (3) across the second tile row, a cirrus column (10), single defective pixels (1), valid classes elsewhere."""
    hs, ws = -(-H // ratio), -(-W // ratio)
    rng = np.random.default_rng(H + W + ratio)
    cls = rng.choice(np.array([2, 4, 5, 6, 7, 11], np.uint8), size=(hs, ws))
    cls[:(inner + 12) // ratio + 1, :(inner + 12) // ratio + 1] = 9
    cls[(inner + 40) // ratio:(inner + 52) // ratio, :] = 3
    cls[:, (inner + 70) // ratio:(inner + 76) // ratio] = 10
    cls[hs - 1, ws - 1] = cls[hs - 2, 1] = 1
    return cls


def case_inputs(name, holes=False):
    """(function, [d10, d20(, d60)] uint16, class raster, inner); holes: a no-data block in d10 that the mask does not cover."""
    run_60, H, W, ratio = CASES[name]
    inner = 168 if run_60 else 112
    rng = np.random.default_rng(H + W)
    d10 = rng.integers(35, 9000, size=(H, W, 4), dtype=np.uint16)
    if holes:
        d10[H - 40:H - 10, 20:W // 2] = 0
    args = [d10, rng.integers(35, 9000, size=(H // 2, W // 2, 6), dtype=np.uint16)]
    if run_60:
        args.append(rng.integers(35, 9000, size=(H // 6, W // 6, 2), dtype=np.uint16))
    return ('DSen2_60' if run_60 else 'DSen2_20'), args, class_raster(H, W, ratio, inner), inner


def restated_valid(cls, H, W, dilate=0, classes=masks.SCL_INVALID):
    up, down = masks.ratio(cls.shape, (H, W))
    return vr.valid_pixels(cls, vr.lut(classes), up, down, H, W, dilate)


def check_case(name, dilate=0, holes=False, **kw):
    """R_mask == where(valid, R_without_mask, 0) bit for bit, the same prints, and the skipped count of the restatement."""
    from dsen2_amd import supres
    fn_name, args, cls, inner = case_inputs(name, holes)
    fn = getattr(supres, fn_name)
    H, W = args[0].shape[:2]
    valid = restated_valid(cls, H, W, dilate)
    if kw.get('skip_nodata'):
        valid = valid & nr.valid_pixels(args[0])
    empty = nr.patch_empty(valid, inner)
    n, skipped = empty.size, int((empty != 0).sum())
    own = nr.owner_map(H, W, inner)
    partly = sum(1 for k in range(n) if valid[own == k].any() and not valid[own == k].all())
    assert 1 <= skipped < n and partly >= 2, (name, n, skipped, partly)       # one whole patch is masked, others are cut through
    plain = dict((k, v) for k, v in kw.items() if k in ('feather', 'border'))
    off, printed_off = quiet(fn, *args, deep=False, **plain)
    assert supres.last_run_stats() == {'patches': n, 'kept': n, 'skipped': 0}
    on, printed_on = quiet(fn, *args, deep=False, mask=cls, mask_dilate=dilate, **kw)
    assert supres.last_run_stats() == {'patches': n, 'kept': n - skipped, 'skipped': skipped}
    assert on.shape == off.shape == (H, W, off.shape[2]) and on.dtype == np.float32
    want = np.where(valid[:, :, None], off, np.float32(0))
    assert np.array_equal(on.view(np.int32), want.view(np.int32)), (name, int((on != want).sum()))
    assert np.abs(off[~valid]).max() > 0 and printed_on == printed_off
    return on, off, args, cls, valid


@pytest.mark.parametrize('precision', ['fp32', 'bf16', 'bf16x3'])
@pytest.mark.parametrize('name', list(CASES))
def test_masked_image_is_the_plain_image_with_the_invalid_pixels_zeroed(model_dir, monkeypatch, name, precision):
    from dsen2_amd import supres
    monkeypatch.setattr(supres, 'PRECISION', precision)
    check_case(name)


@pytest.mark.parametrize('name', ['20_224x336_scl20', '60_336x504_scl60', '20_300x412_scl60'])
def test_dilation_skip_nodata_and_other_classes(model_dir, name):
    from dsen2_amd import supres
    check_case(name, dilate=3)
    on, off, args, cls, valid = check_case(name, dilate=2, holes=True, skip_nodata=True)
    assert not nr.valid_pixels(args[0])[valid.shape[0] - 20, 30] and not on[valid.shape[0] - 20, 30].any()
    # classes of the caller's: cloud alone
    fn = getattr(supres, case_inputs(name)[0])
    cloud, _ = quiet(fn, *case_inputs(name)[1], mask=cls, mask_classes=(9,))
    only9 = restated_valid(cls, valid.shape[0], valid.shape[1], 0, (9,))
    plain, _ = quiet(fn, *case_inputs(name)[1])
    assert np.array_equal(cloud.view(np.int32), np.where(only9[:, :, None], plain, np.float32(0)).view(np.int32))


@pytest.mark.parametrize('name,feather', [('20_224x336_scl20', 4), ('20_224x336_scl20', True), ('60_336x504_scl60', 6)])
def test_feather(model_dir, name, feather):
    """The mask reaches further past the skipped patch than the blend is wide, so every valid pixel blends the patches it always
    blended.  (A valid pixel within the feather width of a skipped patch blends the patches that are left, as under skip_nodata.)"""
    check_case(name, feather=feather)


@pytest.mark.parametrize('name', ['20_224x336_scl20', '60_336x504_scl60'])
def test_self_ensemble_and_every_ending(model_dir, monkeypatch, name):
    from dsen2_amd import supres
    from dsen2_amd.DSen2Net import S2Model
    monkeypatch.setattr(supres, 'SELF_ENSEMBLE', True)
    check_case(name)
    monkeypatch.setattr(supres, 'SELF_ENSEMBLE', False)
    monkeypatch.setattr(supres, 'PINNED_OUTPUT_MIN_BYTES', 0)
    monkeypatch.setattr(S2Model, 'batch_limit', lambda self, hh, ww: 2)
    for ending in ('banded', 'one_shot', 'pageable'):
        monkeypatch.delenv('DSEN2_BANDED_OUTPUT', raising=False)
        monkeypatch.delenv('DSEN2_PINNED_OUTPUT', raising=False)
        if ending == 'one_shot':
            monkeypatch.setenv('DSEN2_BANDED_OUTPUT', '0')
        if ending == 'pageable':
            monkeypatch.setenv('DSEN2_PINNED_OUTPUT', '0')
        check_case(name)


def test_mask_none_is_the_call_without_the_arguments(model_dir):
    from dsen2_amd import supres
    fn_name, args, cls, inner = case_inputs('20_224x336_scl20')
    a, pa = quiet(supres.DSen2_20, *args)
    b, pb = quiet(supres.DSen2_20, *args, mask=None, mask_classes=None, mask_dilate=0)
    assert np.array_equal(a.view(np.int32), b.view(np.int32)) and pa == pb
    assert supres.last_run_stats()['skipped'] == 0
    # a mask that marks nothing: the same image through the bitmap path
    c, _ = quiet(supres.DSen2_20, *args, mask=np.full(cls.shape, 4, np.uint8))
    assert np.array_equal(a.view(np.int32), c.view(np.int32)) and supres.last_run_stats()['skipped'] == 0
    # one that marks everything: zeros, and no forward
    z, _ = quiet(supres.DSen2_20, *args, mask=np.full(cls.shape, 9, np.uint8))
    assert not z.any() and z.shape == a.shape and supres.last_run_stats()['kept'] == 0


def test_refusals(model_dir, monkeypatch):
    from dsen2_amd import patches, supres
    fn_name, args, cls, inner = case_inputs('20_224x336_scl20')
    for kw in (dict(mask=cls.astype(np.int16)), dict(mask=cls[None]), dict(mask=cls[:, :100]), dict(mask=cls, mask_dilate=33),
               dict(mask=cls, mask_dilate=-1), dict(mask=cls, mask_classes=(256,)), dict(mask=np.zeros((10, 10), np.uint8))):
        with pytest.raises(ValueError):
            quiet(supres.DSen2_20, *args, **kw)
    # the single-patch shortcut (one allocated patch, returned uncropped: no legal extent of the two geometries reaches it) refuses
    # a mask, as it refuses skip_nodata on an image that is not the patch
    real = patches.tile_origins
    monkeypatch.setattr(patches, 'tile_origins', lambda *a: (real(*a)[0][:1], 1))
    with pytest.raises(ValueError, match='single-patch'):
        quiet(supres.DSen2_20, *args, mask=cls)


def test_cli_mask_from_the_npz_and_from_a_file(model_dir, tmp_path):
    from dsen2_amd import cli, supres
    on, off, args, cls, valid = check_case('20_224x336_scl20', dilate=2)
    inp, out = str(tmp_path / 'tile.npz'), str(tmp_path / 'sr.npz')
    np.savez(inp, data10=args[0], data20=args[1], scl=cls)
    np.save(str(tmp_path / 'scl.npy'), cls)
    for spec in ('scl', str(tmp_path / 'scl.npy')):
        rc, _ = quiet(cli.main, [inp, out, '--mask', spec, '--mask_dilate', '2', '--models', supres.MDL_PATH])
        assert rc == 0
        bands = np.load(out, allow_pickle=True)['bands'].item()
        for i, b in enumerate(bands.values()):
            assert np.array_equal(b, on[:, :, i])


def test_apply_to_image_is_numpys_where():
    """What `train.py --predict --mask` does to the image it recomposed on the host."""
    rng = np.random.default_rng(4)
    image = rng.standard_normal((90, 132, 6)).astype(np.float32)
    cls = class_raster(90, 132, 6, 40)
    for classes, dilate in ((None, 0), ((9, 10), 3)):
        got = masks.apply_to_image(image, cls, classes, dilate)
        valid = restated_valid(cls, 90, 132, dilate, masks.SCL_INVALID if classes is None else classes)
        assert 0 < valid.mean() < 1 and got.dtype == np.float32
        assert got.tobytes() == np.where(valid[:, :, None], image, np.float32(0)).tobytes()


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return str(p)


def test_two_ranks_equal_the_single_rank_image():
    """tools/bench_valid_mask.py under two gloo ranks on a 600^2 tile (36 patches) with a diagonal half masked: plain, with
    skip_nodata and a dilation, and with feather.  Rank 0's images equal the single-rank images and (hard cut)
    where(valid, no mask, 0); rank 1 returns None (the tool asserts it)."""
    env = dict(os.environ)
    env.pop('DSEN2_CHUNKED_GATHER', None)
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2', '--master-addr', '127.0.0.1',
           '--master-port', _free_port(), os.path.join(ROOT, 'tools', 'bench_valid_mask.py'), '--size', '600', '--backend', 'gloo',
           '--check']
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    assert p.returncode == 0, p.stderr[-2000:]
    r = json.loads([line for line in p.stdout.splitlines() if line.startswith('{')][0])
    assert r['n_gpus'] == 2 and r['on']['plain']['patches'] == 36
    assert 12 < r['on']['plain']['kept'] < 30 and r['on']['nodata_dilate']['kept'] < r['on']['plain']['kept']
    assert r['matches_single_rank'] is True and r['matches_masked_off'] is True


# ---- training ----------------------------------------------------------------------------------------------------------------------
BANDS, D, F = (4, 6), 1, 128
BATCH, STEPS, SEED = 4, 2, 17


def _tiles20():
    """The grids of the corpus tests: 24 x 40 uint16 and 33 x 17 float32."""
    rng = np.random.default_rng(1)
    tiles = []
    for (gh, gw), dtype in (((24, 40), np.uint16), ((33, 17), np.float32)):
        tiles.append(tuple(rng.integers(200, 12000, (gh * f, gw * f, c)).astype(dtype) for f, c in ((4, 4), (2, 6))))
    return tiles


def _class_masks(band=False):
    """One raster per tile: the first on the 20 m grid of its ground truth [48, 80], the second on the 60 m grid of [66, 34]
    (up = 3, 22 x 12 with a partial last column).  band: also a cloud band that every crop of either tile crosses."""
    rng = np.random.default_rng(2)
    a = rng.choice(np.array([4, 5, 6], np.uint8), size=(48, 80))
    a[5:9, 60:70], a[40, 3], a[0, 0] = 9, 3, 1
    b = rng.choice(np.array([4, 5, 6], np.uint8), size=(22, 12))
    b[20:, :3], b[2, 11] = 8, 10
    if band:
        a[20:26, :], b[10:12, :] = 9, 9
    return [a, b]


def _model(mixed_precision=None, mask_nodata=True):
    m = s2model(tuple((c, None, None) for c in BANDS), num_layers=D, feature_size=F, device=DEV)
    m.set_weights_flat(weights.random_he_uniform(sum(BANDS), BANDS[-1], D, F, seed=5, bias_scale=0.05))
    m.compile(training.Nadam(lr=1e-3), mixed_precision=mixed_precision, mask_nodata=mask_nodata)
    return m


def _zeroed_by_numpy(tiles, class_masks, dilate):
    """A corpus of the unmasked tiles whose ground truth numpy zeroed with the restated mask, in place on the device."""
    c = corpus.TileCorpus(tiles, device=DEV)
    valids = []
    for i, (gt, cls) in enumerate(zip(c.gt, class_masks)):
        H, W = int(gt.shape[0]), int(gt.shape[1])
        valid = restated_valid(cls, H, W, dilate)
        host = gt.cpu().numpy()
        host[~valid] = 0
        gt.copy_(torch.from_numpy(host))
        valids.append(valid)
    return c, valids


@pytest.mark.parametrize('mixed', [None, 'bf16'])
def test_fit_corpus_on_class_masks_is_fit_corpus_on_a_zeroed_ground_truth(mixed):
    tiles, class_masks, dilate = _tiles20(), _class_masks(band=True), 1
    masked = corpus.TileCorpus(tiles, device=DEV, class_masks=class_masks, mask_dilate=dilate)
    assert masked.class_masked is True
    ref, valids = _zeroed_by_numpy(tiles, class_masks, dilate)
    plain = corpus.TileCorpus(tiles, device=DEV)
    assert plain.class_masked is False
    for i, valid in enumerate(valids):
        assert 0.5 < valid.mean() < 1
        got, want, was = masked.gt[i].cpu().numpy(), ref.gt[i].cpu().numpy(), plain.gt[i].cpu().numpy()
        assert got.tobytes() == want.tobytes() and not got[~valid].any() and got[valid].tobytes() == was[valid].tobytes()
        for a, b in zip(masked.lr[i], plain.lr[i]):
            assert torch.equal(a, b)                                              # the inputs are not touched
    table = masked.validation_table(2, SEED)
    a, b = _model(mixed), _model(mixed)
    logs_a, logs_b = [], []

    class Log(training.Callback):
        def __init__(self, sink):
            super().__init__()
            self.sink = sink

        def on_epoch_end(self, epoch, logs=None):
            self.sink.append(sorted((k, repr(v)) for k, v in logs.items()))
    ha = a.fit_corpus(masked, BATCH, STEPS, epochs=1, validation_crops=table, seed=SEED, augment=True, verbose=0, callbacks=[Log(logs_a)])
    hb = b.fit_corpus(ref, BATCH, STEPS, epochs=1, validation_crops=table, seed=SEED, augment=True, verbose=0, callbacks=[Log(logs_b)])
    wa, wb = a.get_weights_flat(), b.get_weights_flat()
    assert wa.tobytes() == wb.tobytes(), '%d of %d weights differ' % (int((wa != wb).sum()), wa.size)
    assert logs_a == logs_b and ha.history == hb.history and len(logs_a) == 1
    # and the mask did something: the same steps on the unmasked tiles end elsewhere
    c = _model(mixed)
    c.fit_corpus(plain, BATCH, STEPS, epochs=1, validation_crops=table, seed=SEED, augment=True, verbose=0)
    assert c.get_weights_flat().tobytes() != wa.tobytes()
    # a model that would train on the zeros is refused, by fit_corpus and by fit on arrays cut from the corpus
    loose = _model(mixed, mask_nodata=False)
    with pytest.raises(ValueError, match='mask_nodata'):
        loose.fit_corpus(masked, BATCH, STEPS, verbose=0)
    xs, y = masked.table_arrays(table)
    assert isinstance(y, training.MaskedTarget) and not isinstance(plain.table_arrays(table)[1], training.MaskedTarget)
    with pytest.raises(ValueError, match='mask_nodata'):
        loose.fit(xs, y, batch_size=BATCH, epochs=1, verbose=0)


def test_skip_masked_draws_no_crop_that_touches_the_mask(capsys):
    tiles, class_masks, dilate = _tiles20(), _class_masks(), 1
    tiles[0][0][:, :16, 0] = 0                                           # and four blank cell columns in the first tile
    for skip_blank in (False, True):
        c = corpus.TileCorpus(tiles, device=DEV, class_masks=class_masks, mask_dilate=dilate, skip_masked=True, skip_blank=skip_blank)
        printed = capsys.readouterr().out
        assert printed.count('origins free of %s pixels' % ('blank and masked' if skip_blank else 'masked')) == 2
        bitmaps, counts = c.origin_masks()
        for i, (tile, cls, grid) in enumerate(zip(tiles, class_masks, c.extents)):
            valid = restated_valid(cls, 2 * grid[0], 2 * grid[1], dilate)
            cells = vr.cells(valid, 2)
            if skip_blank:
                cells = cells | cm.origin_mask(tile[0], grid, 4)[2]
            assert np.array_equal(c.blank_cells[i].cpu().numpy() != 0, cells != 0)
            ok = np.array([[not cells[oy:oy + 16, ox:ox + 16].any() for ox in range(grid[1] - 15)] for oy in range(grid[0] - 15)])
            want = np.packbits(ok, axis=1, bitorder='little')
            assert bitmaps[i].tobytes() == want.tobytes() and counts[i] == int(ok.sum()) and 0 < counts[i] < ok.size
        sampler = corpus.CorpusSampler(c, seed=SEED, augment=True, masks=bitmaps)
        table = sampler.draw(64)
        xs, y = c.batch(table)
        y = y.cpu().numpy()
        assert (y != 0).any(axis=1).all()                                  # every drawn crop is mask-free: no no-data pixel in it
        loose = corpus.CorpusSampler(c, seed=SEED, augment=True).draw(64)
        _, y_loose = c.batch(loose)
        assert not (y_loose.cpu().numpy() != 0).any(axis=1).all()          # without the bitmaps crops do touch the mask
