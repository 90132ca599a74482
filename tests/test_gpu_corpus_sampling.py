"""Drawing crops with origin masks and validating on the device, on the GPU: dsen2_corpus_origin_mask against a numpy restatement
of its definitions (bitmap bytes, count and cell map equal) inside guard bands; dsen2_abs_sq_error_sums against a restatement of
its summation order, bit for bit, and against np.sum within the bound between two orders; S2Model.fit_corpus(validation_crops=)
against the host-array validation; the hold-out property; and the command line."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import corpus_mask_restatement as cm  # noqa: E402
import trainset_fixtures as fx  # noqa: E402
from guarded import run_three_ways  # noqa: E402

from dsen2_amd import _lib, corpus, dist, patches, train, training, weights  # noqa: E402
from dsen2_amd.DSen2Net import S2Model, s2model  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)


# ---- 1. the origin mask ----------------------------------------------------------------------------------------------------------
# (grid, footprint, dtype, bands): windows and packed bytes that cross the 16 x 64 workgroup tiles and a ragged last byte (24 x 40:
# 25 origins per row; 70 x 33: 55 rows of 18), ONE origin (16 x 16), the 60 m footprint, one band
CASES = [((24, 40), 4, np.uint16, 4), ((70, 33), 4, np.uint16, 4), ((16, 16), 4, np.uint16, 4), ((18, 20), 36, np.float32, 4),
         ((24, 40), 4, np.float32, 1), ((20, 95), 4, np.uint16, 1)]
BLANKS = ['none', 'corners', 'cell_edge', 'stripe', 'all']


def _raster(grid, f, dtype, c, blanks, seed=0):
    gh, gw = grid
    rng = np.random.default_rng(seed)
    a = rng.integers(200, 12000, (gh * f, gw * f, c)).astype(dtype)
    if c > 1:
        a[::3, ::5, 1:] = 0                      # the other bands are not looked at
    a[1, 2, 0] = 1                               # 1 itself is not blank
    low = (0, np.nan, 0.5) if dtype == np.float32 else (0, 0, 0)
    if blanks == 'corners':
        a[0, 0, 0], a[0, -1, 0], a[-1, 0, 0], a[-1, -1, 0] = low[0], low[1], low[2], low[0]
    elif blanks == 'cell_edge':                  # the last row of one cell's footprint, the last column of another's
        a[f * (gh - 3) + f - 1, f * 2 + 1, 0] = low[1]
        a[f * 1, f * (gw - 2) + f - 1, 0] = low[2]
    elif blanks == 'stripe':
        a[f * (gh // 2) + 1, :, 0] = low[0]
    elif blanks == 'all':
        a[:, :, 0] = low[0]
    return a


def _holdouts(grid):
    gh, gw = grid
    last = (gh - 16, gw - 16)
    five = [(0, 0), last, (last[0] // 2, last[1] // 2), (0, last[1]), last]
    return [([], 0), ([last], 0), (five, 0), ([(0, 0)], 3), (five[1:4], 3)]


def _upload(a):
    return patches.upload_raster(a, DEV)[0]


def _mask_call(grid, f, holdout, margin):
    rows = np.asarray(holdout, np.int32).reshape(-1, 2)

    def call(inp, out, _inplace, scratch):
        corpus.origin_mask_device(inp[0], grid, f, rows, margin, holdout_dev=inp[1], out=(scratch[0], out[0], out[1]))
    return rows, call


@pytest.mark.parametrize('blanks', BLANKS)
@pytest.mark.parametrize('grid,f,dtype,c', CASES)
def test_origin_mask_equals_the_restatement(grid, f, dtype, c, blanks):
    a = _raster(grid, f, dtype, c, blanks)
    src = _upload(a)
    cells_shape, bitmap_shape = corpus.mask_shapes(grid)
    for holdout, margin in _holdouts(grid):
        what = 'grid %r F %d %s C %d, blanks %s, hold-out %r margin %d' % (grid, f, np.dtype(dtype).name, c, blanks, holdout, margin)
        rows, call = _mask_call(grid, f, holdout, margin)
        inputs = [src, torch.from_numpy(rows).to(DEV) if rows.shape[0] else None]
        (bitmap, count), _ = run_three_ways(call, inputs, [(bitmap_shape, torch.uint8), ((1,), torch.int32)],
                                            scratch=[(cells_shape, torch.uint8)], device=DEV, what=what)
        want_bitmap, want_count, want_cells = cm.origin_mask(a, grid, f, holdout, margin)
        assert bitmap.cpu().numpy().tobytes() == want_bitmap.tobytes(), what
        assert int(count.cpu()) == want_count, what
        cells, _, _ = corpus.origin_mask_device(src, grid, f, rows, margin)
        assert np.array_equal(cells.cpu().numpy(), want_cells), what
        if blanks == 'all':
            assert want_count == 0 and not bitmap.any()
        if blanks == 'none' and not holdout:
            assert want_count == (grid[0] - 15) * (grid[1] - 15)


def test_origin_mask_from_a_kept_blank_map_equals_the_mask_from_the_raster():
    grid, f = (70, 33), 4
    a = _raster(grid, f, np.uint16, 4, 'cell_edge')
    src = _upload(a)
    blank, _, _ = corpus.origin_mask_device(src, grid, f)
    cells_shape, bitmap_shape = corpus.mask_shapes(grid)
    for holdout, margin in _holdouts(grid)[1:]:
        rows, call = _mask_call(grid, f, holdout, margin)
        (bitmap, count), _ = run_three_ways(call, [blank, torch.from_numpy(rows).to(DEV)], [(bitmap_shape, torch.uint8), ((1,), torch.int32)],
                                            scratch=[(cells_shape, torch.uint8)], device=DEV, what='blank map, hold-out %r' % (holdout,))
        _, direct, direct_count = corpus.origin_mask_device(src, grid, f, rows, margin)
        assert torch.equal(bitmap, direct) and int(count.cpu()) == int(direct_count.cpu())
        want_bitmap, want_count, _ = cm.origin_mask(a, grid, f, holdout, margin)
        assert bitmap.cpu().numpy().tobytes() == want_bitmap.tobytes() and int(count.cpu()) == want_count
    with pytest.raises(ValueError, match='two buffers'):
        corpus.origin_mask_device(blank, grid, f, out=(blank, torch.empty(bitmap_shape, dtype=torch.uint8, device=DEV),
                                                      torch.empty(1, dtype=torch.int32, device=DEV)))
    with pytest.raises(_lib.DSen2Error, match='hold-out origin 0'):
        corpus.origin_mask_device(src, grid, f, np.asarray([[55, 0]], np.int32))


def _tiles20(blank=True):
    """The grids of the corpus tests (24 x 40 uint16, 33 x 17 float32), the left 12 cell columns of the first and the top 6 cell rows
    of the second blank in band 0."""
    rng = np.random.default_rng(1)
    tiles = []
    for (gh, gw), dtype in (((24, 40), np.uint16), ((33, 17), np.float32)):
        tiles.append([rng.integers(200, 12000, (gh * f, gw * f, c)).astype(dtype) for f, c in ((4, 4), (2, 6))])
    if blank:
        tiles[0][0][:, :48, 0] = 0
        tiles[1][0][:24, :, 0] = 0.5
    return [tuple(t) for t in tiles]


def test_tile_corpus_keeps_the_blank_masks(capsys):
    tiles = _tiles20()
    plain = corpus.TileCorpus(tiles, device=DEV)
    assert capsys.readouterr().out == ''
    c = corpus.TileCorpus(tiles, device=DEV, skip_blank=True)
    want = [cm.origin_mask(t[0], g, 4) for t, g in zip(tiles, c.extents)]
    said = capsys.readouterr().out.splitlines()
    assert said == ['tile %d: %d of %d origins free of blank pixels' % (i, w[1], (g[0] - 15) * (g[1] - 15))
                    for i, (w, g) in enumerate(zip(want, c.extents))]
    assert [w[1] for w in want] == [9 * 13, 12 * 2]
    bitmaps, counts = c.origin_masks()
    assert counts == [w[1] for w in want] and all(b.tobytes() == w[0].tobytes() for b, w in zip(bitmaps, want))
    assert all(np.array_equal(b.cpu().numpy(), w[2]) for b, w in zip(c.blank_cells, want))
    # the corpus itself is the one without the option
    assert all(torch.equal(a, b) for la, lb in zip(c.lr, plain.lr) for a, b in zip(la, lb)) and all(torch.equal(a, b) for a, b in zip(c.gt, plain.gt))
    # with a hold-out: the cell map is rebuilt from the kept blank map and the rectangles of each tile's rows
    # (on grids this small a crop takes every origin row of the wide tile and 16 + margin of the tall tile's 18: the hold-out
    # crops sit at the edge so that 1 origin in 64 is left: 9 x 9 and 2 x 2 with margin 0, 9 x 8 and 1 x 2 with margin 1)
    table = np.asarray([(0, 2, 0, 0), (1, 0, 0, 0), (0, 8, 0, 0)], np.int32)
    for margin in (0, 1):
        bitmaps, counts = c.origin_masks(holdout=table, margin=margin)
        for i, (t, g) in enumerate(zip(tiles, c.extents)):
            wb, wc, _ = cm.origin_mask(t[0], g, 4, table[table[:, 0] == i, 1:3], margin)
            assert bitmaps[i].tobytes() == wb.tobytes() and counts[i] == wc
    # without skip_blank a hold-out works on an all-clear blank map
    bitmaps, counts = plain.origin_masks(holdout=table[:2])
    clear = [np.ones_like(t[0]) for t in tiles]
    for i, g in enumerate(c.extents):
        wb, wc, _ = cm.origin_mask(clear[i], g, 4, table[:2][table[:2, 0] == i, 1:3], 0)
        assert bitmaps[i].tobytes() == wb.tobytes() and counts[i] == wc
    assert plain.origin_masks()[1] == [9 * 25, 18 * 2]
    # the validation table drawn with the blank masks avoids the blank cells; the sampler too
    vt = c.validation_table(30, 3, c.origin_masks()[0])
    assert (vt[vt[:, 0] == 0, 2] >= 12).all() and (vt[vt[:, 0] == 1, 1] >= 6).all()
    tr = corpus.CorpusSampler(c, 3, masks=c.origin_masks()[0]).draw(200)
    assert (tr[tr[:, 0] == 0, 2] >= 12).all() and (tr[tr[:, 0] == 1, 1] >= 6).all()
    xs, y = c.validation_arrays(30, 3, masks=c.origin_masks()[0])
    dx, _ = c.batch(vt)
    assert xs[0].shape == (60, 4, 32, 32) and np.array_equal(xs[0], dx[0].cpu().numpy()) and y.shape == (60, 6, 32, 32)


def test_tile_corpus_refuses_a_tile_that_is_nearly_all_blank(capsys):
    tiles = _tiles20(blank=False)
    tiles[1][0][:, :, 0] = 0
    with pytest.raises(ValueError, match=r'tile 1: 0 of 36 origins are valid, fewer than 1 in 64'):
        corpus.TileCorpus(tiles, device=DEV, skip_blank=True)
    assert 'tile 1: 0 of 36 origins free of blank pixels' in capsys.readouterr().out
    c = corpus.TileCorpus(tiles, device=DEV)
    with pytest.raises(ValueError, match=r'tile 1: 0 of 36 origins are valid'):
        c.origin_masks(holdout=np.asarray([(1, 9, 0, 0)], np.int32))             # every crop of the 17-wide tile overlaps it


# ---- 2. the error sums -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('count', [1, 255, 4097, 2 * 6 * 32 * 32 * 3, 4096 * 2048 + 257])      # the last: above the grid's cap, a ninth pass
def test_error_sums_equal_the_restated_order_bit_for_bit(count):
    rng = np.random.default_rng(count)
    p = (rng.random(count, dtype=np.float32) * 5).astype(np.float32)
    t = (rng.random(count, dtype=np.float32) * 5).astype(np.float32)
    t[::7] = p[::7]                                                            # exact zeros among the differences
    need = ctypes_size()
    model = _model()

    def call(inp, out, _inplace, scratch):
        with torch.cuda.device(DEV):
            _lib.call('dsen2_abs_sq_error_sums', patches._ptr(inp[0]), patches._ptr(inp[1]), count, patches._ptr(scratch[0]),
                      scratch[0].numel(), patches._ptr(out[0]), patches._stream(DEV))
    (got,), _ = run_three_ways(call, [torch.from_numpy(p).to(DEV), torch.from_numpy(t).to(DEV)], [((2,), torch.float64)], scratch=[need],
                               device=DEV, what='error sums, count %d' % count)
    got = got.cpu().numpy()
    want = cm.abs_sq_error_sums(p, t)
    print('count %d: kernel %r restatement %r' % (count, got.tolist(), want))
    assert got.tobytes() == np.asarray(want, np.float64).tobytes()
    d = p.astype(np.float64) - t.astype(np.float64)
    for g, ref in zip(got.tolist(), (float(np.sum(np.abs(d))), float(np.sum(d * d)))):
        print('  against np.sum: %r vs %r, relative %.3e, bound %.3e' % (g, ref, abs(g - ref) / ref if ref else 0.0, cm.sums_bound(count)))
        assert abs(g - ref) <= cm.sums_bound(count) * ref
    # the wrapper gives the same pair
    out = model.abs_sq_error_sums_device(torch.from_numpy(p).to(DEV), torch.from_numpy(t).to(DEV), torch.empty(2, dtype=torch.float64, device=DEV))
    assert out.cpu().numpy().tobytes() == got.tobytes()


def ctypes_size():
    import ctypes
    need = ctypes.c_size_t(0)
    _lib.call('dsen2_abs_sq_error_sums_workspace_bytes', ctypes.byref(need))
    return int(need.value)


# ---- 3. fit_corpus(validation_crops=) ------------------------------------------------------------------------------------------------
BANDS, D, F = (4, 6), 1, 128
BATCH, STEPS, EPOCHS, SEED = 4, 3, 2, 17


def _model(mixed_precision=None):
    m = s2model(tuple((c, None, None) for c in BANDS), num_layers=D, feature_size=F, device=DEV)
    m.set_weights_flat(weights.random_he_uniform(sum(BANDS), BANDS[-1], D, F, seed=5, bias_scale=0.05))
    m.compile(training.Nadam(lr=1e-3), mixed_precision=mixed_precision)
    return m


@pytest.fixture(scope='module')
def corpus20():
    c = corpus.TileCorpus(_tiles20(blank=False), device=DEV)
    table = c.validation_table(2, SEED)
    xs, y = c.validation_arrays(2, SEED)
    dx, dy = c.batch(table)
    assert all(np.array_equal(a, t.cpu().numpy()) for a, t in zip(xs + [y], dx + [dy]))     # validation_arrays = cut validation_table
    return c, table, (xs, y)


class _AtEpochEnd(training.Callback):
    """What the host forms from predict() of the validation crops with the weights of each epoch's end."""

    def __init__(self, arrays, shards=1):
        super().__init__()
        self.arrays, self.shards, self.logs, self.restated, self.evaluated = arrays, shards, [], [], []

    def on_epoch_end(self, epoch, logs=None):
        xs, y = self.arrays
        n = y.shape[0]
        sa = sq = cnt = 0.0
        for r in range(self.shards):                                          # the triples of the shards, added in rank order
            first, k = dist.shard_range(n, r, self.shards)
            pred = self.model.predict([a[first:first + k] for a in xs])
            a, b = cm.abs_sq_error_sums(pred, y[first:first + k])             # one chunk per shard: 0.0 + the chunk's pair
            sa, sq, cnt = sa + (0.0 + a), sq + (0.0 + b), cnt + float(pred.size)
        self.restated.append([float(sa / cnt), float(sq / cnt)])
        self.evaluated.append(self.model.evaluate(xs, y))
        self.logs.append([logs['val_loss'], logs['val_mean_squared_error']])


@pytest.mark.parametrize('mixed', [None, 'bf16'])
def test_fit_corpus_validates_on_the_device(corpus20, mixed):
    c, table, arrays = corpus20
    a, b = _model(mixed), _model(mixed)
    assert a._validation_chunk(c) >= table.shape[0]                            # one chunk
    seen = _AtEpochEnd(arrays)
    ha = a.fit_corpus(c, BATCH, STEPS, epochs=EPOCHS, validation_crops=table, seed=SEED, augment=True, verbose=0, callbacks=[seen])
    hb = b.fit_corpus(c, BATCH, STEPS, epochs=EPOCHS, validation_data=arrays, seed=SEED, augment=True, verbose=0)
    wa, wb = a.get_weights_flat(), b.get_weights_flat()
    assert wa.tobytes() == wb.tobytes(), '%d of %d weights differ' % (int((wa != wb).sum()), wa.size)
    assert ha.history['loss'] == hb.history['loss'] and ha.history['mean_squared_error'] == hb.history['mean_squared_error']
    count = arrays[1].size
    for e in range(EPOCHS):
        got = [ha.history['val_loss'][e], ha.history['val_mean_squared_error'][e]]
        print('epoch %d: device %r restated %r evaluate %r host path %r' % (e, got, seen.restated[e], seen.evaluated[e],
                                                                            [hb.history['val_loss'][e], hb.history['val_mean_squared_error'][e]]))
        assert got == seen.logs[e] == seen.restated[e]
        for g, ref, host in zip(got, seen.evaluated[e], (hb.history['val_loss'][e], hb.history['val_mean_squared_error'][e])):
            assert ref == host                                                 # evaluate's numbers are the host path's
            assert abs(g - ref) <= cm.sums_bound(count) * ref
    assert ha.history['val_loss'][0] != ha.history['val_loss'][1]
    with pytest.raises(ValueError, match='exclude each other'):
        a.fit_corpus(c, BATCH, STEPS, validation_data=arrays, validation_crops=table, verbose=0)
    with pytest.raises(ValueError, match='no sample'):
        a.fit_corpus(c, BATCH, STEPS, validation_crops=table[:0], verbose=0)


def test_fit_corpus_validates_in_several_chunks(corpus20, monkeypatch):
    """A chunk of 3 crops for 4: two rows of sums, added in chunk order."""
    c, table, arrays = corpus20
    monkeypatch.setattr(S2Model, '_validation_chunk', lambda self, corp: 3)
    a = _model()
    got = []

    class Restate(training.Callback):
        def on_epoch_end(self, epoch, logs=None):
            pred = self.model.predict(arrays[0])
            sa = sq = 0.0
            for i0 in (0, 3):
                p, q = cm.abs_sq_error_sums(pred[i0:i0 + 3], arrays[1][i0:i0 + 3])
                sa, sq = sa + p, sq + q
            got.append(([logs['val_loss'], logs['val_mean_squared_error']], [sa / pred.size, sq / pred.size]))
    a.fit_corpus(c, BATCH, STEPS, epochs=EPOCHS, validation_crops=table, seed=SEED, verbose=0, callbacks=[Restate()])
    assert len(got) == EPOCHS and all(dev == host for dev, host in got), got
    # with sharded steps (gradient accumulation) the device pass is the same
    b, seen = _model(), _AtEpochEnd(arrays)
    monkeypatch.undo()
    b.fit_corpus(c, BATCH, STEPS, epochs=EPOCHS, validation_crops=table, seed=SEED, verbose=0, shards=2, callbacks=[seen])
    assert seen.logs == seen.restated


def test_fit_corpus_emulated_world_shards_the_validation_crops(corpus20):
    c, table, arrays = corpus20
    table3 = table[:3]                                                         # shards of 2 and 1
    arrays3 = ([a[:3] for a in arrays[0]], arrays[1][:3])
    assert [dist.shard_range(3, r, 2)[1] for r in (0, 1)] == [2, 1]
    a, b = _model(), _model()
    seen = _AtEpochEnd(arrays3, shards=2)
    ha = a.fit_corpus(c, BATCH, STEPS, epochs=EPOCHS, validation_crops=table3, seed=SEED, verbose=0, callbacks=[seen],
                      data_parallel=True, emulate_world=2)
    hb = b.fit_corpus(c, BATCH, STEPS, epochs=EPOCHS, validation_data=arrays3, seed=SEED, verbose=0, data_parallel=True, emulate_world=2)
    assert a.get_weights_flat().tobytes() == b.get_weights_flat().tobytes()
    assert seen.logs == seen.restated, (seen.logs, seen.restated)
    count = arrays3[1].size
    for e in range(EPOCHS):
        for g, ref in ((ha.history['val_loss'][e], hb.history['val_loss'][e]),
                       (ha.history['val_mean_squared_error'][e], hb.history['val_mean_squared_error'][e])):
            assert abs(g - ref) <= cm.sums_bound(count) * ref


# ---- 4. hold-out ---------------------------------------------------------------------------------------------------------------------
def test_no_training_crop_overlaps_a_held_out_validation_crop():
    grid = (40, 72)
    rng = np.random.default_rng(2)
    tile = (rng.integers(200, 12000, (160, 288, 4)).astype(np.uint16), rng.integers(200, 12000, (80, 144, 6)).astype(np.uint16))
    c = corpus.TileCorpus([tile], device=DEV)
    val = np.asarray([(0, 0, 0, 0), (0, 24, 56, 0), (0, 10, 30, 0)], np.int32)
    bitmaps, counts = c.origin_masks(holdout=val)
    assert counts[0] * 64 >= 25 * 57 and counts[0] == cm.origin_mask(np.ones_like(tile[0]), grid, 4, val[:, 1:3])[1]

    def overlaps(table):
        dy = np.abs(table[:, None, 1] - val[None, :, 1])
        dx = np.abs(table[:, None, 2] - val[None, :, 2])
        return int(((dy < 16) & (dx < 16)).any(axis=1).sum())
    held, free = corpus.CorpusSampler(c, 11, masks=bitmaps), corpus.CorpusSampler(c, 11)
    hit_held = hit_free = 0
    for _ in range(50):
        hit_held += overlaps(held.draw(32))
        hit_free += overlaps(free.draw(32))
    assert hit_held == 0 and hit_free > 0, (hit_held, hit_free)
    # a margin widens the rectangles: no training crop within 3 cells of a validation crop either
    wide = corpus.CorpusSampler(c, 11, masks=c.origin_masks(holdout=val[:2], margin=3)[0]).draw(400)
    dy, dx = np.abs(wide[:, None, 1] - val[None, :2, 1]), np.abs(wide[:, None, 2] - val[None, :2, 2])
    assert not ((dy < 19) & (dx < 19)).any()


# ---- 5. command line -----------------------------------------------------------------------------------------------------------------
def _blank_tile_files(tmp_path):
    """The two bundled tiles with the top third of the first blank (zeros in every raster, as a partial swath is)."""
    files = []
    for k, name in enumerate(fx.TILES):
        d10, d20, d60 = (np.array(a) for a in fx.load_tile(name))
        if k == 0:
            d10[:204], d20[:102], d60[:34] = 0, 0, 0
        path = str(tmp_path / ('tile_%s.npz' % name))
        np.savez(path, d10=d10, d20=d20, d60=d60)
        files.append(path)
    return files


def _args(files, path, out, extra=()):
    return ['--tiles'] + files + ['--path', str(path), '--out', str(out), '--epochs', '2', '--steps_per_epoch', '3', '--val_crops', '2',
                                  '--batch_size', '5', '--seed', '7', '--lr', '1e-3', '--augment'] + list(extra)


def _files(out):
    ckpt, log = out / 's2_038_lr_1e-03.npy', out / 's2_038__lr_1.0e-03.txt'
    assert ckpt.exists() and log.exists(), sorted(os.listdir(str(out)))
    return ckpt.read_bytes(), log.read_bytes()


def test_train_tiles_with_the_three_flags(tmp_path, capsys, monkeypatch):
    files = _blank_tile_files(tmp_path)
    flags = ['--skip_blank', '--holdout', '--val_on_device']
    calls = []
    real = S2Model.fit_corpus

    def spy(self, corp, *a, **kw):
        calls.append((corp, kw))
        return real(self, corp, *a, **kw)
    monkeypatch.setattr(S2Model, 'fit_corpus', spy)
    assert train.main(_args(files, tmp_path, tmp_path / 'a', flags)) == 0
    said = capsys.readouterr().out
    assert 'tile 0: %d of %d origins free of blank pixels' % (135 * 84, 135 * 135) in said and 'tile 1: 18225 of 18225' in said
    assert 'Hold-out: training crops are drawn from' in said and '4 crops for validation' in said
    corp, kw = calls[-1]
    assert kw['validation_data'] is None and kw['validation_crops'].shape == (4, 4) and len(kw['masks']) == 2
    val = kw['validation_crops']
    assert (val[val[:, 0] == 0, 1] >= 51).all()                                # the validation crops avoid the blank third
    assert train.main(_args(files, tmp_path, tmp_path / 'b', flags)) == 0      # the same --seed: the same bytes
    assert _files(tmp_path / 'a') == _files(tmp_path / 'b')
    lines = _files(tmp_path / 'a')[1].decode().splitlines()
    assert len(lines) == 2 and all(l.startswith('Finished epoch') and 'valid:' in l and 'None' not in l for l in lines)
    # without the three flags: the call of the code as it was — host arrays of validation_arrays' crops, no mask, no table
    capsys.readouterr()
    assert train.main(_args(files, tmp_path, tmp_path / 'c')) == 0
    assert 'origins free of blank pixels' not in capsys.readouterr().out
    corp, kw = calls[-1]
    assert 'masks' not in kw and 'validation_crops' not in kw
    table = cm.validation_table(corp.extents, 2, 7, corpus.CorpusSampler.VAL_STREAM)
    dx, dy = corp.batch(table)
    for got, want in zip(list(kw['validation_data'][0]) + [kw['validation_data'][1]], dx + [dy]):
        assert got.tobytes() == want.cpu().numpy().tobytes()
    assert _files(tmp_path / 'c') != _files(tmp_path / 'a')
    # ... and its files are those of the call the command line made before the flags existed, restated here with the same model,
    # optimizer and callbacks: fit_corpus(validation_data=corpus.validation_arrays(...)).  (That fit_corpus itself — whose loss
    # buffer now shares an allocation with the validation sums — still takes the steps of the host path byte for byte is pinned
    # by tests/test_gpu_corpus.py, which this pull request does not touch.)
    out = tmp_path / 'e'
    out.mkdir()
    ckpt, log_path = out / 's2_038_lr_1e-03.npy', out / 's2_038__lr_1.0e-03.txt'
    log_path.write_bytes(b'')
    model = s2model(((4, None, None), (6, None, None)), num_layers=6, feature_size=128, device=DEV)
    model.set_weights_flat(weights.random_he_uniform(model.cin, model.cout, model.num_layers, model.feature_size, seed=7))
    model.compile(optimizer=training.Nadam(lr=1e-3, beta_1=0.9, beta_2=0.999, epsilon=1e-8, schedule_decay=0.004),
                  loss='mean_absolute_error', mixed_precision=None)

    class EpochLog(training.Callback):
        def on_epoch_end(self, epoch, logs=None):
            with open(str(log_path), 'a') as f:
                f.write('Finished epoch {:5d}: loss {:.3e}, valid: {:.3e}, lr: {:.1e}\n'
                        .format(epoch, logs.get('loss'), logs.get('val_loss'), self.model.optimizer.lr))
    callbacks = [training.ModelCheckpoint(str(ckpt), monitor='val_loss', verbose=0, save_best_only=True), EpochLog(),
                 training.ReduceLROnPlateau(monitor='val_loss', factor=0.5, patience=5, verbose=0, min_delta=1e-6, cooldown=20, min_lr=1e-5)]
    real(model, corp, 5, 3, epochs=2, validation_data=corp.validation_arrays(2, 7), seed=7, augment=True, callbacks=callbacks, verbose=0)
    assert _files(out) == _files(tmp_path / 'c')
