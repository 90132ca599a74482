"""Host side of training from tiles (no GPU): the crop sampler, the refusals of dsen2_corpus_create / dsen2_corpus_batch — which
check host memory only and touch no device — the refusals of TileCorpus, and the command-line flags."""
import ctypes
import os
import re

import numpy as np
import pytest

from dsen2_amd import _lib, corpus, patches, train, training

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXTENTS = [(24, 40), (33, 17)]


# ---- the sampler --------------------------------------------------------------------------------------------------------------
def test_sampler_is_a_function_of_the_seed_and_the_sequence_of_n():
    a, b = corpus.CorpusSampler(EXTENTS, 7, augment=True), corpus.CorpusSampler(EXTENTS, 7, augment=True)
    for n in (5, 5, 2, 0, 9):
        x, y = a.draw(n), b.draw(n)
        assert x.dtype == np.int32 and x.shape == (n, 4) and x.flags['C_CONTIGUOUS'] and np.array_equal(x, y)
    assert not np.array_equal(corpus.CorpusSampler(EXTENTS, 8, True).draw(64), corpus.CorpusSampler(EXTENTS, 7, True).draw(64))
    # a stream of its own: neither the shuffle's, nor the augmentation's, nor the validation crops'
    assert not np.array_equal(corpus.CorpusSampler(EXTENTS, 7, True).draw(64)[:, 3], training.AugmentOps(7).draw(64))
    assert corpus.CorpusSampler.STREAM not in (training.AugmentOps.STREAM, corpus.CorpusSampler.VAL_STREAM)
    assert corpus.CorpusSampler(EXTENTS, None).draw(3).shape == (3, 4)
    # the documented order of the draws: tiles, row origins, column origins, ops
    rng = np.random.default_rng(np.random.SeedSequence([7, corpus.CorpusSampler.STREAM]))
    ext = np.asarray(EXTENTS)
    tiles = rng.integers(0, 2, size=6)
    oy = rng.integers(0, ext[tiles, 0] - 16)
    ox = rng.integers(0, ext[tiles, 1] - 16)
    ops = rng.integers(0, 8, size=6)
    assert np.array_equal(corpus.CorpusSampler(EXTENTS, 7, True).draw(6), np.stack([tiles, oy, ox, ops], axis=1))


def test_sampler_ranges_are_the_references():
    """Tiles uniform; origins uniform over [0, extent - 16) per axis, the range random.randrange(0, extent - 16) of
    patches.random_origins covers: extent - 16 itself is never drawn, extent - 17 is."""
    t = corpus.CorpusSampler(EXTENTS, 3, augment=True).draw(20000)
    assert set(np.unique(t[:, 0])) == {0, 1} and abs((t[:, 0] == 0).mean() - 0.5) < 0.02
    for i, (eh, ew) in enumerate(EXTENTS):
        mine = t[t[:, 0] == i]
        assert mine[:, 1].min() == 0 and mine[:, 1].max() == eh - 17
        assert mine[:, 2].min() == 0 and mine[:, 2].max() == ew - 17
    assert EXTENTS[1][1] - 17 == 0                                 # the narrow tile has ONE column origin
    assert set(np.unique(t[:, 3])) == set(range(8)) and abs(np.bincount(t[:, 3], minlength=8) / 20000.0 - 0.125).max() < 0.02
    org = patches.random_origins((24, 40), 16, 4000, seed=1)       # the reference's draw covers the same range
    assert org[:, 0].max() == 24 - 17 and org[:, 1].max() == 40 - 17 and org.min() == 0


def test_sampler_without_augment_draws_op_zero_and_the_same_crops():
    plain, aug = corpus.CorpusSampler(EXTENTS, 5).draw(50), corpus.CorpusSampler(EXTENTS, 5, augment=True).draw(50)
    assert (plain[:, 3] == 0).all() and aug[:, 3].max() > 0
    assert np.array_equal(plain[:, :3], aug[:, :3])                # within ONE draw the ops come last


def test_sampler_depends_on_the_extents_alone():
    class Built(object):                                           # what a TileCorpus shows the sampler
        extents = [(24, 40), (33, 17)]
        lr = 'images of any content'
    assert np.array_equal(corpus.CorpusSampler(Built(), 11, True).draw(40), corpus.CorpusSampler(EXTENTS, 11, True).draw(40))
    with pytest.raises(ValueError):
        corpus.CorpusSampler([(16, 40)], 1)                        # no room for a draw: extent - 16 = 0


# ---- the C ABI's refusals: no device is touched ---------------------------------------------------------------------------------
FAKE = 0x10000      # a non-NULL "device pointer": the refused calls never read it


def _handle(run_60=False, extents=EXTENTS, dtypes=None):
    table = (_lib.CorpusTile * len(extents))()
    for i, (eh, ew) in enumerate(extents):
        table[i] = _lib.CorpusTile(FAKE, FAKE, FAKE if run_60 else None, FAKE, eh, ew, (dtypes or [_lib.DTYPE_U16] * len(extents))[i])
    h = ctypes.c_void_p(0)
    _lib.call('dsen2_corpus_create', table, len(extents), int(run_60), ctypes.byref(h))
    return h


def _batch(h, samples, n=None, x60=None, host=True, dev=True, divisor=2000.0, x10=FAKE, x20=FAKE, y=FAKE):
    s = np.ascontiguousarray(samples, np.int32).reshape(-1, 4)
    n = s.shape[0] if n is None else n
    return _lib.load().dsen2_corpus_batch(h, s.ctypes.data_as(ctypes.c_void_p) if host else None, FAKE if dev else None, n,
                                          divisor, x10, x20, x60, y, None)


def _refused(code, pattern):
    assert code == _lib.ERR_INVALID, code
    msg = _lib.load().dsen2_last_error().decode()
    assert re.search(pattern, msg), msg


def test_batch_refusals_come_back_as_invalid_with_their_message():
    lib = _lib.load()
    h, h60 = _handle(), _handle(run_60=True)
    try:
        ok = [[0, 0, 0, 0]]
        _refused(_batch(None, ok), 'NULL')
        for kw in ({'x10': None}, {'x20': None}, {'y': None}):
            _refused(_batch(h, ok, **kw), 'NULL')
        _refused(_batch(h, ok, x60=FAKE), 'dev_x60 given')
        _refused(_batch(h60, ok), 'needs dev_x60')
        _refused(_batch(h, ok, host=False), 'both required')
        _refused(_batch(h, ok, dev=False), 'both required')
        _refused(_batch(h, [[2, 0, 0, 0]]), 'tile 2 outside the table of 2')
        _refused(_batch(h, [[-1, 0, 0, 0]]), 'tile -1 outside')
        _refused(_batch(h, [[0, 24 - 15, 0, 0]]), r'origin \(9, 0\) \+ 16 reaches outside the 24 x 40 grid of tile 0')
        _refused(_batch(h, [[0, 0, 40 - 15, 0]]), r'origin \(0, 25\)')
        _refused(_batch(h, [[1, 0, 2, 0]]), r'origin \(0, 2\) \+ 16 reaches outside the 33 x 17 grid of tile 1')
        _refused(_batch(h, [[0, -1, 0, 0]]), 'origin')
        _refused(_batch(h, ok + [[1, 17, 1, 8]]), 'sample 1: op 8 outside 0..7')
        _refused(_batch(h, [[0, 0, 0, -1]]), 'op -1')
        _refused(_batch(h, ok, divisor=0.0), 'divisor')
        _refused(_batch(h, ok, n=-1), 'batch of -1')
        # n == 0 is not an error, and needs no tables
        assert _batch(h, np.zeros((0, 4), np.int32), host=False, dev=False) == _lib.OK
    finally:
        lib.dsen2_corpus_destroy(h)
        lib.dsen2_corpus_destroy(h60)
    lib.dsen2_corpus_destroy(None)


def test_create_refusals():
    lib = _lib.load()
    out = ctypes.c_void_p(0)
    one = (_lib.CorpusTile * 1)(_lib.CorpusTile(FAKE, FAKE, None, FAKE, 16, 16, _lib.DTYPE_F32))
    assert lib.dsen2_corpus_create(one, 1, 0, ctypes.byref(out)) == _lib.OK and out.value       # 16 x 16: one origin, (0, 0)
    lib.dsen2_corpus_destroy(out)
    _refused(lib.dsen2_corpus_create(one, 1, 1, ctypes.byref(out)), '60 m image')
    assert not out.value
    _refused(lib.dsen2_corpus_create(one, 0, 0, ctypes.byref(out)), 'at least one tile')
    _refused(lib.dsen2_corpus_create(None, 1, 0, ctypes.byref(out)), 'NULL')
    _refused(lib.dsen2_corpus_create(one, 1, 0, None), 'NULL')
    for bad, pattern in ((_lib.CorpusTile(None, FAKE, None, FAKE, 16, 16, 1), 'NULL image'),
                         (_lib.CorpusTile(FAKE, FAKE, None, None, 16, 16, 1), 'NULL image'),
                         (_lib.CorpusTile(FAKE, FAKE, FAKE, FAKE, 16, 16, 1), '60 m image'),
                         (_lib.CorpusTile(FAKE, FAKE, None, FAKE, 15, 16, 1), 'no room'),
                         (_lib.CorpusTile(FAKE, FAKE, None, FAKE, 16, 16, _lib.DTYPE_F64), 'uint16 or float32')):
        _refused(lib.dsen2_corpus_create((_lib.CorpusTile * 1)(bad), 1, 0, ctypes.byref(out)), pattern)


def test_header_declares_the_corpus_entries():
    header = open(os.path.join(ROOT, 'include', 'dsen2_hip.h')).read()
    lib = _lib.load()
    for name in ('dsen2_corpus_create', 'dsen2_corpus_destroy', 'dsen2_corpus_batch'):
        assert re.search(r'\b(int|void) %s\s*\(' % name, header) and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert ctypes.sizeof(_lib.CorpusTile) == 4 * ctypes.sizeof(ctypes.c_void_p) + 4 * 4     # 3 ints and the tail padding


# ---- TileCorpus: every refusal before anything reaches a GPU ----------------------------------------------------------------------
def _tile(h, w, dtype=np.uint16):
    return np.zeros((h, w, 4), dtype), np.zeros((h // 2, w // 2, 6), dtype), np.zeros((h // 6, w // 6, 2), dtype)


def test_tile_corpus_refuses_what_create_patches_refuses():
    d10, d20, d60 = _tile(72, 72)
    with pytest.raises(ValueError, match=r'downPixelAggr: image of 71 x 72 pixels is not a multiple of SCALE = 2'):
        corpus.TileCorpus([(d10[:71], d20)])
    with pytest.raises(ValueError, match=r'downPixelAggr: image of 36 x 35 pixels is not a multiple of SCALE = 2'):
        corpus.TileCorpus([(d10, d20[:, :35])])
    with pytest.raises(ValueError, match=r'not a multiple of SCALE = 6'):
        corpus.TileCorpus([_tile(600, 600)], run_60=True)          # the 100 x 100 60 m image of the bundled tiles
    with pytest.raises(ValueError, match=r'does not cover 2 x the lower-resolution image'):
        corpus.TileCorpus([(d10[:68], d20)])
    with pytest.raises(ValueError, match=r'is not 2 x the lowest-resolution image'):
        corpus.TileCorpus([(d10, d20[:34])])
    with pytest.raises(ValueError, match=r'does not cover 3 x'):
        corpus.TileCorpus([(np.zeros((1152, 1152, 4), np.uint16), np.zeros((570, 576, 6), np.uint16), np.zeros((192, 192, 2), np.uint16))],
                          run_60=True)
    with pytest.raises(ValueError, match=r'leaves no room for a 16 x 16 patch'):
        corpus.TileCorpus([_tile(60, 72)[:2]])                     # lr20 of 15 x 18
    with pytest.raises(ValueError, match=r'6 bands'):
        corpus.TileCorpus([(d10, d20[:, :, :5])])
    with pytest.raises(ValueError, match=r'd60'):
        corpus.TileCorpus([(d10, d20)], run_60=True)
    with pytest.raises(ValueError, match=r'at least one tile'):
        corpus.TileCorpus([])
    # a good tile behind a bad one is not uploaded either: the second tile's refusal comes first
    with pytest.raises(ValueError, match=r'not a multiple'):
        corpus.TileCorpus([(d10, d20), (d10[:71], d20)])


def test_tile_corpus_needs_a_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip('CPU-box behaviour')
    d10, d20, _ = _tile(72, 72)
    with pytest.raises(RuntimeError):
        corpus.TileCorpus([(d10, d20)])


# ---- command line ---------------------------------------------------------------------------------------------------------------
def test_train_flags(capsys, tmp_path):
    a = train.parse_args([])
    assert a.tiles is None and a.steps_per_epoch is None and a.val_crops is None
    a = train.parse_args(['--tiles', 'a.npz', 'b.mat', '--steps_per_epoch', '3', '--val_crops', '4', '--augment', '--run_60'])
    assert a.tiles == ['a.npz', 'b.mat'] and a.steps_per_epoch == 3 and a.val_crops == 4 and a.augment and a.run_60
    for bad, word in ((['--steps_per_epoch', '3'], '--tiles'), (['--val_crops', '3'], '--tiles'),
                      (['--tiles', 'a.npz', '--predict', 'm/s2_999_lr_1e-04.npy'], '--predict'),
                      (['--tiles', 'a.npz', '--steps_per_epoch', '0'], 'at least 1')):
        with pytest.raises(SystemExit):
            train.parse_args(bad)
        assert word in capsys.readouterr().err
    # --tiles against a populated --path
    path = str(tmp_path) + '/'
    args = train.parse_args(['--tiles', 'a.npz', '--path', path])
    assert train.tiles_conflict(args, path) is None
    os.makedirs(path + 'train/S2A_X.SAFE')
    msg = train.tiles_conflict(args, path)
    assert msg and '--tiles and a training set under --path exclude each other' in msg
    assert train.tiles_conflict(train.parse_args(['--tiles', 'a.npz', '--run_60']), path) is None       # train60/ is empty
    assert train.tiles_conflict(train.parse_args(['--path', path]), path) is None                       # without --tiles: as before
    assert train.main(['--tiles', 'a.npz', '--path', path]) == 2
    assert 'exclude each other' in capsys.readouterr().err
