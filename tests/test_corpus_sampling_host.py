"""Host side of drawing crops with origin masks and of validating on the device (no GPU): the sampler with and without masks
against a from-scratch restatement, the validation table, the 1-in-64 refusal, the refusals of dsen2_corpus_origin_mask and
dsen2_abs_sq_error_sums — which check host memory only and touch no device — and the command-line flags."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import corpus_mask_restatement as cm  # noqa: E402

from dsen2_amd import _lib, corpus, train  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXTENTS = [(24, 40), (33, 17)]
FAKE = 0x10000      # a non-NULL "device pointer": the refused calls never read it


def _valid_maps(seed=0, share=0.5):
    """Random bool maps [grid_h - 15, grid_w - 15] per tile of EXTENTS, about `share` of the origins valid."""
    rng = np.random.default_rng(seed)
    return [rng.random((gh - 15, gw - 15)) < share for gh, gw in EXTENTS]


# ---- the sampler ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('augment', [False, True])
def test_masks_none_is_the_sampler_as_it_was(augment):
    for seed in (0, 7, 12345):
        a, b = corpus.CorpusSampler(EXTENTS, seed, augment), corpus.CorpusSampler(EXTENTS, seed, augment, masks=None)
        for n in (5, 5, 2, 0, 9, 128):
            x, y = a.draw(n), b.draw(n)
            assert x.dtype == np.int32 and np.array_equal(x, y)
        # ... and as its documented order of draws
        rng = np.random.default_rng(np.random.SeedSequence([seed, corpus.CorpusSampler.STREAM]))
        ext = np.asarray(EXTENTS)
        tiles = rng.integers(0, 2, size=6)
        want = [tiles, rng.integers(0, ext[tiles, 0] - 16), rng.integers(0, ext[tiles, 1] - 16)]
        want.append(rng.integers(0, 8, size=6) if augment else np.zeros(6, np.int64))
        assert np.array_equal(corpus.CorpusSampler(EXTENTS, seed, augment, masks=None).draw(6), np.stack(want, axis=1))


@pytest.mark.parametrize('augment', [False, True])
def test_masked_draws_are_valid_and_equal_the_restated_redraw_rule(augment):
    valid = _valid_maps(seed=3, share=0.3)
    masks = [cm.pack(v) for v in valid]
    for seed in (1, 9):
        s = corpus.CorpusSampler(EXTENTS, seed, augment, masks=masks)
        plain = corpus.CorpusSampler(EXTENTS, seed, augment)
        rng = np.random.default_rng(np.random.SeedSequence([seed, corpus.CorpusSampler.STREAM]))
        moved = 0
        for n in (7, 64, 1, 0, 33):
            got = s.draw(n)
            assert got.dtype == np.int32 and got.shape == (n, 4) and got.flags['C_CONTIGUOUS']
            assert all(valid[t][oy, ox] for t, oy, ox, _ in got.tolist())
            assert np.array_equal(got, cm.draw_with_masks(rng, EXTENTS, valid, n, augment))
            first = plain.draw(n) if moved == 0 else None
            if first is not None and n:
                # the first call starts from the unmasked draws: tiles and ops are kept, only invalid origins moved
                assert np.array_equal(got[:, 0], first[:, 0]) and np.array_equal(got[:, 3], first[:, 3])
                was_valid = np.array([valid[t][oy, ox] for t, oy, ox, _ in first.tolist()])
                assert np.array_equal(got[was_valid], first[was_valid]) and not was_valid.all()
                moved = 1
    # a function of the masks too
    other = [cm.pack(v) for v in _valid_maps(seed=4, share=0.3)]
    assert not np.array_equal(corpus.CorpusSampler(EXTENTS, 1, masks=masks).draw(64), corpus.CorpusSampler(EXTENTS, 1, masks=other).draw(64))


def test_masked_draws_hit_every_valid_origin_and_no_other():
    """A handful of valid origins per tile (at least 1 in 64 of 9 x 25 = 225 and of 18 x 2 = 36): 20 000 draws reach each."""
    valid = [np.zeros((9, 25), bool), np.zeros((18, 2), bool)]
    for oy, ox in ((0, 0), (7, 23), (3, 8), (3, 9), (5, 17), (0, 23)):        # (7, 23): the last origin the sampler draws
        valid[0][oy, ox] = True
    for oy in (0, 16, 9):                                                      # column 0 is the one column origin of this tile
        valid[1][oy, 0] = True
    t = corpus.CorpusSampler(EXTENTS, 5, augment=True, masks=[cm.pack(v) for v in valid]).draw(20000)
    for i in (0, 1):
        mine = t[t[:, 0] == i]
        assert {(oy, ox) for oy, ox in mine[:, 1:3].tolist()} == {(int(a), int(b)) for a, b in np.argwhere(valid[i])}
    assert abs((t[:, 0] == 0).mean() - 0.5) < 0.02                             # tiles stay uniform: not weighted by valid area
    assert set(np.unique(t[:, 3])) == set(range(8))


def test_too_few_valid_origins_are_refused_with_tile_count_and_total():
    full = [np.ones((9, 25), bool), np.ones((18, 2), bool)]
    few = np.zeros((9, 25), bool)
    few[0, :3] = True                                                          # 3 of 225: 3 * 64 < 225
    with pytest.raises(ValueError, match=r'tile 0: 3 of 225 origins are valid, fewer than 1 in 64'):
        corpus.CorpusSampler(EXTENTS, 1, masks=[cm.pack(few), cm.pack(full[1])])
    few[0, 3] = True                                                           # 4 of 225: 256 >= 225
    corpus.CorpusSampler(EXTENTS, 1, masks=[cm.pack(few), cm.pack(full[1])]).draw(8)
    with pytest.raises(ValueError, match=r'tile 1: 0 of 36 origins are valid'):
        corpus.CorpusSampler(EXTENTS, 1, masks=[cm.pack(full[0]), cm.pack(np.zeros((18, 2), bool))])
    with pytest.raises(ValueError, match=r'tile 2: 1 of 100'):
        corpus.check_origin_counts([(16, 16), (16, 16), (25, 25)], [1, 1, 1])
    corpus.check_origin_counts([(16, 16)], [1])                                # one origin, valid
    # masks that do not describe the tiles
    with pytest.raises(ValueError, match=r'1 masks for 2 tiles'):
        corpus.CorpusSampler(EXTENTS, 1, masks=[cm.pack(full[0])])
    with pytest.raises(ValueError, match=r'tile 1: a packed origin bitmap of shape'):
        corpus.CorpusSampler(EXTENTS, 1, masks=[cm.pack(full[0]), cm.pack(full[0])])
    assert corpus.mask_shapes((24, 40)) == ((24, 40), (9, 4)) and corpus.mask_shapes((16, 16)) == ((16, 16), (1, 1))


def test_redraw_stops_hard_when_no_valid_origin_can_be_drawn(monkeypatch):
    """Valid origins on the last row alone pass the 1-in-64 test and are never drawn (origins are drawn below extent - 16)."""
    valid = np.zeros((9, 25), bool)
    valid[8, :] = True
    monkeypatch.setattr(corpus, 'MAX_REDRAW_ROUNDS', 20)
    s = corpus.CorpusSampler([(24, 40)], 1, masks=[cm.pack(valid)])
    with pytest.raises(RuntimeError, match=r'after 20 redraw rounds'):
        s.draw(4)
    assert corpus.CorpusSampler([(24, 40)], 1, masks=[cm.pack(valid)]).draw(0).shape == (0, 4)


# ---- the validation table --------------------------------------------------------------------------------------------------------
class _Corpus(object):
    """What validation_table looks at of a TileCorpus."""
    extents = EXTENTS

    def __len__(self):
        return len(self.extents)


def test_validation_table_is_the_table_validation_arrays_drew():
    for seed, m in ((17, 2), (3, 11)):
        got = corpus.TileCorpus.validation_table(_Corpus(), m, seed)
        assert got.dtype == np.int32 and got.shape == (2 * m, 4) and (got[:, 3] == 0).all()
        assert np.array_equal(got, cm.validation_table(EXTENTS, m, seed, corpus.CorpusSampler.VAL_STREAM))
        assert np.array_equal(got, corpus.TileCorpus.validation_table(_Corpus(), m, seed, masks=None))
    # a stream of its own, as before
    assert not np.array_equal(corpus.TileCorpus.validation_table(_Corpus(), 32, 17)[:, 1:3], corpus.CorpusSampler(EXTENTS, 17).draw(64)[:, 1:3])
    valid = _valid_maps(seed=8, share=0.4)
    got = corpus.TileCorpus.validation_table(_Corpus(), 40, 17, masks=[cm.pack(v) for v in valid])
    assert all(valid[t][oy, ox] for t, oy, ox, _ in got.tolist()) and got[:, 0].tolist() == [0] * 40 + [1] * 40
    assert np.array_equal(got, cm.validation_table(EXTENTS, 40, 17, corpus.CorpusSampler.VAL_STREAM, valid))
    assert not np.array_equal(got, corpus.TileCorpus.validation_table(_Corpus(), 40, 17))


# ---- the C ABI's refusals: no device is touched ---------------------------------------------------------------------------------
def _refused(code, pattern, want=_lib.ERR_INVALID):
    assert code == want, code
    msg = _lib.load().dsen2_last_error().decode()
    assert re.search(pattern, msg), msg


def _mask(src=FAKE, dtype=_lib.DTYPE_U16, H=96, W=160, C=4, gh=24, gw=40, holdout=None, host=True, dev=True, m=None, margin=0,
          cells=FAKE, bitmap=FAKE, count=FAKE):
    h = np.ascontiguousarray(holdout if holdout is not None else np.zeros((0, 2)), np.int32).reshape(-1, 2)
    m = h.shape[0] if m is None else m
    return _lib.load().dsen2_corpus_origin_mask(src, dtype, H, W, C, gh, gw, h.ctypes.data_as(ctypes.c_void_p) if host and h.size else None,
                                                FAKE if dev and h.size else None, m, margin, cells, bitmap, count, None)


def test_origin_mask_refusals_come_back_as_invalid_with_their_message():
    for kw in ({'src': None}, {'cells': None}, {'bitmap': None}, {'count': None}):
        _refused(_mask(**kw), 'NULL')
    _refused(_mask(dtype=_lib.DTYPE_F64), 'dtype 2 is not supported')
    _refused(_mask(dtype=7), 'dtype 7')
    _refused(_mask(gh=15, H=60), 'no room for a 16 x 16 patch')
    _refused(_mask(gw=15, W=60), 'no room')
    _refused(_mask(C=0), 'bands')
    _refused(_mask(gh=(1 << 15) + 1, H=4 * ((1 << 15) + 1)), r'is beyond 32768')   # (grid - 15)^2 origins must fit the int32 count
    assert ((1 << 15) - 15) ** 2 < 1 << 31
    _refused(_mask(H=97), 'is not F x the 24 x 40 origin grid')
    _refused(_mask(W=161), 'is not F x')
    _refused(_mask(H=96, W=40 * 36), 'is not F x')                               # two footprints
    _refused(_mask(H=24 * 2, W=40 * 2), 'footprint F = 2')
    _refused(_mask(H=24 * 6, W=40 * 6), 'footprint F = 6')
    _refused(_mask(H=0, W=0), 'is not F x')
    _refused(_mask(m=-1), '-1 hold-out origins')
    _refused(_mask(margin=-1), 'margin -1')
    ok = [[0, 0], [8, 24]]                                                       # (grid - 16, grid - 16) is the last valid origin
    _refused(_mask(holdout=ok, host=False), 'both required')
    _refused(_mask(holdout=ok, dev=False), 'both required')
    _refused(_mask(holdout=ok + [[9, 0]]), r'hold-out origin 2: \(9, 0\) \+ 16 reaches outside the 24 x 40 grid')
    _refused(_mask(holdout=[[0, 25]]), r'hold-out origin 0: \(0, 25\)')
    _refused(_mask(holdout=[[-1, 0]]), r'hold-out origin 0')
    _refused(_mask(holdout=[[0, -1]]), r'hold-out origin 0')
    _refused(_mask(dtype=_lib.MASK_BLANK_MAP, H=95), 'is not F x')               # the blank-map form has the same shape checks
    _refused(_mask(dtype=_lib.DTYPE_F32, H=24 * 36, W=40 * 36, gh=24, gw=40, holdout=[[9, 0]]), 'hold-out origin 0')


def test_error_sums_refusals():
    lib = _lib.load()
    need = ctypes.c_size_t(0)
    assert lib.dsen2_abs_sq_error_sums_workspace_bytes(ctypes.byref(need)) == _lib.OK and need.value == 4096 * 2 * 8
    _refused(lib.dsen2_abs_sq_error_sums_workspace_bytes(None), 'NULL')
    for args in ((None, FAKE, 8, FAKE, need.value, FAKE), (FAKE, None, 8, FAKE, need.value, FAKE), (FAKE, FAKE, 8, None, need.value, FAKE),
                 (FAKE, FAKE, 8, FAKE, need.value, None)):
        _refused(lib.dsen2_abs_sq_error_sums(*args, None), 'NULL')
    _refused(lib.dsen2_abs_sq_error_sums(FAKE, FAKE, 0, FAKE, need.value, FAKE, None), r'0 pairs outside')
    _refused(lib.dsen2_abs_sq_error_sums(FAKE, FAKE, -3, FAKE, need.value, FAKE, None), r'-3 pairs')
    _refused(lib.dsen2_abs_sq_error_sums(FAKE, FAKE, 1 << 31, FAKE, need.value, FAKE, None), r'2147483648 pairs')
    _refused(lib.dsen2_abs_sq_error_sums(FAKE, FAKE, 8, FAKE, need.value - 1, FAKE, None), 'workspace of 65535 bytes', want=_lib.ERR_WORKSPACE)


def test_header_exports_and_signatures_agree_for_the_new_entries():
    header = open(os.path.join(ROOT, 'include', 'dsen2_hip.h')).read()
    lib = _lib.load()
    for name in ('dsen2_corpus_origin_mask', 'dsen2_abs_sq_error_sums', 'dsen2_abs_sq_error_sums_workspace_bytes'):
        assert re.search(r'\bint %s\s*\(' % name, header) and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert re.search(r'#define DSEN2_MASK_BLANK_MAP %d\b' % _lib.MASK_BLANK_MAP, header)
    # the declared argument counts are the bound ones
    for name in ('dsen2_corpus_origin_mask', 'dsen2_abs_sq_error_sums'):
        decl = re.search(r'\bint %s\s*\(([^;]*)\);' % name, header).group(1)
        assert len(decl.split(',')) == len(_lib.SIGNATURES[name][1]), name


# ---- command line ---------------------------------------------------------------------------------------------------------------
def test_train_flags(capsys):
    a = train.parse_args(['--tiles', 'a.npz'])
    assert not a.skip_blank and not a.holdout and a.holdout_margin is None and not a.val_on_device
    a = train.parse_args(['--tiles', 'a.npz', '--skip_blank', '--holdout', '--holdout_margin', '3', '--val_on_device'])
    assert a.skip_blank and a.holdout and a.holdout_margin == 3 and a.val_on_device
    assert train.parse_args(['--tiles', 'a.npz', '--holdout']).holdout_margin is None
    for bad, word in ((['--skip_blank'], '--tiles'), (['--holdout'], '--tiles'), (['--val_on_device'], '--tiles'),
                      (['--holdout', '--holdout_margin', '2'], '--tiles'),
                      (['--tiles', 'a.npz', '--holdout_margin', '2'], '--holdout'),
                      (['--tiles', 'a.npz', '--holdout', '--holdout_margin', '-1'], '--holdout')):
        with pytest.raises(SystemExit):
            train.parse_args(bad)
        assert word in capsys.readouterr().err


def test_fit_corpus_refuses_both_validations():
    """validation_data and validation_crops exclude each other: refused before anything touches a model or a GPU."""
    from dsen2_amd.DSen2Net import S2Model

    class Plain(object):
        device, run_60, cout, patch = 'cpu', False, 6, 32

        def output_shapes(self, n):
            return [(n, 4, 32, 32), (n, 6, 32, 32)], (n, 6, 32, 32)

    class Model(object):
        device, bands, cout = 'cpu', (4, 6), 6
        _data_parallel_plan = staticmethod(lambda data_parallel, emulate_world: None)

    with pytest.raises(ValueError, match=r'validation_data .* and validation_crops .* exclude each other'):
        S2Model.fit_corpus(Model(), Plain(), 4, 3, validation_data=([], []), validation_crops=np.zeros((2, 4), np.int32))


def test_validation_crops_must_have_op_zero():
    """Validation is never augmented: a table that carries ops (a CorpusSampler(augment=True) draw) is refused, not turned."""
    from dsen2_amd.DSen2Net import S2Model
    ok = np.asarray([(0, 1, 2, 0), (1, 3, 0, 0)], np.int32)
    assert np.array_equal(S2Model._check_validation_crops(corpus.TileCorpus, ok), ok)
    bad = ok.copy()
    bad[1, 3] = 5
    with pytest.raises(ValueError, match=r'must have op 0 .* got ops \[0, 5\]'):
        S2Model._check_validation_crops(corpus.TileCorpus, bad)
    with pytest.raises(ValueError, match='no sample'):
        S2Model._check_validation_crops(corpus.TileCorpus, ok[:0])


class _Recording(_Corpus):
    """A corpus stand-in for train.tiles_validation: draws tables as TileCorpus does, records what it is asked to mask and to cut."""

    def __init__(self):
        self.held, self.cut, self.draws = [], [], 0

    def validation_table(self, crops_per_tile, seed, masks=None):
        self.draws += 1
        return corpus.TileCorpus.validation_table(self, crops_per_tile, seed, masks)

    def origin_masks(self, holdout=None, margin=0):
        self.held.append((holdout, margin))
        return [cm.pack(np.ones((gh - 15, gw - 15), bool)) for gh, gw in self.extents], [(gh - 15) * (gw - 15) for gh, gw in self.extents]

    def table_arrays(self, table, chunk=256):
        self.cut.append(table)
        return ['x10', 'x20'], 'y'

    def validation_arrays(self, *a, **k):
        raise AssertionError('a second draw of the validation crops: without --seed it gives other crops than the ones held out')


@pytest.mark.parametrize('seed', [None, 7])
def test_one_validation_table_serves_hold_out_arrays_and_device_validation(seed):
    """Without --seed every draw comes from fresh entropy: the table that is held out, the table that is cut into host arrays and
    the table handed to fit_corpus must be ONE draw."""
    base = ['--tiles', 'a.npz'] + ([] if seed is None else ['--seed', str(seed)])
    said = []
    c = _Recording()
    table, masks, arrays = train.tiles_validation(c, train.parse_args(base + ['--holdout', '--holdout_margin', '2']), 6, said.append)
    assert c.draws == 1 and len(c.held) == 1 and len(c.cut) == 1
    assert c.held[0][0] is table and c.held[0][1] == 2 and c.cut[0] is table and arrays == (['x10', 'x20'], 'y') and len(masks) == 2
    assert table.shape == (12, 4) and said and 'Hold-out' in said[0]
    c = _Recording()
    table, masks, arrays = train.tiles_validation(c, train.parse_args(base + ['--holdout', '--skip_blank', '--val_on_device']), 6, said.append)
    assert c.draws == 1 and arrays is None and not c.cut and c.held[-1][0] is table and c.held[0] == (None, 0)
    c = _Recording()                                               # no flag: one draw, cut into arrays, no masks
    table, masks, arrays = train.tiles_validation(c, train.parse_args(base), 6, said.append)
    assert c.draws == 1 and masks is None and not c.held and c.cut[0] is table
    if seed is not None:
        assert np.array_equal(table, cm.validation_table(EXTENTS, 6, seed, corpus.CorpusSampler.VAL_STREAM))
    else:
        assert not np.array_equal(table, corpus.TileCorpus.validation_table(_Corpus(), 6, None))     # fresh entropy each draw
