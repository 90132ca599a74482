"""No-data in, no-data out — what can be checked without a GPU: the slot map and the slot-aware "which rows are final" logic
against a numpy restatement of the owned rectangles, the new C-ABI symbols and their refusals (all of which come before any
launch), the command-line flag and the environment default."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nodata_restatement as nr  # noqa: E402

from dsen2_amd import _lib, patches  # noqa: E402

FAKE = ctypes.c_void_p(0x1000)           # never dereferenced: every refusal below comes before a launch


# ---- the restatement itself ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('H,W,inner', [(12, 12, 12), (13, 33, 12), (24, 64, 12), (31, 65, 12), (50, 130, 12), (300, 412, 112),
                                       (224, 336, 112), (396, 540, 168)])
def test_owned_rectangles_partition_the_image_and_are_what_the_last_writer_leaves(H, W, inner):
    x_tiles, y_tiles = nr.grid(H, W, inner)
    own = nr.owner_map(H, W, inner)
    seen = np.zeros((H, W), int)
    for ty in range(y_tiles):
        for tx in range(x_tiles):
            y0, y1, x0, x1 = nr.owned_rectangle(ty, tx, H, W, inner)
            assert y1 > y0 and x1 > x0
            assert (own[y0:y1, x0:x1] == ty * x_tiles + tx).all()
            seen[y0:y1, x0:x1] += 1
    assert (seen == 1).all()
    assert (x_tiles, y_tiles) == patches.recompose_grid((H, W), inner, 0)


def test_valid_pixels_definition():
    img = np.zeros((2, 4, 3), np.float32)
    img[0, 1, 2] = -0.0
    img[0, 2, 1] = np.nan
    img[0, 3, 0] = -3.0
    img[1, 0] = (0.0, 1e-45, 0.0)        # the smallest subnormal is data
    img[1, 1, 0] = 5.0                   # one band only (a dark pixel with zero bands elsewhere) is data
    assert nr.valid_pixels(img).tolist() == [[False, False, True, True], [True, True, False, False]]
    bits = nr.pack_bits(np.ones((1, 33), bool))
    assert bits.tolist() == [[0xFFFFFFFF, 1]]


# ---- slot_map and the final-rows logic -----------------------------------------------------------------------------------------
def _empties_of_a_3x4_grid():
    """Every subset of empty patches of a 3 x 4 grid that leaves a whole tile row empty (721 of the 4096 subsets)."""
    for mask in range(1 << 12):
        e = np.array([(mask >> k) & 1 for k in range(12)], np.uint8)
        if e.reshape(3, 4).all(axis=1).any():
            yield e


@pytest.mark.parametrize('H,W', [(36, 48), (31, 41), (36, 41), (25, 48)])      # multiples of inner = 12, and not
def test_slot_map_and_final_rows_on_every_subset_with_an_empty_tile_row(H, W):
    inner = 12
    assert nr.grid(H, W, inner) == (4, 3)
    count = 0
    for empty in _empties_of_a_3x4_grid():
        count += 1
        kept, slots = patches.slot_map(empty)
        want_kept, want_slots = nr.slot_map(empty)
        assert kept.tolist() == want_kept.tolist() and slots.dtype == np.int32 and slots.tolist() == want_slots.tolist()
        n = len(kept)
        # one rank: the batches complete slots in order, whatever the batch size; two ranks: the shards complete side by side
        for per in sorted({n, (n + 1) // 2}):
            done = np.zeros(3, bool)
            covered = np.zeros(H, int)
            for slots_done in range(0, per + 1):
                want_ready = nr.final_rows(slots, slots_done, per, H, W, inner) & ~done
                runs = patches.final_row_runs_slots(slots, slots_done, per, done, (H, W), inner)
                rows = np.zeros(H, int)
                for r0, r1 in runs:
                    assert 0 <= r0 < r1 <= H
                    rows[r0:r1] += 1
                want_rows = np.zeros(H, int)
                for ty in np.nonzero(want_ready)[0]:
                    r0, r1 = nr.tile_row_rows(int(ty), H, inner)
                    want_rows[r0:r1] += 1
                assert (rows == want_rows).all(), (empty.tolist(), per, slots_done)
                assert all(a[1] < b[0] for a, b in zip(runs, runs[1:]))        # merged and ascending
                covered += rows
            assert done.all() and (covered == 1).all(), (empty.tolist(), per)
    assert count == 3 * 2 ** 8 - 3 * 2 ** 4 + 1                                # inclusion-exclusion over the three rows: 721
    # the subset that empties the clamped last tile row alone is among them: its rows are final before anything is computed
    empty = np.array([0] * 8 + [1] * 4, np.uint8)
    _, slots = patches.slot_map(empty)
    done = np.zeros(3, bool)
    assert patches.final_row_runs_slots(slots, 0, 8, done, (H, W), inner) == [(H - inner, H)]
    assert done.tolist() == [False, False, True]


def test_final_rows_without_empty_patches_is_the_existing_logic():
    H, W, inner = 31, 41, 12
    slots = np.arange(12, dtype=np.int32)
    for per in (12, 6, 4):
        for slots_done in range(per + 1):
            a, b = np.zeros(3, bool), np.zeros(3, bool)
            assert patches.final_row_runs_slots(slots, slots_done, per, a, (H, W), inner) == \
                patches.final_row_runs(np.arange(12) % per < slots_done, b, (H, W), inner)
            assert (a == b).all()
    done = np.zeros(3, bool)             # nothing kept: everything is final at once
    assert patches.final_row_runs_slots(np.full(12, -1, np.int32), 0, 0, done, (H, W), inner) == [(0, H)]


def test_skipping_cannot_change_the_image():
    """The restatement's recomposition never reads a patch without a slot for a pixel with data: NaN in the buffer's unused tail
    does not reach the image, and the image is where(valid, full recomposition, 0)."""
    rng = np.random.default_rng(3)
    H, W, P, border = 31, 41, 16, 2
    inner = P - 2 * border
    valid = rng.random((H, W)) < 0.4
    valid[:12, :] = False                # an empty tile row
    empty = nr.patch_empty(valid, inner)
    kept, slots = nr.slot_map(empty)
    assert 0 < len(kept) < 12
    full = rng.standard_normal((12, 3, P, P)).astype(np.float32)
    compact = np.full((len(kept) + 2, 3, P, P), np.nan, np.float32)
    compact[:len(kept)] = full[kept]
    got = nr.recompose(compact[:len(kept)], slots, valid, border, 2000.0)
    want = np.where(valid[:, :, None], nr.recompose(full, np.arange(12), np.ones((H, W), bool), border, 2000.0), np.float32(0))
    assert np.isfinite(got).all() and np.array_equal(got, want)


# ---- the C ABI: symbols, and the refusals that come before the GPU ---------------------------------------------------------------
def test_header_declares_the_nodata_entries():
    header = open(os.path.join(ROOT, 'include', 'dsen2_hip.h')).read()
    lib = _lib.load()
    for name in ('dsen2_tile_nodata_geometry', 'dsen2_tile_nodata', 'dsen2_recompose_rows_nodata'):
        assert re.search(r'\bint %s\s*\(' % name, header) and name in _lib.SIGNATURES and hasattr(lib, name), name


def _refused(code):
    assert code == _lib.ERR_INVALID, code
    assert _lib.load().dsen2_last_error().decode()


def test_geometry_entry_and_its_refusals():
    lib = _lib.load()
    xt, yt, words = ctypes.c_int(), ctypes.c_int(), ctypes.c_size_t()
    out = (ctypes.byref(xt), ctypes.byref(yt), ctypes.byref(words))
    for (H, W, P, b) in ((12, 12, 16, 2), (13, 33, 16, 2), (24, 64, 16, 2), (31, 65, 16, 2), (50, 130, 16, 2), (10980, 10980, 128, 8)):
        assert lib.dsen2_tile_nodata_geometry(H, W, P, b, *out) == _lib.OK
        assert (xt.value, yt.value) == nr.grid(H, W, P - 2 * b) and words.value == H * ((W + 31) // 32)
        assert patches.nodata_geometry((H, W), P, b) == (xt.value, yt.value, words.value)
    assert patches.nodata_geometry((10980, 10980), 128, 8) == (99, 99, 10980 * 344)      # 15.1 MB of bitmap
    for bad in ((12, 12, 16, 8), (12, 12, 16, 9), (11, 12, 16, 2), (12, 11, 16, 2), (0, 12, 16, 2), (12, 12, 0, 0), (12, 12, 16, -1)):
        _refused(lib.dsen2_tile_nodata_geometry(*bad, *out))
    _refused(lib.dsen2_tile_nodata_geometry(12, 12, 16, 2, None, ctypes.byref(yt), ctypes.byref(words)))
    _refused(lib.dsen2_tile_nodata_geometry(12, 12, 16, 2, ctypes.byref(xt), ctypes.byref(yt), None))
    with pytest.raises(_lib.DSen2Error):
        patches.nodata_geometry((11, 12), 16, 2)


def test_launching_entries_refuse_before_they_launch():
    lib = _lib.load()

    def tile(img=FAKE, H=24, W=64, C10=4, P=16, border=2, empty=FAKE, bits=FAKE):
        return lib.dsen2_tile_nodata(img, H, W, C10, P, border, empty, bits, None)
    for kw in (dict(img=None), dict(empty=None), dict(bits=None), dict(C10=0), dict(C10=17), dict(C10=-1), dict(border=8),
               dict(H=11), dict(W=11), dict(H=0), dict(P=0), dict(border=-1)):
        _refused(tile(**kw))

    def rec(p=FAKE, slots=3, C=6, P=16, border=2, smap=FAKE, bits=FAKE, img=FAKE, H=24, W=64, row0=0, row1=24):
        return lib.dsen2_recompose_rows_nodata(p, slots, C, P, border, smap, bits, img, H, W, 2000.0, row0, row1, None)
    for kw in (dict(p=None), dict(smap=None), dict(bits=None), dict(img=None), dict(slots=-1), dict(C=0), dict(border=8), dict(H=11),
               dict(W=11), dict(row0=-1), dict(row1=25), dict(row0=5, row1=4), dict(p=None, slots=0, smap=None)):
        _refused(rec(**kw))
    # an empty row range is accepted and launches nothing (as dsen2_recompose_rows); so is slots == 0 with no patch buffer
    assert rec(row0=7, row1=7) == _lib.OK and rec(p=None, slots=0, row0=7, row1=7) == _lib.OK


# ---- command line and environment ------------------------------------------------------------------------------------------------
def test_cli_skip_nodata_sets_the_module_switch(tmp_path, monkeypatch):
    from dsen2_amd import cli, supres
    seen = []

    def fake20(d10, d20, deep=False):
        seen.append(supres.SKIP_NODATA)
        return np.repeat(np.repeat(np.asarray(d20, np.float32), 2, 0), 2, 1)
    monkeypatch.setattr(supres, 'DSen2_20', fake20)
    monkeypatch.setattr(supres, 'SKIP_NODATA', False)
    src = str(tmp_path / 'tile.npz')
    np.savez(src, data10=np.zeros((12, 12, 4), np.uint16), data20=np.ones((6, 6, 6), np.uint16))
    assert cli.main([src, str(tmp_path / 'plain.npz')]) == 0
    assert cli.main([src, str(tmp_path / 'masked.npz'), '--skip_nodata']) == 0
    assert seen == [False, True]


def test_the_environment_switch_is_read_at_import_and_off_by_default():
    from dsen2_amd import supres
    if os.environ.get('DSEN2_SKIP_NODATA', '0') in ('', '0'):
        assert supres.SKIP_NODATA is False
    code = 'import dsen2_amd.supres as s; print(int(s.SKIP_NODATA is True))'
    for value, want in (('1', '1'), ('0', '0'), ('', '0')):
        out = subprocess.run([sys.executable, '-c', code], cwd=ROOT, env=dict(os.environ, DSEN2_SKIP_NODATA=value),
                             capture_output=True, text=True, check=True).stdout
        assert out.strip().splitlines()[-1] == want, (value, out)


def test_the_keyword_is_keyword_only_and_the_reference_surface_is_unchanged(monkeypatch):
    """DSen2_20 / DSen2_60 report the reference's signature (tests/test_cabi_and_host.py pins it) and take skip_nodata by keyword
    only, None by default; anything else the reference's signature would refuse is still a TypeError."""
    import inspect
    from dsen2_amd import supres
    assert list(inspect.signature(supres.DSen2_20).parameters) == ['d10', 'd20', 'deep']
    assert list(inspect.signature(supres.DSen2_60).parameters) == ['d10', 'd20', 'd60', 'deep']
    seen = []
    monkeypatch.setattr(supres, '_run', lambda dsets, scales, **kw: seen.append((len(dsets), kw['deep'], kw['skip_nodata'])))
    supres.DSen2_20(1, 2)
    supres.DSen2_20(1, 2, True, skip_nodata=True)
    supres.DSen2_60(1, 2, 3, deep=True, skip_nodata=False)
    assert seen == [(2, False, None), (2, True, True), (3, True, False)]
    for bad in (lambda: supres.DSen2_20(1, 2, False, True), lambda: supres.DSen2_20(1, 2, nodata=True), lambda: supres.DSen2_60(1, 2)):
        with pytest.raises(TypeError):
            bad()
    assert supres.last_run_stats() == {} or set(supres.last_run_stats()) == {'patches', 'kept', 'skipped'}
