"""Adjustable overlap and feathered blending — what can be checked without a GPU: the properties of the blend weights on the
numpy restatement (tests/blend_restatement.py), the blend form of "which rows are final" against a brute-force count over the
weighted patches of every row, the new C-ABI symbol and its refusals (all of which come before any launch), the ValueErrors of
the Python surface, the command-line flags and the environment defaults."""
import ctypes
import inspect
import itertools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import blend_restatement as br  # noqa: E402
import nodata_restatement as nr  # noqa: E402

from dsen2_amd import _lib, patches  # noqa: E402

FAKE = ctypes.c_void_p(0x1000)           # never dereferenced: every refusal below comes before a launch


def feathers(b):
    return sorted({1, (b + 1) // 2, b})


# ---- the five properties of the definition ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('P', [16, 128, 192])
def test_weights_cover_every_pixel_with_at_most_three_patches_and_crop_alike(P):
    """Per axis (a patch's weight is the product of its two axis weights, so sums and counts factor): (1) the tile that owns a
    coordinate under "last wins" has weight >= F + 1 there, so the sum is positive; (2) at most 3 tiles carry weight, 3 exactly
    only where the clamped last tile reaches back over two neighbours (L - (T - 1) * inner < 2 b), and always where its
    support does (< 2 F); (3) the weights
    of (P, b, F) are those of (P - 2 (b - F), F, F)."""
    threes = 0
    for b in range(1, P // 4 + 1):
        inner = P - 2 * b
        for F in feathers(b):
            for L in range(inner, 4 * inner + 3):
                w = br.axis_weights(L, P, b, F)
                starts = br.origins(L, inner)
                T = len(starts)
                x = np.arange(L)
                owner = np.where(x >= L - inner, T - 1, x // inner)
                assert (w[owner, x] >= F + 1).all(), (P, b, F, L)
                assert w.max() == 2 * F
                count = (w > 0).sum(axis=0)
                assert 1 <= count.min() and count.max() <= 3, (P, b, F, L)
                if count.max() == 3:
                    threes += 1
                    assert T >= 3 and L - (T - 1) * inner < 2 * b, (P, b, F, L)
                if T >= 3 and L - (T - 1) * inner < 2 * F:                # the last tile's support reaches the one before the last's
                    assert count.max() == 3, (P, b, F, L)
                # support of tile t: [s - F, s + inner + F)
                for t, s in enumerate(starts):
                    nz = np.flatnonzero(w[t])
                    assert (nz[0], nz[-1] + 1) == br.row_support(t, L, inner, F) == (max(0, s - F), min(L, s + inner + F))
                assert np.array_equal(w, br.axis_weights(L, P - 2 * (b - F), F, F)), (P, b, F, L)
    assert threes > 0


@pytest.mark.parametrize('H,W', [(8, 20), (19, 27), (24, 32), (33, 70)])
@pytest.mark.parametrize('F', [1, 3, 4])
def test_single_patch_pixels_are_the_hard_cut_and_agreeing_patches_come_back(H, W, F):
    P, b, C = 16, 4, 3
    inner = P - 2 * b
    x_tiles, y_tiles = br.grid(H, W, inner)
    rng = np.random.default_rng(H * W + F)
    a = rng.standard_normal((x_tiles * y_tiles, C, P, P)).astype(np.float32)
    a[0, 0] = -0.0
    got = br.blend(a, b, F, H, W, 2000.0)
    hard = nr.recompose(a, np.arange(len(a)), np.ones((H, W), bool), b, 2000.0)
    single = br.weighted_patch_count(H, W, P, b, F) == 1
    assert single.any() and not single.all()
    assert np.array_equal(got[single].view(np.int32), hard[single].view(np.int32))            # (4): bit for bit, -0.0 included
    assert not np.array_equal(got[~single], hard[~single])
    image = rng.standard_normal((H, W, C)).astype(np.float32)                                    # (5)
    back = br.blend(br.cut_patches(image, P, b), b, F, H, W, 1.0)
    assert np.array_equal(back.view(np.int32), image.view(np.int32))
    # on crops with (F, F): the same image
    crop = b - F
    cropped = np.ascontiguousarray(a[:, :, crop:P - crop, crop:P - crop])
    assert np.array_equal(br.blend(cropped, F, F, H, W, 2000.0).view(np.int32), got.view(np.int32))


def test_restatement_with_slot_map_and_bitmap():
    """A patch without a slot carries no weight; a pixel without data is 0; NaN in never-read places does not reach the image."""
    H, W, P, b, F, C = 33, 70, 16, 4, 3, 2
    inner = P - 2 * b
    rng = np.random.default_rng(7)
    valid = rng.random((H, W)) < 0.5
    valid[:inner] = False
    empty = nr.patch_empty(valid, inner)
    kept, slots = nr.slot_map(empty)
    assert 0 < len(kept) < empty.size
    full = rng.standard_normal((empty.size, C, P, P)).astype(np.float32)
    compact = full[kept]
    got = br.blend(compact, b, F, H, W, 2000.0, slots=slots, valid=valid)
    assert not got[~valid].any() and np.isfinite(got).all()
    own = nr.owner_map(H, W, inner)
    assert (np.abs(got[valid]).sum(axis=1) > 0).all()                    # every data pixel's owner is kept: the sum is positive
    # the full buffer with the empty patches' weight removed is the same computation
    poisoned = full.copy()
    poisoned[empty != 0] = np.nan
    full_slots = np.where(empty != 0, -1, np.arange(empty.size)).astype(np.int32)
    assert np.array_equal(br.blend(poisoned, b, F, H, W, 2000.0, slots=full_slots, valid=valid), got)
    assert own.shape == (H, W)
    # an out-of-range slot counts as no slot; slots = 0 gives the zero image
    bad = slots.copy()
    bad[kept[0]] = len(kept)
    dropped = slots.copy()
    dropped[kept[0]] = -1
    assert np.array_equal(br.blend(compact, b, F, H, W, 1.0, slots=bad, valid=valid), br.blend(compact, b, F, H, W, 1.0, slots=dropped, valid=valid))
    assert not br.blend(compact[:0], b, F, H, W, 1.0, slots=slots, valid=valid).any()


# ---- which rows are final ----------------------------------------------------------------------------------------------------------
def _brute_final(have, H, W, P, b, F):
    """bool [H]: every patch that carries weight somewhere on the row is there."""
    inner = P - 2 * b
    x_tiles, y_tiles = br.grid(H, W, inner)
    wy, wx = br.axis_weights(H, P, b, F), br.axis_weights(W, P, b, F)
    out = np.ones(H, bool)
    for y in range(H):
        for ty in range(y_tiles):
            for tx in range(x_tiles):
                if wy[ty, y] * wx[tx].max() > 0 and not have[ty * x_tiles + tx]:
                    out[y] = False
    return out


@pytest.mark.parametrize('H,W', [(24, 32), (19, 27), (24, 27), (17, 32), (23, 26)])
@pytest.mark.parametrize('F', [1, 3, 4])
def test_final_rows_in_every_completion_order_of_a_3x4_grid(H, W, F):
    P, b = 16, 4
    inner = P - 2 * b
    assert br.grid(H, W, inner) == (4, 3)
    for order in itertools.permutations(range(3)):
        have = np.zeros(12, bool)
        done = np.zeros(H, bool)
        assert patches.final_row_runs_blend(have, done, (H, W), inner, F) == [] and not done.any()
        for step, ty in enumerate(order):
            for tx in range(4):                                          # a tile row completes patch by patch
                have[ty * 4 + tx] = True
                before = done.copy()
                runs = patches.final_row_runs_blend(have, done, (H, W), inner, F)
                want = _brute_final(have, H, W, P, b, F)
                assert np.array_equal(done, want), (order, ty, tx)
                rows = np.zeros(H, int)
                for r0, r1 in runs:
                    assert 0 <= r0 < r1 <= H
                    rows[r0:r1] += 1
                assert np.array_equal(rows, (want & ~before).astype(int))
                assert all(a[1] < c[0] for a, c in zip(runs, runs[1:]))            # merged and ascending
        assert done.all()
    for ty in range(3):
        assert patches.blend_row_support(ty, (H, W), inner, F) == br.row_support(ty, H, inner, F)


@pytest.mark.parametrize('H,W', [(24, 32), (19, 27)])
def test_final_rows_slot_form_with_empty_patches(H, W):
    P, b, F = 16, 4, 3
    inner = P - 2 * b
    rng = np.random.default_rng(H)
    cases = [np.array([0] * 8 + [1] * 4, np.uint8), np.array([1] * 4 + [0] * 8, np.uint8), np.array([1, 0, 1, 0] * 3, np.uint8)]
    cases += [(rng.random(12) < 0.4).astype(np.uint8) for _ in range(12)]
    for empty in cases:
        kept, slots = patches.slot_map(empty)
        n = len(kept)
        for per in sorted({n, (n + 1) // 2}):
            done = np.zeros(H, bool)
            covered = np.zeros(H, int)
            for slots_done in range(0, per + 1):
                have = (slots < 0) | ((slots >= 0) & (slots % max(per, 1) < slots_done) & (per > 0))
                runs = patches.final_row_runs_slots_blend(slots, slots_done, per, done, (H, W), inner, F)
                assert np.array_equal(done, _brute_final(have, H, W, P, b, F)), (empty.tolist(), per, slots_done)
                for r0, r1 in runs:
                    covered[r0:r1] += 1
            assert done.all() and (covered == 1).all(), (empty.tolist(), per)
    done = np.zeros(H, bool)             # nothing kept: everything is final at once
    assert patches.final_row_runs_slots_blend(np.full(12, -1, np.int32), 0, 0, done, (H, W), inner, F) == [(0, H)]


# ---- the C ABI: the symbol, and the refusals that come before the GPU --------------------------------------------------------------
def test_header_declares_the_blend_entry_and_the_signature_agrees():
    header = open(os.path.join(ROOT, 'include', 'dsen2_hip.h')).read()
    name = 'dsen2_recompose_rows_blend'
    m = re.search(r'\bint %s\s*\(([^)]*)\)' % name, header)
    assert m and name in _lib.SIGNATURES and hasattr(_lib.load(), name)
    params = [p.strip() for p in m.group(1).split(',')]
    restype, argtypes = _lib.SIGNATURES[name]
    assert restype is ctypes.c_int and len(params) == len(argtypes) == 15
    for p, t in zip(params, argtypes):
        want = ctypes.c_void_p if '*' in p else ctypes.c_float if p.startswith('float ') else ctypes.c_int
        assert t is want, (p, t)
    assert [p.split()[-1].lstrip('*') for p in params] == ['dev_patches', 'count_or_slots', 'C', 'P', 'border', 'feather', 'dev_slot_of_patch',
                                                          'dev_valid_bits', 'dev_img', 'H', 'W', 'scale', 'row0', 'row1', 'stream']


def _refused(code):
    assert code == _lib.ERR_INVALID, code
    assert _lib.load().dsen2_last_error().decode()


def test_the_blend_entry_refuses_before_it_launches():
    lib = _lib.load()

    def rec(p=FAKE, count=24, C=6, P=16, border=4, feather=3, smap=None, bits=None, img=FAKE, H=24, W=64, row0=0, row1=24):
        return lib.dsen2_recompose_rows_blend(p, count, C, P, border, feather, smap, bits, img, H, W, 2000.0, row0, row1, None)
    for kw in (dict(p=None), dict(img=None), dict(smap=FAKE), dict(bits=FAKE), dict(C=0), dict(C=-1), dict(count=23), dict(count=-1),
               dict(border=5), dict(border=8), dict(border=0, feather=0), dict(border=-1), dict(feather=0), dict(feather=5), dict(feather=-1),
               dict(H=7), dict(W=7), dict(H=0), dict(P=0), dict(row0=-1), dict(row1=25), dict(row0=5, row1=4),
               dict(p=None, count=0), dict(p=None, smap=FAKE, bits=FAKE, count=1), dict(smap=FAKE, bits=FAKE, count=-1),
               dict(P=128, border=33, feather=8, H=300, W=300, count=100), dict(P=192, border=49, feather=8, H=300, W=300, count=100)):
        _refused(rec(**kw))
    # an empty row range is accepted and launches nothing (as dsen2_recompose_rows); so is slots == 0 with no patch buffer
    assert rec(row0=7, row1=7) == _lib.OK
    assert rec(p=None, count=0, smap=FAKE, bits=FAKE, row0=7, row1=7) == _lib.OK
    assert rec(P=128, border=32, feather=32, H=300, W=300, count=100, row0=0, row1=0) == _lib.OK
    assert rec(smap=FAKE, bits=FAKE, count=1, row0=24, row1=24) == _lib.OK             # a compact buffer may hold fewer patches than the grid


# ---- the Python surface ------------------------------------------------------------------------------------------------------------
def test_feather_width():
    for off in (None, False, 0, np.int64(0)):
        assert patches.feather_width(off, 8) == 0
    assert patches.feather_width(True, 8) == 8 and patches.feather_width(1, 8) == 1 and patches.feather_width(np.int32(8), 8) == 8
    for bad in (9, -1, 2.0, '4', 1.5):
        with pytest.raises(ValueError):
            patches.feather_width(bad, 8)


def test_bad_border_or_feather_is_a_value_error_before_the_gpu(monkeypatch):
    from dsen2_amd import supres

    def no_gpu(*a, **k):
        raise AssertionError('the GPU was touched')
    monkeypatch.setattr(patches, 'default_device', no_gpu)
    monkeypatch.setattr(patches, '_to_device_f32', no_gpu)
    d10, d20, d60 = np.ones((384, 384, 4), np.uint16), np.ones((192, 192, 6), np.uint16), np.ones((64, 64, 2), np.uint16)
    for kw in (dict(border=7), dict(border=0), dict(border=34), dict(border=-2), dict(border=8.0), dict(border=True), dict(feather=9),
               dict(feather=-1), dict(border=16, feather=17), dict(feather=2.5), dict(feather='3')):
        with pytest.raises(ValueError):
            supres.DSen2_20(d10, d20, **kw)
    for kw in (dict(border=8), dict(border=0), dict(border=54), dict(border=50), dict(feather=13), dict(border=18, feather=19)):
        with pytest.raises(ValueError):
            supres.DSen2_60(d10, d20, d60, **kw)
    # the module switches are checked the same way
    monkeypatch.setattr(supres, 'BORDER_20', 9)
    with pytest.raises(ValueError):
        supres.DSen2_20(d10, d20)
    monkeypatch.setattr(supres, 'BORDER_20', 8)
    monkeypatch.setattr(supres, 'FEATHER', 12)
    with pytest.raises(ValueError):
        supres.DSen2_20(d10, d20)
    monkeypatch.setattr(supres, 'FEATHER', None)
    # recompose_images refuses a bad feather before it uploads anything
    with pytest.raises(ValueError):
        patches.recompose_images(np.zeros((4, 2, 16, 16), np.float32), 4, size=(16, 16), feather=5)
    # legal values get past the check (and reach the stand-in for the GPU)
    for kw in (dict(border=2), dict(border=32, feather=32), dict(border=16, feather=True), dict(feather=8)):
        with pytest.raises(AssertionError, match='the GPU was touched'):
            supres.DSen2_20(d10, d20, **kw)
    with pytest.raises(AssertionError, match='the GPU was touched'):
        supres.DSen2_60(d10, d20, d60, border=48, feather=1)


def test_the_keywords_reach_run_and_the_reference_surface_is_unchanged(monkeypatch):
    from dsen2_amd import supres
    assert list(inspect.signature(supres.DSen2_20).parameters) == ['d10', 'd20', 'deep']
    assert list(inspect.signature(supres.DSen2_60).parameters) == ['d10', 'd20', 'd60', 'deep']
    seen = []
    monkeypatch.setattr(supres, '_run', lambda dsets, scales, **kw: seen.append((len(dsets), kw['patch'], kw['border'], kw['feather'], kw['skip_nodata'])))
    monkeypatch.setattr(supres, 'BORDER_20', 8)
    monkeypatch.setattr(supres, 'BORDER_60', 12)
    monkeypatch.setattr(supres, 'FEATHER', None)
    supres.DSen2_20(1, 2)
    supres.DSen2_20(1, 2, True, border=16, feather=4)
    supres.DSen2_60(1, 2, 3, feather=True, skip_nodata=True)
    monkeypatch.setattr(supres, 'BORDER_20', 16)
    monkeypatch.setattr(supres, 'BORDER_60', 18)
    monkeypatch.setattr(supres, 'FEATHER', 6)
    supres.DSen2_20(1, 2)
    supres.DSen2_60(1, 2, 3)
    supres.DSen2_60(1, 2, 3, border=12, feather=False)
    assert seen == [(2, 128, 8, None, None), (2, 128, 16, 4, None), (3, 192, 12, True, True), (2, 128, 16, 6, None), (3, 192, 18, 6, None),
                    (3, 192, 12, False, None)]
    for bad in (lambda: supres.DSen2_20(1, 2, False, None, 16), lambda: supres.DSen2_20(1, 2, overlap=16), lambda: supres.DSen2_60(1, 2, border=12)):
        with pytest.raises(TypeError):
            bad()


# ---- command line and environment ------------------------------------------------------------------------------------------------
def test_cli_flags_set_the_module_switches(tmp_path, monkeypatch):
    from dsen2_amd import cli, supres
    seen = []

    def fake20(d10, d20, deep=False):
        seen.append((supres.BORDER_20, supres.BORDER_60, supres.FEATHER))
        return np.repeat(np.repeat(np.asarray(d20, np.float32), 2, 0), 2, 1)
    monkeypatch.setattr(supres, 'DSen2_20', fake20)
    for name, value in (('BORDER_20', 8), ('BORDER_60', 12), ('FEATHER', None)):
        monkeypatch.setattr(supres, name, value)
    src = str(tmp_path / 'tile.npz')
    np.savez(src, data10=np.zeros((12, 12, 4), np.uint16), data20=np.ones((6, 6, 6), np.uint16))
    assert cli.main([src, str(tmp_path / 'a.npz')]) == 0
    assert cli.main([src, str(tmp_path / 'b.npz'), '--border20', '16', '--feather', '4']) == 0
    assert cli.main([src, str(tmp_path / 'c.npz'), '--border60', '18', '--feather', '0']) == 0
    assert seen == [(8, 12, None), (16, 12, 4), (16, 18, None)]


def test_train_predict_takes_feather():
    from dsen2_amd import train
    args = train.parse_args(['--predict', 'w.npy', '--feather', '4'])
    assert args.feather == 4 and train.parse_args(['--predict', 'w.npy']).feather is None
    for bad in (['--feather', '4'], ['--predict', 'w.npy', '--feather', '0']):
        with pytest.raises(SystemExit):
            train.parse_args(bad)


def test_the_environment_switches_are_read_at_import_and_off_by_default():
    code = 'import dsen2_amd.supres as s; print(repr((s.BORDER_20, s.BORDER_60, s.FEATHER)))'
    base = {k: v for k, v in os.environ.items() if k not in ('DSEN2_BORDER_20', 'DSEN2_BORDER_60', 'DSEN2_FEATHER')}
    for env, want in (({}, (8, 12, None)), ({'DSEN2_BORDER_20': '16', 'DSEN2_BORDER_60': '18', 'DSEN2_FEATHER': '4'}, (16, 18, 4)),
                      ({'DSEN2_BORDER_20': '', 'DSEN2_FEATHER': '0'}, (8, 12, None)), ({'DSEN2_FEATHER': 'true'}, (8, 12, True))):
        out = subprocess.run([sys.executable, '-c', code], cwd=ROOT, env=dict(base, **env), capture_output=True, text=True, check=True).stdout
        assert out.strip().splitlines()[-1] == repr(want), (env, out)
