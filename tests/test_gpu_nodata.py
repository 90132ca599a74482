"""No-data in, no-data out on the GPU: dsen2_tile_nodata and dsen2_recompose_rows_nodata bit for bit against the numpy
restatement (tests/nodata_restatement.py) and inside guard bands; DSen2_20 / DSen2_60 with skip_nodata against
where(valid, the image the option off returns, 0) for every precision, ending and batch size; the command line; two gloo ranks.
Everything is an equality: no tolerance anywhere."""
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
import nodata_restatement as nr  # noqa: E402
from guarded import run_three_ways  # noqa: E402

from dsen2_amd import _lib, patches, weights  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
P, BORDER, INNER = 16, 2, 12
SHAPES = [(12, 12), (13, 33), (24, 64), (31, 65), (50, 130)]
BANDS = [(1, 2), (3, 5), (4, 6)]                  # (C10, C)


def _bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


# ---- rasters ---------------------------------------------------------------------------------------------------------------------
def _overlap_pixel(H, W):
    """A pixel that lies inside the square of a tile before the last one but is overwritten by the clamped last tile (None on an
    axis whose extent is a multiple of inner)."""
    ys, xs = nr.origins(H, INNER), nr.origins(W, INNER)
    y = ys[-1] + 1 if len(ys) > 1 and ys[-1] < ys[-2] + INNER else None
    x = xs[-1] + 1 if len(xs) > 1 and xs[-1] < xs[-2] + INNER else None
    return y, x


def rasters(H, W, C10, seed):
    """name -> float32 [H, W, C10]: the cases the kernels must tell apart."""
    rng = np.random.default_rng(seed)
    data = rng.uniform(1.0, 9000.0, size=(H, W, C10)).astype(np.float32)
    out = {'none': np.zeros((H, W, C10), np.float32), 'all': data.copy()}
    x_tiles, y_tiles = nr.grid(H, W, INNER)
    corners = np.zeros((H, W, C10), np.float32)            # the four corners of every other owned rectangle, one band each
    for ty in range(y_tiles):
        for tx in range(x_tiles):
            if (ty + tx) % 2 == 0:
                y0, y1, x0, x1 = nr.owned_rectangle(ty, tx, H, W, INNER)
                for i, (y, x) in enumerate(((y0, x0), (y0, x1 - 1), (y1 - 1, x0), (y1 - 1, x1 - 1))):
                    corners[y, x, i % C10] = 7.0
    out['corners'] = corners
    oy, ox = _overlap_pixel(H, W)
    if oy is not None or ox is not None:                   # data ONLY where the clamped last tile overwrites its neighbour
        over = np.zeros((H, W, C10), np.float32)
        over[oy if oy is not None else 0, ox if ox is not None else 0, C10 - 1] = 3.0
        out['overlap'] = over
    mixed = data.copy()
    blocks = rng.random((H // 5 + 1, W // 7 + 1)) < 0.5
    mixed[np.kron(blocks, np.ones((5, 7), bool))[:H, :W]] = 0.0
    mixed[rng.random((H, W)) < 0.3] = -0.0                  # -0.0 in every band: no data
    mixed[0, 0] = -0.0
    mixed[H - 1, W - 1] = 0.0
    mixed[H - 1, W - 1, C10 - 1] = np.nan                   # a NaN in one band: data
    mixed[H // 2, W // 2] = 0.0
    mixed[H // 2, W // 2, 0] = -1.0                         # a negative value in one band: data
    mixed[0, W - 1] = 0.0
    mixed[0, W - 1, 0] = 1e-45                              # the smallest subnormal: data
    out['mixed'] = mixed
    return out


def run_tile_nodata(img):
    empty, bits = patches.nodata_device(torch.from_numpy(img).to(DEV), P, BORDER)
    return empty.cpu().numpy(), bits.cpu().numpy().view(np.uint32)


# ---- kernel level ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('C10,C', BANDS)
@pytest.mark.parametrize('H,W', SHAPES)
def test_kernels_equal_the_restatement_bit_for_bit(H, W, C10, C):
    x_tiles, y_tiles = nr.grid(H, W, INNER)
    n = x_tiles * y_tiles
    rng = np.random.default_rng(H * 1000 + W + C)
    full = rng.standard_normal((n, C, P, P)).astype(np.float32)
    for name, img in rasters(H, W, C10, seed=H + W + C10).items():
        valid = nr.valid_pixels(img)
        want_empty, want_bits = nr.patch_empty(valid, INNER), nr.pack_bits(valid)
        empty, bits = run_tile_nodata(img)
        assert empty.dtype == np.uint8 and np.array_equal(empty, want_empty), (name, empty.tolist(), want_empty.tolist())
        assert bits.shape == want_bits.shape and np.array_equal(bits, want_bits), name
        if name == 'none':
            assert empty.all() and not bits.any()
        if name == 'all':
            assert not empty.any()
        if name == 'overlap':
            assert (empty == 0).sum() == 1             # the tile whose square also covers the pixel, but loses it, is empty
        # recomposition: the full buffer's empty patches and the compact buffer's unused tail hold NaN
        kept, slots = patches.slot_map(empty)
        assert kept.tolist() == nr.slot_map(want_empty)[0].tolist()
        poisoned = full.copy()
        poisoned[want_empty != 0] = np.nan
        compact = np.full((len(kept) + 3, C, P, P), np.nan, np.float32)
        compact[:len(kept)] = full[kept]
        c_dev, f_dev = torch.from_numpy(compact).to(DEV), torch.from_numpy(poisoned).to(DEV)
        s_dev, b_dev = torch.from_numpy(slots).to(DEV), torch.from_numpy(bits.view(np.int32)).to(DEV)
        one = torch.full((H, W, C), -7.0, device=DEV)
        patches.recompose_rows_device(c_dev, BORDER, one, 0, H, scale=2000.0, slots=s_dev, valid_bits=b_dev)
        want = torch.from_numpy(nr.recompose(compact, slots, valid, BORDER, 2000.0)).to(DEV)
        assert same_bits(one, want), name
        off = patches.recompose_device(f_dev, BORDER, (H, W), scale=2000.0)
        masked = torch.where(torch.from_numpy(valid).to(DEV)[:, :, None], off, torch.zeros_like(off))
        assert same_bits(one, masked) and bool(torch.isfinite(one).all()), name
        for step in (1, 2, INNER):
            img_b = torch.full((H, W, C), -7.0, device=DEV)
            for r0 in range(0, H, step):
                r1 = min(H, r0 + step)
                patches.recompose_rows_device(c_dev, BORDER, img_b, r0, r1, scale=2000.0, slots=s_dev, valid_bits=b_dev)
                assert bool((img_b[r1:] == -7.0).all())                    # rows outside the band are not touched
            assert same_bits(img_b, one), (name, step)


@pytest.mark.parametrize('H,W', SHAPES)
def test_a_single_pixel_at_each_corner_of_each_owned_rectangle(H, W):
    """One pixel with data in the whole raster, at a corner of an owned rectangle: that patch alone is not empty, and the bitmap
    holds that one bit."""
    x_tiles, y_tiles = nr.grid(H, W, INNER)
    img_dev = torch.zeros((H, W, 4), dtype=torch.float32, device=DEV)
    flags, rows = [], []
    for ty in range(y_tiles):
        for tx in range(x_tiles):
            y0, y1, x0, x1 = nr.owned_rectangle(ty, tx, H, W, INNER)
            for y, x in ((y0, x0), (y0, x1 - 1), (y1 - 1, x0), (y1 - 1, x1 - 1)):
                img_dev[y, x, (y + x) % 4] = 1.0
                empty, bits = patches.nodata_device(img_dev, P, BORDER)
                img_dev[y, x] = 0.0
                flags.append(empty)
                rows.append((ty * x_tiles + tx, y, x, bits))
    flags = torch.stack(flags).cpu().numpy()
    for i, (k, y, x, bits) in enumerate(rows):
        want = np.ones(x_tiles * y_tiles, np.uint8)
        want[k] = 0
        assert np.array_equal(flags[i], want), (k, y, x)
    k, y, x, bits = rows[-1]
    want_bits = np.zeros((H, (W + 31) // 32), np.uint32)
    want_bits[y, x >> 5] = np.uint32(1) << np.uint32(x & 31)
    assert np.array_equal(bits.cpu().numpy().view(np.uint32), want_bits)


def test_a_pointer_that_is_not_16_byte_aligned_takes_the_general_kernel():
    H, W = 31, 65
    img = rasters(H, W, 4, seed=9)['mixed']
    base = torch.zeros(H * W * 4 + 1, dtype=torch.float32, device=DEV)
    base[1:].copy_(torch.from_numpy(img).reshape(-1))
    shifted = base[1:].view(H, W, 4)
    assert shifted.data_ptr() % 16 == 4
    a = patches.nodata_device(torch.from_numpy(img).to(DEV), P, BORDER)
    b = patches.nodata_device(shifted, P, BORDER)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ---- memory contract -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('C10,C', [(3, 5), (4, 6), (6, 2)])
def test_both_entry_points_inside_guard_bands(C10, C):
    H, W = 31, 65
    x_tiles, y_tiles, words = patches.nodata_geometry((H, W), P, BORDER)
    n = x_tiles * y_tiles
    raster = rasters(H, W, C10, seed=C10)['mixed']
    for ty, tx in ((0, 1), (2, 5)):                      # two empty patches for certain
        y0, y1, x0, x1 = nr.owned_rectangle(ty, tx, H, W, INNER)
        raster[y0:y1, x0:x1] = 0.0
    img = torch.from_numpy(raster).to(DEV)

    def tile(inputs, outputs, inplace, scratch):
        _lib.call('dsen2_tile_nodata', patches._ptr(inputs[0]), H, W, C10, P, BORDER, patches._ptr(outputs[0]), patches._ptr(outputs[1]),
                  patches._stream(DEV))
    (empty, bits), _ = run_three_ways(tile, [img], [((n,), torch.uint8), ((H, words // H), torch.int32)], what='dsen2_tile_nodata')
    valid = nr.valid_pixels(img.cpu().numpy())
    assert np.array_equal(empty.cpu().numpy(), nr.patch_empty(valid, INNER))
    assert np.array_equal(bits.cpu().numpy().view(np.uint32), nr.pack_bits(valid))

    kept, slots = patches.slot_map(empty.cpu().numpy())
    assert 2 <= len(kept) < n
    rng = np.random.default_rng(C)
    compact = torch.from_numpy(rng.standard_normal((len(kept), C, P, P)).astype(np.float32)).to(DEV)
    # slots that are out of range — one past the end, far beyond, negative — must write 0 and read nothing
    bad = slots.copy()
    bad[kept[0]], bad[kept[1]] = len(kept), 10 ** 6
    bad[np.nonzero(slots < 0)[0][0]] = -5
    for smap, dropped in ((slots, []), (bad, [kept[0], kept[1]])):
        s_dev = torch.from_numpy(smap).to(DEV)

        def rec(inputs, outputs, inplace, scratch):
            _lib.call('dsen2_recompose_rows_nodata', patches._ptr(inputs[0]), inputs[0].shape[0], C, P, BORDER, patches._ptr(inputs[1]),
                      patches._ptr(inputs[2]), patches._ptr(outputs[0]), H, W, 2000.0, 0, H, patches._stream(DEV))
        (out,), _ = run_three_ways(rec, [compact, s_dev, bits], [((H, W, C), torch.float32)], what='dsen2_recompose_rows_nodata')
        want_slots = smap.copy()
        want_slots[dropped] = -1
        want = nr.recompose(compact.cpu().numpy(), want_slots, valid, BORDER, 2000.0)
        assert same_bits(out, torch.from_numpy(want).to(DEV))
        if dropped:
            own = nr.owner_map(H, W, INNER)
            gone = np.isin(own, dropped)
            assert valid[gone].any() and not out.cpu().numpy()[gone].any()
    # slots == 0: every pixel is 0 and the patch buffer may be NULL
    img0 = torch.full((H, W, C), -7.0, device=DEV)
    _lib.call('dsen2_recompose_rows_nodata', None, 0, C, P, BORDER, patches._ptr(torch.from_numpy(slots).to(DEV)), patches._ptr(bits),
              patches._ptr(img0), H, W, 2000.0, 0, H, patches._stream(DEV))
    assert not bool(img0.any())


# ---- end to end --------------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def model_dir(tmp_path, monkeypatch):
    """A MDL_PATH holding synthetic checkpoints under the reference's file names (as .npy), as tests/test_gpu_supres.py's."""
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


CASES = {'20_300x412': (False, 300, 412), '20_224x336': (False, 224, 336), '60_396x540': (True, 396, 540)}


def nodata_mask(H, W, inner):
    """bool [H, W], True = no data: the lower-right region x/W + y/H >= 0.9, a lone pixel with data at (H-3, W-2) inside it, and a
    hole across the last overlap column (the last column of the tile before the clamped one that the clamped one overwrites).  A
    grid without an overlap (the exact 2 x 3 one) has no empty patch under that: two owned rectangles are blanked."""
    y, x = np.mgrid[0:H, 0:W]
    nod = x / float(W) + y / float(H) >= 0.9
    nod[H - 3, W - 2] = False
    x_tiles, y_tiles = nr.grid(H, W, inner)
    if (x_tiles - 1) * inner > W - inner:
        nod[:, (x_tiles - 1) * inner - 1] = True
    if nr.patch_empty(~nod, inner).sum() < 2:
        for ty, tx in ((0, 1), (1, 0)):
            y0, y1, x0, x1 = nr.owned_rectangle(ty, tx, H, W, inner)
            nod[y0:y1, x0:x1] = True
    return nod


def case_inputs(name):
    """(function name, [d10, d20(, d60)] uint16, valid bool [H, W], inner)"""
    run_60, H, W = CASES[name]
    inner = 168 if run_60 else 112
    rng = np.random.default_rng(H + W)
    d10 = rng.integers(35, 9000, size=(H, W, 4), dtype=np.uint16)
    d10[nodata_mask(H, W, inner)] = 0
    args = [d10, rng.integers(35, 9000, size=(H // 2, W // 2, 6), dtype=np.uint16)]
    if run_60:
        args.append(rng.integers(35, 9000, size=(H // 6, W // 6, 2), dtype=np.uint16))
    return ('DSen2_60' if run_60 else 'DSen2_20'), args, nr.valid_pixels(d10), inner


def patch_census(valid, inner):
    """(patches, kept, partly valid) by the restatement."""
    empty = nr.patch_empty(valid, inner)
    own = nr.owner_map(valid.shape[0], valid.shape[1], inner)
    partly = sum(1 for k in range(empty.size) if valid[own == k].any() and not valid[own == k].all())
    return empty.size, int((empty == 0).sum()), partly


def check_case(name, **kw):
    """R_on == where(valid, R_off, 0) bit for bit, the same prints, and the kept count of the restatement."""
    from dsen2_amd import supres
    fn_name, args, valid, inner = case_inputs(name)
    fn = getattr(supres, fn_name)
    n, kept, partly = patch_census(valid, inner)
    assert n - kept >= 2 and partly >= 2, (name, n, kept, partly)             # or the case shows nothing
    off, printed_off = quiet(fn, *args, deep=False, skip_nodata=False)
    assert supres.last_run_stats() == {'patches': n, 'kept': n, 'skipped': 0}
    on, printed_on = quiet(fn, *args, deep=False, skip_nodata=True, **kw)
    assert supres.last_run_stats() == {'patches': n, 'kept': kept, 'skipped': n - kept}
    assert on.shape == off.shape == valid.shape + (off.shape[2],) and on.dtype == np.float32
    want = np.where(valid[:, :, None], off, np.float32(0))
    assert np.array_equal(on.view(np.int32), want.view(np.int32)), name
    assert np.abs(off[~valid]).max() > 0                                       # the option off does return net(0) * 2000 there
    assert printed_on == printed_off
    return on, args, valid


def test_the_cases_have_empty_and_partly_valid_patches():
    for name in CASES:
        _, _, valid, inner = case_inputs(name)
        n, kept, partly = patch_census(valid, inner)
        assert n - kept >= 2 and partly >= 2, (name, n, kept, partly)
    assert patch_census(case_inputs('20_300x412')[2], 112) == (12, 9, 7)
    assert patch_census(case_inputs('60_396x540')[2], 168) == (12, 9, 7)


@pytest.mark.parametrize('precision', ['fp32', 'bf16', 'bf16x3'])
@pytest.mark.parametrize('name', list(CASES))
def test_on_equals_the_masked_off_image(model_dir, monkeypatch, name, precision):
    from dsen2_amd import supres
    monkeypatch.setattr(supres, 'PRECISION', precision)
    check_case(name)


@pytest.mark.parametrize('name', list(CASES))
def test_module_switch_and_self_ensemble(model_dir, monkeypatch, name):
    """skip_nodata=None reads supres.SKIP_NODATA; SELF_ENSEMBLE composes (only `forward` is swapped)."""
    from dsen2_amd import supres
    monkeypatch.setattr(supres, 'SELF_ENSEMBLE', True)
    on, args, valid = check_case(name)
    fn = getattr(supres, case_inputs(name)[0])
    monkeypatch.setattr(supres, 'SKIP_NODATA', True)
    again, _ = quiet(fn, *args)
    assert np.array_equal(on, again) and supres.last_run_stats()['skipped'] >= 2
    monkeypatch.setattr(supres, 'SKIP_NODATA', False)
    quiet(fn, *args)
    assert supres.last_run_stats()['skipped'] == 0


@pytest.mark.parametrize('ending', ['banded', 'one_shot', 'pageable'])
@pytest.mark.parametrize('limit', [1, 5])
@pytest.mark.parametrize('name', list(CASES))
def test_every_ending_and_batch_size(model_dir, monkeypatch, name, limit, ending):
    from dsen2_amd import supres
    from dsen2_amd.DSen2Net import S2Model
    monkeypatch.setattr(supres, 'PINNED_OUTPUT_MIN_BYTES', 0)
    monkeypatch.delenv('DSEN2_BANDED_OUTPUT', raising=False)
    monkeypatch.delenv('DSEN2_PINNED_OUTPUT', raising=False)
    if ending == 'one_shot':
        monkeypatch.setenv('DSEN2_BANDED_OUTPUT', '0')
    if ending == 'pageable':
        monkeypatch.setenv('DSEN2_PINNED_OUTPUT', '0')
    monkeypatch.setattr(S2Model, 'batch_limit', lambda self, hh, ww: limit)
    check_case(name)


def test_dtypes_and_views_give_the_same_image(model_dir):
    from dsen2_amd import supres
    on, args, valid = check_case('20_300x412')
    as_f32 = [a.astype(np.float32) for a in args]
    assert np.array_equal(quiet(supres.DSen2_20, *as_f32, skip_nodata=True)[0], on)
    views = [np.rollaxis(np.ascontiguousarray(np.rollaxis(a, 2, 0)), 0, 3) for a in args]       # HWC views of CHW arrays
    assert not views[0].flags.c_contiguous
    assert np.array_equal(quiet(supres.DSen2_20, *views, skip_nodata=True)[0], on)
    neg = as_f32[0].copy()
    neg[~valid] = -0.0                                                           # -0.0 is no data too
    assert np.array_equal(quiet(supres.DSen2_20, neg, as_f32[1], skip_nodata=True)[0], on)


@pytest.mark.parametrize('name', list(CASES))
def test_all_nodata_returns_zeros_without_a_forward(model_dir, monkeypatch, name):
    from dsen2_amd import supres
    from dsen2_amd.DSen2Net import S2Model
    fn_name, args, valid, inner = case_inputs(name)
    fn = getattr(supres, fn_name)
    _, printed_off = quiet(fn, *args, skip_nodata=False)

    def never(self, *a, **k):
        raise AssertionError('a forward pass ran on a tile without data')
    monkeypatch.setattr(S2Model, 'forward_device', never)
    monkeypatch.setattr(S2Model, 'forward_device_ensemble', never)
    args[0] = np.zeros_like(args[0])
    out, printed = quiet(fn, *args, skip_nodata=True)
    assert out.shape == valid.shape + (2 if fn_name == 'DSen2_60' else 6,) and out.dtype == np.float32 and not out.any()
    assert printed == printed_off
    n = nr.patch_empty(valid, inner).size
    assert supres.last_run_stats() == {'patches': n, 'kept': 0, 'skipped': n}


@pytest.mark.parametrize('name', list(CASES))
def test_fully_valid_input_is_the_off_image(model_dir, name):
    from dsen2_amd import supres
    fn_name, args, valid, inner = case_inputs(name)
    fn = getattr(supres, fn_name)
    rng = np.random.default_rng(1)
    args[0] = rng.integers(35, 9000, size=args[0].shape, dtype=np.uint16)
    off, p_off = quiet(fn, *args, skip_nodata=False)
    on, p_on = quiet(fn, *args, skip_nodata=True)
    st = supres.last_run_stats()
    assert np.array_equal(on.view(np.int32), off.view(np.int32)) and p_on == p_off
    assert st['kept'] == st['patches'] == nr.patch_empty(valid, inner).size and st['skipped'] == 0


def test_cli_skip_nodata_on_an_npz(model_dir, tmp_path, monkeypatch):
    from dsen2_amd import cli, supres
    monkeypatch.setattr(supres, 'SKIP_NODATA', False)
    on, args, valid = check_case('20_300x412')
    inp, out = str(tmp_path / 'tile.npz'), str(tmp_path / 'sr.npz')
    np.savez(inp, data10=args[0], data20=args[1])
    rc, printed = quiet(cli.main, [inp, out, '--skip_nodata', '--models', supres.MDL_PATH])
    assert rc == 0 and supres.SKIP_NODATA is True
    bands = np.load(out, allow_pickle=True)['bands'].item()
    assert list(bands) == ['SRB5', 'SRB6', 'SRB7', 'SRB8A', 'SRB11', 'SRB12']
    for i, b in enumerate(bands.values()):
        assert np.array_equal(b, on[:, :, i])
    assert not bands['SRB5'][~valid].any()


# ---- two gloo ranks sharing the GPU ------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return str(p)


@pytest.mark.parametrize('chunked', [False, True])
def test_two_ranks_equal_the_single_rank_image(chunked):
    """tools/bench_skip_nodata.py under two gloo ranks on a 1200^2 tile (121 patches): a diagonal half without data, and a tile
    with data in ONE patch — fewer kept patches than ranks, so rank 1's shard is empty.  Rank 0's image equals the single-rank
    image and where(valid, option off, 0); rank 1 returns None (the tool asserts it)."""
    env = dict(os.environ)
    env.pop('DSEN2_CHUNKED_GATHER', None)
    if chunked:
        env['DSEN2_CHUNKED_GATHER'] = '1'
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2', '--master-addr', '127.0.0.1',
           '--master-port', _free_port(), os.path.join(ROOT, 'tools', 'bench_skip_nodata.py'), '--size', '1200', '--backend', 'gloo',
           '--check', '--masks', 'diagonal,few']
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    assert p.returncode == 0, p.stderr[-2000:]
    r = json.loads([line for line in p.stdout.splitlines() if line.startswith('{')][0])
    assert r['n_gpus'] == 2 and r['chunked_gather'] is chunked
    assert r['on']['few']['kept'] == 1 and r['on']['few']['patches'] == 121
    assert 40 < r['on']['diagonal']['kept'] < 90
    assert r['matches_single_rank'] is True and r['matches_masked_off'] is True
