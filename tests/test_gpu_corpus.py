"""Training from tiles on the GPU: dsen2_corpus_batch against the chain of launches it replaces (gather_patches_device ->
interp_patches_device -> dihedral) and against a numpy restatement, BIT FOR BIT; against the reference's recorded training files;
inside guard bands; S2Model.fit_corpus against the same steps fed from host arrays, plain, sharded and as gloo ranks; and the
command line.  Everything is an equality: no tolerance anywhere."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dihedral_restatement as dr  # noqa: E402
import trainset_fixtures as fx  # noqa: E402
from bits import assert_same_bits  # noqa: E402
from guarded import Guarded, run_three_ways  # noqa: E402
from oracle import patches_oracle as po  # noqa: E402

from dsen2_amd import _lib, corpus, patches, train, training, weights  # noqa: E402
from dsen2_amd.DSen2Net import dihedral, s2model  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
SCALE = 2000


def _rasters(grid, factors, bands, dtype, seed):
    """The rasters (d10, d20(, d60)) of one tile, `factors` times the origin grid `grid` each, of `dtype`."""
    rng = np.random.default_rng(seed)
    out = []
    for f, c in zip(factors, bands):
        a = rng.integers(200, 12000, (grid[0] * f, grid[1] * f, c)).astype(dtype)
        if dtype == np.float32:
            a += rng.random(a.shape, dtype=np.float32)
        out.append(a)
    return tuple(out)


def _corners(grid):
    return [(0, 0), (0, grid[1] - 16), (grid[0] - 16, 0), (grid[0] - 16, grid[1] - 16)]


@pytest.fixture(scope='module')
def corpus20():
    """Origin grids 24 x 40 (uint16 rasters, uint16 target) and 33 x 17 (float32): lr10 and d20 are twice that."""
    grids = [(24, 40), (33, 17)]
    tiles = [_rasters(grids[0], (4, 2), (4, 6), np.uint16, 1), _rasters(grids[1], (4, 2), (4, 6), np.float32, 2)]
    c = corpus.TileCorpus(tiles, device=DEV)
    assert c.extents == grids and c.gt[0].dtype == torch.int16 and c.gt[1].dtype == torch.float32
    assert c.nbytes == sum(g[0] * g[1] * (4 * 4 * 4 + 6 * 4) for g in grids) + 24 * 40 * 4 * 6 * 2 + 33 * 17 * 4 * 6 * 4
    # 19 samples: the four corner origins of each tile (the last valid origin, extent - 16, included), all 8 ops on both tiles
    table = [(t, oy, ox, (2 * i + t) % 8) for t, g in enumerate(grids) for i, (oy, ox) in enumerate(_corners(g))]
    table += [(0, 3, 11, 1), (1, 9, 0, 0), (0, 7, 24, 3), (1, 16, 1, 5), (0, 1, 1, 7), (1, 2, 0, 2), (0, 5, 13, 4), (1, 11, 1, 6),
              (0, 8, 23, 0), (1, 4, 0, 3), (0, 2, 9, 5)]
    table = np.asarray(table, np.int32)
    assert table.shape == (19, 4)
    assert set(table[:, 3]) == set(range(8)) and set(table[:, 0]) == {0, 1}
    return c, table


@pytest.fixture(scope='module')
def corpus60():
    """Origin grids 18 x 20 and 16 x 31 (the second: ONE row origin), P = 96."""
    grids = [(18, 20), (16, 31)]
    tiles = [_rasters(grids[0], (36, 18, 6), (4, 6, 2), np.uint16, 3), _rasters(grids[1], (36, 18, 6), (4, 6, 2), np.float32, 4)]
    c = corpus.TileCorpus(tiles, run_60=True, device=DEV)
    assert c.extents == grids and c.patch == 96
    table = np.asarray([(0, 2, 4, 1), (1, 0, 15, 6), (0, 0, 0, 0), (1, 0, 0, 3), (0, 1, 3, 4)], np.int32)
    return c, table


def _gt_f32(c, t):
    return patches._widen(c.gt[t], np.uint16) if c.gt_dtypes[t] == np.uint16 else c.gt[t]


def chain(c, table, divisor):
    """The launches corpus.batch replaces, sample by sample: gather (border 0) -> up-sampler -> dihedral."""
    P, s = c.patch, c.scale
    cols = [[] for _ in range(4 if c.run_60 else 3)]
    for t, oy, ox, _ in table.tolist():
        org = np.asarray([[oy, ox]], np.int32)
        lr = c.lr[t]
        cols[0].append(patches.gather_patches_device(lr[0], org, s, 0, P, 1, divisor=divisor))
        if c.run_60:
            cols[1].append(patches.interp_patches_device(patches.gather_patches_device(lr[1], org, 3, 0, 48, 1), (P, P), post_divisor=divisor))
            cols[2].append(patches.interp_patches_device(patches.gather_patches_device(lr[2], org, 1, 0, 16, 1), (P, P), post_divisor=divisor))
        else:
            cols[1].append(patches.interp_patches_device(patches.gather_patches_device(lr[1], org, 1, 0, 16, 1), (P, P), post_divisor=divisor))
        cols[-1].append(patches.gather_patches_device(_gt_f32(c, t), org, s, 0, P, 1, divisor=divisor))
    ops = torch.from_numpy(np.ascontiguousarray(table[:, 3])).to(c.device)
    out = [dihedral(torch.cat(col).contiguous(), ops=ops) for col in cols]
    return out[:-1], out[-1]


def restate(c, table, divisor):
    """The same in numpy: slices of the downloaded images, the CPU up-sampler the interp tests compare against
    (patches_oracle.interp_patches, f32_coords), an IEEE float32 divide, np.rot90."""
    P, s = c.patch, c.scale
    div = (lambda a: a) if divisor == 1 else (lambda a: (a / np.float32(divisor)).astype(np.float32))
    lr = [[a.cpu().numpy() for a in tile] for tile in c.lr]
    gt = [_gt_f32(c, t).cpu().numpy() for t in range(len(c))]

    def crop(a, y0, x0, edge):
        return np.ascontiguousarray(a[y0:y0 + edge, x0:x0 + edge].transpose(2, 0, 1))

    def up(a):
        return po.interp_patches(a[None], (1, a.shape[0], P, P), f32_coords=True)[0].astype(np.float32)
    cols = [[] for _ in range(4 if c.run_60 else 3)]
    for t, oy, ox, op in table.tolist():
        parts = [div(crop(lr[t][0], s * oy, s * ox, P))]
        if c.run_60:
            parts += [div(up(crop(lr[t][1], 3 * oy, 3 * ox, 48))), div(up(crop(lr[t][2], oy, ox, 16)))]
        else:
            parts += [div(up(crop(lr[t][1], oy, ox, 16)))]
        parts += [div(crop(gt[t], s * oy, s * ox, P))]
        for col, a in zip(cols, parts):
            col.append(dr.forward(a, op))
    out = [np.stack(col) for col in cols]
    return out[:-1], out[-1]


def _names(c):
    return (['data10', 'data20', 'data60'] if c.run_60 else ['data10', 'data20']) + ['target']


def _check_kernel(c, table, divisor):
    xs, y = c.batch(table, divisor=divisor)
    cx, cy = chain(c, table, divisor)
    rx, ry = restate(c, table, divisor)
    for name, got, a, b in zip(_names(c), xs + [y], cx + [cy], rx + [ry]):
        got = got.cpu().numpy()
        assert got.shape == (table.shape[0], got.shape[1], c.patch, c.patch)
        assert_same_bits(got, a.cpu().numpy(), '%s, divisor %g: kernel against the chain of launches' % (name, divisor))
        assert_same_bits(got, b, '%s, divisor %g: kernel against the numpy restatement' % (name, divisor))
    return xs, y


# ---- 1, 2. the kernel against the existing chain ---------------------------------------------------------------------------------
@pytest.mark.parametrize('divisor', [SCALE, 1])
def test_kernel_equals_the_chain_20m(corpus20, divisor):
    c, table = corpus20
    xs, y = _check_kernel(c, table, divisor)
    assert [tuple(t.shape) for t in xs + [y]] == [(19, 4, 32, 32), (19, 6, 32, 32), (19, 6, 32, 32)]
    # op 0 is the plain crop: the ops above did something
    plain = table.copy()
    plain[:, 3] = 0
    px, _ = c.batch(plain, divisor=divisor)
    assert not torch.equal(px[0], xs[0])
    # the Python wrapper refuses what the library refuses, before anything is launched
    bad = table.copy()
    bad[3, 1] = c.extents[bad[3, 0]][0] - 15
    with pytest.raises(_lib.DSen2Error, match='sample 3: origin'):
        c.batch(bad)


@pytest.mark.parametrize('divisor', [SCALE, 1])
def test_kernel_equals_the_chain_60m(corpus60, divisor):
    c, table = corpus60
    xs, y = _check_kernel(c, table, divisor)
    assert [tuple(t.shape) for t in xs + [y]] == [(5, 4, 96, 96), (5, 6, 96, 96), (5, 2, 96, 96), (5, 2, 96, 96)]


# ---- 3. against the reference's own files ------------------------------------------------------------------------------------------
def _same_bytes(got, want, what):
    got = got.cpu().numpy()
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    assert got.tobytes() == want.tobytes(), '%s: %d of %d values differ' % (what, int((got != want).sum()), got.size)


def test_kernel_reproduces_the_references_recorded_files():
    """The inputs of tests/golden/make_golden_trainset.py, its recorded origins, op 0, divisor 1: the reference's .npy contents."""
    d10, d20, _ = fx.load_tile('T33UUB')
    c = corpus.TileCorpus([(d10, d20)], device=DEV)
    org = fx.load_split('trainset_random20', 'origins')
    table = np.zeros((org.shape[0], 4), np.int32)
    table[:, 1:3] = org
    xs, y = c.batch(table, divisor=1)
    for key, got in (('data10', xs[0]), ('data20', xs[1]), ('data20_gt', y)):
        _same_bytes(got, fx.load_split('trainset_random20', key), 'trainset_random20 ' + key)
    c = corpus.TileCorpus([fx.mosaic_60(*fx.load_tile('T33UUB'))], run_60=True, device=DEV)
    org = fx.load_split('trainset_random60', 'origins')
    table = np.zeros((org.shape[0], 4), np.int32)
    table[:, 1:3] = org
    xs, y = c.batch(table, divisor=1)
    for key, got in (('data10', xs[0]), ('data20', xs[1]), ('data60', xs[2]), ('data60_gt', y)):
        _same_bytes(got, fx.load_split('trainset_random60', key), 'trainset_random60 ' + key)


# ---- 4. memory contract --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('which,n', [('20', 19), ('20', 1), ('60', 5), ('60', 1)])
def test_kernel_memory_contract(corpus20, corpus60, which, n):
    """Outputs inside guard bands and poisoned (tests/guarded.py): every element written, no guard byte changed, the sample table
    unchanged, and the same bits as the plain run — which are the chain's."""
    c, table = corpus20 if which == '20' else corpus60
    table = np.ascontiguousarray(table[-n:])
    x_shapes, y_shape = c.output_shapes(n)

    def call(inp, out, _inplace, _scratch):
        c.batch(table, table_dev=inp[0], out=(out[:-1], out[-1]))
    out, _ = run_three_ways(call, [torch.from_numpy(table).to(DEV)], [(s, torch.float32) for s in x_shapes + [y_shape]], device=DEV,
                            what='corpus batch %s m, n = %d' % (which, n))
    cx, cy = chain(c, table, SCALE)
    for name, got, want in zip(_names(c), out, cx + [cy]):
        assert_same_bits(got.cpu().numpy(), want.cpu().numpy(), name)


def test_an_empty_batch_writes_nothing(corpus20):
    c, table = corpus20
    x_shapes, y_shape = c.output_shapes(1)
    bufs = [Guarded(s, torch.float32, DEV, 0xFF) for s in x_shapes + [y_shape]]
    with torch.cuda.device(DEV):
        _lib.call('dsen2_corpus_batch', c._handle, None, None, 0, float(SCALE), patches._ptr(bufs[0].t), patches._ptr(bufs[1].t), None,
                  patches._ptr(bufs[2].t), patches._stream(DEV))
    torch.cuda.synchronize()
    for g in bufs:
        g.check('n = 0')
        assert bool((g.raw == 0xFF).all()), 'n = 0 wrote into an output'
    xs, y = c.batch(np.zeros((0, 4), np.int32))
    assert [tuple(t.shape) for t in xs + [y]] == [(0, 4, 32, 32), (0, 6, 32, 32), (0, 6, 32, 32)]


# ---- 5. fit_corpus against the host path ---------------------------------------------------------------------------------------
BANDS, D, F = (4, 6), 1, 128
BATCH, STEPS, EPOCHS, SEED = 6, 3, 2, 17


def _model(precision='fp32', mixed_precision=None):
    m = s2model(tuple((c, None, None) for c in BANDS), num_layers=D, feature_size=F, device=DEV, precision=precision)
    m.set_weights_flat(weights.random_he_uniform(sum(BANDS), BANDS[-1], D, F, seed=5, bias_scale=0.05))
    m.compile(training.Nadam(lr=1e-3), mixed_precision=mixed_precision)
    return m


def _host_run(c, model, val, shards=None):
    """The steps of fit_corpus on the parent's path: each step's batch cut by the existing chain (no op), downloaded, and fed to
    train_on_batch(augment_ops=) as host arrays; fit's epoch loss and validation."""
    sampler = corpus.CorpusSampler(c, SEED, augment=True)
    losses, val_losses = [], []
    for _ in range(EPOCHS):
        sums = np.zeros(2)
        for _ in range(STEPS):
            table = sampler.draw(BATCH)
            plain = table.copy()
            plain[:, 3] = 0
            xs, y = chain(c, plain, SCALE)
            r = model.train_on_batch([a.cpu().numpy() for a in xs], y.cpu().numpy(), shards=shards, augment_ops=table[:, 3])
            sums += np.asarray(r) * BATCH
        losses.append(sums / (STEPS * BATCH))
        val_losses.append(model.evaluate(val[0], val[1], batch_size=BATCH))
    return losses, val_losses


def _compare_history(h, losses, val_losses):
    assert h.epoch == list(range(EPOCHS))
    for e in range(EPOCHS):
        assert h.history['loss'][e] == losses[e][0] and h.history['mean_squared_error'][e] == losses[e][1], (e, h.history, losses)
        assert h.history['val_loss'][e] == val_losses[e][0] and h.history['val_mean_squared_error'][e] == val_losses[e][1]
    assert h.history['loss'][0] != h.history['loss'][1] and np.isfinite(h.history['loss']).all()


@pytest.fixture(scope='module')
def validation(corpus20):
    c, _ = corpus20
    xs, y = c.validation_arrays(2, SEED)
    assert [a.shape for a in xs + [y]] == [(4, 4, 32, 32), (4, 6, 32, 32), (4, 6, 32, 32)] and all(a.dtype == np.float32 for a in xs)
    again = c.validation_arrays(2, SEED)
    assert all(np.array_equal(a, b) for a, b in zip(xs + [y], again[0] + [again[1]]))
    return xs, y


@pytest.mark.parametrize('precision,mixed', [('fp32', None), ('fp32', 'bf16'), ('bf16x3', None)])
def test_fit_corpus_equals_the_host_path(corpus20, validation, precision, mixed):
    c, _ = corpus20
    a, b = _model(precision, mixed), _model(precision, mixed)
    start = a.get_weights_flat()
    h = a.fit_corpus(c, BATCH, STEPS, epochs=EPOCHS, validation_data=validation, seed=SEED, augment=True, verbose=0)
    losses, val_losses = _host_run(c, b, validation)
    wa, wb = a.get_weights_flat(), b.get_weights_flat()
    assert not np.array_equal(wa, start)
    assert wa.tobytes() == wb.tobytes(), '%d of %d weights differ' % (int((wa != wb).sum()), wa.size)
    _compare_history(h, losses, val_losses)
    assert a.optimizer.iterations == b.optimizer.iterations == STEPS * EPOCHS


def test_train_on_device_batch_keeps_the_losses_on_the_device(corpus20):
    c, table = corpus20
    a, b = _model(), _model()
    xs, y = c.batch(table[:BATCH])
    out = torch.full((3, 2), -1.0, device=DEV)
    got = a.train_on_device_batch(xs, y, loss_out=out[1])
    assert got.data_ptr() == out[1].data_ptr() and got.is_cuda
    want = b.train_on_batch([t.cpu().numpy() for t in xs], y.cpu().numpy())
    assert out.cpu().numpy().astype(np.float64)[1].tolist() == want and out[0].tolist() == [-1.0, -1.0] == out[2].tolist()
    assert a.get_weights_flat().tobytes() == b.get_weights_flat().tobytes()
    assert a.train_on_device_batch(xs, y).data_ptr() == a._train['loss2'].data_ptr()      # without loss_out: the state's own pair
    with pytest.raises(ValueError):
        a.train_on_device_batch(xs, y, loss_out=torch.zeros(3, device=DEV))


# ---- 6. sharded steps ------------------------------------------------------------------------------------------------------------
def test_fit_corpus_shards_equal_the_restated_sharded_steps(corpus20, validation):
    c, _ = corpus20
    a, b = _model(), _model()
    h = a.fit_corpus(c, BATCH, STEPS, epochs=EPOCHS, validation_data=validation, seed=SEED, augment=True, verbose=0, shards=2)
    losses, val_losses = _host_run(c, b, validation, shards=2)
    assert a.get_weights_flat().tobytes() == b.get_weights_flat().tobytes()
    _compare_history(h, losses, val_losses)
    plain = _model()
    plain.fit_corpus(c, BATCH, STEPS, epochs=EPOCHS, seed=SEED, augment=True, verbose=0)
    assert plain.get_weights_flat().tobytes() != a.get_weights_flat().tobytes()          # the summation order differs: another run
    with pytest.raises(ValueError):
        a.fit_corpus(c, BATCH, STEPS, shards=2, data_parallel=True, emulate_world=2)


TILE_FILES = [os.path.join(fx.GOLDEN, 'tile_%s_600.npz' % t) for t in fx.TILES]


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return str(p)


def _tiles_args(path, out, extra=()):
    return ['--tiles'] + TILE_FILES + ['--path', str(path), '--out', str(out), '--epochs', '2', '--steps_per_epoch', '3', '--val_crops', '2',
                                       '--batch_size', '5', '--seed', '3', '--lr', '1e-3', '--augment'] + list(extra)


def _files(out):
    ckpt, log = out / 's2_038_lr_1e-03.npy', out / 's2_038__lr_1.0e-03.txt'
    assert ckpt.exists() and log.exists(), sorted(os.listdir(str(out)))
    return ckpt.read_bytes(), log.read_bytes()


def test_two_gloo_ranks_equal_the_one_process_restatement(tmp_path):
    """fit_corpus(data_parallel=True, emulate_world=2) against 2 gloo ranks sharing the GPU, each with its own copy of the corpus:
    the checkpoint and the log, byte for byte (batch 5: shards of 3 and 2)."""
    out_n, out_1 = tmp_path / 'ranks', tmp_path / 'one'
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    r = subprocess.run([sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2', '--master-addr',
                        '127.0.0.1', '--master-port', _free_port(), '-m', 'dsen2_amd.train'] +
                       _tiles_args(tmp_path, out_n, ['--data_parallel', '--backend', 'gloo']),
                       cwd=ROOT, capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert r.stdout.count('Training starts...') == 1                   # one rank talked
    assert train.main(_tiles_args(tmp_path, out_1, ['--data_parallel', '--emulate_world', '2'])) == 0
    (ckpt_n, log_n), (ckpt_1, log_1) = _files(out_n), _files(out_1)
    assert len(log_n.splitlines()) == 2
    assert log_n == log_1, (log_n, log_1)
    assert ckpt_n == ckpt_1, 'the checkpoint of 2 ranks differs from the one-process restatement'


# ---- 7. command line ---------------------------------------------------------------------------------------------------------------
def test_train_tiles_command_line(tmp_path, capsys):
    out_a, out_b = tmp_path / 'a', tmp_path / 'b'
    assert train.main(_tiles_args(tmp_path, out_a)) == 0
    said = capsys.readouterr().out
    assert 'Holding 2 tiles' in said and '3 steps of 5 crops per epoch, 4 crops for validation' in said
    ckpt, log = _files(out_a)
    lines = log.decode().splitlines()
    assert len(lines) == 2 and all(l.startswith('Finished epoch') and 'valid:' in l for l in lines)
    flat = np.load(str(out_a / 's2_038_lr_1e-03.npy'))
    assert flat.dtype == np.float32 and np.isfinite(flat).all()
    assert train.main(_tiles_args(tmp_path, out_b)) == 0               # the same --seed: the same bytes
    assert _files(out_b) == (ckpt, log)
    capsys.readouterr()
    # --tiles against a populated training set under --path
    os.makedirs(str(tmp_path / 'train' / 'S2A_X.SAFE'))
    assert train.main(_tiles_args(tmp_path, tmp_path / 'c')) == 2
    assert '--tiles and a training set under --path exclude each other' in capsys.readouterr().err
    assert not (tmp_path / 'c').exists()
