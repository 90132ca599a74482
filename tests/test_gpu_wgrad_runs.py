"""The three weight-gradient kernels where a split-K run holds SEVERAL tiles: conv3x3_wgrad.hip (fp32) and conv3x3_wgrad16.hip
with two operand planes (bf16x3) and one (bf16, mixed precision).

All three cut the pixels into 4 x 16 tiles, divide the tiles into `splits` contiguous runs (one per workgroup column), walk a
run double buffered (load tile t + 1 into registers, MFMAs of tile t from LDS buffer `cur`, store tile t + 1 into `cur ^ 1`,
barrier) and add the partial sums in a second kernel.  With tiles <= splits every run is one tile and none of that is taken;
the kernel tests of test_gpu_train*.py are all in that regime.  Here every case first ASSERTS, through
dsen2_conv3x3_wgrad_geometry, the run lengths it is meant to produce, so that a later change of tile size or split policy
fails loudly instead of emptying the test.

 1. small integers, dense: every product, every partial sum in any order and the double second pass are exact, so dW and db
    are compared with np.array_equal — no tolerance;
 2. 9-bit integers with g non-zero at <= 32 chosen pixels (corners, tile seams, ragged edges, first / last image, tiles that
    are not the first of their run): exact again, exercises the second planes and the three-product form of bf16x3, and a
    wrong halo column or tap shift shows as a wrong integer at a known (tap, ci, co);
 3. uniform(-1, 1) operands against float64 with gates of 10 x what the kernels measure (profiles/wgrad_gates.txt)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from dsen2_amd import _lib  # noqa: E402
from dsen2_amd.DSen2Net import (_ptr, _stream_ptr, bf16_plane_f32, conv3x3_wgrad_bf16, conv3x3_wgrad_bf16x3,  # noqa: E402
                                conv3x3_wgrad_geometry, split3_f32)

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda', 0)

# n, h, w; tiles = n * ceil(h / 4) * ceil(w / 16)
SHAPES = {
    'A': (9, 32, 32),       # 144 tiles, 16 per image: at 64 splits runs of 2-3 that cross image boundaries
    'B': (7, 21, 37),       # 126: ragged bottom and right tiles inside runs of 1-2
    'C': (19, 21, 37),      # 342: the 256- and 128-split layers (first, output) get runs of 1-2 and 2-3
    'D': (40, 32, 32),      # 640: 10 per run at 64 splits, 40 at 16: buffer parity over many iterations
    'E': (2, 21, 37),       # 36: F = 256 body, 16 splits: runs of 2-3
    'F': (1, 8, 600),       # 76, one image of two tile rows of 38: 76 * 32 / 64 = 38, so a run ENDS at the row's end
    'G': (1, 12, 600),      # 114, three tile rows of 38: the run [37, 39) wraps a tile row
}
# (shape, splits) -> (shortest, longest run)
RUN_LENGTHS = {('A', 64): (2, 3), ('B', 64): (1, 2), ('D', 64): (10, 10), ('F', 64): (1, 2), ('G', 64): (1, 2),
               ('E', 16): (2, 3), ('D', 16): (40, 40),
               ('C', 256): (1, 2), ('C', 128): (2, 3), ('D', 256): (2, 3), ('D', 128): (5, 5)}


def _assert_runs(kind, shape, ca, cg, splits):
    """The regime of one case, from the library's own geometry.  Returns (tiles_x, tiles per image, run bounds)."""
    n, h, w = SHAPES[shape]
    tiles, got_splits, _ = conv3x3_wgrad_geometry(kind, n, h, w, ca, cg)
    tiles_x, tiles_y = (w + 15) // 16, (h + 3) // 4
    assert tiles == n * tiles_x * tiles_y and got_splits == splits, (tiles, got_splits)
    bounds = [tiles * s // splits for s in range(splits + 1)]
    lens = np.diff(bounds)
    lo, hi = RUN_LENGTHS[(shape, splits)]
    assert tiles > splits and hi >= 2                          # some run holds more than one tile
    assert tiles // splits >= lo and (int(lens.min()), int(lens.max())) == (lo, hi), (tiles, splits, lens.min(), lens.max())
    assert (tiles % splits != 0) == (lo != hi)                 # uneven runs where they are the point
    per_img = tiles_x * tiles_y
    runs = list(zip(bounds[:-1], bounds[1:]))
    if shape == 'A':
        assert any(b // per_img != (e - 1) // per_img for b, e in runs)       # a run crosses from one image into the next
    if shape in ('B', 'C', 'E'):
        assert h % 4 != 0 and w % 16 != 0                      # ragged bottom and right tiles
    if shape == 'G':
        assert any(b // tiles_x != (e - 1) // tiles_x for b, e in runs)       # a run wraps a tile row
    return tiles_x, per_img, bounds


def _wgrad64(a, g):
    """float64 reference as nine BLAS matrix products: dW (3, 3, ci, co), db (co)."""
    n, h, w, ci = a.shape
    co = g.shape[3]
    ap = np.pad(a.astype(np.float64), ((0, 0), (1, 1), (1, 1), (0, 0)))
    g2 = g.astype(np.float64).reshape(-1, co)
    dw = np.empty((3, 3, ci, co))
    for ky in range(3):
        for kx in range(3):
            dw[ky, kx] = np.ascontiguousarray(ap[:, ky:ky + h, kx:kx + w]).reshape(-1, ci).T @ g2
    return dw, g2.sum(axis=0)


def _frozen(*arrays):
    for x in arrays:
        x.setflags(write=False)
    return arrays


def _operands(kind, a, g):
    """fp32 NHWC host arrays -> what the kernel of `kind` reads, on the device."""
    ad, gd = (torch.tensor(x, device=DEV) for x in (a, g))             # (a copy: the cached host arrays are read-only)
    if kind == 'fp32':
        return ad, gd
    if kind == 'bf16x3':
        return split3_f32(ad)[0], split3_f32(gd)[0]
    return bf16_plane_f32(ad), bf16_plane_f32(gd)


def _launch(kind, ops, dims, ci, co, scale):
    """-> (dW (3, 3, ci, co), db (co)) as host float64 arrays, and the device tensors."""
    n, h, w, ca, cg = dims
    if kind == 'fp32':
        dw = torch.empty((3, 3, ci, co), dtype=torch.float32, device=DEV)
        db = torch.empty(co, dtype=torch.float32, device=DEV)
        with torch.cuda.device(DEV):
            _lib.call('dsen2_conv3x3_wgrad', _ptr(ops[0]), _ptr(ops[1]), _ptr(dw), _ptr(db), n, h, w, ca, cg, ci, co, float(scale),
                      _stream_ptr(DEV))
    else:
        dw, db = (conv3x3_wgrad_bf16x3 if kind == 'bf16x3' else conv3x3_wgrad_bf16)(ops[0], ops[1], scale=scale)
    torch.cuda.synchronize()
    return dw.cpu().numpy().astype(np.float64), db.cpu().numpy().astype(np.float64), (dw, db)


def _assert_exact(got, ref, what):
    if not np.array_equal(got, ref):
        bad = np.argwhere(got != ref)
        lines = ['%s got %r want %r' % (tuple(int(v) for v in i), got[tuple(i)], ref[tuple(i)]) for i in bad[:12]]
        extent = ', '.join('axis %d: %d..%d' % (k, bad[:, k].min(), bad[:, k].max()) for k in range(bad.shape[1]))
        raise AssertionError('%s: %d of %d elements differ (%s); the first (index = tap row, tap column, ci, co):\n  %s'
                             % (what, len(bad), ref.size, extent, '\n  '.join(lines)))


# ---- 1. dense small integers: exact ----
@functools.lru_cache(maxsize=2)
def _dense_case(shape, ca, cg, ci, co):
    """Integers from {-3..3} (exact in bf16: the second plane of bf16x3 is zero), the padded channels zero.  Every product is an
    integer of magnitude <= 9 and every partial sum is bounded by 9 * pixels <= 3.7e5 < 2^24: fp32 accumulation in any order,
    the partial sums and the double second pass are exact.  Shared by the kernels that run the same case, never modified."""
    n, h, w = SHAPES[shape]
    rng = np.random.default_rng([n, h, w, ca, cg, ci, co])
    a = rng.integers(-3, 4, (n, h, w, ca)).astype(np.float32)
    g = rng.integers(-3, 4, (n, h, w, cg)).astype(np.float32)
    a[..., ci:] = 0
    g[..., co:] = 0
    ref_w, ref_b = _wgrad64(a[..., :ci], g[..., :co])
    assert 9 * n * h * w < 2 ** 24 and np.abs(ref_w).max() < 2 ** 24
    return _frozen(a, g, ref_w, ref_b)


def _body(kinds, feat, splits, shapes):
    return [(kind, shape, feat, feat, feat, feat, splits) for shape in shapes for kind in kinds]


# kind, shape, ca, cg, ci, co, splits — ordered so that the kernels sharing a case follow one another
DENSE = _body(('fp32', 'bf16x3', 'bf16'), 128, 64, 'ABDFG') + _body(('fp32', 'bf16x3', 'bf16'), 256, 16, 'ED') + \
    [('fp32', shape, 16, cg, ci, cg, 32768 // cg) for shape in 'CD' for cg in (128, 256) for ci in (10, 12)] + \
    [('fp32', shape, ca, 16, ca, co, 32768 // ca) for shape in 'CD' for ca in (128, 256) for co in (6, 2)]


@pytest.mark.parametrize('kind,shape,ca,cg,ci,co,splits', DENSE)
def test_small_integer_operands_give_the_exact_gradient(kind, shape, ca, cg, ci, co, splits):
    _assert_runs(kind, shape, ca, cg, splits)
    a, g, ref_w, ref_b = _dense_case(shape, ca, cg, ci, co)
    n, h, w = SHAPES[shape]
    ops = _operands(kind, a, g)
    for scale in (1.0, 0.5):                    # the reference times 0.5 is exact too
        dw, db, _ = _launch(kind, ops, (n, h, w, ca, cg), ci, co, scale)
        what = '%s %s n=%d %dx%d %d->%d scale %g' % (kind, shape, n, h, w, ci, co, scale)
        _assert_exact(dw, ref_w * scale, what + ' dW')
        _assert_exact(db, ref_b * scale, what + ' db')


# ---- 2. 9-bit integers, g non-zero at <= 32 pixels: exact, the second planes of bf16x3, a delta test for all three ----
def _planes_to_f32(planes):
    """int16 [n, 2, c/8, h, w, 8] (bf16 bit patterns) -> two fp32 NHWC arrays (plane 0, plane 1): test_gpu_bf16x3.py's decoder
    of what split3_f32 returns (split3_f32 itself is pinned bit for bit there)."""
    n, _, b, h, w, _ = planes.shape
    u = planes.cpu().numpy().view(np.uint16).astype(np.uint32) << 16
    f = u.view(np.float32)
    f = f.transpose(0, 1, 3, 4, 2, 5).reshape(n, 2, h, w, b * 8)
    return f[:, 0], f[:, 1]


def _sparse_pixels(shape, tiles_x, per_img, bounds):
    """(image, y, x) of the pixels where g is non-zero, and how many of them lie in a tile that is not the first of its run."""
    n, h, w = SHAPES[shape]
    pix = set()
    for img in (0, n - 1):                                                 # the four corners, first and last image
        pix.update((img, y, x) for y in (0, h - 1) for x in (0, w - 1))
    pix.update((n // 2, y, x) for y in (3, 4) for x in (15, 16))           # both sides of the tile seams x = 15 | 16, y = 3 | 4
    pix.update([(1, h - 1, 17), (n - 2, 5, w - 1)])                        # the last (ragged) row and column, away from the corners
    runs = [(b, e) for b, e in zip(bounds[:-1], bounds[1:]) if e - b >= 2]
    later = [runs[0][0] + 1, runs[len(runs) // 2][1] - 1, runs[-1][1] - 1]  # the second tile of a run, the last tiles of two more
    longest = max(runs, key=lambda r: r[1] - r[0])
    later += list(range(longest[0] + 1, longest[1]))                       # every later tile of one longest run
    for t in later:
        img, r = divmod(t, per_img)
        pix.add((img, min(4 * (r // tiles_x) + 1, h - 1), min(16 * (r % tiles_x) + 5, w - 1)))
    pix = sorted(pix)
    assert len(pix) <= 32
    starts = np.asarray(bounds)

    def not_first(p):
        t = p[0] * per_img + (p[1] // 4) * tiles_x + p[2] // 16
        return t != starts[np.searchsorted(starts, t, side='right') - 1]
    count = sum(not_first(p) for p in pix)
    assert count >= len(set(later)) >= 2
    return pix, count


@functools.lru_cache(maxsize=None)
def _sparse_case(shape, feat, vmax, pix):
    n, h, w = SHAPES[shape]
    rng = np.random.default_rng([n, h, w, feat, vmax])
    a = rng.integers(-vmax, vmax + 1, (n, h, w, feat)).astype(np.float32)
    g = np.zeros((n, h, w, feat), np.float32)
    for p in pix:
        g[p] = rng.integers(-vmax, vmax + 1, feat)
    return _frozen(a, g)


# the bf16 kernel takes one bf16 per operand: 8 significant bits
@pytest.mark.parametrize('kind,vmax', [('bf16x3', 511), ('bf16', 255), ('fp32', 511)])
@pytest.mark.parametrize('shape', ['B', 'A'])
def test_sparse_integer_gradient_is_exact_at_every_tap(shape, kind, vmax):
    """|values| <= 511 = 9 bits: plane 0 + plane 1 of bf16x3 hold them exactly.  A plane product is an integer of magnitude
    <= 512 * 512 < 2.7e5 and a0 g0 + a0 g1 + a1 g0 = a g - a1 g1 with |a1|, |g1| <= 1; g is non-zero at <= 32 pixels, so every
    sum of any subset of the products of one dW element is an integer bounded by 32 * (2^18 + 2 * 512) = 8.4e6 < 2^24: exact in
    fp32 in any order.  The bf16x3 reference is the sum over the THREE plane products, decoded from what split3_f32 returned;
    it does not contain a1 g1 (which would change it: asserted)."""
    feat = 128
    n, h, w = SHAPES[shape]
    tiles_x, per_img, bounds = _assert_runs(kind, shape, feat, feat, 64)
    pix, later = _sparse_pixels(shape, tiles_x, per_img, bounds)
    a, g = _sparse_case(shape, feat, vmax, tuple(pix))
    assert 32 * (2 ** 18 + 2 * 512) < 2 ** 24
    ops = _operands(kind, a, g)
    if kind == 'bf16x3':
        (a0, a1), (g0, g1) = _planes_to_f32(ops[0]), _planes_to_f32(ops[1])
        assert np.array_equal(a0.astype(np.float64) + a1, a) and np.array_equal(g0.astype(np.float64) + g1, g)
        assert np.abs(a1).max() == 1 and np.abs(g1).max() == 1 and np.abs(a0).max() <= 512            # second planes in use
        terms = [_wgrad64(x, y) for x, y in ((a0, g0), (a0, g1), (a1, g0))]
        ref_w, ref_b = sum(t[0] for t in terms), terms[0][1] + terms[1][1]
        assert not np.array_equal(ref_w, _wgrad64(a, g)[0])
    else:
        ref_w, ref_b = _wgrad64(a, g)
    assert np.abs(ref_w).max() < 2 ** 24
    dw, db, _ = _launch(kind, ops, (n, h, w, feat, feat), feat, feat, 1.0)
    what = '%s %s n=%d %dx%d, g at %d pixels (%d in a later tile of a run)' % (kind, shape, n, h, w, len(pix), later)
    _assert_exact(dw, ref_w, what + ' dW')
    _assert_exact(db, ref_b, what + ' db')


# ---- 3. uniform(-1, 1) operands against float64: calibrated gates ----
# Gates = 10 x the largest figure the kernel measures against the float64 reference over the cases below (relative L2 error =
# rms error / rms of the reference tensor); max |error| / rms of the reference <= 12 x that gate (a 5-sigma tail over <= 1e6
# elements is ~ 5 x the rms: test_gpu_conv.py).  `python -m pytest tests/test_gpu_wgrad_runs.py -m gpu -s -k float_operands`
# prints every case's figures; profiles/wgrad_gates.txt holds the run the numbers below were read from.
# measured, largest over the cases (dW, db): fp32 4.46e-7 (shape D: ten tiles per run; 1.8e-7 .. 2.2e-7 on A, B, E), 3.38e-7;
# bf16x3 3.79e-6 (the same on every shape: the 2^-17 each operand loses in the split), 2.28e-6; bf16 (operands already bf16: only
# the fp32 accumulation is left) 1.28e-7, 2.93e-8.  Largest max |error| / rms: 2.2e-6, 2.1e-5, 6.1e-7 (dW), 1.1e-6, 7.7e-6, 1.7e-7 (db).
RMS_GATE = {'fp32': {'dW': 4.46e-6, 'db': 3.38e-6}, 'bf16x3': {'dW': 3.79e-5, 'db': 2.29e-5}, 'bf16': {'dW': 1.28e-6, 'db': 2.93e-7}}
MAX_GATE_FACTOR = 12


def _to_bf16(x):
    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(torch.bfloat16).to(torch.float32).numpy()


@functools.lru_cache(maxsize=2)
def _float_case(shape, feat, rounded):
    """The operand recipe of the kernel tests of test_gpu_train*.py (the bf16 kernel's operands rounded to bf16 first) and its
    float64 reference; computed once per (shape, rounding), never modified."""
    n, h, w = SHAPES[shape]
    rng = np.random.default_rng(n * 1000 + h * 10 + w)
    a = rng.uniform(-1, 1, (n, h, w, feat)).astype(np.float32)
    g = rng.uniform(-1, 1, (n, h, w, feat)).astype(np.float32)
    if rounded:
        a, g = _to_bf16(a), _to_bf16(g)
    return _frozen(a, g, *_wgrad64(a, g))


FLOAT_CASES = [(kind, shape, 128, 64) for shape in 'ABD' for kind in ('fp32', 'bf16x3', 'bf16')] + \
    [(kind, 'E', 256, 16) for kind in ('fp32', 'bf16x3', 'bf16')]


@pytest.mark.parametrize('kind,shape,feat,splits', FLOAT_CASES)
def test_float_operands_against_float64(kind, shape, feat, splits):
    _assert_runs(kind, shape, feat, feat, splits)
    n, h, w = SHAPES[shape]
    a, g, ref_w, ref_b = _float_case(shape, feat, kind == 'bf16')
    ops = _operands(kind, a, g)
    dw, db, dev = _launch(kind, ops, (n, h, w, feat, feat), feat, feat, 1.0)
    figures = {}
    for name, got, ref in (('dW', dw, ref_w), ('db', db, ref_b)):
        rms = np.linalg.norm(ref) / np.sqrt(ref.size)
        figures[name] = (float(np.linalg.norm(got - ref) / np.linalg.norm(ref)), float(np.abs(got - ref).max() / rms))
    print('wgrad %-6s %s n=%d %dx%d F=%d: ' % (kind, shape, n, h, w, feat) +
          '  '.join('%s rel. L2 %.3e (gate %.2e) max/rms %.3e' % (k, v[0], RMS_GATE[kind][k], v[1]) for k, v in figures.items()))
    for name, (rel, mx) in figures.items():
        gate = RMS_GATE[kind][name]
        assert gate <= 1e-4                     # never looser than the kernel tests' own bound
        assert rel <= gate, (kind, shape, name, rel)
        assert mx <= MAX_GATE_FACTOR * gate, (kind, shape, name, mx)
    if shape == 'A':                            # no float atomics: the same bits on every launch, with several tiles per run too
        _, _, again = _launch(kind, ops, (n, h, w, feat, feat), feat, feat, 1.0)
        assert torch.equal(dev[0], again[0]) and torch.equal(dev[1], again[1])
