"""Adam, SGD, gradient clipping and decoupled weight decay on the GPU: dsen2_optimizer_step against its float64 numpy restatement
(tests/optimizer_restatement.py) bit for bit — the mean gradient, p, m, v and the global norm —, against the entries it generalises,
inside guard bands; train_on_batch (plain, sharded, mixed precision, bf16x3) and fit_corpus against gradients_device followed by
the restatement; two gloo ranks against their one-process restatement byte for byte; and learning.  No tolerance anywhere but in
the learning test."""
import ctypes
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import optimizer_restatement as orst  # noqa: E402
from dsen2_amd import _lib, corpus, training, weights  # noqa: E402
from dsen2_amd.DSen2Net import _ptr, _stream_ptr, s2model  # noqa: E402
from guarded import run_three_ways  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)

# ---- 1. the kernels -----------------------------------------------------------------------------------------------------------
LARGE = (1000003, 1000003 + 5, (3, 0, 2))          # a scalar tail of 3 behind 250000 16-byte units; one empty shard
MATRIX = (4099, 4100, (1,) * 64)                   # the largest number of shards
SMALL = [(3, 8, (2, 5)),                           # fewer than four values
         (1024, 1024, (0, 1)),                     # no tail; the first shard empty
         (5003, 5005, (1, 4, 0, 2))]               # an odd stride: rows off the 16-byte grid (ODD_STRIDE below)
ODD_STRIDE = SMALL[2]                              # in ONE pass the step kernel itself takes its scalar form here: 20 workgroups
KINDS = ('nadam', 'adam', 'sgd', 'nesterov')
CLIPS = ('none', 'clipnorm', 'clipvalue', 'both')
LR, WD = 1e-3, 0.05


def _kind_desc(kind, step=3):
    """The descriptor's scalars of step `step` of each update rule, from the optimisers of training.py."""
    if kind == 'nadam':
        opt = training.Nadam(lr=LR)
    elif kind == 'adam':
        opt = training.Adam(lr=LR)
    else:
        opt = training.SGD(lr=LR, momentum=0.9, nesterov=kind == 'nesterov')
    for _ in range(step):
        s = opt.next_step()
    return dict(s, kind=opt.KIND)


def _inputs(count, stride, counts, large=False):
    """Gradient rows whose padding and empty shards hold all-ones NaN patterns; p, m, v as tests/test_gpu_train_parallel.py."""
    rng = np.random.default_rng([count, stride])
    g = np.zeros((len(counts), stride), np.float32)
    g.view(np.uint8)[...] = 0xFF
    for r, c in enumerate(counts):
        if c > 0:
            g[r, :count] = rng.standard_normal(count).astype(np.float32) * np.float32(10.0 ** -r if large else 1.0)
    p, m = (rng.uniform(-1, 1, count).astype(np.float32) for _ in range(2))
    v = rng.uniform(0, 1, count).astype(np.float32)
    return g, p, m, v


def _ranges(count):
    """Decay ranges: one of length 1, one from 0, one up to count, one across a 16-byte unit and across the 256-thread block
    boundaries of both kernel forms (element 256 of the scalar form, element 1024 of the wide one)."""
    if count < 2000:
        return [(0, 1)] if count < 8 else [(0, 1), (5, 6), (250, 262), (count - 3, count)]
    return [(0, 3), (5, 6), (250, 262), (1000, 1100), (count // 2, count // 2 + count // 4), (count - 9, count)]


def _check_ranges(count, ranges):
    assert any(hi - lo == 1 for lo, hi in ranges) and ranges[0][0] == 0 and ranges[-1][1] == count
    assert any(lo % 4 and lo // 4 != (hi - 1) // 4 for lo, hi in ranges)                                   # across a 16-byte unit
    assert any(lo < 256 <= hi - 1 for lo, hi in ranges) and any(lo < 1024 <= hi - 1 for lo, hi in ranges)    # across a block of either form
    assert sum(hi - lo for lo, hi in ranges) <= 0.7 * count


def _options(clip, decay, rows, counts):
    """clipnorm = a quarter of the norm (so s = 0.25), clipvalue = the median magnitude of what reaches it: both from the inputs."""
    mean = orst.mean_gradient(rows, counts)
    o = {}
    if clip in ('clipnorm', 'both'):
        o['clipnorm'] = float(np.float32(orst.global_norm(mean) / 4))
        mean = (mean.astype(np.float64) * orst.clip_scale(orst.global_norm(mean), o['clipnorm'])).astype(np.float32)
    if clip in ('clipvalue', 'both'):
        o['clipvalue'] = float(np.float32(np.median(np.abs(mean))))
    if decay:
        o['weight_decay'] = WD
    return o


def _case(shape, kind, clip, decay, large=False, step=3):
    count, stride, counts = shape
    g, p, m, v = _inputs(count, stride, counts, large)
    rows = [g[r, :count] for r in range(len(counts))]
    desc = dict(_kind_desc(kind, step), **_options(clip, decay, rows, counts))
    ranges = _ranges(count) if decay else []
    want = orst.restate(desc, p, rows, counts, m, v, ranges)
    # the conditions the case is there for, on the restatement alone
    if 'clipnorm' in desc:
        assert want['norm'] >= desc['clipnorm'] and want['scale'] < 0.5
    if 'clipvalue' in desc and count >= 1000:
        clamped = np.mean(np.abs(want['g']) == np.float32(desc['clipvalue']))
        assert 0.05 <= clamped <= 0.95, clamped
    if decay and count >= 2000:
        _check_ranges(count, ranges)
    return dict(g=g, p=p, m=m, v=v, desc=desc, ranges=ranges, want=want, count=count, stride=stride, counts=counts)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _c_desc(desc, ranges):
    d = _lib.OptimizerDesc()
    d.kind = desc['kind']
    for k in ('lr', 'b1', 'b2', 'eps', 'mc_t', 'mc_t1', 'ms_new', 'ms_next', 'b2_pow_t', 'lr_t', 'momentum', 'clipnorm', 'clipvalue',
              'weight_decay'):
        setattr(d, k, desc.get(k, 0.0))
    d.nesterov = int(bool(desc.get('nesterov')))
    flat = [int(x) for r in ranges for x in r]
    d.n_ranges = len(ranges)
    d._keep = (ctypes.c_uint * max(1, len(flat)))(*flat)
    d.host_ranges = ctypes.cast(d._keep, ctypes.POINTER(ctypes.c_uint)) if ranges else None
    return d


def _work_bytes(d, count, shards, have_mean, want_norm):
    need = ctypes.c_size_t(0)
    _lib.call('dsen2_optimizer_step_work_bytes', ctypes.byref(d), count, shards, int(have_mean), int(want_norm), ctypes.byref(need))
    return need.value


def _call(desc, ranges, p, g, stride, counts, g_mean, m, v, count, norm=None, work=None):
    d = _c_desc(desc, ranges)
    if work is None:
        need = _work_bytes(d, count, len(counts), g_mean is not None, norm is not None)
        work = torch.empty(need, dtype=torch.uint8, device=DEV) if need else None
    with torch.cuda.device(DEV):
        _lib.call('dsen2_optimizer_step', ctypes.byref(d), _ptr(p), _ptr(g), stride, len(counts), (_lib.c_int * len(counts))(*counts),
                  _ptr(g_mean), _ptr(m), _ptr(v), count, _ptr(work), work.numel() if work is not None else 0, _ptr(norm), _stream_ptr(DEV))


def _bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint64).ravel()


def _same_bits(got, want, what):
    g, w = _bits(got), _bits(want)
    bad = np.flatnonzero(g != w)
    assert bad.size == 0, '%s: %d of %d elements differ, first at %d: got %#x want %#x' % (what, bad.size, g.size, bad[0], g[bad[0]], w[bad[0]])


def _run(k, with_mean=True, with_norm=True):
    """One call on fresh copies of the case's tensors: (g_mean, norm, p, m, v) as device tensors (v None for SGD)."""
    sgd = k['desc']['kind'] == orst.SGD
    p, m, v = _dev(k['p']), _dev(k['m']), None if sgd else _dev(k['v'])
    g_mean = torch.zeros(k['count'], device=DEV) if with_mean else None
    norm = torch.full((1,), -1.0, dtype=torch.float64, device=DEV) if with_norm else None
    _call(k['desc'], k['ranges'], p, k['g_dev'], k['stride'], k['counts'], g_mean, m, v, k['count'], norm)
    torch.cuda.synchronize()
    return g_mean, norm, p, m, v


def _against_restatement(k):
    k['g_dev'] = _dev(k['g'])
    want, sgd = k['want'], k['desc']['kind'] == orst.SGD
    runs = [_run(k), _run(k)]
    names = ('g_mean', 'norm', 'p', 'm') + (() if sgd else ('v',))
    for name, got in zip(names, runs[0]):
        _same_bits(got, want[name], '%r %s' % (k['desc'], name))
    for name, a, b in zip(names, runs[0], runs[1]):
        _same_bits(a, b, 'repeat call, ' + name)
    _same_bits(k['g_dev'].view(torch.int32), k['g'], 'dev_g_shards after the calls')
    # without the optional outputs: the same p, m, v (one pass where nothing needs the norm; the mean in the scratch where it does)
    lean = _run(k, with_mean=False, with_norm=False)
    for name, a, b in zip(names[2:], lean[2:], runs[0][2:]):
        _same_bits(a, b, 'g_mean and norm NULL, ' + name)


@pytest.mark.parametrize('decay', [False, True], ids=['plain', 'decay'])
@pytest.mark.parametrize('clip', CLIPS)
@pytest.mark.parametrize('kind', KINDS)
def test_every_kind_and_option_equals_the_restatement_bit_for_bit(kind, clip, decay):
    _against_restatement(_case(MATRIX, kind, clip, decay))


@pytest.mark.parametrize('shape', SMALL, ids=['3', '1024', '5003-odd-stride'])
@pytest.mark.parametrize('kind', KINDS)
def test_kernel_paths_agree_with_the_restatement(kind, shape):
    """With clipnorm the call takes two passes: the norm pass reads the rows (at the odd stride too), the step kernel reads their
    MEAN from an aligned buffer, so it runs in its 16-byte form here.  Its scalar form: the two tests below."""
    _against_restatement(_case(shape, kind, 'both', True, step=1))


@pytest.mark.parametrize('decay', [False, True], ids=['plain', 'decay'])
@pytest.mark.parametrize('clip', ['none', 'clipvalue'])
@pytest.mark.parametrize('kind', KINDS)
def test_the_scalar_step_kernel_in_one_pass(kind, clip, decay):
    """5003 parameters in rows 5005 floats apart, no clipnorm and no norm asked for: ONE pass, in which the step kernel reads the
    rows itself and, their starts being off the 16-byte grid, takes its scalar form — one parameter per thread, 20 workgroups, the
    decay ranges crossing workgroup boundaries (a range across element 256, one of length 1, one from 0, one up to count)."""
    k = _case(ODD_STRIDE, kind, clip, decay)
    assert k['stride'] % 4 != 0 and len(k['counts']) > 1 and k['count'] > 4 * 256 and 'clipnorm' not in k['desc']
    k['g_dev'] = _dev(k['g'])
    sgd = k['desc']['kind'] == orst.SGD
    names = ('g_mean', 'p', 'm') + (() if sgd else ('v',))
    runs = []
    for with_mean in (True, False):
        gm, _, p, m, v = _run(k, with_mean=with_mean, with_norm=False)
        runs.append(dict(g_mean=gm, p=p, m=m, v=v))
    for name in names:
        _same_bits(runs[0][name], k['want'][name], '%r %s' % (k['desc'], name))
    for name in names[1:]:
        _same_bits(runs[1][name], runs[0][name], 'g_mean NULL, ' + name)
    _same_bits(k['g_dev'].view(torch.int32), k['g'], 'dev_g_shards after the calls')


@pytest.mark.parametrize('passes', ['one-pass', 'two-pass'])
@pytest.mark.parametrize('shifted', ['p', 'm', 'v', 'g', 'g_mean', 'pmv', 'all'])
@pytest.mark.parametrize('kind', ['nadam', 'adam', 'nesterov'])
def test_a_base_that_is_not_16_byte_aligned_gives_the_same_bits(kind, shifted, passes):
    """Every vector may start 4 bytes off a 16-byte boundary (the stride itself is a multiple of 4 floats): the step kernel takes
    its scalar form — with clipnorm (two passes) as well, where it reads the mean from g_mean and p, m, v where they are —, gives the
    restatement's bits, and writes not one byte in front of or behind a vector."""
    count, stride, counts = 5003, 5004, (1, 4, 0, 2)
    k = _case((count, stride, counts), kind, 'both' if passes == 'two-pass' else 'clipvalue', True)
    sgd = k['desc']['kind'] == orst.SGD
    if sgd and shifted == 'v':
        shifted = 'pmv'                      # SGD has no v: shift the vectors it has
    FILL = 0x5A

    def place(a, off):
        """`a` at float offset `off` of a buffer of 0x5A bytes with 4 floats of margin on both sides."""
        buf = torch.full(((a.size + 8) * 4,), FILL, dtype=torch.uint8, device=DEV)
        t = buf.view(torch.float32)[4 + off:4 + off + a.size]
        t.copy_(torch.from_numpy(np.ascontiguousarray(a).ravel()))
        assert (t.data_ptr() % 16 != 0) == bool(off)
        return buf, t
    names = ('p', 'g', 'm', 'v', 'g_mean')
    which = {'pmv': ('p', 'm', 'v'), 'all': names}.get(shifted, (shifted,))
    off = {n: int(n in which) for n in names}
    # (with only g shifted, the two-pass step reads the aligned mean and stays wide: there the norm pass alone sees the shift)
    (bp, tp), (bg, tg), (bm, tm) = place(k['p'], off['p']), place(k['g'], off['g']), place(k['m'], off['m'])
    bv, tv = (None, None) if sgd else place(k['v'], off['v'])
    bo, to = place(np.zeros(count, np.float32), off['g_mean'])
    assert any(off.values())
    g_bytes = bg.clone()
    norm = torch.full((1,), -1.0, dtype=torch.float64, device=DEV) if passes == 'two-pass' else None
    _call(k['desc'], k['ranges'], tp, tg, stride, counts, to, tm, tv, count, norm)
    torch.cuda.synchronize()
    got = dict(g_mean=to, p=tp, m=tm, v=tv, norm=norm)
    for name in ('g_mean', 'p', 'm') + (() if sgd else ('v',)) + (('norm',) if norm is not None else ()):
        _same_bits(got[name], k['want'][name], '%s shifted, %s' % (shifted, name))
    assert torch.equal(bg, g_bytes), 'dev_g_shards was modified'
    for name, buf, t in (('p', bp, tp), ('m', bm, tm), ('v', bv, tv), ('g_mean', bo, to)):
        if buf is not None:
            lo = t.data_ptr() - buf.data_ptr()
            assert bool((buf[:lo] == FILL).all()) and bool((buf[lo + 4 * count:] == FILL).all()), 'written outside %s' % name


@pytest.mark.parametrize('kind,clip,decay', [('nadam', c, d) for c in CLIPS for d in (False, True)] + [('adam', 'both', True)])
def test_a_large_count_equals_the_restatement_bit_for_bit(kind, clip, decay):
    """1,000,003 parameters: from the header's grid rule a thread of the sum of squares adds more than one element and the finish
    sees more than 256 partials."""
    blocks, per_thread = orst.sqsum_grid(LARGE[0])
    assert blocks > 256 and per_thread > 1, (blocks, per_thread)
    _against_restatement(_case(LARGE, kind, clip, decay, large=True))


def test_a_norm_below_clipnorm_is_the_unclipped_step():
    k = _case(MATRIX, 'adam', 'none', True)
    k['g_dev'] = _dev(k['g'])
    plain = _run(k)
    norm = k['want']['norm']
    c = dict(k, desc=dict(k['desc'], clipnorm=float(np.float32(norm * 1.5))))
    c['want'] = orst.restate(c['desc'], c['p'], [c['g'][r, :c['count']] for r in range(len(c['counts']))], c['counts'], c['m'], c['v'], c['ranges'])
    assert c['want']['norm'] < c['desc']['clipnorm'] and c['want']['scale'] == 1.0
    clipped = _run(c)
    for name, a, b, w in zip(('g_mean', 'norm', 'p', 'm', 'v'), clipped, plain, (c['want'][n] for n in ('g_mean', 'norm', 'p', 'm', 'v'))):
        _same_bits(a, b, 'clipnorm above the norm against no clipnorm, ' + name)
        _same_bits(a, w, 'clipnorm above the norm, ' + name)


@pytest.mark.parametrize('sign', [1.0, -1.0])
def test_a_norm_equal_to_clipnorm_scales_by_one(sign):
    """g is a single element +-c: the sum of squares is c * c exactly, its root c, and c / c = 1."""
    count, c = 1024, float(np.float32(0.3))
    g = np.zeros((1, count), np.float32)
    g[0, 517] = np.float32(sign * c)
    rng = np.random.default_rng(5)
    p, m, v = (rng.uniform(0.1, 1, count).astype(np.float32) for _ in range(3))
    desc = dict(_kind_desc('adam'), clipnorm=c)
    want = orst.restate(desc, p, [g[0]], (7,), m, v)
    assert want['norm'] == np.float64(np.float32(c)) and want['scale'] == 1.0
    unclipped = orst.restate(_kind_desc('adam'), p, [g[0]], (7,), m, v)
    k = dict(g=g, p=p, m=m, v=v, desc=desc, ranges=[], want=want, count=count, stride=count, counts=(7,))
    _against_restatement(k)
    for name in ('p', 'm', 'v'):
        _same_bits(want[name], unclipped[name], name)


def test_clipvalue_lets_a_nan_pass():
    count = 1024
    g, p, m, v = _inputs(count, count, (1,))
    g[0, 100] = np.nan
    g[0, 200], g[0, 201] = np.inf, -np.inf
    desc = dict(_kind_desc('sgd'), clipvalue=0.5)
    want = orst.restate(desc, p, [g[0]], (1,), m, v)
    pd, md = _dev(p), _dev(m)
    _call(desc, [], pd, _dev(g), count, (1,), None, md, None, count)
    got_p, got_m = pd.cpu().numpy(), md.cpu().numpy()
    assert np.isnan(got_p[100]) and np.isnan(got_m[100]) and np.isnan(want['p'][100])
    keep = np.arange(count) != 100
    _same_bits(got_p[keep], want['p'][keep], 'p')
    _same_bits(got_m[keep], want['m'][keep], 'm')
    assert got_m[200] == np.float32(np.float32(0.9) * np.float64(m[200]) - np.float64(np.float32(LR)) * 0.5)      # the infinity was clamped


# ---- 2. equivalence with the entries it generalises ---------------------------------------------------------------------------
def _nadam_scalars(desc):
    return [desc[k] for k in orst.NADAM_NAMES]


@pytest.mark.parametrize('shape,large', [(LARGE, True), (SMALL[2], False), (MATRIX, False)], ids=['large', 'scalar', '64-shards'])
def test_nadam_without_options_is_nadam_step_shards_bit_for_bit(shape, large):
    k = _case(shape, 'nadam', 'none', False, large=large)
    k['g_dev'] = _dev(k['g'])
    p0, m0, v0, gm0 = _dev(k['p']), _dev(k['m']), _dev(k['v']), torch.zeros(k['count'], device=DEV)
    with torch.cuda.device(DEV):
        _lib.call('dsen2_nadam_step_shards', _ptr(p0), _ptr(k['g_dev']), k['stride'], len(k['counts']),
                  (_lib.c_int * len(k['counts']))(*k['counts']), _ptr(gm0), _ptr(m0), _ptr(v0), k['count'],
                  *(_nadam_scalars(k['desc']) + [_stream_ptr(DEV)]))
    for with_norm in (False, True):           # one pass, and the two passes a norm asks for
        gm, _, p, m, v = _run(k, with_norm=with_norm)
        for name, a, b in zip(('g_mean', 'p', 'm', 'v'), (gm, p, m, v), (gm0, p0, m0, v0)):
            _same_bits(a, b, 'with_norm %r, %s' % (with_norm, name))


def test_one_shard_is_the_plain_nadam_step_bit_for_bit():
    count = LARGE[0]
    g, p, m, v = _inputs(count, count, (1,))
    desc = _kind_desc('nadam')
    gd, p0, m0, v0 = _dev(g[0]), _dev(p), _dev(m), _dev(v)
    with torch.cuda.device(DEV):
        _lib.call('dsen2_nadam_step', _ptr(p0), _ptr(gd), _ptr(m0), _ptr(v0), count, *(_nadam_scalars(desc) + [_stream_ptr(DEV)]))
    for c in (1, 5, (1 << 24) - 1):
        for norm in (None, torch.zeros(1, dtype=torch.float64, device=DEV)):
            p1, m1, v1 = _dev(p), _dev(m), _dev(v)
            _call(desc, [], p1, gd, count, (c,), None, m1, v1, count, norm)
            for name, a, b in zip(('p', 'm', 'v'), (p1, m1, v1), (p0, m0, v0)):
                _same_bits(a, b, 'count %d, %s' % (c, name))


# ---- 3. the memory contract -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind,shape,with_mean', [('nadam', (4099, 4100, (2, 0, 3)), True), ('adam', (4099, 4100, (2, 0, 3)), True),
                                                  ('nesterov', (4099, 4100, (2, 0, 3)), True), ('adam', ODD_STRIDE, True),
                                                  ('adam', (4099, 4100, (2, 0, 3)), False), ('sgd', LARGE, False)],
                         ids=['nadam', 'adam', 'sgd-nesterov', 'adam-odd-stride', 'adam-mean-in-scratch', 'sgd-large-mean-in-scratch'])
def test_memory_contract(kind, shape, with_mean):
    """Guard bands around every tensor, outputs and scratch poisoned (tests/guarded.py): nothing written outside, dev_g_shards
    unchanged, g_mean and the norm written completely, the restatement's bits whatever the scratch held.  SGD gets no v at all.
    Clipped, so two passes: the step kernel reads the mean and runs in its 16-byte form (its scalar form: the next test)."""
    k = _case(shape, kind, 'both', True, large=shape is LARGE)
    count, stride, counts, sgd = k['count'], k['stride'], k['counts'], k['desc']['kind'] == orst.SGD
    need = _work_bytes(_c_desc(k['desc'], k['ranges']), count, len(counts), with_mean, True)
    assert need > 0

    def call(inp, out, inplace, scratch):
        _call(k['desc'], k['ranges'], inplace[0], inp[0], stride, counts, out[1] if with_mean else None, inplace[1],
              None if sgd else inplace[2], count, out[0], scratch[0])
    outputs = [((1,), torch.float64)] + ([((count,), torch.float32)] if with_mean else [])
    out, inplace = run_three_ways(call, [_dev(k['g'])], outputs, inplace=[_dev(k['p']), _dev(k['m'])] + ([] if sgd else [_dev(k['v'])]),
                                  scratch=[need], device=DEV, what='%s %d' % (kind, count))
    names = ['norm'] + (['g_mean'] if with_mean else []) + ['p', 'm'] + ([] if sgd else ['v'])
    for name, got in zip(names, out + inplace):
        _same_bits(got, k['want'][name], name)


@pytest.mark.parametrize('kind,with_mean', [('nadam', True), ('adam', True), ('adam', False), ('nesterov', True), ('sgd', False)])
def test_scalar_step_kernel_memory_contract(kind, with_mean):
    """The same around the step kernel's SCALAR form: one pass (clipvalue and decay, no clipnorm, no norm asked for, so no scratch)
    over rows at an odd stride, several workgroups.  The guarded tensors themselves are aligned; the rows' starts are not."""
    k = _case(ODD_STRIDE, kind, 'clipvalue', True)
    count, stride, counts, sgd = k['count'], k['stride'], k['counts'], k['desc']['kind'] == orst.SGD
    assert stride % 4 != 0 and len(counts) > 1 and count > 4 * 256
    assert _work_bytes(_c_desc(k['desc'], k['ranges']), count, len(counts), with_mean, False) == 0

    def call(inp, out, inplace, scratch):
        _call(k['desc'], k['ranges'], inplace[0], inp[0], stride, counts, out[0] if with_mean else None, inplace[1],
              None if sgd else inplace[2], count)
    out, inplace = run_three_ways(call, [_dev(k['g'])], [((count,), torch.float32)] if with_mean else [],
                                  inplace=[_dev(k['p']), _dev(k['m'])] + ([] if sgd else [_dev(k['v'])]), device=DEV,
                                  what='%s %d, stride %d' % (kind, count, stride))
    names = (['g_mean'] if with_mean else []) + ['p', 'm'] + ([] if sgd else ['v'])
    for name, got in zip(names, out + inplace):
        _same_bits(got, k['want'][name], name)


# ---- 4. the model -----------------------------------------------------------------------------------------------------------------
BANDS, D, F = (4, 6), 2, 128


def _batch(n, h, w, seed):
    rng = np.random.default_rng(seed)
    xs = [rng.uniform(0.0, 0.5, (n, c, h, w)).astype(np.float32) for c in BANDS]
    return xs, rng.uniform(0.0, 0.5, (n, BANDS[-1], h, w)).astype(np.float32)


def _model(optimizer, flat=None, precision='fp32', mixed_precision=None, seed=1):
    m = s2model(tuple((c, None, None) for c in BANDS), num_layers=D, feature_size=F, device=DEV, precision=precision)
    flat = weights.random_he_uniform(sum(BANDS), BANDS[-1], D, F, seed=seed, bias_scale=0.05) if flat is None else flat
    m.set_weights_flat(flat)
    m.compile(optimizer, mixed_precision=mixed_precision)
    return m, flat


def _optimizer(kind, **options):
    if kind == 'nadam':
        return training.Nadam(lr=LR, **options)
    if kind == 'adam':
        return training.Adam(lr=LR, **options)
    return training.SGD(lr=LR, momentum=0.9, nesterov=kind == 'nesterov', **options)


def _gradient(probe, flat, xs, y):
    """gradients_device of the probe model at the weights `flat`: the keras-flat gradient as a host array."""
    probe.set_weights_flat(flat)
    xd = [_dev(a) for a in xs]
    grad, loss2 = torch.empty(flat.size, device=DEV), torch.empty(2, device=DEV)
    probe.gradients_device(xd, _dev(y), grad, loss2)
    return grad.cpu().numpy()


def _first_norm(precision, mixed, xs, y, shards):
    probe, flat = _model('nadam', precision=precision, mixed_precision=mixed)
    rows = [_gradient(probe, flat, [a[lo:hi] for a in xs], y[lo:hi]) for lo, hi in shards]
    return float(orst.global_norm(orst.mean_gradient(rows, [hi - lo for lo, hi in shards])))


def _steps_against_restatement(kind, precision, mixed, steps, shards=None):
    """train_on_batch against gradients_device followed by the restatement on the flat weights, step by step."""
    xs, y = _batch(4, 16, 16, seed=21)
    cuts = [(0, 4)] if shards is None else [(0, 2), (2, 4)]
    counts = [hi - lo for lo, hi in cuts]
    clipnorm = float(np.float32(_first_norm(precision, mixed, xs, y, cuts) / 2))
    options = dict(clipnorm=clipnorm, weight_decay=WD)
    model, flat = _model(_optimizer(kind, **options), precision=precision, mixed_precision=mixed)
    probe, _ = _model('nadam', precision=precision, mixed_precision=mixed)
    ranges = training.decay_ranges(sum(BANDS), BANDS[-1], D, F)
    twin = _optimizer(kind, **options)
    m, v = np.zeros_like(flat), np.zeros_like(flat)
    for step in range(steps):
        rows = [_gradient(probe, flat, [a[lo:hi] for a in xs], y[lo:hi]) for lo, hi in cuts]
        want = orst.restate(dict(twin.next_step(), kind=twin.KIND, **options), flat, rows, counts, m, v, ranges)
        if step == 0:
            assert want['scale'] < 1.0                       # the clip acts
        model.train_on_batch(xs, y, shards=shards)
        _same_bits(model.get_weights_flat(), want['p'], '%s step %d' % (kind, step + 1))
        assert model.last_grad_norm() == float(want['norm'])
        flat, m, v = want['p'], want['m'], want['v'] if want['v'] is not None else v
    assert model.optimizer.iterations == steps
    return model


@pytest.mark.parametrize('kind', KINDS)
def test_train_on_batch_equals_gradients_and_the_restatement(kind):
    model = _steps_against_restatement(kind, 'fp32', None, 3)
    st = model._train_state()
    assert (st['v'] is None) == (kind in ('sgd', 'nesterov'))


@pytest.mark.parametrize('precision,mixed', [('fp32', 'bf16'), ('bf16x3', None)])
def test_one_step_in_the_other_arithmetics(precision, mixed):
    _steps_against_restatement('adam', precision, mixed, 1)


@pytest.mark.parametrize('kind', ['adam', 'nesterov'])
def test_two_shards_equal_the_restatement_on_the_shard_gradients(kind):
    _steps_against_restatement(kind, 'fp32', None, 2, shards=2)


@pytest.mark.parametrize('kind', ['nadam', 'adam', 'sgd'])
def test_a_clipnorm_far_above_the_norm_changes_nothing(kind):
    xs, y = _batch(4, 16, 16, seed=21)
    a, _ = _model(_optimizer(kind, clipnorm=1e6))
    b, _ = _model(_optimizer(kind))
    for _ in range(2):
        assert a.train_on_batch(xs, y) == b.train_on_batch(xs, y)
    _same_bits(a.get_weights_flat(), b.get_weights_flat(), kind)
    assert 0.0 < a.last_grad_norm() < 1e6
    if kind == 'nadam':
        with pytest.raises(RuntimeError):
            b.last_grad_norm()                              # a Nadam without options steps through the old kernels: no norm
    else:
        assert b.last_grad_norm() == a.last_grad_norm()     # formed without clipnorm too: look first, then choose a clipnorm


def test_fit_corpus_equals_the_same_steps_through_train_on_batch():
    rng = np.random.default_rng(3)
    tile = (rng.integers(200, 12000, (24 * 4, 40 * 4, 4)).astype(np.uint16), rng.integers(200, 12000, (24 * 2, 40 * 2, 6)).astype(np.uint16))
    c = corpus.TileCorpus([tile], device=DEV)
    batch, steps, seed = 4, 4, 11
    make = lambda: training.Adam(lr=LR, clipnorm=0.05)      # noqa: E731
    a, _ = _model(make())
    b, _ = _model(make())
    a.fit_corpus(c, batch, steps, epochs=1, seed=seed, verbose=0)
    sampler = corpus.CorpusSampler(c, seed, False)
    for _ in range(steps):
        xs, y = c.batch(sampler.draw(batch))
        b.train_on_batch([t.cpu().numpy() for t in xs], y.cpu().numpy())
    _same_bits(a.get_weights_flat(), b.get_weights_flat(), 'fit_corpus against train_on_batch')
    assert a.optimizer.iterations == b.optimizer.iterations == steps and a.last_grad_norm() == b.last_grad_norm() > 0.05


# ---- 5. two ranks equal the one-process restatement, byte for byte --------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return str(p)


@pytest.fixture(scope='module')
def tiny_data(tmp_path_factory):
    """7 training and 3 validation patches of 8 x 8 in two tiles (tests/test_gpu_train_parallel.py's): batches of 5 and 2."""
    root = tmp_path_factory.mktemp('opt_dp')
    rng = np.random.default_rng(41)
    train_dir = root / 'data' / 'train'
    for name, n in (('S2A_A.SAFE', 6), ('S2B_B.SAFE', 4)):
        d = train_dir / name
        os.makedirs(str(d))
        d10 = rng.uniform(0, 3000, (n, 4, 8, 8)).astype(np.float32)
        d20 = rng.uniform(0, 3000, (n, 6, 8, 8)).astype(np.float32)
        np.save(str(d / 'data10.npy'), d10)
        np.save(str(d / 'data20.npy'), d20)
        np.save(str(d / 'data20_gt.npy'), (d20 + rng.uniform(-50, 50, d20.shape)).astype(np.float32))
    val = np.zeros(10, bool)
    val[[1, 4, 8]] = True
    np.save(str(train_dir / 'val_index.npy'), val)
    return root


def _train_args(data, out, extra):
    return ['--path', str(data / 'data'), '--epochs', '2', '--batch_size', '5', '--seed', '3', '--lr', '1e-3', '--out', str(out),
            '--data_parallel'] + list(extra)


def _files(out):
    ckpt, log = out / 's2_038_lr_1e-03.npy', out / 's2_038__lr_1.0e-03.txt'
    assert ckpt.exists() and log.exists(), sorted(os.listdir(str(out)))
    return ckpt.read_bytes(), log.read_bytes()


def _ranks_against_restatement(tiny_data, world, extra, backend='gloo'):
    tag = '%s_w%d_%s' % (backend, world, '_'.join(a.strip('-') for a in extra) or 'fp32')
    out_n, out_1 = tiny_data / ('ranks_' + tag), tiny_data / ('one_' + tag)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    r = subprocess.run([sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', str(world), '--master-addr',
                        '127.0.0.1', '--master-port', _free_port(), '-m', 'dsen2_amd.train'] +
                       _train_args(tiny_data, out_n, extra) + ['--backend', backend],
                       cwd=ROOT, capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert r.stdout.count('Training starts...') == 1                   # one rank talked
    from dsen2_amd import train
    assert train.main(_train_args(tiny_data, out_1, extra) + ['--emulate_world', str(world)]) == 0
    (ckpt_n, log_n), (ckpt_1, log_1) = _files(out_n), _files(out_1)
    assert len(log_n.splitlines()) == 2
    assert log_n == log_1, (log_n, log_1)
    assert ckpt_n == ckpt_1, 'the checkpoint of %d ranks differs from the one-process restatement' % world
    return ckpt_n, log_n


def test_two_ranks_with_adam_clipping_and_decay_equal_the_one_process_restatement(tiny_data):
    ckpt, _ = _ranks_against_restatement(tiny_data, 2, ('--optimizer', 'adam', '--clipnorm', '0.01', '--weight_decay', '0.05'))
    # ... and EACH option reached the step: the same run without either option and with one of the two alone writes another
    # checkpoint every time (a train.py that dropped --clipnorm would write the weight-decay-only one)
    from dsen2_amd import train
    others = {'adam': ['--optimizer', 'adam'], 'clipnorm-only': ['--optimizer', 'adam', '--clipnorm', '0.01'],
              'decay-only': ['--optimizer', 'adam', '--weight_decay', '0.05']}
    seen = {'all': ckpt}
    for name, extra in others.items():
        out = tiny_data / name
        assert train.main(_train_args(tiny_data, out, extra + ['--emulate_world', '2'])) == 0
        seen[name] = _files(out)[0]
    names = sorted(seen)
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            assert seen[a] != seen[b], 'the runs %r and %r wrote the same checkpoint' % (a, b)


# ---- 6. learning ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('make', [lambda: training.SGD(lr=0.05, momentum=0.9), lambda: training.Adam(lr=1e-3, clipnorm=0.05)],
                         ids=['sgd-momentum', 'adam-clipnorm'])
def test_a_teacher_is_learnt(make):
    """tests/test_gpu_train_parallel.py's teacher and student, 20 steps on a batch of 16 as two shards of 8, and its threshold:
    the validation loss falls below half of where it started.  The threshold holds on a CPU restatement of these 20 steps (float64
    torch autograd of the graph for the gradient, tests/optimizer_restatement.py for the update): the MAE ends at 0.234 of its
    start under SGD (lr 0.05, momentum 0.9) and at 0.295 under Adam (lr 1e-3) with clipnorm 0.05, where the first gradient's norm
    is 4.65 and the clip scales it by 0.011; Nadam (lr 1e-3), which that test gates, reaches 0.405 there."""
    def model(seed=1, flat=None):
        return _model(training.Nadam(lr=1e-3) if flat is None else make(), flat=flat, seed=seed)
    teacher, tflat = model(seed=3)
    rng = np.random.default_rng(0)
    xs, _ = _batch(16, 16, 16, seed=14)
    y = teacher.predict(xs)
    student, _ = model(flat=(tflat + rng.uniform(-0.15, 0.15, tflat.shape)).astype(np.float32))
    first = student.evaluate(xs, y)
    h = student.fit(xs, y, batch_size=16, epochs=20, verbose=0, validation_data=(xs, y), shuffle=True, seed=1, data_parallel=True,
                    emulate_world=2)
    last = h.history['val_loss'][-1]
    print('%s learning: validation MAE %.4e -> %.4e (%.3f of the start) in %d steps'
          % (type(student.optimizer).__name__, first[0], last, last / first[0], student.optimizer.iterations))
    assert student.optimizer.iterations == 20
    assert h.history['loss'][0] == pytest.approx(first[0], rel=1e-5)
    assert last < 0.5 * first[0]
