"""Adam, SGD, gradient clipping and decoupled weight decay, host side (no GPU): the refusals of dsen2_optimizer_step (all of which
come before any launch), the scratch size, the optimisers' scalars against a hand computation, the decay ranges of both networks,
the training CLI's flags, and the dispatch: a Nadam without options still takes the entries it always took."""
import contextlib
import ctypes
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from dsen2_amd import _lib, training, weights  # noqa: E402

PARTIALS_BYTES = 2 * 8 + 4096 * 8          # the sum and its padding, then one partial per block of the largest grid


def _desc(kind=0, ranges=(), **kw):
    d = _lib.OptimizerDesc()
    d.kind = kind
    d.lr, d.b1, d.b2, d.eps = 1e-3, 0.9, 0.999, 1e-8
    d.mc_t, d.mc_t1, d.ms_new, d.ms_next, d.b2_pow_t, d.lr_t = 0.5, 0.5, 0.5, 0.25, 0.999, 1e-3
    for k, x in kw.items():
        setattr(d, k, x)
    flat = [int(x) for r in ranges for x in r]
    arr = (ctypes.c_uint * max(1, len(flat)))(*flat)
    d.n_ranges = kw.get('n_ranges', len(ranges))
    d.host_ranges = ctypes.cast(arr, ctypes.POINTER(ctypes.c_uint)) if (flat or kw.get('n_ranges')) and not kw.get('null_ranges') else None
    d._keep = arr
    return d


def test_the_entries_are_declared_exported_and_built_from_the_new_file():
    from dsen2_amd import build
    build.build()
    lib = _lib.load()
    header = open(os.path.join(ROOT, 'include', 'dsen2_hip.h')).read()
    for name in ('dsen2_optimizer_step', 'dsen2_optimizer_step_work_bytes'):
        assert re.search(r'\bint %s\s*\(' % name, header) and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert 'optimizer_step.hip' in build.SOURCES
    assert 'typedef struct dsen2_optimizer_desc' in header
    fields = re.search(r'typedef struct dsen2_optimizer_desc \{(.*?)\} dsen2_optimizer_desc;', header, re.S).group(1)
    fields = re.sub(r'/\*.*?\*/', '', fields, flags=re.S)
    names = [n.strip(' *') for decl in fields.split(';') if decl.strip() for n in decl.strip().split(None, 1)[1].replace('unsigned', '').split(',')]
    assert names == [f[0] for f in _lib.OptimizerDesc._fields_], names


def test_every_refusal_comes_before_a_launch_and_leaves_p_m_v_alone():
    """No device is needed and none is touched: p, m, v, g and the scratch are HOST arrays here, which a launch could not use and
    a refused call must not write."""
    lib = _lib.load()
    count = 100
    rng = np.random.default_rng(1)
    p, m, v, g = (rng.standard_normal(n).astype(np.float32) for n in (count, count, count, 2 * count))
    work = np.zeros(PARTIALS_BYTES + 16 * count + 64, np.uint8)
    norm = np.zeros(1, np.float64)
    keep = [a.copy() for a in (p, m, v, g, work, norm)]
    ptr = lambda a: None if a is None else ctypes.c_void_p(a.ctypes.data)      # noqa: E731
    aligned = work[-work.ctypes.data % 16:]

    def refused(desc, shards=1, counts=(1,), stride=count, n=count, p_=p, g_=g, m_=m, v_=v, work_=aligned, work_bytes=None, counts_ptr=True,
                norm_=None):
        arr = (ctypes.c_int * max(1, len(counts)))(*counts) if counts_ptr else None
        wb = (0 if work_ is None else work_.size) if work_bytes is None else work_bytes
        rc = lib.dsen2_optimizer_step(ctypes.byref(desc) if desc is not None else None, ptr(p_), ptr(g_), stride, shards, arr, None, ptr(m_),
                                      ptr(v_), n, ptr(work_), wb, ptr(norm_), None)
        assert rc == _lib.ERR_INVALID, (rc, lib.dsen2_last_error())
        msg = lib.dsen2_last_error().decode()
        assert msg
        for a, b in zip((p, m, v, g, work, norm), keep):
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), msg
        return msg

    assert 'descriptor' in refused(None)
    for kind in (-1, 3, 7):
        assert 'kind' in refused(_desc(kind))
    for name in ('clipnorm', 'clipvalue', 'weight_decay', 'momentum'):
        for bad in (-1.0, -1e-30, float('nan'), float('inf')):
            assert name in refused(_desc(2 if name == 'momentum' else 0, **{name: bad})), (name, bad)
    for mu in (1.0, 1.5):
        assert 'momentum' in refused(_desc(2, momentum=mu))
    assert 'ranges' in refused(_desc(0, weight_decay=0.1, ranges=[(k, k + 1) for k in range(0, 258, 2)][:129]))
    assert 'ranges' in refused(_desc(0, weight_decay=0.1, n_ranges=-1))
    assert 'host_ranges' in refused(_desc(0, weight_decay=0.1, n_ranges=2, null_ranges=True))
    for bad in ([(10, 20), (5, 8)],            # unsorted
                [(0, 10), (9, 20)],            # overlapping
                [(0, 10), (10, 10)],           # empty
                [(20, 10)],                    # reversed
                [(0, 10), (90, 101)],          # beyond count
                [(100, 101)]):
        assert 'range' in refused(_desc(1, weight_decay=0.1, ranges=bad)), bad
    assert 'shards' in refused(_desc(1), shards=0, counts=())
    assert 'shards' in refused(_desc(1), shards=65, counts=(1,) * 65)
    for kind in (0, 1):
        assert 'second-moment' in refused(_desc(kind), v_=None)
    # scratch: needed with clipnorm or a norm to report; NULL, too small by one byte, or off the 16-byte grid
    need = ctypes.c_size_t(0)
    for desc, norm_ in ((_desc(1, clipnorm=1.0), None), (_desc(2), norm)):
        assert lib.dsen2_optimizer_step_work_bytes(ctypes.byref(desc), count, 2, 0, int(norm_ is not None), ctypes.byref(need)) == _lib.OK
        assert need.value == PARTIALS_BYTES + 16 * (count // 4)
        assert 'scratch' in refused(desc, shards=2, counts=(1, 1), work_=None, norm_=norm_)
        assert 'scratch' in refused(desc, shards=2, counts=(1, 1), work_bytes=need.value - 1, norm_=norm_)
        assert 'scratch' in refused(desc, shards=2, counts=(1, 1), work_=aligned[4:], norm_=norm_)
    # the count rules of dsen2_nadam_step_shards
    assert 'negative' in refused(_desc(1), shards=2, counts=(3, -1))
    assert 'zero' in refused(_desc(1), shards=3, counts=(0, 0, 0))
    assert '2^24' in refused(_desc(1), shards=2, counts=(1, 1 << 24))
    assert 'shard_stride' in refused(_desc(1), shards=2, counts=(1, 1), stride=count - 1)
    assert 'NULL' in refused(_desc(1), counts_ptr=False)
    for k in ('p_', 'g_', 'm_'):
        assert 'NULL' in refused(_desc(2), **{k: None})
    # not refused for their size: 128 ranges, 64 shards of the largest count, SGD without v; with count = 0 nothing is launched
    arr = (ctypes.c_int * 64)(*([(1 << 24) - 1] * 64))
    assert lib.dsen2_optimizer_step(ctypes.byref(_desc(2, momentum=0.9)), None, None, 0, 64, arr, None, None, None, 0, None, 0, None, None) == _lib.OK
    full = _desc(1, weight_decay=0.1, ranges=[(2 * k, 2 * k + 1) for k in range(128)])
    assert lib.dsen2_optimizer_step_work_bytes(ctypes.byref(full), 256, 1, 0, 0, ctypes.byref(need)) == _lib.OK and need.value == 0


def test_scratch_size():
    lib = _lib.load()
    need = ctypes.c_size_t(7)

    def size(desc, count, shards, have_mean, want_norm):
        assert lib.dsen2_optimizer_step_work_bytes(ctypes.byref(desc), count, shards, have_mean, want_norm, ctypes.byref(need)) == _lib.OK
        return need.value
    plain, clip = _desc(1), _desc(1, clipnorm=0.5)
    assert size(plain, 1000, 4, 0, 0) == 0 and size(_desc(2, clipvalue=1.0, weight_decay=0.1), 1000, 4, 0, 0) == 0
    assert size(plain, 1000, 1, 0, 1) == size(clip, 1000, 1, 0, 0) == PARTIALS_BYTES          # one shard: the row is its own mean
    assert size(clip, 1000, 4, 1, 0) == PARTIALS_BYTES                                          # the caller's g_mean holds it
    assert size(clip, 1001, 4, 0, 0) == PARTIALS_BYTES + 16 * 251
    assert lib.dsen2_optimizer_step_work_bytes(ctypes.byref(clip), 10, 1, 0, 0, None) == _lib.ERR_INVALID
    assert lib.dsen2_optimizer_step_work_bytes(ctypes.byref(clip), 10, 0, 0, 0, ctypes.byref(need)) == _lib.ERR_INVALID


@pytest.mark.parametrize('t', [1, 2, 1000])
def test_adam_and_sgd_scalars_match_a_hand_computation(t):
    lr, b1, b2, eps = 3e-4, 0.8, 0.99, 1e-7
    opt = training.Adam(lr=lr, beta_1=b1, beta_2=b2, epsilon=eps)
    for _ in range(t):
        s = opt.next_step()
    pb1, pb2 = 1.0, 1.0
    for _ in range(t):                      # the powers by repeated multiplication
        pb1, pb2 = pb1 * b1, pb2 * b2
    want = lr * math.sqrt(1.0 - pb2) / (1.0 - pb1)
    assert s['t'] == t == opt.iterations and (s['lr'], s['b1'], s['b2'], s['eps']) == (lr, b1, b2, eps)
    assert s['lr_t'] == pytest.approx(want, rel=1e-12)
    if t == 1:
        assert s['lr_t'] == lr * math.sqrt(1.0 - b2) / (1.0 - b1)
    sgd = training.SGD(lr=0.05, momentum=0.9, nesterov=True)
    for _ in range(t):
        q = sgd.next_step()
    assert q == dict(t=t, lr=0.05, momentum=0.9, nesterov=True)
    sgd.lr = 0.025                          # ReduceLROnPlateau writes it
    assert sgd.next_step()['lr'] == 0.025 and sgd.iterations == t + 1
    state = sgd.step_state()
    sgd.next_step()
    sgd.set_step_state(state)
    assert sgd.iterations == t + 1
    sgd.reset()
    opt.reset()
    assert sgd.iterations == opt.iterations == 0 and opt.next_step()['t'] == 1


def test_optimizer_options():
    for cls in (training.Nadam, training.Adam, training.SGD):
        o = cls()
        assert (o.clipnorm, o.clipvalue, o.weight_decay, o.decay_bias) == (0.0, 0.0, 0.0, False) and not o.has_options()
        assert cls(clipnorm=1.0).has_options() and cls(clipvalue=0.5).has_options() and cls(weight_decay=1e-4).has_options()
        with pytest.raises(TypeError):
            cls(1e-3, 0.9, 0.999, 1e-8, 0.004, 1.0)          # the options are keyword-only
        for bad in (-1.0, float('nan'), float('inf')):
            for name in ('clipnorm', 'clipvalue', 'weight_decay'):
                with pytest.raises(ValueError):
                    cls(**{name: bad})
    for mu in (-0.1, 1.0, float('nan')):
        with pytest.raises(ValueError):
            training.SGD(momentum=mu)
    n = training.Nadam(lr=1e-3)
    n.next_step()
    assert n.step_state() == (1, n.m_schedule) and n.m_schedule != 1.0
    assert training.OPTIMIZERS == {'nadam': training.Nadam, 'adam': training.Adam, 'sgd': training.SGD}


@pytest.mark.parametrize('d,feat,kernels', [(6, 128, 14), (32, 256, 66)])
def test_decay_ranges_cover_every_kernel_element_and_no_bias(d, feat, kernels):
    cin, cout = 10, 6
    ranges = training.decay_ranges(cin, cout, d, feat)
    count = weights.num_params(cin, cout, d, feat)
    assert len(ranges) == kernels <= training.MAX_DECAY_RANGES
    is_kernel = np.zeros(count, bool)
    off = 0
    for ci, co in weights.layer_shapes(cin, cout, d, feat):
        is_kernel[off:off + 9 * ci * co] = True
        off += 9 * ci * co + co
    assert off == count
    covered = np.zeros(count, np.int32)
    behind = 0
    for lo, hi in ranges:
        assert behind <= lo < hi <= count
        covered[lo:hi] += 1
        behind = hi
    assert np.array_equal(covered, is_kernel.astype(np.int32))
    assert int((~is_kernel).sum()) == sum(co for _, co in weights.layer_shapes(cin, cout, d, feat))
    assert training.decay_ranges(cin, cout, d, feat, decay_bias=True) == [(0, count)]
    # the library takes them as they are
    need = ctypes.c_size_t(0)
    assert _lib.load().dsen2_optimizer_step_work_bytes(ctypes.byref(_desc(1, weight_decay=0.01, ranges=ranges)), count, 1, 0, 0,
                                                       ctypes.byref(need)) == _lib.OK
    with pytest.raises(ValueError):
        training.decay_ranges(cin, cout, 64, feat)           # 130 kernels


def test_train_cli_flags():
    from dsen2_amd import train
    a = train.parse_args([])
    assert (a.optimizer, a.momentum, a.nesterov, a.clipnorm, a.clipvalue, a.weight_decay) == (None, None, False, None, None, None)
    opt = train.make_optimizer(a)
    assert type(opt) is training.Nadam and not opt.has_options() and train.describe_optimizer(a) is None
    assert (opt.lr, opt.beta_1, opt.beta_2, opt.epsilon, opt.schedule_decay) == (1e-4, 0.9, 0.999, 1e-8, 0.004)
    a = train.parse_args(['--optimizer', 'adam', '--clipnorm', '0.5', '--weight_decay', '1e-4', '--lr', '1e-3', '--data_parallel',
                          '--emulate_world', '2'])
    opt = train.make_optimizer(a)
    assert type(opt) is training.Adam and (opt.lr, opt.clipnorm, opt.clipvalue, opt.weight_decay) == (1e-3, 0.5, 0.0, 1e-4)
    assert train.describe_optimizer(a) == 'adam, clipnorm 0.5, weight_decay 0.0001'
    a = train.parse_args(['--optimizer', 'sgd', '--momentum', '0.9', '--nesterov', '--clipvalue', '0.01', '--mixed_precision', 'bf16'])
    opt = train.make_optimizer(a)
    assert type(opt) is training.SGD and (opt.momentum, opt.nesterov, opt.clipvalue) == (0.9, True, 0.01)
    a = train.parse_args(['--clipnorm', '2', '--precision', 'bf16x3', '--tiles', 'a.npz'])
    opt = train.make_optimizer(a)
    assert type(opt) is training.Nadam and opt.clipnorm == 2.0 and train.describe_optimizer(a) == 'nadam, clipnorm 2'
    for bad in (['--optimizer', 'rmsprop'], ['--momentum', '0.9'], ['--nesterov'], ['--optimizer', 'adam', '--momentum', '0.9'],
                ['--optimizer', 'nadam', '--nesterov'], ['--optimizer', 'sgd', '--momentum', '1'], ['--optimizer', 'sgd', '--momentum', '-0.1'],
                ['--clipnorm', '0'], ['--clipnorm', '-1'], ['--clipvalue', 'nan'], ['--weight_decay', 'inf'], ['--clipvalue', '-0.5'],
                ['--optimizer', 'adam', '--predict', 'w.npy'], ['--clipnorm', '1', '--predict', 'w.npy'],
                ['--weight_decay', '0.1', '--predict', 'w.npy']):
        with pytest.raises(SystemExit):
            train.parse_args(bad)
    for flag in ('--optimizer', '--momentum', '--nesterov', '--clipnorm', '--clipvalue', '--weight_decay'):
        assert flag in train.__doc__, flag


def _fake_model(monkeypatch, calls):
    """An S2Model without a handle or a GPU: every library call is recorded instead of made."""
    from dsen2_amd import DSen2Net
    m = DSen2Net.S2Model.__new__(DSen2Net.S2Model)
    m.precision, m._handle, m.device = 'fp32', None, torch.device('cpu')
    m.bands, m.cin, m.cout, m.num_layers, m.feature_size = (4, 6), 10, 6, 2, 16
    m.optimizer, m._train = None, None
    count = weights.num_params(10, 6, 2, 16)
    m.count_params = lambda: count
    monkeypatch.setattr(DSen2Net._lib, 'call', lambda name, *a: calls.append(name))
    monkeypatch.setattr(DSen2Net, '_stream_ptr', lambda device: None)
    monkeypatch.setattr(torch.cuda, 'device', lambda device: contextlib.nullcontext())
    return m, count


STEP_ENTRIES = ('dsen2_nadam_step', 'dsen2_nadam_step_shards', 'dsen2_optimizer_step')


def test_the_default_compile_is_a_plain_nadam_on_the_old_entries(monkeypatch):
    calls = []
    m, count = _fake_model(monkeypatch, calls)
    m.compile()
    assert type(m.optimizer) is training.Nadam and not m.optimizer.has_options() and m._plain_nadam()
    m.compile('NADAM')
    assert type(m.optimizer) is training.Nadam and m._plain_nadam()
    del calls[:]
    g = torch.zeros(count)
    m.nadam_update(g)
    assert [c for c in calls if c in STEP_ENTRIES] == ['dsen2_nadam_step'] and m.optimizer.iterations == 1
    st = m._train_state()
    assert st['v'] is not None and st['norm'] is None and st['opt_work'] is None and st['ranges'] is None and not st['norm_valid']
    rows = torch.zeros(2, count + 4)
    m.nadam_update_shards(rows, [3, 2])
    assert [c for c in calls if c in STEP_ENTRIES] == ['dsen2_nadam_step', 'dsen2_nadam_step_shards'] and m.optimizer.iterations == 2
    assert calls.count('dsen2_model_set_weights_device') == 2
    with pytest.raises(RuntimeError):
        m.last_grad_norm()


@pytest.mark.parametrize('make,has_v', [(lambda: training.Nadam(clipnorm=1.0), True), (lambda: training.Nadam(weight_decay=1e-4), True),
                                        (lambda: 'adam', True), (lambda: training.Adam(clipvalue=0.1), True),
                                        (lambda: 'sgd', False), (lambda: training.SGD(momentum=0.9, clipnorm=1.0, weight_decay=0.1), False)])
def test_every_other_optimizer_takes_the_new_entry(monkeypatch, make, has_v):
    calls = []
    m, count = _fake_model(monkeypatch, calls)
    m.compile(make())
    assert not m._plain_nadam()
    del calls[:]
    m.nadam_update(torch.zeros(count))
    m.nadam_update_shards(torch.zeros(2, count + 4), [3, 2])
    assert [c for c in calls if c in STEP_ENTRIES] == ['dsen2_optimizer_step'] * 2 and m.optimizer.iterations == 2
    st = m._train_state()
    assert (st['v'] is not None) == has_v and st['norm'].dtype == torch.float64 and st['norm_valid']
    m.last_grad_norm()                       # formed by every step of this route, with or without clipnorm
    n, arr = st['ranges'][1]
    if m.optimizer.weight_decay:
        assert n == 6 and list(arr)[:2] == [0, 9 * 10 * 16]
    else:
        assert (n, arr) == (0, None)
    desc = m._optimizer_desc(m.optimizer.next_step())
    assert desc.kind == m.optimizer.KIND and desc.n_ranges == n
    assert desc.clipnorm == np.float32(m.optimizer.clipnorm) and desc.weight_decay == np.float32(m.optimizer.weight_decay)


def test_options_set_after_the_first_step_move_the_next_step(monkeypatch):
    """An optimiser's options are as mutable as its lr: the route is chosen step by step, the decay ranges follow the options."""
    calls = []
    m, count = _fake_model(monkeypatch, calls)
    m.compile(training.Nadam(lr=1e-3))
    g = torch.zeros(count)
    m.nadam_update(g)
    m.optimizer.clipnorm = 1.0
    m.nadam_update(g)
    st = m._train_state()
    assert [c for c in calls if c in STEP_ENTRIES] == ['dsen2_nadam_step', 'dsen2_optimizer_step'] and st['norm_valid']
    assert st['ranges'][1] == (0, None)
    m.optimizer.weight_decay = 0.01
    m.nadam_update_shards(torch.zeros(2, count + 4), [1, 1])
    n, arr = st['ranges'][1]
    assert n == 6 and list(arr)[:2] == [0, 9 * 10 * 16]
    m.optimizer.decay_bias = True
    m.nadam_update(g)
    n, arr = st['ranges'][1]
    assert n == 1 and list(arr) == [0, count]
    m.optimizer.clipnorm = m.optimizer.weight_decay = 0.0
    m.nadam_update(g)                        # a plain Nadam again: the old entry, and no norm of that step
    assert [c for c in calls if c in STEP_ENTRIES][-1] == 'dsen2_nadam_step' and not st['norm_valid']
    assert m.optimizer.iterations == 5
    with pytest.raises(RuntimeError):
        m.last_grad_norm()


def test_the_largest_finite_float_is_a_finite_option():
    lib = _lib.load()
    need = ctypes.c_size_t(0)
    for x in (3.2e38, float(np.finfo(np.float32).max)):
        for name in ('clipnorm', 'clipvalue', 'weight_decay'):
            assert lib.dsen2_optimizer_step_work_bytes(ctypes.byref(_desc(1, **{name: x})), 100, 1, 0, 0, ctypes.byref(need)) == _lib.OK, (name, x)


def test_compile_refuses_what_is_no_optimizer(monkeypatch):
    calls = []
    m, _ = _fake_model(monkeypatch, calls)
    for bad in ('rmsprop', 'adamw', 3, None, object()):
        with pytest.raises(ValueError):
            m.compile(bad)
    assert m.optimizer is None
    m.num_layers = 64                        # 130 kernels: weight decay has no room for them
    with pytest.raises(ValueError):
        m.compile(training.Adam(weight_decay=0.1))
    m.compile(training.Adam(weight_decay=0.1, decay_bias=True))
    assert isinstance(m.optimizer, training.Adam)
