#!/usr/bin/env python3
"""dsen2_nadam_step_shards alone: one JSON line per (parameter count, number of shards), beside dsen2_nadam_step on the same buffers.

    python tools/bench_nadam_shards.py [--iters N] [--shards 1 2 8] [--rounds R]

HIP events around `iters` back-to-back launches, after a warm-up; `rounds` repetitions interleave the kernels so that a drifting
clock shows as spread, not as a difference: ms is the median over the rounds, ms_min / ms_max its range.  bytes = (shards + 3) reads
+ 3 writes of 4 * count (4 writes with --g_mean), GBps = bytes / ms.  The parameter counts are DSen2's and VDSen2's (6 x 128 and
32 x 256, bands 4 + 6)."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dsen2_amd import _lib, training, weights  # noqa: E402
from dsen2_amd.DSen2Net import _ptr, _stream_ptr  # noqa: E402

NAMES = ('lr', 'b1', 'b2', 'eps', 'mc_t', 'mc_t1', 'ms_new', 'ms_next', 'b2_pow_t')


def timed(fn, iters, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


KINDS = {'nadam': 0, 'adam': 1, 'sgd': 2}


def optimizer_cases(args):
    """(label, kind, options) of the dsen2_optimizer_step rows: --matrix: every kind x {none, clipnorm, clipvalue, both} x {no
    decay, decay}; else the one case the flags describe, if any."""
    def label(kind, o):
        on = [k for k in ('clipnorm', 'clipvalue', 'weight_decay') if o.get(k)]
        return 'optimizer_step<%s%s>' % (kind, ''.join(', ' + k for k in on))
    if args.matrix:
        cases = []
        for kind in KINDS:
            for cn, cv in ((0, 0), (1, 0), (0, 1), (1, 1)):
                for wd in (0, 1):
                    o = dict(clipnorm=cn * 1e-3, clipvalue=cv * 1e-3, weight_decay=wd * 1e-2)
                    cases.append((label(kind, o), kind, o))
        return cases
    o = dict(clipnorm=args.clipnorm, clipvalue=args.clipvalue, weight_decay=args.weight_decay)
    if args.optimizer is None and not any(o.values()):
        return []
    return [(label(args.optimizer or 'nadam', o), args.optimizer or 'nadam', o)]


def optimizer_step(kind, options, k, count, stride, p, g, gm, m, v, dev, args):
    """A closure that calls dsen2_optimizer_step on the benchmark's buffers: k shards of 16 samples, the decay ranges of the
    network whose parameter count this is (every kernel, no bias), the scalars of step 1."""
    import ctypes
    d = _lib.OptimizerDesc()
    d.kind = KINDS[kind]
    s = dict(training.Nadam(lr=1e-4).next_step(), lr_t=training.Adam(lr=1e-4).next_step()['lr_t'], momentum=args.momentum)
    for name in NAMES + ('lr_t', 'momentum'):
        setattr(d, name, s[name])
    d.nesterov = int(args.nesterov)
    d.clipnorm, d.clipvalue, d.weight_decay = options['clipnorm'], options['clipvalue'], options['weight_decay']
    layers = (6, 128) if count == weights.num_params(10, 6, 6, 128) else (32, 256)
    ranges = training.decay_ranges(10, 6, *layers) if options['weight_decay'] else []
    arr = (ctypes.c_uint * max(1, 2 * len(ranges)))(*[x for r in ranges for x in r])
    d.n_ranges, d.host_ranges = len(ranges), ctypes.cast(arr, ctypes.POINTER(ctypes.c_uint)) if ranges else None
    need = ctypes.c_size_t(0)
    _lib.call('dsen2_optimizer_step_work_bytes', ctypes.byref(d), count, k, int(gm is not None), 0, ctypes.byref(need))
    work = torch.empty(need.value, dtype=torch.uint8, device=dev) if need.value else None
    counts = (_lib.c_int * k)(*([16] * k))
    vv = None if kind == 'sgd' else v

    def call(keep=(arr, work)):
        _lib.call('dsen2_optimizer_step', ctypes.byref(d), _ptr(p), _ptr(g), stride, k, counts, _ptr(gm), _ptr(m), _ptr(vv), count, _ptr(work),
                  need.value, None, _stream_ptr(dev))
    return call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--optimizer', default=None, choices=sorted(KINDS), help='also time dsen2_optimizer_step of this kind')
    ap.add_argument('--momentum', type=float, default=0.9)
    ap.add_argument('--nesterov', action='store_true')
    ap.add_argument('--clipnorm', type=float, default=0.0)
    ap.add_argument('--clipvalue', type=float, default=0.0)
    ap.add_argument('--weight_decay', type=float, default=0.0)
    ap.add_argument('--matrix', action='store_true', help='time every instantiation of dsen2_optimizer_step (kind x clipping x decay)')
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--shards', type=int, nargs='+', default=[1, 2, 8])
    ap.add_argument('--g_mean', action='store_true', help='also write the averaged gradient')
    args = ap.parse_args()
    dev = torch.device('cuda', 0)
    s = training.Nadam(lr=1e-4).next_step()
    scalars = [s[k] for k in NAMES]
    for name, d, F in (('dsen2', 6, 128), ('vdsen2', 32, 256)):
        count = weights.num_params(10, 6, d, F)
        stride = -(-(count + 2) // 4) * 4
        kmax = max(args.shards)
        g = torch.randn((kmax, stride), device=dev) * 1e-3
        p, m = torch.randn(count, device=dev), torch.zeros(count, device=dev)
        v = torch.zeros(count, device=dev)
        gm = torch.empty(count, device=dev) if args.g_mean else None

        def plain():
            _lib.call('dsen2_nadam_step', _ptr(p), _ptr(g), _ptr(m), _ptr(v), count, *(scalars + [_stream_ptr(dev)]))

        def sharded(k):
            counts = (_lib.c_int * k)(*([16] * k))
            return lambda: _lib.call('dsen2_nadam_step_shards', _ptr(p), _ptr(g), stride, k, counts, _ptr(gm), _ptr(m), _ptr(v), count,
                                     *(scalars + [_stream_ptr(dev)]))
        kernels = [('nadam_kernel', 1, plain)] + [('nadam_shards_kernel', k, sharded(k)) for k in args.shards]
        for label, kind, options in optimizer_cases(args):
            kernels += [(label, k, optimizer_step(kind, options, k, count, stride, p, g, gm, m, v, dev, args)) for k in args.shards]
        times = {i: [] for i in range(len(kernels))}
        with torch.cuda.device(dev):
            for _ in range(args.rounds):
                for i, (_, _, fn) in enumerate(kernels):
                    times[i].append(timed(fn, args.iters))
        for i, (kernel, k, _) in enumerate(kernels):
            ms = statistics.median(times[i])
            writes = 3 + (1 if (args.g_mean and kernel != 'nadam_kernel') else 0)
            nbytes = 4 * count * (k + 3 + writes)
            if kernel.startswith('optimizer_step'):
                # SGD has no v (one read and one write fewer); clipnorm reads the rows once more for the norm and, with several
                # rows, writes their mean and reads that instead of the rows in the step
                state = 2 if '<sgd' in kernel else 3
                nbytes = 4 * count * (k + 2 * state + (1 if args.g_mean else 0))
                if 'clipnorm' in kernel:
                    nbytes = 4 * count * (k + (2 if k > 1 else 1) + 2 * state)
            print(json.dumps(dict(config=name, count=count, kernel=kernel, shards=k, ms=round(ms, 5), ms_min=round(min(times[i]), 5),
                                  ms_max=round(max(times[i]), 5), bytes=nbytes, GBps=round(nbytes / ms / 1e6, 1))), flush=True)


if __name__ == '__main__':
    main()
