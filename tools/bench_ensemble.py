"""What the self-ensemble and the training augmentation cost (profiles/self_ensemble.md).

    python tools/bench_ensemble.py [--precision fp32|bf16|bf16x3] [--iters 20] [--out FILE.json]

1. dsen2_dihedral_nchw, every op, at 512 x 10 x 32 x 32 and 64 x 10 x 128 x 128: GB/s of the algorithmic bytes (every element
   read once and written once) beside the 6.3 TB/s a float4 copy reaches on this part (the figure profiles/evaluate.md uses).
2. forward_device_ensemble (all 8 members) against forward_device on the same batch in the same session, and the transforms'
   share (ens - 8 plain) / ens.
3. One train_on_batch with and without augment_ops (host wall clock around synchronised steps: a step uploads its batch).
Device events around `iters` launches (10 x iters for the dihedral kernel, over 8 buffer pairs in turn) after warm-up launches.  The
launches go through Python: where a kernel is shorter than its enqueue (about 10 us), the figure is the enqueue's.  One JSON object
on the last line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from dsen2_amd import training, weights  # noqa: E402
from dsen2_amd.DSen2Net import dihedral, s2model  # noqa: E402

ROOFLINE_GBS = 6300.0
ROTATE = 8


def timed(fn, iters, warm=3):
    for _ in range(warm):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--precision', default='fp32', choices=['fp32', 'bf16', 'bf16x3'])
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--out', default=None)
    args = ap.parse_args(argv)
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    res = {'precision': args.precision, 'roofline_gbs': ROOFLINE_GBS, 'dihedral': [], 'forward': [], 'train': []}

    for shape in ((512, 10, 32, 32), (64, 10, 128, 128)):
        # ROTATE input / output pairs taken in turn (0.3 - 0.7 GB in all): a pair is not served from the 256 MB Infinity Cache by
        # the launch before it.  10 x iters launches after 30 warm-up launches: the kernels take tens of microseconds.
        pairs = [(torch.rand(shape, device=dev), torch.empty(shape, device=dev)) for _ in range(ROTATE)]
        x, out = pairs[0]
        turn = [0]

        def one(**kw):
            a, b = pairs[turn[0] % ROTATE]
            turn[0] += 1
            dihedral(a, out=b, **kw)
        mb = 2 * x.numel() * 4 / 1e6
        for op in range(8):
            ms = timed(lambda: one(op=op), 10 * args.iters, warm=30)
            row = {'shape': list(shape), 'op': op, 'ms': ms, 'algorithmic_mb': mb, 'gbs': mb / ms, 'share_of_roofline': mb / ms / ROOFLINE_GBS}
            res['dihedral'].append(row)
            print('dihedral %s op %d: %.4f ms  %.1f MB  %.0f GB/s  %.3f of the roofline' % ('x'.join(map(str, shape)), op, ms, mb, mb / ms,
                                                                                            row['share_of_roofline']))
        ops = torch.randint(0, 8, (shape[0],), dtype=torch.int32, device=dev)
        ms = timed(lambda: one(ops=ops), 10 * args.iters, warm=30)
        res['dihedral'].append({'shape': list(shape), 'op': 'per-sample', 'ms': ms, 'algorithmic_mb': mb, 'gbs': mb / ms,
                                'share_of_roofline': mb / ms / ROOFLINE_GBS})
        print('dihedral %s per-sample ops: %.4f ms  %.0f GB/s' % ('x'.join(map(str, shape)), ms, mb / ms))

    bands = (4, 6)
    m = s2model(tuple((c, None, None) for c in bands), num_layers=6, feature_size=128, device=dev, precision=args.precision)
    m.set_weights_flat(weights.random_he_uniform(10, 6, 6, 128, seed=1))
    for n, p in ((512, 32), (64, 128)):
        xs = [torch.rand((n, c, p, p), device=dev) * 5 for c in bands]
        out = torch.empty((n, 6, p, p), device=dev)
        plain = timed(lambda: m.forward_device(xs, out=out), args.iters)
        ens = timed(lambda: m.forward_device_ensemble(xs, out=out), args.iters)
        row = {'batch': [n, p, p], 'plain_ms': plain, 'ensemble_ms': ens, 'ratio': ens / plain, 'transforms_share': (ens - 8 * plain) / ens}
        res['forward'].append(row)
        print('DSen2 (d=6, F=128, %s) %dx%dx%d: plain %.3f ms, ensemble %.3f ms (%.2f x), transforms (ens - 8 plain) / ens = %.3f'
              % (args.precision, n, p, p, plain, ens, row['ratio'], row['transforms_share']))

    if args.precision != 'bf16':
        m.compile(training.Nadam(lr=1e-4))
        rng = np.random.default_rng(0)
        n, p = 128, 32
        x = [rng.uniform(0, 0.5, (n, c, p, p)).astype(np.float32) for c in bands]
        y = rng.uniform(0, 0.5, (n, 6, p, p)).astype(np.float32)
        ops = training.AugmentOps(0).draw(n)

        def wall(fn):
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.iters):
                fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3 / args.iters
        plain = wall(lambda: m.train_on_batch(x, y))
        aug = wall(lambda: m.train_on_batch(x, y, augment_ops=ops))
        res['train'].append({'batch': [n, p, p], 'step_ms': plain, 'augmented_step_ms': aug, 'ratio': aug / plain})
        print('train_on_batch %dx%dx%d: %.3f ms plain, %.3f ms augmented (%.3f x)' % (n, p, p, plain, aug, aug / plain))
    line = json.dumps(res)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')
    print(line)
    return 0


if __name__ == '__main__':
    sys.exit(main())
