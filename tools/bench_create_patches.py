#!/usr/bin/env python3
"""Training-set creation on the GPU: the downPixelAggr kernel against the HBM roofline, and one whole create_patches run.

The kernel moves 2 B in per sample (uint16) and 4 B out per SCALE^2 samples (float32): `algorithmic bytes = input + output`, over
the 8 TB/s of HBM3E, next to the 0.40-0.60 the other patch kernels reach.  Timed with events on the launch stream.
    python tools/bench_create_patches.py [--no-cli] [--out FILE.jsonl]
The whole run: a synthetic full-size tile (10980^2 x 4, 5490^2 x 6, 1830^2 x 2, uint16) written as .npz to a scratch directory,
then `python -m dsen2_amd.create_patches` on it in train mode (8000 crops), wall clock of the process, of which the load of the
2.4 GB .npz is reported separately.
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dsen2_amd import patches as P        # noqa: E402

PEAK = 8000.0   # GB/s, HBM3E spec (MI355X_MICROARCH.md)


def timeit(fn, iters=20):
    fn(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--no-cli', action='store_true', help='kernel timings only')
    ap.add_argument('--out', default=None, help='also append the JSON lines to this file')
    args = ap.parse_args()
    dev = P.default_device()
    lines = []

    def emit(d):
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)

    g = torch.Generator(device='cuda').manual_seed(1)
    for n, c in ((10980, 4), (5490, 6)):
        img = torch.randint(-32768, 32768, (n, n, c), dtype=torch.int16, device=dev, generator=g)
        for scale in (2, 6):
            ms = timeit(lambda: P.down_pixel_aggr_device(img, scale, np.uint16))
            byt = n * n * c * 2 + (n // scale) ** 2 * c * 4
            # non-fused float64 operations: per input sample 1 + 3r (vertical) and per horizontally filtered sample 1 + 3r + 1
            r = P.gaussian_weights(scale)[1]
            flop = n * n * c * ((1 + 3 * r) * 2 + 1)
            emit({'kernel': 'down_pixel_aggr uint16 %dx%dx%d scale %d -> float32' % (n, n, c, scale), 'ms': round(ms, 4),
                  'algorithmic_MB': round(byt / 1e6, 1), 'GB_per_s': round(byt / ms / 1e6, 1), 'frac_of_8TBps': round(byt / ms / 1e6 / PEAK, 3),
                  'fp64_Gop_per_s': round(flop / ms / 1e6, 1)})
        del img
    if not args.no_cli:
        rng = np.random.default_rng(0)
        with tempfile.TemporaryDirectory(prefix='dsen2_cp_') as tmp:
            tile = os.path.join(tmp, 'S2_SYNTH.npz')
            np.savez(tile, data10=rng.integers(1, 12000, (10980, 10980, 4), dtype=np.uint16),
                     data20=rng.integers(1, 12000, (5490, 5490, 6), dtype=np.uint16),
                     data60=rng.integers(1, 12000, (1830, 1830, 2), dtype=np.uint16))
            t0 = time.time()
            z = np.load(tile)
            _ = z['data10'], z['data20']
            load_s = time.time() - t0
            for extra, label in (([], 'train, 8000 crops of 32^2'), (['--run_60'], 'train60, 500 crops of 96^2')):
                t0 = time.time()
                subprocess.run([sys.executable, '-m', 'dsen2_amd.create_patches', tile, '--save_prefix', tmp + '/', '--seed', '1'] + extra,
                               cwd=ROOT, check=True, stdout=subprocess.DEVNULL, timeout=900)
                emit({'run': 'python -m dsen2_amd.create_patches (%s), full-size synthetic tile' % label, 'wall_s': round(time.time() - t0, 2),
                      'of_which_npz_load_s_about': round(load_s, 2)})
    if args.out:
        with open(args.out, 'a') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
