#!/usr/bin/env python3
"""What a wider overlap and the feathered blend cost (profiles/seam_blend.md), and the multi-rank check of them.

    python tools/bench_seam_blend.py [--size 10980] [--repeat 3] [--kernels] [--tile] [--precision fp32]
        --kernels  dsen2_recompose_rows and dsen2_recompose_rows_blend at (border, feather) = (8, 8), (16, 16), (16, 4) on a
                   size^2 x 6 image (device events, 20 launches each, median / min / max): the bytes each launch has to move —
                   the image written, every patch value that carries weight read — and their share of the 6.3 TB/s float4-copy
                   rate tools/bench_evaluate.py uses as the HBM roofline.
        --tile     fp32 DSen2_20 over a seeded synthetic uint16 tile: knobs off (`repeat` times: the baseline and its spread),
                   then (8, 8), (16, None), (16, 4); wall time of the call, device-synchronised, and the patch count.
    python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr 127.0.0.1 tools/bench_seam_blend.py \
        --size 600 --backend gloo --check
        every rank runs DSen2_20 for every setting of --settings (and the first of them with skip_nodata on a tile whose lower
        right half holds no data); with --check rank 0 then leaves the group and compares its images with the single-rank ones
        (`matches_single_rank`).
Rank 0 prints one JSON line.  Random-init weights; the data is synthetic."""
import argparse
import contextlib
import io
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dsen2_amd import dist, patches, supres, weights        # noqa: E402

HBM_COPY_TBPS = 6.3          # tools/bench_evaluate.py: the float4-copy rate taken as the HBM roofline

ap = argparse.ArgumentParser()
ap.add_argument('--size', type=int, default=10980)
ap.add_argument('--repeat', type=int, default=3)
ap.add_argument('--kernels', action='store_true')
ap.add_argument('--tile', action='store_true')
ap.add_argument('--settings', default='8:8,16:0,16:4', help='border:feather pairs (feather 0 = the hard cut)')
ap.add_argument('--precision', default=None, choices=['fp32', 'bf16', 'bf16x3'])
ap.add_argument('--backend', default='nccl', choices=['nccl', 'gloo'])
ap.add_argument('--check', action='store_true', help='multi-rank: verify against the single-rank run')
args = ap.parse_args()

rank, world, dev = dist.init_from_env(args.backend)
if args.precision:
    supres.PRECISION = args.precision
n = args.size - args.size % 6
settings = [tuple(int(v) for v in s.split(':')) for s in args.settings.split(',') if s]
out = {'tile': [n, n], 'data': 'synthetic', 'n_gpus': world, 'precision': supres.PRECISION}


def timed(fn, *a, **k):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with contextlib.redirect_stdout(io.StringIO()):
        y = fn(*a, **k)
    torch.cuda.synchronize()
    return y, time.perf_counter() - t0


if args.tile or world > 1:
    rng = np.random.default_rng(0)
    d10 = rng.integers(35, 13110, size=(n, n, 4), dtype=np.uint16)
    d20 = rng.integers(35, 13110, size=(n // 2, n // 2, 6), dtype=np.uint16)
    tmp = tempfile.mkdtemp()
    if rank == 0:               # every other rank receives the weights by broadcast
        np.save(os.path.join(tmp, 's2_032_lr_1e-04.npy'), weights.random_he_uniform(10, 6, 6, 128, seed=11))
    supres.MDL_PATH = os.path.join(tmp, '')
    with contextlib.redirect_stdout(io.StringIO()):          # warm-up: library load, model build, weight upload, both kernels
        supres.DSen2_20(d10[:240, :240], d20[:120, :120], False)
        supres.DSen2_20(d10[:240, :240], d20[:120, :120], False, border=16, feather=4)

if args.tile and world == 1:
    offs = []
    for _ in range(args.repeat):
        y, t = timed(supres.DSen2_20, d10, d20, False)
        offs.append(round(t, 4))
        del y
    out['off_s_runs'], out['off_s_median'], out['off_patches'] = offs, round(float(np.median(offs)), 4), supres.last_run_stats()['patches']
    out['on'] = {}
    for b, f in settings:
        runs = []
        for _ in range(args.repeat):
            y, t = timed(supres.DSen2_20, d10, d20, False, border=b, feather=f)
            runs.append(round(t, 4))
            del y
        out['on']['%d:%d' % (b, f)] = {'s_runs': runs, 's_median': round(float(np.median(runs)), 4), 'patches': supres.last_run_stats()['patches']}

if world > 1:
    out['chunked_gather'] = supres._chunked_gather_wanted()
    half = d10.copy()
    r = np.arange(n) / float(n)
    half[r[None, :] + r[:, None] >= 1.0] = 0
    jobs = [(d10, b, f, False) for b, f in settings] + [(half, settings[0][0], settings[0][1], True)]
    images = []
    for a10, b, f, skip in jobs:
        y, t = timed(supres.DSen2_20, a10, d20, False, border=b, feather=f, skip_nodata=skip)
        assert (y is None) == (rank != 0)
        images.append(y)
    if args.check:
        import torch.distributed as td
        td.barrier()
        td.destroy_process_group()            # dist.rank_world() now reports (0, 1): rank 0 computes everything
        if rank == 0:
            same = True
            for (a10, b, f, skip), got in zip(jobs, images):
                with contextlib.redirect_stdout(io.StringIO()):
                    ref = supres.DSen2_20(a10, d20, False, border=b, feather=f, skip_nodata=skip)
                same = same and got.shape == ref.shape and bool(np.array_equal(ref.view(np.int32), got.view(np.int32)))
            out['matches_single_rank'], out['jobs'] = same, len(jobs)

if args.kernels and world == 1:
    P, C = 128, 6
    img = torch.empty((n, n, C), dtype=torch.float32, device=dev)

    def events(fn, iters=20):
        fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(iters):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        return float(np.median(ms)) * 1e3, float(min(ms)) * 1e3, float(max(ms)) * 1e3      # microseconds

    def weighted_reads(border, feather):
        """Patch values that carry weight, per channel: sum over the pixels of the number of weighted patches."""
        inner = P - 2 * border
        tiles = -(-n // inner)
        count = np.zeros(n, np.int64)
        for t in range(tiles):
            s = n - inner if t == tiles - 1 else t * inner
            count[max(0, s - feather):min(n, s + inner + feather)] += 1
        return int(count.sum()) ** 2, float((count == 1).mean()) ** 2

    out['kernels'] = {}
    for border, feather in [(8, 0)] + [s for s in settings if s[1]]:
        inner = P - 2 * border
        tiles = -(-n // inner)
        buf = torch.randn((tiles * tiles, C, P, P), dtype=torch.float32, device=dev)
        us = events(lambda: patches.recompose_rows_device(buf, border, img, 0, n, scale=2000.0, feather=feather))
        reads, single = weighted_reads(border, feather) if feather else (n * n, 1.0)
        moved = (n * n + reads) * C * 4
        out['kernels']['%d:%d' % (border, feather)] = {
            'us_median_min_max': [round(v, 1) for v in us], 'patches': tiles * tiles, 'bytes_written': n * n * C * 4, 'bytes_read': reads * C * 4,
            'single_patch_share': round(single, 4), 'share_of_copy_rate': round(moved / (us[0] * 1e-6) / (HBM_COPY_TBPS * 1e12), 3)}
        del buf

if rank == 0:
    print(json.dumps(out), flush=True)
dist.finalize()
