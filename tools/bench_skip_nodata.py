#!/usr/bin/env python3
"""What SKIP_NODATA costs and saves (profiles/skip_nodata.md), and the multi-rank check of it.

    python tools/bench_skip_nodata.py [--size 10980] [--repeat 3] [--masks none,diagonal,all] [--kernels] [--precision fp32]
        DSen2_20 over a seeded synthetic uint16 tile: the option off (`repeat` times: the baseline and its spread), then on
        for every mask, alternating with nothing else in between; per run the wall time of the call (device-synchronised),
        kept / patches and the residual  T_on - T_off * kept / patches  — what the feature itself costs.  --kernels adds
        dsen2_tile_nodata and dsen2_recompose_rows_nodata alone at that size (device events, 20 launches each, median and
        spread) beside the 6.3 TB/s float4-copy rate tools/bench_evaluate.py uses as the HBM roofline.
    python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr 127.0.0.1 tools/bench_skip_nodata.py \
        --size 1200 --backend gloo --check --masks diagonal,few
        every rank runs DSen2_20(skip_nodata=True) for every mask; with --check rank 0 then leaves the group and compares its
        image with the single-rank one and with where(valid, option off, 0) (`matches_single_rank`, `matches_masked_off`).
Masks: none (0 % no-data), diagonal (x/W + y/H >= 1: about half), all (100 %), few (data in one patch only: fewer kept patches
than ranks, so a shard ends up empty).  Rank 0 prints one JSON line.  Random-init weights; the data is synthetic."""
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
ap.add_argument('--masks', default='none,diagonal,all')
ap.add_argument('--kernels', action='store_true')
ap.add_argument('--precision', default=None, choices=['fp32', 'bf16', 'bf16x3'])
ap.add_argument('--backend', default='nccl', choices=['nccl', 'gloo'])
ap.add_argument('--check', action='store_true', help='multi-rank: verify against the single-rank run and the masked option-off image')
args = ap.parse_args()

rank, world, dev = dist.init_from_env(args.backend)
if args.precision:
    supres.PRECISION = args.precision
n = args.size - args.size % 6
rng = np.random.default_rng(0)
d10 = rng.integers(35, 13110, size=(n, n, 4), dtype=np.uint16)
d20 = rng.integers(35, 13110, size=(n // 2, n // 2, 6), dtype=np.uint16)
tmp = tempfile.mkdtemp()
if rank == 0:               # every other rank receives the weights by broadcast
    np.save(os.path.join(tmp, 's2_032_lr_1e-04.npy'), weights.random_he_uniform(10, 6, 6, 128, seed=11))
supres.MDL_PATH = os.path.join(tmp, '')


def nodata_mask(name):
    """bool [n, n]: True where the tile holds no data."""
    if name == 'none':
        return np.zeros((n, n), bool)
    if name == 'all':
        return np.ones((n, n), bool)
    if name == 'diagonal':
        r = np.arange(n) / float(n)
        return r[None, :] + r[:, None] >= 1.0
    if name == 'few':
        m = np.ones((n, n), bool)
        m[130:170, 20:90] = False          # inside the owned rectangle of patch (1, 0)
        return m
    raise SystemExit('unknown mask %r' % name)


def masked(name):
    a = d10.copy()
    a[nodata_mask(name)] = 0
    return a


def timed(fn, *a, **k):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with contextlib.redirect_stdout(io.StringIO()):
        y = fn(*a, **k)
    torch.cuda.synchronize()
    return y, time.perf_counter() - t0


with contextlib.redirect_stdout(io.StringIO()):          # warm-up: library load, model build, weight upload, both paths
    supres.DSen2_20(d10[:240, :240], d20[:120, :120], False)
    supres.DSen2_20(d10[:240, :240], d20[:120, :120], False, skip_nodata=True)

out = {'tile': [n, n], 'data': 'synthetic', 'n_gpus': world, 'precision': supres.PRECISION}
mask_names = [m for m in args.masks.split(',') if m]
images = {}
if world == 1:
    offs = []
    for _ in range(args.repeat):
        y, t = timed(supres.DSen2_20, d10, d20, False, skip_nodata=False)
        offs.append(round(t, 4))
        del y
    out['off_s_runs'] = offs
    t_off = float(np.median(offs))
    out['off_s_median'] = round(t_off, 4)
    out['on'] = {}
    for name in mask_names:
        a10 = masked(name)
        runs = []
        for _ in range(args.repeat):
            y, t = timed(supres.DSen2_20, a10, d20, False, skip_nodata=True)
            runs.append(round(t, 4))
            del y
        st = supres.last_run_stats()
        t_on = float(np.median(runs))
        out['on'][name] = {'s_runs': runs, 's_median': round(t_on, 4), 'kept': st['kept'], 'patches': st['patches'],
                           'residual_s': round(t_on - t_off * st['kept'] / float(st['patches']), 4)}
        del a10
else:
    out['chunked_gather'] = supres._chunked_gather_wanted()
    for name in mask_names:
        y, t = timed(supres.DSen2_20, masked(name), d20, False, skip_nodata=True)
        assert (y is None) == (rank != 0)
        images[name] = (y, supres.last_run_stats())
        out.setdefault('on', {})[name] = {'s': round(t, 4), 'kept': images[name][1]['kept'], 'patches': images[name][1]['patches']}
    if args.check:
        import torch.distributed as td
        td.barrier()
        td.destroy_process_group()            # dist.rank_world() now reports (0, 1): rank 0 computes everything
        if rank == 0:
            same, masked_off = True, True
            for name in mask_names:
                a10 = masked(name)
                with contextlib.redirect_stdout(io.StringIO()):
                    ref = supres.DSen2_20(a10, d20, False, skip_nodata=True)
                    stats = supres.last_run_stats()
                    off = supres.DSen2_20(a10, d20, False, skip_nodata=False)
                same = same and bool(np.array_equal(ref, images[name][0])) and stats == images[name][1]
                valid = ~nodata_mask(name)
                masked_off = masked_off and bool(np.array_equal(np.where(valid[:, :, None], off, np.float32(0)), images[name][0]))
            out['matches_single_rank'], out['matches_masked_off'] = same, masked_off

if args.kernels and world == 1:
    P, border, C = 128, 8, 6
    img10 = patches._to_device_f32(d10, dev)
    xt, yt, words = patches.nodata_geometry((n, n), P, border)

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

    empty, bits = patches.nodata_device(img10, P, border)
    us = events(lambda: patches.nodata_device(img10, P, border))
    moved = n * n * 4 * 4 + words * 4 * 2 + xt * yt
    out['tile_nodata'] = {'us_median_min_max': [round(v, 1) for v in us], 'bytes': moved,
                          'share_of_copy_rate': round(moved / (us[0] * 1e-6) / (HBM_COPY_TBPS * 1e12), 3)}
    del img10
    kept, slots = patches.slot_map(empty.cpu().numpy())
    assert kept.size == xt * yt
    slots_dev = torch.from_numpy(slots).to(dev)
    buf = torch.zeros((xt * yt, C, P, P), dtype=torch.float32, device=dev)
    img = torch.empty((n, n, C), dtype=torch.float32, device=dev)
    us = events(lambda: patches.recompose_rows_device(buf, border, img, 0, n, scale=2000.0, slots=slots_dev, valid_bits=bits))
    moved = 2 * n * n * C * 4 + words * 4
    out['recompose_rows_nodata'] = {'us_median_min_max': [round(v, 1) for v in us], 'bytes': moved,
                                    'share_of_copy_rate': round(moved / (us[0] * 1e-6) / (HBM_COPY_TBPS * 1e12), 3)}
    us = events(lambda: patches.recompose_rows_device(buf, border, img, 0, n, scale=2000.0))
    out['recompose_rows'] = {'us_median_min_max': [round(v, 1) for v in us], 'bytes': 2 * n * n * C * 4,
                             'share_of_copy_rate': round(2 * n * n * C * 4 / (us[0] * 1e-6) / (HBM_COPY_TBPS * 1e12), 3)}

if rank == 0:
    print(json.dumps(out), flush=True)
dist.finalize()
