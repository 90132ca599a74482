#!/usr/bin/env python3
"""What a class mask costs and saves (profiles/valid_mask.md), and the multi-rank check of it.

    python tools/bench_valid_mask.py --kernels
        dsen2_class_valid_bits alone through the C ABI (device events around 10 back-to-back launches, 20 times: median, min, max
        in microseconds per launch): a 5490^2 class raster to
        the 10980^2 grid (up = 2) with dilate 0, 8 and 32, and to the 1830^2 grid (down = 3), each next to a device-to-device copy
        that moves the same number of bytes (read plus written), timed the same way in the same run.
    python tools/bench_valid_mask.py [--size 10980] [--repeat 3] [--precision fp32] --tile
        DSen2_20 over a seeded synthetic uint16 tile: without a mask (`repeat` times: the baseline and its spread), with a mask that
        removes nothing, with one that removes a diagonal half; wall time of the call (device-synchronised), kept / patches.
    python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr 127.0.0.1 tools/bench_valid_mask.py \
        --size 600 --backend gloo --check
        every rank runs DSen2_20(mask=...) for the diagonal mask: plain, with skip_nodata and a dilation, and with feather; with
        --check rank 0 then leaves the group and compares its images with the single-rank ones and (the hard cut only: under
        feather a valid pixel beside a skipped patch blends the patches that are left) with where(valid, no mask, 0).
Rank 0 prints one JSON line.  Random-init weights; the data is synthetic."""
import argparse
import contextlib
import ctypes
import io
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dsen2_amd import _lib, dist, masks, supres, weights        # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--size', type=int, default=10980)
ap.add_argument('--repeat', type=int, default=3)
ap.add_argument('--kernels', action='store_true')
ap.add_argument('--tile', action='store_true')
ap.add_argument('--precision', default=None, choices=['fp32', 'bf16', 'bf16x3'])
ap.add_argument('--backend', default='nccl', choices=['nccl', 'gloo'])
ap.add_argument('--check', action='store_true', help='multi-rank: verify against the single-rank run and the masked image without a mask')
args = ap.parse_args()

rank, world, dev = dist.init_from_env(args.backend)
if args.precision:
    supres.PRECISION = args.precision
out = {'data': 'synthetic', 'n_gpus': world, 'precision': supres.PRECISION}


BACK_TO_BACK = 10


def events(fn, iters=20):
    """(median, min, max) microseconds per launch: BACK_TO_BACK launches between two events — the queue stays full, so the host's
    time per call (which for a kernel this short would otherwise be what the events see) is not part of the figure."""
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(BACK_TO_BACK):
            fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / BACK_TO_BACK)
    return [round(float(v) * 1e3, 1) for v in (np.median(ms), min(ms), max(ms))]


if args.kernels and world == 1:
    rng = np.random.default_rng(1)
    scl = rng.choice(np.array([2, 4, 5, 6, 7, 11], np.uint8), size=(5490, 5490))
    scl[rng.random(scl.shape) < 0.001] = 9
    r = np.arange(5490)
    scl[(r[None, :] + r[:, None]) >= 2 * 5490 * 0.8] = 8            # a cloud bank over a corner, isolated pixels elsewhere
    scl_dev = torch.from_numpy(scl).to(dev)
    out['class_valid_bits'] = {}
    table, entry = masks.lut(masks.SCL_INVALID), _lib.load().dsen2_class_valid_bits
    for name, shape, dilate in (('up2_dilate0', (10980, 10980), 0), ('up2_dilate8', (10980, 10980), 8),
                                ('up2_dilate32', (10980, 10980), 32), ('down3_dilate0', (1830, 1830), 0)):
        bits = torch.empty(masks.bitmap_shape(shape), dtype=torch.int32, device=dev)
        masks.valid_bits_device(scl_dev, shape, masks.SCL_INVALID, dilate, out=bits)        # the checked call once; then the entry alone
        up, down = masks.ratio(scl_dev.shape, shape)
        call = (ctypes.c_void_p(scl_dev.data_ptr()), 5490, 5490, table.ctypes.data, up, down, shape[0], shape[1], dilate, None,
                ctypes.c_void_p(bits.data_ptr()), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        us = events(lambda: _lib.check(entry(*call)))
        moved = scl_dev.numel() + bits.numel() * 4
        src = torch.empty(moved // 2, dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)
        copy_us = events(lambda: dst.copy_(src))
        out['class_valid_bits'][name] = {'us_median_min_max': us, 'bytes_read_plus_written': moved, 'copy_us_median_min_max': copy_us,
                                         'times_the_copy': round(us[0] / copy_us[0], 2),
                                         'valid_share': round(float(np.unpackbits(bits.cpu().numpy().view(np.uint8)).sum()) /
                                                              (shape[0] * shape[1]), 4)}
        del bits, src, dst

n = args.size - args.size % 6
if args.tile or world > 1:
    rng = np.random.default_rng(0)
    d10 = rng.integers(35, 13110, size=(n, n, 4), dtype=np.uint16)
    d20 = rng.integers(35, 13110, size=(n // 2, n // 2, 6), dtype=np.uint16)
    tmp = tempfile.mkdtemp()
    if rank == 0:               # every other rank receives the weights by broadcast
        np.save(os.path.join(tmp, 's2_032_lr_1e-04.npy'), weights.random_he_uniform(10, 6, 6, 128, seed=11))
    supres.MDL_PATH = os.path.join(tmp, '')
    r = np.arange(n // 2) / float(n // 2)
    clear = np.full((n // 2, n // 2), 4, np.uint8)                  # a mask that removes nothing
    diagonal = np.where(r[None, :] + r[:, None] >= 1.0, np.uint8(9), np.uint8(4))
    out['tile'] = [n, n]


def timed(fn, *a, **k):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with contextlib.redirect_stdout(io.StringIO()):
        y = fn(*a, **k)
    torch.cuda.synchronize()
    return y, time.perf_counter() - t0


if args.tile and world == 1:
    with contextlib.redirect_stdout(io.StringIO()):          # warm-up: library load, model build, weight upload, both paths
        supres.DSen2_20(d10[:240, :240], d20[:120, :120], False)
        supres.DSen2_20(d10[:240, :240], d20[:120, :120], False, mask=diagonal[:120, :120])
    for name, kw in (('no_mask', {}), ('mask_removes_nothing', dict(mask=clear)), ('mask_diagonal_half', dict(mask=diagonal))):
        runs = []
        for _ in range(args.repeat):
            y, t = timed(supres.DSen2_20, d10, d20, False, **kw)
            runs.append(round(t, 4))
            del y
        st = supres.last_run_stats()
        out[name] = {'s_runs': runs, 's_median': round(float(np.median(runs)), 4), 's_spread': round(max(runs) - min(runs), 4),
                     'kept': st['kept'], 'patches': st['patches']}

if world > 1:
    out['chunked_gather'] = supres._chunked_gather_wanted()
    holes = d10.copy()
    holes[:n // 3, :n // 3] = 0                                     # no-data the mask does not cover: the two bitmaps are ANDed
    runs = {'plain': (d10, dict(mask=diagonal)),
            'nodata_dilate': (holes, dict(mask=diagonal, mask_dilate=5, skip_nodata=True)),
            'feather': (d10, dict(mask=diagonal, feather=4))}
    images = {}
    for name, (a10, kw) in runs.items():
        y, t = timed(supres.DSen2_20, a10, d20, False, **kw)
        assert (y is None) == (rank != 0)
        images[name] = (y, supres.last_run_stats())
        out.setdefault('on', {})[name] = {'s': round(t, 4), 'kept': images[name][1]['kept'], 'patches': images[name][1]['patches']}
    if args.check:
        import torch.distributed as td
        td.barrier()
        td.destroy_process_group()            # dist.rank_world() now reports (0, 1): rank 0 computes everything
        if rank == 0:
            same, masked_off = True, True
            for name, (a10, kw) in runs.items():
                with contextlib.redirect_stdout(io.StringIO()):
                    ref = supres.DSen2_20(a10, d20, False, **kw)
                    stats = supres.last_run_stats()
                same = same and bool(np.array_equal(ref, images[name][0])) and stats == images[name][1]
                if kw.get('feather'):
                    continue
                with contextlib.redirect_stdout(io.StringIO()):
                    off = supres.DSen2_20(a10, d20, False)
                bits = masks.valid_bits_device(diagonal, (n, n), masks.SCL_INVALID, kw.get('mask_dilate', 0), device=dev)
                valid = np.unpackbits(bits.cpu().numpy().view(np.uint8), axis=1, bitorder='little')[:, :n].astype(bool)
                if kw.get('skip_nodata'):
                    valid &= (a10 != 0).any(axis=2)
                masked_off = masked_off and bool(np.array_equal(np.where(valid[:, :, None], off, np.float32(0)), images[name][0]))
            out['matches_single_rank'], out['matches_masked_off'] = same, masked_off

if rank == 0:
    print(json.dumps(out), flush=True)
dist.finalize()
