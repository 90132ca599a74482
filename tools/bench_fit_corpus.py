#!/usr/bin/env python3
"""Training from a device-resident corpus against training from host arrays: one JSON line per measurement.

    python tools/bench_fit_corpus.py --mode kernel [--iters N]
        dsen2_corpus_batch against the chain of launches it replaces (per tile: dsen2_tile_gather x 3 (4), then
        dsen2_upsample_mirror_bilinear and dsen2_dihedral_nchw per tensor, and the torch.cat that joins the tiles' crops), for the
        SAME sample table, alternated in this one process: batch 128 at 20 m and batch 16 at 60 m, 4 synthetic tiles.  HIP events
        around `iters` calls each (a call's launches, not the kernel alone); the kernel's own time comes from
        `rocprofv3 --kernel-trace --stats -- python tools/bench_fit_corpus.py --mode kernel`.  bytes_moved is what the batch must
        read and write, computed from the shapes (bytes_of_batch below).
    python tools/bench_fit_corpus.py --mode epoch [--steps 200]
        wall time of `steps` steps of S2Model.fit_corpus (batch 128, DSen2) against S2Model.fit on host arrays that hold the same
        batches, cut beforehand (shuffle=False) — the path without a corpus — for fp32, bf16x3 and mixed precision, each after a
        warm-up fit of its own and ending in a synchronise; beside `steps` x the device-resident step time (what bench_train.py calls
        step_ms), measured in the same process.
    python tools/bench_fit_corpus.py --mode copies --path corpus|host [--steps 5]
        one epoch of `steps` steps of one path and nothing else, for `rocprofv3 --memory-copy-trace` (a run without counters): the
        copies per step are the difference of two runs with different `steps` over the difference of the steps (the set-up —
        weights, the corpus — is the same in both).
    python tools/bench_fit_corpus.py --mode mask [--iters N]
        dsen2_corpus_origin_mask on a full tile's raw 10 m raster (10980 x 10980 x 4 uint16, origin grid 2745 x 2745): HIP events
        around `iters` calls (two launches each; three with a hold-out table), beside the HBM bound of the bytes it must touch — the whole raster, since band 0
        shares its sectors with the other bands — and the same entry rebuilding the mask from the kept blank map with the 800
        hold-out crops of train.py's default.
    python tools/bench_fit_corpus.py --mode validation [--crops M]
        the end of an epoch with validation on the device (fit_corpus(validation_crops=T)) against the host-array path
        (validation_data=corpus.validation_arrays(...): evaluate -> predict, an upload and a download of every crop) for the SAME
        M crops per tile of 4 tiles: wall time of fits of one step per epoch, alternated, minus the same fit without validation,
        per epoch; beside the time of the forward passes alone — in the device pass's chunks, and at the training batch, which is
        what the host path's predict runs them at — and the bytes the host path moves over the bus.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dsen2_amd import corpus, patches, training, weights  # noqa: E402
from dsen2_amd.DSen2Net import dihedral, s2model  # noqa: E402

DEV = torch.device('cuda', 0)
HBM_PEAK = 8.0e12          # bytes / s (MI355X_MICROARCH.md)
SCALE = 2000


def make_corpus(run_60, tiles=4, grid=(366, 366), seed=0):
    """`tiles` synthetic uint16 tiles whose origin grid is `grid` (20 m: a 1464 x 1464 10 m image each)."""
    rng = np.random.default_rng(seed)
    factors, bands = ((36, 18, 6), (4, 6, 2)) if run_60 else ((4, 2), (4, 6))
    rasters = [tuple(rng.integers(200, 12000, (grid[0] * f, grid[1] * f, c)).astype(np.uint16) for f, c in zip(factors, bands))
               for _ in range(tiles)]
    return corpus.TileCorpus(rasters, run_60=run_60, device=DEV)


def bytes_of_batch(c, n):
    """Bytes one batch must move: every source pixel of every crop once, every output element once."""
    p, s = c.patch, c.scale
    gt_size = c.gt[0].element_size()
    if c.run_60:
        read = p * p * 4 * 4 + 48 * 48 * 6 * 4 + 16 * 16 * 2 * 4 + p * p * 2 * gt_size
        written = p * p * (4 + 6 + 2 + 2) * 4
    else:
        read = p * p * 4 * 4 + 16 * 16 * 6 * 4 + p * p * 6 * gt_size
        written = p * p * (4 + 6 + 6) * 4
    del s
    return n * (read + written + 16)


def chain_batched(c, table, gt_f32):
    """The launches corpus.batch replaces, for a table sorted by tile: per tile one gather per tensor, then one up-sampler launch
    and one dihedral launch per tensor over the whole batch."""
    P, s = c.patch, c.scale
    cols = [[] for _ in range(4 if c.run_60 else 3)]
    for t in range(len(c)):
        org = np.ascontiguousarray(table[table[:, 0] == t, 1:3])
        if not org.shape[0]:
            continue
        n = org.shape[0]
        cols[0].append(patches.gather_patches_device(c.lr[t][0], org, s, 0, P, n, divisor=SCALE))
        if c.run_60:
            cols[1].append(patches.gather_patches_device(c.lr[t][1], org, 3, 0, 48, n))
            cols[2].append(patches.gather_patches_device(c.lr[t][2], org, 1, 0, 16, n))
        else:
            cols[1].append(patches.gather_patches_device(c.lr[t][1], org, 1, 0, 16, n))
        cols[-1].append(patches.gather_patches_device(gt_f32[t], org, s, 0, P, n, divisor=SCALE))
    cols = [torch.cat(col) for col in cols]
    for k in range(1, len(cols) - 1):
        cols[k] = patches.interp_patches_device(cols[k], (P, P), post_divisor=SCALE)
    ops = torch.from_numpy(np.ascontiguousarray(table[:, 3])).to(c.device)
    out = [dihedral(t, ops=ops) for t in cols]
    return out[:-1], out[-1]


def timed(fn, iters, warm=3):
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


def mode_kernel(iters):
    for run_60, n in ((False, 128), (True, 16)):
        c = make_corpus(run_60, grid=(366, 366) if not run_60 else (61, 61))
        table = corpus.CorpusSampler(c, 1, augment=True).draw(n)
        table = np.ascontiguousarray(table[np.argsort(table[:, 0], kind='stable')])
        table_dev = c.upload_table(table)
        gt_f32 = [patches._widen(t, np.uint16) for t in c.gt]
        xs, y = c.batch(table, table_dev=table_dev)
        cx, cy = chain_batched(c, table, gt_f32)
        same = all(torch.equal(a, b) for a, b in zip(xs + [y], cx + [cy]))
        out = (xs, y)
        rounds = []
        for _ in range(3):                                    # alternated: kernel, chain, kernel, chain, ...
            rounds.append((timed(lambda: c.batch(table, table_dev=table_dev, out=out), iters),
                           timed(lambda: chain_batched(c, table, gt_f32), iters)))
        moved = bytes_of_batch(c, n)
        print(json.dumps(dict(mode='kernel', run_60=run_60, batch=n, tiles=len(c), same_bits_as_chain=same, bytes_moved=moved,
                              hbm_bound_us=round(moved / HBM_PEAK * 1e6, 3), workgroups=n * (36 if run_60 else 3),
                              corpus_batch_call_us=[round(a * 1e3, 2) for a, _ in rounds],
                              chain_call_us=[round(b * 1e3, 2) for _, b in rounds])), flush=True)


def _model(precision, mixed):
    m = s2model(((4, None, None), (6, None, None)), num_layers=6, feature_size=128, device=DEV, precision=precision)
    m.set_weights_flat(weights.random_he_uniform(10, 6, 6, 128, seed=1, bias_scale=0.05))
    m.compile(training.Nadam(lr=1e-4), mixed_precision=mixed)
    return m


def host_arrays(c, steps, batch, seed):
    """The batches fit_corpus(seed) cuts in its first `steps` steps, as host arrays in step order."""
    sampler = corpus.CorpusSampler(c, seed, augment=False)
    parts = [[], [], []]
    for _ in range(steps):
        xs, y = c.batch(sampler.draw(batch))
        for col, t in zip(parts, xs + [y]):
            col.append(t.cpu().numpy())
    arrays = [np.concatenate(col) for col in parts]
    return arrays[:2], arrays[2]


def mode_epoch(steps, batch=128):
    c = make_corpus(False)
    x, y = host_arrays(c, steps, batch, seed=1)
    for precision, mixed in (('fp32', None), ('bf16x3', None), ('fp32', 'bf16')):
        m = _model(precision, mixed)
        st = m._train_state()
        xs_d, y_d = [torch.from_numpy(a[:batch]).to(DEV) for a in x], torch.from_numpy(y[:batch]).to(DEV)

        def step():
            m.gradients_device(xs_d, y_d, st['grad'], st['loss2'])
            m.nadam_update(st['grad'])
        step_ms = timed(step, 20)
        walls = {}
        for name in ('fit_corpus', 'fit_host', 'fit_corpus', 'fit_host'):          # alternated, two rounds
            if name == 'fit_corpus':
                run = lambda k: m.fit_corpus(c, batch, k, seed=1, verbose=0)                                       # noqa: E731
            else:
                run = lambda k: m.fit([a[:k * batch] for a in x], y[:k * batch], batch_size=batch, shuffle=False, verbose=0)   # noqa: E731
            run(5)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(steps)
            torch.cuda.synchronize()
            walls.setdefault(name, []).append(round((time.perf_counter() - t0) * 1e3, 1))
        print(json.dumps(dict(mode='epoch', precision=precision, mixed_precision=mixed, batch=batch, steps=steps,
                              device_step_ms=round(step_ms, 4), steps_x_device_step_ms=round(steps * step_ms, 1),
                              fit_corpus_wall_ms=walls['fit_corpus'], fit_host_wall_ms=walls['fit_host'])), flush=True)
        del m


def mode_copies(path, steps, batch=128):
    m = _model('fp32', None)
    if path == 'corpus':
        m.fit_corpus(make_corpus(False, tiles=1), batch, steps, seed=1, verbose=0)
    else:
        rng = np.random.default_rng(0)                    # (what the arrays hold does not change the copies)
        x = [rng.uniform(0, 0.5, (steps * batch, k, 32, 32)).astype(np.float32) for k in (4, 6)]
        y = rng.uniform(0, 0.5, (steps * batch, 6, 32, 32)).astype(np.float32)
        m.fit(x, y, batch_size=batch, shuffle=False, verbose=0)
    torch.cuda.synchronize()
    print(json.dumps(dict(mode='copies', path=path, steps=steps, batch=batch)), flush=True)


def mode_mask(iters):
    grid, f, c = (2745, 2745), 4, 4
    raster = torch.randint(200, 12000, (grid[0] * f, grid[1] * f, c), dtype=torch.int16, device=DEV)       # uint16 bits
    raster[:, :3000, 0] = 0                                          # a blank strip, as a partial swath has
    out = corpus.origin_mask_device(raster, grid, f)
    blank = out[0].clone()
    valid = int(out[2].cpu())
    rng = np.random.default_rng(0)
    holdout = np.ascontiguousarray(rng.integers(0, grid[0] - 16, (800, 2)), dtype=np.int32)
    holdout_dev = torch.from_numpy(holdout).to(DEV)
    rounds = []
    for _ in range(3):                                               # alternated: from the raster, from the blank map
        rounds.append((timed(lambda: corpus.origin_mask_device(raster, grid, f, out=out), iters),
                       timed(lambda: corpus.origin_mask_device(blank, grid, f, holdout, 0, holdout_dev=holdout_dev, out=out), iters)))
    cells, bitmap = out[0].numel(), out[1].numel()
    raster_bytes = raster.numel() * 2
    moved = raster_bytes + cells + cells * 2 + bitmap                # the raster once; the cell map written, then read by the window
    ms = min(a for a, _ in rounds)
    print(json.dumps(dict(mode='mask', raster=list(raster.shape), dtype='uint16', origin_grid=list(grid), valid_origins=valid,
                          raster_bytes=raster_bytes, band0_bytes=raster_bytes // c, bitmap_bytes=bitmap, bytes_moved=moved,
                          hbm_bound_us=round(moved / HBM_PEAK * 1e6, 1), from_raster_call_us=[round(a * 1e3, 1) for a, _ in rounds],
                          achieved_tb_s=round(moved / (ms * 1e-3) / 1e12, 3), fraction_of_hbm_peak=round(moved / (ms * 1e-3) / HBM_PEAK, 3),
                          from_blank_map_800_holdout_call_us=[round(b * 1e3, 1) for _, b in rounds])), flush=True)


def mode_validation(crops, batch=128):
    c = make_corpus(False)
    table = c.validation_table(crops, 1)
    arrays = c.validation_arrays(crops, 1)
    m = _model('fp32', None)
    epochs = 3
    chunk = m._validation_chunk(c)
    xs, y = c.batch(table[:chunk])
    forward_ms = timed(lambda: m.forward_device(xs), 5) * (table.shape[0] / float(xs[0].shape[0]))
    xs_b = [t[:batch].contiguous() for t in xs]                      # the host path's predict runs its forwards at the training batch
    forward_b_ms = timed(lambda: m.forward_device(xs_b), 10) * (table.shape[0] / float(batch))
    runs = {'none': {}, 'host_arrays': dict(validation_data=arrays), 'device': dict(validation_crops=table)}
    walls = {k: [] for k in runs}
    for name in ('none', 'host_arrays', 'device') * 3:                 # alternated, three rounds; the first is the warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m.fit_corpus(c, batch, 1, epochs=epochs, seed=1, verbose=0, **runs[name])
        torch.cuda.synchronize()
        walls[name].append((time.perf_counter() - t0) * 1e3 / epochs)
    per_epoch = {k: [round(v, 2) for v in w[1:]] for k, w in walls.items()}
    base = min(walls['none'][1:])
    crop_bytes = sum(a[0].nbytes for a in arrays[0]) + arrays[1][0].nbytes     # inputs up, ...
    pred_bytes = arrays[1][0].nbytes                                          # ... predictions down
    print(json.dumps(dict(mode='validation', tiles=len(c), crops=int(table.shape[0]), train_batch=batch, device_chunk=int(chunk),
                          epoch_ms=per_epoch, epoch_end_ms={k: round(min(walls[k][1:]) - base, 2) for k in ('host_arrays', 'device')},
                          forwards_alone_ms=round(forward_ms, 2), forwards_at_train_batch_ms=round(forward_b_ms, 2),
                          host_path_bus_bytes=int(table.shape[0] * (crop_bytes - arrays[1][0].nbytes + pred_bytes)),
                          host_arrays_bytes=int(table.shape[0] * crop_bytes), device_path_bus_bytes=int(table.nbytes + 16 * -(-table.shape[0] // chunk)))),
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--mode', required=True, choices=['kernel', 'epoch', 'copies', 'mask', 'validation'])
    ap.add_argument('--crops', type=int, default=800)
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--steps', type=int, default=None)
    ap.add_argument('--path', default='corpus', choices=['corpus', 'host'])
    args = ap.parse_args()
    if args.mode == 'kernel':
        mode_kernel(args.iters)
    elif args.mode == 'epoch':
        mode_epoch(args.steps or 200)
    elif args.mode == 'mask':
        mode_mask(min(args.iters, 20))
    elif args.mode == 'validation':
        mode_validation(args.crops)
    else:
        mode_copies(args.path, args.steps or 5)


if __name__ == '__main__':
    main()
