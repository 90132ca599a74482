#!/usr/bin/env python3
"""The evaluation kernels against the HBM roofline: the two passes of the bicubic `imresize`, the per-band error reduction, and the
fused form (second pass + reduction, nothing stored) against resize-then-reduce, at the sizes of a full Sentinel-2 tile:
  5490^2 x 6 float32 enlarged by 2  (the 20 m bands)       1830^2 x 2 float32 enlarged by 6  (the 60 m bands)
and the paper's two further metrics at the enlarged sizes (csrc/quality_metrics.hip): the UIQ map, the fused UIQ sums, SAM, and
their fused bicubic forms (second pass inside the metric's loader, nothing stored), with the numpy restatement of the UIQ
(tests/quality_restatement.py) timed on one 2000^2 band of the host for context; and the SSIM (csrc/ssim.hip, Gaussian window of 11,
L = 10000) at the same sizes: the map, the fused sums, the fused bicubic sums, beside uiq_sums at block 11 on the same images, the
kernel with the same halo and the same staging.
    python tools/bench_evaluate.py [--out FILE.jsonl] [--iters N] [--numpy_band 2000]

`algorithmic bytes` of a kernel = what it must read once + what it must write once (the tap tables, a few hundred KB that stay in
L2, are left out); the roofline is those bytes over the 6.3 TB/s a float4 copy reaches on this part (8 TB/s is the HBM3E spec:
MI355X_MICROARCH.md).  Timed with events on the launch stream after a warm-up of every shape; the tap tables are built and
uploaded outside the timed loops.  Also counted: the un-fused float64 multiplies and adds (2 P - 1 per output, P taps).
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dsen2_amd import imresize as ir      # noqa: E402
from dsen2_amd import metrics             # noqa: E402
from dsen2_amd import patches as P        # noqa: E402

ACHIEVABLE = 6300.0   # GB/s, measured float4 copy (MI355X_MICROARCH.md); the HBM3E spec is 8000


def timeit(fn, iters):
    fn(); fn(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None, help='also append the JSON lines to this file')
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--numpy_band', type=int, default=2000, help='side of the one band the numpy restatement of the UIQ is timed on (0: skip)')
    args = ap.parse_args()
    dev = P.default_device()
    lines = []

    def emit(what, ms, byt, flop=None, **more):
        d = {'kernel': what, 'ms': round(ms, 4), 'algorithmic_MB': round(byt / 1e6, 1), 'GB_per_s': round(byt / ms / 1e6, 1),
             'frac_of_6.3TBps': round(byt / ms / 1e6 / ACHIEVABLE, 3)}
        if flop:
            d['fp64_Gop_per_s'] = round(flop / ms / 1e6, 1)
        d.update(more)
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)

    g = torch.Generator(device='cuda').manual_seed(1)
    for n, c, scale in ((5490, 6, 2), (1830, 2, 6)):
        tag = '%dx%dx%d float32 x%d' % (n, n, c, scale)
        lr = torch.randint(1, 12000, (n, n, c), device=dev, generator=g).to(torch.float32)
        on = n * scale
        gt = torch.randint(1, 12000, (on, on, c), device=dev, generator=g).to(torch.float32)
        t0 = ir.device_taps(n, on, float(scale), dev)
        t1 = ir.device_taps(n, on, float(scale), dev)
        taps = t0[2]
        mid = ir.resize_axis_device(lr, 0, on, t0)
        ms_a = timeit(lambda: ir.resize_axis_device(lr, 0, on, t0), args.iters)
        emit('imresize pass 1 (axis 0) %s' % tag, ms_a, n * n * c * 4 + on * n * c * 8, on * n * c * (2 * taps - 1), taps=taps)
        ms_b = timeit(lambda: ir.resize_axis_device(mid, 1, on, t1), args.iters)
        emit('imresize pass 2 (axis 1) %s' % tag, ms_b, on * n * c * 8 + on * on * c * 8, on * on * c * (2 * taps - 1), taps=taps)
        full = ir.resize_axis_device(mid, 1, on, t1)
        ms_r = timeit(lambda: metrics.error_sums_device(full, gt), args.iters)
        emit('band_errors float64 vs float32 %dx%dx%d' % (on, on, c), ms_r, on * on * c * 12, on * on * c * 4)
        ms_f = timeit(lambda: metrics.resample_error_sums_device(mid, 1, on, t1, gt), args.iters)
        emit('imresize pass 2 + band_errors fused %s' % tag, ms_f, on * n * c * 8 + on * on * c * 4, on * on * c * (2 * taps + 3), taps=taps)
        two = metrics.error_sums_device(full, gt).cpu().numpy()
        one = metrics.resample_error_sums_device(mid, 1, on, t1, gt).cpu().numpy()
        rel = float(np.abs(one / two - 1).max())
        d = {'compare': 'bicubic baseline of %s: resize, store, reduce vs fused' % tag, 'resize_then_reduce_ms': round(ms_a + ms_b + ms_r, 4),
             'fused_ms': round(ms_a + ms_f, 4), 'speedup': round((ms_a + ms_b + ms_r) / (ms_a + ms_f), 3),
             'stored_GB_avoided': round(on * on * c * 8 / 1e9, 3), 'max_relative_difference_of_the_sums': rel}
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)
        # UIQ (8 x 8 windows) and SAM: algorithmic bytes = each input read once (the map's float64 store is listed beside them)
        size = '%dx%dx%d' % (on, on, c)
        win = (on - 7) * (on - 7) * c
        ms = timeit(lambda: metrics.uiq_map_device(full, gt), args.iters)
        emit('uiq_map float64 vs float32 %s' % size, ms, on * on * c * 12, stored_MB=round(win * 8 / 1e6, 1), Gwindows_per_s=round(win / ms / 1e6, 2))
        ms_u = timeit(lambda: metrics.uiq_sums_device(full, gt), args.iters)
        emit('uiq_sums float64 vs float32 %s' % size, ms_u, on * on * c * 12, Gwindows_per_s=round(win / ms_u / 1e6, 2))
        x32 = full.to(torch.float32)
        ms = timeit(lambda: metrics.uiq_sums_device(x32, gt), args.iters)
        emit('uiq_sums float32 vs float32 %s' % size, ms, on * on * c * 8, Gwindows_per_s=round(win / ms / 1e6, 2))
        ms_s = timeit(lambda: metrics.sam_sums_device(full, gt), args.iters)
        emit('sam_sums float64 vs float32 %s' % size, ms_s, on * on * c * 12)
        ms = timeit(lambda: metrics.sam_sums_device(x32, gt), args.iters)
        emit('sam_sums float32 vs float32 %s' % size, ms, on * on * c * 8)
        del x32
        ms_fu = timeit(lambda: metrics.resample_quality_sums_device(mid, 1, on, t1, gt, 8), args.iters)
        emit('imresize pass 2 + uiq_sums fused %s' % tag, ms_fu, on * n * c * 8 + on * on * c * 4, taps=taps, Gwindows_per_s=round(win / ms_fu / 1e6, 2))
        ms_fs = timeit(lambda: metrics.resample_quality_sums_device(mid, 1, on, t1, gt), args.iters)
        emit('imresize pass 2 + sam_sums fused %s' % tag, ms_fs, on * n * c * 8 + on * on * c * 4, taps=taps)
        same = bool(torch.equal(metrics.resample_quality_sums_device(mid, 1, on, t1, gt, 8), metrics.uiq_sums_device(full, gt))
                    and torch.equal(metrics.resample_quality_sums_device(mid, 1, on, t1, gt), metrics.sam_sums_device(full, gt)))
        d = {'compare': 'UIQ and SAM of the bicubic baseline of %s: resize, store, measure vs fused' % tag,
             'uiq_store_then_measure_ms': round(ms_a + ms_b + ms_u, 4), 'uiq_fused_ms': round(ms_a + ms_fu, 4),
             'sam_store_then_measure_ms': round(ms_a + ms_b + ms_s, 4), 'sam_fused_ms': round(ms_a + ms_fs, 4),
             'stored_GB_avoided': round(on * on * c * 8 / 1e9, 3), 'identical_bits': same}
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)
        # SSIM, window 11: the same algorithmic bytes; uiq_sums at block 11 has the same halo tile and the same staging
        win = (on - 10) * (on - 10) * c
        ms = timeit(lambda: metrics.ssim_map_device(full, gt, 1e4), args.iters)
        emit('ssim_map float64 vs float32 %s' % size, ms, on * on * c * 12, stored_MB=round(win * 8 / 1e6, 1), Gwindows_per_s=round(win / ms / 1e6, 2))
        ms_q = timeit(lambda: metrics.ssim_sums_device(full, gt, 1e4), args.iters)
        emit('ssim_sums float64 vs float32 %s' % size, ms_q, on * on * c * 12, Gwindows_per_s=round(win / ms_q / 1e6, 2))
        ms_u11 = timeit(lambda: metrics.uiq_sums_device(full, gt, 11), args.iters)
        emit('uiq_sums block 11 float64 vs float32 %s' % size, ms_u11, on * on * c * 12, Gwindows_per_s=round(win / ms_u11 / 1e6, 2))
        x32 = full.to(torch.float32)
        ms = timeit(lambda: metrics.ssim_sums_device(x32, gt, 1e4), args.iters)
        emit('ssim_sums float32 vs float32 %s' % size, ms, on * on * c * 8, Gwindows_per_s=round(win / ms / 1e6, 2))
        del x32
        ms_fq = timeit(lambda: metrics.resample_ssim_sums_device(mid, 1, on, t1, gt, 1e4), args.iters)
        emit('imresize pass 2 + ssim_sums fused %s' % tag, ms_fq, on * n * c * 8 + on * on * c * 4, taps=taps, Gwindows_per_s=round(win / ms_fq / 1e6, 2))
        same = bool(torch.equal(metrics.resample_ssim_sums_device(mid, 1, on, t1, gt, 1e4), metrics.ssim_sums_device(full, gt, 1e4)))
        d = {'compare': 'SSIM of the bicubic baseline of %s: resize, store, measure vs fused' % tag,
             'ssim_store_then_measure_ms': round(ms_a + ms_b + ms_q, 4), 'ssim_fused_ms': round(ms_a + ms_fq, 4),
             'ssim_sums_over_uiq_sums_block_11': round(ms_q / ms_u11, 3), 'stored_GB_avoided': round(on * on * c * 8 / 1e9, 3),
             'identical_bits': same}
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)
        del lr, gt, mid, full
    if args.numpy_band:
        # context: the numpy restatement of the UIQ on the host against the kernel, one band
        import time
        sys.path.insert(0, os.path.join(ROOT, 'tests'))
        import quality_restatement as qr
        nb = args.numpy_band
        rng = np.random.RandomState(0)
        y = (rng.rand(nb, nb) * 4000).astype(np.float32)
        x = y + rng.normal(0, 20, y.shape).astype(np.float32)
        t = time.time()
        q = qr.uiq_map(x, y)
        host_s = time.time() - t
        tx, ty = torch.from_numpy(x[:, :, None]).to(dev), torch.from_numpy(y[:, :, None]).to(dev)
        ms = timeit(lambda: metrics.uiq_sums_device(tx, ty), args.iters)
        same = metrics.uiq_map_device(tx, ty).cpu().numpy()[:, :, 0].tobytes() == q.tobytes()
        d = {'compare': 'UIQ of one %dx%d float32 band: numpy restatement on the host vs uiq_sums' % (nb, nb), 'numpy_s': round(host_s, 3),
             'uiq_sums_ms': round(ms, 4), 'map_identical_bits': same}
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)
    if args.out:
        with open(args.out, 'a') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
