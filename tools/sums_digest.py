#!/usr/bin/env python3
"""Digests of every entry that forms a fixed-order float64 sum, for refactors of those sums that must not change a bit: one JSON
line per case with the sha256 of the entry's outputs.

    python tools/sums_digest.py > after.jsonl        (and the same at the commit before; the two files must be equal)

Entries and shapes (those of the entries' GPU tests): dsen2_loss_grad and dsen2_loss_sums for the 4 kinds x 2 mask modes,
dsen2_abs_sq_error_sums (tests/test_gpu_loss.py, test_gpu_corpus_sampling.py, the sums above their grid's cap included);
dsen2_band_errors and dsen2_imresize_band_errors (test_gpu_evaluate.py); dsen2_uiq_sums, dsen2_sam_sums and their imresize_ forms
(test_gpu_quality_metrics.py); dsen2_ssim_sums and dsen2_imresize_ssim_sums (test_gpu_ssim.py).  Only the C ABI and the metrics
wrappers are used, so the script runs unchanged on older trees.

Each group runs in a child process under a time limit of its own; the first child that fails ends the run.
"""
import ctypes
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GROUP_SECONDS = {'loss': 240, 'band': 120, 'quality': 180, 'ssim': 120}
PARAM = {0: 0.0, 1: 0.0, 2: 0.03, 3: 0.01}                                   # Huber's delta, Charbonnier's epsilon
LOSS_SHAPES = [(1, 1, 1, 1), (3, 6, 5, 7), (2, 2, 9, 21), (2, 15, 4, 4), (5, 6, 232, 232)]
SUMS_ONLY_SHAPES = [(1, 1, 2897, 2897)]                                      # above the 4096 x 2048 cap of the sums' grid
COUNTS = [1, 255, 4097, 2 * 6 * 32 * 32 * 3, 4096 * 2048 + 257]
BAND_CASES = [((300, 300, 6), 'f4', 'f4'), ((257, 129, 6), 'f8', 'f4'), ((64, 100, 2), 'f4', 'f8'), ((91, 37, 13), 'f8', 'f8'),
              ((5, 3, 1), 'f4', 'f4'), ((1200, 1100, 6), 'f4', 'u2')]
BICUBIC_CASES = [((150, 150, 6), 'f4', 2), ((40, 33, 2), 'f8', 6), ((64, 48, 13), 'f4', 2), ((90, 120, 6), 'u2', 2), ((120, 96, 3), 'f4', 0.5)]
UIQ_CASES = [((9, 23, 2), 'f4', 'f4', 8), ((64, 100, 13), 'f8', 'f4', 8), ((300, 257, 6), 'f4', 'u2', 8), ((40, 40, 1), 'f4', 'f8', 8),
             ((64, 100, 13), 'f4', 'f4', 3), ((1100, 2100, 1), 'f4', 'f4', 8)]
SAM_CASES = [((5, 3, 1), 'f4', 'f4'), ((50, 70, 6), 'f4', 'u2'), ((257, 129, 13), 'f8', 'f4'), ((50, 70, 6), 'f4', 'f8')]
QUALITY_BICUBIC_CASES = [((40, 33, 2), 'f8', 6), ((90, 120, 6), 'u2', 2), ((31, 57, 1), 'f4', 2)]
SSIM_CASES = [((11, 11, 1), 11), ((26, 42, 6), 11), ((27, 43, 2), 11), ((40, 70, 3), 11), ((12, 200, 1), 11), ((33, 47, 2), 3), ((33, 47, 2), 15)]
SSIM_BICUBIC_CASES = [((14, 22, 6), 'f4', 2), ((14, 22, 6), 'u2', 2), ((5, 8, 2), 'f4', 6)]


def sha(a):
    import torch
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def emit(entry, case, **digests):
    print(json.dumps(dict(entry=entry, case=case, **digests)), flush=True)


def loss_pair(shape):
    """(out, y) float32 NCHW: errors of both signs, exact zeros among them, a rectangle of no-data pixels and a -0.0 pixel."""
    n, c, h, w = shape
    rng = np.random.default_rng(n * 1000 + c * 100 + h)
    out = rng.uniform(0.1, 0.5, shape).astype(np.float32)
    y = (out + rng.uniform(0.01, 0.06, shape).astype(np.float32) * rng.choice(np.float32([-1, 1]), shape)).astype(np.float32)
    y.ravel()[::7] = out.ravel()[::7]
    y[:, :, :max(1, h // 3), :max(1, w // 3)] = 0.0
    y[0, :, h - 1, 0] = -0.0
    return out, y


def image_pair(shape, dx, dg, seed):
    rng = np.random.RandomState(seed)
    gt = rng.randint(1, 12000, size=shape).astype(dg)
    return (gt.astype(np.float64) + rng.normal(0, 80, size=shape)).astype(dx), gt


def bicubic_pair(shape, dtype, scale, seed):
    """(lr, gt): gt float32 with the shape of the enlargement of lr"""
    from dsen2_amd import imresize as ir
    rng = np.random.RandomState(seed)
    lr = rng.randint(1, 12000, size=shape).astype(dtype)
    size = ir.plan(lr.shape, scalar_scale=scale)[0]
    return lr, rng.randint(1, 12000, size=(size[0], size[1], shape[2])).astype(np.float32)


def group_loss():
    import torch
    from dsen2_amd import _lib
    from dsen2_amd.DSen2Net import _ptr, _stream_ptr
    dev = torch.device('cuda', 0)
    need = ctypes.c_size_t(0)
    _lib.call('dsen2_loss_sums_workspace_bytes', ctypes.byref(need))
    work = torch.zeros(need.value, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        for shape in LOSS_SHAPES + SUMS_ONLY_SHAPES:
            n, c, h, w = shape
            out, y = (torch.from_numpy(a).to(dev) for a in loss_pair(shape))
            for kind in range(4):
                for mask in (0, 1):
                    res = {}
                    if shape in LOSS_SHAPES:
                        g, loss2 = torch.zeros(n * h * w, 16, device=dev), torch.zeros(2, device=dev)
                        _lib.call('dsen2_loss_grad', _ptr(out), _ptr(y), n, c, h, w, kind, PARAM[kind], mask, _ptr(g), _ptr(loss2), _stream_ptr(dev))
                        res.update(grad=sha(g), loss2=sha(loss2))
                    sums = torch.zeros(3, dtype=torch.float64, device=dev)
                    _lib.call('dsen2_loss_sums', _ptr(out), _ptr(y), n, c, h * w, kind, PARAM[kind], mask, _ptr(work), work.numel(), _ptr(sums),
                              _stream_ptr(dev))
                    emit('loss', [list(shape), kind, mask], sums=sha(sums), **res)
        for count in COUNTS:
            rng = np.random.default_rng(count)
            p = (rng.random(count, dtype=np.float32) * 5).astype(np.float32)
            t = (rng.random(count, dtype=np.float32) * 5).astype(np.float32)
            t[::7] = p[::7]
            pair = torch.zeros(2, dtype=torch.float64, device=dev)
            _lib.call('dsen2_abs_sq_error_sums', _ptr(torch.from_numpy(p).to(dev)), _ptr(torch.from_numpy(t).to(dev)), count, _ptr(work),
                      work.numel(), _ptr(pair), _stream_ptr(dev))
            emit('abs_sq_error_sums', count, sums=sha(pair))


def group_band():
    from dsen2_amd import metrics
    for shape, dx, dg in BAND_CASES:
        x, gt = image_pair(shape, dx, dg, shape[0] + shape[1])
        emit('band_errors', [list(shape), dx, dg], sums=sha(metrics.error_sums(x, gt)))
    for shape, dtype, scale in BICUBIC_CASES:
        lr, gt = bicubic_pair(shape, dtype, scale, shape[0] * 7 + shape[1])
        emit('imresize_band_errors', [list(shape), dtype, scale], sums=sha(metrics.bicubic_error_sums(lr, gt, scale)))


def group_quality():
    from dsen2_amd import metrics
    for shape, dx, dg, block in UIQ_CASES:
        x, gt = image_pair(shape, dx, dg, shape[0] * 31 + shape[1])
        emit('uiq_sums', [list(shape), dx, dg, block], sums=sha(metrics.uiq_sums(x, gt, block)))
    for shape, dx, dg in SAM_CASES:
        x, gt = image_pair(shape, dx, dg, shape[0] * 31 + shape[1])
        gt[shape[0] // 2, shape[1] // 2] = 0                                      # a pixel that SAM leaves out
        emit('sam_sums', [list(shape), dx, dg], sums=sha(metrics.sam_sums(x, gt)))
    for shape, dtype, scale in QUALITY_BICUBIC_CASES:
        lr, gt = bicubic_pair(shape, dtype, scale, shape[0] * 7 + shape[1])
        for block in (8, 5):
            emit('imresize_uiq_sums', [list(shape), dtype, scale, block], sums=sha(metrics.bicubic_uiq_sums(lr, gt, scale, block)))
        emit('imresize_sam_sums', [list(shape), dtype, scale], sums=sha(metrics.bicubic_sam_sums(lr, gt, scale)))


def group_ssim():
    from dsen2_amd import metrics
    for shape, win in SSIM_CASES:
        for dx, dg in (('f4', 'f4'), ('f4', 'f8'), ('f8', 'f4')):
            x, gt = image_pair(shape, dx, dg, shape[0] * 31 + shape[1])
            emit('ssim_sums', [list(shape), win, dx, dg], sums=sha(metrics.ssim_sums(x, gt, 1e4, win_size=win)))
    for shape, dtype, scale in SSIM_BICUBIC_CASES:
        lr, gt = bicubic_pair(shape, dtype, scale, shape[0] * 7 + shape[1])
        emit('imresize_ssim_sums', [list(shape), dtype, scale], sums=sha(metrics.bicubic_ssim_sums(lr, gt, scale, 1e4)))


GROUPS = {'loss': group_loss, 'band': group_band, 'quality': group_quality, 'ssim': group_ssim}

if __name__ == '__main__':
    if len(sys.argv) == 3 and sys.argv[1] == '--group':
        GROUPS[sys.argv[2]]()
        sys.exit(0)
    for name in GROUPS:                        # this process never opens the GPU: a child per group, each under its own limit
        sys.stdout.flush()
        code = subprocess.run([sys.executable, os.path.abspath(__file__), '--group', name], timeout=GROUP_SECONDS[name]).returncode
        if code != 0:
            sys.exit('group %s ended with status %d: nothing more is run' % (name, code))
