#!/usr/bin/env python3
"""How much of the seam lattice a wider overlap and the feathered blend remove (profiles/seam_blend.md §3).

    python tools/seam_study.py [--size 672] [--margin 80] [--settings 8:0,8:8,16:0,16:4] [--precision fp32]

For DSen2 (d = 6, F = 128) and VDSen2 (d = 32, F = 256) with SYNTHETIC (random He-uniform) weights — the trained checkpoints are
not part of this repository — on a smooth random field: DSen2_20 at every (border, feather) setting against the UNTILED forward
of the same model on the same GPU (the whole 20 m image up-sampled in one piece, one forward over the whole image), on the
pixels at least `margin` from the image edge (beyond VDSen2's receptive-field radius of 66, so neither the network's zero padding
nor the tiling's mirror padding is seen).  Per setting:
    rmse_seam / rmse_rest   normalised (/2000) RMSE to the untiled forward inside the 2 b wide bands around the seam lines of
                            that setting's grid, and outside them;
    step_ratio              mean |out[:, x] - out[:, x - 1]| over the seam columns x = s_t (and the same over rows), divided by
                            the mean over all other columns (rows): 1 = no visible step;
    step_ratio_err          the same on the error image out - untiled, where the scene's own gradients cancel.
Prints one JSON line."""
import argparse
import contextlib
import io
import json
import os
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dsen2_amd import patches, supres, weights        # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--size', type=int, default=672)
ap.add_argument('--margin', type=int, default=80)
ap.add_argument('--settings', default='8:0,8:8,16:0,16:4')
ap.add_argument('--precision', default='fp32', choices=['fp32', 'bf16', 'bf16x3'])
args = ap.parse_args()
supres.PRECISION = args.precision
n = args.size - args.size % 2
settings = [tuple(int(v) for v in s.split(':')) for s in args.settings.split(',') if s]
P = 128


def smooth_field(rng, size, bands, period=24):
    """[size, size, bands] float32 in about 500..6000: coarse noise interpolated linearly (a feature every `period` pixels) plus
    1 % white noise."""
    k = size // period + 2
    coarse = rng.uniform(500.0, 6000.0, size=(k, k, bands))
    pos = np.arange(size) / float(period)
    i0 = np.floor(pos).astype(int)
    f = (pos - i0)[:, None, None]
    rows = coarse[i0] * (1 - f) + coarse[i0 + 1] * f
    f = (pos - i0)[None, :, None]
    img = rows[:, i0] * (1 - f) + rows[:, i0 + 1] * f
    return (img * (1 + 0.01 * rng.standard_normal(img.shape))).astype(np.float32)


rng = np.random.default_rng(0)
d10 = smooth_field(rng, n, 4)
hr20 = smooth_field(rng, n, 6)
d20 = hr20.reshape(n // 2, 2, n // 2, 2, 6).mean(axis=(1, 3)).astype(np.float32)
tmp = tempfile.mkdtemp()
np.save(os.path.join(tmp, 's2_032_lr_1e-04.npy'), weights.random_he_uniform(10, 6, 6, 128, seed=11))
np.save(os.path.join(tmp, 's2_033_lr_1e-04.npy'), weights.random_he_uniform(10, 6, 32, 256, seed=13))
supres.MDL_PATH = os.path.join(tmp, '')


def seam_lines(border):
    inner = P - 2 * border
    tiles = -(-n // inner)
    return [n - inner if t == tiles - 1 else t * inner for t in range(1, tiles)]


def step_ratio(img, lines, margin):
    """Mean absolute step across the seam lines over the mean absolute step across all other lines, rows and columns pooled."""
    core = img[margin:n - margin, margin:n - margin].astype(np.float64)
    seam = np.zeros(n, bool)
    seam[lines] = True
    seam = seam[margin + 1:n - margin]                             # step k of the core lies between lines margin + k and margin + k + 1
    dx = np.abs(np.diff(core, axis=1)).mean(axis=(0, 2))
    dy = np.abs(np.diff(core, axis=0)).mean(axis=(1, 2))
    on = np.concatenate([dx[seam], dy[seam]])
    off = np.concatenate([dx[~seam], dy[~seam]])
    return float(on.mean() / off.mean())


out = {'size': n, 'margin': args.margin, 'precision': args.precision, 'weights': 'synthetic (He-uniform)', 'field': 'smooth random'}
quiet = contextlib.redirect_stdout(io.StringIO())
for deep, label in ((False, 'DSen2'), (True, 'VDSen2')):
    with quiet:
        model = supres._get_model(((4, None, None), (6, None, None)), deep, False)
    dev = patches.default_device()
    x10 = (torch.from_numpy(d10).to(dev) / supres.SCALE).permute(2, 0, 1)[None].contiguous()
    lr = torch.from_numpy(d20).to(dev).permute(2, 0, 1)[None].contiguous()
    x20 = patches.interp_patches_device(lr, (n, n), post_divisor=supres.SCALE)
    untiled = (model.forward_device([x10, x20])[0].permute(1, 2, 0) * supres.SCALE).cpu().numpy()
    out[label] = {}
    m = args.margin
    for border, feather in settings:
        with quiet:
            img = supres.DSen2_20(d10, d20, deep, border=border, feather=feather)
        err = img.astype(np.float64) - untiled
        lines = seam_lines(border)
        band = np.zeros(n, bool)
        for s in lines:
            band[max(0, s - border):s + border] = True
        in_band = (band[:, None] | band[None, :])[m:n - m, m:n - m]
        e = err[m:n - m, m:n - m]
        out[label]['%d:%d' % (border, feather)] = {
            'rmse_seam': float(np.sqrt(np.mean(e[in_band] ** 2))) / supres.SCALE,
            'rmse_rest': float(np.sqrt(np.mean(e[~in_band] ** 2))) / supres.SCALE,
            'seam_share': round(float(in_band.mean()), 3),
            'step_ratio': round(step_ratio(img, lines, m), 4),
            'step_ratio_err': round(step_ratio(err, lines, m), 4),
            'patches': supres.last_run_stats()['patches']}
    del model
    supres.clear_model_cache()
print(json.dumps(out), flush=True)
