#!/usr/bin/env python3
"""tests/golden/ssim_skimage.npz: the SSIM maps scikit-image computes, an independent statement of what csrc/ssim.hip and
tests/ssim_restatement.py define.  Run under the interpreter that has scikit-image (0.18.3 when the file was made):

    python3 tests/golden/make_golden_ssim.py

Inputs: a 48 x 64 x 2 crop of the 20 m bands of tests/golden/tile_T33UUB_crop.npz as the ground truth, and the same plus a seeded
integer perturbation as the image under test; both are stored (uint16) so that the test needs nothing else.  Maps:
structural_similarity(gaussian_weights=True, sigma=1.5, use_sample_covariance=False, data_range=L, full=True) per band, cropped by
(win_size - 1) / 2 = 5 to the valid windows, float64 [38, 54, 2]."""
import os

import numpy as np
import skimage
from skimage.metrics import structural_similarity

HERE = os.path.dirname(os.path.abspath(__file__))
L = 10000.0

gt = np.load(os.path.join(HERE, 'tile_T33UUB_crop.npz'))['d20'][40:88, 30:94, 1:3]
noise = np.rint(np.random.RandomState(2004).normal(0, 120, gt.shape))
x = np.clip(gt.astype(np.float64) + noise, 0, 65535).astype(np.uint16)
maps = []
for c in range(gt.shape[2]):
    _, full = structural_similarity(x[:, :, c].astype(np.float64), gt[:, :, c].astype(np.float64), gaussian_weights=True, sigma=1.5,
                                    use_sample_covariance=False, data_range=L, full=True)
    maps.append(full[5:-5, 5:-5])
q = np.stack(maps, axis=2)
assert q.shape == (38, 54, 2) and q.dtype == np.float64
out = os.path.join(HERE, 'ssim_skimage.npz')
np.savez_compressed(out, x=x, gt=gt, ssim_map=q, data_range=np.float64(L), skimage_version=np.array(skimage.__version__))
print(out, os.path.getsize(out), 'bytes; skimage', skimage.__version__, '; values', int(min(x.min(), gt.min())), '..', int(max(x.max(), gt.max())),
      '; ssim', q.mean(axis=(0, 1)))
