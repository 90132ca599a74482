"""Training from tiles: the corpus lives on the GPU and every batch is cut from it there.

The reference joins its training stages through the disk: create_patches writes a fixed set of random crops per tile, the
training script loads them all into host memory and gathers a batch from there for every step.  Here

  TileCorpus     does what create_patches.readS2fromFile does in train mode and stops before the crops: every raster of every
                 tile is uploaded in its own dtype (patches.upload_raster), downsampled on the GPU (patches.down_pixel_aggr_device,
                 SCALE 2, or 6 with run_60) and kept there as float32, next to the ground truth (d20, or d60) in ITS own dtype
  CorpusSampler  draws the crops of a step: an int32 [n, 4] table (tile, oy, ox, op)
  corpus.batch   cuts the whole batch in one launch (dsen2_corpus_batch, csrc/corpus_batch.hip): (xs, y) as device tensors,
                 already divided by SCALE = 2000 and turned by the sample's dihedral op

Crop geometry (save_random_patches / save_random_patches60, utils/patches.py:181-271); origins live on the lowest-resolution
low-res grid, the ORIGIN GRID:

                   20 m (run_60=False)                        60 m (run_60=True)
  origin grid      lr20                                       lr60
  data10           lr10 at origin x 2, 32 x 32                lr10 at origin x 6, 96 x 96
  data20           lr20 at origin, 16 x 16, up-sampled x 2    lr20 at origin x 3, 48 x 48, up-sampled x 2
  data60           -                                          lr60 at origin, 16 x 16, up-sampled x 6
  target           d20 at origin x 2, 32 x 32                 d60 at origin x 6, 96 x 96

S2Model.fit_corpus trains from it; `python -m dsen2_amd.train --tiles` is the command line.
"""
import ctypes

import numpy as np
import torch

from . import _lib, patches, training

PATCH_LR = 16                  # edge of a crop on the origin grid
BANDS = (4, 6, 2)              # the Sentinel-2 band groups of the 10 m, 20 m and 60 m inputs


def _check_tile(index, rasters, run_60):
    """The refusals of `python -m dsen2_amd.create_patches` for one tile, before anything reaches the GPU, with its messages:
    a size SCALE does not divide (patches._check_divisible), resolutions that do not have the 10 m : 20 m (: 60 m) ratio
    (patches.check_sizes), a tile with no room for one 16 x 16 low-resolution patch (patches.random_origins).  Returns the extent
    (rows, columns) of the origin grid."""
    scale = 6 if run_60 else 2
    want = 3 if run_60 else 2
    if len(rasters) < want:
        raise ValueError('tile %d: %d rasters where (d10, d20%s) is expected' % (index, len(rasters), ', d60' if run_60 else ''))
    rasters = [np.asarray(a) if not isinstance(a, torch.Tensor) else a for a in rasters[:want]]
    for a, bands in zip(rasters, BANDS):
        if len(a.shape) != 3:
            raise ValueError('expected HWC images, got shape %r' % (tuple(a.shape),))
        if a.shape[2] != bands:
            raise ValueError('tile %d: image of shape %r where %d bands are expected' % (index, tuple(a.shape), bands))
        patches._check_divisible(int(a.shape[0]), int(a.shape[1]), scale)

    class _Shape(object):                                  # what check_sizes looks at
        def __init__(self, a):
            self.shape = (int(a.shape[0]) // scale, int(a.shape[1]) // scale, int(a.shape[2]))
    low = [_Shape(a) for a in rasters]
    ratios = [6, 3, 1] if run_60 else [2, 1]
    patches.check_sizes(low, ratios, 'lower')
    grid = low[-1].shape[:2]
    for lr, s in zip(low, ratios):
        if lr.shape[0] != s * grid[0] or lr.shape[1] != s * grid[1]:
            raise ValueError('image of shape %r is not %d x the lowest-resolution image %r' % (tuple(lr.shape), s, tuple(low[-1].shape)))
    if grid[0] < PATCH_LR or grid[1] < PATCH_LR:
        # (a grid of exactly 16 holds ONE origin, 0: corpus.batch takes it; the reference's randrange(0, 0) and CorpusSampler,
        # which draw below extent - 16, cannot)
        raise ValueError('low-resolution image %r leaves no room for a %d x %d patch' % (tuple(grid), PATCH_LR, PATCH_LR))
    return grid


class TileCorpus(object):
    """tiles: a list of (d10, d20) HWC rasters — (d10, d20, d60) with run_60 — each uint16 or float32.

    Holds, per tile and on the device, the float32 low-resolution images lr10, lr20 (and lr60) and the target (d20, or d60 with
    run_60) in its own dtype: uint16 stays uint16 (as its bits in an int16 tensor) and is widened in the kernel, which is exact.
    A 10980^2 tile is 663 MB of low-resolution images and 362 MB of uint16 target."""

    def __init__(self, tiles, run_60=False, device=None):
        self.run_60 = bool(run_60)
        self.scale = 6 if self.run_60 else 2
        self.patch = PATCH_LR * self.scale
        tiles = [tuple(t) for t in tiles]
        if not tiles:
            raise ValueError('a corpus needs at least one tile')
        self.extents = [_check_tile(i, t, self.run_60) for i, t in enumerate(tiles)]      # every refusal before any upload
        self.device = torch.device(device) if device is not None else patches.default_device()
        if self.device.type == 'cuda' and self.device.index is None:
            self.device = torch.device('cuda', torch.cuda.current_device())
        self.lr, self.gt, self.gt_dtypes = [], [], []
        want = 3 if self.run_60 else 2
        for rasters in tiles:
            lr = []
            for k in range(want):
                t, dt = patches.upload_raster(rasters[k], self.device)
                lr.append(patches.down_pixel_aggr_device(t, self.scale, dt))
                if k == want - 1:
                    self.gt.append(t)
                    self.gt_dtypes.append(dt)
                del t
            self.lr.append(lr)
        self.cout = BANDS[want - 1]
        self._handle = ctypes.c_void_p(0)
        table = (_lib.CorpusTile * len(tiles))()
        for i, (lr, gt, dt, grid) in enumerate(zip(self.lr, self.gt, self.gt_dtypes, self.extents)):
            table[i] = _lib.CorpusTile(lr[0].data_ptr(), lr[1].data_ptr(), lr[2].data_ptr() if self.run_60 else None, gt.data_ptr(),
                                       grid[0], grid[1], _lib.DTYPE_U16 if dt == np.uint16 else _lib.DTYPE_F32)
        _lib.call('dsen2_corpus_create', table, len(tiles), int(self.run_60), ctypes.byref(self._handle))

    def __len__(self):
        return len(self.extents)

    @property
    def nbytes(self):
        """Device bytes of the low-resolution images and the targets."""
        return sum(t.numel() * t.element_size() for lr in self.lr for t in lr) + sum(t.numel() * t.element_size() for t in self.gt)

    def output_shapes(self, n):
        """The shapes of ([x10, x20(, x60)], y) for n samples."""
        p = self.patch
        return [(n, c, p, p) for c in BANDS[:3 if self.run_60 else 2]], (n, self.cout, p, p)

    @staticmethod
    def check_table(table):
        table = np.ascontiguousarray(table, dtype=np.int32)
        if table.ndim != 2 or table.shape[1] != 4:
            raise ValueError('a sample table is int32 [n, 4] (tile, oy, ox, op), got shape %r' % (table.shape,))
        return table

    def upload_table(self, table):
        """The checked host table -> a device tensor, through page-locked memory and without waiting for the stream."""
        return torch.from_numpy(self.check_table(table)).pin_memory().to(self.device, non_blocking=True)

    def batch(self, table, divisor=training.SCALE, table_dev=None, out=None):
        """table: int32 [n, 4] (tile, oy, ox, op) on the host (CorpusSampler.draw).  Returns ([x10, x20(, x60)], y): float32 NCHW
        device tensors, divided by `divisor` (1: the raw values) and turned by D_op — the bits of gather_patches_device (border 0),
        interp_patches_device(post_divisor=divisor) and dihedral(ops=) for the same origins.  The library checks the host table
        (a tile, an origin or an op outside its range is a DSen2Error) and the kernel reads `table_dev`, the same table on the
        device (uploaded here when not given).  out: ([x10, ...], y) to write into.  One launch, no synchronisation."""
        table = self.check_table(table)
        n = table.shape[0]
        x_shapes, y_shape = self.output_shapes(n)
        if out is None:
            xs = [torch.empty(s, dtype=torch.float32, device=self.device) for s in x_shapes]
            y = torch.empty(y_shape, dtype=torch.float32, device=self.device)
        else:
            xs, y = list(out[0]), out[1]
            for t, s in zip(xs + [y], x_shapes + [y_shape]):
                if tuple(t.shape) != s or t.dtype != torch.float32 or not t.is_contiguous() or t.device != self.device:
                    raise ValueError('out must hold contiguous float32 %s tensors of shapes %r' % (self.device, x_shapes + [y_shape]))
        if n == 0:
            return xs, y                     # (an empty tensor has no address to hand to the library)
        if table_dev is None:
            table_dev = self.upload_table(table)
        elif tuple(table_dev.shape) != table.shape or table_dev.dtype != torch.int32 or not table_dev.is_contiguous() or \
                table_dev.device != self.device:
            raise ValueError('table_dev must be the int32 %s copy of the table, shape %r' % (self.device, table.shape))
        with torch.cuda.device(self.device):
            _lib.call('dsen2_corpus_batch', self._handle, table.ctypes.data_as(ctypes.c_void_p), patches._ptr(table_dev),
                      n, float(divisor), patches._ptr(xs[0]), patches._ptr(xs[1]), patches._ptr(xs[2]) if self.run_60 else None,
                      patches._ptr(y), patches._stream(self.device))
        return xs, y

    def validation_arrays(self, crops_per_tile, seed, chunk=256):
        """Host arrays (xs, y) of crops_per_tile fixed crops of every tile, op 0, divided by SCALE: drawn once, from a stream of
        their own (CorpusSampler.VAL_STREAM: the training draws of the same seed do not move), tile after tile — for each tile
        crops_per_tile row origins, then crops_per_tile column origins — and cut by the same kernel.  For fit_corpus's
        validation_data.  Training crops may overlap them, as the reference's random crops overlap its validation patches."""
        CorpusSampler(self)                        # (refuses a tile without a range to draw from)
        entropy = None if seed is None else [int(seed), CorpusSampler.VAL_STREAM]
        rng = np.random.default_rng(np.random.SeedSequence(entropy))
        m = int(crops_per_tile)
        table = np.zeros((len(self) * m, 4), np.int32)
        for i, (eh, ew) in enumerate(self.extents):
            table[i * m:(i + 1) * m, 0] = i
            table[i * m:(i + 1) * m, 1] = rng.integers(0, eh - PATCH_LR, size=m)
            table[i * m:(i + 1) * m, 2] = rng.integers(0, ew - PATCH_LR, size=m)
        x_shapes, y_shape = self.output_shapes(table.shape[0])
        xs = [np.empty(s, np.float32) for s in x_shapes]
        y = np.empty(y_shape, np.float32)
        for i0 in range(0, table.shape[0], chunk):
            dx, dy = self.batch(table[i0:i0 + chunk])
            for a, t in zip(xs + [y], dx + [dy]):
                a[i0:i0 + chunk] = t.cpu().numpy()
        return xs, y

    def __del__(self):
        try:
            if self._handle:
                _lib.load().dsen2_corpus_destroy(self._handle)
                self._handle = ctypes.c_void_p(0)
        except Exception:
            pass


class CorpusSampler(object):
    """The crops of fit_corpus: draw(n) returns the int32 [n, 4] table (tile, oy, ox, op) of the next step's (global) batch.

    Tiles are uniform over the corpus (the reference takes the same number of crops from every tile), origins uniform over
    [0, extent - 16) per axis (the range patches.random_origins draws from), op 0 — or uniform in 0..7 with `augment`
    (include/dsen2_hip.h, "dihedral").  The generator is numpy's default_rng on the seed sequence [seed, STREAM], like
    training.AugmentOps on a stream of its own; seed None: fresh entropy.

    Order of the draws inside one draw(n): n tile indices (integers(0, tiles)); then n row origins, each below its tile's
    extent - 16 (one integers call with the per-sample bounds); then n column origins likewise; then, with augment only, n ops
    (integers(0, 8)).  The table is a function of the seed, the tiles' origin-grid extents and the sequence of n alone: identical
    in every process, whatever the images hold."""
    STREAM = 0x636f7270          # 'corp'
    VAL_STREAM = 0x6376616c      # 'cval'

    def __init__(self, corpus, seed=None, augment=False):
        extents = corpus.extents if hasattr(corpus, 'extents') else corpus
        self.extents = np.asarray([(int(h), int(w)) for h, w in extents], np.int64).reshape(-1, 2)
        if self.extents.shape[0] == 0 or (self.extents - PATCH_LR).min() <= 0:
            raise ValueError('origins are drawn below extent - %d: every tile needs an origin grid larger than %d x %d, got %r'
                             % (PATCH_LR, PATCH_LR, PATCH_LR, self.extents.tolist()))
        self.augment = bool(augment)
        entropy = None if seed is None else [int(seed), self.STREAM]
        self.rng = np.random.default_rng(np.random.SeedSequence(entropy))

    def draw(self, n):
        n = int(n)
        table = np.zeros((n, 4), np.int32)
        tiles = self.rng.integers(0, self.extents.shape[0], size=n)
        table[:, 0] = tiles
        table[:, 1] = self.rng.integers(0, self.extents[tiles, 0] - PATCH_LR)
        table[:, 2] = self.rng.integers(0, self.extents[tiles, 1] - PATCH_LR)
        if self.augment:
            table[:, 3] = self.rng.integers(0, 8, size=n)
        return table
