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

Opt-in: which origins may be drawn.  TileCorpus(skip_blank=True) / origin_masks(holdout=, margin=) compute, on the GPU
(dsen2_corpus_origin_mask, csrc/corpus_mask.hip), one bitmap of VALID origins per tile: an origin is valid when none of the 16 x 16
cells of its crop is blank (a band-0 sample of the raw 10 m raster in the cell's footprint fails v >= 1) or lies within `margin`
cells of a hold-out (validation) crop.  CorpusSampler(masks=) and validation_table(masks=) redraw what is not valid.

Opt-in: class masks.  TileCorpus(class_masks=[raster or None per tile], mask_classes=, mask_dilate=) builds every masked tile's
validity bitmap on the ground-truth grid (masks.valid_bits_device) and zeroes the ground truth there, once
(dsen2_raster_apply_valid): to everything downstream — corpus.batch, the sampler, fit_corpus, validation — the masked pixels are
no-data, which a model compiled with mask_nodata=True keeps out of every loss and gradient (fit_corpus refuses any other model).
The low-resolution INPUTS are not touched.  skip_masked=True also ORs the mask into the blank map, so that no crop touches it.
"""
import ctypes
import sys

import numpy as np
import torch

from . import _lib, masks as masks_mod, patches, training

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


MIN_VALID_SHARE = 64          # a tile needs at least 1 valid origin in 64: the expected number of redraw rounds stays bounded
MAX_REDRAW_ROUNDS = 10000


def mask_shapes(grid):
    """(cell map, packed origin bitmap) shapes of a tile whose origin grid is `grid`: one byte per cell; one bit per origin
    (oy, ox), 0 <= oy <= grid_h - 16, 0 <= ox <= grid_w - 16, in rows padded to whole bytes."""
    gh, gw = int(grid[0]), int(grid[1])
    return (gh, gw), (gh - PATCH_LR + 1, (gw - PATCH_LR + 1 + 7) // 8)


def origin_mask_device(src, grid, footprint, holdout=None, margin=0, holdout_dev=None, out=None):
    """dsen2_corpus_origin_mask (include/dsen2_hip.h, "corpus origin mask") on device tensors.  src: the raw 10 m raster [H, W, C]
    (float32, or int16 holding uint16 bits: patches.upload_raster), H = grid_h * footprint — or a uint8 [grid_h, grid_w] blank
    map.  holdout: host int32 [m, 2] origins (vy, vx) whose crops, grown by `margin` cells, no valid origin's crop may touch.
    Returns (cells, bitmap, count): uint8 [grid_h, grid_w], uint8 [grid_h - 15, ceil((grid_w - 15) / 8)] — np.packbits(valid,
    axis=1, bitorder='little') — and int32 [1], on the device; out: the three tensors to write into.  Nothing synchronises."""
    gh, gw = int(grid[0]), int(grid[1])
    f = int(footprint)
    cells_shape, bitmap_shape = mask_shapes((gh, gw))
    if src.dtype == torch.uint8:
        if tuple(src.shape) != cells_shape:
            raise ValueError('a blank map of shape %r where %r is expected' % (tuple(src.shape), cells_shape))
        dtype, h, w, c = _lib.MASK_BLANK_MAP, gh * f, gw * f, 1
    else:
        if src.dim() != 3 or src.dtype not in (torch.int16, torch.float32):
            raise ValueError('the raster must be an HWC tensor of float32 or of uint16 bits (int16), got %r %s' % (tuple(src.shape), src.dtype))
        dtype = _lib.DTYPE_U16 if src.dtype == torch.int16 else _lib.DTYPE_F32
        h, w, c = (int(s) for s in src.shape)
    if not src.is_contiguous():
        raise ValueError('the raster must be contiguous')
    if holdout is None:
        holdout = np.zeros((0, 2), np.int32)
    holdout = np.ascontiguousarray(holdout, dtype=np.int32)
    if holdout.ndim != 2 or holdout.shape[1] != 2:
        raise ValueError('hold-out origins are int32 [m, 2] (vy, vx), got shape %r' % (holdout.shape,))
    m = holdout.shape[0]
    if m and holdout_dev is None:
        holdout_dev = torch.from_numpy(holdout).to(src.device)
    if m and (tuple(holdout_dev.shape) != holdout.shape or holdout_dev.dtype != torch.int32 or not holdout_dev.is_contiguous() or
              holdout_dev.device != src.device):
        raise ValueError('holdout_dev must be the int32 %s copy of the hold-out origins, shape %r' % (src.device, holdout.shape))
    if out is None:
        out = (torch.empty(cells_shape, dtype=torch.uint8, device=src.device),
               torch.empty(bitmap_shape, dtype=torch.uint8, device=src.device),
               torch.empty(1, dtype=torch.int32, device=src.device))
    cells, bitmap, count = out
    for t, shape, dt in ((cells, cells_shape, torch.uint8), (bitmap, bitmap_shape, torch.uint8), (count, (1,), torch.int32)):
        if tuple(t.shape) != shape or t.dtype != dt or not t.is_contiguous() or t.device != src.device:
            raise ValueError('out must hold contiguous %s tensors: uint8 %r, uint8 %r and int32 (1,)' % (src.device, cells_shape, bitmap_shape))
    if cells.data_ptr() == src.data_ptr():
        raise ValueError('the blank map that is read and the cell map that is written must be two buffers')
    with torch.cuda.device(src.device):
        _lib.call('dsen2_corpus_origin_mask', patches._ptr(src), dtype, h, w, c, gh, gw,
                  holdout.ctypes.data_as(ctypes.c_void_p) if m else None, patches._ptr(holdout_dev) if m else None, m, int(margin),
                  patches._ptr(cells), patches._ptr(bitmap), patches._ptr(count), patches._stream(src.device))
    return cells, bitmap, count


def _download_masks(done):
    """done: the (cells, bitmap, count) device tensors of origin_mask_device, one triple per tile.  ([packed bitmap on the host],
    [count]) in ONE synchronising read: every tile's count (as its 4 bytes) and bitmap travel in one uint8 tensor."""
    parts = [t.view(torch.uint8).reshape(-1) for _, bitmap, count in done for t in (count, bitmap)]
    host = torch.cat(parts).cpu().numpy()
    bitmaps, counts, at = [], [], 0
    for _, bitmap, _ in done:
        counts.append(int.from_bytes(host[at:at + 4].tobytes(), sys.byteorder, signed=True))
        at += 4
        bitmaps.append(host[at:at + bitmap.numel()].reshape(tuple(bitmap.shape)).copy())
        at += bitmap.numel()
    return bitmaps, counts


def check_origin_counts(extents, counts):
    """The stated condition of drawing with masks: a tile whose valid origins number fewer than 1 in MIN_VALID_SHARE of its
    origins (none at all included) is refused — a redraw round then succeeds with a probability that is bounded from below."""
    for i, ((gh, gw), n) in enumerate(zip(extents, counts)):
        total = (int(gh) - PATCH_LR + 1) * (int(gw) - PATCH_LR + 1)
        if int(n) * MIN_VALID_SHARE < total:
            raise ValueError('tile %d: %d of %d origins are valid, fewer than 1 in %d: too little of the tile is left to draw crops from'
                             % (i, int(n), total, MIN_VALID_SHARE))


def _check_masks(extents, masks):
    """masks: one packed origin bitmap per tile (mask_shapes; the first of the two lists TileCorpus.origin_masks returns).
    Returns them as uint8 arrays, after check_origin_counts on their popcounts."""
    masks = [np.ascontiguousarray(b, dtype=np.uint8) for b in masks]
    if len(masks) != len(extents):
        raise ValueError('%d masks for %d tiles' % (len(masks), len(extents)))
    for i, (b, grid) in enumerate(zip(masks, extents)):
        if b.shape != mask_shapes(grid)[1]:
            raise ValueError('tile %d: a packed origin bitmap of shape %r where %r is expected' % (i, b.shape, mask_shapes(grid)[1]))
    check_origin_counts(extents, [int(np.unpackbits(b).sum()) for b in masks])
    return masks


def _valid_rows(masks, rows):
    """Per row (tile, oy, ox, ...) of `rows`: is the origin's bit set in its tile's bitmap."""
    ok = np.zeros(rows.shape[0], bool)
    for i in np.unique(rows[:, 0]):
        sel = rows[:, 0] == i
        oy, ox = rows[sel, 1], rows[sel, 2]
        ok[sel] = (masks[i][oy, ox >> 3] >> (ox & 7).astype(np.uint8)) & 1
    return ok


def _redraw_invalid(rng, table, extents, masks):
    """The redraw rule of drawing with masks, in place: while any sample's origin is not valid, the still-invalid sample indices
    in ascending order get new origins — ONE integers call for their rows with the per-sample bounds, then one for their columns.
    The tile is kept and the op is not touched."""
    bad = np.flatnonzero(~_valid_rows(masks, table))
    rounds = 0
    while bad.size:
        if rounds == MAX_REDRAW_ROUNDS:
            raise RuntimeError('%d samples still have no valid origin after %d redraw rounds' % (bad.size, MAX_REDRAW_ROUNDS))
        rounds += 1
        tiles = table[bad, 0]
        table[bad, 1] = rng.integers(0, extents[tiles, 0] - PATCH_LR)
        table[bad, 2] = rng.integers(0, extents[tiles, 1] - PATCH_LR)
        bad = bad[~_valid_rows(masks, table[bad])]
    return table


class TileCorpus(object):
    """tiles: a list of (d10, d20) HWC rasters — (d10, d20, d60) with run_60 — each uint16 or float32.

    Holds, per tile and on the device, the float32 low-resolution images lr10, lr20 (and lr60) and the target (d20, or d60 with
    run_60) in its own dtype: uint16 stays uint16 (as its bits in an int16 tensor) and is widened in the kernel, which is exact.
    A 10980^2 tile is 663 MB of low-resolution images and 362 MB of uint16 target.

    skip_blank=True (default off): while a tile's raw 10 m raster is still on the device, its BLANK MAP is computed there
    (origin_mask_device: a cell of the origin grid is blank when a BAND-0 sample of d10 in its footprint fails v >= 1, the
    reference's `chan3 < 1`; no other band and no other raster is looked at) and kept, one byte per cell, with a host copy of the
    packed bitmap of origins whose crops are free of blank cells (under 1 MB for a 10980^2 tile).  One line per tile is printed.
    origin_masks() returns the bitmaps; CorpusSampler(masks=) and validation_table(masks=) draw from them.

    class_masks (default None): one 2-D uint8 class raster (Sentinel-2's SCL layer, a cloud-probability layer, ...; on the 10, 20 or
    60 m grid of the tile) or None per tile; mask_classes: the class values that are invalid (None = masks.SCL_INVALID);
    mask_dilate: a dilation of the invalid area in GROUND-TRUTH pixels, 0..32.  While a tile is set up its validity bitmap is built
    on the ground-truth grid ([2 grid_h, 2 grid_w]; run_60: [6 grid_h, 6 grid_w]) and the ground truth is zeroed there, once: the
    masked pixels are no-data from then on, and `class_masked` is True (fit_corpus then wants mask_nodata=True).  The inputs stay
    as they are.  skip_masked=True (needs class_masks): a cell of the origin grid that holds a masked pixel counts as blank — the
    mask is OR-ed into the blank map (into an empty one without skip_blank), origin_masks() returns bitmaps free of it, and the
    rule "fewer than 1 valid origin in 64: refused" applies unchanged."""

    def __init__(self, tiles, run_60=False, device=None, skip_blank=False, class_masks=None, mask_classes=None, mask_dilate=0,
                 skip_masked=False):
        self.run_60 = bool(run_60)
        self.skip_blank = bool(skip_blank)
        self.skip_masked = bool(skip_masked)
        self.scale = 6 if self.run_60 else 2
        self.patch = PATCH_LR * self.scale
        tiles = [tuple(t) for t in tiles]
        if not tiles:
            raise ValueError('a corpus needs at least one tile')
        self.extents = [_check_tile(i, t, self.run_60) for i, t in enumerate(tiles)]      # every refusal before any upload
        class_masks = self._check_class_masks(class_masks, mask_classes, mask_dilate, len(tiles))
        self.class_masked = any(m is not None for m in class_masks)
        if self.skip_masked and not self.class_masked:
            raise ValueError('skip_masked needs class_masks: there is no mask to keep the crops out of')
        mask_classes = masks_mod.SCL_INVALID if mask_classes is None else tuple(mask_classes)
        masked_cells = self.skip_blank or self.skip_masked         # the corpus keeps cell maps and origin bitmaps
        self.device = torch.device(device) if device is not None else patches.default_device()
        if self.device.type == 'cuda' and self.device.index is None:
            self.device = torch.device('cuda', torch.cuda.current_device())
        self.lr, self.gt, self.gt_dtypes = [], [], []
        self.footprint = self.scale * self.scale           # samples of d10 per cell of the origin grid, per axis
        self.blank_cells = None                            # skip_blank: per tile, uint8 [grid_h, grid_w] on the device
        self._blank_masks = None                           # skip_blank: ([packed bitmap on the host], [count])
        pending = []
        want = 3 if self.run_60 else 2
        for i, rasters in enumerate(tiles):
            lr = []
            for k in range(want):
                t, dt = patches.upload_raster(rasters[k], self.device)
                if k == 0 and self.skip_blank:             # d10 is still here: its blank map, before it is dropped
                    pending.append(origin_mask_device(t, self.extents[i], self.footprint))
                lr.append(patches.down_pixel_aggr_device(t, self.scale, dt))
                if k == want - 1:
                    if class_masks[i] is not None:         # (after the down-sampling: the inputs see the raster as it was)
                        bits = masks_mod.valid_bits_device(class_masks[i], t.shape[:2], mask_classes, mask_dilate, device=self.device)
                        masks_mod.raster_apply_valid_device(t, bits)
                        if self.skip_masked:
                            blank = pending.pop() if self.skip_blank else None
                            pending.append(self._with_masked_cells(blank, bits, t.shape[:2], i))
                        del bits
                    elif self.skip_masked and not self.skip_blank:
                        blank = torch.zeros(mask_shapes(self.extents[i])[0], dtype=torch.uint8, device=self.device)
                        pending.append(origin_mask_device(blank, self.extents[i], self.footprint))
                    self.gt.append(t)
                    self.gt_dtypes.append(dt)
                del t
            self.lr.append(lr)
        self.cout = BANDS[want - 1]
        self._handle = ctypes.c_void_p(0)
        if masked_cells:                                   # (a nearly blank tile is refused before the handle is made)
            self.blank_cells = [cells for cells, _, _ in pending]
            self._blank_masks = _download_masks(pending)
            what = ' and '.join(w for w, on in (('blank', self.skip_blank), ('masked', self.skip_masked)) if on)
            for i, (n, (gh, gw)) in enumerate(zip(self._blank_masks[1], self.extents)):
                print('tile %d: %d of %d origins free of %s pixels' % (i, n, (gh - PATCH_LR + 1) * (gw - PATCH_LR + 1), what))
            check_origin_counts(self.extents, self._blank_masks[1])
        table = (_lib.CorpusTile * len(tiles))()
        for i, (lr, gt, dt, grid) in enumerate(zip(self.lr, self.gt, self.gt_dtypes, self.extents)):
            table[i] = _lib.CorpusTile(lr[0].data_ptr(), lr[1].data_ptr(), lr[2].data_ptr() if self.run_60 else None, gt.data_ptr(),
                                       grid[0], grid[1], _lib.DTYPE_U16 if dt == np.uint16 else _lib.DTYPE_F32)
        _lib.call('dsen2_corpus_create', table, len(tiles), int(self.run_60), ctypes.byref(self._handle))

    @staticmethod
    def _check_class_masks(class_masks, mask_classes, mask_dilate, n_tiles):
        """One 2-D uint8 raster or None per tile (None: no tile has one), after the refusals that need no GPU."""
        if class_masks is None:
            return [None] * n_tiles
        class_masks = list(class_masks)
        if len(class_masks) != n_tiles:
            raise ValueError('%d class masks for %d tiles (one raster or None per tile)' % (len(class_masks), n_tiles))
        for i, m in enumerate(class_masks):
            if m is None:
                continue
            if len(np.shape(m)) != 2 or m.dtype != (torch.uint8 if isinstance(m, torch.Tensor) else np.uint8):
                raise ValueError('tile %d: a class mask is a 2-D uint8 raster, got shape %r dtype %s' % (i, tuple(np.shape(m)), m.dtype))
        masks_mod.lut(mask_classes)
        if isinstance(mask_dilate, bool) or int(mask_dilate) != mask_dilate or not 0 <= mask_dilate <= masks_mod.MAX_DILATE:
            raise ValueError('mask_dilate is in ground-truth pixels, 0..%d, got %r' % (masks_mod.MAX_DILATE, mask_dilate))
        return class_masks

    def _with_masked_cells(self, blank, bits, gt_shape, i):
        """skip_masked: the (cells, bitmap, count) triple of tile i whose blank map — `blank`'s (skip_blank), or an empty one — has
        the cells that hold a pixel masked in `bits` OR-ed in (dsen2_cells_from_valid_bits, S = 2 or 6 ground-truth pixels per
        cell), handed to dsen2_corpus_origin_mask as DSEN2_MASK_BLANK_MAP."""
        grid = self.extents[i]
        cells = blank[0] if blank is not None else torch.zeros(mask_shapes(grid)[0], dtype=torch.uint8, device=self.device)
        masks_mod.cells_from_bits_device(bits, gt_shape, self.scale, cells=cells)
        return origin_mask_device(cells, grid, self.footprint)

    def origin_masks(self, holdout=None, margin=0):
        """([packed bitmap per tile], [valid origins per tile]) on the host: bit (oy, ox) of a tile's bitmap (mask_shapes;
        np.unpackbits(b, axis=1, bitorder='little')) is set when the crop at that origin touches no blank cell (skip_blank; without
        it nothing is blank) and no cell within `margin` cells of a hold-out crop.  holdout: int32 [k, 4] sample rows (tile, oy,
        ox, op), as validation_table returns them; every tile's cell map is then rebuilt on the device from its blank map and the
        rectangles of its rows.  A tile left with fewer than 1 valid origin in 64 is a ValueError (check_origin_counts)."""
        if holdout is None and self._blank_masks is not None:
            return list(self._blank_masks[0]), list(self._blank_masks[1])
        holdout = np.zeros((0, 4), np.int32) if holdout is None else self.check_table(holdout)
        if int(margin) < 0:
            raise ValueError('margin is in cells and cannot be negative, got %d' % margin)
        if holdout.shape[0] and (holdout[:, 0].min() < 0 or holdout[:, 0].max() >= len(self)):
            raise ValueError('a hold-out row names a tile outside the corpus of %d' % len(self))
        done = []
        for i, grid in enumerate(self.extents):
            blank = self.blank_cells[i] if self.blank_cells is not None else \
                torch.zeros(mask_shapes(grid)[0], dtype=torch.uint8, device=self.device)
            rows = np.ascontiguousarray(holdout[holdout[:, 0] == i, 1:3])
            done.append(origin_mask_device(blank, grid, self.footprint, rows, int(margin)))
        bitmaps, counts = _download_masks(done)
        check_origin_counts(self.extents, counts)
        return bitmaps, counts

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

    def validation_table(self, crops_per_tile, seed, masks=None):
        """The int32 [tiles * crops_per_tile, 4] sample table (tile, oy, ox, 0) of the validation crops: crops_per_tile fixed crops
        of every tile, drawn once, from a stream of their own (CorpusSampler.VAL_STREAM: the training draws of the same seed do
        not move), tile after tile — for each tile crops_per_tile row origins, then crops_per_tile column origins.
        masks (the blank-only bitmaps, origin_masks()[0]): after those draws, rows whose origin is not valid are redrawn by
        CorpusSampler's rule (ascending row order, rows then columns, until none is left).  The masks are fixed before any hold-out
        is formed: validation crops may overlap each other, never a blank cell.
        For fit_corpus's validation_crops, for origin_masks(holdout=), and what validation_arrays cuts."""
        CorpusSampler(self)                        # (refuses a tile without a range to draw from)
        extents = np.asarray(self.extents, np.int64).reshape(-1, 2)
        if masks is not None:
            masks = _check_masks(extents, masks)
        entropy = None if seed is None else [int(seed), CorpusSampler.VAL_STREAM]
        rng = np.random.default_rng(np.random.SeedSequence(entropy))
        m = int(crops_per_tile)
        table = np.zeros((len(self) * m, 4), np.int32)
        for i, (eh, ew) in enumerate(self.extents):
            table[i * m:(i + 1) * m, 0] = i
            table[i * m:(i + 1) * m, 1] = rng.integers(0, eh - PATCH_LR, size=m)
            table[i * m:(i + 1) * m, 2] = rng.integers(0, ew - PATCH_LR, size=m)
        if masks is not None:
            _redraw_invalid(rng, table, extents, masks)
        return table

    def validation_arrays(self, crops_per_tile, seed, chunk=256, masks=None):
        """Host arrays (xs, y) of the crops of validation_table(crops_per_tile, seed, masks), op 0, divided by SCALE, cut by the
        same kernel as the training batches.  For fit_corpus's validation_data.  Training crops may overlap them, as the reference's
        random crops overlap its validation patches, unless the sampler is given origin_masks(holdout=validation_table(...))."""
        return self.table_arrays(self.validation_table(crops_per_tile, seed, masks), chunk)

    def table_arrays(self, table, chunk=256):
        """Host arrays (xs, y) of the crops of the sample table `table` (op as given, divided by SCALE), cut on the device `chunk`
        rows at a time.  What validation_arrays returns for validation_table's rows: a caller that also needs the table — for
        origin_masks(holdout=) — draws it ONCE and cuts it here, so that the crops held out are the crops validated on."""
        table = self.check_table(table)
        x_shapes, y_shape = self.output_shapes(table.shape[0])
        xs = [np.empty(s, np.float32) for s in x_shapes]
        y = np.empty(y_shape, np.float32)
        for i0 in range(0, table.shape[0], chunk):
            dx, dy = self.batch(table[i0:i0 + chunk])
            for a, t in zip(xs + [y], dx + [dy]):
                a[i0:i0 + chunk] = t.cpu().numpy()
        if self.class_masked:                  # (the same bytes; fit then insists on mask_nodata, as fit_corpus does)
            y = y.view(training.MaskedTarget)
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
    in every process, whatever the images hold.

    masks (default None: the draws above, call for call): one packed origin bitmap per tile (TileCorpus.origin_masks()[0]).
    draw(n) first makes the draws above; then, while any sample's origin is not valid, the still-invalid sample indices in
    ascending order are redrawn: one integers call for their rows with the per-sample bounds, then one for their columns.  The
    tile of a sample is kept and the ops are not touched, so tiles stay UNIFORM over the corpus: a tile is not weighted by its
    valid area, and a half-blank tile gives as many crops as a full one, from half the ground.  The table is then a function of
    the seed, the extents, the masks and the sequence of n.  A tile with fewer than 1 valid origin in 64 is refused here
    (check_origin_counts), which bounds the expected number of rounds; after MAX_REDRAW_ROUNDS rounds draw raises RuntimeError
    (it takes valid origins that all lie on the last row or column, which is never drawn)."""
    STREAM = 0x636f7270          # 'corp'
    VAL_STREAM = 0x6376616c      # 'cval'

    def __init__(self, corpus, seed=None, augment=False, masks=None):
        extents = corpus.extents if hasattr(corpus, 'extents') else corpus
        self.extents = np.asarray([(int(h), int(w)) for h, w in extents], np.int64).reshape(-1, 2)
        if self.extents.shape[0] == 0 or (self.extents - PATCH_LR).min() <= 0:
            raise ValueError('origins are drawn below extent - %d: every tile needs an origin grid larger than %d x %d, got %r'
                             % (PATCH_LR, PATCH_LR, PATCH_LR, self.extents.tolist()))
        self.augment = bool(augment)
        self.masks = None if masks is None else _check_masks(self.extents, masks)
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
        if self.masks is not None:
            _redraw_invalid(self.rng, table, self.extents, self.masks)
        return table
