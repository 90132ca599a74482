"""Drop-in for the reference's testing/supres.py: same names, signatures, constants, prints and returns.

    from supres import DSen2_20, DSen2_60          (testing/s2_tiles_supres.py:9, testing/demoDSen2.py:5)

DSen2_20(d10, d20, deep=False)      -> [x, y, 6] float32     testing/supres.py:15-30
DSen2_60(d10, d20, d60, deep=False) -> [x, y, 2] float32     testing/supres.py:33-50
_predict(test, input_shape, deep=False, run_60=False)        testing/supres.py:53-66

The whole chain — symmetric pad + overlapped tiling, mirror-bilinear up-sampling, /2000, the CNN,
recomposition, *2000 — runs on one MI355X without touching the host between stages; with
torch.distributed initialised (one process per GPU, every rank called with the same arrays) the patches are
sharded across ranks, each rank uploads only the rows its patches read, and the inner crops of the predictions are
gathered to rank 0, which recomposes and returns the image; every other rank returns None (dsen2_amd/dist.py).  Models are cached per (device, architecture, weight file) instead of being rebuilt
and re-read on every call as the reference does (supres.py:59,63) — observable behaviour is unchanged.
"""
from __future__ import division

import contextlib
import functools
import inspect
import os

import numpy as np
import torch

from . import dist as _dist
from . import masks as _masks
from . import patches as _patches
from .DSen2Net import s2model

SCALE = 2000
MDL_PATH = '../models/'
# Not in the reference: arithmetic of the residual-block convolutions.  'fp32' (default, what keras computes),
# 'bf16' (bf16 operands, fp32 accumulate and residual stream; ~7x faster for deep=True, ~1e-3 relative error) or
# 'bf16x3' (every fp32 operand as two bf16 numbers, three bf16 MFMAs per product: ~1e-5 rmse in the normalised domain —
# inside the 1e-4 gate — at ~3x the fp32 rate).
PRECISION = os.environ.get('DSEN2_PRECISION', 'fp32')
# Not in the reference either: the geometric self-ensemble ("EDSR+").  On: every patch is predicted in its 8 flips and rotations,
# each prediction is turned back and the 8 are averaged (S2Model.forward_device_ensemble) — about 8 x the network time of a tile;
# tiling, up-sampling, recomposition and the sharding over ranks are untouched (the ensemble is per patch).  Default off.
SELF_ENSEMBLE = os.environ.get('DSEN2_SELF_ENSEMBLE', '0') not in ('', '0')
# Nor this: no-data in, no-data out.  On: a 10 m pixel whose bands are all exactly 0 (the sensor's fill value) comes back as 0 in
# every output band, and a patch that decides no pixel with data is never gathered, up-sampled, predicted, sent or read
# (csrc/nodata.hip); everywhere else the image is the one the option off returns, bit for bit.  Default off.
SKIP_NODATA = os.environ.get('DSEN2_SKIP_NODATA', '0') not in ('', '0')


def _env_int(name, default):
    v = os.environ.get(name, '')
    return int(v) if v.strip() else default


def _env_feather(v):
    v = v.strip().lower()
    if v in ('', '0', 'false', 'off', 'none'):
        return None
    return True if v in ('true', 'on', 'border') else int(v)


# Nor these: the overlap of neighbouring patches and what happens in it.  BORDER_20 / BORDER_60 replace the reference's 8 / 12
# pixels (testing/supres.py:22,41; a multiple of 2 / 6, at most a quarter of the patch of 128 / 192, which keeps its size: a wider
# border means more patches).  FEATHER: None = the reference's hard cut ("the last tile wins"); F in 1..border, or True = border,
# blends neighbouring predictions across F pixels either side of every seam (csrc/recompose_blend.hip).  The
# defaults are the reference's image, bit for bit.
BORDER_20 = _env_int('DSEN2_BORDER_20', 8)
BORDER_60 = _env_int('DSEN2_BORDER_60', 12)
FEATHER = _env_feather(os.environ.get('DSEN2_FEATHER', ''))

_MODEL_CACHE = {}
_LAST_RUN = {}


def last_run_stats():
    """{'patches': ..., 'kept': ..., 'skipped': ...} of the last DSen2_20 / DSen2_60 call of this process (a copy): the patches of
    the tile, those that were predicted and those SKIP_NODATA or a class mask (mask=) left out (always 0 with neither)."""
    return dict(_LAST_RUN)


def _weight_file(deep, run_60):
    # testing/supres.py:55-60
    if deep:
        return MDL_PATH + 's2_034_lr_1e-04.hdf5' if run_60 else MDL_PATH + 's2_033_lr_1e-04.hdf5'
    return MDL_PATH + 's2_030_lr_1e-05.hdf5' if run_60 else MDL_PATH + 's2_032_lr_1e-04.hdf5'


def _get_model(input_shape, deep, run_60):
    if deep:
        num_layers, feature_size = 32, 256      # supres.py:56
    else:
        num_layers, feature_size = 6, 128       # supres.py:59
    predict_file = _weight_file(deep, run_60)
    dev = _patches.default_device()
    # (under torch.distributed the ranks' MDL_PATH may differ — only rank 0's is read — so every rank keys its cache on its
    # own path string: all ranks hit or miss together as long as they make the same calls, which the collectives need anyway)
    key = (str(dev), tuple(s[0] for s in input_shape), num_layers, feature_size, os.path.abspath(predict_file), PRECISION)
    model = _MODEL_CACHE.get(key)
    if model is None:
        model = s2model(input_shape, num_layers=num_layers, feature_size=feature_size, device=dev, precision=PRECISION)
        print('Symbolic Model Created.')
        if _dist.rank_world()[1] > 1:
            # one process per GPU: rank 0 alone reads the checkpoint, one RCCL broadcast delivers it (C1, dsen2_amd/dist.py)
            # — the file need not exist on any other rank.  Collective: every rank
            # gets here on its first call for this architecture, all of them make the same calls.
            model.set_weights_flat(_dist.load_weights_on_root(predict_file, model.cin, model.cout, num_layers, feature_size,
                                                              device=dev))
        else:
            model.load_weights(predict_file)
        _MODEL_CACHE[key] = model
    else:
        print('Symbolic Model Created.')
    print("Predicting using file: {}".format(predict_file))
    return model


def clear_model_cache():
    _MODEL_CACHE.clear()


def _predict(test, input_shape, deep=False, run_60=False):
    """testing/supres.py:53-66 — list of NCHW float32 arrays in, [N, Cout, H, W] float32 array out."""
    model = _get_model(input_shape, deep, run_60)
    return model.predict(test, verbose=1, ensemble=True) if SELF_ENSEMBLE else model.predict(test, verbose=1)


def _row_slab(org_lr, scale, patch, border, height):
    """Rows [r0, r1) of one resolution's image that the patches with low-res origins `org_lr` read (the symmetric
    padding only ever reflects at the true image edges, which a slab touching them shares)."""
    rows = org_lr[:, 0].astype(np.int64) * scale
    r0 = max(0, int(rows.min()) - border)
    r1 = min(int(height), int(rows.max()) - border + patch)
    return r0, r1


class Shard(object):
    """What one rank computes: the network's inputs for the patches with low-res origins `my_org` (at least one).  Uploads
    only the rows those patches read (1/world of the tile; everything when there is one rank) and, once, the origins shifted
    into that slab: batch() only enqueues."""

    def __init__(self, dsets, scales, patch_sizes, borders, my_org, world, img10=None):
        dev = _patches.default_device()
        self.org, self.geom, self.imgs, self.org_dev = my_org, list(zip(scales, patch_sizes, borders)), [], []
        for k, (d, (s, ps, b)) in enumerate(zip(dsets, self.geom)):
            if k == 0 and img10 is not None:       # SKIP_NODATA: the whole 10 m raster is on the device already
                self.imgs.append(img10)
                self.org_dev.append(_patches.device_origins(my_org, s, dev))
                continue
            r0, r1 = _row_slab(my_org, s, ps, b, d.shape[0]) if world > 1 else (0, d.shape[0])
            self.imgs.append(_patches._to_device_f32(d[r0:r1], dev))
            self.org_dev.append(_patches.device_origins(my_org, s, dev, row0=r0))

    def batch(self, i0, n):
        """The inputs of patches [i0, i0 + n) of this shard, one [n, C, P, P] tensor per resolution."""
        patch, n_alloc = self.geom[0][1], self.org.shape[0]         # (n_alloc only sizes a gather without `count`)
        xs = []
        for k, (img, org_dev, (s, ps, b)) in enumerate(zip(self.imgs, self.org_dev, self.geom)):
            if k == 0:
                # `p10 /= SCALE` (supres.py:23) folded into the gather (IEEE divide, bit-identical)
                xs.append(_patches.gather_patches_device(img, self.org, s, b, ps, n_alloc, divisor=SCALE,
                                                         first=i0, count=n, origins_dev=org_dev))
            else:
                lr = _patches.gather_patches_device(img, self.org, s, b, ps, n_alloc, first=i0, count=n, origins_dev=org_dev)
                # up-sample raw values, then `/= SCALE` (supres.py:24,43-44)
                xs.append(_patches.interp_patches_device(lr, (patch, patch), post_divisor=SCALE))
        return xs


PINNED_OUTPUT_MIN_BYTES = 64 << 20     # DSEN2_PINNED_OUTPUT=0 disables; torch caches page-locked blocks for reuse


def _pinned_wanted(shape):
    return os.environ.get('DSEN2_PINNED_OUTPUT', '1') != '0' and 4 * shape[0] * shape[1] * shape[2] >= PINNED_OUTPUT_MIN_BYTES


def _pinned_empty(shape):
    return torch.empty(shape, dtype=torch.float32, pin_memory=True)


class RowSink(object):
    """How the image leaves the GPU, whoever computed its patches: rows() recomposes a band of rows that are final into the
    device image, finish() returns the image — through a page-locked buffer (57 GB/s instead of 11 GB/s from pageable memory)
    that is allocated only when the GPU work is enqueued, UNDER it (0.18 s for a 10980^2 x 6 image), or in one pageable
    download: small image, DSEN2_PINNED_OUTPUT=0, page-locked memory exhausted.

    Bands recomposed on the compute stream are marked with an event each, and finish() downloads them on a copy stream, every
    band as soon as its event has fired: under the batches still computing when the bands came in during the loop (a D2H takes
    5-40 % of its own time away from the kernels, profiles/r04_ablation.md §3).

    own_stream (the chunked gather): a stream that waits for what the current stream holds NOW — the image exists — and for
    nothing later, so that it may start on the first piece while the shard is still computing and the compute stream never
    waits for the collective's.  `with sink.tail():` — entered when the shard is enqueued — allocates the buffer and makes that
    stream current; every band is then downloaded right behind its recomposition and finish() only waits."""

    def __init__(self, shape, dev, own_stream=False, nodata=None):
        self.dev = dev
        self.nodata = nodata        # SKIP_NODATA: (slot map, bitmap) on the device; the patch buffers are then compact
        self.img = torch.empty(shape, dtype=torch.float32, device=dev)         # [H, W, cout]
        self.pinned = _pinned_wanted(shape)
        self.host, self.bands, self.stream = None, [], None
        if own_stream:
            self.stream = torch.cuda.Stream(dev)
            self.stream.wait_stream(torch.cuda.current_stream(dev))

    def _page_locked(self):
        if self.pinned:
            try:
                return _pinned_empty(tuple(self.img.shape))
            except RuntimeError:       # page-locked memory exhausted: the pageable path still works
                pass
        return None

    @contextlib.contextmanager
    def tail(self):
        self.host = self._page_locked()
        with torch.cuda.stream(self.stream):
            yield

    def rows(self, src_patches, border, r0, r1, feather=0):
        """Image rows [r0, r1) from the patch buffer (whole patches with their border, or inner crops with border 0: they tile
        alike, patches.py:380-403), on the current stream; `images *= SCALE` (supres.py:29) folded into the recomposition.
        feather > 0: the blend (whole patches with (border, feather), or crops of side inner + 2 * feather with (feather,
        feather): the same weights on the same values)."""
        slots, bits = self.nodata if self.nodata is not None else (None, None)
        _patches.recompose_rows_device(src_patches, border, self.img, r0, r1, scale=SCALE, slots=slots, valid_bits=bits,
                                       feather=feather)
        if self.stream is not None:
            if self.host is not None:
                self.host[r0:r1].copy_(self.img[r0:r1], non_blocking=True)
        elif self.pinned:
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(self.dev))
            self.bands.append((r0, r1, ev))

    def finish(self):
        """The image as an ndarray (a view of the page-locked tensor, which it keeps alive, where there is one)."""
        if self.stream is not None:
            self.stream.synchronize()
        else:
            self.host = self._page_locked()
            if self.host is not None:
                copy_stream = torch.cuda.Stream(self.dev)
                with torch.cuda.stream(copy_stream):
                    for r0, r1, ev in self.bands:
                        copy_stream.wait_event(ev)
                        self.host[r0:r1].copy_(self.img[r0:r1], non_blocking=True)
                copy_stream.synchronize()
        return self.host.numpy() if self.host is not None else self.img.cpu().numpy()


def _final_bands(slots_done, per, done_rows, size, inner, slot_of_patch=None, feather=0):
    """[(r0, r1)] image rows that became final now that the first `slots_done` slots of every shard of `per` patches are
    there (one rank: per = all patches, slots_done = patches computed so far); `done_rows` as in patches.final_row_runs.
    slot_of_patch (SKIP_NODATA): the shards hold the kept patches only, and an empty patch is final from the start.
    feather > 0: a row waits for every tile row that carries weight on it, and `done_rows` is per image row
    (patches.final_row_runs_blend)."""
    x_tiles, y_tiles = _patches.recompose_grid(size, inner, 0)
    if feather:
        if slot_of_patch is not None:
            return _patches.final_row_runs_slots_blend(slot_of_patch, slots_done, per, done_rows, size, inner, feather)
        return _patches.final_row_runs_blend(np.arange(x_tiles * y_tiles) % per < slots_done, done_rows, size, inner, feather)
    if slot_of_patch is not None:
        return _patches.final_row_runs_slots(slot_of_patch, slots_done, per, done_rows, size, inner)
    return _patches.final_row_runs(np.arange(x_tiles * y_tiles) % per < slots_done, done_rows, size, inner)


def _check_overlap(patch, ratio, border, feather):
    """(border, feather width) of a call, or ValueError: border a multiple of `ratio` (the patch origins lie on the lowest
    resolution's grid) in 1..patch/4, feather None / False / 0 (off), True (= border) or 1..border."""
    if isinstance(border, bool) or not isinstance(border, (int, np.integer)) or border % ratio or not 1 <= border <= patch // 4:
        raise ValueError('border must be a multiple of %d in %d..%d for patches of %d, got %r' % (ratio, ratio, patch // 4, patch, border))
    return int(border), _patches.feather_width(feather, int(border))


def _chunked_gather_wanted():
    return os.environ.get('DSEN2_CHUNKED_GATHER', '0') not in ('', '0')


def _gather_chunks():
    return max(1, int(os.environ.get('DSEN2_GATHER_CHUNKS', '8')))


def _nodata_plan(d10_dev, patch, border, used, size=None, mask=None, dev=None):
    """SKIP_NODATA: (kept patch indices, slot map on the host, (slot map, bitmap) on the device) of the uploaded 10 m raster.  The
    flags come to the host in ONE small read — the only synchronisation the option adds, before anything is enqueued.
    mask = (class raster, classes, dilate): the bitmap is the class mask's on the 10 m grid `size` (masks.valid_bits_device), ANDed
    with the no-data bitmap where d10_dev is given (None: the mask alone), and the flags are formed from THAT bitmap."""
    empty_dev = bits = None
    if d10_dev is not None:
        empty_dev, bits = _patches.nodata_device(d10_dev, patch, border)
        size, dev = tuple(d10_dev.shape[:2]), d10_dev.device
    if mask is not None:
        cls, classes, dilate = mask
        bits = _masks.valid_bits_device(cls, size, classes, dilate, and_bits=bits, device=dev, out=bits)
        empty_dev = _masks.tile_flags_device(bits, size, patch, border)
    empty = empty_dev.cpu().numpy()
    if empty.size != used:
        raise ValueError('the 10 m image of %r pixels has %d patches to recompose but the tiling of the lowest resolution has %d: '
                         'skip_nodata and mask need images in the exact size ratio' % (tuple(size[:2]), empty.size, used))
    kept, slot_of_patch = _patches.slot_map(empty)
    return kept, slot_of_patch, (torch.from_numpy(slot_of_patch).to(dev), bits)


def _check_mask(mask, classes, dilate, size):
    """(class raster, classes, dilate) of a call, or ValueError / TypeError before anything touches the GPU: a 2-D uint8 raster
    whose shape fits the 10 m grid `size` (masks.ratio), classes in 0..255 (None = masks.SCL_INVALID), dilate in 0..32."""
    shape = tuple(int(s) for s in np.shape(mask))
    if not isinstance(mask, torch.Tensor):
        mask = np.asarray(mask)
    if len(shape) != 2 or mask.dtype != (torch.uint8 if isinstance(mask, torch.Tensor) else np.uint8):
        raise ValueError('mask is a 2-D uint8 class raster, got shape %r dtype %s' % (shape, mask.dtype))
    _masks.ratio(shape, size[:2])
    classes = _masks.SCL_INVALID if classes is None else tuple(classes)
    _masks.lut(classes)
    if isinstance(dilate, bool) or not isinstance(dilate, (int, np.integer)) or not 0 <= dilate <= _masks.MAX_DILATE:
        raise ValueError('mask_dilate is in 10 m pixels, 0..%d, got %r' % (_masks.MAX_DILATE, dilate))
    return mask, classes, int(dilate)


def _run(dsets, scales, patch, border, deep, run_60, skip_nodata=None, feather=None, mask=None, mask_classes=None, mask_dilate=0):
    border, feather = _check_overlap(patch, scales[0], border, feather)            # before anything touches the GPU
    skip_nodata = SKIP_NODATA if skip_nodata is None else bool(skip_nodata)
    _patches.check_sizes(dsets, scales)
    if mask is not None:
        mask = _check_mask(mask, mask_classes, mask_dilate, dsets[0].shape)
    dev = _patches.default_device()
    rank, world = _dist.rank_world()
    patch_sizes = [patch // (scales[0] // s) for s in scales]          # P, P//2(, P//6)
    borders = [border // (scales[0] // s) for s in scales]             # b, b//2(, b//6)
    org, n_alloc = _patches.tile_origins(dsets[-1].shape, patch_sizes[-1], borders[-1])
    used = org.shape[0]
    model = _get_model(tuple((int(d.shape[2]), None, None) for d in dsets), deep, run_60)
    cout, size, inner = model.cout, dsets[0].shape, patch - 2 * border
    shape = (int(size[0]), int(size[1]), cout)
    single = n_alloc == 1            # recompose_images' single-patch shortcut (patches.py:375-376): a[0] uncropped
    _LAST_RUN.clear()
    _LAST_RUN.update(patches=used, kept=used, skipped=0)
    # SKIP_NODATA: the 10 m raster goes up once, whole, on every rank (it serves the flags, the gather and, through the bitmap, the
    # recomposition), every rank computes the same flags, and everything below — origins, `used`, the shard ranges, the buffers,
    # the gathers — works on the KEPT patches; slot_of_patch says where a patch of the grid lies among them.
    # mask: the class mask's bitmap, built on the device by every rank from the class raster itself (it is small), takes the place
    # of the no-data bitmap — or is ANDed with it — and everything after is the same run.
    img10 = slot_of_patch = nodata = None
    if mask is not None and single:
        raise ValueError('mask: the single-patch shortcut returns the %d x %d patch uncropped, not the %r image; a mask needs a tile of '
                         'more than one patch' % (patch, patch, tuple(size[:2])))
    if skip_nodata or mask is not None:
        if skip_nodata:
            img10 = _patches._to_device_f32(dsets[0], dev)
        if single:
            valid = (img10 != 0).any(dim=2)
            if tuple(valid.shape) != (patch, patch):
                raise ValueError('skip_nodata: the single-patch shortcut returns the %d x %d patch, not the %r image' % (patch, patch, tuple(valid.shape)))
            if not bool(valid.any()):
                _LAST_RUN.update(kept=0, skipped=1)
                return np.zeros((patch, patch, cout), np.float32) if rank == 0 else None
        else:
            kept, slot_of_patch, nodata = _nodata_plan(img10, patch, border, used, size=(int(size[0]), int(size[1])), mask=mask, dev=dev)
            _LAST_RUN.update(kept=int(kept.size), skipped=used - int(kept.size))
            org, used = org[kept], int(kept.size)
            if used == 0:            # nothing holds data: the zero image, no forward, no collective (every rank knows)
                if rank != 0:
                    return None
                print((cout, size[0], size[1]))                            # patches.py:392
                return np.zeros(shape, np.float32)
    # this rank's contiguous share of the USED patches (the reference's trailing all-zero patches are
    # never read by recompose_images, so they are not computed)
    first, count = _dist.shard_range(used)
    # what is already recomposed: per tile row, or, for the blend, per image row (_final_bands)
    done_rows = np.zeros(shape[0] if feather else _patches.recompose_grid(size, patch, border)[1], bool)
    # Where this rank's predictions go and who feeds the sink.  One rank (or the single patch): whole patches; a large image
    # leaves in bands, each right after the batch that completes its rows.  Several ranks: the inner crops (for the blend: the
    # crops of side inner + 2 * feather, everything that carries weight, recomposed with border = feather), in the [per, ...]
    # buffer the gather sends as it is (2.95 GB for a 10980^2 tile over all ranks instead of 3.85 GB of whole patches to EVERY
    # rank): one gather at the end, or, with DSEN2_CHUNKED_GATHER=1, DSEN2_GATHER_CHUNKS (8) pieces that travel while the
    # shards still compute (dist.ChunkedGather; off by default until an N > 1 box has measured RCCL's kernels
    # next to two CU-filling persistent ones).  The image is the same.
    pred = send = cg = sink = None
    crop, sent_border = border - feather, feather            # what a rank cuts off a prediction, and the border of what it sends
    banded, issued = False, 0
    if world == 1 or single:
        pred = torch.empty((count, cout, patch, patch), dtype=torch.float32, device=dev)
        banded = not single and _pinned_wanted(shape) and os.environ.get('DSEN2_BANDED_OUTPUT', '1') != '0'
    else:
        send = torch.empty((_dist.per_rank(used, world), cout, patch - 2 * crop, patch - 2 * crop), dtype=torch.float32, device=dev)
        if _chunked_gather_wanted():
            cg = _dist.ChunkedGather(send, used, _gather_chunks())
            if rank == 0:
                sink = RowSink(shape, dev, own_stream=True, nodata=nodata)     # BEFORE the loop: its stream waits for nothing later
    if count > 0:
        shard = Shard(dsets, scales, patch_sizes, borders, org[first:first + count], world, img10=img10)
        if banded:
            sink = RowSink(shape, dev, nodata=nodata)
        bs = model.preferred_batch(patch, patch, ensemble=True) if SELF_ENSEMBLE else model.preferred_batch(patch, patch)
        forward = model.forward_device_ensemble if SELF_ENSEMBLE else model.forward_device
        for i0 in range(0, count, bs):                                 # this loop only enqueues
            n = min(bs, count - i0)
            xs = shard.batch(i0, n)
            if send is None:
                forward(xs, out=pred[i0:i0 + n])
                if banded:
                    for r0, r1 in _final_bands(i0 + n, used, done_rows, size, inner, slot_of_patch, feather):
                        sink.rows(pred, border, r0, r1, feather)
            else:
                y = forward(xs)
                send[i0:i0 + n].copy_(y[:, :, crop:patch - crop, crop:patch - crop])
                # a piece whose slots this rank has all written (a short shard: all it will ever write) goes out now
                while cg is not None and issued < cg.n_chunks and i0 + n >= min(cg.bounds[issued][1], count):
                    cg.issue(issued)
                    issued += 1
    if single:
        if rank != 0:
            return None
        image = pred[0].permute(1, 2, 0).contiguous() * SCALE
        if skip_nodata:
            image = torch.where(valid[:, :, None], image, torch.zeros_like(image))
        return image.cpu().numpy()
    if cg is not None:
        # every rank issues every gather (a short or empty shard too); the send buffer stays alive until every piece has left
        for c in range(issued, cg.n_chunks):
            cg.issue(c)
        if rank != 0:
            for c in range(cg.n_chunks):
                cg.complete(c)
            return None
        print((cout, size[0], size[1]))                                # patches.py:392
        with sink.tail():
            for c in range(cg.n_chunks):
                cg.complete(c)                                         # this stream waits for gather c
                for r0, r1 in _final_bands(cg.slots_done(c), cg.per, done_rows, size, inner, slot_of_patch, feather):
                    sink.rows(cg.recv, sent_border, r0, r1, feather)
            assert done_rows.all()
            return sink.finish()
    if world > 1:
        # gather to root: rank 0 receives every rank's inner crops into views of one buffer; the other ranks return None —
        # no page-locked buffer, no download, nothing received
        pred, border = _dist.gather_to_root(send, used), sent_border
        if rank != 0:
            return None
    print((cout, size[0], size[1]))                                    # patches.py:392
    if sink is None:                 # not in bands: the whole image in one
        sink = RowSink(shape, dev, nodata=nodata)
        sink.rows(pred, border, 0, shape[0], feather)
    return sink.finish()


_EXTENSIONS = ('skip_nodata', 'border', 'feather', 'mask', 'mask_classes', 'mask_dilate')


def _reference_surface(fn):
    """fn(<the reference's parameters>, skip_nodata=None, border=None, feather=None, mask=None, mask_classes=None, mask_dilate=0) as
    the public function: this project's
    options (_EXTENSIONS) are taken BY KEYWORD ONLY, and inspect.signature() reports the reference's parameters alone
    (testing/supres.py:15,33) — callers and tools that bind or compare the drop-in surface by introspection see exactly the
    reference's."""
    sig = inspect.signature(fn)
    reference = sig.replace(parameters=[p for p in sig.parameters.values() if p.name not in _EXTENSIONS])

    defaults = dict((name, sig.parameters[name].default) for name in _EXTENSIONS)

    @functools.wraps(fn)
    def call(*args, **kwargs):
        ours = dict((name, kwargs.pop(name, default)) for name, default in defaults.items())
        bound = reference.bind(*args, **kwargs)           # TypeError for anything the reference's signature would refuse
        return fn(*bound.args, **ours, **bound.kwargs)
    call.__signature__ = reference
    return call


@_reference_surface
def DSen2_20(d10, d20, deep=False, skip_nodata=None, border=None, feather=None, mask=None, mask_classes=None, mask_dilate=0):
    """20 m -> 10 m.  d10 [x, y, 4] (B2 B3 B4 B8), d20 [x/2, y/2, 6] (B5 B6 B7 B8A B11 B12), any real dtype, HWC.
    deep=True selects VDSen2 (d=32, F=256).  Returns [x, y, 6] float32.  Geometry of testing/supres.py:21-22:
    patches of 128 with an 8-pixel border.

    With torch.distributed initialised (one process per GPU; every rank must make the same call with the same
    arrays — the call contains a collective) the patches are sharded over the ranks and ONLY RANK 0 returns the
    image; every other rank returns None.  The reference script's `if sr20 is None: exit` branch
    (testing/s2_tiles_supres.py:346-348) is what a non-root rank then takes.

    skip_nodata (keyword only, not in the reference and not part of the reported signature; None = supres.SKIP_NODATA): a pixel of d10 whose bands are all exactly 0 is returned
    as 0 in every band, and patches that decide no pixel with data are not computed; all other pixels are unchanged, bit for bit.

    border, feather (keyword only too; None = supres.BORDER_20 / BORDER_60 and supres.FEATHER): the overlap of neighbouring patches
    in 10 m pixels (a multiple of 2 / 6, at most 32 / 48; the patch keeps its size, so a wider border means more patches) and
    the width of the blend either side of every seam (1..border, True = border; None, False or 0 = the reference's hard cut).
    ValueError for anything else, before the GPU is touched.

    mask, mask_classes, mask_dilate (keyword only too): a 2-D uint8 class raster on the 10, 20 or 60 m grid of the tile (Sentinel-2's
    SCL layer, a cloud-probability layer, ...; dsen2_amd/masks.py), the class values that make a pixel invalid (None =
    masks.SCL_INVALID) and a dilation of the invalid area in 10 m pixels (0..32).  An invalid pixel is returned as 0 in every band and
    a patch that decides no valid pixel is not computed, exactly as skip_nodata treats no-data (the two compose: their bitmaps are
    ANDed); every other pixel is what the call without a mask returns, bit for bit (under feather: every pixel further than the
    feather width from a skipped patch; nearer, the patches that are left are blended).  A tile of one patch refuses a mask."""
    return _run([d10, d20], [2, 1], patch=128, border=BORDER_20 if border is None else border, deep=deep, run_60=False,
                skip_nodata=skip_nodata, feather=FEATHER if feather is None else feather, mask=mask, mask_classes=mask_classes,
                mask_dilate=mask_dilate)


@_reference_surface
def DSen2_60(d10, d20, d60, deep=False, skip_nodata=None, border=None, feather=None, mask=None, mask_classes=None, mask_dilate=0):
    """60 m -> 10 m.  As DSen2_20 plus d60 [x/6, y/6, 2] (B1 B9; B10 is not super-resolved).  Returns [x, y, 2]
    float32.  Geometry of testing/supres.py:40-41: patches of 192 with a 12-pixel border.  Under torch.distributed: the
    image on rank 0, None on every other rank (see DSen2_20).  skip_nodata, border, feather, mask, mask_classes, mask_dilate: as
    DSen2_20."""
    return _run([d10, d20, d60], [6, 3, 1], patch=192, border=BORDER_60 if border is None else border, deep=deep, run_60=True,
                skip_nodata=skip_nodata, feather=FEATHER if feather is None else feather, mask=mask, mask_classes=mask_classes,
                mask_dilate=mask_dilate)
