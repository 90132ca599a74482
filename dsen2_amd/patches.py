"""Host-side mirror of the reference's utils/patches.py, running on the GPU.

Same function names, arguments, defaults, return types and quirks as the reference:
  interp_patches(image_20, image_10_shape)                              utils/patches.py:11-16
  get_test_patches(dset_10, dset_20, patchSize=128, border=4, interp)   utils/patches.py:19-80
  get_test_patches60(dset_10, dset_20, dset_60, patchSize=128, border=8, interp)   :83-156
  recompose_images(a, border, size=None)                                utils/patches.py:374-405  (+ feather=)
and of its training-set half (python -m dsen2_amd.create_patches):
  downPixelAggr(img, SCALE=2)                                           utils/patches.py:353-371
  save_test_patches / save_test_patches60(..., file, ...)               utils/patches.py:159-178
  save_random_patches / save_random_patches60(..., file, NR_CROP)       utils/patches.py:181-271  (+ seed=, origins=)
and of what the evaluation step (python -m dsen2_amd.train --predict) reads back:
  OpenDataFilesTest(path, run_60, SCALE, true_scale=False)              utils/patches.py:327-350
numpy in, numpy out; the ``*_device`` variants keep everything in HBM (torch CUDA tensors) so that
supres.DSen2_20/60 never bounce patches through the host.  The gathers, the mirror-bilinear
up-sampling and the recomposition are HIP kernels behind the C ABI (include/dsen2_hip.h); only the
O(#patches) origin arithmetic runs on the host.
"""
import ctypes
import inspect
import json
import random
from math import ceil

import numpy as np
import torch

from . import _lib


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _stream(device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def default_device():
    if not torch.cuda.is_available():
        raise RuntimeError('dsen2_amd needs a ROCm GPU (gfx950); there is no CPU fallback')
    return torch.device('cuda', torch.cuda.current_device())


def _storage_plan(a):
    """How a non-C-contiguous ndarray can be uploaded WITHOUT a strided pass over it on the host.

    The reference's own callers hand over views: `np.rollaxis(ds.ReadAsArray(...), 0, 3)` (testing/s2_tiles_supres.py: an HWC
    view of a CHW array), `f['im10'][()].transpose()` (testing/demoDSen2.py:16: Fortran order), and under torch.distributed a
    row slab `d[r0:r1]` of either.  numpy needs seconds to make a 10980^2 x 4 view of that kind C-contiguous — longer than the
    GPU needs for the whole tile in the bf16 modes — while the storage underneath is contiguous as it is.  Returns
    (order, mode): `a.transpose(order)` lists the axes by decreasing stride; mode 'whole' = that array is C-contiguous (one
    copy), 'planes' = each `a.transpose(order)[k]` is (a row slab of a plane-major array: one copy per plane), None = neither
    (the caller falls back to np.ascontiguousarray)."""
    if a.ndim < 2 or a.size == 0 or any(st <= 0 for st in a.strides):
        return None, None
    order = tuple(int(i) for i in np.argsort([-st for st in a.strides], kind='stable'))
    base = a.transpose(order)
    if base.flags.c_contiguous:
        return order, 'whole'
    if base.shape[0] <= 64 and base[0].flags.c_contiguous:
        return order, 'planes'
    return None, None


_TORCH_BITS = {np.uint16: torch.int16, np.int16: torch.int16, np.uint8: torch.uint8, np.int8: torch.int8, np.int32: torch.int32,
               np.int64: torch.int64, np.float32: torch.float32, np.float64: torch.float64}


def _widen(t, np_dtype):
    """The uploaded integer tensor (uint16 travels as int16 bits) -> float32, on the GPU."""
    if np_dtype == np.uint16:
        return (t.to(torch.int32) & 0xFFFF).to(torch.float32)
    return t.to(torch.float32)


def _to_device_f32(a, device):
    """Any real array -> contiguous float32 CUDA tensor (the reference's float32 patch arrays take any dtype).
    Integer rasters (Sentinel-2 L1C is uint16) are uploaded as they are and widened on the GPU: half the PCIe
    bytes and no host-side conversion pass (0.15 s of a 10980^2 tile).  Views whose storage is contiguous in another axis
    order (_storage_plan) are uploaded in THAT order and permuted on the GPU."""
    if isinstance(a, torch.Tensor):
        return a.to(device=device, dtype=torch.float32).contiguous()
    a = np.asarray(a)
    direct = a.dtype.type in _TORCH_BITS and a.dtype.isnative
    if direct and not a.flags.c_contiguous:
        order, mode = _storage_plan(a)
        if mode is not None:
            base = a.transpose(order)
            if not base.flags.writeable:
                base = None if mode == 'whole' else base       # (read-only maps: the plane copies below make their own arrays)
            if base is not None:
                as_bits = (lambda x: x.view(np.int16)) if a.dtype == np.uint16 else (lambda x: x)
                if mode == 'whole':
                    t = torch.from_numpy(as_bits(base)).to(device)
                else:
                    t = torch.empty(base.shape, dtype=_TORCH_BITS[a.dtype.type], device=device)
                    for k in range(base.shape[0]):
                        plane = base[k] if base[k].flags.writeable else np.array(base[k])
                        t[k].copy_(torch.from_numpy(as_bits(plane)))
                inverse = [order.index(i) for i in range(a.ndim)]
                # permuted at the storage width (2 B for a Sentinel-2 raster), widened after
                return _widen(t.permute(*inverse).contiguous(), a.dtype)
    a = np.ascontiguousarray(a)
    if not a.flags.writeable:
        a = np.array(a)           # a read-only memory map (cli._load under torch.distributed): copy the slab, not a view torch would warn about
    if a.dtype == np.uint16:
        return _widen(torch.from_numpy(a.view(np.int16)).to(device), np.uint16)
    if direct:
        # converted on the GPU with the same round-to-nearest as numpy's cast into the reference's float32 patch arrays (a
        # float64 raster: twice the PCIe bytes, but no pass over it on the host)
        return torch.from_numpy(a).to(device).to(torch.float32)
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(device)


# ---- interp_patches ---------------------------------------------------------------------------
def interp_patches_device(image_lr, hr_hw, post_divisor=1.0, ref=False):
    """[N,C,h,w] float32 CUDA tensor -> [N,C,H,W]; optionally folds the later ``/= SCALE``.  ref=True: the general
    kernel whatever the scale (dsen2_upsample_mirror_bilinear_ref, kernel-level cross-check)."""
    n, c, h, w = image_lr.shape
    oh, ow = int(hr_hw[0]), int(hr_hw[1])
    out = torch.empty((n, c, oh, ow), dtype=torch.float32, device=image_lr.device)
    with torch.cuda.device(image_lr.device):
        _lib.call('dsen2_upsample_mirror_bilinear_ref' if ref else 'dsen2_upsample_mirror_bilinear', _ptr(image_lr), _ptr(out), n * c, h, w, oh, ow,
                  float(post_divisor), _stream(image_lr.device))
    return out


def interp_patches(image_20, image_10_shape):
    """utils/patches.py:11-16 — bilinear (order 1) resize with mirror boundary, per patch and band."""
    dev = default_device()
    x = _to_device_f32(image_20, dev)
    return interp_patches_device(x, image_10_shape[2:4]).cpu().numpy()


# ---- tiling -----------------------------------------------------------------------------------
def _axis_origins(extent, patch, border):
    """Patch origins (padded low-res coordinates) along one axis: patches.py:45-53 / :114-122."""
    stride = patch - 2 * border
    if stride <= 0:
        raise ValueError('border %d leaves no interior in a patch of %d' % (border, patch))
    if extent + 2 * border < patch:
        # the reference would index with a negative origin here and fail on a shape mismatch
        raise ValueError('image extent %d (+2*%d border) is smaller than one patch of %d' % (extent, border, patch))
    k = extent // stride
    starts = [i * stride for i in range(k)]
    if extent % stride != 0:
        starts.append(extent + 2 * border - patch)      # = padded_extent - patch
    return starts, k


def tile_origins(lr_shape, patch_lr, border_lr):
    """(origins [used,2] int32 in padded LR coordinates (row-major: i outer, j inner), n_alloc).

    n_alloc = (k_i+1)*(k_j+1) is what the reference allocates (patches.py:35/:103); when the stride
    divides an extent only ``used`` < n_alloc patches are filled and the rest stay zero.
    """
    si, ki = _axis_origins(int(lr_shape[0]), patch_lr, border_lr)
    sj, kj = _axis_origins(int(lr_shape[1]), patch_lr, border_lr)
    org = np.array([(i, j) for i in si for j in sj], dtype=np.int32).reshape(-1, 2)
    return org, (ki + 1) * (kj + 1)


def gather_patches_device(img_dev, origins_lr, scale, border, patch, n_alloc, divisor=1.0, first=0, count=None,
                          origins_dev=None):
    """Crop patches [first, first+count) of one resolution from the (virtually symmetric-padded) image.

    img_dev: [H,W,C] float32 CUDA tensor; origins_lr: int32 [used,2] in padded low-res coordinates;
    ``scale`` = resolution ratio to the low-res grid (crop origin and size multiply by it,
    patches.py:67 / :136-137).  Returns [count_or_alloc, C, patch, patch]; rows beyond the used
    patches are zero as in the reference.  ``origins_dev``: the same origins already multiplied by ``scale`` as an
    int32 [used,2] tensor on the device (``device_origins``) — callers that loop over batches pass it so that no
    call uploads anything (a pageable host-to-device copy blocks the host until the stream has drained).
    """
    H, W, C = img_dev.shape
    used = origins_lr.shape[0]
    if count is None:
        first, count, n_out = 0, used, n_alloc
    else:
        n_out = count
    out = torch.empty((n_out, C, patch, patch), dtype=torch.float32, device=img_dev.device)
    if n_out > count:
        out[count:].zero_()          # the reference's trailing never-filled patches (patches.py:35)
    if count > 0:
        if origins_dev is not None:
            org = origins_dev[first:first + count]
        else:
            org = device_origins(origins_lr[first:first + count], scale, img_dev.device)
        with torch.cuda.device(img_dev.device):
            _lib.call('dsen2_tile_gather', _ptr(img_dev), H, W, C, border, _ptr(org), count, patch, float(divisor),
                      _ptr(out), _stream(img_dev.device))
    return out


def device_origins(origins_lr, scale, device, row0=0):
    """int32 [n,2] crop origins at one resolution (low-res origins x scale) as a device tensor; `row0`: the image row the
    uploaded slab starts at (the origins are shifted into it)."""
    org = np.ascontiguousarray(origins_lr * scale, dtype=np.int32)
    org[:, 0] -= row0
    return torch.from_numpy(org).to(device)


def check_sizes(dsets, scales, lowest='lowest'):
    """The reference fails with a broadcasting ValueError when the images do not have the 10 m : 20 m (: 60 m) size ratio its
    crop arithmetic assumes (patches.py:67, :136-137); say so before anything reaches the GPU.  dsets[-1] is the
    lowest-resolution image, scales[i] the ratio of dsets[i] to it."""
    lo = dsets[-1].shape
    for d, s in zip(dsets, scales):
        if len(d.shape) != 3:
            raise ValueError('expected HWC images, got shape %r' % (tuple(d.shape),))
        if d.shape[0] < s * lo[0] or d.shape[1] < s * lo[1]:
            raise ValueError('image of shape %r does not cover %d x the %s-resolution image %r'
                             % (tuple(d.shape), s, lowest, tuple(lo)))


def get_test_patches(dset_10, dset_20, patchSize=128, border=4, interp=True):
    """utils/patches.py:19-80.  Returns (image_10 [N,B10,P,P], data20 [N,B20,P,P]) float32 ndarrays."""
    check_sizes([dset_10, dset_20], [2, 1], 'lower')
    dev = default_device()
    p_lr, b_lr = patchSize // 2, border // 2
    d10, d20 = _to_device_f32(dset_10, dev), _to_device_f32(dset_20, dev)
    org, n_alloc = tile_origins(d20.shape, p_lr, b_lr)
    image_10 = gather_patches_device(d10, org, 2, border, patchSize, n_alloc)
    image_20 = gather_patches_device(d20, org, 1, b_lr, p_lr, n_alloc)
    data20 = interp_patches_device(image_20, image_10.shape[2:4]) if interp else image_20
    return image_10.cpu().numpy(), data20.cpu().numpy()


def get_test_patches60(dset_10, dset_20, dset_60, patchSize=128, border=8, interp=True):
    """utils/patches.py:83-156.  Returns (image_10, data20, data60) float32 ndarrays."""
    check_sizes([dset_10, dset_20, dset_60], [6, 3, 1], 'lower')
    dev = default_device()
    p20, p60 = patchSize // 2, patchSize // 6
    b20, b60 = border // 2, border // 6
    d10, d20, d60 = (_to_device_f32(a, dev) for a in (dset_10, dset_20, dset_60))
    org, n_alloc = tile_origins(d60.shape, p60, b60)
    image_10 = gather_patches_device(d10, org, 6, border, patchSize, n_alloc)
    image_20 = gather_patches_device(d20, org, 3, b20, p20, n_alloc)
    image_60 = gather_patches_device(d60, org, 1, b60, p60, n_alloc)
    if interp:
        image_20 = interp_patches_device(image_20, image_10.shape[2:4])
        image_60 = interp_patches_device(image_60, image_10.shape[2:4])
    return image_10.cpu().numpy(), image_20.cpu().numpy(), image_60.cpu().numpy()


# ---- recomposition ----------------------------------------------------------------------------
def recompose_grid(size, patch, border):
    inner = patch - 2 * border
    return int(ceil(size[1] / float(inner))), int(ceil(size[0] / float(inner)))    # x_tiles, y_tiles


def final_row_runs(have, done_rows, size, inner):
    """Which image rows can be recomposed now.  `have`: bool per patch (row-major patch index, x_tiles * y_tiles of them) —
    the patches that are final; `done_rows`: bool per TILE ROW, rows already recomposed (updated in place).  A tile row is
    ready when all its patches are; tile row ty decides image rows [ty * inner, min((ty + 1) * inner, H - inner)), the last
    one [H - inner, H) (its start is clamped, patches.py:396-401, and it overwrites what the row before it put there).
    Returns merged [(row0, row1)] runs in ascending order."""
    H = int(size[0])
    x_tiles, y_tiles = recompose_grid(size, inner, 0)
    ready = np.asarray(have[:x_tiles * y_tiles], bool).reshape(y_tiles, x_tiles).all(axis=1) & ~done_rows
    runs = []
    for ty in np.nonzero(ready)[0]:
        r0, r1 = (H - inner, H) if ty == y_tiles - 1 else (int(ty) * inner, min((int(ty) + 1) * inner, H - inner))
        if runs and runs[-1][1] == r0:
            runs[-1] = (runs[-1][0], r1)
        else:
            runs.append((r0, r1))
        done_rows[ty] = True
    return runs


def final_row_runs_slots(slot_of_patch, slots_done, per, done_rows, size, inner):
    """final_row_runs for a compact patch buffer (`slot_map`): patch k is final when it is empty (slot -1: nothing will ever be
    computed for it) or when its slot is among the first `slots_done` of its shard of `per` slots (one rank: per = all kept
    patches)."""
    slot = np.asarray(slot_of_patch)
    have = slot < 0
    if per > 0:
        have = have | ((slot >= 0) & (slot % per < slots_done))
    return final_row_runs(have, done_rows, size, inner)


# ---- feathered blend (not in the reference; csrc/recompose_blend.hip) -----------------------------
def feather_width(feather, border):
    """The `feather` argument of the recomposition as an int: None, False or 0 -> 0 (the reference's hard cut), True -> border,
    an int in 1..border -> itself; ValueError for anything else."""
    if feather is None or feather is False or (not isinstance(feather, bool) and isinstance(feather, (int, np.integer)) and feather == 0):
        return 0
    if feather is True:
        feather = border
    if not isinstance(feather, (int, np.integer)) or not 1 <= feather <= border:
        raise ValueError('feather must be None, a bool or an int in 1..border = 1..%d, got %r' % (border, feather))
    return int(feather)


def blend_row_support(ty, size, inner, feather):
    """Image rows [r0, r1) on which tile row ty carries weight in the blend: [s - feather, s + inner + feather) cut to the image,
    s = ty * inner, the last tile row's start clamped to H - inner (include/dsen2_hip.h, "feathered recomposition")."""
    H = int(size[0])
    y_tiles = recompose_grid(size, inner, 0)[1]
    s = H - inner if ty == y_tiles - 1 else int(ty) * inner
    return max(0, s - feather), min(H, s + inner + feather)


def final_row_runs_blend(have, done_rows, size, inner, feather):
    """final_row_runs for the blend: an image row is final once EVERY tile row whose support (blend_row_support) holds it is
    complete.  `have` as in final_row_runs; `done_rows`: bool per IMAGE ROW, rows already recomposed (updated in place).  Returns
    merged [(row0, row1)] runs in ascending order."""
    H = int(size[0])
    x_tiles, y_tiles = recompose_grid(size, inner, 0)
    complete = np.asarray(have[:x_tiles * y_tiles], bool).reshape(y_tiles, x_tiles).all(axis=1)
    final = ~done_rows
    for ty in np.nonzero(~complete)[0]:
        r0, r1 = blend_row_support(int(ty), size, inner, feather)
        final[r0:r1] = False
    edges = np.flatnonzero(np.diff(np.concatenate(([0], final.astype(np.int8), [0]))))
    done_rows |= final
    return [(int(a), int(b)) for a, b in zip(edges[0::2], edges[1::2])]


def final_row_runs_slots_blend(slot_of_patch, slots_done, per, done_rows, size, inner, feather):
    """final_row_runs_slots for the blend (`done_rows` per image row): a patch without a slot carries no weight and is final from
    the start."""
    slot = np.asarray(slot_of_patch)
    have = slot < 0
    if per > 0:
        have = have | ((slot >= 0) & (slot % per < slots_done))
    return final_row_runs_blend(have, done_rows, size, inner, feather)


# ---- no-data (not in the reference; csrc/nodata.hip) ---------------------------------------------
def nodata_geometry(size, patch, border):
    """(x_tiles, y_tiles, bitmap_words) of dsen2_tile_nodata_geometry: host only; DSen2Error for a geometry the recomposition
    refuses."""
    xt, yt, words = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_size_t(0)
    _lib.call('dsen2_tile_nodata_geometry', int(size[0]), int(size[1]), int(patch), int(border), ctypes.byref(xt), ctypes.byref(yt),
              ctypes.byref(words))
    return xt.value, yt.value, words.value


def nodata_device(img10_dev, patch, border):
    """[H,W,C10] float32 CUDA tensor -> (patch_empty uint8 [y_tiles * x_tiles], valid_bits int32 [H, ceil(W / 32)]), both on the
    device (dsen2_tile_nodata): a pixel holds data unless all its bands are exactly 0; a patch is empty when the rectangle of the
    image that recompose_images takes from it holds no data.  Enqueues only."""
    H, W, C = img10_dev.shape
    xt, yt, words = nodata_geometry((H, W), patch, border)
    if not 1 <= C <= 16:
        raise ValueError('no-data detection takes 1..16 bands, got %d' % C)
    dev = img10_dev.device
    empty = torch.empty(xt * yt, dtype=torch.uint8, device=dev)
    bits = torch.empty((H, words // H), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.call('dsen2_tile_nodata', _ptr(img10_dev), H, W, C, int(patch), int(border), _ptr(empty), _ptr(bits), _stream(dev))
    return empty, bits


def slot_map(patch_empty):
    """Host side, numpy: (kept, slot_of_patch) — the indices of the patches that are not empty, ascending, and the int32 map
    patch index -> position in that list, -1 for an empty patch."""
    empty = np.asarray(patch_empty).reshape(-1) != 0
    kept = np.nonzero(~empty)[0].astype(np.int64)
    slot_of_patch = np.full(empty.size, -1, np.int32)
    slot_of_patch[kept] = np.arange(kept.size, dtype=np.int32)
    return kept, slot_of_patch


def recompose_device(a_dev, border, size, scale=1.0, feather=None):
    """[N,C,P,P] CUDA tensor -> [size0,size1,C] CUDA tensor (N > 1).  feather: see recompose_rows_device."""
    n, c, p, _ = a_dev.shape
    H, W = int(size[0]), int(size[1])
    img = torch.empty((H, W, c), dtype=torch.float32, device=a_dev.device)
    if feather_width(feather, border):
        recompose_rows_device(a_dev, border, img, 0, H, scale=scale, feather=feather)
        return img
    with torch.cuda.device(a_dev.device):
        _lib.call('dsen2_recompose', _ptr(a_dev), n, c, p, border, _ptr(img), H, W, float(scale),
                  _stream(a_dev.device))
    return img


def recompose_rows_device(a_dev, border, img, row0, row1, scale=1.0, slots=None, valid_bits=None, feather=None):
    """Rows [row0, row1) of `img` ([H,W,C] CUDA tensor) from the patch buffer a_dev [N,C,P,P] (dsen2_recompose_rows): only the
    patches those rows read need to be final.  slots (int32 device tensor, patch index -> index in a_dev or -1: `slot_map`) and
    valid_bits (`nodata_device`), given together: a_dev is the compact buffer of the kept patches, and a pixel without data, or
    whose patch has no slot in a_dev, becomes 0 (dsen2_recompose_rows_nodata).  feather (None, False or 0: the hard cut; True:
    border; 1..border): the patches are blended across `feather` pixels either side of every seam instead
    (dsen2_recompose_rows_blend), with or without the two maps."""
    n, c, p, _ = a_dev.shape
    H, W = int(img.shape[0]), int(img.shape[1])
    feather = feather_width(feather, border)
    if (slots is None) != (valid_bits is None):
        raise ValueError('slots and valid_bits go together')
    if slots is not None:
        if slots.dtype != torch.int32 or valid_bits.dtype != torch.int32 or not slots.is_contiguous() or not valid_bits.is_contiguous():
            raise TypeError('slots and valid_bits are contiguous int32 tensors')
        xt, yt, words = nodata_geometry((H, W), p, border)
        if slots.numel() != xt * yt or valid_bits.numel() != words:
            raise ValueError('slot map of %d entries and bitmap of %d words for a %d x %d grid and %d words'
                             % (slots.numel(), valid_bits.numel(), yt, xt, words))
    if (slots is not None or feather) and int(img.shape[2]) != c:
        raise ValueError('image of %d channels for patches of %d' % (int(img.shape[2]), c))
    if feather:
        with torch.cuda.device(img.device):
            _lib.call('dsen2_recompose_rows_blend', _ptr(a_dev) if n else None, n, c, p, border, feather,
                      _ptr(slots) if slots is not None else None, _ptr(valid_bits) if slots is not None else None, _ptr(img), H, W,
                      float(scale), int(row0), int(row1), _stream(img.device))
        return
    if slots is not None:
        with torch.cuda.device(img.device):
            _lib.call('dsen2_recompose_rows_nodata', _ptr(a_dev) if n else None, n, c, p, border, _ptr(slots), _ptr(valid_bits),
                      _ptr(img), H, W, float(scale), int(row0), int(row1), _stream(img.device))
        return
    with torch.cuda.device(a_dev.device):
        _lib.call('dsen2_recompose_rows', _ptr(a_dev), n, c, p, border, _ptr(img), H, W, float(scale), int(row0), int(row1),
                  _stream(a_dev.device))


def recompose_images(a, border, size=None, *, feather=None):
    """utils/patches.py:374-405 — including the single-patch shortcut (:375-376) and the shape print (:392).  feather (keyword
    only, not in the reference and not part of the reported signature; see recompose_rows_device): a blend across the seams
    instead of the hard cut; the single-patch shortcut stays."""
    if a.shape[0] == 1:
        images = np.asarray(a[0]) if not isinstance(a, torch.Tensor) else a[0].cpu().numpy()
        return images.transpose((1, 2, 0))
    feather_width(feather, border)              # a bad value is refused before anything reaches the GPU
    dev = default_device()
    x = _to_device_f32(a, dev)
    print((a.shape[1], size[0], size[1]))
    return recompose_device(x, border, size, feather=feather).cpu().numpy()


# inspect.signature() reports the reference's parameters alone, as for supres.DSen2_20 / DSen2_60
recompose_images.__signature__ = inspect.Signature([p for p in inspect.signature(recompose_images).parameters.values()
                                                    if p.name != 'feather'])


# ---- training-set creation (utils/patches.py:159-271, :353-371) --------------------------------
# numpy's exp is not one function: an AVX-512 kernel in some builds, libm in others, and exp(-2) differs in its last bit between
# them — and with it w.sum() and the centre weight.  A drop-in must not depend on that, so the two scales of the DSen2 protocol are
# pinned to what the reference's stack computes (scipy 1.7.1 on numpy 1.26.4, AVX-512; tests/golden/make_golden_trainset.py
# asserts it there and records them); any other scale evaluates the same formula with the numpy at hand.
_REFERENCE_WEIGHTS = {
    2: ('0x1.14aebe6a24088p-12', '0x1.b405b9842b206p-4', '0x1.92b965ef5aaefp-1', '0x1.b405b9842b206p-4', '0x1.14aebe6a24088p-12'),
    6: ('0x1.05a62840e3dcep-26', '0x1.fffffefa59d7cp-1', '0x1.05a62840e3dcep-26'),
}


def gaussian_weights(scale):
    """(weights float64 [2 * radius + 1], radius): what scipy.ndimage.gaussian_filter1d(sigma=1/scale, truncate=4.0) builds
    (scipy/ndimage/filters.py, _gaussian_kernel1d) — float64 on the host, so that the kernel never evaluates exp."""
    sigma = 1.0 / scale
    radius = int(4.0 * sigma + 0.5)
    if scale in _REFERENCE_WEIGHTS:
        return np.array([float.fromhex(v) for v in _REFERENCE_WEIGHTS[scale]]), radius
    x = np.arange(-radius, radius + 1)
    w = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    return w / w.sum(), radius


def _check_divisible(h, w, scale):
    # the reference fails here too: block_reduce pads to a multiple of SCALE while new_dims floors (ValueError on assignment)
    if scale < 1 or h % scale or w % scale:
        raise ValueError('downPixelAggr: image of %d x %d pixels is not a multiple of SCALE = %d' % (h, w, scale))


def _down(img_dev, np_dtype, scale, out_dtype):
    h, w, c = img_dev.shape
    _check_divisible(h, w, scale)
    weights, radius = gaussian_weights(scale)
    if radius > min(h, w):
        raise ValueError('downPixelAggr: image of %d x %d pixels is smaller than the filter radius %d' % (h, w, radius))
    out = torch.empty((h // scale, w // scale, c), dtype=out_dtype, device=img_dev.device)
    if out.numel() == 0:
        return out
    host_w = (ctypes.c_double * len(weights))(*weights)
    with torch.cuda.device(img_dev.device):
        _lib.call('dsen2_down_pixel_aggr', _ptr(img_dev), _lib.DTYPE_U16 if np_dtype == np.uint16 else _lib.DTYPE_F32, h, w, c,
                  int(scale), host_w, radius, _ptr(out), 1 if out_dtype == torch.float64 else 0, _stream(img_dev.device))
    return out


def upload_raster(img, device=None):
    """A host raster -> (device tensor, numpy dtype) IN ITS OWN DTYPE: uint16 travels as its bits in an int16 tensor and is never
    widened (downPixelAggr truncates to uint16 after each filter axis: the float32 path gives other numbers), float32 as it is.
    Any other dtype is refused: the reference would filter it in that dtype, and only these two have a kernel."""
    device = device or default_device()
    a = np.asarray(img)
    if a.dtype not in (np.uint16, np.float32):
        raise TypeError('downPixelAggr on the GPU takes uint16 or float32 rasters, not %s (the reference filters in the input\'s '
                        'dtype: cast explicitly to the one you mean)' % a.dtype)
    a = np.ascontiguousarray(a)
    if not a.flags.writeable:
        a = np.array(a)
    t = torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to(device)
    return t, a.dtype.type


def down_pixel_aggr_device(img_dev, scale, np_dtype=None):
    """[H,W,C] device tensor (float32, or int16 holding uint16 bits — `upload_raster`) -> float32 [H/scale,W/scale,C] device
    tensor: float32(reference downPixelAggr), which is what every consumer of the reference's float64 result casts it to."""
    if np_dtype is None:
        np_dtype = np.uint16 if img_dev.dtype == torch.int16 else np.float32
    if img_dev.dtype != (torch.int16 if np_dtype == np.uint16 else torch.float32):
        raise TypeError('down_pixel_aggr_device: tensor of %s for a raster of %s' % (img_dev.dtype, np.dtype(np_dtype)))
    if img_dev.dim() == 2:
        img_dev = img_dev[:, :, None]
    return _down(img_dev.contiguous(), np_dtype, scale, torch.float32)


def downPixelAggr(img, SCALE=2):
    """utils/patches.py:353-371 — Gaussian blur (sigma = 1/SCALE) + SCALE x SCALE pixel aggregation; float64 ndarray, squeezed,
    the reference's result bit for bit (dsen2_down_pixel_aggr)."""
    img = np.asarray(img)
    if img.ndim == 2:
        img = img[:, :, None]
    _check_divisible(img.shape[0], img.shape[1], SCALE)          # before anything touches the GPU
    t, dt = upload_raster(img)
    return np.squeeze(_down(t, dt, SCALE, torch.float64).cpu().numpy())


def save_test_patches(dset_10, dset_20, file, patchSize=128, border=4, interp=True):
    """utils/patches.py:159-166."""
    image_10, data20_interp = get_test_patches(dset_10, dset_20, patchSize=patchSize, border=border, interp=interp)
    print("Saving to file {}".format(file))
    np.save(file + 'data10', image_10)
    np.save(file + 'data20', data20_interp)
    print('Done!')


def save_test_patches60(dset_10, dset_20, dset_60, file, patchSize=192, border=12, interp=True):
    """utils/patches.py:169-178."""
    image_10, data20_interp, data60_interp = get_test_patches60(dset_10, dset_20, dset_60, patchSize=patchSize, border=border,
                                                                interp=interp)
    print("Saving to file {}".format(file))
    np.save(file + 'data10', image_10)
    np.save(file + 'data20', data20_interp)
    np.save(file + 'data60', data60_interp)
    print('Done!')


def random_origins(lr_shape, patch_lr, nr_crop, seed=None):
    """int32 [nr_crop, 2] upper-left corners on the low-resolution grid, drawn as utils/patches.py:199-200 / :244-245 draws them:
    two randrange calls per crop, axis 0 first, each over [0, extent - patch).  seed=None draws from the `random` module's
    global generator like the reference (random.seed(s) before the call == seed=s)."""
    rr = random.randrange if seed is None else random.Random(seed).randrange
    h, w = int(lr_shape[0]) - patch_lr, int(lr_shape[1]) - patch_lr
    if h <= 0 or w <= 0:
        raise ValueError('low-resolution image %r leaves no room for a %d x %d patch' % (tuple(lr_shape[:2]), patch_lr, patch_lr))
    org = np.empty((nr_crop, 2), np.int32)
    for i in range(nr_crop):
        org[i, 0] = rr(0, h)
        org[i, 1] = rr(0, w)
    return org


def _random_crops(img, origins, scale, patch, device):
    """The crops of one image at `origins * scale`, [N,C,patch,patch] float32 on the device (dsen2_tile_gather, border 0)."""
    img = _to_device_f32(img, device)
    if img.dim() == 2:
        img = img[:, :, None]
    if origins.shape[0] and ((origins.min() < 0) or (origins[:, 0].max() * scale + patch > img.shape[0])
                             or (origins[:, 1].max() * scale + patch > img.shape[1])):
        raise ValueError('crop origins reach outside the image of shape %r' % (tuple(img.shape),))
    return gather_patches_device(img, origins, scale, 0, patch, origins.shape[0])


def _origins_arg(origins, lr_shape, patch_lr, nr_crop, seed):
    if origins is None:
        return random_origins(lr_shape, patch_lr, nr_crop, seed)
    origins = np.ascontiguousarray(origins, dtype=np.int32).reshape(-1, 2)
    if origins.shape[0] != nr_crop:
        raise ValueError('%d origins for NR_CROP = %d' % (origins.shape[0], nr_crop))
    return origins


def save_random_patches(dset_20gt, dset_10, dset_20, file, NR_CROP=8000, seed=None, origins=None):
    """utils/patches.py:181-219: NR_CROP random 32 x 32 (10 m) patches — data10, data20_gt and the up-sampled data20 as float32
    [N,C,32,32] .npy files.  Images: host arrays of any real dtype or device tensors ([H,W,C]); they are cropped and up-sampled
    on the GPU and only the finished arrays are downloaded."""
    dev = default_device()
    org = _origins_arg(origins, dset_20.shape, 16, NR_CROP, seed)
    image_10 = _random_crops(dset_10, org, 2, 32, dev)
    np.save(file + 'data10', image_10.cpu().numpy())
    hr_hw = image_10.shape[2:4]
    del image_10
    np.save(file + 'data20_gt', _random_crops(dset_20gt, org, 2, 32, dev).cpu().numpy())
    image_20 = _random_crops(dset_20, org, 1, 16, dev)
    np.save(file + 'data20', interp_patches_device(image_20, hr_hw).cpu().numpy())
    print('Done!')


def save_random_patches60(dset_60gt, dset_10, dset_20, dset_60, file, NR_CROP=500, seed=None, origins=None):
    """utils/patches.py:222-271: NR_CROP random 96 x 96 (10 m) patches — data10, data60_gt, and data20 / data60 up-sampled."""
    dev = default_device()
    bands = [int(d.shape[2]) for d in (dset_60gt, dset_10, dset_20, dset_60)]
    for b, p in zip(bands, (96, 96, 48, 16)):                  # the reference prints its four array shapes (:236-239)
        print((NR_CROP, b, p, p))
    org = _origins_arg(origins, dset_60.shape, 16, NR_CROP, seed)
    image_10 = _random_crops(dset_10, org, 6, 96, dev)
    np.save(file + 'data10', image_10.cpu().numpy())
    hr_hw = image_10.shape[2:4]
    del image_10
    np.save(file + 'data60_gt', _random_crops(dset_60gt, org, 6, 96, dev).cpu().numpy())
    np.save(file + 'data20', interp_patches_device(_random_crops(dset_20, org, 3, 48, dev), hr_hw).cpu().numpy())
    np.save(file + 'data60', interp_patches_device(_random_crops(dset_60, org, 1, 16, dev), hr_hw).cpu().numpy())
    print('Done!')


# ---- reading a test set back (utils/patches.py:327-350) ------------------------------------------
def OpenDataFilesTest(path, run_60, SCALE, true_scale=False):
    """utils/patches.py:327-350: the tiled test set `python -m dsen2_amd.create_patches --test_data` wrote under `path` — ([data10,
    data20(, data60)] divided by SCALE, image_size).  image_size comes from roi.json = [xmin, ymin, xmax, ymax] and is, as in the
    reference, [xmax - xmin, ymax - ymin] = [width, height]; the three printed lines are the reference's.  Host work only."""
    if not SCALE:
        SCALE = 1
    names = ('data10', 'data20', 'data60') if run_60 else ('data10', 'data20')
    train = []
    for name in names:
        a = np.load(path + '/' + name + '.npy')
        a /= SCALE
        train.append(a)
    with open(path + '/roi.json') as f:
        roi = json.load(f)
    image_size = [roi[2] - roi[0], roi[3] - roi[1]]
    print("The image size is: {}".format(image_size))
    print("The SCALE is: {}".format(SCALE))
    print("The true_scale is: {}".format(true_scale))
    return train, image_size
