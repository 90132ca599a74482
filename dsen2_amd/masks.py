"""Scene-class and cloud masks: a validity bitmap from a class raster the caller brings (include/dsen2_hip.h, "class masks").

Not in the reference, which hand-picks clear tiles.  The class raster is Sentinel-2's SCL layer, a cloud-probability layer or any
2-D uint8 class image on the 10, 20 or 60 m grid of the tile; `classes` lists the values that make a pixel INVALID (lut: a 256-entry
table, so a probability layer with a threshold t is classes=range(t, 256)).  The bitmap is the one dsen2_tile_nodata writes —
uint32 [H][ceil(W/32)] (an int32 tensor here), bit x & 31 of word x >> 5, set = valid — and everything that honours that one honours
this one: supres.DSen2_20 / DSen2_60 (mask=), the recompositions, and, through raster_apply_valid_device, the ground truth of a
TileCorpus, where the training path then sees no-data (mask_nodata).  Everything runs on the GPU (csrc/valid_mask.hip)."""
import numpy as np
import torch

from . import _lib, patches

# Sentinel-2 L2A scene classification: 0 no data, 1 saturated or defective, 3 cloud shadow, 8 cloud medium probability, 9 cloud high
# probability, 10 thin cirrus.  (2 dark area, 4 vegetation, 5 not vegetated, 6 water, 7 unclassified, 11 snow or ice are data.)
SCL_INVALID = (0, 1, 3, 8, 9, 10)
MAX_RATIO = 8
MAX_DILATE = 32


def lut(classes):
    """uint8 [256]: 1 at every value of `classes` (ints in 0..255; None = SCL_INVALID), 0 elsewhere."""
    table = np.zeros(256, np.uint8)
    for c in SCL_INVALID if classes is None else classes:
        if isinstance(c, (bool, np.bool_)) or int(c) != c or not 0 <= int(c) <= 255:
            raise ValueError('a class is an integer in 0..255, got %r' % (c,))
        table[int(c)] = 1
    return table


def parse_classes(text):
    """'0,1,3,8,9,10' -> (0, 1, 3, 8, 9, 10) (the command lines' --mask_classes); None or '' -> None."""
    if text is None or not str(text).strip():
        return None
    try:
        classes = tuple(int(t) for t in str(text).split(',') if t.strip())
    except ValueError:
        raise ValueError('--mask_classes is a comma-separated list of integers in 0..255, got %r' % (text,))
    lut(classes)
    return classes


def ratio(src_shape, shape):
    """(up, down) of a class raster of src_shape = (Hs, Ws) for a target grid of shape = (H, W): per axis up = ceil(H / Hs) in 1..8
    when the source is coarser, or down = Hs // H in 1..8 when it is finer (surplus source rows and columns are never read); both
    axes must agree.  ValueError otherwise."""
    hs, ws = int(src_shape[0]), int(src_shape[1])
    h, w = int(shape[0]), int(shape[1])
    per_axis = []
    for n, ns in ((h, hs), (w, ws)):
        if n < 1 or ns < 1:
            per_axis.append(None)
        elif ns >= n:
            per_axis.append((1, ns // n))
        else:
            per_axis.append((-(-n // ns), 1))
    if None in per_axis or per_axis[0] != per_axis[1] or max(per_axis[0]) > MAX_RATIO:
        raise ValueError('a class raster of %r does not fit a grid of %r: per axis the grid is 1..%d times the raster (rounded up) or '
                         'the raster 1..%d times the grid (rounded down), the same on both axes'
                         % ((hs, ws), (h, w), MAX_RATIO, MAX_RATIO))
    return per_axis[0]


def _class_raster_device(cls, device):
    if isinstance(cls, torch.Tensor):
        if cls.dtype != torch.uint8 or cls.dim() != 2:
            raise ValueError('a class raster is a 2-D uint8 image, got %r %s' % (tuple(cls.shape), cls.dtype))
        return cls.to(device).contiguous()
    a = np.asarray(cls)
    if a.dtype != np.uint8 or a.ndim != 2:
        raise ValueError('a class raster is a 2-D uint8 image, got %r %s' % (a.shape, a.dtype))
    a = np.ascontiguousarray(a)
    if not a.flags.writeable:
        a = np.array(a)
    return torch.from_numpy(a).to(device)


def bitmap_shape(shape):
    return int(shape[0]), (int(shape[1]) + 31) // 32


def valid_bits_device(cls, shape, classes=SCL_INVALID, dilate=0, and_bits=None, device=None, out=None):
    """The validity bitmap (int32 [H, ceil(W / 32)] on the device) of the grid shape = (H, W) from the class raster `cls` (2-D uint8,
    ndarray or tensor): a pixel is invalid when its class — with a finer raster: any class of its block — is in `classes`, or when
    such a pixel lies within `dilate` grid pixels (0..32) of it along both axes; ANDed with `and_bits` (a bitmap of the same grid,
    e.g. patches.nodata_device's; it may be `out`) when given.  dsen2_class_valid_bits; enqueues only."""
    h, w = int(shape[0]), int(shape[1])
    src_shape = tuple(int(s) for s in np.shape(cls))
    if len(src_shape) != 2:
        raise ValueError('a class raster is a 2-D uint8 image, got shape %r' % (src_shape,))
    up, down = ratio(src_shape, (h, w))                    # every refusal before the GPU is touched
    dilate = int(dilate)
    if not 0 <= dilate <= MAX_DILATE:
        raise ValueError('dilate is in pixels, 0..%d, got %d' % (MAX_DILATE, dilate))
    table = lut(classes)
    if device is None:
        device = and_bits.device if and_bits is not None else cls.device if isinstance(cls, torch.Tensor) and cls.is_cuda else \
            patches.default_device()
    cls_dev = _class_raster_device(cls, device)
    want = bitmap_shape((h, w))
    for name, t in (('and_bits', and_bits), ('out', out)):
        if t is not None and (tuple(t.shape) != want or t.dtype != torch.int32 or not t.is_contiguous() or t.device != cls_dev.device):
            raise ValueError('%s must be a contiguous int32 %s bitmap of shape %r' % (name, cls_dev.device, want))
    bits = out if out is not None else torch.empty(want, dtype=torch.int32, device=cls_dev.device)
    with torch.cuda.device(cls_dev.device):
        _lib.call('dsen2_class_valid_bits', patches._ptr(cls_dev), src_shape[0], src_shape[1], table.ctypes.data, up, down, h, w, dilate,
                  patches._ptr(and_bits) if and_bits is not None else None, patches._ptr(bits), patches._stream(cls_dev.device))
    return bits


def tile_flags_device(bits, size, patch, border):
    """uint8 [y_tiles * x_tiles] on the device, 1 = the patch's owned rectangle holds no valid pixel of the bitmap `bits`
    (dsen2_tile_flags_from_bits: what patches.nodata_device returns next to ITS bitmap, for any bitmap)."""
    h, w = int(size[0]), int(size[1])
    xt, yt, words = patches.nodata_geometry((h, w), patch, border)
    if tuple(bits.shape) != bitmap_shape((h, w)) or bits.dtype != torch.int32 or not bits.is_contiguous():
        raise ValueError('the bitmap of a %d x %d grid is a contiguous int32 tensor of shape %r' % (h, w, bitmap_shape((h, w))))
    empty = torch.empty(xt * yt, dtype=torch.uint8, device=bits.device)
    with torch.cuda.device(bits.device):
        _lib.call('dsen2_tile_flags_from_bits', patches._ptr(bits), h, w, int(patch), int(border), patches._ptr(empty),
                  patches._stream(bits.device))
    return empty


def raster_apply_valid_device(img, bits):
    """In place: every sample of a pixel of the HWC raster `img` (float32, or int16 holding uint16 bits: patches.upload_raster)
    whose bit in `bits` is 0 becomes 0; nothing else is written (dsen2_raster_apply_valid)."""
    if img.dim() != 3 or img.dtype not in (torch.int16, torch.float32) or not img.is_contiguous():
        raise ValueError('the raster must be a contiguous HWC tensor of float32 or of uint16 bits (int16), got %r %s' % (tuple(img.shape), img.dtype))
    h, w, c = (int(s) for s in img.shape)
    if tuple(bits.shape) != bitmap_shape((h, w)) or bits.dtype != torch.int32 or not bits.is_contiguous() or bits.device != img.device:
        raise ValueError('the bitmap of a %d x %d raster is a contiguous int32 %s tensor of shape %r' % (h, w, img.device, bitmap_shape((h, w))))
    with torch.cuda.device(img.device):
        _lib.call('dsen2_raster_apply_valid', patches._ptr(img), _lib.DTYPE_U16 if img.dtype == torch.int16 else _lib.DTYPE_F32, h, w, c,
                  patches._ptr(bits), patches._stream(img.device))
    return img


def apply_to_image(image, cls, classes=None, dilate=0):
    """where(valid, image, 0) for a host HWC image: the class raster's bitmap on the image's grid, applied on the GPU.  Returns a
    float32 array.  For images that are recomposed on the host (python -m dsen2_amd.train --predict)."""
    dev = patches.default_device()
    img = patches._to_device_f32(np.asarray(image), dev)
    bits = valid_bits_device(cls, img.shape[:2], SCL_INVALID if classes is None else classes, dilate, device=dev)
    return raster_apply_valid_device(img, bits).cpu().numpy()


def cells_from_bits_device(bits, shape, s, cells=None):
    """uint8 [H / s, W / s] on the device: 1 where any pixel of the cell's s x s footprint is invalid in `bits` (the bitmap of the
    grid shape = (H, W)).  cells: a map of that shape to OR into (a cell that holds non-zero stays as it is) instead of a new one
    (dsen2_cells_from_valid_bits)."""
    h, w, s = int(shape[0]), int(shape[1]), int(s)
    if not 1 <= s <= 8 or h % s or w % s:
        raise ValueError('a cell of %d pixels (1..8) must divide the grid %r' % (s, (h, w)))
    if tuple(bits.shape) != bitmap_shape((h, w)) or bits.dtype != torch.int32 or not bits.is_contiguous():
        raise ValueError('the bitmap of a %d x %d grid is a contiguous int32 tensor of shape %r' % (h, w, bitmap_shape((h, w))))
    accumulate = cells is not None
    if cells is None:
        cells = torch.empty((h // s, w // s), dtype=torch.uint8, device=bits.device)
    elif tuple(cells.shape) != (h // s, w // s) or cells.dtype != torch.uint8 or not cells.is_contiguous() or cells.device != bits.device:
        raise ValueError('cells must be a contiguous uint8 %s map of shape %r' % (bits.device, (h // s, w // s)))
    with torch.cuda.device(bits.device):
        _lib.call('dsen2_cells_from_valid_bits', patches._ptr(bits), h, w, s, int(accumulate), patches._ptr(cells),
                  patches._stream(bits.device))
    return cells
