"""MATLAB-compatible bicubic `imresize` on the GPU: the drop-in for the reference's utils/imresize.py.

    from dsen2_amd.imresize import imresize
    imresize(I, scalar_scale=None, output_shape=None)   -> float64 ndarray (2-D in -> 2-D out), the reference's values
    imresize_device(t, scalar_scale=None, output_shape=None)   -> the float64 device tensor [OH, OW, C]
    contributions(in_length, out_length, scale)         -> (weights float64 [out_length, P], indices int32 [out_length, P])

The resampling itself is two launches of dsen2_imresize_axis (csrc/imresize.hip): one pass per image axis, each output the
sequential float64 sum of `taps` products, the pass with the smaller scale first (numpy's stable argsort of the two scales, as
the reference orders them: equal scales run axis 0 first) and the second pass reading the first's float64 result.  Only the tap
tables are built here, on the host, with numpy — O(out_length) work; they are uploaded and the device evaluates no polynomial.

Inputs: uint16, float32 or float64, [H, W] or [H, W, C].  uint8 is refused (the reference rounds and clips it back to uint8: nobody
here has such data); so is any other dtype.  Neither scalar_scale nor output_shape: ValueError (the reference prints a line and
returns None).
"""
from math import ceil

import numpy as np

_TAPS_WIDTH = 4.0        # support of the cubic convolution kernel (a = -0.5)


def _cubic(x):
    """Keys' cubic convolution kernel with a = -0.5: 1.5|x|^3 - 2.5|x|^2 + 1 on [0, 1], -0.5|x|^3 + 2.5|x|^2 - 4|x| + 2 on (1, 2]."""
    ax = np.abs(np.asarray(x, dtype=np.float64))
    ax2 = ax * ax
    ax3 = ax2 * ax
    near = (1.5 * ax3 - 2.5 * ax2 + 1) * (ax <= 1)
    far = (-0.5 * ax3 + 2.5 * ax2 - 4 * ax + 2) * ((1 < ax) & (ax <= 2))
    return near + far


def contributions(in_length, out_length, scale):
    """The taps of one axis: output o = sum_k weights[o, k] * input[indices[o, k]].

    Output sample x = 1 .. out_length sits at u = x / scale + 0.5 (1 - 1 / scale) on the input's 1-based grid.  When the image
    shrinks (scale < 1) the kernel is stretched by 1 / scale and scaled by `scale`: the antialiasing.  P = ceil(width) + 2 taps
    start at floor(u - width / 2); each row is divided by its sum; an index outside the image is folded through the periodic
    table [0 .. n-1, n-1 .. 0] with a true modulo (an image shorter than the taps reflects more than once); tap columns that are
    zero for every output are dropped."""
    scale = float(scale)
    if scale < 1:
        width = _TAPS_WIDTH / scale

        def kernel(t):
            return scale * _cubic(scale * t)
    else:
        width = _TAPS_WIDTH
        kernel = _cubic
    u = np.arange(1, out_length + 1).astype(np.float64) / scale + 0.5 * (1 - 1 / scale)
    taps = int(ceil(width)) + 2
    first = np.floor(u - width / 2)
    index = (first[:, None] + np.arange(taps) - 1).astype(np.int32)               # 0-based
    weights = kernel(u[:, None] - index - 1)
    weights = weights / np.sum(weights, axis=1)[:, None]
    fold = np.concatenate((np.arange(in_length), np.arange(in_length - 1, -1, -1))).astype(np.int32)
    index = fold[np.mod(index, fold.size)]
    keep = np.any(weights, axis=0)
    return np.ascontiguousarray(weights[:, keep]), np.ascontiguousarray(index[:, keep])


def plan(in_shape, scalar_scale=None, output_shape=None):
    """(output size [OH, OW], scales [s0, s1], pass order (first axis, second axis)) as the reference derives them."""
    if scalar_scale is not None:
        s = float(scalar_scale)
        scale = [s, s]
        size = [int(ceil(scale[k] * in_shape[k])) for k in range(2)]
    elif output_shape is not None:
        size = [int(output_shape[0]), int(output_shape[1])]
        scale = [1.0 * size[k] / in_shape[k] for k in range(2)]
    else:
        raise ValueError('imresize: scalar_scale OR output_shape should be defined')
    if min(size) < 1:
        raise ValueError('imresize: empty output %r' % (size,))
    order = tuple(int(k) for k in np.argsort(np.array(scale), kind='stable'))
    return size, scale, order


_NP_DTYPES = (np.uint16, np.float32, np.float64)


def _check_image(shape, dtype):
    if len(shape) not in (2, 3):
        raise ValueError('imresize takes an [H, W] or [H, W, C] image, not %d dimensions' % len(shape))
    if dtype == np.uint8:
        raise TypeError('imresize: uint8 images are not supported (the reference rounds and clips them back to uint8)')
    if dtype not in _NP_DTYPES:
        raise TypeError('imresize takes uint16, float32 or float64 images, not %s' % np.dtype(dtype))
    if min(shape) < 1:
        raise ValueError('imresize: empty image %r' % (tuple(shape),))


def device_taps(in_length, out_length, scale, device):
    """contributions() as the kernel reads it: (weights [P, out_length] float64, indices [P, out_length] int32, P) on `device`."""
    import torch
    w, i = contributions(in_length, out_length, scale)
    return (torch.from_numpy(np.ascontiguousarray(w.T)).to(device), torch.from_numpy(np.ascontiguousarray(i.T)).to(device), w.shape[1])


def _lib_dtype(t, np_dtype=None):
    import torch
    from . import _lib
    if t.dtype == torch.int16 and np_dtype in (None, np.uint16):
        return _lib.DTYPE_U16
    if t.dtype == torch.float32:
        return _lib.DTYPE_F32
    if t.dtype == torch.float64:
        return _lib.DTYPE_F64
    raise TypeError('imresize on the GPU takes float32, float64 or uint16 (as int16 bits) tensors, not %s' % t.dtype)


def resize_axis_device(t, axis, out_length, taps, np_dtype=None):
    """One pass: t [H, W, C] -> float64 [out_length, W, C] (axis 0) or [H, out_length, C] (axis 1); taps from device_taps."""
    import torch
    from . import _lib, patches
    h, w, c = t.shape
    shape = (out_length, w, c) if axis == 0 else (h, out_length, c)
    out = torch.empty(shape, dtype=torch.float64, device=t.device)
    with torch.cuda.device(t.device):
        _lib.call('dsen2_imresize_axis', patches._ptr(t), _lib_dtype(t, np_dtype), h, w, c, axis, out_length, patches._ptr(taps[0]),
                  patches._ptr(taps[1]), taps[2], patches._ptr(out), patches._stream(t.device))
    return out


def imresize_device(t, scalar_scale=None, output_shape=None, np_dtype=None):
    """[H, W, C] (or [H, W]) device tensor — float32, float64, or int16 holding uint16 bits (patches.upload_raster) — ->
    float64 device tensor [OH, OW, C] ([OH, OW])."""
    import torch
    if not t.is_cuda:
        raise RuntimeError('dsen2_amd needs a ROCm GPU (gfx950); there is no CPU fallback')
    kinds = {torch.int16: np.uint16, torch.float32: np.float32, torch.float64: np.float64, torch.uint8: np.uint8}
    if t.dtype not in kinds:
        raise TypeError('imresize on the GPU takes float32, float64 or uint16 (as int16 bits) tensors, not %s' % t.dtype)
    _check_image(tuple(t.shape), kinds[t.dtype])
    flat = t.dim() == 2
    x = (t[:, :, None] if flat else t).contiguous()
    size, scale, order = plan(x.shape, scalar_scale, output_shape)
    for axis in order:
        taps = device_taps(x.shape[axis], size[axis], scale[axis], x.device)
        x = resize_axis_device(x, axis, size[axis], taps, np_dtype)
        np_dtype = None
    return x[:, :, 0] if flat else x


def _upload(I):
    """A host image in its own dtype (uint16 as int16 bits) on the default device."""
    import torch
    from . import patches
    a = np.asarray(I)
    _check_image(a.shape, a.dtype)
    dev = patches.default_device()
    a = np.ascontiguousarray(a)
    if not a.flags.writeable:
        a = np.array(a)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to(dev)


def imresize(I, scalar_scale=None, output_shape=None):
    """utils/imresize.py:80-112 on the GPU: the reference's float64 result (bit for bit wherever numpy adds the taps of an output
    sequentially: every enlargement, and every reduction of an image with two or more bands)."""
    a = np.asarray(I)
    _check_image(a.shape, a.dtype)
    plan(a.shape, scalar_scale, output_shape)             # argument errors before anything touches the GPU
    return imresize_device(_upload(a), scalar_scale, output_shape).cpu().numpy()

