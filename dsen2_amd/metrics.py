"""Scores of the evaluation step, computed on the GPU (csrc/imresize.hip: dsen2_band_errors, dsen2_imresize_band_errors).

    RMSE(x1, x2)                   testing/demoDSen2.py:31-35 — over all elements in float64; prints 'RMSE: %.4f', returns the value
    band_errors(x, gt)             (rmse [C], sre [C]) per band of two HWC images
    bicubic_errors(lr, gt, scale)  the same for the MATLAB-bicubic enlargement of `lr` — the demo's 'Bicubic:' baseline — without
                                   ever storing the enlarged image (the second resampling pass accumulates the errors itself)
    error_sums / bicubic_error_sums   the float64 sums underneath: [C, 3] = sum (x - gt)^2, sum gt, pixels

SRE is the paper's signal-to-reconstruction error per band, 10 log10(mean(gt)^2 / mean((x - gt)^2)) in dB.  Inputs are numpy
arrays or device tensors, [H, W, C] or [H, W]; float32 and float64 go to the kernel as they are, uint16 (a Sentinel-2 raster as the
ground truth) is widened on the GPU, exactly.  The sums are added in an order that depends on the shapes only: the same bits on
every run.  Like everything in this package there is no host fallback: without a GPU these raise patches.default_device's error.
"""
import ctypes

import numpy as np


def _device_image(a, device=None):
    """numpy array or tensor -> contiguous [H, W, C] float32 / float64 device tensor."""
    import torch
    from . import patches
    if isinstance(a, torch.Tensor):
        if not a.is_cuda:
            raise RuntimeError('dsen2_amd needs a ROCm GPU (gfx950); there is no CPU fallback')
        t = a
        if t.dtype == torch.int16:
            t = patches._widen(t, np.uint16)
        elif t.dtype not in (torch.float32, torch.float64):
            t = t.to(torch.float64)
    else:
        device = device or patches.default_device()
        a = np.asarray(a)
        if a.dtype == np.uint16:
            t = patches._widen(patches.upload_raster(a, device)[0], np.uint16)
        else:
            if a.dtype not in (np.float32, np.float64):
                a = a.astype(np.float64)
            a = np.ascontiguousarray(a)
            t = torch.from_numpy(a if a.flags.writeable else np.array(a)).to(device)
    if t.dim() == 2:
        t = t[:, :, None]
    if t.dim() != 3:
        raise ValueError('an [H, W] or [H, W, C] image is expected, not %d dimensions' % t.dim())
    return t.contiguous()


def _lib_dtype(t):
    import torch
    from . import _lib
    return _lib.DTYPE_F64 if t.dtype == torch.float64 else _lib.DTYPE_F32


def _workspace(c, device):
    import torch
    from . import _lib
    n = ctypes.c_size_t(0)
    _lib.call('dsen2_band_errors_workspace_bytes', c, ctypes.byref(n))
    return torch.empty(n.value, dtype=torch.uint8, device=device), n.value


def error_sums_device(x, gt):
    """[C, 3] float64 device tensor of two [H, W, C] float32 / float64 device tensors: sum (x - gt)^2, sum gt, H * W."""
    import torch
    from . import _lib, patches
    if tuple(x.shape) != tuple(gt.shape):
        raise ValueError('images of shape %r and %r' % (tuple(x.shape), tuple(gt.shape)))
    h, w, c = x.shape
    out = torch.empty((c, 3), dtype=torch.float64, device=x.device)
    with torch.cuda.device(x.device):
        work, nbytes = _workspace(c, x.device)
        _lib.call('dsen2_band_errors', patches._ptr(x), _lib_dtype(x), patches._ptr(gt), _lib_dtype(gt), h, w, c, patches._ptr(work), nbytes,
                  patches._ptr(out), patches._stream(x.device))
    return out


def error_sums(x, gt):
    """[C, 3] float64 ndarray: per band sum (x - gt)^2, sum gt, pixel count."""
    x = _device_image(x)
    gt = _device_image(gt, x.device)
    return error_sums_device(x, gt).cpu().numpy()


def resample_error_sums_device(mid, axis, out_length, taps, gt):
    """[C, 3] float64 device tensor: error_sums_device(resize_axis_device(mid, axis, out_length, taps), gt) in one pass that never
    stores the resampled image (dsen2_imresize_band_errors).  mid: [H, W, C] float32 / float64 device tensor; taps: device_taps."""
    import torch
    from . import _lib, patches
    h, w, c = mid.shape
    out = torch.empty((c, 3), dtype=torch.float64, device=mid.device)
    with torch.cuda.device(mid.device):
        work, nbytes = _workspace(c, mid.device)
        _lib.call('dsen2_imresize_band_errors', patches._ptr(mid), _lib_dtype(mid), h, w, c, axis, out_length, patches._ptr(taps[0]),
                  patches._ptr(taps[1]), taps[2], patches._ptr(gt), _lib_dtype(gt), patches._ptr(work), nbytes, patches._ptr(out),
                  patches._stream(mid.device))
    return out


def bicubic_error_sums(lr, gt, scale):
    """error_sums(imresize(lr, scale), gt) with the second resampling pass fused into the reduction: [C, 3] float64 ndarray."""
    from . import imresize as ir
    lr = _device_image(lr)
    gt = _device_image(gt, lr.device)
    size, scales, order = ir.plan(lr.shape, scalar_scale=scale)
    if tuple(gt.shape) != (size[0], size[1], lr.shape[2]):
        raise ValueError('ground truth of shape %r for an enlargement to %r' % (tuple(gt.shape), (size[0], size[1], lr.shape[2])))
    first, second = order
    mid = ir.resize_axis_device(lr, first, size[first], ir.device_taps(lr.shape[first], size[first], scales[first], lr.device))
    taps = ir.device_taps(mid.shape[second], size[second], scales[second], lr.device)
    return resample_error_sums_device(mid, second, size[second], taps, gt).cpu().numpy()


def scores(sums):
    """(rmse [C], sre [C], rmse over all bands) of a [C, 3] array of sums."""
    sums = np.asarray(sums, np.float64)
    mse = sums[:, 0] / sums[:, 2]
    mean_gt = sums[:, 1] / sums[:, 2]
    with np.errstate(divide='ignore', invalid='ignore'):
        sre = 10.0 * np.log10(mean_gt * mean_gt / mse)
    total = float(np.sqrt(sums[:, 0].sum() / sums[:, 2].sum()))
    return np.sqrt(mse), sre, total


def band_errors(x, gt):
    """(rmse [C], sre [C]) float64 ndarrays of two HWC images."""
    return scores(error_sums(x, gt))[:2]


def bicubic_errors(lr, gt, scale):
    """(rmse [C], sre [C]) of the bicubic enlargement of `lr` by `scale` against `gt` (dsen2_imresize_band_errors)."""
    return scores(bicubic_error_sums(lr, gt, scale))[:2]


def RMSE(x1, x2):
    """testing/demoDSen2.py:31-35: sqrt(mean((x1 - x2)^2)) over all elements in float64, printed with four decimals."""
    a = _device_image(x1)
    b = _device_image(x2, a.device)
    rms = scores(error_sums_device(a, b).cpu().numpy())[2]
    print('RMSE: {:.4f}'.format(rms))
    return rms
