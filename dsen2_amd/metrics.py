"""Scores of the evaluation step, computed on the GPU (csrc/imresize.hip: dsen2_band_errors, dsen2_imresize_band_errors;
csrc/quality_metrics.hip: dsen2_uiq_map, dsen2_uiq_sums, dsen2_sam_sums and their fused bicubic forms; csrc/ssim.hip:
dsen2_ssim_map, dsen2_ssim_sums, dsen2_imresize_ssim_sums).

    RMSE(x1, x2)                   testing/demoDSen2.py:31-35 — over all elements in float64; prints 'RMSE: %.4f', returns the value
    band_errors(x, gt)             (rmse [C], sre [C]) per band of two HWC images
    bicubic_errors(lr, gt, scale)  the same for the MATLAB-bicubic enlargement of `lr` — the demo's 'Bicubic:' baseline — without
                                   ever storing the enlarged image (the second resampling pass accumulates the errors itself)
    error_sums / bicubic_error_sums   the float64 sums underneath: [C, 3] = sum (x - gt)^2, sum gt, pixels
    UIQ(x, gt, block_size=8)       (uiq [C], mean over the bands): the universal image quality index of Wang & Bovik (img_qi.m), the mean
                                   of the quality map over all block_size x block_size windows of a band
    uiq_map(x, gt, block_size=8)   that map, float64 [H - block_size + 1, W - block_size + 1, C] ([.., ..] for 2-D inputs)
    SAM(x, gt)                     the spectral angle mapper: the mean angle in degrees between the two spectra of a pixel, over the
                                   pixels whose spectrum is zero in neither image
    bicubic_UIQ(lr, gt, scale, block_size=8) / bicubic_SAM(lr, gt, scale)   the same for the bicubic enlargement of `lr`, never stored
    uiq_sums / sam_sums / bicubic_uiq_sums / bicubic_sam_sums   the sums underneath: [C, 2] = sum of the map, windows; [2] = sum of
                                   the angles, pixels counted
    SSIM(x, gt, data_range, win_size=11, sigma=1.5)   (ssim [C], mean over the bands): the structural similarity index of Wang et
                                   al. 2004 (ssim_index.m without its down-sampling), the mean of the map over all valid windows of a
                                   band; Gaussian window (ssim_window), biased covariance, C1 = (k1 L)^2, C2 = (k2 L)^2, L = data_range
    ssim_map(x, gt, data_range)    that map, float64 [H - win_size + 1, W - win_size + 1, C]
    bicubic_SSIM(lr, gt, scale, data_range)   the same for the bicubic enlargement of `lr`, never stored
    ssim_sums / bicubic_ssim_sums / ssim_scores   the sums underneath, [C, 2] = sum of the map, windows; and their quotients
    ERGAS(x, gt, scale) / PSNR(x, gt, data_range) / bicubic_ERGAS / bicubic_PSNR   formulas over error_sums / bicubic_error_sums
                                   (ergas_score, psnr_scores): float64 on the host, no kernel of their own

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


# ---- UIQ and SAM (csrc/quality_metrics.hip) ----

def _shape3(a):
    shape = tuple(a.shape)
    if len(shape) == 2:
        shape = shape + (1,)
    if len(shape) != 3:
        raise ValueError('an [H, W] or [H, W, C] image is expected, not %d dimensions' % len(shape))
    return shape


def _check_pair(x, gt, block_size=None):
    """The refusals that need no GPU: shapes, bands, block size.  Returns the common [H, W, C]."""
    shape = _shape3(x)
    if _shape3(gt) != shape:
        raise ValueError('images of shape %r and %r' % (tuple(x.shape), tuple(gt.shape)))
    if min(shape) < 1 or shape[2] > 64:
        raise ValueError('an image of shape %r: empty, or more than 64 bands' % (shape,))
    if block_size is not None:
        _check_block(shape, block_size)
    return shape


def _check_block(shape, block_size):
    if int(block_size) != block_size or not 2 <= block_size <= 16:
        raise ValueError('block_size %r outside 2..16' % (block_size,))
    if shape[0] < block_size or shape[1] < block_size:
        raise ValueError('an image of %d x %d is smaller than the %d x %d block' % (shape[0], shape[1], block_size, block_size))


def _bicubic_shape(lr, gt, scale):
    """The refusals of the fused bicubic forms that need no GPU; returns the enlargement's [H, W, C]."""
    from . import imresize as ir
    shape = _shape3(lr)
    size = ir.plan(shape, scalar_scale=scale)[0]
    want = (size[0], size[1], shape[2])
    if _shape3(gt) != want:
        raise ValueError('ground truth of shape %r for an enlargement to %r' % (tuple(gt.shape), want))
    if shape[2] > 64:
        raise ValueError('an image of shape %r: more than 64 bands' % (shape,))
    return want


def _quality_workspace(c, device):
    import torch
    from . import _lib
    n = ctypes.c_size_t(0)
    _lib.call('dsen2_quality_workspace_bytes', c, ctypes.byref(n))
    return torch.empty(n.value, dtype=torch.uint8, device=device), n.value


def uiq_map_device(x, gt, block_size=8):
    """float64 device tensor [H - B + 1, W - B + 1, C] of two [H, W, C] float32 / float64 device tensors (dsen2_uiq_map)."""
    import torch
    from . import _lib, patches
    h, w, c = _check_pair(x, gt, block_size)
    out = torch.empty((h - block_size + 1, w - block_size + 1, c), dtype=torch.float64, device=x.device)
    with torch.cuda.device(x.device):
        _lib.call('dsen2_uiq_map', patches._ptr(x), _lib_dtype(x), patches._ptr(gt), _lib_dtype(gt), h, w, c, int(block_size),
                  patches._ptr(out), patches._stream(x.device))
    return out


def uiq_sums_device(x, gt, block_size=8):
    """[C, 2] float64 device tensor: per band the sum of the quality map and the number of windows; the map is never stored."""
    import torch
    from . import _lib, patches
    h, w, c = _check_pair(x, gt, block_size)
    out = torch.empty((c, 2), dtype=torch.float64, device=x.device)
    with torch.cuda.device(x.device):
        work, nbytes = _quality_workspace(c, x.device)
        _lib.call('dsen2_uiq_sums', patches._ptr(x), _lib_dtype(x), patches._ptr(gt), _lib_dtype(gt), h, w, c, int(block_size),
                  patches._ptr(work), nbytes, patches._ptr(out), patches._stream(x.device))
    return out


def sam_sums_device(x, gt):
    """[2] float64 device tensor: the sum of the spectral angles in degrees and the number of pixels counted."""
    import torch
    from . import _lib, patches
    h, w, c = _check_pair(x, gt)
    out = torch.empty((2,), dtype=torch.float64, device=x.device)
    with torch.cuda.device(x.device):
        work, nbytes = _quality_workspace(c, x.device)
        _lib.call('dsen2_sam_sums', patches._ptr(x), _lib_dtype(x), patches._ptr(gt), _lib_dtype(gt), h, w, c, patches._ptr(work), nbytes,
                  patches._ptr(out), patches._stream(x.device))
    return out


def resample_quality_sums_device(mid, axis, out_length, taps, gt, block_size=None):
    """uiq_sums_device (block_size given) or sam_sums_device (None) of resize_axis_device(mid, axis, out_length, taps) against gt,
    in one pass that never stores the resampled image (dsen2_imresize_uiq_sums / dsen2_imresize_sam_sums)."""
    import torch
    from . import _lib, patches
    h, w, c = mid.shape
    out = torch.empty((c, 2) if block_size is not None else (2,), dtype=torch.float64, device=mid.device)
    with torch.cuda.device(mid.device):
        work, nbytes = _quality_workspace(c, mid.device)
        head = (patches._ptr(mid), _lib_dtype(mid), h, w, c, axis, out_length, patches._ptr(taps[0]), patches._ptr(taps[1]), taps[2],
                patches._ptr(gt), _lib_dtype(gt))
        tail = (patches._ptr(work), nbytes, patches._ptr(out), patches._stream(mid.device))
        if block_size is not None:
            _lib.call('dsen2_imresize_uiq_sums', *(head + (int(block_size),) + tail))
        else:
            _lib.call('dsen2_imresize_sam_sums', *(head + tail))
    return out


def _pair_on_device(x, gt, block_size=None):
    _check_pair(np.asarray(x) if not hasattr(x, 'shape') else x, np.asarray(gt) if not hasattr(gt, 'shape') else gt, block_size)
    x = _device_image(x)
    return x, _device_image(gt, x.device)


def uiq_map(x, gt, block_size=8):
    """The UIQ quality map, float64 ndarray [H - B + 1, W - B + 1, C] (2-D inputs: [H - B + 1, W - B + 1])."""
    flat = len(np.shape(x)) == 2
    a, b = _pair_on_device(x, gt, block_size)
    q = uiq_map_device(a, b, block_size).cpu().numpy()
    return q[:, :, 0] if flat else q


def uiq_sums(x, gt, block_size=8):
    """[C, 2] float64 ndarray: per band the sum of the quality map and the number of windows."""
    a, b = _pair_on_device(x, gt, block_size)
    return uiq_sums_device(a, b, block_size).cpu().numpy()


def sam_sums(x, gt):
    """[2] float64 ndarray: the sum of the spectral angles in degrees, the number of pixels counted."""
    a, b = _pair_on_device(x, gt)
    return sam_sums_device(a, b).cpu().numpy()


def _bicubic_quality_sums(lr, gt, scale, block_size):
    from . import imresize as ir
    lr = lr if hasattr(lr, 'shape') else np.asarray(lr)
    gt = gt if hasattr(gt, 'shape') else np.asarray(gt)
    want = _bicubic_shape(lr, gt, scale)
    if block_size is not None:
        _check_block(want, block_size)
    lr = _device_image(lr)
    gt = _device_image(gt, lr.device)
    size, scales, order = ir.plan(lr.shape, scalar_scale=scale)
    first, second = order
    mid = ir.resize_axis_device(lr, first, size[first], ir.device_taps(lr.shape[first], size[first], scales[first], lr.device))
    taps = ir.device_taps(mid.shape[second], size[second], scales[second], lr.device)
    return resample_quality_sums_device(mid, second, size[second], taps, gt, block_size).cpu().numpy()


def bicubic_uiq_sums(lr, gt, scale, block_size=8):
    """uiq_sums(imresize(lr, scale), gt, block_size), the same bits, with the second resampling pass computed inside the UIQ
    kernel's loader: the enlarged image is never stored."""
    return _bicubic_quality_sums(lr, gt, scale, block_size)


def bicubic_sam_sums(lr, gt, scale):
    """sam_sums(imresize(lr, scale), gt), the same bits, without storing the enlarged image."""
    return _bicubic_quality_sums(lr, gt, scale, None)


def uiq_scores(sums):
    """(uiq [C], mean over the bands) of a [C, 2] array of sums."""
    sums = np.asarray(sums, np.float64)
    band = sums[:, 0] / sums[:, 1]
    return band, float(np.mean(band))


def sam_score(sums):
    """SAM in degrees of a [2] array of sums; nan when no pixel was counted."""
    sums = np.asarray(sums, np.float64)
    return float(sums[0] / sums[1]) if sums[1] else float('nan')


def UIQ(x, gt, block_size=8):
    """(uiq [C] float64 ndarray, its mean over the bands): the universal image quality index of two HWC images."""
    return uiq_scores(uiq_sums(x, gt, block_size))


def SAM(x, gt):
    """The spectral angle mapper of two HWC images, in degrees."""
    return sam_score(sam_sums(x, gt))


def bicubic_UIQ(lr, gt, scale, block_size=8):
    """UIQ of the bicubic enlargement of `lr` by `scale` against `gt`."""
    return uiq_scores(bicubic_uiq_sums(lr, gt, scale, block_size))


def bicubic_SAM(lr, gt, scale):
    """SAM of the bicubic enlargement of `lr` by `scale` against `gt`, in degrees."""
    return sam_score(bicubic_sam_sums(lr, gt, scale))


# ---- SSIM (csrc/ssim.hip) ----

def ssim_window(win_size=11, sigma=1.5):
    """The separable Gaussian window of the SSIM, float64 [win_size]: w[i] = exp(-(i - (P - 1) / 2)^2 / (2 sigma^2)) divided by
    their sum (ssim_index.m's fspecial('gaussian', 11, 1.5) is its outer product).  The kernels take it from the host."""
    if int(win_size) != win_size or not 3 <= win_size <= 15 or int(win_size) % 2 == 0:
        raise ValueError('win_size %r is not odd or outside 3..15' % (win_size,))
    if not (np.isfinite(sigma) and sigma > 0):
        raise ValueError('sigma %r must be finite and positive' % (sigma,))
    p = int(win_size)
    d = np.arange(p, dtype=np.float64) - (p - 1) / 2.0
    w = np.exp(-(d * d) / (2.0 * float(sigma) * float(sigma)))
    return w / w.sum()


def _ssim_args(shape, data_range, win_size, sigma, k1, k2):
    """The refusals that need no GPU; returns (window as a ctypes array, win_size, c1, c2)."""
    w = ssim_window(win_size, sigma)
    if shape[0] < w.size or shape[1] < w.size:
        raise ValueError('an image of %d x %d is smaller than the %d x %d window' % (shape[0], shape[1], w.size, w.size))
    if not (np.isfinite(data_range) and data_range > 0):
        raise ValueError('data_range %r must be finite and positive' % (data_range,))
    c1, c2 = (float(k1) * float(data_range)) ** 2, (float(k2) * float(data_range)) ** 2
    if not (np.isfinite(c1) and np.isfinite(c2) and c1 > 0 and c2 > 0):
        raise ValueError('k1 = %r and k2 = %r must give finite, positive constants' % (k1, k2))
    return (ctypes.c_double * w.size)(*w.tolist()), int(w.size), c1, c2


def ssim_map_device(x, gt, data_range, win_size=11, sigma=1.5, k1=0.01, k2=0.03):
    """float64 device tensor [H - P + 1, W - P + 1, C] of two [H, W, C] float32 / float64 device tensors (dsen2_ssim_map)."""
    import torch
    from . import _lib, patches
    h, w, c = _check_pair(x, gt)
    win, p, c1, c2 = _ssim_args((h, w, c), data_range, win_size, sigma, k1, k2)
    out = torch.empty((h - p + 1, w - p + 1, c), dtype=torch.float64, device=x.device)
    with torch.cuda.device(x.device):
        _lib.call('dsen2_ssim_map', patches._ptr(x), _lib_dtype(x), patches._ptr(gt), _lib_dtype(gt), h, w, c, win, p, c1, c2,
                  patches._ptr(out), patches._stream(x.device))
    return out


def ssim_sums_device(x, gt, data_range, win_size=11, sigma=1.5, k1=0.01, k2=0.03):
    """[C, 2] float64 device tensor: per band the sum of the SSIM map and the number of windows; the map is never stored."""
    import torch
    from . import _lib, patches
    h, w, c = _check_pair(x, gt)
    win, p, c1, c2 = _ssim_args((h, w, c), data_range, win_size, sigma, k1, k2)
    out = torch.empty((c, 2), dtype=torch.float64, device=x.device)
    with torch.cuda.device(x.device):
        work, nbytes = _quality_workspace(c, x.device)
        _lib.call('dsen2_ssim_sums', patches._ptr(x), _lib_dtype(x), patches._ptr(gt), _lib_dtype(gt), h, w, c, win, p, c1, c2,
                  patches._ptr(work), nbytes, patches._ptr(out), patches._stream(x.device))
    return out


def resample_ssim_sums_device(mid, axis, out_length, taps, gt, data_range, win_size=11, sigma=1.5, k1=0.01, k2=0.03):
    """ssim_sums_device of resize_axis_device(mid, axis, out_length, taps) against gt, in one pass that never stores the resampled
    image (dsen2_imresize_ssim_sums)."""
    import torch
    from . import _lib, patches
    h, w, c = mid.shape
    win, p, c1, c2 = _ssim_args(tuple(gt.shape), data_range, win_size, sigma, k1, k2)
    out = torch.empty((c, 2), dtype=torch.float64, device=mid.device)
    with torch.cuda.device(mid.device):
        work, nbytes = _quality_workspace(c, mid.device)
        _lib.call('dsen2_imresize_ssim_sums', patches._ptr(mid), _lib_dtype(mid), h, w, c, axis, out_length, patches._ptr(taps[0]),
                  patches._ptr(taps[1]), taps[2], patches._ptr(gt), _lib_dtype(gt), win, p, c1, c2, patches._ptr(work), nbytes,
                  patches._ptr(out), patches._stream(mid.device))
    return out


def _ssim_pair_on_device(x, gt, data_range, win_size, sigma, k1, k2):
    x = x if hasattr(x, 'shape') else np.asarray(x)
    gt = gt if hasattr(gt, 'shape') else np.asarray(gt)
    _ssim_args(_check_pair(x, gt), data_range, win_size, sigma, k1, k2)
    x = _device_image(x)
    return x, _device_image(gt, x.device)


def ssim_map(x, gt, data_range, win_size=11, sigma=1.5, k1=0.01, k2=0.03):
    """The SSIM map, float64 ndarray [H - P + 1, W - P + 1, C] (2-D inputs: [H - P + 1, W - P + 1]): Wang et al. 2004 with a Gaussian
    window of win_size weights (odd, 3..15), valid windows only, the biased covariance; data_range is L of C1 = (k1 L)^2."""
    flat = len(np.shape(x)) == 2
    a, b = _ssim_pair_on_device(x, gt, data_range, win_size, sigma, k1, k2)
    q = ssim_map_device(a, b, data_range, win_size, sigma, k1, k2).cpu().numpy()
    return q[:, :, 0] if flat else q


def ssim_sums(x, gt, data_range, win_size=11, sigma=1.5, k1=0.01, k2=0.03):
    """[C, 2] float64 ndarray: per band the sum of the SSIM map and the number of windows."""
    a, b = _ssim_pair_on_device(x, gt, data_range, win_size, sigma, k1, k2)
    return ssim_sums_device(a, b, data_range, win_size, sigma, k1, k2).cpu().numpy()


def bicubic_ssim_sums(lr, gt, scale, data_range, win_size=11, sigma=1.5, k1=0.01, k2=0.03):
    """ssim_sums(imresize(lr, scale), gt, data_range, ...), the same bits, with the second resampling pass computed inside the SSIM
    kernel's loader: the enlarged image is never stored."""
    from . import imresize as ir
    lr = lr if hasattr(lr, 'shape') else np.asarray(lr)
    gt = gt if hasattr(gt, 'shape') else np.asarray(gt)
    _ssim_args(_bicubic_shape(lr, gt, scale), data_range, win_size, sigma, k1, k2)
    lr = _device_image(lr)
    gt = _device_image(gt, lr.device)
    size, scales, order = ir.plan(lr.shape, scalar_scale=scale)
    first, second = order
    mid = ir.resize_axis_device(lr, first, size[first], ir.device_taps(lr.shape[first], size[first], scales[first], lr.device))
    taps = ir.device_taps(mid.shape[second], size[second], scales[second], lr.device)
    return resample_ssim_sums_device(mid, second, size[second], taps, gt, data_range, win_size, sigma, k1, k2).cpu().numpy()


def ssim_scores(sums):
    """(ssim [C], mean over the bands) of a [C, 2] array of sums."""
    sums = np.asarray(sums, np.float64)
    band = sums[:, 0] / sums[:, 1]
    return band, float(np.mean(band))


def SSIM(x, gt, data_range, win_size=11, sigma=1.5, k1=0.01, k2=0.03):
    """(ssim [C] float64 ndarray, its mean over the bands): the structural similarity index of two HWC images."""
    return ssim_scores(ssim_sums(x, gt, data_range, win_size, sigma, k1, k2))


def bicubic_SSIM(lr, gt, scale, data_range, win_size=11, sigma=1.5, k1=0.01, k2=0.03):
    """SSIM of the bicubic enlargement of `lr` by `scale` against `gt`."""
    return ssim_scores(bicubic_ssim_sums(lr, gt, scale, data_range, win_size, sigma, k1, k2))


# ---- ERGAS and PSNR: formulas over the sums of error_sums / bicubic_error_sums, float64 on the host ----

def ergas_score(sums, scale):
    """ERGAS of a [C, 3] array of sums (sum e^2, sum gt, n per band): 100 / scale * sqrt(mean over the bands of mse_c / mean_c^2),
    `scale` being the ratio of the two resolutions (2 for 20 m -> 10 m, 6 for 60 m -> 10 m).  A band whose mean is zero gives
    numpy's inf (nan where its error is zero as well)."""
    sums = np.asarray(sums, np.float64)
    mse = sums[:, 0] / sums[:, 2]
    mean_gt = sums[:, 1] / sums[:, 2]
    with np.errstate(divide='ignore', invalid='ignore'):
        return float(100.0 / scale * np.sqrt(np.mean(mse / (mean_gt * mean_gt))))


def psnr_scores(sums, data_range):
    """(psnr [C], psnr over all bands) in dB of a [C, 3] array of sums: 10 log10(L^2 / mse_c) per band, 10 log10(L^2 / (sum of the
    squared errors / sum of the pixel counts)) overall, L = data_range.  A zero mean squared error gives numpy's inf."""
    sums = np.asarray(sums, np.float64)
    if not (np.isfinite(data_range) and data_range > 0):
        raise ValueError('data_range %r must be finite and positive' % (data_range,))
    peak = float(data_range) * float(data_range)
    with np.errstate(divide='ignore'):
        band = 10.0 * np.log10(peak / (sums[:, 0] / sums[:, 2]))
        total = float(10.0 * np.log10(peak / (sums[:, 0].sum() / sums[:, 2].sum())))
    return band, total


def ERGAS(x, gt, scale):
    """ERGAS (relative dimensionless global error in synthesis) of two HWC images; scale: the resolution ratio."""
    return ergas_score(error_sums(x, gt), scale)


def bicubic_ERGAS(lr, gt, scale):
    """ERGAS of the bicubic enlargement of `lr` by `scale` against `gt`; the enlarged image is never stored."""
    return ergas_score(bicubic_error_sums(lr, gt, scale), scale)


def PSNR(x, gt, data_range):
    """(psnr [C], psnr over all bands) in dB of two HWC images."""
    return psnr_scores(error_sums(x, gt), data_range)


def bicubic_PSNR(lr, gt, scale, data_range):
    """(psnr [C], psnr over all bands) in dB of the bicubic enlargement of `lr` by `scale` against `gt`."""
    return psnr_scores(bicubic_error_sums(lr, gt, scale), data_range)
