#!/usr/bin/env python3
"""Fine-tuning speed: one JSON line per configuration.

    python tools/bench_train.py [--config dsen2|vdsen2|both] [--iters N] [--precision fp32|bf16x3] [--mixed_precision bf16]
                                [--shards K [K ...]] [--loss mae|mse|huber|charbonnier] [--loss_param X] [--mask_nodata] [--ssim_weight X]
                                [--optimizer nadam|adam|sgd] [--momentum X] [--nesterov] [--clipnorm X] [--clipvalue X] [--weight_decay X]

  step_ms            one training step on device-resident data: dsen2_model_gradients + dsen2_nadam_step + the device repack
  train_on_batch_ms  S2Model.train_on_batch from host arrays (adds the H2D copies and the loss read-back)
  forward_ms         dsen2_model_forward at the same batch
  patches_per_s      batch / step_ms
  wgrad_tflops       the weight-gradient kernel of one body layer (conv3x3_wgrad.hip) alone, timed with HIP events over
                     `iters` launches through dsen2_conv3x3_wgrad's kernels on device buffers (2 * 9 * F^2 * n*h*w FLOP each)
--precision bf16x3 trains a bf16x3 model: the weight-gradient kernel timed is then conv3x3_wgrad16.hip (dsen2_conv3x3_wgrad_bf16x3
on two-plane operand tensors), counted at three MFMAs per product (3 * 2 * 9 * F^2 * n*h*w FLOP) against the bf16 MFMA peak.
--mixed_precision bf16 (with --precision fp32) trains an fp32 model with compile(mixed_precision='bf16'): the step runs on bf16
operands.  forward_ms stays the model's own fp32 forward; bf16_forward_ms (and step_over_bf16_forward) is dsen2_model_forward of
a precision='bf16' model with the same weights: the arithmetic of the step's forward (inference may take the chain kernel where
the step goes layer by layer).  The weight-gradient kernel timed is the one-plane instance of conv3x3_wgrad16.hip
(dsen2_conv3x3_wgrad_bf16), one MFMA per product (2 * 9 * F^2 * n*h*w FLOP), against the bf16 MFMA peak.
--shards K ...: beside the plain step, shards_step_ms[K] = the same global batch as K shards on device-resident data (K x
dsen2_model_gradients at batch / K, one dsen2_nadam_step_shards, the repack: what train_on_batch(shards=K) and one rank-local
batch of a K-rank data-parallel run cost in kernel efficiency), and train_on_batch_shards_ms[K] from host arrays.
--loss / --loss_param / --mask_nodata: compile()'s loss, loss_param and mask_nodata (default: the MAE, unmasked; the JSON line
then is what it always was).  With --mask_nodata the target gets a blank corner (a quarter of every patch zero in all bands).
--optimizer / --momentum / --nesterov / --clipnorm / --clipvalue / --weight_decay: the optimiser compile() gets (default: a Nadam
without options, whose step is dsen2_nadam_step; the JSON line then is what it always was); anything else steps through
dsen2_optimizer_step, and update_ms is that step alone (the update and the repack, without the gradients).
DSen2 runs at batch 128, VDSen2 at batch 8, both on 32 x 32 patches (training/supres_train.py's batch sizes).
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dsen2_amd import _lib, training, weights  # noqa: E402
from dsen2_amd.DSen2Net import _ptr, _stream_ptr, bf16_plane_f32, s2model, split3_f32  # noqa: E402

PEAK_TF = 157.3   # fp32 MFMA peak of the MI355X (MI355X_MICROARCH.md)
HBM_BYTES_PER_S = 8.0e12   # the MI355X's HBM3E peak, for the floor of a memory-bound kernel
PEAK_TF_BF16 = 2500.0   # dense bf16 MFMA peak
CONFIGS = {'dsen2': dict(d=6, F=128, batch=128), 'vdsen2': dict(d=32, F=256, batch=8)}


def timed(fn, iters, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def make_optimizer(kind=None, momentum=None, nesterov=False, **options):
    options = {k: v for k, v in options.items() if v}
    if kind == 'adam':
        return training.Adam(lr=1e-4, **options)
    if kind == 'sgd':
        return training.SGD(lr=1e-4, momentum=momentum or 0.0, nesterov=nesterov, **options)
    return training.Nadam(lr=1e-4, **options)


def run(name, iters, precision='fp32', mixed_precision=None, shards=(), loss=None, loss_param=None, mask_nodata=False, ssim_weight=0.0,
        optimizer=None):
    c = CONFIGS[name]
    d, F, n, h, w = c['d'], c['F'], c['batch'], 32, 32
    dev = torch.device('cuda', 0)
    m = s2model(((4, None, None), (6, None, None)), num_layers=d, feature_size=F, device=dev, precision=precision)
    m.set_weights_flat(weights.random_he_uniform(10, 6, d, F, seed=1, bias_scale=0.05))
    m.compile(make_optimizer(**(optimizer or {})), loss=loss or 'mean_absolute_error', mixed_precision=mixed_precision, loss_param=loss_param,
              mask_nodata=mask_nodata, ssim_weight=ssim_weight)
    rng = np.random.default_rng(0)
    xs = [rng.uniform(0, 0.5, (n, k, h, w)).astype(np.float32) for k in (4, 6)]
    y = rng.uniform(0, 0.5, (n, 6, h, w)).astype(np.float32)
    if mask_nodata:
        y[:, :, :h // 2, :w // 2] = 0.0
    xs_d = [torch.from_numpy(a).to(dev) for a in xs]
    y_d = torch.from_numpy(y).to(dev)
    st = m._train_state()

    def step():
        m.gradients_device(xs_d, y_d, st['grad'], st['loss2'])
        m.nadam_update(st['grad'])
    step_ms = timed(step, iters)
    tob_ms = timed(lambda: m.train_on_batch(xs, y), max(2, iters // 2), warm=1)
    fwd_ms = timed(lambda: m.forward_device(xs_d), iters)
    extra = {}
    count = m.count_params()
    for k in shards:
        counts = m._shard_counts(n, k)
        firsts = np.cumsum([0] + counts)
        rows = m._shard_rows(k)

        def shard_step():
            for r, c in enumerate(counts):
                if c:
                    f = int(firsts[r])
                    m.gradients_device([t[f:f + c] for t in xs_d], y_d[f:f + c], rows[r, :count], rows[r, count:count + 2])
            m.nadam_update_shards(rows, counts)
        extra.setdefault('shards_step_ms', {})[str(k)] = round(timed(shard_step, iters), 4)
        extra.setdefault('train_on_batch_shards_ms', {})[str(k)] = round(timed(lambda: m.train_on_batch(xs, y, shards=k),
                                                                                  max(2, iters // 2), warm=1), 4)
    if mixed_precision == 'bf16':
        b16 = s2model(((4, None, None), (6, None, None)), num_layers=d, feature_size=F, device=dev, precision='bf16')
        b16.set_weights_flat(m.get_weights_flat())
        b16_ms = timed(lambda: b16.forward_device(xs_d), iters)
        extra.update(mixed_precision=mixed_precision, bf16_forward_ms=round(b16_ms, 4), step_over_bf16_forward=round(step_ms / b16_ms, 3))
        del b16

    # the weight-gradient kernel of one body layer, through the library's launcher on preallocated buffers
    a = torch.from_numpy(rng.uniform(-1, 1, (n, h, w, F)).astype(np.float32)).to(dev)
    g = torch.from_numpy(rng.uniform(-1, 1, (n, h, w, F)).astype(np.float32)).to(dev)
    dw = torch.empty(9 * F * F, device=dev)
    db = torch.empty(F, device=dev)

    x3 = precision == 'bf16x3'
    amp = mixed_precision == 'bf16'
    if x3:
        a, g = split3_f32(a)[0], split3_f32(g)[0]
    if amp:
        a, g = bf16_plane_f32(a), bf16_plane_f32(g)

    def wgrad():
        if amp:
            _lib.call('dsen2_conv3x3_wgrad_bf16', _ptr(a), _ptr(g), _ptr(dw), _ptr(db), n, h, w, F, 1.0, _stream_ptr(dev))
        elif x3:
            _lib.call('dsen2_conv3x3_wgrad_bf16x3', _ptr(a), _ptr(g), _ptr(dw), _ptr(db), n, h, w, F, 1.0, _stream_ptr(dev))
        else:
            _lib.call('dsen2_conv3x3_wgrad', _ptr(a), _ptr(g), _ptr(dw), _ptr(db), n, h, w, F, F, F, F, 1.0, _stream_ptr(dev))
    # dsen2_conv3x3_wgrad allocates its scratch and synchronises on every call: its kernels' share is what a HIP-event pair
    # around the call measures minus that overhead, so the kernels are timed from a rocprofv3 kernel trace instead when one
    # is given (profiles/); here: the call's wall time, an upper bound of the kernel time
    wg_ms = timed(wgrad, iters, warm=2)
    flop = (3.0 if x3 else 1.0) * 2.0 * 9 * F * F * n * h * w
    peak = PEAK_TF_BF16 if x3 or amp else PEAK_TF
    res = dict(config=name, precision=precision, batch=n, h=h, w=w, num_layers=d, feature_size=F, step_ms=round(step_ms, 4),
               train_on_batch_ms=round(tob_ms, 4), forward_ms=round(fwd_ms, 4), step_over_forward=round(step_ms / fwd_ms, 3),
               patches_per_s=round(n / step_ms * 1e3, 1), wgrad_call_ms=round(wg_ms, 4),
               wgrad_tflops_lower_bound=round(flop / wg_ms / 1e9, 2), wgrad_fraction_of_peak_lower_bound=round(flop / wg_ms / 1e9 / peak, 4))
    res.update(extra)
    if loss is not None or mask_nodata:
        res.update(loss=loss or 'mae', loss_param=loss_param, mask_nodata=bool(mask_nodata))
    if ssim_weight:
        # the term's kernel alone through its test entry, which allocates its scratch and synchronises on every call: an upper
        # bound of the kernel time (the step with the weight at 0 is the other way to read it); and its HBM floor: out and target
        # read, the NHWC16 gradient read and written
        from dsen2_amd import losses
        window, c1, c2 = losses.ssim_constants(losses.ssim_part(m.loss_setting))
        cwin = (ctypes.c_double * window.size)(*window.tolist())
        out_d = torch.from_numpy(rng.uniform(0, 0.5, y.shape).astype(np.float32)).to(dev)
        g16 = torch.zeros((n * h * w, 16), device=dev)
        sums2 = torch.zeros(2, dtype=torch.float64, device=dev)
        call_ms = timed(lambda: _lib.call('dsen2_ssim_loss_grad', _ptr(out_d), _ptr(y_d), n, 6, h, w, float(ssim_weight), cwin,
                                          int(window.size), c1, c2, int(bool(mask_nodata)), _ptr(g16), _ptr(sums2), _stream_ptr(dev)),
                        iters, warm=2)
        hbm_bytes = 2 * y.size * 4 + 2 * g16.numel() * 4
        res.update(ssim_weight=ssim_weight, ssim_loss_call_ms=round(call_ms, 4), ssim_loss_hbm_bytes=hbm_bytes,
                   ssim_loss_hbm_floor_ms=round(hbm_bytes / HBM_BYTES_PER_S * 1e3, 5))
    if not m._plain_nadam():
        opt = m.optimizer
        res.update(optimizer=type(opt).__name__.lower(), clipnorm=opt.clipnorm, clipvalue=opt.clipvalue, weight_decay=opt.weight_decay,
                   update_ms=round(timed(lambda: m.nadam_update(st['grad']), iters), 4))
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--config', default='both', choices=['dsen2', 'vdsen2', 'both'])
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--precision', default='fp32', choices=['fp32', 'bf16x3'])
    ap.add_argument('--mixed_precision', default=None, choices=['bf16'])
    ap.add_argument('--shards', type=int, nargs='+', default=[], help='also time the step as K shards of the same global batch')
    ap.add_argument('--loss', default=None, choices=['mae', 'mse', 'huber', 'charbonnier'])
    ap.add_argument('--loss_param', type=float, default=None)
    ap.add_argument('--mask_nodata', action='store_true')
    ap.add_argument('--ssim_weight', type=float, default=0.0, help="compile()'s ssim_weight (window 11, sigma 1.5, data range 5.0)")
    ap.add_argument('--optimizer', default=None, choices=['nadam', 'adam', 'sgd'])
    ap.add_argument('--momentum', type=float, default=None)
    ap.add_argument('--nesterov', action='store_true')
    ap.add_argument('--clipnorm', type=float, default=0.0)
    ap.add_argument('--clipvalue', type=float, default=0.0)
    ap.add_argument('--weight_decay', type=float, default=0.0)
    args = ap.parse_args()
    if args.mixed_precision and args.precision != 'fp32':
        ap.error('--mixed_precision is an option of --precision fp32')
    optimizer = dict(kind=args.optimizer, momentum=args.momentum, nesterov=args.nesterov, clipnorm=args.clipnorm, clipvalue=args.clipvalue,
                     weight_decay=args.weight_decay)
    for name in (['dsen2', 'vdsen2'] if args.config == 'both' else [args.config]):
        run(name, args.iters, args.precision, args.mixed_precision, args.shards, args.loss, args.loss_param, args.mask_nodata, args.ssim_weight,
            optimizer)


if __name__ == '__main__':
    main()
