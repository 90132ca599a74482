"""python -m dsen2_amd.evaluate — score the predictions of `python -m dsen2_amd.train --predict` against the ground truth, beside
the MATLAB-bicubic baseline: the numbers the reference publishes (testing/demoDSen2.py:45-48, 70-73), computed on the GPU.

    python -m dsen2_amd.evaluate --path P [--run_60] [--model_nr s2_038_] [--json OUT] [--uiq] [--sam] [--block_size 8]
                                 [--ssim] [--ergas] [--psnr] [--data_range 10000] [--win_size 11] [--sigma 1.5]

For every directory below <P>/test/ (test60/ with --run_60) that holds no_tiling/ — what `python -m dsen2_amd.create_patches
--test_data` wrote — it loads the ground truth no_tiling/data20_gt.npy (data60_gt) and the downsampled bands no_tiling/data20.npy
(data60) and prints the demo's block

    <name>
    DSen2:
    RMSE: 12.3456          <model_nr>-predict.npy against the ground truth (left out when there is no such file)
    Bicubic:
    RMSE: 23.4567          imresize(downsampled bands, SCALE) against the ground truth

then RMSE and SRE (dB) per band, and after the last tile the mean of each column over all tiles.  --json writes every value
unrounded.  The bicubic baseline never stores the enlarged image: the second resampling pass adds up the errors itself
(metrics.bicubic_error_sums).  The downsampled bands are read as create_patches stores them, float32.

--uiq and --sam add the paper's two further metrics (metrics.UIQ, metrics.SAM; csrc/quality_metrics.hip): a `UIQ` column per
method in every table — the universal image quality index per band over --block_size x --block_size windows (default 8) — and a
`SAM [deg]` line per method, the mean spectral angle; the JSON entries gain band_uiq, uiq (the mean over the bands), sam and
sam_pixels.  The baseline's enlarged image is not stored for these either.  Without the two flags nothing changes.

--ssim, --ergas and --psnr add the rest of the set the super-resolution literature reports.  --ssim: an `SSIM` column per method
and in the mean row — the structural similarity index of Wang et al. 2004 per band (metrics.SSIM; csrc/ssim.hip), a Gaussian window
of --win_size weights (default 11) with --sigma (default 1.5) over valid windows.  --psnr: a `PSNR [dB]` column per band and a
`<method> PSNR [dB]:` line over all bands.  --ergas: a `<method> ERGAS:` line.  SSIM and PSNR measure against --data_range L
(default 10000, the L1C quantification value: reflectance 1.0).  ERGAS and PSNR come from the sums the RMSE needs anyway.  The JSON
entries gain band_ssim, ssim, ergas, band_psnr, psnr, the top level data_range when --ssim or --psnr is given.  Without these flags
nothing changes either.
"""
import argparse
import glob
import json
import os
import sys

import numpy as np

MODEL_NR = 's2_038_'


def parse_args(argv=None):
    p = argparse.ArgumentParser(prog='python -m dsen2_amd.evaluate', description='RMSE / SRE of predicted test sets and of the bicubic baseline, on the GPU.')
    p.add_argument('--path', default='../data/', help='Path of the data (test/ or test60/ below it).')
    p.add_argument('--run_60', action='store_true', help='Score the 60->10m test sets (test60/). Default 20->10m (test/).')
    p.add_argument('--model_nr', default=MODEL_NR, help='Prefix of the prediction files: <model_nr>-predict.npy.')
    p.add_argument('--json', default=None, metavar='OUT', help='Write every value, unrounded, to this file.')
    p.add_argument('--uiq', action='store_true', help='Also the universal image quality index (Wang & Bovik) per band.')
    p.add_argument('--sam', action='store_true', help='Also the spectral angle mapper, in degrees.')
    p.add_argument('--block_size', type=int, default=8, metavar='N', help='Window of the UIQ, N x N (2..16). Default 8.')
    p.add_argument('--ssim', action='store_true', help='Also the structural similarity index (Wang et al. 2004) per band.')
    p.add_argument('--ergas', action='store_true', help='Also ERGAS, the relative dimensionless global error in synthesis.')
    p.add_argument('--psnr', action='store_true', help='Also the peak signal-to-noise ratio in dB, per band and over all bands.')
    p.add_argument('--data_range', type=float, default=10000.0, metavar='L',
                   help='Data range of SSIM and PSNR. Default 10000, the L1C quantification value, i.e. reflectance 1.0.')
    p.add_argument('--win_size', type=int, default=11, metavar='P', help='Gaussian window of the SSIM, P x P (odd, 3..15). Default 11.')
    p.add_argument('--sigma', type=float, default=1.5, help='Standard deviation of that window in pixels. Default 1.5.')
    return p.parse_args(argv)


def _entry(sums):
    from . import metrics
    rmse, sre, total = metrics.scores(sums)
    return {'rmse': total, 'band_rmse': rmse.tolist(), 'band_sre': sre.tolist()}


def _quality(entry, uiq_sums, sam_sums):
    """Adds what --uiq / --sam computed (None: not asked for) to an entry."""
    from . import metrics
    if uiq_sums is not None:
        band, mean = metrics.uiq_scores(uiq_sums)
        entry.update(band_uiq=band.tolist(), uiq=mean)
    if sam_sums is not None:
        entry.update(sam=metrics.sam_score(sam_sums), sam_pixels=int(sam_sums[1]))
    return entry


def _more(entry, sums, scale, ssim_sums, ergas, psnr, data_range):
    """Adds what --ssim / --ergas / --psnr computed to an entry; sums: the error sums its RMSE came from."""
    from . import metrics
    if ssim_sums is not None:
        band, mean = metrics.ssim_scores(ssim_sums)
        entry.update(band_ssim=band.tolist(), ssim=mean)
    if ergas:
        entry.update(ergas=metrics.ergas_score(sums, scale))
    if psnr:
        band, total = metrics.psnr_scores(sums, data_range)
        entry.update(band_psnr=band.tolist(), psnr=total)
    return entry


# further columns of a table: key of the per-band values, heading, key of the value in the mean row (None: left empty)
COLUMNS = (('band_uiq', 'UIQ', 'uiq'), ('band_ssim', 'SSIM', 'ssim'), ('band_psnr', 'PSNR [dB]', None))


def _table(rows, bands):
    cols = [col for col in COLUMNS if all(col[0] in e for _, e in rows)]
    width = 24 + 12 * len(cols)
    print('%-8s' % 'band' + ''.join('%*s' % (width, name) for name, _ in rows))
    print('%-8s' % '' + ''.join('%12s%12s' % ('RMSE', 'SRE [dB]') + ''.join('%12s' % head for _, head, _ in cols) for _ in rows))
    for c in range(bands):
        print('%-8d' % c + ''.join('%12.4f%12.4f' % (e['band_rmse'][c], e['band_sre'][c]) + ''.join('%12.4f' % e[key][c] for key, _, _ in cols)
                                  for _, e in rows))
    if any(mean for _, _, mean in cols):
        print('%-8s' % 'mean' + ''.join('%24s' % '' + ''.join('%12.4f' % e[mean] if mean else '%12s' % '' for _, _, mean in cols)
                                       for _, e in rows).rstrip())
    for name, e in rows:
        if 'sam' in e:
            print('{} SAM [deg]: {:.4f}'.format(name, e['sam']))
    for key, label in (('psnr', 'PSNR [dB]'), ('ergas', 'ERGAS')):
        for name, e in rows:
            if key in e:
                print('{} {}: {:.4f}'.format(name, label, e[key]))


def evaluate_tile(d, run_60, model_nr, uiq=False, sam=False, block_size=8, ssim=False, ergas=False, psnr=False, data_range=10000.0,
                  win_size=11, sigma=1.5):
    """{'bicubic': {...}, 'dsen2': {...} or absent} of one test directory."""
    from . import metrics
    key, scale = ('data60', 6) if run_60 else ('data20', 2)
    gt = np.load(os.path.join(d, 'no_tiling', key + '_gt.npy'))
    lr = np.load(os.path.join(d, 'no_tiling', key + '.npy'))
    if uiq or sam or ssim:
        gt = metrics._device_image(gt)               # several metrics of the same images: one upload of each
        lr = metrics._device_image(lr, gt.device)
    out = {}
    pred = os.path.join(d, model_nr + '-predict.npy')
    if os.path.exists(pred):
        x = np.load(pred)
        if uiq or sam or ssim:
            x = metrics._device_image(x, gt.device)
        sums = metrics.error_sums(x, gt)
        out['dsen2'] = _quality(_entry(sums), metrics.uiq_sums(x, gt, block_size) if uiq else None, metrics.sam_sums(x, gt) if sam else None)
        _more(out['dsen2'], sums, scale, metrics.ssim_sums(x, gt, data_range, win_size, sigma) if ssim else None, ergas, psnr, data_range)
    sums = metrics.bicubic_error_sums(lr, gt, scale)
    out['bicubic'] = _quality(_entry(sums), metrics.bicubic_uiq_sums(lr, gt, scale, block_size) if uiq else None,
                              metrics.bicubic_sam_sums(lr, gt, scale) if sam else None)
    _more(out['bicubic'], sums, scale, metrics.bicubic_ssim_sums(lr, gt, scale, data_range, win_size, sigma) if ssim else None, ergas, psnr,
          data_range)
    return out


def main(argv=None):
    args = parse_args(argv)
    path = args.path if args.path.endswith('/') else args.path + '/'
    folder = 'test60/' if args.run_60 else 'test/'
    tiles = [d for d in sorted(glob.glob(path + folder + '*')) if os.path.isdir(os.path.join(d, 'no_tiling'))]
    if not tiles:
        print('No test set below {} (python -m dsen2_amd.create_patches --test_data writes one)'.format(path + folder))
        return 2
    result = {'model_nr': args.model_nr, 'folder': folder, 'tiles': {}}
    if args.ssim or args.psnr:
        result['data_range'] = args.data_range
    for d in tiles:
        name = os.path.basename(d)
        if args.ssim or args.ergas or args.psnr:
            r = evaluate_tile(d, args.run_60, args.model_nr, args.uiq, args.sam, args.block_size, args.ssim, args.ergas, args.psnr,
                              args.data_range, args.win_size, args.sigma)
        else:
            r = evaluate_tile(d, args.run_60, args.model_nr, args.uiq, args.sam, args.block_size) if args.uiq or args.sam else \
                evaluate_tile(d, args.run_60, args.model_nr)
        result['tiles'][name] = r
        print(name)
        if 'dsen2' in r:
            print('DSen2:')
            print('RMSE: {:.4f}'.format(r['dsen2']['rmse']))
        print('Bicubic:')
        print('RMSE: {:.4f}'.format(r['bicubic']['rmse']))
        rows = [(k, r[k]) for k in ('dsen2', 'bicubic') if k in r]
        _table([({'dsen2': 'DSen2', 'bicubic': 'Bicubic'}[k], e) for k, e in rows], len(r['bicubic']['band_rmse']))
    mean = {}
    for k in ('dsen2', 'bicubic'):
        have = [r[k] for r in result['tiles'].values() if k in r]
        if have:
            mean[k] = {'tiles': len(have), 'rmse': float(np.mean([e['rmse'] for e in have])),
                       'band_rmse': np.mean([e['band_rmse'] for e in have], axis=0).tolist(),
                       'band_sre': np.mean([e['band_sre'] for e in have], axis=0).tolist()}
            if args.uiq:
                mean[k].update(band_uiq=np.mean([e['band_uiq'] for e in have], axis=0).tolist(), uiq=float(np.mean([e['uiq'] for e in have])))
            if args.sam:
                mean[k].update(sam=float(np.mean([e['sam'] for e in have])))
            if args.ssim:
                mean[k].update(band_ssim=np.mean([e['band_ssim'] for e in have], axis=0).tolist(), ssim=float(np.mean([e['ssim'] for e in have])))
            if args.ergas:
                mean[k].update(ergas=float(np.mean([e['ergas'] for e in have])))
            if args.psnr:
                mean[k].update(band_psnr=np.mean([e['band_psnr'] for e in have], axis=0).tolist(), psnr=float(np.mean([e['psnr'] for e in have])))
    result['mean'] = mean
    print('Mean over {} tile(s)'.format(len(tiles)))
    for k, label in (('dsen2', 'DSen2'), ('bicubic', 'Bicubic')):
        if k in mean:
            print('{}: RMSE {:.4f} ({} tile(s))'.format(label, mean[k]['rmse'], mean[k]['tiles']))
    _table([({'dsen2': 'DSen2', 'bicubic': 'Bicubic'}[k], mean[k]) for k in ('dsen2', 'bicubic') if k in mean],
           len(mean['bicubic']['band_rmse']))
    if args.json:
        with open(args.json, 'w') as f:
            json.dump(result, f, indent=1, sort_keys=True)
            f.write('\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
