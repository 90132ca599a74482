"""python -m dsen2_amd.create_patches — training / test sets from one Sentinel-2 tile: the counterpart of the reference's
training/create_patches.py, with the blur + pixel aggregation, the crops and the up-sampling on the GPU.

    python -m dsen2_amd.create_patches DATA_FILE [--roi_x_y x1,y1,x2,y2] [--test_data] [--run_60] [--true_data]
                                       [--save_prefix ../data/] [--seed N] [--nr_crop N] [--name DIR]

The protocol is the reference's: the 10 m and 20 m (and 60 m) bands are blurred with a Gaussian of sigma = 1/SCALE and averaged over
SCALE x SCALE blocks (SCALE 2; 6 with --run_60), the ORIGINAL 20 m (60 m) bands become the ground truth, and
  (default)     NR_CROP random patches        -> <save_prefix>train/<name>/{data10,data20,data20_gt}.npy
  --run_60                                    -> <save_prefix>train60/<name>/{data10,data20,data60,data60_gt}.npy
  --test_data   the downsampled image, tiled  -> <save_prefix>test/<name>/{data10,data20}.npy, roi.json, no_tiling/*.npy
                (with --run_60: test60/, + data60)
  --true_data   the image itself, tiled       -> <save_prefix>true/<name>/{data10,data20,data60}.npy, roi.json, no_tiling/*.npy
`python -m dsen2_amd.create_random --path <save_prefix>` then marks the validation patches and `python -m dsen2_amd.train --path
<save_prefix>` reads the result.

DATA_FILE: an array file (.npz / .mat, as python -m dsen2_amd.cli reads them; <name> defaults to the file's stem + '.SAFE', so
that the training loader's *SAFE pattern finds it), or a SAFE directory / product file that GDAL opens when `osgeo` is
importable (<name> = the directory's name, as in the reference).  --seed makes the random crops repeatable
(random.Random(seed)); without it they come from the `random` module's global generator like the reference's.
--write_images is accepted and refused: it needs imageio, which this environment does not have.
"""
from __future__ import division

import argparse
import json
import os
import re
import sys

import numpy as np

SCALE20, SCALE60 = 2, 6
BANDS = "B2,B3,B4,B5,B6,B7,B8,B8A,B11,B12"
BANDS_60 = "B1,B2,B3,B4,B5,B6,B7,B8,B8A,B9,B11,B12"
NO_IMAGES = '--write_images is not supported: it needs imageio, which is not installed here; no PNG is written and nothing was done'


def parse_args(argv=None):
    p = argparse.ArgumentParser(prog='python -m dsen2_amd.create_patches', description='Read Sentinel-2 data and create DSen2 training / test patches on the GPU.',
                                formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument('data_file', help='A Sentinel-2 tile: an array file (.npz / .mat) or, with GDAL, a SAFE directory / product file.')
    p.add_argument('--roi_x_y', default='', help='Region of interest as pixel locations on the 10m bands: x_1,y_1,x_2,y_2 (snapped to multiples of 36).')
    p.add_argument('--test_data', default=False, action='store_true', help='Store test patches in a separate dir.')
    p.add_argument('--write_images', default=False, action='store_true', help='Refused (needs imageio).')
    p.add_argument('--save_prefix', default='../data/', help='Prefix of all output files. Use a trailing / to save into a directory.')
    p.add_argument('--run_60', default=False, action='store_true', help='If set, it will create patches also from the 60m channels.')
    p.add_argument('--true_data', default=False, action='store_true', help='If set, it will create patches for S2 without GT.')
    p.add_argument('--seed', type=int, default=None, help='Seed of the random crops (default: the random module\'s global generator).')
    p.add_argument('--nr_crop', type=int, default=None, help='Random patches per tile (default 8000, 500 with --run_60).')
    p.add_argument('--name', default=None, help='Output sub-directory (default: the product\'s name; FILE-STEM.SAFE for an array file).')
    return p.parse_args(argv)


def product_name(data_file):
    """training/create_patches.py:232-236."""
    if data_file.endswith('/'):
        return os.path.split(os.path.split(data_file)[0])[1]
    return os.path.split(data_file)[1]


def _open_arrays(args, roi):
    """(data10, data20, data60, box) of an array file; box = (tmxmin, tmymin, tmxmax, tmymax), None when the ROI is empty."""
    from . import cli
    data10, data20, data60 = cli._load(args.data_file)
    if data10 is None or data20 is None:
        raise ValueError('%s holds no 10 m / 20 m image' % args.data_file)
    if roi:
        box = cli.snap_roi(roi[0], roi[1], roi[2], roi[3], data10.shape[1], data10.shape[0], 36)
    else:
        box = (0, 0, data10.shape[1] - 1, data10.shape[0] - 1)
    _print_region(box)
    xmin, ymin, xmax, ymax = box
    if xmax < xmin or ymax < ymin:
        return None, None, None, None
    want = (BANDS_60 if args.run_60 else BANDS).split(',')
    for key, names in (('10m', cli.BANDS10), ('20m', cli.BANDS20), ('60m', cli.BANDS60)):
        print('Selected %s bands:%s' % (key, ''.join(' ' + n for n in names if n in want)))
    if not args.run_60 and not args.true_data:
        data60 = None
    for a in (data10, data20, data60):
        if a is not None:
            print('Loading selected data from: %s' % args.data_file)
    data10 = data10[ymin:ymax + 1, xmin:xmax + 1]
    data20 = data20[ymin // 2:ymin // 2 + (ymax - ymin + 1) // 2, xmin // 2:xmin // 2 + (xmax - xmin + 1) // 2]
    if data60 is not None:
        data60 = data60[ymin // 6:ymin // 6 + (ymax - ymin + 1) // 6, xmin // 6:xmin // 6 + (xmax - xmin + 1) // 6]
    return data10, data20, data60, box


def _open_product(args, roi):
    """The same through GDAL (cli.GdalProduct with the ROI snapped to 36), or None when osgeo is not importable."""
    from . import cli
    try:
        from osgeo import gdal
    except ImportError:
        print('%s is not an array file (.npz / .mat) and GDAL (osgeo) is not importable: convert the product to .npz (keys data10, '
              'data20, data60)' % args.data_file)
        return None
    path = args.data_file
    if os.path.isdir(path):
        path = os.path.join(path, 'MTD_MSIL1C.xml')                 # training/create_patches.py:15,32
    product = cli.GdalProduct(gdal, path, (BANDS_60 if args.run_60 or args.true_data else BANDS).split(','), roi, snap=36)
    box = (product.xmin, product.ymin, product.xmax, product.ymax)
    _print_region(box)
    if not product.valid:
        return None, None, None, None
    for key in ('10m', '20m', '60m'):
        print('Selected %s bands:%s' % (key, ''.join(' ' + n for n in product.names[key])))
    for key in ('10m', '20m', '60m'):
        if product.index[key]:
            print('Loading selected data from: %s' % product.sub_desc[key])
    return product.read('10m'), product.read('20m'), product.read('60m'), box


def open_tile(data_file, run_60=False, quiet=False):
    """(d10, d20) — (d10, d20, d60) with run_60 — of one whole tile, through the opener DATA_FILE goes through above (an array
    file, or a SAFE product where GDAL is importable); None, with the opener's message printed, when it cannot be opened.  For
    `python -m dsen2_amd.train --tiles`."""
    import contextlib
    import io
    from . import cli
    args = argparse.Namespace(data_file=data_file, run_60=bool(run_60), true_data=False, roi_x_y='')
    is_array = os.path.splitext(data_file)[1].lower() in cli.ARRAY_EXTENSIONS
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf if quiet else sys.stdout):
        opened = _open_arrays(args, None) if is_array else _open_product(args, None)
    if opened is None:
        if quiet:
            sys.stdout.write(buf.getvalue())
        return None
    data10, data20, data60, box = opened
    if box is None:
        print('%s: empty image' % data_file)
        return None
    if run_60 and data60 is None:
        print('%s holds no 60 m image: --run_60 needs one' % data_file)
        return None
    return (data10, data20, data60) if run_60 else (data10, data20)


def _print_region(box):
    xmin, ymin, xmax, ymax = box
    print('Selected UTM Zone:')                                     # (the reference's format string has no placeholder)
    print('Selected pixel region: xmin=%d, ymin=%d, xmax=%d, ymax=%d:' % (xmin, ymin, xmax, ymax))
    print('Selected pixel region: tmxmin=%d, tmymin=%d, tmxmax=%d, tmymax=%d:' % (xmin, ymin, xmax, ymax))
    print('Image size: width=%d x height=%d' % (xmax - xmin + 1, ymax - ymin + 1))


def _out_dir(save_prefix, kind, name):
    out = save_prefix + kind + '/' + name + '/'
    os.makedirs(out, exist_ok=True)
    return out


def readS2fromFile(args):
    from . import cli, patches
    roi = [float(x) for x in re.split(',', args.roi_x_y)] if args.roi_x_y else None
    is_array = os.path.splitext(args.data_file)[1].lower() in cli.ARRAY_EXTENSIONS
    opened = _open_arrays(args, roi) if is_array else _open_product(args, roi)
    if opened is None:
        return 2
    data10, data20, data60, box = opened
    if box is None:
        print('Invalid region of interest / UTM Zone combination')
        return 0
    tmxmin, tmymin, tmxmax, tmymax = box
    need60 = args.run_60 or args.true_data
    if need60 and data60 is None:
        print('%s holds no 60 m image: --run_60 / --true_data need one' % args.data_file)
        return 2
    if int(np.sum(np.asarray(data10[:, :, 0]) < 1)) > 0:
        print('The selected image has some blank pixels')

    name = args.name or (os.path.splitext(os.path.basename(args.data_file))[0] + '.SAFE' if is_array else product_name(args.data_file))
    prefix = args.save_prefix
    dev = patches.default_device()
    # the rasters go up in their own dtype (uint16 as uint16: the downsampler truncates to it after each filter axis)
    gt = [patches.upload_raster(a, dev) if a is not None else None for a in (data10, data20, data60 if need60 else None)]
    as_f32 = lambda td: patches._widen(td[0], td[1]) if td[1] == np.uint16 else td[0]       # noqa: E731
    lr = None
    if not args.true_data:
        scale = SCALE60 if args.run_60 else SCALE20
        lr = [patches.down_pixel_aggr_device(td[0], scale, td[1]) if td is not None else None for td in gt]
    print(name)

    if args.test_data:
        scale = SCALE60 if args.run_60 else SCALE20
        out = _out_dir(prefix, 'test60' if args.run_60 else 'test', name)
        print('Writing files for testing to:{}'.format(out))
        if args.run_60:
            patches.save_test_patches60(lr[0], lr[1], lr[2], out)
        else:
            patches.save_test_patches(lr[0], lr[1], out)
        with open(out + 'roi.json', 'w') as f:
            json.dump([tmxmin // scale, tmymin // scale, (tmxmax + 1) // scale, (tmymax + 1) // scale], f)
        os.makedirs(out + 'no_tiling/', exist_ok=True)
        print('Now saving the whole image without tiling...')
        if args.run_60:
            np.save(out + 'no_tiling/' + 'data60_gt', np.asarray(data60).astype(np.float32))
            np.save(out + 'no_tiling/' + 'data60', lr[2].cpu().numpy())
        else:
            np.save(out + 'no_tiling/' + 'data20_gt', np.asarray(data20).astype(np.float32))     # (the reference's RGB.png needs imageio)
        np.save(out + 'no_tiling/' + 'data10', lr[0].cpu().numpy())
        np.save(out + 'no_tiling/' + 'data20', lr[1].cpu().numpy())
    elif args.true_data:
        out = _out_dir(prefix, 'true', name)
        print('Writing files for testing to:{}'.format(out))
        patches.save_test_patches60(as_f32(gt[0]), as_f32(gt[1]), as_f32(gt[2]), out, patchSize=384, border=12)
        with open(out + 'roi.json', 'w') as f:
            json.dump([tmxmin, tmymin, tmxmax + 1, tmymax + 1], f)
        os.makedirs(out + 'no_tiling/', exist_ok=True)
        print('Now saving the whole image without tiling...')
        for key, a in (('data10', data10), ('data20', data20), ('data60', data60)):
            np.save(out + 'no_tiling/' + key, np.asarray(a).astype(np.float32))
    else:
        out = _out_dir(prefix, 'train60' if args.run_60 else 'train', name)
        print('Writing files for training to:{}'.format(out))
        if args.run_60:
            patches.save_random_patches60(as_f32(gt[2]), lr[0], lr[1], lr[2], out, NR_CROP=args.nr_crop or 500, seed=args.seed)
        else:
            patches.save_random_patches(as_f32(gt[1]), lr[0], lr[1], out, NR_CROP=args.nr_crop or 8000, seed=args.seed)
    print('Success.')
    return 0


def main(argv=None):
    args = parse_args(argv)
    if args.write_images:
        print(NO_IMAGES)
        return 2
    print('I will proceed with file {}'.format(args.data_file))
    try:
        return readS2fromFile(args)
    except ValueError as e:              # an image SCALE does not divide (the reference fails inside downPixelAggr), a bad ROI
        print('Error: %s' % e)
        return 2


if __name__ == '__main__':
    sys.exit(main())
