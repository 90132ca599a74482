"""python -m dsen2_amd.train — fine-tune DSen2 / VDSen2 on the GPU: the counterpart of training/supres_train.py.

Keeps that script's flags (--path, --resume, --run_60, --deep) and its recipe: MAE loss with MSE as a metric, keras-2 Nadam
(beta_1 0.9, beta_2 0.999, epsilon 1e-8, schedule_decay 0.004), ReduceLROnPlateau (factor 0.5, patience 5, min_delta 1e-6,
cooldown 20, min_lr 1e-5), best-only checkpointing on val_loss, shuffled epochs.  Each run writes

  <out>/<model_nr>lr_<lr>.npy       the best-val_loss weights, flat (weights.load_flat reads it; DSen2_20 / DSen2_60 pick it up
                                    in place of a missing .hdf5 of the same name)
  <out>/<model_nr>_lr_<lr>.txt      one line per epoch: loss, val_loss, lr

One GPU unless --data_parallel is given (below).  --precision fp32 (default) trains in fp32; --precision bf16x3 runs the forward and the residual blocks' backward
on the bf16 matrix cores with fp32-grade products (three bf16 MFMAs each).  --mixed_precision bf16 (default off, fp32 models only:
refused together with --precision bf16x3) is ordinary mixed-precision training: the step's convolutions run on bf16 operands with
fp32 accumulation, the arithmetic `--precision bf16` inference uses (one bf16 MFMA per product, ~1e-3 relative error per
convolution, no loss scaling: bf16 has fp32's exponent), while validation, the model and everything stored stay fp32.  The master
weights, the optimizer and the checkpoint are fp32 in every case, so a checkpoint loads into a model of any precision.
Data: <path>/train/*SAFE/{data10,data20,data20_gt}.npy (train60/ and data60, data60_gt with
--run_60) and val_index.npy, as `python -m dsen2_amd.create_patches` and `python -m dsen2_amd.create_random` write them (the
counterparts of training/create_patches.py and create_random.py, whose files it reads just the same).

    python -m torch.distributed.run --nnodes=1 --nproc-per-node N -m dsen2_amd.train --data_parallel [--backend nccl|gloo] ...
trains on N GPUs, one process each (S2Model.fit(data_parallel=True)): --batch_size is the GLOBAL batch, of which every rank
takes its dist.shard_range share; the ranks all-gather their gradient vectors and take the same step on the count-weighted mean,
added in rank order, so every rank holds the same weights bit for bit and an N-rank run writes the files a one-process run of
fit(data_parallel=True, emulate_world=N) writes, byte for byte.  --resume is read by rank 0 alone; the checkpoint, the epoch log
and the progress line are rank 0's; ReduceLROnPlateau runs on every rank, on identical numbers.  Every rank loads the whole
training set into host memory (a global permutation can ask any rank for any sample), and the all-gather is not overlapped with
the backward pass.  --backend gloo rehearses the control flow with ranks sharing GPUs.  Without --data_parallel a launch with
WORLD_SIZE > 1 is refused; with it, a single process trains exactly as without.  --data_parallel --emulate_world N in a single
process is fit(data_parallel=True, emulate_world=N): the N-rank run restated on one GPU (its files, without its speed).

--augment (not in the reference; default off) turns every training sample of every step by one of the 8 flips and rotations of the
square, inputs and target alike, on the GPU after the upload (S2Model.fit(augment=True); training.AugmentOps draws the ops from
--seed on a stream of its own, so the epoch permutations do not change; square patches; validation is never augmented).  Under
--data_parallel every rank draws the ops of the global batch, so an N-rank run still equals its one-process restatement.

    python -m dsen2_amd.train --tiles F [F ...] [--steps_per_epoch N] [--val_crops M] ...
trains from tiles instead of from files of crops (not in the reference): every F is a tile as `python -m dsen2_amd.create_patches
DATA_FILE` opens it (.npz / .mat, or a SAFE product where GDAL is importable; the same opener).  The tiles are downsampled on the GPU
and stay there with their ground truth (corpus.TileCorpus; about 1 GB per 10980^2 tile), and every step's batch is cut from them on
the GPU — fresh random crops each step, uniform over the tiles (S2Model.fit_corpus).  An epoch is --steps_per_epoch batches
(default: as many crops as the reference's files hold, 8000 per tile, 500 with --run_60); validation is --val_crops fixed crops per
tile (default a tenth of that), drawn once from --seed.  All other flags keep their meaning, --augment (the ops are drawn with the
crops) and --data_parallel / --emulate_world included: every rank holds the whole corpus in ITS GPU's memory, draws the crops of the
global batch and cuts its own share, so no rank needs the training set in host memory; with more than one rank --seed is required
(the validation crops must be the same everywhere).  The log and the checkpoint are the same files.  --tiles and a training set
under --path exclude each other.
With --tiles only (each without it is an error; with none of them the log and the checkpoint are the bytes they always were):
--skip_blank draws no crop, training or validation, that touches a blank cell — a cell of the origin grid with a band-0 sample of
the 10 m raster < 1, the reference's `chan3 < 1`; no other band is looked at — and prints how many origins each tile keeps;
--holdout [--holdout_margin K] keeps the training crops out of the validation crops (and K cells around them); --val_on_device
validates from the table of validation crops on the GPU and builds no host arrays.  Tiles stay uniform: a tile is not weighted by
its valid area; a tile left with fewer than 1 valid origin in 64 is refused.  Under --data_parallel every rank builds the same
masks from its own copy of the corpus and the same --seed.

--mask_key NAME [--mask_classes 0,1,3,8,9,10] [--mask_dilate N] [--skip_masked] (with --tiles; not in the reference): NAME is an
array in each tile's .npz — a 2-D uint8 class raster on the 10, 20 or 60 m grid: Sentinel-2's SCL layer, a cloud-probability
layer — and a tile without it has no mask.  Pixels of the listed classes (default: SCL no data, saturated or defective, cloud
shadow, cloud medium and high probability, thin cirrus), grown by N ground-truth pixels (0..32), become no-data in the tile's ground
truth on the GPU (corpus.TileCorpus(class_masks=)); --mask_key implies --mask_nodata, and says so, because a mask the loss ignored
would train on zeros.  --skip_masked also draws no crop, training or validation, that touches a masked pixel.

--loss {mae,mse,huber,charbonnier} [--loss_param X] [--mask_nodata] (not in the reference; without them the output, the log and
the checkpoint are the bytes they always were) choose what is minimised (S2Model.compile(loss=, loss_param=, mask_nodata=);
losses.py has the table): --loss_param is Huber's delta / Charbonnier's epsilon in the reflectance / 2000 domain, required for
those two and refused otherwise; --mask_nodata keeps every pixel whose target is 0 in all bands — the fill of a swath edge or a
tile corner, which prediction blanks by itself — out of the loss, the validation loss and every gradient (the denominator stays
the number of all elements).  The epoch log's loss and valid columns, ReduceLROnPlateau and the checkpoint follow the chosen loss;
min_delta stays 1e-6, which is large beside an MSE in this domain.  They work with --path and --tiles, every precision flag,
--data_parallel and --emulate_world; a line at start-up names the loss.

--ssim_weight X [--ssim_win 11] [--ssim_sigma 1.5] [--ssim_data_range 5.0] add Zhao et al. 2017's term, X times the mean over all
windows of (1 - SSIM), to whatever --loss chose (S2Model.compile(ssim_weight=, ...); the gradient is a GPU kernel of its own).  The
window is odd, 3..11; the data range lives in the reflectance / 2000 domain.  Patches must be at least the window on a side.  With
--mask_nodata a window that holds a masked pixel adds nothing.  The loss and valid columns are then the total that is minimised.

--optimizer {nadam,adam,sgd} [--momentum X] [--nesterov] [--clipnorm X] [--clipvalue X] [--weight_decay X] (not in the reference,
whose Nadam call carries a commented-out clipvalue=; with none of them the log and the checkpoint are the bytes they always were)
choose the update rule and bound or regularise the step (training.Nadam / Adam / SGD; the step is one GPU kernel,
dsen2_optimizer_step): adam and sgd are keras 2.2's (no amsgrad, no decay=; --momentum in [0, 1) and --nesterov belong to sgd);
--clipnorm scales the gradient to the norm X when its global norm over ALL weights is larger (formed on the GPU in a fixed order;
the host never waits for it), --clipvalue then clamps every element to [-X, X]; --weight_decay is decoupled (AdamW's): after every
step p -= lr * X * p on the convolution kernels, never on the biases.  They work with every other training flag, --data_parallel
and --emulate_world included: every rank forms the same norm from the same gathered gradients.  A line at start-up names them.
The optimiser's state is not in the checkpoint: --resume starts it fresh, as keras does after compile().

    python -m dsen2_amd.train --predict FILE [--true] [--run_60] [--deep] [--self_ensemble] [--mask M ...] --path P
is that script's predict branch (--self_ensemble, not in the reference: predict(ensemble=True), the mean over the 8 flips and
rotations of every patch; --augment is refused here): for every *SAFE directory (sorted) under <P>/test/ (test60/ with --run_60, true/ with --true) it
loads the tiled test set (patches.OpenDataFilesTest), runs predict(batch_size=8), recomposes the image (border 4; 12 for test60/
and true/), multiplies by SCALE = 2000 and writes <P>/<folder>/<dset>/<model_nr>-predict.npy, model_nr being the seven
characters in front of 'lr_1e-04' in FILE's name (model_number).  `python -m dsen2_amd.evaluate` scores those files.
--mask NAME_OR_FILE [--mask_classes ...] [--mask_dilate N] (with --predict; not in the reference): a .npy class raster — a file of
that name in every test-set directory, or one file given by its path — whose invalid pixels (as above; N in pixels of the image)
are written as 0 in every band of the recomposed image, on the GPU.
DECISION: the reference hands recompose_images `image_size` = [width, height] as read from roi.json, where that function takes
(rows, columns).  For a square region the two agree, and that is what the recorded behaviour pins; for any other region the
reference recomposes a transposed canvas.  Here recompose_images always gets (rows, columns) = (height, width), so a non-square
region predicts to the shape of its ground truth.
"""
import argparse
import glob
import os
import sys
import time

MODEL_NR = 's2_038_'    # training/supres_train.py: prefix of a new training
SCALE = 2000


def parse_args(argv=None):
    p = argparse.ArgumentParser(prog='python -m dsen2_amd.train', description='Fine-tune DSen2 / VDSen2 on the GPU (SupResS2).')
    p.add_argument('--predict', action='store', dest='predict_file', help='Predict: the test sets below --path with these weights (.hdf5 / .npy).')
    p.add_argument('--true', action='store_true', help='Use true scale data. No simulation or different resolutions.')
    p.add_argument('--resume', action='store', dest='resume_file', help='Resume training from these weights (.hdf5 / .npy).')
    p.add_argument('--run_60', action='store_true', help='Train a 60->10m network. Default 20->10m.')
    p.add_argument('--deep', action='store_true', help='VDSen2: 32 blocks of 256 features, batch 8 (default DSen2: 6 x 128, batch 128).')
    p.add_argument('--path', default='../data/', help='Path of the data (train/ or train60/ below it).')
    p.add_argument('--epochs', type=int, default=8 * 1024, help='Epochs (default 8192, as the reference).')
    p.add_argument('--lr', type=float, default=1e-4, help='Initial learning rate (default 1e-4).')
    p.add_argument('--batch_size', type=int, default=None, help='Batch size (default 128, 8 with --deep).')
    p.add_argument('--out', default=None, help='Output directory (default <path>/network_data/).')
    p.add_argument('--seed', type=int, default=None, help='Seed of the epoch shuffles.')
    p.add_argument('--precision', choices=('fp32', 'bf16x3'), default='fp32',
                   help='Arithmetic of the residual blocks while training (default fp32); checkpoints are fp32 either way.')
    p.add_argument('--mixed_precision', choices=('bf16',), default=None,
                   help='Run the training step of an fp32 model on bf16 operands, fp32 accumulate (default off; not with --precision bf16x3).')
    p.add_argument('--data_parallel', action='store_true',
                   help='Data-parallel training under torch.distributed.run: one process per GPU, --batch_size is the global batch.')
    p.add_argument('--backend', choices=('nccl', 'gloo'), default='nccl',
                   help='Collectives of --data_parallel: nccl (RCCL, default) or gloo (a rehearsal with ranks sharing GPUs).')
    p.add_argument('--emulate_world', type=int, default=None, metavar='N',
                   help='With --data_parallel in ONE process: compute what an N-rank run computes, bit for bit, shard after shard.')
    p.add_argument('--augment', action='store_true',
                   help='Training: flip and rotate every sample of every step at random (the 8 symmetries of the square, inputs and '
                        'target alike, on the GPU; square patches).  Validation is never augmented.')
    p.add_argument('--tiles', nargs='+', default=None, metavar='F',
                   help='Train from these tiles (as create_patches DATA_FILE opens them), kept on the GPU; batches are cut there.')
    p.add_argument('--steps_per_epoch', type=int, default=None, metavar='N',
                   help='With --tiles: batches per epoch (default: 8000 crops per tile, 500 with --run_60, over the batch size).')
    p.add_argument('--val_crops', type=int, default=None, metavar='M',
                   help='With --tiles: fixed validation crops per tile (default 800, 50 with --run_60).')
    p.add_argument('--skip_blank', action='store_true',
                   help='With --tiles: draw no crop (training or validation) that touches a blank cell: band 0 of the 10 m raster < 1.')
    p.add_argument('--holdout', action='store_true',
                   help='With --tiles: keep the training crops out of the validation crops (no training crop overlaps one).')
    p.add_argument('--holdout_margin', type=int, default=None, metavar='K',
                   help='With --holdout: also keep K cells of the origin grid around every validation crop free (default 0).')
    p.add_argument('--val_on_device', action='store_true',
                   help='With --tiles: validate from the table of validation crops on the GPU; no host arrays are built.')
    p.add_argument('--loss', choices=('mae', 'mse', 'huber', 'charbonnier'), default=None,
                   help='Training: the loss to minimise (default mae, the mean absolute error of the reference).')
    p.add_argument('--loss_param', type=float, default=None, metavar='X',
                   help='With --loss huber / charbonnier (required there): delta / epsilon, in the reflectance / 2000 domain.')
    p.add_argument('--mask_nodata', action='store_true',
                   help='Training: a pixel whose target is 0 in every band carries no ground truth: it adds nothing to the loss, '
                        'the validation loss or any gradient.')
    p.add_argument('--ssim_weight', type=float, default=0.0, metavar='X',
                   help='Training: add X * mean over all windows of (1 - SSIM) to the loss (default 0: no such term).')
    p.add_argument('--ssim_win', type=int, default=11, metavar='P', help='With --ssim_weight: the window, odd, 3..11 (default 11).')
    p.add_argument('--ssim_sigma', type=float, default=1.5, help="With --ssim_weight: the Gaussian window's sigma (default 1.5).")
    p.add_argument('--ssim_data_range', type=float, default=5.0, metavar='L',
                   help='With --ssim_weight: the data range of c1 = (0.01 L)^2, c2 = (0.03 L)^2 in the reflectance / 2000 domain '
                        '(default 5.0 = 10000 / 2000).')
    p.add_argument('--optimizer', choices=('nadam', 'adam', 'sgd'), default=None,
                   help="Training: the update rule (default nadam, the reference's keras-2 Nadam; adam and sgd are keras 2.2's).")
    p.add_argument('--momentum', type=float, default=None, metavar='X', help='With --optimizer sgd: the momentum, in [0, 1) (default 0).')
    p.add_argument('--nesterov', action='store_true', help='With --optimizer sgd: Nesterov momentum.')
    p.add_argument('--clipnorm', type=float, default=None, metavar='X',
                   help='Training: scale the gradient to the global norm X when its norm over all weights is larger (default off).')
    p.add_argument('--clipvalue', type=float, default=None, metavar='X',
                   help='Training: clamp every gradient element to [-X, X], after --clipnorm (default off).')
    p.add_argument('--weight_decay', type=float, default=None, metavar='X',
                   help='Training: decoupled weight decay, p -= lr * X * p after every step, on the convolution kernels (default off).')
    p.add_argument('--self_ensemble', action='store_true',
                   help='With --predict: average the predictions for the 8 flips and rotations of every patch (~8x the network time).')
    p.add_argument('--feather', type=int, default=None, metavar='F',
                   help='With --predict: blend neighbouring patches across F pixels either side of every seam when the image is '
                        "recomposed, 1 <= F <= the border of the patch files (default: the reference's hard cut).")
    p.add_argument('--mask_key', default=None, metavar='NAME',
                   help="With --tiles: the array of each tile's .npz that holds its class raster (2-D uint8: SCL, cloud probability); its "
                        'invalid pixels become no-data in the ground truth.  Implies --mask_nodata.')
    p.add_argument('--mask', default=None, metavar='NAME_OR_FILE',
                   help='With --predict: a .npy class raster (a name inside every test-set directory, or a path); its invalid pixels '
                        'are written as 0.')
    p.add_argument('--mask_classes', default=None, metavar='C,C,...',
                   help='With --mask_key / --mask: the class values that are invalid (default 0,1,3,8,9,10 of the SCL layer).')
    p.add_argument('--mask_dilate', type=int, default=None, metavar='N',
                   help='With --mask_key / --mask: grow the invalid area by N pixels (ground-truth pixels; 0..32, default 0).')
    p.add_argument('--skip_masked', action='store_true',
                   help='With --mask_key: draw no crop (training or validation) that touches a masked pixel.')
    args = p.parse_args(argv)
    if args.mask_key is not None and args.tiles is None:
        p.error('--mask_key is an option of --tiles')
    if args.mask is not None and not args.predict_file:
        p.error('--mask is an option of --predict (training from tiles takes --mask_key)')
    if args.skip_masked and args.mask_key is None:
        p.error('--skip_masked is an option of --mask_key')
    if args.mask_key is None and args.mask is None and (args.mask_classes is not None or args.mask_dilate is not None):
        p.error('--mask_classes and --mask_dilate are options of --mask_key and --mask')
    if args.mask_dilate is not None and not 0 <= args.mask_dilate <= 32:
        p.error('--mask_dilate N: N is in pixels, 0..32')
    if args.mask_classes is not None:
        from . import masks
        try:
            args.mask_classes = masks.parse_classes(args.mask_classes)
        except ValueError as e:
            p.error(str(e))
    if args.feather is not None and (not args.predict_file or args.feather < 1):
        p.error('--feather F (F >= 1) is an option of --predict')
    if args.augment and args.predict_file:
        p.error('--augment is an option of training: it cannot be combined with --predict')
    if args.predict_file and (args.loss is not None or args.loss_param is not None or args.mask_nodata):
        p.error('--loss, --loss_param and --mask_nodata are options of training: they cannot be combined with --predict')
    if args.loss in ('huber', 'charbonnier') and not (args.loss_param is not None and 0 < args.loss_param < float('inf')):
        p.error('--loss %s needs --loss_param X with a finite X > 0' % args.loss)
    if args.loss_param is not None and args.loss not in ('huber', 'charbonnier'):
        p.error('--loss_param is an option of --loss huber and --loss charbonnier')
    if args.predict_file and args.ssim_weight:
        p.error('--ssim_weight is an option of training: it cannot be combined with --predict')
    if not 0.0 <= args.ssim_weight < float('inf'):
        p.error('--ssim_weight must be finite and >= 0')
    if args.ssim_win % 2 == 0 or not 3 <= args.ssim_win <= 11:
        p.error('--ssim_win must be odd and in 3..11')
    if not (0.0 < args.ssim_sigma < float('inf') and 0.0 < args.ssim_data_range < float('inf')):
        p.error('--ssim_sigma and --ssim_data_range must be finite and > 0')
    step_flags = [args.optimizer, args.momentum, args.clipnorm, args.clipvalue, args.weight_decay]
    if args.predict_file and (any(f is not None for f in step_flags) or args.nesterov):
        p.error('--optimizer, --momentum, --nesterov, --clipnorm, --clipvalue and --weight_decay are options of training: they cannot '
                'be combined with --predict')
    if (args.momentum is not None or args.nesterov) and args.optimizer != 'sgd':
        p.error('--momentum and --nesterov are options of --optimizer sgd')
    if args.momentum is not None and not 0.0 <= args.momentum < 1.0:
        p.error('--momentum must be in [0, 1)')
    for name in ('clipnorm', 'clipvalue', 'weight_decay'):
        x = getattr(args, name)
        if x is not None and not 0.0 < x < float('inf'):
            p.error('--%s must be finite and > 0' % name)
    if args.self_ensemble and not args.predict_file:
        p.error('--self_ensemble is an option of --predict')
    if args.tiles is None and (args.steps_per_epoch is not None or args.val_crops is not None):
        p.error('--steps_per_epoch and --val_crops are options of --tiles')
    if args.tiles is None and (args.skip_blank or args.holdout or args.val_on_device or args.holdout_margin is not None):
        p.error('--skip_blank, --holdout, --holdout_margin and --val_on_device are options of --tiles')
    if args.holdout_margin is not None and (not args.holdout or args.holdout_margin < 0):
        p.error('--holdout_margin K (K >= 0) is an option of --holdout')
    if args.tiles is not None and args.predict_file:
        p.error('--tiles is an option of training: it cannot be combined with --predict')
    if args.tiles is not None and ((args.steps_per_epoch is not None and args.steps_per_epoch < 1) or
                                   (args.val_crops is not None and args.val_crops < 1)):
        p.error('--steps_per_epoch and --val_crops must be at least 1')
    if args.emulate_world is not None and (not args.data_parallel or args.emulate_world < 1):
        p.error('--emulate_world N (N >= 1) restates a --data_parallel run in one process: pass --data_parallel too')
    if args.mixed_precision is not None and args.precision != 'fp32':
        p.error('--mixed_precision %s is an option of --precision fp32 (got --precision %s)' % (args.mixed_precision, args.precision))
    return args


def model_number(resume_file):
    """The reference's args.resume_file[-20:-13] for 's2_032_lr_1e-04.hdf5', for any extension."""
    stem = os.path.splitext(os.path.basename(resume_file))[0]
    return stem[-15:-8]


def predict(model, args, path):
    """training/supres_train.py:149-179."""
    import numpy as np
    from . import patches
    if args.true:
        folder, border = 'true/', 12
    elif args.run_60:
        folder, border = 'test60/', 12
    else:
        folder, border = 'test/', 4
    model_nr = model_number(args.predict_file)
    print('Changing the model number to: {}'.format(model_nr))
    model.load_weights(args.predict_file)
    print('Predicting using file: {}'.format(args.predict_file))
    for dset in [os.path.basename(x) for x in sorted(glob.glob(path + folder + '*SAFE'))]:
        start = time.time()
        print('Timer started.')
        print('Predicting: {}.'.format(dset))
        train, image_size = patches.OpenDataFilesTest(path + folder + dset, args.run_60, SCALE, args.true)
        if args.self_ensemble:
            prediction = model.predict(train, batch_size=8, verbose=1, ensemble=True)
        else:
            prediction = model.predict(train, batch_size=8, verbose=1)
        size = (image_size[1], image_size[0])                                                                 # (rows, columns): see above
        if args.feather:
            images = patches.recompose_images(prediction, border=border, size=size, feather=args.feather)
        else:
            images = patches.recompose_images(prediction, border=border, size=size)
        if args.mask:
            from . import masks
            in_dset = os.path.join(path + folder + dset, args.mask if args.mask.lower().endswith('.npy') else args.mask + '.npy')
            images = masks.apply_to_image(images, np.load(in_dset if os.path.exists(in_dset) else args.mask), args.mask_classes,
                                          args.mask_dilate or 0)
        print('Writing to file...')
        np.save(path + folder + dset + '/' + model_nr + '-predict', images * SCALE)
        print('Elapsed time: {}.'.format(time.time() - start))
    return 0


TILES_AND_PATH = '--tiles and a training set under --path exclude each other: {} holds {} *SAFE director{} of crops'


def tiles_conflict(args, path):
    """The message when --tiles meets a populated training set under --path, else None."""
    train_dir = path + ('train60' if args.run_60 else 'train')
    found = glob.glob(os.path.join(train_dir, '*SAFE'))
    if args.tiles is not None and found:
        return TILES_AND_PATH.format(train_dir, len(found), 'y' if len(found) == 1 else 'ies')
    return None


def tile_class_mask(tile_file, key):
    """The array `key` of the tile's .npz (--mask_key), or None for a tile that has none."""
    import numpy as np
    if not tile_file.lower().endswith('.npz'):
        return None
    z = np.load(tile_file)
    return z[key] if key in z else None


def tiles_validation(corpus, args, crops_per_tile, say=print):
    """(validation table, training masks or None, validation host arrays or None) of a --tiles run.  The table is drawn ONCE
    (without --seed it comes from fresh entropy: a second draw would be other crops) and everything is derived from that one table:
    the hold-out masks of --holdout, the host arrays (cut from it, unless --val_on_device) and fit_corpus's validation_crops.  Every
    rank builds the same masks from its own copy of the corpus and the same --seed."""
    blank = corpus.origin_masks()[0] if args.skip_blank or getattr(args, 'skip_masked', False) else None
    masks = blank
    val_table = corpus.validation_table(crops_per_tile, args.seed, blank)
    if args.holdout:
        masks, left = corpus.origin_masks(holdout=val_table, margin=args.holdout_margin or 0)
        say('Hold-out: training crops are drawn from {} origins outside the validation crops.'.format(sum(left)))
    arrays = None if args.val_on_device else corpus.table_arrays(val_table)
    return val_table, masks, arrays


def make_optimizer(args):
    """The optimiser of the run: without --optimizer and its options the reference's Nadam, constructed as it always was."""
    from . import training
    options = {k: getattr(args, k) for k in ('clipnorm', 'clipvalue', 'weight_decay') if getattr(args, k, None) is not None}
    kind = getattr(args, 'optimizer', None) or 'nadam'
    if kind == 'adam':
        return training.Adam(lr=args.lr, beta_1=0.9, beta_2=0.999, epsilon=1e-8, **options)
    if kind == 'sgd':
        return training.SGD(lr=args.lr, momentum=args.momentum or 0.0, nesterov=args.nesterov, **options)
    return training.Nadam(lr=args.lr, beta_1=0.9, beta_2=0.999, epsilon=1e-8, schedule_decay=0.004, **options)


def describe_optimizer(args):
    """The start-up line of a run with --optimizer or one of its options; None for a run without them."""
    parts = []
    if getattr(args, 'optimizer', None) == 'sgd':
        parts.append('sgd, momentum {:g}{}'.format(args.momentum or 0.0, ', nesterov' if args.nesterov else ''))
    elif getattr(args, 'optimizer', None) is not None:
        parts.append(args.optimizer)
    for k in ('clipnorm', 'clipvalue', 'weight_decay'):
        if getattr(args, k, None) is not None:
            parts.append('{} {:g}'.format(k, getattr(args, k)))
    if parts and getattr(args, 'optimizer', None) is None:
        parts.insert(0, 'nadam')
    return ', '.join(parts) or None


def main(argv=None):
    args = parse_args(argv)
    world = int(os.environ.get('WORLD_SIZE', '1'))
    if world > 1 and not (args.data_parallel and not args.predict_file and args.emulate_world is None):
        sys.stderr.write('dsen2_amd.train runs on one GPU: data-parallel training (WORLD_SIZE > 1) is not supported unless asked '
                         'for: pass --data_parallel (training only)\n')
        return 2
    rank = 0
    if args.data_parallel and world > 1:
        from . import dist
        rank, world, _ = dist.init_from_env(args.backend)        # before anything touches HIP
    rc = run(args, rank, world)
    if args.data_parallel and world > 1:
        dist.finalize()                # barrier, then leave the group (a rank that raised skips the barrier: its peers are
    return rc                          # stuck in a collective, and torch.distributed.run ends them; as dsen2_amd.cli does)


def run(args, rank, world):
    from . import training
    from .DSen2Net import s2model
    say = print if rank == 0 else (lambda *a, **k: None)      # one rank talks

    path = args.path if args.path.endswith('/') else args.path + '/'
    if args.predict_file:
        bands = ((4, None, None), (6, None, None), (2, None, None)) if args.run_60 else ((4, None, None), (6, None, None))
        return predict(s2model(bands, num_layers=32 if args.deep else 6, feature_size=256 if args.deep else 128,
                               precision=args.precision), args, path)
    if args.tiles is not None:
        conflict = tiles_conflict(args, path)
        if conflict:
            sys.stderr.write(conflict + '\n')
            return 2
        if world > 1 and args.seed is None:
            sys.stderr.write('--tiles under --data_parallel needs --seed: every rank draws the validation crops itself\n')
            return 2
    out = args.out if args.out is not None else path + 'network_data/'
    if rank == 0:
        os.makedirs(out, exist_ok=True)
    bands = ((4, None, None), (6, None, None), (2, None, None)) if args.run_60 else ((4, None, None), (6, None, None))
    if args.deep:
        model = s2model(bands, num_layers=32, feature_size=256, precision=args.precision)
        batch_size = 8
    else:
        model = s2model(bands, num_layers=6, feature_size=128, precision=args.precision)
        batch_size = 128
    if args.batch_size:
        batch_size = args.batch_size
    model_nr = MODEL_NR
    if args.resume_file:
        say('Will resume from the weights {}'.format(args.resume_file))
        if world > 1:
            from . import dist
            model.set_weights_flat(dist.load_weights_on_root(args.resume_file, model.cin, model.cout, model.num_layers,
                                                             model.feature_size, device=model.device))
        else:
            model.load_weights(args.resume_file)
        model_nr = model_number(args.resume_file)
        say('Changing the model number to: {}'.format(model_nr))
    else:
        from . import weights
        model.set_weights_flat(weights.random_he_uniform(model.cin, model.cout, model.num_layers, model.feature_size,
                                                         seed=args.seed if args.seed is not None else 1))
        say('Model number is {}'.format(model_nr))
    if args.mask_key is not None and not args.mask_nodata:
        args.mask_nodata = True
        say('--mask_key implies --mask_nodata: the masked pixels are no-data in the ground truth.')
    model.compile(optimizer=make_optimizer(args), loss=args.loss or 'mean_absolute_error', mixed_precision=args.mixed_precision, loss_param=args.loss_param,
                  mask_nodata=args.mask_nodata, ssim_weight=args.ssim_weight, ssim_win=args.ssim_win, ssim_sigma=args.ssim_sigma,
                  ssim_data_range=args.ssim_data_range)
    if args.loss is not None or args.mask_nodata or args.ssim_weight:     # (without the new flags: the output as it always was)
        from . import losses
        say('Loss: {}.'.format(losses.describe(model.loss_setting)))
    if describe_optimizer(args):                                          # (without the new flags: the output as it always was)
        say('Optimizer: {}.'.format(describe_optimizer(args)))

    corpus = None
    if args.tiles is not None:
        from . import corpus as corpus_mod, create_patches
        say('Loading {} tile{} onto the GPU...'.format(len(args.tiles), '' if len(args.tiles) == 1 else 's'))
        rasters = []
        for f in args.tiles:
            opened = create_patches.open_tile(f, args.run_60, quiet=rank != 0)
            if opened is None:
                return 2
            rasters.append(opened)
        if args.mask_key is not None:
            class_masks = [tile_class_mask(f, args.mask_key) for f in args.tiles]
            say('Class masks ({}): {} of {} tile{} carry one.'.format(args.mask_key, sum(m is not None for m in class_masks), len(class_masks),
                                                                   '' if len(class_masks) == 1 else 's'))
            masked = dict(class_masks=class_masks, mask_classes=args.mask_classes, mask_dilate=args.mask_dilate or 0,
                          skip_masked=args.skip_masked)
            import contextlib
            with open(os.devnull, 'w') as quiet, contextlib.redirect_stdout(quiet if rank != 0 else sys.stdout):
                corpus = corpus_mod.TileCorpus(rasters, run_60=args.run_60, device=model.device, skip_blank=args.skip_blank, **masked)
        elif args.skip_blank and rank != 0:                      # (one rank talks: the others build the same masks quietly)
            import contextlib
            with open(os.devnull, 'w') as quiet, contextlib.redirect_stdout(quiet):
                corpus = corpus_mod.TileCorpus(rasters, run_60=args.run_60, device=model.device, skip_blank=True)
        elif args.skip_blank:
            corpus = corpus_mod.TileCorpus(rasters, run_60=args.run_60, device=model.device, skip_blank=True)
        else:
            corpus = corpus_mod.TileCorpus(rasters, run_60=args.run_60, device=model.device)
        del rasters
        nr_crop = 500 if args.run_60 else 8000
        steps = args.steps_per_epoch or max(1, len(corpus) * nr_crop // batch_size)
        val_table, masks, val_arrays = tiles_validation(corpus, args, args.val_crops or nr_crop // 10, say)
        if val_arrays is not None:
            val_tr, val_lb = val_arrays
        say('Holding {} tile{} ({:.1f} MB on the GPU): {} steps of {} crops per epoch, {} crops for validation.'
            .format(len(corpus), '' if len(corpus) == 1 else 's', corpus.nbytes / 1e6, steps, batch_size, val_table.shape[0]))
    else:
        say('Loading the training data...')
        train, label, val_tr, val_lb = training.load_training_data(path, args.run_60, training.SCALE)
        say('Loaded {} patches for training, {} for validation.'.format(label.shape[0], val_lb.shape[0]))

    ckpt = os.path.join(out, model_nr + 'lr_{:.0e}.npy'.format(args.lr))
    log_path = os.path.join(out, model_nr + '_lr_{:.1e}.txt'.format(args.lr))
    if rank == 0:
        open(log_path, 'w').close()

    class EpochLog(training.Callback):
        def on_epoch_end(self, epoch, logs=None):
            with open(log_path, 'a') as f:
                f.write('Finished epoch {:5d}: loss {:.3e}, valid: {:.3e}, lr: {:.1e}\n'
                        .format(epoch, logs.get('loss'), logs.get('val_loss'), self.model.optimizer.lr))

    # the files and the progress line are rank 0's; the learning-rate schedule runs everywhere, on identical numbers
    files = [training.ModelCheckpoint(ckpt, monitor='val_loss', verbose=1, save_best_only=True), EpochLog()] if rank == 0 else []
    callbacks = files + [training.ReduceLROnPlateau(monitor='val_loss', factor=0.5, patience=5, verbose=int(rank == 0), min_delta=1e-6,
                                                    cooldown=20, min_lr=1e-5)]
    say('Training starts...')
    if corpus is not None:
        extra = {}                              # (without the new flags: the call as it always was)
        if masks is not None:
            extra['masks'] = masks
        if args.val_on_device:
            extra['validation_crops'] = val_table
        model.fit_corpus(corpus, batch_size, steps, epochs=args.epochs, validation_data=None if args.val_on_device else (val_tr, val_lb),
                         seed=args.seed, augment=args.augment, callbacks=callbacks, verbose=int(rank == 0),
                         data_parallel=args.data_parallel, emulate_world=args.emulate_world, **extra)
        say('best weights: {}\nlog: {}'.format(ckpt, log_path))
        return 0
    model.fit(x=train, y=label, batch_size=batch_size, epochs=args.epochs, verbose=int(rank == 0), callbacks=callbacks,
              validation_data=(val_tr, val_lb), shuffle=True, seed=args.seed, data_parallel=args.data_parallel,
              emulate_world=args.emulate_world, augment=args.augment)
    say('best weights: {}\nlog: {}'.format(ckpt, log_path))
    return 0


if __name__ == '__main__':
    sys.exit(main())
