"""python -m dsen2_amd.create_random — mark the validation patches: the counterpart of the reference's training/create_random.py.

    python -m dsen2_amd.create_random --path DIR [--run_60] [--ratio 0.1] [--seed N] [--size N]

Writes DIR/train/val_index.npy (DIR/train60/ with --run_60): a bool array with int(size * ratio) entries set, chosen by the
reference's loop — randrange(0, size) until enough DISTINCT entries are set.  `size` defaults to the number of patches found
under DIR/train*/ (the reference has `45 * 8000` written in); it must be regenerated whenever that number changes.  --seed draws
from random.Random(seed), which gives the sequence random.seed(seed) would give the reference.
"""
import argparse
import glob
import os
import random
import sys

import numpy as np


def make_index(size, ratio=.1, seed=None):
    """(bool [size] mask, number of draws)."""
    rr = random.randrange if seed is None else random.Random(seed).randrange
    nb = int(size * ratio)
    if size <= 0 or not 0 <= nb <= size:
        raise ValueError('cannot mark %d of %d patches' % (nb, size))
    index = np.zeros(size, dtype=bool)
    i = marked = 0
    while marked < nb:
        x = rr(0, size)
        marked += not index[x]
        index[x] = True
        i += 1
    return index, i


def count_patches(train_path):
    """Patches in every <train_path>/*SAFE/data10.npy, in the order the training loader concatenates them."""
    dirs = sorted(glob.glob(os.path.join(train_path, '*SAFE')))
    if not dirs:
        raise OSError('no *SAFE directories under %s' % train_path)
    return sum(int(np.load(os.path.join(d, 'data10.npy'), mmap_mode='r').shape[0]) for d in dirs)


def main(argv=None):
    p = argparse.ArgumentParser(prog='python -m dsen2_amd.create_random', description='Define the validation split of a training set.')
    p.add_argument('--path', default='../data/', help='Path of the data (train/ or train60/ below it).')
    p.add_argument('--run_60', action='store_true', help='The 60->10m training set (train60/).')
    p.add_argument('--ratio', type=float, default=.1, help='Share of the patches used for validation.')
    p.add_argument('--seed', type=int, default=None)
    p.add_argument('--size', type=int, default=None, help='Number of patches (default: counted under the training directory).')
    args = p.parse_args(argv)
    train_path = os.path.join(args.path, 'train60' if args.run_60 else 'train')
    size = args.size if args.size is not None else count_patches(train_path)
    index, draws = make_index(size, args.ratio, args.seed)
    np.save(os.path.join(train_path, 'val_index.npy'), index)
    print('Full no of samples: {}'.format(size))
    print('Validation samples: {}'.format(int(np.sum(index))))
    print('Number of iterations: {}'.format(draws))
    return 0


if __name__ == '__main__':
    sys.exit(main())
