#!/usr/bin/env python3
"""Small stand-ins for the reference's two demo tiles (data/S2A_MSIL1C_20170527_T33UUB.mat, data/S2B_MSIL1C_20171022_T49JGM.mat,
3.7 MB each) -> tests/golden/tiles/<tile>.mat and tests/golden/tiles/crops.json.

A crop of each tile, written the way MATLAB wrote the originals: the original 512-byte user block (the MAT-file header),
superblock of the earliest format, im10 / im20 / im60 as float32 datasets stored CHW-transposed, chunked along the last
on-disk axis with the originals' chunk widths (6 / 9 / 50), gzip level 3, the library's default fill value, and a
null-terminated ASCII MATLAB_class = "single" attribute.  The crop is 390 x 12 pixels at 10 m (195 x 6 at 20 m, 65 x 2 at
60 m), so that im10 has 65 chunks — more than one v1 B-tree node holds, a two-level chunk index like the originals' — and
im20 / im60 end in a partial chunk.  Needs h5py:

    python tests/golden/make_golden_tiles.py <directory holding the reference's data/*.mat>
"""
import json
import os
import sys

import h5py
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, 'tiles')
TILES = {'T33UUB': 'S2A_MSIL1C_20170527_T33UUB.mat', 'T49JGM': 'S2B_MSIL1C_20171022_T49JGM.mat'}
# [first row, rows, first column, columns] at 10 m; 20 m and 60 m are the same window / 2 and / 6
WINDOW10 = [0, 390, 240, 12]
CHUNK_WIDTH = {'im10': 6, 'im20': 9, 'im60': 50}
SCALE = {'im10': 1, 'im20': 2, 'im60': 6}


def matlab_class_attr(dset):
    t = h5py.h5t.C_S1.copy()
    t.set_size(6)
    t.set_strpad(h5py.h5t.STR_NULLTERM)
    a = h5py.h5a.create(dset.id, b'MATLAB_class', t, h5py.h5s.create(h5py.h5s.SCALAR))
    a.write(np.array(b'single', dtype='S6'), mtype=t)          # as stored: no conversion to a terminated string


def main(src_dir):
    os.makedirs(OUT, exist_ok=True)
    meta = {'window10': WINDOW10, 'tiles': {}}
    for tile, name in TILES.items():
        src = os.path.join(src_dir, name)
        dst = os.path.join(OUT, tile + '.mat')
        with h5py.File(src, 'r') as f:
            hwc = {k: f[k][()].transpose() for k in SCALE}                       # rows, columns, bands
        with h5py.File(dst, 'w', userblock_size=512, libver='earliest') as g:
            for k, s in SCALE.items():
                r0, nr, c0, nc = (v // s for v in WINDOW10)
                chw = np.ascontiguousarray(hwc[k][r0:r0 + nr, c0:c0 + nc].transpose())
                dcpl = h5py.h5p.create(h5py.h5p.DATASET_CREATE)
                dcpl.set_chunk((chw.shape[0], chw.shape[1], min(CHUNK_WIDTH[k], chw.shape[2])))
                dcpl.set_deflate(3)
                dcpl.set_fill_time(h5py.h5d.FILL_TIME_IFSET)
                did = h5py.h5d.create(g.id, k.encode(), h5py.h5t.IEEE_F32LE, h5py.h5s.create_simple(chw.shape), dcpl=dcpl)
                did.write(h5py.h5s.ALL, h5py.h5s.ALL, chw)
                matlab_class_attr(g[k])
        header = open(src, 'rb').read(512)
        with open(dst, 'r+b') as fh:
            fh.write(header)
        meta['tiles'][tile] = {'source': name, 'golden': 'tile_%s_600.npz' % tile}
        print(dst, os.path.getsize(dst))
    with open(os.path.join(OUT, 'crops.json'), 'w') as fh:
        json.dump(meta, fh, indent=1)
        fh.write('\n')


if __name__ == '__main__':
    main(sys.argv[1])
