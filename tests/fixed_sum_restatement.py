"""The summation order of dsen2_abs_sq_error_sums and dsen2_loss_sums (csrc/fixed_sum.h, error_sums.hip) in numpy float64, for the
restatements that need it (corpus_mask_restatement.py, loss_restatement.py): numpy rounds every addition on its own."""
import numpy as np

THREADS, PER_THREAD, MAX_BLOCKS = 256, 8, 4096


def tree(s):
    """[rows, 256] -> [rows]: the halving tree of a workgroup."""
    s = s.copy()
    half = THREADS // 2
    while half > 0:
        s[:, :half] = s[:, :half] + s[:, half:2 * half]
        half //= 2
    return s[:, 0]


def strided(values, lanes):
    """Lane j adds values[j], values[j + lanes], ... in index order onto 0.0.  Padding with +0.0 changes no bit, nor does a masked
    element, which the device skips and which is a +0.0 term here: every term is >= +0.0, and x + 0.0 == x for such x."""
    v = np.concatenate([values, np.zeros(-values.size % lanes)]).reshape(-1, lanes)
    acc = np.zeros(lanes)
    for row in v:
        acc = acc + row
    return acc


def fixed_order_sum(terms):
    n = terms.size
    blocks = min(max(-(-n // (THREADS * PER_THREAD)), 1), MAX_BLOCKS)
    partials = tree(strided(terms, blocks * THREADS).reshape(blocks, THREADS))
    return float(tree(strided(partials, THREADS).reshape(1, THREADS))[0])
