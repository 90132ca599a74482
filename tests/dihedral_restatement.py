"""The 8 flips and rotations of a patch and the geometric self-ensemble, restated in numpy (no GPU, no package code): what the
tests of csrc/dihedral.hip, of dsen2_model_forward_ensemble and of the training augmentation compare against, bit for bit.

    op = k + 4 f,  k in 0..3 quarter turns counter-clockwise,  f in 0..1 a left-right flip first
    D_op(a)    = np.rot90(a[..., ::-1] if f else a, k, axes=(-2, -1))
    D_op^-1(b) = t[..., ::-1] if f else t,   t = np.rot90(b, -k, axes=(-2, -1))
Odd k swaps H and W."""
import numpy as np

OPS = tuple(range(8))


def forward(a, op):
    k, f = int(op) & 3, (int(op) >> 2) & 1
    return np.ascontiguousarray(np.rot90(a[..., ::-1] if f else a, k, axes=(-2, -1)))


def inverse(b, op):
    k, f = int(op) & 3, (int(op) >> 2) & 1
    t = np.rot90(b, -k, axes=(-2, -1))
    return np.ascontiguousarray(t[..., ::-1] if f else t)


def per_sample(a, ops, inv=False):
    """Sample s of a [n, ...] array turned by ops[s] & 7 (square images: the shape stays)."""
    return np.stack([(inverse if inv else forward)(a[s], int(ops[s]) & 7) for s in range(a.shape[0])])


def members(ensemble):
    """The member ops of an ensemble in the order they are summed: True -> all 8, else the distinct ops, ascending."""
    return list(OPS) if ensemble is True else sorted(set(int(op) for op in ensemble))


def ensemble(predict, xs, ops=True):
    """The self-ensemble of `predict` (list of [n, c, h, w] float32 arrays -> [n, cout, h, w] float32) on xs: members in ascending
    op order, y_op = D_op^-1(predict(D_op xs)), s = y_first, then s = s + y_next in float32, and s / float32(count) after the last
    (no divide for a single member)."""
    ms = members(ops)
    s = None
    for op in ms:
        y = inverse(np.asarray(predict([forward(x, op) for x in xs]), np.float32), op)
        s = y if s is None else (s + y).astype(np.float32)
    return s if len(ms) == 1 else (s / np.float32(len(ms))).astype(np.float32)


def ensemble_f64(predict, xs, ops=True):
    """The same mean formed in float64 from a float64 `predict` (the oracle side of the accuracy gate)."""
    ms = members(ops)
    return sum(inverse(np.asarray(predict([forward(x, op) for x in xs]), np.float64), op) for op in ms) / float(len(ms))
