"""A numpy float64 restatement of the losses and the no-data mask (include/dsen2_hip.h, "losses and the no-data mask"), written
from the header alone: rho, rho', the mask, dL/dout as dsen2_loss_grad writes it, and dsen2_loss_sums with its summation order.
numpy rounds every operation on its own and has no FMA, which is the arithmetic the header states.  Nothing here imports the
product's own losses.py."""
import numpy as np

from fixed_sum_restatement import fixed_order_sum as _fixed_order_sum      # the entries' order of addition

MAE, MSE, HUBER, CHARBONNIER = 0, 1, 2, 3
KINDS = (MAE, MSE, HUBER, CHARBONNIER)
NAMES = {MAE: 'mae', MSE: 'mse', HUBER: 'huber', CHARBONNIER: 'charbonnier'}


def _p(param):
    return float(np.float32(param))            # (double) of the float32 that crosses the ABI


def sign(d):
    return (d > 0).astype(np.float64) - (d < 0).astype(np.float64)      # sign(0) = 0


def rho(d, kind, param=0.0):
    d, p = np.asarray(d, np.float64), _p(param)
    if kind == MAE:
        return np.abs(d)
    if kind == MSE:
        return d * d
    if kind == HUBER:
        return np.where(np.abs(d) <= p, 0.5 * (d * d), p * (np.abs(d) - 0.5 * p))
    assert kind == CHARBONNIER
    return np.sqrt(d * d + p * p)


def slope(d, kind, param=0.0):
    d, p = np.asarray(d, np.float64), _p(param)
    if kind == MAE:
        return sign(d)
    if kind == MSE:
        return 2.0 * d
    if kind == HUBER:
        return np.where(np.abs(d) <= p, d, p * sign(d))
    assert kind == CHARBONNIER
    return d / np.sqrt(d * d + p * p)


def valid(y, mask):
    """[n, 1, h, w] bool: which pixels of the NCHW target carry ground truth under mask mode `mask`."""
    y = np.asarray(y)
    if not mask:
        return np.ones((y.shape[0], 1) + y.shape[2:], bool)
    return (y != 0).any(axis=1, keepdims=True)


def loss_grad(out, y, kind, param=0.0, mask=0):
    """(g [n*h*w, 16] float32, (mean rho, mean d^2) float64) of the step's loss kernel: e = out - y in float32, d = (double)e,
    g = (float)(rho'(d) * (double)inv), inv = (float)(1 / N), N = every element, masked or not."""
    out, y = np.asarray(out, np.float32), np.asarray(y, np.float32)
    n, c, h, w = out.shape
    d = (out - y).astype(np.float64)
    v = valid(y, mask)
    inv = float(np.float32(1.0 / float(out.size)))
    g = np.where(v, (slope(d, kind, param) * inv).astype(np.float32), np.float32(0.0)).astype(np.float32)
    g16 = np.zeros((n, h, w, 16), np.float32)
    g16[..., :c] = g.transpose(0, 2, 3, 1)
    r, q = np.where(v, rho(d, kind, param), 0.0), np.where(v, d * d, 0.0)
    return g16.reshape(n * h * w, 16), (float(np.sum(r)) / out.size, float(np.sum(q)) / out.size)


# ---- dsen2_loss_sums: dsen2_abs_sq_error_sums' order ------------------------------------------------------------------------------
def loss_sums(pred, y, kind, param=0.0, mask=0):
    """[sum rho, sum d^2, unmasked elements] as float64: d = (double)p - (double)t over NCHW in element order."""
    pred, y = np.asarray(pred, np.float32), np.asarray(y, np.float32)
    d = pred.astype(np.float64) - y.astype(np.float64)
    v = np.broadcast_to(valid(y, mask), d.shape)
    r, q = np.where(v, rho(d, kind, param), 0.0), np.where(v, d * d, 0.0)
    return np.array([_fixed_order_sum(r.ravel()), _fixed_order_sum(q.ravel()), _fixed_order_sum(v.astype(np.float64).ravel())])
