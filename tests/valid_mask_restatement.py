"""numpy restatement of the class-mask entries (include/dsen2_hip.h, "class masks"): loops of shifted ORs and np.packbits, written
from the header's definitions and from nothing in csrc/valid_mask.hip."""
import numpy as np


def lut(classes):
    table = np.zeros(256, np.uint8)
    table[list(classes)] = 1
    return table


def raw_invalid(cls, table, up, down, H, W):
    """bool [H, W]: RAW.  up: target (y, x) reads source (y // up, x // up); down: any pixel of the down x down block."""
    bad = np.asarray(table)[np.asarray(cls)] != 0
    if down > 1:
        assert up == 1 and H * down <= bad.shape[0] and W * down <= bad.shape[1]
        out = np.zeros((H, W), bool)
        for dy in range(down):
            for dx in range(down):
                out |= bad[dy:H * down:down, dx:W * down:down]
        return out
    assert (H - 1) // up < bad.shape[0] and (W - 1) // up < bad.shape[1]
    return bad[np.arange(H)[:, None] // up, np.arange(W)[None, :] // up]


def dilate(inv, d):
    """DILATED: OR of the image shifted by every (dy, dx) with |dy| <= d and |dx| <= d; what lies outside is valid (False)."""
    H, W = inv.shape
    along_x = inv.copy()
    for s in range(1, min(d, W - 1) + 1):
        along_x[:, s:] |= inv[:, :-s]
        along_x[:, :-s] |= inv[:, s:]
    out = along_x.copy()
    for s in range(1, min(d, H - 1) + 1):
        out[s:, :] |= along_x[:-s, :]
        out[:-s, :] |= along_x[s:, :]
    return out


def pack_bits(valid):
    """bool [H, W] -> uint32 [H, ceil(W / 32)]: bit x & 31 of word x >> 5, padding bits 0."""
    H, W = valid.shape
    padded = np.zeros((H, (W + 31) // 32 * 32), bool)
    padded[:, :W] = valid
    return np.ascontiguousarray(np.packbits(padded, axis=1, bitorder='little')).view('<u4')


def unpack_bits(bits, W):
    return np.unpackbits(np.ascontiguousarray(bits).view(np.uint8), axis=1, bitorder='little')[:, :W].astype(bool)


def valid_pixels(cls, table, up, down, H, W, d=0):
    return ~dilate(raw_invalid(cls, table, up, down, H, W), d)


def valid_bits(cls, table, up, down, H, W, d=0, and_bits=None):
    bits = pack_bits(valid_pixels(cls, table, up, down, H, W, d))
    return bits if and_bits is None else bits & np.asarray(and_bits).view(np.uint32)


def apply_valid(img, valid):
    out = img.copy()
    out[~valid] = 0
    return out


def cells(valid, S, prior=None):
    """uint8 [H / S, W / S]: 1 where any pixel of the S x S footprint is invalid; prior: a map whose non-zero cells stay as they are."""
    H, W = valid.shape
    got = (~valid).reshape(H // S, S, W // S, S).any(axis=(1, 3)).astype(np.uint8)
    return got if prior is None else np.where(prior != 0, prior, got).astype(np.uint8)
