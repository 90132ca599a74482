"""float64 torch-CPU restatement of the mixed-precision training step (include/dsen2_hip.h, "training": train precision 1), the
yardstick of tests/test_train_amp_host.py and tests/test_gpu_train_amp.py.  Written from the header's description, not from the
kernels: every convolution accumulates in float64; what is restated is WHERE operands are rounded to bf16 and HOW.

  weights, the first convolution's inputs, t_l and du    round to nearest even            (bf16_rne_bits)
  the hi plane of a residual stream (x_l, g)             (u + 0x8000) >> 16, ties away    (bf16_hi_bits)

  forward   x_0 = relu(conv(r(x), r(W0)) + b0) (band groups other than 4 + 6 (+ 2): x and W0 unrounded);
            t_l = r(relu(conv(hi(x_{l-1}), r(WA)) + bA));
            x_l = x_{l-1} + 0.1 * (conv(t_l, r(WB)) + bB);  out = conv(x_d, W_out) + b_out + skip   (unrounded)
  backward  g = dL/dx_l:  dWB = 0.1 * wgrad(t_l, hi(g)), dbB = 0.1 * sum hi(g), du = r([t_l > 0] * 0.1 * conv_T(hi(g), r(WB))),
            dWA = wgrad(hi(x_{l-1}), du), dbA = sum du, g += conv_T(du, r(WA));
            the output layer's and the first layer's gradients are unrounded (fp32 kernels on fp32 tensors).
With emulate=False every rounding is the identity: the plain float64 autograd of the same graph.
The product must never import this file."""
import functools

import numpy as np
import torch

RES_SCALE = 0.1


# ---- the two roundings, on fp32 bit patterns (uint32 -> the bf16's uint16) ----
def bf16_rne_bits(u):
    """Round to nearest even, the host packers' f32_to_bf16_rne."""
    u = np.asarray(u, dtype=np.uint32).astype(np.uint64)
    return (((u + np.uint64(0x7fff) + ((u >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)) & np.uint64(0xffff)).astype(np.uint16)


def bf16_hi_bits(u):
    """The hi plane of a residual stream: (u + 0x8000) >> 16 mod 2^16, nearest with ties away from zero."""
    u = np.asarray(u, dtype=np.uint32).astype(np.uint64)
    return (((u + np.uint64(0x8000)) >> np.uint64(16)) & np.uint64(0xffff)).astype(np.uint16)


def _round_with(bits_fn, x):
    """float64 tensor -> float64 tensor of the bf16 values (through the fp32 value the device holds)."""
    u = x.detach().to(torch.float32).contiguous().numpy().view(np.uint32)
    back = (bits_fn(u).astype(np.uint32) << np.uint32(16)).view(np.float32)
    return torch.from_numpy(back.astype(np.float64)).reshape(x.shape)


def rne(x):
    return _round_with(bf16_rne_bits, x)


def hi(x):
    return _round_with(bf16_hi_bits, x)


def _identity(x):
    return x.detach().clone()


# ---- the convolutions ----
def _conv_grads(xq, wq, gq):
    """(conv_T(gq, wq), wgrad(xq, gq)) in float64."""
    with torch.enable_grad():
        xq = xq.detach().requires_grad_(True)
        wq = wq.detach().requires_grad_(True)
        y = torch.nn.functional.conv2d(xq, wq, padding=1)
        return torch.autograd.grad(y, (xq, wq), gq)


class _QConv(torch.autograd.Function):
    """scale * (conv(rx(x), rw(W)) + b); backward on the rounded operands: gq = rg(G), dX = scale * conv_T(gq, rw(W)),
    dW = scale * wgrad(rx(x), gq), db = scale * sum gq."""

    @staticmethod
    def forward(ctx, x, w, b, rx, rw, rg, scale):
        xq, wq = rx(x), rw(w)
        ctx.save_for_backward(xq, wq)
        ctx.rg, ctx.scale = rg, scale
        return scale * (torch.nn.functional.conv2d(xq, wq, padding=1) + b.view(1, -1, 1, 1))

    @staticmethod
    def backward(ctx, G):
        xq, wq = ctx.saved_tensors
        gq = ctx.rg(G)
        dx, dw = _conv_grads(xq, wq, gq)
        return ctx.scale * dx, ctx.scale * dw, ctx.scale * gq.sum(dim=(0, 2, 3)), None, None, None, None


class _FirstConv(torch.autograd.Function):
    """conv(rx(x), rw(W)) + b forward; the weight gradient is the fp32 kernel's: wgrad(x, G), sum G, both unrounded."""

    @staticmethod
    def forward(ctx, x, w, b, rx, rw):
        ctx.save_for_backward(x, w)
        return torch.nn.functional.conv2d(rx(x), rw(w), padding=1) + b.view(1, -1, 1, 1)

    @staticmethod
    def backward(ctx, G):
        x, w = ctx.saved_tensors
        _, dw = _conv_grads(x, w, G)
        return None, dw, G.sum(dim=(0, 2, 3)), None, None


class _RoundSTE(torch.autograd.Function):
    """t = r(relu output) forward; the gradient passes (the mask is the ReLU's: t > 0 where the ReLU input is)."""

    @staticmethod
    def forward(ctx, x, r):
        return r(x)

    @staticmethod
    def backward(ctx, G):
        return G, None


def layer_shapes(cin, cout, d, F):
    return [(cin, F)] + [(F, F)] * (2 * d) + [(F, cout)]


def unflatten(flat, bands, d, F):
    """keras-flat -> [W0 (OIHW), b0, WA1, bA1, WB1, ...] float64 leaves."""
    ps, o = [], 0
    for a, b in layer_shapes(sum(bands), bands[-1], d, F):
        k = np.asarray(flat[o:o + 9 * a * b], dtype=np.float64).reshape(3, 3, a, b)
        o += 9 * a * b
        ps.append(torch.tensor(k).permute(3, 2, 0, 1).contiguous().requires_grad_(True))
        ps.append(torch.tensor(np.asarray(flat[o:o + b], dtype=np.float64)).requires_grad_(True))
        o += b
    return ps


def split_flat(flat, bands, d, F):
    parts, o = [], 0
    for a, b in layer_shapes(sum(bands), bands[-1], d, F):
        parts.append(flat[o:o + 9 * a * b])
        o += 9 * a * b
        parts.append(flat[o:o + b])
        o += b
    return parts


def forward(xs, ps, d, emulate, pre=None):
    """xs: float64 NCHW tensors; pre (a list) receives every ReLU input."""
    r, h = (rne, hi) if emulate else (_identity, _identity)
    keep = pre.append if pre is not None else (lambda v: None)
    # the first convolution of a precision-1 model runs on bf16 operands for the band groups 4 + 6 (+ 2) only; any other
    # grouping's is fp32 (include/dsen2_hip.h: dsen2_model_create), and the training step runs that model's forward
    r0 = r if tuple(int(x.shape[1]) for x in xs) in ((4, 6), (4, 6, 2)) else _identity
    v = _FirstConv.apply(torch.cat(xs, 1), ps[0], ps[1], r0, r0)
    keep(v)
    x = torch.relu(v)
    for l in range(d):
        v = _QConv.apply(x, ps[2 + 4 * l], ps[3 + 4 * l], h, r, r, 1.0)
        keep(v)
        t = _RoundSTE.apply(torch.relu(v), r)
        x = x + _QConv.apply(t, ps[4 + 4 * l], ps[5 + 4 * l], _identity, r, h, RES_SCALE)
    return torch.nn.functional.conv2d(x, ps[-2], ps[-1], padding=1) + xs[-1]


def step(xs, y, flat, bands, d, F, emulate):
    """One gradients call: dict(out [n,cout,h,w], grads (per tensor, keras order, raveled HWIO / bias), mae, mse, pre)."""
    ps = unflatten(flat, bands, d, F)
    x64 = [torch.tensor(np.asarray(a, dtype=np.float64)) for a in xs]
    pre = []
    out = forward(x64, ps, d, emulate, pre)
    e = out - torch.tensor(np.asarray(y, dtype=np.float64))
    loss = e.abs().mean()
    loss.backward()
    grads = []
    for i, p in enumerate(ps):
        g = p.grad.permute(2, 3, 1, 0) if i % 2 == 0 else p.grad
        grads.append(g.contiguous().numpy().ravel().copy())
    return dict(out=out.detach().numpy(), grads=grads, mae=float(loss.detach()), mse=float((e * e).mean().detach()),
                pre=[v.detach().numpy() for v in pre])


# ---- the whole-gradient cases: ReLU masks and loss signs fixed by construction ----
CASES = [((4, 6), 2, 128, 2, 8, 8),
         ((4, 6, 2), 1, 128, 1, 8, 8),
         ((4, 6), 1, 256, 1, 9, 21),        # ragged, F = 256
         ((4, 6), 6, 128, 1, 4, 4),         # full depth: layer indexing
         ((4, 6), 2, 128, 3, 20, 28),       # several tiles and images
         # several tiles per split-K run of the weight-gradient kernels (tests/test_gpu_train_amp.py asserts the run lengths):
         ((4, 6), 1, 128, 20, 21, 37),      # 360 tiles: more than 5 per run in the body layers, 1-2 in the first and output layer
         ((4, 6), 1, 256, 3, 21, 37)]       # 54 tiles over the 16 splits of F = 256


def he_uniform(cin, cout, d, F, seed=1, bias_scale=0.05):
    """dsen2_amd.weights.random_he_uniform, restated (the product is not imported here)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    parts = []
    for a, b in layer_shapes(cin, cout, d, F):
        limit = np.sqrt(6.0 / (9 * a))
        parts.append(rng.uniform(-limit, limit, size=(3, 3, a, b)).astype(np.float32).ravel())
        parts.append(rng.uniform(-bias_scale, bias_scale, size=(b,)).astype(np.float32))
    return np.concatenate(parts)


def case_weights(bands, d, F):
    """he_uniform(seed 1, bias 0.05); every kernel but the output layer's times 0.25 (0.15 at d = 6); every ReLU layer's bias
    + 1 on even channels, - 1 on odd ones: each ReLU input sits near +-1, so no bf16 error can flip a mask."""
    flat = he_uniform(sum(bands), bands[-1], d, F).copy()
    parts = split_flat(flat, bands, d, F)          # views into flat
    shrink = np.float32(0.15 if d == 6 else 0.25)
    n_layers = 2 * d + 2
    for li in range(n_layers - 1):
        parts[2 * li] *= shrink
    sign = np.where(np.arange(F) % 2 == 0, 1.0, -1.0).astype(np.float32)
    parts[1] += sign
    for l in range(d):
        parts[3 + 4 * l] += sign
    return flat


def case_inputs(bands, n, h, w, seed=5):
    rng = np.random.default_rng(seed)
    return [rng.uniform(0.0, 0.5, (n, c, h, w)).astype(np.float32) for c in bands]


def case_target(out64, seed=3):
    """out64 +- (0.01 + uniform(0, 0.05)): no output of the bf16 forward (1-2e-4 away from out64) lies on the other side."""
    rng = np.random.default_rng(seed)
    s = np.where(rng.uniform(size=out64.shape) < 0.5, -1.0, 1.0)
    return (out64 + s * (0.01 + rng.uniform(0.0, 0.05, out64.shape))).astype(np.float32)


@functools.lru_cache(maxsize=None)
def case(bands, d, F, n, h, w):
    """(flat, xs, y, float64 step, restated step) of one case: computed once, never modified."""
    flat = case_weights(bands, d, F)
    xs = case_inputs(bands, n, h, w)
    with torch.no_grad():
        out64 = forward([torch.tensor(a.astype(np.float64)) for a in xs], unflatten(flat, bands, d, F), d, False).numpy()
    y = case_target(out64)
    return flat, xs, y, step(xs, y, flat, bands, d, F, False), step(xs, y, flat, bands, d, F, True)


def rel(got, ref):
    return float(np.linalg.norm(np.asarray(got, np.float64) - ref) / np.linalg.norm(ref))


def check_preconditions(bands, d, F, n, h, w):
    """What the whole-gradient comparison rests on, from the two references alone.  Returns the per-tensor relative L2 distance of
    the restated gradients from the float64 ones."""
    flat, xs, y, s64, sr = case(bands, d, F, n, h, w)
    for k, (a, b) in enumerate(zip(s64['pre'], sr['pre'])):
        assert np.abs(a).min() >= 0.2 and np.abs(b).min() >= 0.2, ('ReLU layer %d: an input within 0.2 of zero' % k)
        assert np.array_equal(a > 0, b > 0), 'ReLU layer %d: the masks differ' % k
        active = float((a > 0).mean())
        assert 0.4 <= active <= 0.6, 'ReLU layer %d: %.2f active' % (k, active)
    margin = np.abs(s64['out'] - y.astype(np.float64)).min()
    worst = np.abs(sr['out'] - s64['out']).max()
    assert margin >= 10 * worst, 'loss signs: margin %.2e against a forward error of %.2e' % (margin, worst)
    return [rel(g, ref) for g, ref in zip(sr['grads'], s64['grads'])]
