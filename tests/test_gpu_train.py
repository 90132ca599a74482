"""Fine-tuning on the GPU (include/dsen2_hip.h "training"): gradients against a float64 torch-CPU autograd of the same graph,
the weight-gradient kernel alone, bit-identity with the forward, determinism, the device repack, the Nadam kernel,
train_on_batch, learning, refusals and the training CLI."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from dsen2_amd import _lib, training, weights  # noqa: E402
from dsen2_amd.DSen2Net import _ptr, _stream_ptr, conv3x3_wgrad_geometry, s2model  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda', 0)


# ---- float64 restatement of the training graph (the arithmetic of include/dsen2_hip.h) ----
def _unflatten(flat, bands, d, F):
    ps, o = [], 0
    for a, b in weights.layer_shapes(sum(bands), bands[-1], d, F):
        k = flat[o:o + 9 * a * b].reshape(3, 3, a, b)
        o += 9 * a * b
        ps.append(torch.tensor(k, dtype=torch.float64).permute(3, 2, 0, 1).contiguous().requires_grad_(True))
        ps.append(torch.tensor(flat[o:o + b], dtype=torch.float64).requires_grad_(True))
        o += b
    return ps


def _forward64(xs, ps, d, pre=None):
    """pre (a list): receives every ReLU input."""
    conv = torch.nn.functional.conv2d
    keep = pre.append if pre is not None else (lambda v: None)
    v = conv(torch.cat(xs, 1), ps[0], ps[1], padding=1)
    keep(v)
    x = torch.relu(v)
    for l in range(d):
        v = conv(x, ps[2 + 4 * l], ps[3 + 4 * l], padding=1)
        keep(v)
        x = x + 0.1 * conv(torch.relu(v), ps[4 + 4 * l], ps[5 + 4 * l], padding=1)
    return conv(x, ps[-2], ps[-1], padding=1) + xs[-1]


def _grads64(xs, y, flat, bands, d, F):
    ps = _unflatten(flat.astype(np.float64), bands, d, F)
    x64 = [torch.tensor(a, dtype=torch.float64) for a in xs]
    out = _forward64(x64, ps, d)
    e = out - torch.tensor(y, dtype=torch.float64)
    loss = e.abs().mean()
    loss.backward()
    grads = []
    for i, p in enumerate(ps):
        g = p.grad.permute(2, 3, 1, 0) if i % 2 == 0 else p.grad
        grads.append(g.contiguous().numpy().ravel())
    return out.detach().numpy(), grads, float(loss.detach()), float((e * e).mean().detach())


def _split(flat, bands, d, F):
    parts, o = [], 0
    for a, b in weights.layer_shapes(sum(bands), bands[-1], d, F):
        parts.append(flat[o:o + 9 * a * b])
        o += 9 * a * b
        parts.append(flat[o:o + b])
        o += b
    return parts


def _inputs(bands, n, h, w, seed):
    rng = np.random.default_rng(seed)
    return [rng.uniform(0.0, 0.5, (n, c, h, w)).astype(np.float32) for c in bands]


def _model(bands, d, F, seed=1, precision='fp32'):
    m = s2model(tuple((c, None, None) for c in bands), num_layers=d, feature_size=F, device=DEV, precision=precision)
    flat = weights.random_he_uniform(sum(bands), bands[-1], d, F, seed=seed, bias_scale=0.05)
    m.set_weights_flat(flat)
    return m, flat


def _dev(arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays]


def _gradients(m, xs_d, y_d, out=None):
    grad = torch.empty(m.count_params(), dtype=torch.float32, device=DEV)
    loss2 = torch.empty(2, dtype=torch.float32, device=DEV)
    m.gradients_device(xs_d, y_d, grad, loss2, out=out)
    torch.cuda.synchronize()
    return grad, loss2


CASES = [((4, 6), 2, 128, 2, 16, 16), ((4, 6, 2), 1, 128, 2, 16, 16), ((4, 6), 1, 256, 2, 16, 16), ((4, 6), 6, 128, 3, 20, 28)]
# The whole step where a split-K run of the weight-gradient kernel holds several tiles and ONE workspace (the largest of the
# three layer kinds' sizes) serves the first, the body and the output layer in turn: case -> (input seed, tiles, the split
# counts of the body / first / output layer).  360 tiles: more than 5 per run in the body layers, 1-2 in the first and the
# output layer; 54 tiles at F = 256: 3-4 per run in the body layers.
# With 4e6 (1.2e6) ReLU inputs one of them lies within ~1e-7 of zero for most input seeds, which is the error of an fp32
# forward (rms 1e-7 on these layers: torch's fp32 CPU convolutions against float64), and ONE flipped mask moves a bias
# gradient by ~1e-3 of its norm.  So these cases ASSERT that every float64 ReLU input is at least MULTI_RUN_MARGIN = 8e-7
# away from zero, and use input seeds, found on the CPU from the float64 reference alone, for which that holds.
MULTI_RUN = {((4, 6), 1, 128, 20, 21, 37): (182, 360, 64, 256, 256), ((4, 6), 1, 256, 3, 21, 37): (139, 54, 16, 54, 54)}
MULTI_RUN_MARGIN = 8e-7


def _target(out64, seed):
    rng = np.random.default_rng(seed)
    s = np.where(rng.uniform(size=out64.shape) < 0.5, -1.0, 1.0)
    return (out64 + s * (0.01 + rng.uniform(0.0, 0.05, out64.shape))).astype(np.float32)


@pytest.mark.parametrize('bands,d,F,n,h,w', CASES + list(MULTI_RUN))
def test_gradients_match_float64_autograd(bands, d, F, n, h, w):
    seed, pre = 2, None
    if (bands, d, F, n, h, w) in MULTI_RUN:
        seed, tiles, s_body, s_first, s_out = MULTI_RUN[(bands, d, F, n, h, w)]
        for ca, cg, splits in ((F, F, s_body), (16, F, s_first), (F, 16, s_out)):
            assert conv3x3_wgrad_geometry('fp32', n, h, w, ca, cg)[:2] == (tiles, splits)
        assert tiles // s_body >= 3 and tiles % s_body != 0
        pre = []
    m, flat = _model(bands, d, F)
    xs = _inputs(bands, n, h, w, seed=seed)
    with torch.no_grad():
        out64 = _forward64([torch.tensor(a, dtype=torch.float64) for a in xs], _unflatten(flat.astype(np.float64), bands, d, F), d, pre)
    if pre is not None:
        margin = min(float(v.abs().min()) for v in pre)
        assert margin >= MULTI_RUN_MARGIN, 'input seed %d: a ReLU input lies %.2e from zero' % (seed, margin)
    y = _target(out64.numpy(), seed=3)
    _, g64, loss64, mse64 = _grads64(xs, y, flat, bands, d, F)
    m.compile()
    grad, loss2 = _gradients(m, _dev(xs), _dev([y])[0])
    parts = _split(grad.cpu().numpy().astype(np.float64), bands, d, F)
    worst = 0.0
    for i, (g, ref) in enumerate(zip(parts, g64)):
        err = np.linalg.norm(g - ref) / np.linalg.norm(ref)
        worst = max(worst, err)
        assert err <= 1e-4, (i, err)
    l2 = loss2.cpu().numpy().astype(np.float64)
    print('gradients %s d=%d F=%d n=%d %dx%d: worst per-tensor rel. L2 error %.2e, loss %.3e (rel %.1e), mse rel %.1e'
          % (bands, d, F, n, h, w, worst, l2[0], abs(l2[0] - loss64) / loss64, abs(l2[1] - mse64) / mse64))
    assert abs(l2[0] - loss64) <= 1e-6 * loss64
    assert abs(l2[1] - mse64) <= 1e-6 * mse64


def _wgrad64(a, g, ci, co):
    n, h, w, _ = a.shape
    ap = np.pad(a[..., :ci].astype(np.float64), ((0, 0), (1, 1), (1, 1), (0, 0)))
    g64 = g[..., :co].astype(np.float64)
    dw = np.empty((3, 3, ci, co))
    for ky in range(3):
        for kx in range(3):
            dw[ky, kx] = np.einsum('nhwc,nhwo->co', ap[:, ky:ky + h, kx:kx + w], g64)
    return dw, g64.sum(axis=(0, 1, 2))


@pytest.mark.parametrize('n,h,w,ca,cg,ci,co', [
    (2, 16, 16, 128, 128, 128, 128),      # body
    (1, 9, 21, 256, 256, 256, 256),       # body F = 256, ragged, n = 1
    (3, 5, 7, 16, 128, 10, 128),          # first layer (NHWC16 input, 10 real channels)
    (2, 12, 12, 16, 256, 12, 256),
    (2, 11, 13, 128, 16, 128, 6),         # output layer (dL/dout padded to 16)
    (1, 1, 1, 256, 16, 256, 2),           # a 1 x 1 image
    (1, 1, 1, 128, 128, 128, 128),
])
def test_wgrad_kernel_against_numpy(n, h, w, ca, cg, ci, co):
    rng = np.random.default_rng(n * 1000 + h * 10 + w)
    a = rng.uniform(-1, 1, (n, h, w, ca)).astype(np.float32)
    g = rng.uniform(-1, 1, (n, h, w, cg)).astype(np.float32)
    a[..., ci:] = 0
    g[..., co:] = 0
    ad, gd = _dev([a, g])
    dw = torch.empty(9 * ci * co, dtype=torch.float32, device=DEV)
    db = torch.empty(co, dtype=torch.float32, device=DEV)
    with torch.cuda.device(DEV):
        _lib.call('dsen2_conv3x3_wgrad', _ptr(ad), _ptr(gd), _ptr(dw), _ptr(db), n, h, w, ca, cg, ci, co, 1.0, _stream_ptr(DEV))
    ref_w, ref_b = _wgrad64(a, g, ci, co)
    ew = np.linalg.norm(dw.cpu().numpy().reshape(3, 3, ci, co) - ref_w) / np.linalg.norm(ref_w)
    eb = np.linalg.norm(db.cpu().numpy() - ref_b) / np.linalg.norm(ref_b)
    print('wgrad n=%d %dx%d %d->%d: rel. L2 error dW %.2e, db %.2e' % (n, h, w, ci, co, ew, eb))
    assert ew <= 1e-4 and eb <= 1e-4


@pytest.mark.parametrize('bands,d,F,n,h,w', CASES[:3])
def test_training_forward_bit_identical_and_deterministic(bands, d, F, n, h, w):
    m, _ = _model(bands, d, F)
    xs_d = _dev(_inputs(bands, n, h, w, seed=5))
    y_d = _dev([np.random.default_rng(6).uniform(0, 0.5, (n, bands[-1], h, w)).astype(np.float32)])[0]
    ref = m.forward_device(xs_d)
    out = torch.empty_like(ref)
    g1, l1 = _gradients(m, xs_d, y_d, out=out)
    assert torch.equal(out, ref)
    g2, l2 = _gradients(m, xs_d, y_d)
    assert torch.equal(g1, g2) and torch.equal(l1, l2)


@pytest.mark.parametrize('bands,d,F,n,h,w', CASES[:3])
def test_device_repack_matches_host_pack(bands, d, F, n, h, w):
    m, flat = _model(bands, d, F)
    new = weights.random_he_uniform(sum(bands), bands[-1], d, F, seed=9, bias_scale=0.1)
    m.set_weights_device(torch.from_numpy(new).to(DEV))
    fresh, _ = _model(bands, d, F)
    fresh.set_weights_flat(new)
    xs_d = _dev(_inputs(bands, n, h, w, seed=7))
    assert torch.equal(m.forward_device(xs_d), fresh.forward_device(xs_d))
    back = torch.empty(m.count_params(), dtype=torch.float32, device=DEV)
    with torch.cuda.device(DEV):
        _lib.call('dsen2_model_get_weights', m._handle, _ptr(back), _stream_ptr(DEV))
    np.testing.assert_array_equal(back.cpu().numpy(), new)


def test_nadam_kernel_against_float64():
    rng = np.random.default_rng(11)
    count = 10007
    p = rng.uniform(-1, 1, count).astype(np.float32)
    m = np.zeros(count, np.float32)
    v = np.zeros(count, np.float32)
    lr = 1e-3
    opt = training.Nadam(lr=lr)
    pd, md, vd = _dev([p.copy(), m, v])
    for step in range(3):
        g = rng.uniform(-1, 1, count).astype(np.float32) * np.float32(10.0 ** -step)
        gd = _dev([g])[0]
        p0, m0, v0 = pd.cpu().numpy(), md.cpu().numpy(), vd.cpu().numpy()
        s = opt.next_step()
        with torch.cuda.device(DEV):
            _lib.call('dsen2_nadam_step', _ptr(pd), _ptr(gd), _ptr(md), _ptr(vd), count, lr, s['b1'], s['b2'], s['eps'], s['mc_t'],
                      s['mc_t1'], s['ms_new'], s['ms_next'], s['b2_pow_t'], _stream_ptr(DEV))
        torch.cuda.synchronize()
        g64, p64, m64, v64 = (a.astype(np.float64) for a in (g, p0, m0, v0))
        b1, b2 = float(np.float32(s['b1'])), float(np.float32(s['b2']))    # the kernel's float arguments (keras: float32)
        gp = g64 / (1 - s['ms_new'])
        m64 = b1 * m64 + (1 - b1) * g64
        mp = m64 / (1 - s['ms_next'])
        v64 = b2 * v64 + (1 - b2) * g64 * g64
        vp = v64 / (1 - s['b2_pow_t'])
        p64 = p64 - lr * ((1 - s['mc_t']) * gp + s['mc_t1'] * mp) / (np.sqrt(vp) + s['eps'])
        ulp = np.spacing(np.abs(p64).astype(np.float32)).astype(np.float64)
        assert np.all(np.abs(pd.cpu().numpy() - p64) <= 2 * ulp + 1e-5 * lr), step
        for got, want in ((md, m64), (vd, v64)):
            rel = np.abs(got.cpu().numpy() - want) / np.maximum(np.abs(want), 1e-30)
            assert rel.max() <= 1e-6, (step, rel.max())


def test_train_on_batch_is_gradients_nadam_repack():
    bands, d, F = (4, 6), 2, 128
    xs = _inputs(bands, 4, 16, 16, seed=12)
    y = np.random.default_rng(13).uniform(0, 0.5, (4, 6, 16, 16)).astype(np.float32)
    a, flat = _model(bands, d, F)
    b, _ = _model(bands, d, F)
    a.compile(training.Nadam(lr=1e-3))
    b.compile(training.Nadam(lr=1e-3))
    # by hand on b
    count = b.count_params()
    pb = torch.from_numpy(flat.copy()).to(DEV)
    mb = torch.zeros(count, device=DEV)
    vb = torch.zeros(count, device=DEV)
    opt = training.Nadam(lr=1e-3)
    xs_d, y_d = _dev(xs), _dev([y])[0]
    for _ in range(2):
        la = a.train_on_batch(xs, y)
        grad, loss2 = _gradients(b, xs_d, y_d)
        s = opt.next_step()
        with torch.cuda.device(DEV):
            _lib.call('dsen2_nadam_step', _ptr(pb), _ptr(grad), _ptr(mb), _ptr(vb), count, s['lr'], s['b1'], s['b2'], s['eps'],
                      s['mc_t'], s['mc_t1'], s['ms_new'], s['ms_next'], s['b2_pow_t'], _stream_ptr(DEV))
        b.set_weights_device(pb)
        assert la == [float(x) for x in loss2.cpu().numpy()]
    np.testing.assert_array_equal(a.get_weights_flat(), pb.cpu().numpy())
    for _ in range(3):
        a.train_on_batch(xs, y)
    fresh, _ = _model(bands, d, F)
    fresh.set_weights_flat(a.get_weights_flat())
    np.testing.assert_array_equal(a.predict(xs), fresh.predict(xs))


def test_training_learns_teacher():
    bands, d, F = (4, 6), 2, 128
    teacher, tflat = _model(bands, d, F, seed=3)
    rng = np.random.default_rng(0)
    xs = _inputs(bands, 16, 32, 32, seed=14)
    y = teacher.predict(xs)
    student, _ = _model(bands, d, F)
    student.set_weights_flat((tflat + rng.uniform(-0.15, 0.15, tflat.shape)).astype(np.float32))
    student.compile(training.Nadam(lr=1e-3))
    first = student.evaluate(xs, y)
    losses = [student.train_on_batch(xs, y)[0] for _ in range(40)]
    last = student.evaluate(xs, y)
    print('learning: MAE %.4e -> %.4e (%.3f of the start)' % (first[0], last[0], last[0] / first[0]))
    assert losses[0] == pytest.approx(first[0], rel=1e-5)
    assert last[0] < 0.5 * first[0]
    pred = student.predict(xs).astype(np.float64)
    assert last[0] == pytest.approx(np.mean(np.abs(pred - y)), rel=1e-6)
    assert last[1] == pytest.approx(np.mean((pred - y) ** 2), rel=1e-6)


def test_refusals():
    bf, _ = _model((4, 6), 1, 128, precision='bf16')
    with pytest.raises(ValueError, match='fp32'):
        bf.compile()
    with pytest.raises(Exception):
        bf.train_on_batch(_inputs((4, 6), 1, 8, 8, seed=0), np.zeros((1, 6, 8, 8), np.float32))
    size = ctypes.c_size_t(0)
    with torch.cuda.device(DEV):
        rc = _lib.load().dsen2_model_train_workspace_bytes(bf._handle, 1, 8, 8, ctypes.byref(size))
    assert rc == _lib.ERR_INVALID and b'training needs an fp32 model' in _lib.load().dsen2_last_error()
    m, _ = _model((4, 6), 1, 128)
    m.compile()
    with pytest.raises(ValueError):
        m.train_on_batch(_inputs((4, 6), 1, 8, 8, seed=0), np.zeros((1, 2, 8, 8), np.float32))
    xs_d = _dev(_inputs((4, 6), 1, 8, 8, seed=0))
    y_d = torch.zeros((1, 6, 8, 8), device=DEV)
    grad = torch.empty(m.count_params(), device=DEV)
    loss2 = torch.empty(2, device=DEV)
    need = m.train_workspace_bytes(1, 8, 8)
    ws = torch.empty(need - 256, dtype=torch.uint8, device=DEV)
    with torch.cuda.device(DEV):
        rc = _lib.load().dsen2_model_gradients(m._handle, _ptr(xs_d[0]), _ptr(xs_d[1]), None, _ptr(y_d), None, _ptr(grad),
                                               _ptr(loss2), 1, 8, 8, _ptr(ws), ws.numel(), _stream_ptr(DEV))
    assert rc == _lib.ERR_WORKSPACE


def test_train_cli_end_to_end(tmp_path):
    rng = np.random.default_rng(21)
    train_dir = tmp_path / 'data' / 'train'
    for name in ('S2A_A.SAFE', 'S2B_B.SAFE'):
        d = train_dir / name
        os.makedirs(str(d))
        d10 = rng.uniform(0, 3000, (64, 4, 32, 32)).astype(np.float32)
        d20 = rng.uniform(0, 3000, (64, 6, 32, 32)).astype(np.float32)
        np.save(str(d / 'data10.npy'), d10)
        np.save(str(d / 'data20.npy'), d20)
        np.save(str(d / 'data20_gt.npy'), (d20 + rng.uniform(-50, 50, d20.shape)).astype(np.float32))
    val = np.zeros(128, bool)
    val[::8] = True
    np.save(str(train_dir / 'val_index.npy'), val)
    out = tmp_path / 'out'
    r = subprocess.run([sys.executable, '-m', 'dsen2_amd.train', '--path', str(tmp_path / 'data'), '--epochs', '2',
                        '--batch_size', '32', '--out', str(out), '--seed', '0'], cwd=ROOT, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    ckpt = out / 's2_038_lr_1e-04.npy'
    log = out / 's2_038__lr_1.0e-04.txt'
    assert ckpt.exists() and log.exists()
    lines = log.read_text().splitlines()
    assert len(lines) == 2 and lines[0].startswith('Finished epoch     0: loss')
    flat = weights.load_flat(str(ckpt), 10, 6, 6, 128)
    m = s2model(((4, None, None), (6, None, None)), num_layers=6, feature_size=128, device=DEV)
    m.set_weights_flat(flat)
    pred = m.predict(_inputs((4, 6), 2, 32, 32, seed=1))
    assert pred.shape == (2, 6, 32, 32) and np.isfinite(pred).all()
