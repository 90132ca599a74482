"""Fine-tuning of bf16x3 models on the GPU (include/dsen2_hip.h "training"): the bf16x3 weight-gradient kernel against float64,
dsen2_join3_f32, whole gradients against a float64 torch-CPU autograd of the same graph on inputs whose ReLU masks cannot
flip, the mask-free tensors at real shapes, bit-identity with the forward, determinism, the device repack, train_on_batch,
learning, and the training CLI.

A ReLU input within the bf16x3 forward's error of zero may get the other mask on the device, and with an MAE loss a handful
of flipped elements move a gradient tensor by ~1e-2 (measured on the float64 reference alone).  So the whole-gradient cases
ASSERT that every float64 ReLU input is at least MARGIN = 5e-5 away from zero (ten times the per-layer conv-A error of bf16x3
recorded in DESIGN.md §3.4) and use input seeds, found on the CPU from the float64 reference, for which that holds."""
import functools
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
from dsen2_amd.DSen2Net import (_ptr, _stream_ptr, conv3x3_wgrad_bf16x3, conv3x3_wgrad_geometry, join3_f32, s2model,  # noqa: E402
                                split3_f32)

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda', 0)
MARGIN = 5e-5


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


def _relu_margin(xs, flat, bands, d, F):
    pre = []
    with torch.no_grad():
        out = _forward64([torch.tensor(a, dtype=torch.float64) for a in xs], _unflatten(flat.astype(np.float64), bands, d, F), d, pre)
    return min(float(v.abs().min()) for v in pre), out.numpy()


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
    return grads, float(loss.detach()), float((e * e).mean().detach())


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


def _flat(bands, d, F, seed=1):
    return weights.random_he_uniform(sum(bands), bands[-1], d, F, seed=seed, bias_scale=0.05)


def _model(bands, d, F, seed=1, precision='bf16x3'):
    m = s2model(tuple((c, None, None) for c in bands), num_layers=d, feature_size=F, device=DEV, precision=precision)
    flat = _flat(bands, d, F, seed)
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


def _target(out64, seed):
    rng = np.random.default_rng(seed)
    s = np.where(rng.uniform(size=out64.shape) < 0.5, -1.0, 1.0)
    return (out64 + s * (0.01 + rng.uniform(0.0, 0.05, out64.shape))).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _reference(bands, d, F, n, h, w, seed):
    """(inputs, target, float64 gradients, loss, mse, min |ReLU input|) of one case: computed once, never modified."""
    flat = _flat(bands, d, F)
    xs = _inputs(bands, n, h, w, seed)
    margin, out64 = _relu_margin(xs, flat, bands, d, F)
    y = _target(out64, seed=3)
    g64, loss64, mse64 = _grads64(xs, y, flat, bands, d, F)
    return xs, y, g64, loss64, mse64, margin


def _rel(got, ref):
    return float(np.linalg.norm(got - ref) / np.linalg.norm(ref))


# ---- 1. the weight-gradient kernel ----
def _wgrad64(a, g):
    n, h, w, _ = a.shape
    ap = np.pad(a.astype(np.float64), ((0, 0), (1, 1), (1, 1), (0, 0)))
    g64 = g.astype(np.float64)
    dw = np.empty((3, 3, a.shape[3], g.shape[3]))
    for ky in range(3):
        for kx in range(3):
            dw[ky, kx] = np.einsum('nhwc,nhwo->co', ap[:, ky:ky + h, kx:kx + w], g64)
    return dw, g64.sum(axis=(0, 1, 2))


@pytest.mark.parametrize('n,h,w,F,gscale', [
    (2, 16, 16, 128, 1.0),
    (1, 9, 21, 256, 1.0),         # ragged, n = 1
    (3, 20, 28, 128, 1.0),        # several tiles and images
    (1, 1, 1, 128, 1.0),
    (2, 5, 40, 128, 1.0),         # wider than a tile
    (2, 16, 16, 128, 1e-6),       # real loss gradients are 1 / (n c h w)
])
def test_wgrad_bf16x3_kernel_against_numpy(n, h, w, F, gscale):
    rng = np.random.default_rng(n * 1000 + h * 10 + w)
    a = rng.uniform(-1, 1, (n, h, w, F)).astype(np.float32)
    g = (rng.uniform(-1, 1, (n, h, w, F)) * gscale).astype(np.float32)
    ad, gd = _dev([a, g])
    ap, gp = split3_f32(ad)[0], split3_f32(gd)[0]
    dw, db = conv3x3_wgrad_bf16x3(ap, gp)
    ref_w, ref_b = _wgrad64(a, g)
    ew, eb = _rel(dw.cpu().numpy(), ref_w), _rel(db.cpu().numpy(), ref_b)
    print('bf16x3 wgrad n=%d %dx%d F=%d g x %g: rel. L2 error dW %.2e, db %.2e' % (n, h, w, F, gscale, ew, eb))
    assert ew <= 1e-4 and eb <= 1e-4
    dw2, db2 = conv3x3_wgrad_bf16x3(ap, gp)
    assert torch.equal(dw, dw2) and torch.equal(db, db2)
    dws, dbs = conv3x3_wgrad_bf16x3(ap, gp, scale=0.1)
    es, ebs = _rel(dws.cpu().numpy(), 0.1 * ref_w), _rel(dbs.cpu().numpy(), 0.1 * ref_b)
    print('   scale 0.1: dW %.2e, db %.2e' % (es, ebs))
    assert es <= 1e-4 and ebs <= 1e-4


# ---- 2. join3 ----
@pytest.mark.parametrize('n,h,w,c', [(2, 5, 7, 128), (1, 33, 3, 8), (3, 4, 4, 256)])
def test_join3_inverts_split3_bit_for_bit(n, h, w, c):
    rng = np.random.default_rng(c + h)
    u = rng.integers(0, 1 << 32, (n, h, w, c), dtype=np.uint64).astype(np.uint32)
    special = (u & np.uint32(0x7f800000)) == np.uint32(0x7f800000)              # NaN and Inf excluded
    u = np.where(special, u & np.uint32(0xbfffffff), u).astype(np.uint32)
    x = torch.from_numpy(u.view(np.float32)).to(DEV)
    hx, lo = split3_f32(x)
    back = join3_f32(hx, lo)
    torch.cuda.synchronize()
    assert np.array_equal(back.cpu().numpy().view(np.uint32), u)


# ---- 3. whole gradients where no ReLU mask can flip ----
SAFE_CASES = [((4, 6), 1, 128, 1, 8, 8, s) for s in (136, 204)] + \
             [((4, 6, 2), 1, 128, 1, 8, 8, s) for s in (204, 228)] + \
             [((4, 6), 2, 128, 1, 8, 8, s) for s in (111, 117, 137)] + \
             [((4, 6), 1, 256, 1, 6, 6, s) for s in (103, 112, 118)] + \
             [((4, 6), 6, 128, 1, 4, 4, s) for s in (101, 116)]      # the full DSen2 depth: layer indexing


@pytest.mark.parametrize('bands,d,F,n,h,w,seed', SAFE_CASES)
def test_gradients_match_float64_autograd_where_no_mask_can_flip(bands, d, F, n, h, w, seed):
    xs, y, g64, loss64, mse64, margin = _reference(bands, d, F, n, h, w, seed)
    assert margin >= MARGIN, 'input seed %d: a ReLU input lies %.2e from zero' % (seed, margin)
    m, _ = _model(bands, d, F)
    m.compile()
    grad, loss2 = _gradients(m, _dev(xs), _dev([y])[0])
    parts = _split(grad.cpu().numpy().astype(np.float64), bands, d, F)
    errs = [_rel(g, ref) for g, ref in zip(parts, g64)]
    l2 = loss2.cpu().numpy().astype(np.float64)
    print('bf16x3 gradients %s d=%d F=%d n=%d %dx%d seed %d (margin %.1e): worst per-tensor rel. L2 error %.2e, loss rel %.1e, mse rel %.1e'
          % (bands, d, F, n, h, w, seed, margin, max(errs), abs(l2[0] - loss64) / loss64, abs(l2[1] - mse64) / mse64))
    for i, err in enumerate(errs):
        assert err <= 1e-4, (i, err)
    assert abs(l2[0] - loss64) <= 1e-5 * loss64
    assert abs(l2[1] - mse64) <= 1e-5 * mse64


# ---- 4. real shapes: the tensors no mask touches, and no mis-indexed layer ----
# case -> (tiles, the split counts of the bf16x3 body kernel and of the fp32 kernel in the first / output layer): the whole step
# where a split-K run of the weight-gradient kernels holds several tiles (more than 5 per run in the body layers, 1-2 in the
# first and the output layer; 3-4 per run at F = 256) and one workspace serves the three layer kinds in turn
MULTI_RUN = {((4, 6), 1, 128, 20, 21, 37): (360, 64, 256, 256), ((4, 6), 1, 256, 3, 21, 37): (54, 16, 54, 54)}


@pytest.mark.parametrize('bands,d,F,n,h,w', [((4, 6), 6, 128, 3, 20, 28), ((4, 6), 1, 256, 2, 16, 16)] + list(MULTI_RUN))
def test_gradients_at_real_shapes(bands, d, F, n, h, w):
    if (bands, d, F, n, h, w) in MULTI_RUN:
        tiles, s_body, s_first, s_out = MULTI_RUN[(bands, d, F, n, h, w)]
        assert conv3x3_wgrad_geometry('bf16x3', n, h, w, F)[:2] == (tiles, s_body)
        assert conv3x3_wgrad_geometry('fp32', n, h, w, 16, F)[:2] == (tiles, s_first)
        assert conv3x3_wgrad_geometry('fp32', n, h, w, F, 16)[:2] == (tiles, s_out)
        assert tiles // s_body >= 3 and tiles % s_body != 0
    xs, y, g64, loss64, mse64, _ = _reference(bands, d, F, n, h, w, 2)
    m, _ = _model(bands, d, F)
    m.compile()
    grad, loss2 = _gradients(m, _dev(xs), _dev([y])[0])
    parts = _split(grad.cpu().numpy().astype(np.float64), bands, d, F)
    errs = [_rel(g, ref) for g, ref in zip(parts, g64)]
    smooth = [4 * d, 4 * d + 1, 4 * d + 2, 4 * d + 3]       # the last block's conv-B and the output layer: kernel, bias
    print('bf16x3 gradients %s d=%d F=%d n=%d %dx%d: mask-free tensors %s, worst of all %.2e'
          % (bands, d, F, n, h, w, ' '.join('%.2e' % errs[i] for i in smooth), max(errs)))
    for i in smooth:
        assert errs[i] <= 1e-4, (i, errs[i])
    for i, err in enumerate(errs):
        assert err <= 0.1, (i, err)
    l2 = loss2.cpu().numpy().astype(np.float64)
    assert abs(l2[0] - loss64) <= 1e-5 * loss64 and abs(l2[1] - mse64) <= 1e-5 * mse64


# ---- 5. forward bits, determinism ----
CASES = [((4, 6), 2, 128, 2, 16, 16), ((4, 6, 2), 1, 128, 2, 16, 16), ((4, 6), 1, 256, 2, 16, 16)]


@pytest.mark.parametrize('bands,d,F,n,h,w', CASES)
def test_training_forward_bit_identical_and_deterministic(bands, d, F, n, h, w):
    m, _ = _model(bands, d, F)
    # (where inference takes the chain kernel instead, that kernel gives the per-layer kernels' bits: test_gpu_bf16x3.py)
    xs_d = _dev(_inputs(bands, n, h, w, seed=5))
    y_d = _dev([np.random.default_rng(6).uniform(0, 0.5, (n, bands[-1], h, w)).astype(np.float32)])[0]
    ref = m.forward_device(xs_d)
    m.compile()
    out = torch.empty_like(ref)
    g1, l1 = _gradients(m, xs_d, y_d, out=out)
    assert torch.equal(out, ref)
    g2, l2 = _gradients(m, xs_d, y_d)
    assert torch.equal(g1, g2) and torch.equal(l1, l2)
    assert torch.isfinite(g1).all() and float(g1.abs().max()) > 0


# ---- 6. device repack = host pack ----
@pytest.mark.parametrize('bands,d,F,n,h,w', CASES)
def test_device_repack_matches_host_pack(bands, d, F, n, h, w):
    m, flat = _model(bands, d, F)
    xs = _inputs(bands, n, h, w, seed=7)
    xs_d = _dev(xs)
    # through set_weights_device
    new = weights.random_he_uniform(sum(bands), bands[-1], d, F, seed=9, bias_scale=0.1)
    m.set_weights_device(torch.from_numpy(new).to(DEV))
    fresh, _ = _model(bands, d, F)
    fresh.set_weights_flat(new)
    assert torch.equal(m.forward_device(xs_d), fresh.forward_device(xs_d))
    back = torch.empty(m.count_params(), dtype=torch.float32, device=DEV)
    with torch.cuda.device(DEV):
        _lib.call('dsen2_model_get_weights', m._handle, _ptr(back), _stream_ptr(DEV))
    np.testing.assert_array_equal(back.cpu().numpy(), new)
    # the host-loaded weights come back as fp32, not as hi + lo
    with torch.cuda.device(DEV):
        _lib.call('dsen2_model_get_weights', fresh._handle, _ptr(back), _stream_ptr(DEV))
    np.testing.assert_array_equal(back.cpu().numpy(), new)
    # through a Nadam step on the device
    m.compile(training.Nadam(lr=1e-3))
    y = np.random.default_rng(8).uniform(0, 0.5, (n, bands[-1], h, w)).astype(np.float32)
    m.train_on_batch(xs, y)
    stepped = m.get_weights_flat()
    assert not np.array_equal(stepped, new)
    fresh.set_weights_flat(stepped)
    assert torch.equal(m.forward_device(xs_d), fresh.forward_device(xs_d))
    # and the checkpoint of a bf16x3 model is an ordinary fp32 one
    f32, _ = _model(bands, d, F, precision='fp32')
    f32.set_weights_flat(stepped)
    np.testing.assert_array_equal(f32.get_weights_flat(), stepped)


def test_bf16x3_model_without_blocks_trains_as_the_fp32_model():
    """num_layers = 0: every layer of a bf16x3 model is planned fp32, so its gradients are the fp32 model's bits."""
    bands, d, F = (4, 6), 0, 128
    xs_d = _dev(_inputs(bands, 2, 9, 11, seed=15))
    y_d = _dev([np.random.default_rng(16).uniform(0, 0.5, (2, 6, 9, 11)).astype(np.float32)])[0]
    got = []
    for precision in ('bf16x3', 'fp32'):
        m, _ = _model(bands, d, F, precision=precision)
        m.compile()
        got.append(_gradients(m, xs_d, y_d))
    assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1])
    assert float(got[0][0].abs().max()) > 0


# ---- 7. train_on_batch = gradients + nadam + repack ----
def test_train_on_batch_is_gradients_nadam_repack():
    bands, d, F = (4, 6), 2, 128
    xs = _inputs(bands, 4, 16, 16, seed=12)
    y = np.random.default_rng(13).uniform(0, 0.5, (4, 6, 16, 16)).astype(np.float32)
    a, flat = _model(bands, d, F)
    b, _ = _model(bands, d, F)
    a.compile(training.Nadam(lr=1e-3))
    b.compile(training.Nadam(lr=1e-3))
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


# ---- 8. learning ----
def test_bf16x3_student_learns_teacher():
    bands, d, F = (4, 6), 2, 128
    teacher, tflat = _model(bands, d, F, seed=3, precision='fp32')
    rng = np.random.default_rng(0)
    xs = _inputs(bands, 16, 32, 32, seed=14)
    y = teacher.predict(xs)
    start = (tflat + rng.uniform(-0.15, 0.15, tflat.shape)).astype(np.float32)
    student, _ = _model(bands, d, F)
    student.set_weights_flat(start)
    student.compile(training.Nadam(lr=1e-3))
    twin, _ = _model(bands, d, F, precision='fp32')
    twin.set_weights_flat(start)
    twin.compile(training.Nadam(lr=1e-3))
    first32 = twin.train_on_batch(xs, y)[0]
    first = student.evaluate(xs, y)
    losses = [student.train_on_batch(xs, y)[0] for _ in range(40)]
    last = student.evaluate(xs, y)
    print('bf16x3 learning: MAE %.4e -> %.4e (%.3f of the start); first loss against fp32: rel %.1e'
          % (first[0], last[0], last[0] / first[0], abs(losses[0] - first32) / first32))
    assert losses[0] == pytest.approx(first32, rel=1e-4)
    assert losses[0] == pytest.approx(first[0], rel=1e-4)
    assert last[0] < 0.5 * first[0]
    # the trained weights are an ordinary fp32 checkpoint
    f32, _ = _model(bands, d, F, precision='fp32')
    f32.set_weights_flat(student.get_weights_flat())
    assert f32.evaluate(xs, y)[0] == pytest.approx(last[0], abs=1e-4)      # the two forwards differ by ~1e-5 per output


# ---- 9. the CLI ----
def test_train_cli_bf16x3_end_to_end(tmp_path):
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
                        '--batch_size', '32', '--out', str(out), '--seed', '0', '--precision', 'bf16x3'], cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    ckpt = out / 's2_038_lr_1e-04.npy'
    log = out / 's2_038__lr_1.0e-04.txt'
    assert ckpt.exists() and log.exists()
    lines = log.read_text().splitlines()
    assert len(lines) == 2 and lines[0].startswith('Finished epoch     0: loss')
    flat = weights.load_flat(str(ckpt), 10, 6, 6, 128)
    assert flat.dtype == np.float32
    for precision in ('fp32', 'bf16x3'):
        m = s2model(((4, None, None), (6, None, None)), num_layers=6, feature_size=128, device=DEV, precision=precision)
        m.set_weights_flat(flat)
        pred = m.predict(_inputs((4, 6), 2, 32, 32, seed=1))
        assert pred.shape == (2, 6, 32, 32) and np.isfinite(pred).all()
