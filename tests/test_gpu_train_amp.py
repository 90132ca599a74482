"""Mixed-precision fine-tuning on the GPU: compile(mixed_precision='bf16') on an fp32 model (include/dsen2_hip.h "training",
dsen2_model_set_train_precision).  The one-plane weight-gradient kernel against float64, whole gradients against the float64
restatement of the step (tests/amp_bf16_restatement.py) on inputs whose ReLU masks and loss signs cannot flip, bit-identity of the
step's forward with a precision='bf16' model, determinism, the device repack, train_on_batch, learning, refusals, and the CLI.

Whole gradients, err(a, b) = per-tensor relative L2:
  (a) err(gpu, f64) <= 2 * err(restatement, f64): the device may differ from the restatement by the operands whose
      fp32-accumulated value rounds to the other bf16 neighbour and by the accumulation order, not by more than the bf16
      arithmetic itself costs.  One tensor, and only that one, gets a floor instead: the output layer's bias gradient (the last
      tensor) is the sum of sign(e) / N, which the restatement and float64 form identically (err = 0 exactly), while the device
      forms it in fp32 (1 / N rounded to fp32, fp32 partial sums that cancel).  FP32_FLOOR = 1e-6 is 16 fp32 epsilons, the
      project's gate for fp32 sums (test_gpu_train.py's loss gate).
  (b) err(gpu, restatement) <= 0.5 * err(restatement, f64) for every kernel tensor: the device is closer to its own arithmetic
      than to float64.
  (c) the RMSE of out against the float64 output <= 2 * the restatement's.
  (d) the returned (mae, mse) = float64 MAE / MSE of the returned out against y within 1e-5 relative."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import amp_bf16_restatement as R  # noqa: E402
from dsen2_amd import _lib, training, weights  # noqa: E402
from dsen2_amd.DSen2Net import _ptr, _stream_ptr, bf16_plane_f32, conv3x3_wgrad_bf16, conv3x3_wgrad_geometry, s2model  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda', 0)
FP32_FLOOR = 1e-6


def _inputs(bands, n, h, w, seed):
    rng = np.random.default_rng(seed)
    return [rng.uniform(0.0, 0.5, (n, c, h, w)).astype(np.float32) for c in bands]


def _flat(bands, d, F, seed=1):
    return weights.random_he_uniform(sum(bands), bands[-1], d, F, seed=seed, bias_scale=0.05)


def _model(bands, d, F, seed=1, precision='fp32', flat=None):
    m = s2model(tuple((c, None, None) for c in bands), num_layers=d, feature_size=F, device=DEV, precision=precision)
    flat = _flat(bands, d, F, seed) if flat is None else flat
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


def _weights_of(m):
    back = torch.empty(m.count_params(), dtype=torch.float32, device=DEV)
    with torch.cuda.device(DEV):
        _lib.call('dsen2_model_get_weights', m._handle, _ptr(back), _stream_ptr(DEV))
    return back.cpu().numpy()


# ---- 1. the one-plane weight-gradient kernel ----
def _wgrad64(a, g):
    n, h, w, _ = a.shape
    ap = np.pad(a.astype(np.float64), ((0, 0), (1, 1), (1, 1), (0, 0)))
    g64 = g.astype(np.float64)
    dw = np.empty((3, 3, a.shape[3], g.shape[3]))
    for ky in range(3):
        for kx in range(3):
            dw[ky, kx] = np.einsum('nhwc,nhwo->co', ap[:, ky:ky + h, kx:kx + w], g64)
    return dw, g64.sum(axis=(0, 1, 2))


def _to_bf16(x):
    """fp32 array -> the fp32 array of its bf16 (RNE) values: products of two such values are exact in fp32."""
    return (R.bf16_rne_bits(np.ascontiguousarray(x, np.float32).view(np.uint32)).astype(np.uint32) << np.uint32(16)).view(np.float32)


@pytest.mark.parametrize('n,h,w,F,gscale', [
    (2, 16, 16, 128, 1.0),
    (1, 9, 21, 256, 1.0),         # ragged, n = 1
    (3, 20, 28, 128, 1.0),        # several tiles and images
    (1, 1, 1, 128, 1.0),
    (2, 5, 40, 128, 1.0),         # wider than a tile
    (2, 16, 16, 128, 1e-6),       # real loss gradients are 1 / (n c h w)
])
def test_wgrad_bf16_kernel_against_numpy(n, h, w, F, gscale):
    rng = np.random.default_rng(n * 1000 + h * 10 + w)
    a = _to_bf16(rng.uniform(-1, 1, (n, h, w, F)).astype(np.float32))
    g = _to_bf16((rng.uniform(-1, 1, (n, h, w, F)) * gscale).astype(np.float32))
    ad, gd = _dev([a, g])
    ap, gp = bf16_plane_f32(ad), bf16_plane_f32(gd)
    dw, db = conv3x3_wgrad_bf16(ap, gp)
    ref_w, ref_b = _wgrad64(a, g)
    ew, eb = R.rel(dw.cpu().numpy(), ref_w), R.rel(db.cpu().numpy(), ref_b)
    print('bf16 wgrad n=%d %dx%d F=%d g x %g: rel. L2 error dW %.2e, db %.2e' % (n, h, w, F, gscale, ew, eb))
    assert ew <= 1e-4 and eb <= 1e-4
    dw2, db2 = conv3x3_wgrad_bf16(ap, gp)
    assert torch.equal(dw, dw2) and torch.equal(db, db2)
    dws, dbs = conv3x3_wgrad_bf16(ap, gp, scale=0.1)
    es, ebs = R.rel(dws.cpu().numpy(), 0.1 * ref_w), R.rel(dbs.cpu().numpy(), 0.1 * ref_b)
    print('   scale 0.1: dW %.2e, db %.2e' % (es, ebs))
    assert es <= 1e-4 and ebs <= 1e-4


# ---- 2. whole gradients where no ReLU mask and no loss sign can flip ----
# case -> (tiles, the split counts of the bf16 body kernel and of the fp32 kernel in the first / output layer): the cases of
# R.CASES where a split-K run of the weight-gradient kernels holds several tiles and one workspace serves the three in turn
MULTI_RUN = {((4, 6), 1, 128, 20, 21, 37): (360, 64, 256, 256), ((4, 6), 1, 256, 3, 21, 37): (54, 16, 54, 54)}
assert set(MULTI_RUN) <= set(R.CASES)


@pytest.mark.parametrize('bands,d,F,n,h,w', R.CASES)
def test_gradients_against_the_restatement_and_float64(bands, d, F, n, h, w):
    if (bands, d, F, n, h, w) in MULTI_RUN:
        tiles, s_body, s_first, s_out = MULTI_RUN[(bands, d, F, n, h, w)]
        assert conv3x3_wgrad_geometry('bf16', n, h, w, F)[:2] == (tiles, s_body)
        assert conv3x3_wgrad_geometry('fp32', n, h, w, 16, F)[:2] == (tiles, s_first)
        assert conv3x3_wgrad_geometry('fp32', n, h, w, F, 16)[:2] == (tiles, s_out)
        assert tiles // s_body >= 3 and tiles % s_body != 0
    err_r = R.check_preconditions(bands, d, F, n, h, w)
    flat, xs, y, s64, sr = R.case(bands, d, F, n, h, w)
    m, _ = _model(bands, d, F, flat=flat)
    m.compile(mixed_precision='bf16')
    out = torch.empty((n, bands[-1], h, w), dtype=torch.float32, device=DEV)
    grad, loss2 = _gradients(m, _dev(xs), _dev([y])[0], out=out)
    parts = R.split_flat(grad.cpu().numpy().astype(np.float64), bands, d, F)
    err_g = [R.rel(g, ref) for g, ref in zip(parts, s64['grads'])]
    err_gr = [R.rel(g, ref) if np.linalg.norm(ref) > 0 else 0.0 for g, ref in zip(parts, sr['grads'])]
    out_g = out.cpu().numpy().astype(np.float64)
    rmse_g = float(np.sqrt(np.mean((out_g - s64['out']) ** 2)))
    rmse_r = float(np.sqrt(np.mean((sr['out'] - s64['out']) ** 2)))
    e = out_g - y.astype(np.float64)
    mae, mse = float(np.abs(e).mean()), float((e * e).mean())
    l2 = loss2.cpu().numpy().astype(np.float64)
    print('amp gradients %s d=%d F=%d n=%d %dx%d: out rmse gpu %.2e restatement %.2e; loss rel %.1e mse rel %.1e'
          % (bands, d, F, n, h, w, rmse_g, rmse_r, abs(l2[0] - mae) / mae, abs(l2[1] - mse) / mse))
    for i in range(len(parts)):
        print('   tensor %2d (%s): err(gpu, f64) %.2e  err(restatement, f64) %.2e  err(gpu, restatement) %.2e  ratio %s'
              % (i, 'kernel' if i % 2 == 0 else 'bias', err_g[i], err_r[i], err_gr[i],
                 '%.3f' % (err_gr[i] / err_r[i]) if err_r[i] > 0 else '-'))
    assert torch.isfinite(grad).all()
    for i in range(len(parts)):
        bound = FP32_FLOOR if i == len(parts) - 1 and err_r[i] == 0.0 else 2 * err_r[i]
        assert err_g[i] <= bound, ('(a)', i, err_g[i], err_r[i])
    for i in range(0, len(parts), 2):
        assert err_gr[i] <= 0.5 * err_r[i], ('(b)', i, err_gr[i], err_r[i])
    assert rmse_g <= 2 * rmse_r, ('(c)', rmse_g, rmse_r)
    assert abs(l2[0] - mae) <= 1e-5 * mae and abs(l2[1] - mse) <= 1e-5 * mse, ('(d)', l2, mae, mse)


# ---- 3. forward bits, determinism ----
CASES = [((4, 6), 2, 128, 2, 16, 16), ((4, 6, 2), 1, 128, 2, 16, 16), ((4, 6), 1, 256, 2, 16, 16)]
# the same networks on patches of more than one tile, which inference runs layer by layer: the chain kernel is out of the picture
LAYERWISE_CASES = [((4, 6), 2, 128, 2, 32, 32), ((4, 6, 2), 1, 128, 2, 32, 32), ((4, 6), 1, 256, 2, 32, 32)]


@pytest.mark.parametrize('bands,d,F,n,h,w', CASES + LAYERWISE_CASES)
def test_training_forward_is_the_bf16_models_and_deterministic(bands, d, F, n, h, w):
    m, flat = _model(bands, d, F)
    b16, _ = _model(bands, d, F, precision='bf16')
    # The step runs layer by layer.  The switch that turns the chain kernel off exists in the diagnostic build only, so the
    # 32 x 32 cases are the comparison with the chain kernel out of the way: there inference goes layer by layer too.  For the
    # single-tile 16 x 16 patches it takes the chain kernel, which gives the per-layer kernels' bits
    # (test_gpu_vdsen2_bf16.py::test_chain_kernel_equals_the_per_layer_kernels_bit_for_bit).
    if (bands, d, F, n, h, w) in LAYERWISE_CASES:
        assert b16.body_launches(n, h, w) == 2 * d
    xs_d = _dev(_inputs(bands, n, h, w, seed=5))
    y_d = _dev([np.random.default_rng(6).uniform(0, 0.5, (n, bands[-1], h, w)).astype(np.float32)])[0]
    ref = b16.forward_device(xs_d)
    m.compile(mixed_precision='bf16')
    out = torch.empty_like(ref)
    g1, l1 = _gradients(m, xs_d, y_d, out=out)
    assert torch.equal(out, ref)
    g2, l2 = _gradients(m, xs_d, y_d)
    assert torch.equal(g1, g2) and torch.equal(l1, l2)
    assert torch.isfinite(g1).all() and float(g1.abs().max()) > 0
    # the model's own forward stays fp32
    f32, _ = _model(bands, d, F)
    assert torch.equal(m.forward_device(xs_d), f32.forward_device(xs_d))


# ---- 4. device repack = host pack, of the fp32 buffers and of the companion's ----
@pytest.mark.parametrize('bands,d,F,n,h,w', CASES)
def test_device_repack_matches_host_pack(bands, d, F, n, h, w):
    m, _ = _model(bands, d, F)
    m.compile(training.Nadam(lr=1e-3), mixed_precision='bf16')
    xs = _inputs(bands, n, h, w, seed=7)
    xs_d = _dev(xs)
    y = np.random.default_rng(8).uniform(0, 0.5, (n, bands[-1], h, w)).astype(np.float32)
    y_d = _dev([y])[0]

    def check(current):
        f32, _ = _model(bands, d, F, flat=current)
        b16, _ = _model(bands, d, F, precision='bf16', flat=current)
        assert torch.equal(m.forward_device(xs_d), f32.forward_device(xs_d))
        out = torch.empty((n, bands[-1], h, w), dtype=torch.float32, device=DEV)
        _gradients(m, xs_d, y_d, out=out)
        assert torch.equal(out, b16.forward_device(xs_d))
        np.testing.assert_array_equal(_weights_of(m), current)

    new = weights.random_he_uniform(sum(bands), bands[-1], d, F, seed=9, bias_scale=0.1)
    m.set_weights_device(torch.from_numpy(new).to(DEV))
    check(new)
    m.set_weights_flat(new)       # dsen2_model_load_weights on a model being trained: the companion follows too
    m.train_on_batch(xs, y)
    stepped = m.get_weights_flat()
    assert not np.array_equal(stepped, new)
    check(stepped)


# ---- 5. train_on_batch = gradients + nadam + repack ----
def test_train_on_batch_is_gradients_nadam_repack():
    bands, d, F = (4, 6), 2, 128
    xs = _inputs(bands, 4, 16, 16, seed=12)
    y = np.random.default_rng(13).uniform(0, 0.5, (4, 6, 16, 16)).astype(np.float32)
    a, flat = _model(bands, d, F)
    b, _ = _model(bands, d, F)
    a.compile(training.Nadam(lr=1e-3), mixed_precision='bf16')
    b.compile(training.Nadam(lr=1e-3), mixed_precision='bf16')
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
    fresh, _ = _model(bands, d, F, flat=a.get_weights_flat())
    np.testing.assert_array_equal(a.predict(xs), fresh.predict(xs))


# ---- 6. / 7. where the setting changes nothing ----
def test_model_without_blocks_steps_in_fp32():
    """num_layers = 0: a precision-1 plan of such a network is fp32 in every layer, so the step is the fp32 step's bits."""
    bands, d, F = (4, 6), 0, 128
    xs_d = _dev(_inputs(bands, 2, 9, 11, seed=15))
    y_d = _dev([np.random.default_rng(16).uniform(0, 0.5, (2, 6, 9, 11)).astype(np.float32)])[0]
    got = []
    for mixed in ('bf16', None):
        m, _ = _model(bands, d, F)
        m.compile(mixed_precision=mixed)
        got.append(_gradients(m, xs_d, y_d))
    assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1])
    assert float(got[0][0].abs().max()) > 0


def test_mixed_precision_none_is_todays_step():
    bands, d, F, n, h, w = (4, 6), 2, 128, 2, 16, 16
    xs_d = _dev(_inputs(bands, n, h, w, seed=17))
    y_d = _dev([np.random.default_rng(18).uniform(0, 0.5, (n, 6, h, w)).astype(np.float32)])[0]
    a, _ = _model(bands, d, F)
    a.compile()
    b, _ = _model(bands, d, F)
    b.compile(mixed_precision=None)
    ga, la = _gradients(a, xs_d, y_d)
    gb, lb = _gradients(b, xs_d, y_d)
    assert torch.equal(ga, gb) and torch.equal(la, lb)
    # and back from 'bf16': the state is rebuilt, the weights survive, the step is the fp32 one again
    b.compile(mixed_precision='bf16')
    gm, _ = _gradients(b, xs_d, y_d)
    assert not torch.equal(gm, ga)
    b.compile(mixed_precision=None)
    gc, lc = _gradients(b, xs_d, y_d)
    assert torch.equal(gc, ga) and torch.equal(lc, la)


# ---- 8. learning ----
def test_mixed_precision_student_learns_teacher():
    """40 steps: the float64 restatement of this run (same teacher, start, inputs and Nadam, on the CPU) brings the float64 MAE
    to 0.32 of its start, so the halving asked here is the arithmetic's, not a lucky device;
    test_train_amp_host.py::test_restated_student_halves_its_error_in_40_steps keeps a reduced form of that run."""
    bands, d, F = (4, 6), 2, 128
    teacher, tflat = _model(bands, d, F, seed=3)
    rng = np.random.default_rng(0)
    xs = _inputs(bands, 16, 32, 32, seed=14)
    y = teacher.predict(xs)
    start = (tflat + rng.uniform(-0.15, 0.15, tflat.shape)).astype(np.float32)
    student, _ = _model(bands, d, F, flat=start)
    student.compile(training.Nadam(lr=1e-3), mixed_precision='bf16')
    b16, _ = _model(bands, d, F, precision='bf16', flat=start)
    first16 = b16.evaluate(xs, y)
    first = student.evaluate(xs, y)              # fp32: the model's own forward
    losses = [student.train_on_batch(xs, y)[0] for _ in range(40)]
    last = student.evaluate(xs, y)
    print('mixed-precision learning: fp32 MAE %.4e -> %.4e (%.3f of the start); first loss %.6e, bf16 forward MAE %.6e'
          % (first[0], last[0], last[0] / first[0], losses[0], first16[0]))
    assert losses[0] == pytest.approx(first16[0], rel=1e-5)
    assert last[0] < 0.5 * first[0]
    assert student.get_weights_flat().dtype == np.float32


# ---- 9. refusals ----
def test_refusals():
    bands, d, F = (4, 6), 1, 128
    for precision in ('bf16x3', 'bf16'):
        m, _ = _model(bands, d, F, precision=precision)
        with pytest.raises(ValueError):
            m.compile(mixed_precision='bf16')
        with torch.cuda.device(DEV):
            assert _lib.load().dsen2_model_set_train_precision(m._handle, 1) == _lib.ERR_INVALID
            assert _lib.load().dsen2_model_set_train_precision(m._handle, 0) == _lib.ERR_INVALID
    m, _ = _model(bands, d, F)
    with pytest.raises(ValueError):
        m.compile(mixed_precision='fp16')
    with torch.cuda.device(DEV):
        assert _lib.load().dsen2_model_set_train_precision(m._handle, 2) == _lib.ERR_INVALID
        assert _lib.load().dsen2_model_set_train_precision(m._handle, -1) == _lib.ERR_INVALID
    # a workspace sized for train precision 0 is too small for 1 at d = 1 (five fp32 tensors against seven and a half)
    n, h, w = 2, 16, 16
    m.compile()
    small = m.train_workspace_bytes(n, h, w)
    m.compile(mixed_precision='bf16')
    need = m.train_workspace_bytes(n, h, w)
    assert need > small
    xs_d = _dev(_inputs(bands, n, h, w, seed=19))
    y_d = _dev([np.zeros((n, 6, h, w), np.float32)])[0]
    grad = torch.empty(m.count_params(), dtype=torch.float32, device=DEV)
    loss2 = torch.empty(2, dtype=torch.float32, device=DEV)
    with pytest.raises(_lib.DSen2Error) as ei:
        m.gradients_device(xs_d, y_d, grad, loss2, workspace=torch.empty(small, dtype=torch.uint8, device=DEV))
    assert ei.value.code == _lib.ERR_WORKSPACE
    m.gradients_device(xs_d, y_d, grad, loss2, workspace=torch.empty(need, dtype=torch.uint8, device=DEV))
    torch.cuda.synchronize()
    assert torch.isfinite(grad).all()


# ---- 10. the CLI ----
def test_train_cli_mixed_precision_end_to_end(tmp_path):
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
                        '--batch_size', '32', '--out', str(out), '--seed', '0', '--mixed_precision', 'bf16'], cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    ckpt = out / 's2_038_lr_1e-04.npy'
    log = out / 's2_038__lr_1.0e-04.txt'
    assert ckpt.exists() and log.exists()
    lines = log.read_text().splitlines()
    assert len(lines) == 2 and lines[0].startswith('Finished epoch     0: loss')
    flat = weights.load_flat(str(ckpt), 10, 6, 6, 128)
    assert flat.dtype == np.float32
    for precision in ('fp32', 'bf16', 'bf16x3'):
        m = s2model(((4, None, None), (6, None, None)), num_layers=6, feature_size=128, device=DEV, precision=precision)
        m.set_weights_flat(flat)
        pred = m.predict(_inputs((4, 6), 2, 32, 32, seed=1))
        assert pred.shape == (2, 6, 32, 32) and np.isfinite(pred).all()
