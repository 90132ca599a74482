"""Mixed-precision fine-tuning (an fp32 model's step on bf16 operands), host side (no GPU): the two new C entries are declared,
exported and refuse bad arguments before touching a device; the training CLI has --mixed_precision; the float64 restatement's
two roundings are pinned on hand-made bit patterns; and the whole-gradient cases of tests/test_gpu_train_amp.py meet their
preconditions (no ReLU mask and no loss sign can flip) on the two references alone."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import amp_bf16_restatement as R  # noqa: E402


def test_c_abi_declares_exports_and_checks_the_new_entries():
    from dsen2_amd import _lib, build
    build.build()
    lib = _lib.load()
    header = open(os.path.join(ROOT, 'include', 'dsen2_hip.h')).read()
    for name in ('dsen2_model_set_train_precision', 'dsen2_conv3x3_wgrad_bf16'):
        assert re.search(r'\bint %s\s*\(' % name, header) and name in _lib.SIGNATURES and hasattr(lib, name), name
    a, b, c, d = (ctypes.c_void_p(0x1000 * k) for k in (1, 2, 3, 4))       # never dereferenced: every call below is refused first

    def refused(fn, *args):
        assert fn(*args) == _lib.ERR_INVALID
        return lib.dsen2_last_error().decode()
    f = lib.dsen2_conv3x3_wgrad_bf16
    for k in range(4):
        args = [a, b, c, d]
        args[k] = None
        assert 'NULL' in refused(f, *(args + [2, 16, 16, 128, 1.0, None]))
    assert 'feat 64' in refused(f, a, b, c, d, 2, 16, 16, 64, 1.0, None)
    assert 'feat 192' in refused(f, a, b, c, d, 2, 16, 16, 192, 1.0, None)
    assert 'bad shape' in refused(f, a, b, c, d, 0, 16, 16, 128, 1.0, None)
    assert 'bad shape' in refused(f, a, b, c, d, 1, 16, -1, 128, 1.0, None)
    assert '2^31' in refused(f, a, b, c, d, 1, 4096, 4096, 256, 1.0, None)
    assert 'NULL' in refused(lib.dsen2_model_set_train_precision, None, 1)


def test_train_cli_has_the_mixed_precision_flag():
    r = subprocess.run([sys.executable, '-m', 'dsen2_amd.train', '--help'], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert '--mixed_precision' in r.stdout
    from dsen2_amd import train
    assert train.parse_args([]).mixed_precision is None
    assert train.parse_args(['--mixed_precision', 'bf16']).mixed_precision == 'bf16'
    assert train.parse_args(['--precision', 'bf16x3']).mixed_precision is None
    with pytest.raises(SystemExit):
        train.parse_args(['--precision', 'bf16x3', '--mixed_precision', 'bf16'])
    with pytest.raises(SystemExit):
        train.parse_args(['--mixed_precision', 'fp16'])


def test_the_product_does_not_import_the_restatement():
    for dirpath, _, files in os.walk(os.path.join(ROOT, 'dsen2_amd')):
        for name in files:
            if name.endswith('.py'):
                assert 'amp_bf16_restatement' not in open(os.path.join(dirpath, name)).read(), name


def test_rounding_helpers_on_hand_made_bit_patterns():
    u = np.array([
        0x3f800000,     # 1.0: exact
        0x3f808000,     # tie, even mantissa below: RNE down, ties-away up
        0x3f818000,     # tie, odd mantissa below: both up
        0x3f807fff,     # just below a tie: both down
        0x3f808001,     # just above a tie: both up
        0xbf808000,     # the negative tie: sign untouched; RNE to even (towards zero here), ties-away away from zero
        0xbf818000,
        0x3fffffff,     # carry through the mantissa into the exponent: 2.0
        0x3fff8000,     # tie with an all-ones bf16 mantissa: carries into the exponent both ways
        0x7f7fffff,     # the largest finite fp32 rounds to +inf
        0x00000000, 0x80000000,
    ], dtype=np.uint32)
    rne = np.array([0x3f80, 0x3f80, 0x3f82, 0x3f80, 0x3f81, 0xbf80, 0xbf82, 0x4000, 0x4000, 0x7f80, 0x0000, 0x8000], dtype=np.uint16)
    hi = np.array([0x3f80, 0x3f81, 0x3f82, 0x3f80, 0x3f81, 0xbf81, 0xbf82, 0x4000, 0x4000, 0x7f80, 0x0000, 0x8000], dtype=np.uint16)
    assert np.array_equal(R.bf16_rne_bits(u), rne)
    assert np.array_equal(R.bf16_hi_bits(u), hi)
    # the tensor forms are those bits, and leave a value that already is a bf16 alone
    import torch
    finite = u[:9]
    x = torch.from_numpy(finite.view(np.float32).astype(np.float64))
    assert np.array_equal(R.rne(x).numpy().astype(np.float32).view(np.uint32) >> 16, rne[:9])
    assert np.array_equal(R.hi(x).numpy().astype(np.float32).view(np.uint32) >> 16, hi[:9])
    assert torch.equal(R.rne(R.hi(x)), R.hi(x)) and torch.equal(R.hi(R.rne(x)), R.rne(x))
    # against torch's own bfloat16 conversion (round to nearest even) on random values
    v = torch.from_numpy(np.random.default_rng(0).standard_normal(4096).astype(np.float32))
    assert torch.equal(R.rne(v.double()).float(), v.to(torch.bfloat16).float())


def test_restated_weights_are_the_products():
    from dsen2_amd import weights
    for bands, d, F in (((4, 6), 2, 128), ((4, 6, 2), 1, 256)):
        assert np.array_equal(R.he_uniform(sum(bands), bands[-1], d, F), weights.random_he_uniform(sum(bands), bands[-1], d, F, seed=1, bias_scale=0.05))


@pytest.mark.parametrize('bands,d,F,n,h,w', R.CASES)
def test_whole_gradient_cases_meet_their_preconditions(bands, d, F, n, h, w):
    errs = R.check_preconditions(bands, d, F, n, h, w)
    _, _, _, s64, sr = R.case(bands, d, F, n, h, w)
    print('amp restatement %s d=%d F=%d n=%d %dx%d: out rmse %.2e; per-tensor rel. L2 from float64: %s'
          % (bands, d, F, n, h, w, float(np.sqrt(np.mean((sr['out'] - s64['out']) ** 2))), ' '.join('%.1e' % e for e in errs)))
    assert max(errs) < 2e-2 and np.isfinite(errs).all()       # bf16 operands: a fraction of a percent, not garbage


def test_identity_roundings_give_the_plain_float64_autograd():
    import torch
    bands, d, F, n, h, w = R.CASES[0]
    flat, xs, y, s64, _ = R.case(bands, d, F, n, h, w)
    ps = R.unflatten(flat, bands, d, F)
    conv = torch.nn.functional.conv2d
    x64 = [torch.tensor(a.astype(np.float64)) for a in xs]
    x = torch.relu(conv(torch.cat(x64, 1), ps[0], ps[1], padding=1))
    for l in range(d):
        x = x + 0.1 * conv(torch.relu(conv(x, ps[2 + 4 * l], ps[3 + 4 * l], padding=1)), ps[4 + 4 * l], ps[5 + 4 * l], padding=1)
    out = conv(x, ps[-2], ps[-1], padding=1) + x64[-1]
    (out - torch.tensor(y.astype(np.float64))).abs().mean().backward()
    for i, p in enumerate(ps):
        g = (p.grad.permute(2, 3, 1, 0) if i % 2 == 0 else p.grad).contiguous().numpy().ravel()
        assert R.rel(s64['grads'][i], g) <= 1e-12, i


def test_restated_student_halves_its_error_in_40_steps():
    """The step count of test_gpu_train_amp.py's learning test comes from the restatement, not from the device: the same
    teacher (seed 3), start (+- 0.15) and keras-2 Nadam (lr 1e-3, the header's update in float64, parameters kept as fp32),
    40 restated mixed-precision steps, on 2 x 8 x 8 patches to stay quick.  The float64 MAE ends at 0.18 of its start here; the
    full-size run of the GPU test (16 x 32 x 32), restated the same way on the CPU, ends at 0.32."""
    import torch
    from dsen2_amd import training, weights
    bands, d, F = (4, 6), 2, 128
    tflat = weights.random_he_uniform(10, 6, d, F, seed=3, bias_scale=0.05)
    xs = R.case_inputs(bands, 2, 8, 8, seed=14)

    def out64(flat):
        with torch.no_grad():
            return R.forward([torch.tensor(a.astype(np.float64)) for a in xs], R.unflatten(flat, bands, d, F), d, False).numpy()
    y = out64(tflat).astype(np.float32)
    start = (tflat + np.random.default_rng(0).uniform(-0.15, 0.15, tflat.shape)).astype(np.float32)
    p = start.astype(np.float64)
    m, v = np.zeros_like(p), np.zeros_like(p)
    opt = training.Nadam(lr=1e-3)
    first = float(np.abs(out64(start) - y).mean())
    for _ in range(40):
        g = np.concatenate(R.step(xs, y, p.astype(np.float32), bands, d, F, True)['grads'])
        s = opt.next_step()
        gp = g / (1 - s['ms_new'])
        m = s['b1'] * m + (1 - s['b1']) * g
        v = s['b2'] * v + (1 - s['b2']) * g * g
        p = p - s['lr'] * ((1 - s['mc_t']) * gp + s['mc_t1'] * (m / (1 - s['ms_next']))) / (np.sqrt(v / (1 - s['b2_pow_t'])) + s['eps'])
        p = p.astype(np.float32).astype(np.float64)
    last = float(np.abs(out64(p.astype(np.float32)) - y).mean())
    print('restated mixed-precision learning, 2 x 8 x 8: float64 MAE %.4e -> %.4e (%.3f of the start)' % (first, last, last / first))
    assert last < 0.5 * first
