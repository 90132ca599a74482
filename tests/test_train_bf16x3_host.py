"""Fine-tuning of bf16x3 models, host side (no GPU): the two new C entries are declared, exported and refuse bad arguments
before touching a device; the new kernel file is part of the build; the training CLI has --precision."""
import ctypes
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def test_c_abi_declares_exports_and_checks_the_new_entries():
    from dsen2_amd import _lib, build
    build.build()
    lib = _lib.load()
    header = open(os.path.join(ROOT, 'include', 'dsen2_hip.h')).read()
    for name in ('dsen2_conv3x3_wgrad_bf16x3', 'dsen2_join3_f32'):
        assert re.search(r'\bint %s\s*\(' % name, header) and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert 'conv3x3_wgrad16.hip' in build.SOURCES
    a, b, c, d = (ctypes.c_void_p(0x1000 * k) for k in (1, 2, 3, 4))       # never dereferenced: every call below is refused first

    def refused(fn, *args):
        assert fn(*args) == _lib.ERR_INVALID
        return lib.dsen2_last_error().decode()
    f = lib.dsen2_conv3x3_wgrad_bf16x3
    for k in range(4):
        args = [a, b, c, d]
        args[k] = None
        assert 'NULL' in refused(f, *(args + [2, 16, 16, 128, 1.0, None]))
    assert 'feat 64' in refused(f, a, b, c, d, 2, 16, 16, 64, 1.0, None)
    assert 'feat 192' in refused(f, a, b, c, d, 2, 16, 16, 192, 1.0, None)
    assert 'bad shape' in refused(f, a, b, c, d, 0, 16, 16, 128, 1.0, None)
    assert 'bad shape' in refused(f, a, b, c, d, 1, 16, -1, 128, 1.0, None)
    assert '2^31' in refused(f, a, b, c, d, 1, 4096, 4096, 256, 1.0, None)
    g = lib.dsen2_join3_f32
    for k in range(3):
        args = [a, b, c]
        args[k] = None
        refused(g, *(args + [1, 8, 8, 128, None]))
    assert 'multiple of 8' in refused(g, a, b, c, 1, 8, 8, 12, None)
    assert 'multiple of 8' in refused(g, a, b, c, 1, 8, 8, 520, None)
    refused(g, a, b, c, 1, 0, 8, 128, None)


def test_train_cli_has_the_precision_flag():
    r = subprocess.run([sys.executable, '-m', 'dsen2_amd.train', '--help'], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert '--precision' in r.stdout and 'bf16x3' in r.stdout
    from dsen2_amd import train
    assert train.parse_args([]).precision == 'fp32'
    assert train.parse_args(['--precision', 'bf16x3']).precision == 'bf16x3'
