#!/usr/bin/env python3
"""Are the kernels of a translation unit the same instruction stream in two versions of the source?

    python tools/isa_diff.py conv3x3_body16w.hip [--rev HEAD] [--filter body16w_kernel] [-DDSEN2_DIAG ...]
    python tools/isa_diff.py --all [--rev HEAD] [-D...]       every conv3x3_*.hip of the library
Compiles dsen2_amd/csrc/<source> from the working tree and from git revision --rev (with that revision's headers) to
gfx950 ISA with the product's flags (dsen2_amd/build.py) plus the -D flags given, and compares, kernel by kernel, the
instruction lists with local labels normalised (dsen2_amd/asm_contract.py: the parser and the normalisation of the ISA
hashes).  For refactors that must not change the generated code.  Last line: `N kernels, M different, K missing`; exit
code 1 unless M = K = 0.
"""
import argparse
import concurrent.futures
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dsen2_amd import asm_contract, build as b      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('source', nargs='?')
    ap.add_argument('--all', action='store_true', help='every conv3x3_*.hip in build.SOURCES')
    ap.add_argument('--rev', default='HEAD')
    ap.add_argument('--filter', default='', help='only kernels whose mangled name contains this')
    args, defines = ap.parse_known_args()
    if [d for d in defines if not d.startswith('-D')] or bool(args.source) == args.all:
        ap.error('one source or --all, and -D... flags only')
    sources = [s for s in b.SOURCES if s.startswith('conv3x3_')] if args.all else [args.source]
    with tempfile.TemporaryDirectory(prefix='dsen2_isa_') as tmp:
        os.makedirs(os.path.join(tmp, 'dsen2_amd', 'csrc'))
        os.makedirs(os.path.join(tmp, 'include'))
        for f in subprocess.check_output(['git', 'ls-tree', '--name-only', args.rev, 'dsen2_amd/csrc/', 'include/'], cwd=ROOT, text=True).split():
            with open(os.path.join(tmp, f), 'wb') as fh:
                fh.write(subprocess.check_output(['git', 'show', '%s:%s' % (args.rev, f)], cwd=ROOT))

        def kernels(job):
            text = asm_contract.compile_isa(b.HIPCC, b.FLAGS + defines, os.path.join(job[0], job[1]), os.path.join(tmp, '%d.s' % job[2]))
            return {k: asm_contract.normalised(v) for k, v in asm_contract._kernels(text).items() if args.filter in k}
        jobs = [(d, s, 2 * i + j) for i, s in enumerate(sources) for j, d in enumerate((os.path.join(tmp, 'dsen2_amd', 'csrc'), b.CSRC))]
        with concurrent.futures.ThreadPoolExecutor(max_workers=max(1, b.JOBS)) as pool:
            out = list(pool.map(kernels, jobs))
    n = different = missing = 0
    for old, new in zip(out[0::2], out[1::2]):
        for k in sorted(old):
            verdict = 'same' if old[k] == new.get(k) else 'DIFFERENT' if k in new else 'MISSING'
            n, different, missing = n + 1, different + (verdict == 'DIFFERENT'), missing + (verdict == 'MISSING')
            print('%-110s %5d instructions  %s' % (k[:110], len(old[k]), verdict))
    print('%d kernels, %d different, %d missing' % (n, different, missing))
    return 1 if different + missing else 0


if __name__ == '__main__':
    sys.exit(main())
