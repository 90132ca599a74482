"""Helper of the memory-contract tests: guard bands around every tensor handed to the C ABI, and poisoned outputs and scratch.

GPU AddressSanitizer is not available to this project; this is the substitute.  A tensor lives in the middle of ONE allocation
whose head and tail ("guards") hold a known byte; after the call the guards must still hold it.  The same call is run three
times (run_three_ways): plainly on zeroed outputs and scratch, then with everything poisoned with 0xFF (NaN as fp32, bf16 and
fp64; 65535 as uint16, -1 as int32), then with 0x7F (about 3.39e38 as fp32 and bf16, huge as fp64, finite: relu = fmaxf(v, 0)
swallows a NaN, it cannot swallow this).  The three runs must give the same BITS, which fails for an output element left
unwritten, a result that depends on what the scratch held, a read of a neighbour that reaches the result, and nondeterminism;
the guards fail for a write outside.  tests/test_guarded_host.py shows each of these failing on CPU tensors."""
import numpy as np
import torch

GUARD_MIN = 64 << 10
PAGE = 4096
POISONS = (0xFF, 0x7F)


def _numel(shape):
    n = 1
    for s in shape:
        n *= int(s)
    return n


def _describe(raw_bytes, first, dtype, count=6):
    """A few values of `dtype` from the uint8 tensor raw_bytes, starting at the element that holds byte `first`."""
    size = torch.empty((), dtype=dtype).element_size()
    start = first - first % size
    stop = min(start + count * size, raw_bytes.numel() - raw_bytes.numel() % size)
    chunk = raw_bytes[start:stop].cpu().contiguous()
    return chunk.view(dtype).tolist(), chunk.tolist()


class Guarded(object):
    """A contiguous tensor `.t` of `shape` and `dtype` inside ONE uint8 allocation guard | payload | guard, every byte `fill`."""

    def __init__(self, shape, dtype, device, fill):
        shape = tuple(int(s) for s in (shape if hasattr(shape, '__len__') else (shape,)))
        device = torch.device(device)
        self.dtype, self.fill = dtype, int(fill)
        self.payload = _numel(shape) * torch.empty((), dtype=dtype).element_size()
        self.guard = max(GUARD_MIN, -(-self.payload // PAGE) * PAGE)
        total = 2 * self.guard + self.payload
        if device.type == 'cuda':
            self.raw = torch.empty(total, dtype=torch.uint8, device=device)
        else:
            # the host allocator aligns to 64 bytes only: take the page-aligned window of one larger allocation
            self._base = torch.empty(total + PAGE, dtype=torch.uint8, device=device)
            skip = -self._base.data_ptr() % PAGE
            self.raw = self._base[skip:skip + total]
        self.raw.fill_(self.fill)
        assert self.guard % PAGE == 0
        self.t = self.raw[self.guard:self.guard + self.payload].view(dtype).view(shape)
        if self.payload == 0:              # an empty tensor has no address: nothing to align
            return
        assert self.t.is_contiguous() and self.t.data_ptr() == self.raw.data_ptr() + self.guard
        assert self.t.data_ptr() % 512 == 0,'the interior at %#x lost the alignment of an allocation' % self.t.data_ptr()

    def check(self, what):
        """Both guards still hold `fill` in every byte."""
        for side, lo, hi in (('head', 0, self.guard), ('tail', self.guard + self.payload, 2 * self.guard + self.payload)):
            g = self.raw[lo:hi]
            if bool((g == self.fill).all()):
                continue
            bad = (g != self.fill).nonzero().flatten()
            first, last = int(bad[0]), int(bad[-1])
            # byte offsets relative to the interior: negative in front of it, from its end behind it
            rel = (first - self.guard, last - self.guard) if side == 'head' else (first, last)
            where = 'bytes %d..%d before the first element' % (-rel[0], -rel[1]) if side == 'head' else \
                'bytes %d..%d past the last element' % rel
            values, raw = _describe(g, first, self.dtype)
            raise AssertionError('%s: the %s guard was written: %d of %d bytes changed, %s (guard byte %#04x); '
                                 'as %s from the first changed element: %r (bytes %r)'
                                 % (what, side, bad.numel(), g.numel(), where, self.fill, self.dtype, values, raw[:16]))


def _bytes(t):
    return t.contiguous().view(-1).view(torch.uint8)


def _assert_same_bits(got, want, what, poison):
    """got == want in their bits (NaN payloads and -0.0 count), through integer views."""
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    gb, wb = _bytes(got), _bytes(want)
    if torch.equal(gb, wb):
        return
    size = got.element_size()
    bad = (gb != wb).view(-1, size).any(dim=1).nonzero().flatten()
    first, last = int(bad[0]), int(bad[-1])
    shape = tuple(got.shape)
    lines = []
    for k in bad[:8].tolist():
        idx = tuple(int(v) for v in np.unravel_index(k, shape)) if shape else ()
        g, w = gb[k * size:(k + 1) * size].cpu(), wb[k * size:(k + 1) * size].cpu()
        note = ' (still the poison: never written)' if bool((g == poison).all()) else ''
        lines.append('%r byte offset %d: got %r want %r%s' % (idx, k * size, g.view(got.dtype).item(), w.view(got.dtype).item(), note))
    raise AssertionError('%s: %d of %d elements differ in their bits from the plain run (zeroed outputs and scratch), elements '
                         '%d..%d (byte offsets %d..%d), poison byte %#04x:\n  %s'
                         % (what, bad.numel(), gb.numel() // size, first, last, first * size, last * size + size - 1, poison,
                            '\n  '.join(lines)))


def _spec(s):
    """An output or scratch description -> (shape, dtype): a byte count is uint8 scratch of exactly that size."""
    if isinstance(s, int):
        return (s,), torch.uint8
    return tuple(s[0]), s[1]


def _sync(device):
    if torch.device(device).type == 'cuda':
        torch.cuda.synchronize(device)


def run_three_ways(call, inputs, outputs, inplace=(), scratch=(), device=None, what=''):
    """call(inputs, outputs, inplace, scratch) launches ONE entry point on the tensors it is given (lists, in the order of the
    arguments here) and does not allocate anything the library writes.

    inputs:  tensors the entry point only reads (None is passed through: an optional pointer);
    outputs: (shape, dtype) of every tensor it must write completely;
    inplace: tensors it reads and updates;
    scratch: byte counts (or (shape, dtype)) of workspaces, from the library's own size function.

    (a) plain torch tensors, outputs and scratch zeroed; (b) every tensor in a Guarded of fill 0xFF, outputs and scratch 0xFF
    throughout; (c) the same with 0x7F.  After (b) and (c): every guard intact, the inputs unchanged, every output and in-place
    tensor equal to (a) in its bits.  Returns (outputs, inplace) of run (a)."""
    if device is None:
        device = next(t.device for t in list(inputs) + list(inplace) if t is not None)
    outputs, scratch = [_spec(s) for s in outputs], [_spec(s) for s in scratch]
    base_out = [torch.zeros(shape, dtype=dtype, device=device) for shape, dtype in outputs]
    base_inp = [t.clone() for t in inplace]
    plain_in = [None if t is None else t.clone() for t in inputs]
    call(plain_in, base_out, base_inp, [torch.zeros(shape, dtype=dtype, device=device) for shape, dtype in scratch])
    _sync(device)
    for i, (c, t) in enumerate(zip(plain_in, inputs)):
        if t is not None:
            _assert_same_bits(c, t, '%s, plain run: input %d was modified' % (what, i), 0x00)
    for poison in POISONS:
        tag = '%s, poison %#04x' % (what, poison)
        g_in = [None if t is None else Guarded(t.shape, t.dtype, device, poison) for t in inputs]
        g_out = [Guarded(shape, dtype, device, poison) for shape, dtype in outputs]
        g_inp = [Guarded(t.shape, t.dtype, device, poison) for t in inplace]
        g_scr = [Guarded(shape, dtype, device, poison) for shape, dtype in scratch]
        for g, t in zip(g_in + g_inp, list(inputs) + list(inplace)):
            if g is not None:
                g.t.copy_(t)
        call([None if g is None else g.t for g in g_in], [g.t for g in g_out], [g.t for g in g_inp], [g.t for g in g_scr])
        _sync(device)
        for name, group in (('input', g_in), ('output', g_out), ('in-place tensor', g_inp), ('scratch', g_scr)):
            for i, g in enumerate(group):
                if g is not None:
                    g.check('%s: %s %d %r' % (tag, name, i, tuple(g.t.shape)))
        for i, (g, t) in enumerate(zip(g_in, inputs)):
            if g is not None:
                _assert_same_bits(g.t, t, '%s: input %d was modified' % (tag, i), poison)
        for i, (g, t) in enumerate(zip(g_out, base_out)):
            _assert_same_bits(g.t, t, '%s: output %d' % (tag, i), poison)
        for i, (g, t) in enumerate(zip(g_inp, base_inp)):
            _assert_same_bits(g.t, t, '%s: in-place tensor %d' % (tag, i), poison)
    return base_out, base_inp
