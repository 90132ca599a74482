"""tests/guarded.py can fail: stand-in "kernels" (Python functions on CPU tensors) commit each violation the memory-contract
tests look for, and run_three_ways must report it with the side and the offset.  A well-behaved stand-in passes."""
import re

import pytest
import torch

from guarded import GUARD_MIN, Guarded, run_three_ways

CPU = torch.device('cpu')


def _outside(t, element):
    """One element at `element` (negative: in front of t, >= numel: behind it) of the storage t lives in — what a kernel does
    with a pointer and a wrong index."""
    return torch.as_strided(t, (1,), (1,), t.storage_offset() + element)


def _good(inputs, outputs, inplace, scratch):
    x, = inputs
    scratch[0][:x.numel() * 4].view(torch.float32).copy_(x.flatten() * 2)       # scratch written before it is read
    outputs[0].copy_(scratch[0][:x.numel() * 4].view(torch.float32).view(x.shape) + 1)
    inplace[0].add_(x)


def _args(kernel):
    x = torch.arange(15, dtype=torch.float32).reshape(3, 5) - 7
    p = torch.linspace(-1, 1, 15).reshape(3, 5).clone()
    return dict(call=kernel, inputs=[x], outputs=[((3, 5), torch.float32)], inplace=[p], scratch=[15 * 4], what='stand-in')


def test_a_well_behaved_kernel_passes_and_returns_the_plain_run():
    out, inp = run_three_ways(**_args(_good))
    x = torch.arange(15, dtype=torch.float32).reshape(3, 5) - 7
    assert torch.equal(out[0], x * 2 + 1) and torch.equal(inp[0], torch.linspace(-1, 1, 15).reshape(3, 5) + x)


def test_an_optional_null_input_is_passed_through():
    seen = []

    def kernel(inputs, outputs, inplace, scratch):
        seen.append(inputs[1])
        outputs[0].copy_(inputs[0])
    run_three_ways(kernel, [torch.ones(4), None], [((4,), torch.float32)])
    assert seen == [None, None, None]


def test_a_write_in_front_of_the_output_is_reported_with_side_and_offset():
    def kernel(inputs, outputs, inplace, scratch):
        _good(inputs, outputs, inplace, scratch)
        if outputs[0].storage_offset():                        # the plain run has nothing in front: only the guarded runs stray
            _outside(outputs[0], -1).fill_(3.5)
    with pytest.raises(AssertionError) as e:
        run_three_ways(**_args(kernel))
    msg = str(e.value)
    assert 'output 0' in msg and 'head guard' in msg and 'bytes 4..1 before the first element' in msg
    assert '4 of %d bytes' % GUARD_MIN in msg or '3 of %d bytes' % GUARD_MIN in msg      # 3.5 = 00 00 60 40: no byte is 0xff
    assert '[3.5' in msg


def test_a_write_behind_an_in_place_tensor_is_reported_with_side_and_offset():
    def kernel(inputs, outputs, inplace, scratch):
        _good(inputs, outputs, inplace, scratch)
        if inplace[0].storage_offset():
            _outside(inplace[0], inplace[0].numel() + 2).fill_(-2.0)       # two elements past the end, as a stride error would
    with pytest.raises(AssertionError) as e:
        run_three_ways(**_args(kernel))
    msg = str(e.value)
    assert 'in-place tensor 0' in msg and 'tail guard' in msg and re.search(r'bytes (8|9|10|11)\.\.11 past the last element', msg)
    assert '-2.0' in msg


def test_a_write_behind_the_scratch_means_the_size_function_is_short():
    def kernel(inputs, outputs, inplace, scratch):
        _good(inputs, outputs, inplace, scratch)
        if scratch[0].storage_offset():
            _outside(scratch[0], scratch[0].numel()).fill_(1)
    with pytest.raises(AssertionError) as e:
        run_three_ways(**_args(kernel))
    assert 'scratch 0' in str(e.value) and 'tail guard' in str(e.value) and 'bytes 0..0 past the last element' in str(e.value)


def test_an_output_element_left_unwritten_is_reported_with_its_index_and_offset():
    def kernel(inputs, outputs, inplace, scratch):
        keep = outputs[0][2, 3].clone()
        _good(inputs, outputs, inplace, scratch)
        outputs[0][2, 3] = keep
    with pytest.raises(AssertionError) as e:
        run_three_ways(**_args(kernel))
    msg = str(e.value)
    assert 'output 0' in msg and '1 of 15 elements' in msg and '(2, 3) byte offset 52' in msg and 'never written' in msg


def test_a_scratch_byte_that_reaches_the_output_is_reported():
    def kernel(inputs, outputs, inplace, scratch):
        stale = scratch[0][7].clone()                         # read before anything wrote it
        _good(inputs, outputs, inplace, scratch)
        outputs[0].view(-1).view(torch.uint8)[4 * 6] = stale
    with pytest.raises(AssertionError) as e:
        run_three_ways(**_args(kernel))
    msg = str(e.value)
    assert 'output 0' in msg and '1 of 15 elements' in msg and '(1, 1) byte offset 24' in msg and 'poison 0xff' in msg


def test_a_huge_finite_neighbour_is_caught_where_a_nan_is_swallowed():
    """relu(v) = max(v, 0) as fmaxf computes it drops a NaN: the stray read in front of it shows only under the 0x7f poison."""
    def kernel(inputs, outputs, inplace, scratch):
        x = inputs[0]
        stray = _outside(x, -1) if x.storage_offset() else torch.zeros(1)
        v = x.flatten().clone()
        v[0] += 1e-30 * stray[0]                                                    # x[0] = -7: relu gives 0 with and without a NaN
        outputs[0].copy_(torch.where(v > 0, v, torch.zeros(())).view(x.shape))      # v > 0 is false for NaN: fmaxf(v, 0)
    with pytest.raises(AssertionError) as e:
        run_three_ways(kernel, [torch.arange(15, dtype=torch.float32).reshape(3, 5) - 7], [((3, 5), torch.float32)])
    assert 'poison 0x7f' in str(e.value) and 'output 0' in str(e.value)


def test_a_modified_input_and_a_nondeterministic_result_are_reported():
    def writes_input(inputs, outputs, inplace, scratch):
        outputs[0].copy_(inputs[0])
        inputs[0][0] = 9
    with pytest.raises(AssertionError, match='input 0 was modified'):
        run_three_ways(writes_input, [torch.ones(4)], [((4,), torch.float32)])
    calls = []

    def drifts(inputs, outputs, inplace, scratch):
        calls.append(0)
        outputs[0].copy_(inputs[0] + (len(calls) == 3))
    with pytest.raises(AssertionError, match='poison 0x7f: output 0'):
        run_three_ways(drifts, [torch.ones(4)], [((4,), torch.float32)])


@pytest.mark.parametrize('shape,dtype', [((), torch.float32), ((3, 7, 9, 8), torch.int16), ((300, 301), torch.float64), ((0,), torch.uint8)])
def test_guarded_layout(shape, dtype):
    for fill in (0xFF, 0x7F):
        g = Guarded(shape, dtype, CPU, fill)
        payload = g.t.numel() * g.t.element_size()
        assert tuple(g.t.shape) == shape and g.t.dtype == dtype and g.t.is_contiguous()
        assert g.raw.numel() == 2 * g.guard + payload and g.guard >= max(GUARD_MIN, payload) and g.guard % 4096 == 0
        assert g.guard - payload <= max(GUARD_MIN, 4095)
        assert payload == 0 or (g.t.data_ptr() - g.raw.data_ptr() == g.guard and g.t.data_ptr() % 512 == 0)
        assert bool((g.raw == fill).all())
        g.check('fresh')
    nan = Guarded((2,), torch.float32, CPU, 0xFF).t
    big = Guarded((2,), torch.bfloat16, CPU, 0x7F).t
    assert bool(torch.isnan(nan).all()) and bool(torch.isfinite(big).all()) and float(big[0]) > 3.3e38
    assert bool(torch.isfinite(Guarded((1,), torch.float64, CPU, 0x7F).t).all())
