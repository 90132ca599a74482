"""Data-parallel fine-tuning, host side (no GPU): the C ABI of dsen2_nadam_step_shards and its refusals, the shard arithmetic, the
count-weighted loss, the all-gather of rows and the replica check over gloo, and the training CLI's flag."""
import ctypes
import os
import re
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.distributed as td
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def test_nadam_step_shards_is_declared_exported_and_refuses_bad_arguments():
    """Every refusal comes before anything is launched (no device is needed, none is touched): the pointers are never followed."""
    from dsen2_amd import _lib, build
    build.build()
    lib = _lib.load()
    header = open(os.path.join(ROOT, 'include', 'dsen2_hip.h')).read()
    name = 'dsen2_nadam_step_shards'
    assert re.search(r'\bint %s\s*\(' % name, header) and name in _lib.SIGNATURES and hasattr(lib, name)
    fake = ctypes.c_void_p(4096)          # a non-NULL pointer that a refused call must not follow
    scalars = (1e-3, 0.9, 0.999, 1e-8, 0.5, 0.5, 0.5, 0.25, 0.999)

    def refused(shards, counts, stride=100, count=100, p=fake, g=fake, m=fake, v=fake, counts_ptr=True):
        arr = (ctypes.c_int * max(1, len(counts)))(*counts) if counts_ptr else None
        rc = lib.dsen2_nadam_step_shards(p, g, stride, shards, arr, None, m, v, count, *(scalars + (None,)))
        assert rc == _lib.ERR_INVALID, (shards, counts, rc)
        msg = lib.dsen2_last_error().decode()
        assert msg
        return msg
    assert 'shards' in refused(0, [])
    assert 'shards' in refused(-1, [])
    assert 'shards' in refused(65, [1] * 65)
    assert 'negative' in refused(2, [3, -1])
    assert 'zero' in refused(3, [0, 0, 0])
    assert '2^24' in refused(2, [1, 1 << 24])
    assert 'shard_stride' in refused(2, [1, 1], stride=99)
    assert 'NULL' in refused(1, [1], counts_ptr=False)
    for k in ('p', 'g', 'm', 'v'):
        assert 'NULL' in refused(1, [1], **{k: None})
    # the largest count and the largest number of shards are NOT refused for their size: with count = 0 nothing is launched
    arr = (ctypes.c_int * 64)(*([(1 << 24) - 1] * 64))
    assert lib.dsen2_nadam_step_shards(None, None, 0, 64, arr, None, None, None, 0, *(scalars + (None,))) == _lib.OK


def test_shard_counts_add_up_to_the_batch():
    from dsen2_amd import dist
    want = {(5, 2): [3, 2], (5, 3): [2, 2, 1], (2, 3): [1, 1, 0], (7, 3): [3, 3, 1], (5, 1): [5]}
    for (n, world), counts in want.items():
        spans = [dist.shard_range(n, r, world) for r in range(world)]
        assert [c for _, c in spans] == counts and sum(counts) == n
        assert [f for f, _ in spans] == list(np.cumsum([0] + counts)[:-1])          # contiguous, in rank order


def test_count_weighted_loss_on_hand_made_numbers():
    """[sum n_r mae_r / n, sum n_r mse_r / n] in float64, in shard order; the row of a shard without samples is never read."""
    from dsen2_amd.DSen2Net import S2Model
    loss2 = np.array([[0.5, 0.25], [2.0, 4.0], [np.nan, np.inf]])
    got = S2Model.weighted_loss(loss2, [3, 2, 0])
    assert got == [(3 * 0.5 + 2 * 2.0) / 5, (3 * 0.25 + 2 * 4.0) / 5] == [1.1, 1.75]
    assert S2Model.weighted_loss(loss2[:1], [7]) == [0.5, 0.25]
    # float32 losses are widened, not rounded again: 0.1f stays 0.1f
    f = np.float32(0.1)
    assert S2Model.weighted_loss(np.array([[f, f]], np.float32), [3]) == [float(f), float(f)]


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    td.init_process_group('gloo', rank=rank, world_size=world)
    try:
        from dsen2_amd import dist
        n = 1003
        send = torch.arange(n, dtype=torch.float32) + 10000.0 * rank
        rows = dist.all_gather_rows(send)
        ok = tuple(rows.shape) == (world, n) and rows.dtype == torch.float32
        ok = ok and all(torch.equal(rows[r], torch.arange(n, dtype=torch.float32) + 10000.0 * r) for r in range(world))
        # float64 triples travel the same way (the validation sums)
        t = dist.all_gather_rows(torch.tensor([rank + 0.1, 2.0, 3.0], dtype=torch.float64))
        ok = ok and t.dtype == torch.float64 and [float(v) for v in t[:, 0]] == [r + 0.1 for r in range(world)]
        # identical replicas pass (NaN patterns and -0.0 included: the check is on bits) ...
        flat = torch.linspace(-1, 1, n)
        flat[5], flat[6] = float('nan'), -0.0
        dist.assert_replicas_identical(flat)
        # ... one flipped low bit on rank 1 raises on EVERY rank and names rank 1
        if rank == 1:
            flat.view(torch.int32)[17] ^= 1
        try:
            dist.assert_replicas_identical(flat)
            ok = False
        except RuntimeError as e:
            ok = ok and 'rank 1 ' in str(e)
        # -0.0 against 0.0 is a difference too
        z = torch.zeros(8)
        if rank == 1:
            z[3] = -0.0
        try:
            dist.assert_replicas_identical(z)
            ok = False
        except RuntimeError as e:
            ok = ok and 'rank 1 ' in str(e)
        q.put((rank, bool(ok)))
    finally:
        td.destroy_process_group()


@pytest.mark.parametrize('world', [2, 3])
def test_all_gather_rows_and_replica_check_over_gloo(world):
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    res = dict(q.get(timeout=10) for _ in range(world))
    assert res == {r: True for r in range(world)}


def test_single_process_gather_and_check_are_the_identity():
    from dsen2_amd import dist
    send = torch.arange(5, dtype=torch.float32)
    rows = dist.all_gather_rows(send)
    assert tuple(rows.shape) == (1, 5) and rows.data_ptr() == send.data_ptr()
    dist.assert_replicas_identical(send)
    assert int(dist.weights_checksum(torch.tensor([1.0, -0.0]))) == 0x3f800000 - 0x80000000


def test_train_cli_lists_data_parallel_and_still_refuses_without_it():
    r = subprocess.run([sys.executable, '-m', 'dsen2_amd.train', '--help'], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert '--data_parallel' in r.stdout and '--backend' in r.stdout
    env = dict(os.environ, WORLD_SIZE='2')
    r = subprocess.run([sys.executable, '-m', 'dsen2_amd.train', '--epochs', '1'], cwd=ROOT, capture_output=True, text=True,
                       timeout=120, env=env)
    assert r.returncode == 2 and 'WORLD_SIZE' in r.stderr and '--data_parallel' in r.stderr
    # predicting is not a data-parallel job: refused with the flag too
    r = subprocess.run([sys.executable, '-m', 'dsen2_amd.train', '--data_parallel', '--predict', 'x.npy'], cwd=ROOT, capture_output=True,
                       text=True, timeout=120, env=env)
    assert r.returncode == 2 and 'WORLD_SIZE' in r.stderr
