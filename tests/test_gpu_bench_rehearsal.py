"""The N>1 control flow of bench.py (weight broadcast, per-step async output gather, barriers, max-over-ranks
timing, one JSON line from rank 0) rehearsed with 2 ranks on ONE GPU over gloo.  Not a measurement."""
import json
import os
import socket
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return str(p)


def test_bench_two_ranks_gloo_rehearsal():
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2', '--master-addr',
           '127.0.0.1', '--master-port', _free_port(), os.path.join(ROOT, 'bench.py'), '--gpus', '2', '--steps', '2',
           '--warmup', '1', '--batch', '64', '--backend', 'gloo', '--full', '--roofline-seconds', '0.5', '--sustain-seconds', '0.3']
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1                               # exactly one JSON line, from rank 0
    r = json.loads(lines[0])
    assert r['n_gpus'] == 2 and r['steps'] == 2 and r['scaling'] == 'weak' and r['config']['output_gather'] is True
    assert r['value'] > 0 and 'roofline' in r and 'cpu_baseline' not in r and 'other_configs' not in r
    # an N > 1 line explains itself (VERDICT r4 #1b): the collectives saw both ranks, each rank's own step, the time a
    # stream (gloo: the host) stood waiting for a gather, and the same K steps with the gather off
    assert r['ranks_in_collective'] == 2
    assert set(r['dist_setup_s']) == {'init_process_group(gloo)', 'first all_reduce', 'broadcast of the weights (C1)'}
    pr = r['per_rank_ms_per_step']
    assert len(pr['ranks']) == 2 and 0 < pr['min'] <= pr['max'] <= r['ms_per_step'] * 1.001
    gwait = r['gather_wait_ms_per_step']
    assert len(gwait['ranks']) == 2 and gwait['host_max'] >= 0
    assert 0 < r['ms_per_step_no_gather'] and r['value_no_gather'] > 0
    assert r['per_rank_ms_per_step_no_gather']['max'] <= r['ms_per_step_no_gather'] * 1.001


def test_bench_two_ranks_without_gather_still_reports_the_ranks():
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2', '--master-addr',
           '127.0.0.1', '--master-port', _free_port(), os.path.join(ROOT, 'bench.py'), '--gpus', '2', '--steps', '2',
           '--warmup', '1', '--batch', '64', '--backend', 'gloo', '--full', '--roofline-seconds', '0.3', '--sustain-seconds', '0', '--no-gather']
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    r = json.loads([l for l in p.stdout.splitlines() if l.startswith('{')][0])
    assert r['config']['output_gather'] is False and r['gather_wait_ms_per_step'] is None and r['ranks_in_collective'] == 2


def test_bench_with_a_missing_rank_exits_fast_and_names_the_step():
    """WORLD_SIZE=2 but only rank 0 is started (what a rank that died in start-up looks like to its peer): bench.py must not
    wait torch's 10 minutes — it leaves within DSEN2_DIST_TIMEOUT with the step's name on stderr and no JSON line."""
    import time
    env = dict(os.environ, RANK='0', LOCAL_RANK='0', WORLD_SIZE='2', MASTER_ADDR='127.0.0.1', MASTER_PORT=_free_port(),
               DSEN2_DIST_TIMEOUT='8')
    t0 = time.time()
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '2', '--backend', 'gloo'],
                       capture_output=True, text=True, timeout=300, cwd=ROOT, env=env)
    assert p.returncode != 0 and time.time() - t0 < 120
    assert 'init_process_group(gloo)' in p.stderr and not [l for l in p.stdout.splitlines() if l.startswith('{')]


def test_bench_single_gpu_line_has_contract_fields():
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--steps', '2', '--warmup', '1', '--full', '--cpu-budget', '2', '--roofline-seconds', '0.5', '--sustain-seconds', '0.3'],
                       capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    r = json.loads([l for l in p.stdout.splitlines() if l.startswith('{')][0])
    for k in ('metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup', 'ms_per_step', 'higher_is_better', 'scaling',
              'vs_baseline', 'dtype', 'data', 'config', 'roofline', 'cpu_baseline'):
        assert k in r, k
    assert r['dtype'] == 'f32' and r['vs_baseline'] is None and r['roofline']['bound'] == 'mfma'
    assert 0 < r['roofline']['frac'] <= 1 and r['cpu_baseline']['kind'] == 'port'
    # N = 1 carries nothing of the multi-rank diagnostics
    assert not ({'ranks_in_collective', 'per_rank_ms_per_step', 'gather_wait_ms_per_step', 'ms_per_step_no_gather'} & set(r))
    # BASELINE configs[2] and configs[4] ride along on the same box
    oc = r['other_configs']
    assert set(oc) == {'dsen2_60_fp32', 'vdsen2_20_bf16'}
    for name, dtype, peak in (('dsen2_60_fp32', 'f32', 157.3), ('vdsen2_20_bf16', 'bf16', 2500.0)):
        c = oc[name]
        assert c['dtype'] == dtype and c['peak_tflops'] == peak and c['finite'] and c['value'] > 0
        assert 0.3 < c['roofline_frac'] <= 1.0 and c['launches_per_forward'] >= 1
        assert abs(c['value'] * c['ms_per_step'] * 1e-3 - c['batch']) < 1e-3 * c['batch']
    assert oc['dsen2_60_fp32']['launches_per_forward'] == 12 and oc['vdsen2_20_bf16']['launches_per_forward'] == 1


def test_bench_plain_line_is_the_headline_alone_and_dumps_the_last_step(tmp_path):
    """Without --full the line carries the headline and nothing measured beside it; --dump-outputs writes the last timed
    step's output, which is the network on the bench's own inputs (PCG64(0), he_uniform seed 1) by the float64 C oracle."""
    import numpy as np
    sys.path.insert(0, ROOT)
    from dsen2_amd import weights as dweights
    from oracle import c_oracle, dsen2_oracle as do          # checker only
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--steps', '3', '--warmup', '1', '--dump-outputs', str(tmp_path)],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    r = json.loads([l for l in p.stdout.splitlines() if l.startswith('{')][0])
    assert r['steps'] == 3 and r['warmup'] == 1 and r['dtype'] == 'f32' and r['higher_is_better'] is True and r['unit'] == 'patches/s'
    assert abs(r['value'] * r['ms_per_step'] * 1e-3 - 512) < 1e-2 * 512
    assert not ({'roofline', 'cpu_baseline', 'rmse_vs_cpu_fp32', 'other_configs'} & set(r))
    assert sorted(os.listdir(str(tmp_path))) == ['output.npy']
    y = np.load(str(tmp_path / 'output.npy'))
    assert y.dtype == np.float32 and y.shape == (512, 6, 32, 32) and np.isfinite(y).all()
    xs = [a[:4] for a in do.synthetic_inputs(512, 32, 32, (4, 6), seed=0)]      # rank 0's batch: same generator, same order
    ref = c_oracle.forward(xs, dweights.random_he_uniform(10, 6, 6, 128, seed=1), 6, 128)
    assert do.rmse(y[:4], ref) < 1e-4


def test_bench_line_closes_on_itself_and_other_configs_run():
    """The roofline object of the default line: launches x ms_per_launch + first_ms + out_ms = forward_ms (same events), the
    traffic figure is quoted only with the ISA hash of this build; the bf16x3 config reports dtype "bf16x3" against the bf16
    peak with three MFMAs per product and never claims the headline metric."""
    def line(*extra):
        p = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--steps', '3', '--warmup', '2', '--full', '--no-cpu-baseline', '--roofline-seconds', '0.5', '--sustain-seconds', '0.3'] + list(extra),
                           capture_output=True, text=True, timeout=900, cwd=ROOT)
        assert p.returncode == 0, p.stderr[-2000:]
        return json.loads([l for l in p.stdout.splitlines() if l.startswith('{')][0])
    r = line()
    rl = r['roofline']
    assert abs(rl['launches_per_forward'] * rl['ms_per_launch'] + rl['first_ms'] + rl['out_ms'] - rl['forward_ms']) < 2e-3
    assert abs(rl['closure_ms'] - rl['forward_ms']) < 2e-3 and rl['replay_ms_per_step'] > 0
    assert rl['traffic'] is None or 'STALE' not in rl['traffic_source']
    assert (rl['traffic'] is None) == ('STALE' in rl['traffic_source'] or 'no committed' in rl['traffic_source'])
    x = line('--config', 'dsen2_20_bf16x3')
    assert x['dtype'] == 'bf16x3' and x['roofline']['peak'] == 2500.0 and 'bf16x3' in x['metric'] and x['metric'] != r['metric']
    assert abs(x['roofline']['achieved'] / x['roofline']['algorithmic_tflops'] - 3.0) < 0.01
    assert x['value'] > 1.5 * r['value']                      # the go / no-go threshold of the mode (measured: 3.0-3.1 x)


def test_full_tile_two_ranks_gloo_matches_single_rank():
    """supres._run patch sharding + slab uploads + dist.gather_to_root with 2 ranks (gloo, both on the one GPU): the
    image rank 0 returns equals the single-rank image bit for bit; rank 1 returns None."""
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2', '--master-addr',
           '127.0.0.1', '--master-port', _free_port(), os.path.join(ROOT, 'tools', 'bench_full_tile.py'), '--size', '600',
           '--skip60', '--backend', 'gloo', '--check']
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    r = json.loads([l for l in p.stdout.splitlines() if l.startswith('{')][0])
    assert r['n_gpus'] == 2 and r['patches20'] == 36 and r['matches_single_rank'] is True


def test_full_tile_two_ranks_read_only_their_rows():
    """Images handed over as cli.LazyRows (what the GDAL branch of the command line does under torch.distributed): each of
    two ranks reads the rows its patches need — about half the tile, not all of it — and the result is the single-rank image."""
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2', '--master-addr',
           '127.0.0.1', '--master-port', _free_port(), os.path.join(ROOT, 'tools', 'bench_full_tile.py'), '--size', '1200',
           '--backend', 'gloo', '--check', '--lazy', '192']
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    r = json.loads([l for l in p.stdout.splitlines() if l.startswith('{')][0])
    assert r['n_gpus'] == 2 and r['matches_single_rank'] is True
    assert 0.45 < r['largest_share_of_rows_read_by_a_rank'] < 0.85, r        # half the tile + the margin kept for DSen2_60's window


def test_full_tile_three_ranks_gloo_uneven_shards():
    """3 ranks over 36 patches of a non-dividing tile size (uneven shards, ragged last tile row/column)."""
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '3', '--master-addr',
           '127.0.0.1', '--master-port', _free_port(), os.path.join(ROOT, 'tools', 'bench_full_tile.py'), '--size', '570',
           '--skip60', '--backend', 'gloo', '--check']
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    r = json.loads([l for l in p.stdout.splitlines() if l.startswith('{')][0])
    assert r['n_gpus'] == 3 and r['matches_single_rank'] is True


def test_full_tile_four_ranks_gloo_on_one_gpu():
    """Four ranks sharing the card (the box allows 6 processes on it, this test process included): 36 patches of a 600^2
    tile, 9 per rank, every rank's row slab overlapping its neighbours' by the patches' borders; DSen2_60 too (16 patches,
    4 per rank)."""
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '4', '--master-addr',
           '127.0.0.1', '--master-port', _free_port(), os.path.join(ROOT, 'tools', 'bench_full_tile.py'), '--size', '600',
           '--backend', 'gloo', '--check']
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    r = json.loads([l for l in p.stdout.splitlines() if l.startswith('{')][0])
    assert r['n_gpus'] == 4 and r['patches20'] == 36 and r['matches_single_rank'] is True


@pytest.mark.parametrize('ranks,size,chunks,extra', [(2, 600, 8, []), (3, 570, 8, ['--skip60']), (4, 600, 3, []), (2, 240, 8, ['--skip60']), (4, 600, 50, ['--skip60'])])
def test_full_tile_chunked_gather_matches_single_rank(ranks, size, chunks, extra):
    """DSEN2_CHUNKED_GATHER=1: the crops travel in pieces while the shards compute and rank 0 recomposes +
    downloads what has arrived — the image must be the single-rank image bit for bit.  2 / 3 / 4 ranks (gloo, one GPU):
    even and uneven shards, a ragged last tile row (570), DSen2_60 too, a 240^2 image whose 9 patches leave short and uneven
    shards, and more pieces asked for than a shard has slots."""
    env = dict(os.environ, DSEN2_CHUNKED_GATHER='1', DSEN2_GATHER_CHUNKS=str(chunks), DSEN2_PINNED_OUTPUT='1')
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', str(ranks), '--master-addr',
           '127.0.0.1', '--master-port', _free_port(), os.path.join(ROOT, 'tools', 'bench_full_tile.py'), '--size', str(size),
           '--backend', 'gloo', '--check'] + extra
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    assert p.returncode == 0, p.stderr[-2000:]
    r = json.loads([l for l in p.stdout.splitlines() if l.startswith('{')][0])
    assert r['n_gpus'] == ranks and r['chunked_gather'] is True and r['matches_single_rank'] is True


_RCCL_ONE_RANK = r'''
import os, sys
import torch
import torch.distributed as td
dev = torch.device('cuda', 0)
torch.cuda.set_device(dev)
td.init_process_group('nccl', rank=0, world_size=1, device_id=dev)
assert td.get_backend() == 'nccl'
# the collectives bench.py / dsen2_amd.dist issue, with the tensor placement they use (all on the GPU)
w = torch.arange(1000, dtype=torch.float32, device=dev)
td.broadcast(w, src=0)
out = torch.full((8, 6, 32, 32), 3.0, device=dev)
recv = torch.empty((8, 6, 32, 32), device=dev)
h = td.gather(out, list(recv.chunk(1)), dst=0, async_op=True)
h.wait()
td.barrier()
t = torch.tensor([1.25], dtype=torch.float64, device=dev)
td.all_reduce(t, op=td.ReduceOp.MAX)
torch.cuda.synchronize()
assert torch.equal(recv, out) and float(t) == 1.25 and float(w[999]) == 999.0
td.destroy_process_group()
print('rccl one rank ok')
'''


def test_rccl_initialises_and_runs_the_bench_collectives_on_one_rank():
    """The only RCCL evidence a one-GPU box can give: backend "nccl" (= RCCL) initialises with the environment the
    product sets (HSA_ENABLE_IPC_MODE_LEGACY=0, rendezvous on 127.0.0.1) and the collectives of bench.py and
    dsen2_amd.dist (broadcast, asynchronous gather into chunks of one buffer, barrier, all_reduce MAX) run on device
    tensors.  With one rank nothing crosses xGMI: the N>1 data path stays unmeasured."""
    env = dict(os.environ, MASTER_ADDR='127.0.0.1', MASTER_PORT=_free_port(), RANK='0', WORLD_SIZE='1', LOCAL_RANK='0',
               HSA_ENABLE_IPC_MODE_LEGACY='0')
    p = subprocess.run([sys.executable, '-c', _RCCL_ONE_RANK], capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    assert p.returncode == 0 and 'rccl one rank ok' in p.stdout, (p.stdout[-500:], p.stderr[-2000:])


_RCCL_CONNECT_ONE_RANK = r'''
import torch
from dsen2_amd import dist
dev = torch.device('cuda', 0)
torch.cuda.set_device(dev)
dist.connect('nccl', 0, 1, dev)                      # the product's own entry: timeout, guarded steps, counting all-reduce
assert dist.first_contact()['ranks_in_collective'] == 1
t = torch.ones(4, device=dev)
torch.distributed.all_reduce(t)
torch.cuda.synchronize()
dist.finalize()
print('connect ok')
'''


@pytest.mark.parametrize('high_priority', ['0', '1'])
def test_dist_connect_over_rccl_on_one_rank(high_priority):
    """dist.connect over backend "nccl" as the product calls it (group timeout, guarded steps, the counting all-reduce), with
    and without DSEN2_RCCL_HIGH_PRIORITY — one rank: the most a one-GPU box can show."""
    env = dict(os.environ, MASTER_ADDR='127.0.0.1', MASTER_PORT=_free_port(), RANK='0', WORLD_SIZE='1', LOCAL_RANK='0',
               HSA_ENABLE_IPC_MODE_LEGACY='0', DSEN2_RCCL_HIGH_PRIORITY=high_priority,
               PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    p = subprocess.run([sys.executable, '-c', _RCCL_CONNECT_ONE_RANK], capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    assert p.returncode == 0 and 'connect ok' in p.stdout, (p.stdout[-500:], p.stderr[-2000:])


def test_cli_two_ranks_gloo_writes_the_single_rank_file_from_rank_0_only(tmp_path):
    """The drop-in CLI under torch.distributed.run (the stand-in for testing/s2_tiles_supres.py:332-342,371-420 on N
    GPUs): `python -m torch.distributed.run ... -m dsen2_amd.cli tile.npz out.npz` with 2 ranks (gloo rehearsal, both on
    the one GPU) enters the process group itself, shards the patches, and rank 0 alone prints and writes — the same
    bytes per band as the single-process run."""
    import numpy as np
    sys.path.insert(0, ROOT)
    from dsen2_amd import weights
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'tile_T33UUB_crop.npz'))
    inp = str(tmp_path / 'tile.npz')
    np.savez(inp, data10=g['d10'], data20=g['d20'], data60=g['d60'])
    mdl = tmp_path / 'models'
    mdl.mkdir()
    np.save(str(mdl / 's2_032_lr_1e-04.npy'), weights.random_he_uniform(10, 6, 6, 128, seed=11))
    np.save(str(mdl / 's2_030_lr_1e-05.npy'), weights.random_he_uniform(12, 2, 6, 128, seed=12))
    common = ['--run_60', '--copy_original_bands', '--models', str(mdl)]
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    single = subprocess.run([sys.executable, '-m', 'dsen2_amd.cli', inp, str(tmp_path / 'one.npz')] + common,
                            capture_output=True, text=True, timeout=600, cwd=str(tmp_path), env=env)
    assert single.returncode == 0, single.stderr[-2000:]
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2', '--master-addr', '127.0.0.1',
           '--master-port', _free_port(), '-m', 'dsen2_amd.cli', inp, str(tmp_path / 'two.npz'), '--backend', 'gloo'] + common
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(tmp_path), env=env)
    assert p.returncode == 0, p.stderr[-3000:]
    # one rank talked: every line of the single-process run appears exactly once
    assert p.stdout.count('Writing the original 10m bands and the super-resolved bands') == 1
    assert p.stdout.count('Super-resolving the 20m data into 10m bands') == 1
    one = np.load(str(tmp_path / 'one.npz'), allow_pickle=True)['bands'].item()
    two = np.load(str(tmp_path / 'two.npz'), allow_pickle=True)['bands'].item()
    assert list(one) == list(two) and len(one) == 12
    for k in one:
        assert np.array_equal(one[k], two[k]), k


def test_dist_preflight_two_ranks_gloo():
    """python -m dsen2_amd.dist: first contact + the product's two collectives at their real sizes, without the network — what an
    operator runs on a new node before the bench.  Two ranks over gloo on the one GPU: control flow and payload checks (the
    rates it prints mean nothing here)."""
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2', '--master-addr', '127.0.0.1',
           '--master-port', _free_port(), '-m', 'dsen2_amd.dist', '--backend', 'gloo', '--reps', '3', '--shard-patches', '37']
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    assert p.returncode == 0, p.stderr[-2000:]
    r = json.loads([l for l in p.stdout.splitlines() if l.startswith('{')][0])
    assert r['world'] == 2 and r['first_contact']['ranks_in_collective'] == 2
    assert r['gather_payload_ok'] is True and r['chunked_payload_ok'] is True and r['gather_12p6MB_ms'] > 0
