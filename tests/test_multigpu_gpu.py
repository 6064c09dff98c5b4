"""Multi-GPU data parallelism over RCCL / xGMI (BASELINE configs[2]), self-activating:
on a box with W = min(torch.cuda.device_count(), 8) >= 2 devices these tests launch W ranks (one process per GPU,
`python -m torch.distributed.run`, backend "nccl" = RCCL) and check

  * rank 0's initial weights and rank 0's data-initialised codebooks are on every rank,
  * mean of the shard gradients == gradient of the global batch (against the CPU oracle on the concatenated batch),
  * bit-identical parameters on all ranks after 3 training steps,
  * `bench.py --gpus W` prints one JSON line with n_gpus == W and a whole-job `value`.

On a 1-GPU box (the builder's gpurun boxes) they skip; the same contract is covered at world_size 2 on CPU/gloo by
tests/test_parallel_cpu.py, and the RCCL code path by the single-rank VQCPC_FORCE_DIST run in tests/test_decoder_gpu.py.
No scaling curve has been measured yet (no multi-GPU node was available to the builder): DESIGN.md section 6."""
import json
import os
import socket
import subprocess
import sys

import pytest
import torch

from conftest import ROOT

pytestmark = pytest.mark.gpu
WORKER = os.path.join(ROOT, 'tests', 'multigpu_worker.py')


def _world():
    n = torch.cuda.device_count() if torch.cuda.is_available() else 0
    return min(n, 8)


def _free_port():
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        return s.getsockname()[1]


def _launch(world, script, *args, timeout=900):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY='0', PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', f'--nproc-per-node={world}', '--master-addr',
           '127.0.0.1', '--master-port', str(_free_port()), script, *args]
    return subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, env=env, cwd=ROOT)


def _check_graphed_dp(res, two_graphs=True, tol=2e-6):
    """The data-parallel step as graph replays: replays happened on every rank, the replicas are still bit-identical, and
    the result equals the eager twin's (same tolerance as the single-rank graph tests)."""
    for x in res:
        assert x['graph_replays'] >= 4, x['graph_replays']
        assert x['graph_two'] == two_graphs
        assert x['graph_vs_eager'] < tol, x['graph_vs_eager']
        assert x['graph_digest'] == res[0]['graph_digest'], 'replicas must stay bit-identical through graph replays'


needs_multi = pytest.mark.skipif(_world() < 2, reason='needs >= 2 visible GPUs (self-activates on a multi-GPU node)')


@needs_multi
def test_rccl_data_parallel_training_contract(tmp_path):
    world = _world()
    r = _launch(world, WORKER, str(tmp_path))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    res = [torch.load(tmp_path / f'r{k}.pt') for k in range(world)]
    for k, x in enumerate(res):
        assert x['world'] == world and x['rank'] == k
        assert x['init_equal'], 'rank-0 broadcast of the initial weights'
        assert x['codebook_equal'], 'rank-0 data-initialised codebooks on every rank'
        assert x['grad_worst'] < 5e-4, ('mean of shard gradients vs global-batch oracle gradient', x['grad_worst'])
        assert x['idx_equal'], 'shard code assignment == oracle assignment of the same windows'
    for x in res[1:]:
        assert x['param_digest'] == res[0]['param_digest'], 'replicas must stay bit-identical after 3 steps'
        assert x['loss_global'] == res[0]['loss_global']
    _check_graphed_dp(res)


@needs_multi
def test_bench_reports_whole_job_throughput_on_all_gpus():
    world = _world()
    r = _launch(world, os.path.join(ROOT, 'bench.py'), '--gpus', str(world), '--steps', '8', '--warmup', '2', '--batch', '64')
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1, lines
    line = json.loads(lines[0])
    assert line['n_gpus'] == world and line['scaling'] == 'weak'
    assert line['config']['global_batch'] == 64 * world
    assert abs(line['value'] - 64 * world * 8 / (line['ms_per_step'] * 8e-3)) < 0.01 * line['value']


def test_single_rank_rccl_path_runs_here():
    """Always runs (1 GPU is enough): the same worker with world 1 and VQCPC_FORCE_DIST=1 goes through
    init_process_group('nccl'), the broadcasts and the flat all-reduce on this GPU."""
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY='0', VQCPC_FORCE_DIST='1', RANK='0', WORLD_SIZE='1',
                   LOCAL_RANK='0', MASTER_ADDR='127.0.0.1', MASTER_PORT=str(_free_port()),
                   PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
        r = subprocess.run([sys.executable, WORKER, d], capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        x = torch.load(os.path.join(d, 'r0.pt'))
        assert x['world'] == 1 and x['init_equal'] and x['codebook_equal'] and x['idx_equal'] and x['grad_worst'] < 5e-4
        _check_graphed_dp([x])                       # graph 1, RCCL all-reduce (eager, world 1), graph 2


def test_single_rank_rccl_all_reduce_captured_inside_the_step_graph():
    """VQCPC_DP_GRAPH=capture: ONE graph per step with the RCCL all-reduce recorded in it (torch's NCCL ops are
    capturable); single rank here, the multi-GPU test above takes the same switch on a multi-GPU node."""
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY='0', VQCPC_FORCE_DIST='1', VQCPC_DP_GRAPH='capture', RANK='0',
                   WORLD_SIZE='1', LOCAL_RANK='0', MASTER_ADDR='127.0.0.1', MASTER_PORT=str(_free_port()),
                   PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
        r = subprocess.run([sys.executable, WORKER, d], capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        x = torch.load(os.path.join(d, 'r0.pt'))
        assert x['world'] == 1 and x['grad_worst'] < 5e-4
        _check_graphed_dp([x], two_graphs=False)


def test_two_ranks_share_this_gpu_over_gloo(tmp_path):
    """Always runs (1 GPU is enough): TWO ranks, both on device 0, gradients / broadcasts over gloo (device tensors staged
    through the host).  Everything but the transport is the multi-GPU path: rank-0 weight and codebook broadcasts, shard
    gradients averaged to the global-batch gradient (vs the oracle on the concatenated batch), bit-identical replicas
    after 3 steps."""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY='0', VQCPC_DP_SHARE_GPU='1', VQCPC_DP_BACKEND='gloo',
               PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node=2', '--master-addr', '127.0.0.1',
           '--master-port', str(_free_port()), WORKER, str(tmp_path)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    res = [torch.load(tmp_path / f'r{k}.pt') for k in range(2)]
    for k, x in enumerate(res):
        assert x['world'] == 2 and x['rank'] == k
        assert x['init_equal'] and x['codebook_equal'] and x['idx_equal']
        assert x['grad_worst'] < 5e-4, x['grad_worst']
    assert res[1]['param_digest'] == res[0]['param_digest'] and res[1]['loss_global'] == res[0]['loss_global']
    _check_graphed_dp(res)                           # two graph replays per step around the (gloo) all-reduce


def test_two_ranks_share_this_gpu_over_gloo_under_the_training_defaults(tmp_path):
    """The same harness with what train_model() selects: f16x3 forward and gradient products (every eligible product forced through
    the 256-tile kernels at d_model = ff = 256).  Each rank owns its scale tables -- the amax of ITS shard -- so the shard gradients
    are computed under different scales; the contract is unchanged: mean of shard gradients == oracle gradient of the global batch,
    indices bit-exact, replicas bit-identical after the eager steps AND after the replayed steps."""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY='0', VQCPC_DP_SHARE_GPU='1', VQCPC_DP_BACKEND='gloo',
               VQCPC_TEST_TRAINING_DEFAULTS='1', PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node=2', '--master-addr', '127.0.0.1',
           '--master-port', str(_free_port()), WORKER, str(tmp_path)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    res = [torch.load(tmp_path / f'r{k}.pt') for k in range(2)]
    for k, x in enumerate(res):
        assert x['world'] == 2 and x['rank'] == k and x['f16x3_calls'] > 50, x['f16x3_calls']
        assert x['init_equal'] and x['codebook_equal'] and x['idx_equal']
        assert x['grad_worst'] < 5e-4, x['grad_worst']
    assert res[1]['param_digest'] == res[0]['param_digest'] and res[1]['loss_global'] == res[0]['loss_global']
    # the eager twin is a NEW trainer: its scale tables are primed with the current amax while the graphed trainer's follow the
    # previous step's -- another power-of-two scale wherever an amax sits near a binade boundary, i.e. other roundings of the same
    # fp32-class products, amplified by Adam over six steps (measured 9e-6 of the largest parameter); the replicas themselves
    # stay bit-identical
    _check_graphed_dp(res, tol=5e-5)


def test_student_step_bucketed_all_reduce_two_ranks_share_this_gpu(tmp_path):
    """StudentEncoderTrainer under data parallelism (BASELINE configs[3] with several ranks): the teacher's gradient range is
    all-reduced asynchronously while the encoder / decoder half runs, the rest afterwards (opt-in: VQCPC_DP_BUCKETS=2; the default is one call).
    Two ranks on this GPU over gloo: the bucketed gradients equal the single-call gradients bit for bit, replicas stay
    bit-identical through eager steps and through replays of the three-graph step, and the trajectories agree."""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY='0', VQCPC_DP_SHARE_GPU='1', VQCPC_DP_BACKEND='gloo',
               PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node=2', '--master-addr', '127.0.0.1',
           '--master-port', str(_free_port()), os.path.join(ROOT, 'tests', 'multigpu_student_worker.py'), str(tmp_path)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    res = [torch.load(tmp_path / f's{k}.pt') for k in range(2)]
    for k, x in enumerate(res):
        assert x['world'] == 2 and x['rank'] == k
        assert x['grads_equal'], ('bucketed vs single-call all-reduce', x['grad_rel'])
        assert x['stages'] == 3 and x['replays'] == 5, (x['stages'], x['replays'])
        assert x['graph_vs_eager'] < 2e-6, x['graph_vs_eager']
        assert x['single_vs_bucketed'] < 2e-6, x['single_vs_bucketed']       # same gradients, other launch order
    assert res[0]['digest_bucketed'] == res[1]['digest_bucketed'], 'replicas must stay bit-identical (eager)'
    assert res[0]['digest_graph'] == res[1]['digest_graph'], 'replicas must stay bit-identical (graph replays)'


def test_bench_contract_with_two_ranks_sharing_this_gpu():
    """PLAIN `python bench.py --gpus 2` (the driver's command form, no launcher): bench.py starts the two ranks itself (both
    on device 0 here, gloo): ONE JSON line from rank 0, n_gpus = rccl_ranks = 2, whole-job value = global batch * steps /
    max-over-ranks time; the timed steps are graph replays (two per step around the all-reduce), as on one rank."""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY='0', VQCPC_DP_SHARE_GPU='1', VQCPC_DP_BACKEND='gloo',
               PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    for k in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT'):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '2', '--steps', '4', '--warmup', '2', '--batch', '32', '--full']
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1, lines
    line = json.loads(lines[0])
    assert line['n_gpus'] == 2 and line['scaling'] == 'weak' and line['cpu_baseline'] is None
    assert line['rccl_ranks'] == 2 and line['allreduce']['rccl_ranks'] == 2 and line['allreduce']['ms_per_step'] > 0
    assert line['allreduce']['bucket_bytes'] == 4 * line['config']['params']
    assert line['step_graph'] is not None and line['step_graph']['replays_in_run'] >= 8 and line['step_graph']['graphs_per_step'] == 2
    assert line['config']['global_batch'] == 64 and line['config']['parallelism'] == 'dp2'
    assert abs(line['value'] - 64 * 4 / (line['ms_per_step'] * 4e-3)) < 0.01 * line['value']
    assert line['roofline'] is not None and line['roofline']['achieved'] > 0
    # round 5: what makes the first real multi-GPU run self-explaining -- every rank's own time, and a single-rank leg of the same
    # command on rank 0's GPU in the same job (here: the same GPU both ranks share), from which the same-node efficiency follows
    pr = line['per_rank']
    assert len(pr['ms_per_step']) == 2 and 0 < pr['ms_per_step_min'] <= pr['ms_per_step_max'] <= line['ms_per_step'] * 1.001
    n1 = line['n1_same_node']
    assert n1 and n1.get('value', 0) > 0 and n1['steps'] == 4, n1
    ss = line['scaling_same_node']
    assert abs(ss['efficiency'] - line['value'] / (2 * n1['value'])) < 1e-3
    assert abs(ss['exposed_ms_per_step'] - (line['ms_per_step'] - n1['ms_per_step'])) < 2e-3


def test_bench_refuses_a_rank_count_that_differs_from_gpus():
    """A launcher that starts 1 rank for `--gpus 2` must not produce a (mislabelled) line."""
    env = dict(os.environ, RANK='0', WORLD_SIZE='1', LOCAL_RANK='0', MASTER_ADDR='127.0.0.1', MASTER_PORT=str(_free_port()))
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '2', '--steps', '2', '--warmup', '1'],
                       capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode != 0 and 'WORLD_SIZE=1' in r.stderr
    assert not [l for l in r.stdout.splitlines() if l.startswith('{')]


@pytest.mark.skipif(_world() != 1, reason='the refusal for too few GPUs is only observable on a 1-GPU box')
def test_bench_refuses_more_gpus_than_the_node_has():
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'VQCPC_DP_SHARE_GPU')}
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '2', '--steps', '2', '--warmup', '1'],
                       capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode != 0 and 'needs 2 visible GPUs' in r.stderr


@pytest.mark.skipif(_world() != 1, reason='needs a 1-GPU box: two ranks must land on the same physical GPU')
def test_bench_refuses_ranks_that_share_a_gpu_without_the_harness_flag():
    """Two ranks whose visible device is the same physical GPU (a launcher masking visibility, or a 1-GPU box) are not a
    2-GPU measurement: the PCI-id census after the process group is up makes every rank exit non-zero, no JSON line."""
    env = {k: v for k, v in os.environ.items() if k != 'VQCPC_DP_SHARE_GPU'}
    env.update(HSA_ENABLE_IPC_MODE_LEGACY='0', VQCPC_DP_BACKEND='gloo', PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node=2', '--master-addr', '127.0.0.1',
           '--master-port', str(_free_port()), os.path.join(ROOT, 'bench.py'), '--gpus', '2', '--steps', '2', '--warmup', '1',
           '--batch', '16']
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode != 0 and 'distinct GPUs' in r.stderr, r.stderr[-2000:]
    assert not [l for l in r.stdout.splitlines() if l.startswith('{')]
