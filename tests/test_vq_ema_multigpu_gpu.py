"""EMA codebooks under data parallelism: two ranks on this GPU over gloo (the harness of tests/test_multigpu_gpu.py; everything
but the transport is the multi-GPU path), tests/multigpu_vq_ema_worker.py on each.  The two processes are started directly, each
under its own time limit."""
import os
import socket
import subprocess
import sys

import pytest
import torch

from conftest import ROOT

pytestmark = pytest.mark.gpu
WORKER = os.path.join(ROOT, 'tests', 'multigpu_vq_ema_worker.py')
LIMIT = 300          # seconds per process


def _free_port():
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        return s.getsockname()[1]


def test_two_ranks_keep_identical_ema_codebooks_and_sum_their_statistics(tmp_path):
    port = str(_free_port())
    procs = []
    for rank in range(2):
        env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY='0', VQCPC_DP_SHARE_GPU='1', VQCPC_DP_BACKEND='gloo', RANK=str(rank),
                   WORLD_SIZE='2', LOCAL_RANK=str(rank), MASTER_ADDR='127.0.0.1', MASTER_PORT=port,
                   PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
        procs.append(subprocess.Popen([sys.executable, WORKER, str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                                      text=True, env=env, cwd=ROOT))
    outs = []
    try:
        for p in procs:
            outs.append(p.communicate(timeout=LIMIT)[0])
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.communicate()
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o[-3000:]
    res = [torch.load(tmp_path / f'e{k}.pt') for k in range(2)]
    for k, x in enumerate(res):
        assert x['world'] == 2 and x['rank'] == k
        assert x['rows'] == x['rows_expected'], 'the all-reduced counts cover the rows of BOTH ranks'
        assert x['counts_equal'], 'all-reduced counts == counts of one rank given both halves of the batch'
        assert x['idx_equal'], 'row by row the ranks assign the codes the one-rank run assigns'
        print(f"rank {k}: max |z_dp - z_one_rank| {x['z_delta']:.3e}, sums excess over the bound: vs exact {x['excess_exact']:.3e}, "
              f"vs one rank {x['excess']:.3e}")
        # sums: within the summation bound of the exact sum of the rows that were summed, and of the one-rank run's sums once
        # the last-bit difference of its rows (the worker's comment) is accounted for
        assert x['excess_exact'] <= 0.0 and x['excess'] <= 0.0, (x['excess_exact'], x['excess'])
        assert x['stages'] == 2 and x['replays'] == 2, (x['stages'], x['replays'])
    a, b = res
    assert a['init_digest'] == b['init_digest'], "rank 0's parameters and EMA buffers on every rank"
    assert a['eager_digest'] == b['eager_digest'], 'EMA buffers bit-identical after three steps'
    assert a['param_digest'] == b['param_digest']
    assert a['graph_digest'] == b['graph_digest'], 'EMA buffers bit-identical through the two-graph replays'
