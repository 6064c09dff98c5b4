"""Dead-code restarts under data parallelism: two ranks on this GPU over gloo (the harness of tests/test_vq_ema_multigpu_gpu.py),
tests/multigpu_vq_restart_worker.py on each.  The two processes are started directly, each under its own time limit."""
import os
import socket
import subprocess
import sys

import pytest
import torch

from conftest import ROOT

pytestmark = pytest.mark.gpu
WORKER = os.path.join(ROOT, 'tests', 'multigpu_vq_restart_worker.py')
LIMIT = 300          # seconds per process


def _free_port():
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        return s.getsockname()[1]


def test_two_ranks_restart_the_same_codes_from_the_same_rows(tmp_path):
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
    res = [torch.load(tmp_path / f'r{k}.pt') for k in range(2)]
    for k, x in enumerate(res):
        assert x['world'] == 2 and x['rank'] == k
        assert x['rows_equal'], 'the summed candidates are the rows the reference names among BOTH ranks\' rows'
        assert x['revived'], 'every restarted codeword of step 1 is its named row, with m = e and N = 1'
        assert x['others_alive'] and x['owners'] == [0, 1], x['owners']
        half, quarter = x['K'] // 2, x['K'] // 4
        want = [half, half + quarter, half + quarter] + [half + (2 + i) * quarter for i in range(4)]
        assert x['counts'] == [[c] * x['ncb'] for c in want], x['counts']
        assert x['stages'] == 2 and x['replays'] == 2, (x['stages'], x['replays'])
    a, b = res
    assert a['eager_digest'] == b['eager_digest'], 'EMA buffers bit-identical after three steps with restarts'
    assert a['param_digest'] == b['param_digest']
    assert a['graph_digest'] == b['graph_digest'], 'bit-identical through the two-graph replays'
