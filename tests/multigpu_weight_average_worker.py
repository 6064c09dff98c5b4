"""One rank of the weight-averaging data-parallel test (tests/test_weight_averaging_gpu.py): the student trainer -- three
optimisers, the step cut into graphs around its all-reduces -- runs the same six steps without and with weight averaging, every
rank on its own sequences.  Counted: the collectives of either run.  Writes <out_dir>/w<rank>.pt."""
import collections
import hashlib
import os
import sys

os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import weight_average_reference as R  # noqa: E402
from oracle import student_oracle as S  # noqa: E402

DECAY = 0.3
COLLECTIVES = ('all_reduce', 'broadcast', 'all_gather', 'reduce', 'barrier', 'reduce_scatter', 'all_to_all')


def digest(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def main():
    out_dir = sys.argv[1]
    from test_student_gpu import build_student
    from vqcpc_bach_amd import hip
    hip.load()
    hip.set_gemm_mode(1)
    cfg = S.make_cfg(ticks=16, d=64, H=4, ff=128, enc_layers=[1, 1], K=8, teacher_layers=2, dec_layers=[1, 1],
                     num_events_masked=2, B=4, vocab=[23, 19, 30, 14], emb=16)
    sd = S.init_state(cfg, seed=5)
    counts = collections.Counter()
    for name in COLLECTIVES:                    # count what the step asks of the process group
        def counted(*a, _real=getattr(dist, name), _name=name, **k):
            counts[_name] += 1
            return _real(*a, **k)
        setattr(dist, name, counted)

    results, dp = {}, None
    for averaging in (False, True):
        tr = build_student(cfg, sd, lr=1e-3)          # init_optimizers(): process group, rank-0 broadcast
        dp = dp or tr.dp                              # the first context owns the process group
        batches = [S.synthetic_batch(cfg, seed=60 + 10 * dp.rank + i) for i in range(6)]      # every rank its own sequences
        tr.train()
        tr.enable_step_graph(True)
        start = tr.flat.flat.detach().cpu().numpy().copy()
        if averaging:
            tr.enable_weight_averaging(DECAY)
        counts.clear()
        traj = []
        for b in batches:
            tr.train_step({k: v.cuda() for k, v in b.items()}, train=True, masked_event_index=3)
            traj.append(tr.flat.flat.detach().cpu().numpy().copy())
        val = None
        if averaging:
            with tr.averaged_weights():
                tr.eval()
                common = S.synthetic_batch(cfg, seed=999)                                     # the same sequences on every rank
                out = tr.train_step({k: v.cuda() for k, v in common.items()}, train=False, masked_event_index=3)
                val = float(out['loss_monitor'])
                tr.train()
        results[averaging] = dict(traj=traj, start=start, counts=dict(counts), replays=tr._graph.replays,
                                  avg=None if not averaging else tr.weight_average().detach().cpu().numpy().copy(), val=val)
        tr.enable_step_graph(False)
    on, off = results[True], results[False]
    want = R.average_f32(on['start'], on['traj'], DECAY, u0=1)
    torch.cuda.synchronize()
    torch.save(dict(rank=dp.rank, world=dp.world_size, replays=on['replays'],
                    restatement_ok=bool(np.array_equal(want.view(np.int32), on['avg'].view(np.int32))),
                    raw_equal_off=all(np.array_equal(a.view(np.int32), b.view(np.int32)) for a, b in zip(on['traj'], off['traj'])),
                    collectives_on=on['counts'], collectives_off=off['counts'],
                    avg_digest=digest(torch.from_numpy(on['avg'])), param_digest=digest(torch.from_numpy(on['traj'][-1])),
                    val_inside=on['val']),
               os.path.join(out_dir, f'w{dp.rank}.pt'))
    dp.barrier()
    dp.shutdown()


if __name__ == '__main__':
    main()
