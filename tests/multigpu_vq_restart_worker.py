"""One rank of tests/test_vq_restart_multigpu_gpu.py: an EMA-codebook trainer with dead-code restarts under data parallelism.

Every rank builds the model from a DIFFERENT seed (rank 0's broadcast makes them equal), kills half of the codes (the same on
every rank) and trains three steps on its shard of a global batch; before the second step other codes are killed.  The restarted
codewords of step 1 are compared with the rows of BOTH ranks' quantiser inputs that tests/vq_restart_reference.py names.  Two
warm-up steps and two replays of the two-graph step follow.  What was observed goes to <out_dir>/r<rank>.pt."""
import hashlib
import os
import sys

os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')

import numpy as np  # noqa: E402
import torch  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import vq_restart_reference as Rr  # noqa: E402

SEED, THR = 0xA5A5A5A55A5A5A5A, 0.5


def digest(tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def build(model_dir, seed, dp):
    from vqcpc_bach_amd import configs, getters
    torch.manual_seed(seed)
    config = configs.make_config('C0', dropout=0.0, quantizer_type='ema', ema_restart_threshold=THR, ema_restart_seed=SEED)
    config['quantizer_kwargs'].update(num_codebooks=2, initialize=False)
    dlg = getters.get_dataloader_generator('bach', 'vqcpc', dict(config['dataloader_generator_kwargs'], device='cuda'))
    enc = getters.get_encoder(model_dir, dlg, config)
    tr = getters.get_encoder_trainer(model_dir, dlg, 'vqcpc', enc, config['auxiliary_networks_kwargs'])
    tr.to('cuda')
    tr.init_optimizers(lr=1e-3, schedule_lr=False, dp=dp)
    return tr, dlg


def kill(q, start, stride):
    """Codes start, start + stride, ..: far away from any data, with the cluster size of a code long without a row."""
    with torch.no_grad():
        q.embeddings[:, start::stride] += 1000.0
        q.ema_sum[:, start::stride] = q.embeddings[:, start::stride]
        q.ema_cluster_size[:, start::stride] = 0.1


def main():
    out_dir = sys.argv[1]
    from vqcpc_bach_amd import hip
    from vqcpc_bach_amd.parallel import DataParallelContext
    hip.load()
    hip.set_gemm_mode(1)
    dp = DataParallelContext()
    rank, world = dp.rank, dp.world_size
    per_rank = 4
    tr, dlg = build(os.path.join(out_dir, f'm{rank}'), 100 + rank, dp)
    q = tr.encoder.quantizer
    assert tr.dp.world_size == world and q.restarting
    ncb, K, dsub = q.embeddings.shape

    gen = torch.Generator().manual_seed(77)
    full = [dlg.batch(per_rank * world, gen) for _ in range(7)]
    lo, hi = rank * per_rank, (rank + 1) * per_rank
    shard = lambda b: {k: v[lo:hi].contiguous() for k, v in b.items()}

    tr.train()
    kill(q, 1, 2)
    rec = {}
    h = q.register_forward_hook(lambda mod, args, out: rec.update(z=args[0].detach().reshape(-1, mod.codebook_dim).clone()))
    tr.train_step(shard(full[0]), train=True)
    torch.cuda.synchronize()
    h.remove()
    e, N, m = (t.detach().cpu().numpy() for t in q.ema_buffers())
    rows_dev = q.restart_rows.detach().cpu().numpy()
    counts = [q.restarts.tolist()]
    zs = [torch.empty_like(rec['z']) for _ in range(world)]
    torch.distributed.all_gather(zs, rec['z'])
    per = Rr.candidates([z.cpu().numpy() for z in zs], SEED, 1, ncb, K)              # step 1 = Adam's t of the first step
    owner = Rr.rows(SEED, 1, ncb, K, world * rec['z'].shape[0]) // rec['z'].shape[0]
    want = per[0] + per[1]
    dead = np.zeros((ncb, K), dtype=bool)
    dead[:, 1::2] = True
    rows_equal = bool(np.array_equal(rows_dev, want))                 # the all-reduced candidates: the named row on every rank
    revived = bool(np.array_equal(e[dead], want[dead]) and np.array_equal(m[dead], want[dead]) and (N[dead] == 1.0).all())
    others_alive = bool((N[~dead] >= THR).all())
    owners = sorted(set(owner[dead].tolist()))                        # rows of BOTH ranks were drawn

    kill(q, 0, 4)
    tr.train_step(shard(full[1]), train=True)
    counts.append(q.restarts.tolist())
    tr.train_step(shard(full[2]), train=True)
    counts.append(q.restarts.tolist())
    torch.cuda.synchronize()
    eager_digest = digest(q.ema_buffers())
    param_digest = digest([tr.flat.flat])

    # the two-graph step: compute | all-reduce of gradients, statistics and candidates | Adam + EMA update + restart
    tr.enable_step_graph(True)
    for i, b in enumerate(full[3:7]):
        kill(q, i % 4, 4)
        tr.train_step(shard(b), train=True)
        counts.append(q.restarts.tolist())
    torch.cuda.synchronize()
    g = tr._graph
    replays, stages = (g.replays, len(g.stages)) if g is not None else (0, 0)
    graph_digest = digest(q.ema_buffers() + [tr.flat.flat])
    tr.enable_step_graph(False)

    torch.save(dict(rank=rank, world=world, rows_equal=rows_equal, revived=revived, others_alive=others_alive, owners=owners,
                    counts=counts, eager_digest=eager_digest, param_digest=param_digest, graph_digest=graph_digest,
                    replays=replays, stages=stages, K=K, ncb=ncb),
               os.path.join(out_dir, f'r{rank}.pt'))
    dp.barrier()
    dp.shutdown()


if __name__ == '__main__':
    main()
