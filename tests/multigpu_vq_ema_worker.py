"""One rank of tests/test_vq_ema_multigpu_gpu.py: an EMA-codebook trainer (quantizer_type 'ema') under data parallelism.

Every rank builds the model from a DIFFERENT seed (only rank 0's broadcast -- flat parameters AND the EMA buffers, which live
outside the flat buffer -- can make them equal), trains three steps on its shard of a global batch, then a one-rank twin starts
from the state before the third step and takes that step on the WHOLE batch: its counts must equal the all-reduced counts
exactly, its sums within the summation bound.  Two warm-up steps and two replays of the two-graph step follow.  What was observed
goes to <out_dir>/e<rank>.pt."""
import hashlib
import os
import sys

os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')

import torch  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import vq_ema_reference as E  # noqa: E402


def digest(tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def build(model_dir, seed, dp):
    from vqcpc_bach_amd import configs, getters
    torch.manual_seed(seed)
    config = configs.make_config('C0', dropout=0.0, quantizer_type='ema')
    config['quantizer_kwargs'].update(num_codebooks=2)
    dlg = getters.get_dataloader_generator('bach', 'vqcpc', dict(config['dataloader_generator_kwargs'], device='cuda'))
    enc = getters.get_encoder(model_dir, dlg, config)
    tr = getters.get_encoder_trainer(model_dir, dlg, 'vqcpc', enc, config['auxiliary_networks_kwargs'])
    tr.to('cuda')
    tr.init_optimizers(lr=1e-3, schedule_lr=False, dp=dp)
    return tr, dlg


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
    assert tr.dp.world_size == world and list(q.parameters()) == []
    init_digest = digest([tr.flat.flat] + q.ema_buffers())

    gen = torch.Generator().manual_seed(77)
    full = [dlg.batch(per_rank * world, gen) for _ in range(7)]
    lo, hi = rank * per_rank, (rank + 1) * per_rank
    shard = lambda b: {k: v[lo:hi].contiguous() for k, v in b.items()}

    tr.train()
    for b in full[:2]:
        tr.train_step(shard(b), train=True)
    torch.cuda.synchronize()
    state = dict(flat=tr.flat.flat.clone(), m=tr.optimizer.m.clone(), v=tr.optimizer.v.clone(), step=tr.optimizer.step_count,
                 buffers=[t.clone() for t in q.ema_buffers()])
    rec3 = {}
    h3 = q.register_forward_hook(lambda mod, args, out: rec3.update(z=args[0].detach().reshape(-1, mod.codebook_dim).clone(),
                                                                    idx=out[1].reshape(-1, mod.num_codebooks).clone()))
    tr.train_step(shard(full[2]), train=True)
    torch.cuda.synchronize()
    h3.remove()
    # every rank's quantiser input of this step, put in the row order of the one-rank pass: [negatives | left | right], ranks
    # in order inside each segment
    zs = [torch.empty_like(rec3['z']) for _ in range(world)]
    ids = [torch.empty_like(rec3['idx']) for _ in range(world)]
    torch.distributed.all_gather(zs, rec3['z'])
    torch.distributed.all_gather(ids, rec3['idx'])
    seg = [per_rank * dlg.num_negative_samples * dlg.num_blocks_right, per_rank * dlg.num_blocks_left, per_rank * dlg.num_blocks_right]
    assert sum(seg) == rec3['z'].shape[0]
    cut = lambda ts: torch.cat([t.split(seg)[i] for i in range(3) for t in ts]).cpu()
    z_dp, idx_dp = cut(zs), cut(ids)
    stats_dp = q.stats.detach().cpu().double()
    eager_digest = digest(q.ema_buffers())
    param_digest = digest([tr.flat.flat])

    # the two-graph step: compute | all-reduce of the gradient bucket and of the statistics | Adam + EMA update
    tr.enable_step_graph(True)
    for b in full[3:7]:
        tr.train_step(shard(b), train=True)
    torch.cuda.synchronize()
    g = tr._graph
    replays, stages = (g.replays, len(g.stages)) if g is not None else (0, 0)
    graph_digest = digest(q.ema_buffers())
    tr.enable_step_graph(False)

    # one rank, both halves of the batch, from the state before the third step
    env = {k: os.environ.get(k) for k in ('RANK', 'WORLD_SIZE')}
    os.environ.update(RANK='0', WORLD_SIZE='1')
    solo_dp = DataParallelContext(device=dp.device)
    os.environ.update({k: v for k, v in env.items() if v is not None})
    assert not solo_dp.distributed
    solo, _ = build(os.path.join(out_dir, f's{rank}'), 500 + rank, solo_dp)
    sq = solo.encoder.quantizer
    sq.initialize = False
    solo.flat.flat.copy_(state['flat'])
    solo.optimizer.m.copy_(state['m'])
    solo.optimizer.v.copy_(state['v'])
    solo.optimizer.step_count = state['step']
    for dst, src in zip(sq.ema_buffers(), state['buffers']):
        dst.copy_(src)
    rec = {}
    h = sq.register_forward_hook(lambda mod, args, out: rec.update(z=args[0].detach().reshape(-1, mod.codebook_dim).cpu(),
                                                                   idx=out[1].reshape(-1, mod.num_codebooks).cpu()))
    solo.train()
    solo.train_step(full[2], train=True)
    torch.cuda.synchronize()
    h.remove()
    stats_solo = sq.stats.detach().cpu().double()
    K = sq.codebook_size
    n, s, a = E.stats(rec['z'], rec['idx'], K)
    n_dp, s_dp, a_dp = E.stats(z_dp, idx_dp, K)
    idx_equal = bool(torch.equal(idx_dp, rec['idx']))
    counts_equal = bool(torch.equal(stats_dp[..., 0], stats_solo[..., 0])) and bool(torch.equal(stats_solo[..., 0], n))
    # the all-reduced sums against the exact sum of the rows the ranks summed: the summation bound (any order, the all-reduce's
    # addition included)
    excess_exact = float(((stats_dp[..., 1:] - s_dp).abs() - E.sum_bound(n_dp, a_dp)).max())
    # ... and against the one-rank run.  Its rows are NOT the ranks' rows bit for bit: the encoder's GEMMs pick their tiles by
    # the row count, so z of a block differs in the last bits between a pass of B and of 2 B windows (z_delta below).  Triangle
    # inequality per cell: |S_dp - S_solo| <= bound(dp rows) + bound(solo rows) + sum over the cell's rows of |z_dp - z_solo|
    delta = E.stats((z_dp.double() - rec['z'].double()).abs(), rec['idx'], K)[1]
    excess = float(((stats_dp[..., 1:] - stats_solo[..., 1:]).abs() - E.sum_bound(n_dp, a_dp) - E.sum_bound(n, a) - delta).max())
    z_delta = float((z_dp.double() - rec['z'].double()).abs().max())
    print(f'rank {rank}: max |z_dp - z_solo| {z_delta:.3e}; sums vs exact: excess {excess_exact:.3e}; vs one rank: {excess:.3e}')
    rows = int(stats_dp[..., 0].sum())

    torch.save(dict(rank=rank, world=world, init_digest=init_digest, eager_digest=eager_digest, param_digest=param_digest,
                    graph_digest=graph_digest, replays=replays, stages=stages, counts_equal=counts_equal, excess=excess,
                    excess_exact=excess_exact, idx_equal=idx_equal, z_delta=z_delta, rows=rows, rows_expected=int(rec['z'].shape[0]) * sq.num_codebooks),
               os.path.join(out_dir, f'e{rank}.pt'))
    dp.barrier()
    dp.shutdown()


if __name__ == '__main__':
    main()
