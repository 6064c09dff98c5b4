"""EMA codebooks against Adam-trained codebooks at the flagship step (profiles/vq_ema_perf_log.md).

    python tools/bench_vq_ema.py                      # step time of configs 'commitment' and 'ema', alternating windows
    python tools/bench_vq_ema.py --codewords 300      # + num_codewords over 300 synthetic steps, both quantisers
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/bench_vq_ema.py --windows 1 --steps 20 --kernels-only

Both trainers are built in ONE process from configs.make_config('C1') (dropout 0.1, batch 256) under what train_model() selects
(`use_training_defaults()`: bf16x6 GEMMs, f16x3 gradient products, step-graph replay).  After the warm-up (eager steps, the graph
capture, a few replays) the timed windows alternate between the two trainers; a window is `--steps` replayed steps between two
device synchronisations.  Printed: every window's ms / step, and per quantiser the median, minimum and maximum over the windows --
the spread is the run-to-run noise a difference has to exceed.  One JSON line at the end.

--kernels-only skips the statistics: under rocprofv3 the kernel table separates the two by name (vq_bwd_kernel against
vq_ema_stats_kernel + vq_commit_bwd_kernel + vq_ema_update_kernel; the reduce_splits launches of both are shared names).
The num_codewords figures are for information: synthetic tokens say nothing about music.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def build(qtype, name, batch):
    from vqcpc_bach_amd import configs, getters
    torch.manual_seed(0)
    config = configs.make_config(name, quantizer_type=qtype)
    dlg = getters.get_dataloader_generator('bach', 'vqcpc', dict(config['dataloader_generator_kwargs'], device='cuda'))
    enc = getters.get_encoder(f'/tmp/vqcpc_bench_vq_ema_{qtype}', dlg, config)
    tr = getters.get_encoder_trainer(f'/tmp/vqcpc_bench_vq_ema_{qtype}', dlg, 'vqcpc', enc, config['auxiliary_networks_kwargs'])
    tr.to('cuda')
    tr.use_training_defaults()
    tr.init_optimizers(lr=config['lr'], schedule_lr=config['schedule_lr'])
    tr.train()
    return tr, dlg.dataloaders(batch_size=batch or config['batch_size'])[0]


def window(tr, loader, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        tr.train_step(next(loader), train=True)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--config', default='C1')
    ap.add_argument('--batch', type=int, default=0)
    ap.add_argument('--steps', type=int, default=40)
    ap.add_argument('--windows', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=8)
    ap.add_argument('--codewords', type=int, default=0, help='also: num_codewords over this many steps, per quantiser')
    ap.add_argument('--kernels-only', action='store_true')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'this measurement needs the GPU'
    from vqcpc_bach_amd import hip
    hip.load()
    runs = {q: build(q, args.config, args.batch) for q in ('commitment', 'ema')}
    for tr, loader in runs.values():
        for _ in range(args.warmup):
            tr.train_step(next(loader), train=True)
    replayed = {q: bool(tr._graph is not None and tr._graph.replays > 0) for q, (tr, _) in runs.items()}
    times = {q: [] for q in runs}
    for w in range(args.windows):
        for q, (tr, loader) in runs.items():
            ms = window(tr, loader, args.steps)
            times[q].append(ms)
            print(f'window {w} {q:10s} {ms:8.3f} ms/step', flush=True)
    line = dict(config=args.config, steps=args.steps, windows=args.windows, graph_replay=replayed,
                params={q: int(tr.flat.numel) for q, (tr, _) in runs.items()})
    if not args.kernels_only:
        for q, t in times.items():
            line[q] = dict(median_ms=statistics.median(t), min_ms=min(t), max_ms=max(t))
            print(f'{q:10s} median {line[q]["median_ms"]:.3f}  min {min(t):.3f}  max {max(t):.3f} ms/step over {len(t)} windows')
        line['ema_over_commitment'] = line['ema']['median_ms'] / line['commitment']['median_ms']
    if args.codewords:
        for q, (tr, loader) in runs.items():
            m = tr.epoch(loader, train=True, num_batches=args.codewords, corrupt_labels=False)
            line.setdefault('num_codewords', {})[q] = dict(train=m['num_codewords'], negative=m['num_codewords_negative'],
                                                           loss_quantize=m['loss_quantize'])
            print(f'{q:10s} num_codewords {m["num_codewords"]:.1f} (negatives {m["num_codewords_negative"]:.1f}) '
                  f'over {args.codewords} steps')
    for tr, _ in runs.values():
        tr.enable_step_graph(False)
    print(json.dumps(line))


if __name__ == '__main__':
    main()
