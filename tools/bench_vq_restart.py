"""Dead-code restarts of the EMA codebooks at the flagship step (profiles/vq_restart_perf_log.md).

    python tools/bench_vq_restart.py                    # step time of 'ema' without / with ema_restart_threshold=0.5 (+ a control)
    python tools/bench_vq_restart.py --codewords 300    # + num_codewords, codebook_perplexity, restarts over 300 synthetic steps
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/bench_vq_restart.py --windows 1 --steps 20 --kernels-only

The trainers ('ema', 'ema+restart' and the control 'ema+launches': RUNS below) are built in ONE process from
configs.make_config('C1', quantizer_type='ema') (dropout 0.1, batch 256) under what train_model() selects
(`use_training_defaults()`: bf16x6 GEMMs, f16x3 gradient products, step-graph replay).  After the warm-up (eager steps, the graph
capture, a few replays) the timed windows alternate between the trainers; a window is `--steps` replayed steps between two device
synchronisations.  Printed: every window's ms / step, and per trainer the median, minimum and maximum over the windows -- the
spread is the run-to-run noise a difference has to exceed.  The two entry points are also timed alone at the configuration's shapes: `--calls` back-to-back launches between two device
events (a CALL time: it includes the launch gap; the kernel time is rocprofv3's, with --kernels-only, by the kernel names
vq_restart_candidates_kernel and vq_ema_restart_kernel).  vqcpc_vq_ema_update is timed the same way as the yardstick.

Written: <--out>.md and <--out>.json.  The codeword figures are for information: synthetic tokens say nothing about music.
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

THRESHOLD = 0.5
# 'ema+launches': the two launches in every step under a threshold no cluster size ever falls below, so that nothing restarts and
# the codebooks evolve exactly as 'ema' does: separates the cost of the launches from what a fuller codebook does to the step
RUNS = {'ema': None, 'ema+launches': 1e-30, 'ema+restart': THRESHOLD}


def build(threshold, name, batch):
    from vqcpc_bach_amd import configs, getters
    torch.manual_seed(0)
    extra = dict(ema_restart_threshold=threshold) if threshold else {}
    config = configs.make_config(name, quantizer_type='ema', **extra)
    dlg = getters.get_dataloader_generator('bach', 'vqcpc', dict(config['dataloader_generator_kwargs'], device='cuda'))
    tag = f'/tmp/vqcpc_bench_vq_restart_{threshold}'
    enc = getters.get_encoder(tag, dlg, config)
    tr = getters.get_encoder_trainer(tag, dlg, 'vqcpc', enc, config['auxiliary_networks_kwargs'])
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


def call_times(q, rows, calls):
    """us per call of the two new entry points and of vqcpc_vq_ema_update at the quantiser's shapes, on copies of its state."""
    from vqcpc_bach_amd import hip
    ncb, K, dsub = q.embeddings.shape
    z = torch.randn(rows, ncb * dsub, device='cuda')
    cand = torch.empty(ncb, K, dsub, device='cuda')
    e, N, m = (t.clone() for t in q.ema_buffers())
    stats = torch.zeros(ncb, K, dsub + 1, device='cuda')
    restarts = torch.zeros(ncb, dtype=torch.int32, device='cuda')
    step_dev = torch.ones(1, dtype=torch.int64, device='cuda')
    jobs = {
        'vq_restart_candidates': lambda: hip.call('vqcpc_vq_restart_candidates', z, rows, ncb, K, dsub, 0, 1, step_dev, 0, 1, cand),
        # the threshold of a real step: whether a lane copies a row depends on N, so the state is the trainer's own
        'vq_ema_restart': lambda: hip.call('vqcpc_vq_ema_restart', cand, N, m, e, ncb, K, dsub, THRESHOLD, restarts),
        'vq_ema_update': lambda: hip.call('vqcpc_vq_ema_update', stats, N, m, e, ncb, K, dsub, 0.99, 0.01, 1e-5),
        'fill_only': lambda: N.fill_(0.0),
        'vq_ema_restart_all_dead': lambda: (N.fill_(0.0), hip.call('vqcpc_vq_ema_restart', cand, N, m, e, ncb, K, dsub, THRESHOLD,
                                                                     restarts)),
    }
    out = {}
    for name, fn in jobs.items():
        for _ in range(20):
            fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        torch.cuda.synchronize()
        out[name] = a.elapsed_time(b) * 1e3 / calls
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--config', default='C1')
    ap.add_argument('--batch', type=int, default=0)
    ap.add_argument('--steps', type=int, default=40)
    ap.add_argument('--windows', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=8)
    ap.add_argument('--calls', type=int, default=500)
    ap.add_argument('--codewords', type=int, default=0, help='also: codebook usage over this many steps, per trainer')
    ap.add_argument('--kernels-only', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'vq_restart_perf_log'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'this measurement needs the GPU'
    from vqcpc_bach_amd import hip
    hip.load()
    runs = {name: build(thr, args.config, args.batch) for name, thr in RUNS.items()}
    rows = {}
    for name, (tr, loader) in runs.items():
        q = tr.encoder.quantizer
        h = q.register_forward_hook(lambda mod, a, out, name=name: rows.__setitem__(name, a[0].numel() // mod.codebook_dim))
        for _ in range(args.warmup):
            tr.train_step(next(loader), train=True)
        h.remove()
    replayed = {name: bool(tr._graph is not None and tr._graph.replays > 0) for name, (tr, _) in runs.items()}
    times = {name: [] for name in runs}
    for w in range(args.windows):
        for name, (tr, loader) in runs.items():
            ms = window(tr, loader, args.steps)
            times[name].append(ms)
            print(f'window {w} {name:12s} {ms:8.3f} ms/step', flush=True)
    q = runs['ema+restart'][0].encoder.quantizer
    line = dict(config=args.config, steps=args.steps, windows=args.windows, graph_replay=replayed, threshold=THRESHOLD,
                quantizer_rows=rows['ema+restart'], codebooks=list(q.embeddings.shape))
    md = ['# Dead-code restarts of the EMA codebooks: measurements', '',
          f'`tools/bench_vq_restart.py`, configuration {args.config} ({q.embeddings.shape[0]} x {q.embeddings.shape[1]} codes of '
          f'{q.embeddings.shape[2]} floats, {rows["ema+restart"]} quantiser rows per step), `ema_restart_threshold = {THRESHOLD}`, '
          f'replayed steps: {replayed}.', '']
    if not args.kernels_only:
        md += [f'## Step time, {args.windows} alternating windows of {args.steps} replayed steps', '',
               '| trainer | median ms/step | min | max |', '|---|---|---|---|']
        for name, t in times.items():
            line[name] = dict(median_ms=statistics.median(t), min_ms=min(t), max_ms=max(t), windows_ms=t)
            print(f'{name:12s} median {line[name]["median_ms"]:.3f}  min {min(t):.3f}  max {max(t):.3f} ms/step over {len(t)} windows')
            md.append(f'| {name} | {line[name]["median_ms"]:.3f} | {min(t):.3f} | {max(t):.3f} |')
        line['restart_over_ema'] = line['ema+restart']['median_ms'] / line['ema']['median_ms']
        line['launches_over_ema'] = line['ema+launches']['median_ms'] / line['ema']['median_ms']
        md += ['', f'Ratios of the medians to `ema`: {line["launches_over_ema"]:.4f} (`ema+launches`: the two launches under a '
               f'threshold of 1e-30, nothing ever restarts), {line["restart_over_ema"]:.4f} (`ema+restart`).  The spread of one '
               'trainer\'s windows is the noise.', '']
        line['call_us'] = call_times(q, rows['ema+restart'], args.calls)
        md += [f'## The entry points alone: us per call, {args.calls} back-to-back calls between two device events', '',
               '| entry point | us / call |', '|---|---|']
        for name, us in line['call_us'].items():
            print(f'{name:28s} {us:8.2f} us/call')
            md.append(f'| {name} | {us:.2f} |')
        md += ['', '`vq_ema_restart` runs on the trainer\'s state after its steps (the state a step meets); `_all_dead` puts a fill in '
               'front of every call so that each of them copies every row (`fill_only` is that fill alone).  A call time in a '
               'back-to-back loop includes the launch gap; the yardstick is `vq_ema_update` in the same loop.', '']
    if args.codewords:
        md += [f'## Codebook usage over {args.codewords} synthetic steps (for information)', '',
               '| trainer | num_codewords | negatives | codebook_perplexity | codebook_restarts |', '|---|---|---|---|---|']
        for name, (tr, loader) in runs.items():
            m = tr.epoch(loader, train=True, num_batches=args.codewords, corrupt_labels=False)
            ppl = m.get('codebook_perplexity', [float(v) for v in tr.encoder.quantizer.codebook_perplexity().tolist()])
            line.setdefault('usage', {})[name] = dict(num_codewords=m['num_codewords'], negative=m['num_codewords_negative'],
                                                      loss_quantize=m['loss_quantize'], codebook_perplexity=ppl,
                                                      codebook_restarts=m.get('codebook_restarts'))
            print(f'{name:12s} num_codewords {m["num_codewords"]:.1f} (negatives {m["num_codewords_negative"]:.1f}) perplexity '
                  f'{[round(v, 1) for v in ppl]} restarts {m.get("codebook_restarts")} over {args.codewords} steps')
            md.append(f'| {name} | {m["num_codewords"]:.1f} | {m["num_codewords_negative"]:.1f} | '
                      f'{", ".join(f"{v:.1f}" for v in ppl)} | {m.get("codebook_restarts", "-")} |')
        md.append('')
    for tr, _ in runs.values():
        tr.enable_step_graph(False)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out + '.json', 'w') as f:
        json.dump(line, f, indent=1)
        f.write('\n')
    with open(args.out + '.md', 'w') as f:
        f.write('\n'.join(md))
    print(json.dumps(line))


if __name__ == '__main__':
    main()
