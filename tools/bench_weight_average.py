"""What weight averaging costs at the C1 and DEC steps (profiles/weight_average_perf_log.md).

    python tools/bench_weight_average.py                       # C1 and DEC: replayed step without / with averaging, the launch alone
    python tools/bench_weight_average.py --config DEC --legs off_a,off_b      # the default step only (also runs on a tree without the feature)

Per shape the trainers are built in ONE process under what train_model() selects (`use_training_defaults()`: bf16x6 GEMMs, f16x3
gradient products, step-graph replay): two identical legs without averaging (`off_a`, `off_b`: their difference is the spread a
difference has to exceed) and one with `enable_weight_averaging(0.999)` (`on`).  After the warm-up (eager steps, the capture, a few
replays) the timed windows alternate between the legs; a window is `--steps` replayed steps between two device synchronisations.

The launch alone: `vqcpc_weight_average` (device form) next to `vqcpc_adam_step_dev` on scratch buffers of the shape's parameter
count, `--launches` back-to-back launches between two device events, windows alternating.  By bytes moved the average (12 bytes per
parameter: read p, read and write avg) should take about 12 / 28 of Adam's time (read p, g, m, v, write p, m, v).  Back to back, a
buffer set that fits the 256 MiB last-level cache is served from there: the ratio of the two is the figure, not the GB/s.

One JSON line at the end.
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

DECAY = 0.999


def build(name, batch, tag):
    from vqcpc_bach_amd import configs, getters
    torch.manual_seed(0)
    config = configs.make_config(name)
    model_dir = f'/tmp/vqcpc_bench_weight_average_{name}_{tag}'
    if name == 'DEC':
        enc_cfg = config['config_encoder']
        dlg = getters.get_dataloader_generator(config['dataset'], config['training_method'],
                                               dict(config['dataloader_generator_kwargs'], device='cuda'))
        enc_dlg = getters.get_dataloader_generator(enc_cfg['dataset'], enc_cfg['training_method'],
                                                   dict(enc_cfg['dataloader_generator_kwargs'], device='cuda'))
        encoder = getters.get_encoder(model_dir, enc_dlg, enc_cfg)
        dp = getters.get_data_processor(dlg, config['data_processor_type'], config['data_processor_kwargs'])
        tr = getters.get_decoder(model_dir, dlg, dp, encoder, config['decoder_type'], config['decoder_kwargs'])
        tr.cuda()
    else:
        dlg = getters.get_dataloader_generator('bach', 'vqcpc', dict(config['dataloader_generator_kwargs'], device='cuda'))
        enc = getters.get_encoder(model_dir, dlg, config)
        tr = getters.get_encoder_trainer(model_dir, dlg, 'vqcpc', enc, config['auxiliary_networks_kwargs'])
        tr.to('cuda')
    tr.use_training_defaults()
    tr.init_optimizers(lr=config['lr'], schedule_lr=config['schedule_lr'])
    if tag == 'on':
        tr.enable_weight_averaging(DECAY)
    tr.train()
    return tr, dlg.dataloaders(batch_size=batch or config['batch_size'])[0]


def window(tr, loader, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        tr.train_step(next(loader), train=True)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def stats(t):
    return dict(median_ms=statistics.median(t), min_ms=min(t), max_ms=max(t))


def steps_of(name, args, legs):
    runs = {leg: build(name, args.batch, leg) for leg in legs}
    for tr, loader in runs.values():
        for _ in range(args.warmup):
            tr.train_step(next(loader), train=True)
    times = {leg: [] for leg in runs}
    for w in range(args.windows):
        for leg, (tr, loader) in runs.items():
            ms = window(tr, loader, args.steps)
            times[leg].append(ms)
            print(f'{name} window {w} {leg:6s} {ms:8.3f} ms/step', flush=True)
    out = dict(params=int(next(iter(runs.values()))[0].flat.numel),
               graph_replay={leg: bool(tr._graph is not None and tr._graph.replays > 0) for leg, (tr, _) in runs.items()})
    for leg, t in times.items():
        out[leg] = stats(t)
        print(f'{name} {leg:6s} median {out[leg]["median_ms"]:.3f}  min {min(t):.3f}  max {max(t):.3f} ms/step over {len(t)} windows')
    if 'off_a' in out and 'off_b' in out:
        out['spread_ms'] = abs(out['off_a']['median_ms'] - out['off_b']['median_ms'])
        if 'on' in out:
            out['on_minus_off_ms'] = out['on']['median_ms'] - 0.5 * (out['off_a']['median_ms'] + out['off_b']['median_ms'])
    for tr, _ in runs.values():
        tr.enable_step_graph(False)
    n = out['params']
    del runs
    torch.cuda.empty_cache()
    return out, n


def launches_of(n, args):
    """us per launch of the two kernels alone on scratch buffers of n parameters."""
    from vqcpc_bach_amd import hip
    f32 = dict(dtype=torch.float32, device='cuda')
    p, g = torch.randn(n, **f32), 1e-3 * torch.randn(n, **f32)
    m, v, avg = torch.zeros(n, **f32), torch.zeros(n, **f32), p.clone()
    lr_dev = torch.full((1,), 1e-4, **f32)
    step_dev = torch.full((1,), 100, dtype=torch.int64, device='cuda')
    sumsq = torch.ones(1, dtype=torch.float64, device='cuda')
    kernels = {
        'adam_step_dev': lambda: hip.call('vqcpc_adam_step_dev', p, g, m, v, n, lr_dev, 0.9, 0.999, 1e-8, step_dev, 1.0, 5.0, sumsq),
        'weight_average': lambda: hip.call('vqcpc_weight_average', avg, p, n, DECAY, 0, step_dev, 0),
    }
    times = {k: [] for k in kernels}
    for w in range(args.windows + 1):                        # window 0 warms up
        for k, launch in kernels.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.launches):
                launch()
            b.record()
            b.synchronize()
            if w:
                times[k].append(a.elapsed_time(b) * 1e3 / args.launches)
    out = {}
    for k, t in times.items():
        nbytes = (28 if k == 'adam_step_dev' else 12) * n
        us = statistics.median(t)
        out[k] = dict(median_us=us, min_us=min(t), max_us=max(t), bytes=nbytes, gb_per_s=nbytes / us * 1e-3)
        print(f'{k:15s} n = {n}: median {us:.2f} us  min {min(t):.2f}  max {max(t):.2f}  ({out[k]["gb_per_s"]:.0f} GB/s of {nbytes} bytes)')
    out['average_over_adam'] = out['weight_average']['median_us'] / out['adam_step_dev']['median_us']
    print(f'weight_average / adam_step_dev = {out["average_over_adam"]:.3f} (by bytes: {12 / 28:.3f})')
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--config', default='C1,DEC')
    ap.add_argument('--legs', default='off_a,off_b,on', help="'on' needs the feature; the others run on any tree")
    ap.add_argument('--batch', type=int, default=0)
    ap.add_argument('--steps', type=int, default=40)
    ap.add_argument('--windows', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=8)
    ap.add_argument('--launches', type=int, default=200)
    ap.add_argument('--skip-launch', action='store_true', help='steps only')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'this measurement needs the GPU'
    from vqcpc_bach_amd import hip
    hip.load()
    legs = args.legs.split(',')
    line = dict(steps=args.steps, windows=args.windows, legs=legs, decay=DECAY)
    for name in args.config.split(','):
        line[name], n = steps_of(name, args, legs)
        if not args.skip_launch:
            line[name]['launch'] = launches_of(n, args)
    print(json.dumps(line))


if __name__ == '__main__':
    main()
