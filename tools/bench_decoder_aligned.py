"""The aligned ('diagonal') decoder against the attention decoder at the DEC shape (profiles/decoder_aligned_perf_log.md).

    python tools/bench_decoder_aligned.py                    # training step + generation step, alternating windows
    python tools/bench_decoder_aligned.py --skip-generation  # the training step only

Both decoders ('transformer_relative_diagonal' and 'transformer_relative') are built in ONE process from
configs.make_decoder_config(decoder_type=...) (384 target tokens, 24 codes, d_model 512, 8 heads, 3 + 3 layers, dropout 0.2,
batch 32) on the same frozen encoder configuration, under what train_model() selects (`use_training_defaults()`: bf16x6 GEMMs,
f16x3 gradient products, step-graph replay).

Training: after the warm-up (eager steps, the graph capture, a few replays) the timed windows alternate between the two
trainers; a window is `--steps` replayed steps between two device synchronisations.
Generation: per batch size B in --gen-batches, one IncrementalDecoder per decoder, its step captured once; a window is one
whole sequence (T replays) between two device synchronisations, reported as microseconds per step; windows alternate too.
Printed: every window, and per decoder the median, minimum and maximum over the windows -- the spread is the run-to-run noise a
difference has to exceed.  One JSON line at the end.
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

TYPES = ('transformer_relative_diagonal', 'transformer_relative')


def build(decoder_type, batch):
    from vqcpc_bach_amd import configs, getters
    torch.manual_seed(0)
    config = configs.make_decoder_config(decoder_type=decoder_type)
    dlg = getters.get_dataloader_generator(config['dataset'], config['training_method'],
                                           dict(config['dataloader_generator_kwargs'], seed=1234, device='cuda'))
    enc_cfg = config['config_encoder']
    enc_dlg = getters.get_dataloader_generator(enc_cfg['dataset'], enc_cfg['training_method'],
                                               dict(enc_cfg['dataloader_generator_kwargs'], seed=1234, device='cuda'))
    encoder = getters.get_encoder(f'/tmp/vqcpc_bench_{decoder_type}', enc_dlg, enc_cfg)
    dp = getters.get_data_processor(dlg, config['data_processor_type'], config['data_processor_kwargs'])
    dec = getters.get_decoder(f'/tmp/vqcpc_bench_{decoder_type}', dlg, dp, encoder, decoder_type, config['decoder_kwargs'])
    dec.to('cuda')
    dec.use_training_defaults()
    dec.init_optimizers(lr=config['lr'], schedule_lr=config['schedule_lr'])
    dec.train()
    return dec, dlg.dataloaders(batch_size=batch or config['batch_size'])[0]


def train_window(dec, loader, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        dec.train_step(next(loader), train=True)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


class GenRun:
    """One captured generation step of `dec` at batch B; window() replays one whole sequence."""

    def __init__(self, dec, B):
        from vqcpc_bach_amd.decoders.generation import IncrementalDecoder
        g = torch.Generator().manual_seed(B)
        codes = torch.randint(0, dec.source_embeddings.weight.shape[0], (B, dec.num_tokens_source), generator=g).cuda()
        self.inc = inc = IncrementalDecoder(dec, B)
        with torch.no_grad():
            inc.prefill(codes)
            inc.start(seeds=1, temperature=1.0)
            inc.step()
            torch.cuda.synchronize()
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph, capture_error_mode='thread_local'):
                inc.step()

    def window(self):
        self.inc.reset()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(self.inc.T):
            self.graph.replay()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6 / self.inc.T


def stats(t):
    return dict(median=statistics.median(t), min=min(t), max=max(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=0)
    ap.add_argument('--steps', type=int, default=40)
    ap.add_argument('--windows', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=8)
    ap.add_argument('--gen-batches', default='1,8,32')
    ap.add_argument('--skip-generation', action='store_true')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'this measurement needs the GPU'
    from vqcpc_bach_amd import hip
    hip.load()
    runs = {t: build(t, args.batch) for t in TYPES}
    for dec, loader in runs.values():
        for _ in range(args.warmup):
            dec.train_step(next(loader), train=True)
    line = dict(steps=args.steps, windows=args.windows, device=torch.cuda.get_device_name(0),
                graph_replay={t: bool(d._graph is not None and d._graph.replays > 0) for t, (d, _) in runs.items()},
                params={t: int(d.flat.numel) for t, (d, _) in runs.items()}, train_ms_per_step={}, gen_us_per_step={})
    times = {t: [] for t in runs}
    for w in range(args.windows):
        for t, (dec, loader) in runs.items():
            ms = train_window(dec, loader, args.steps)
            times[t].append(ms)
            print(f'train window {w} {t:30s} {ms:8.3f} ms/step', flush=True)
    for t, v in times.items():
        line['train_ms_per_step'][t] = s = stats(v)
        print(f'train {t:30s} median {s["median"]:.3f}  min {s["min"]:.3f}  max {s["max"]:.3f} ms/step over {len(v)} windows')
    line['train_diagonal_over_attention'] = line['train_ms_per_step'][TYPES[0]]['median'] / line['train_ms_per_step'][TYPES[1]]['median']
    for dec, _ in runs.values():
        dec.enable_step_graph(False)
        dec.eval()
    if not args.skip_generation:
        for B in (int(b) for b in args.gen_batches.split(',')):
            gens = {t: GenRun(dec, B) for t, (dec, _) in runs.items()}
            for g in gens.values():
                g.window()                                           # warm-up
            times = {t: [] for t in gens}
            for w in range(args.windows):
                for t, g in gens.items():
                    times[t].append(g.window())
            line['gen_us_per_step'][B] = {t: stats(v) for t, v in times.items()}
            for t, v in times.items():
                s = stats(v)
                print(f'generation B={B:2d} {t:30s} median {s["median"]:.1f}  min {s["min"]:.1f}  max {s["max"]:.1f} us/step '
                      f'over {len(v)} windows of {gens[t].inc.T} steps')
            line.setdefault('gen_diagonal_over_attention', {})[B] = (line['gen_us_per_step'][B][TYPES[0]]['median']
                                                                    / line['gen_us_per_step'][B][TYPES[1]]['median'])
            del gens
    print(json.dumps(line))


if __name__ == '__main__':
    main()
