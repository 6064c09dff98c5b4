"""The diagonal decoder on continuous latents against the diagonal decoder on codes at the DEC shape
(profiles/decoder_continuous_perf_log.md).

    python tools/bench_decoder_continuous.py

Both decoders are 'transformer_relative_diagonal' from configs.make_decoder_config (384 target tokens, 24 codes, d_model 512,
8 heads, 3 + 3 layers, dropout 0.2, batch 32), built in ONE process: 'codes' on the configuration's own frozen encoder (1 x 32
codes), 'continuous' on the same encoder with quantizer_type None, codebook_dim 32 and no upscaler (dz = 32).  Everything after
the source rows is the same code, so the two are expected to agree within the run-to-run noise; there is no pass bar.

Measured, windows alternating between the two decoders, a window between two device synchronisations:
  train      --steps replayed training steps (use_training_defaults(): bf16x6 GEMMs, f16x3 gradient products, step graph)
  step       one whole sequence of captured generation steps (T replays), per B in --gen-batches, microseconds per step
  slide      --slides replays of ONE captured long-form window move (window kernel, source rows, memory, C per layer, prefix
             re-prefill at P = (S // 2) * U), per B, microseconds per slide
  source     the first launch of a slide alone: vqcpc_decode_source_rows (continuous) against the embedding gather (codes),
             --launches launches in one captured graph, microseconds per launch; and its share of the slide
Printed: per quantity the median, minimum and maximum over the windows.  One JSON line at the end.
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

KINDS = ('continuous', 'codes')
DECODER_TYPE = 'transformer_relative_diagonal'


def build(kind, batch):
    from vqcpc_bach_amd import configs, getters
    torch.manual_seed(0)
    config = configs.make_decoder_config(decoder_type=DECODER_TYPE)
    enc_cfg = config['config_encoder']
    if kind == 'continuous':
        enc_cfg.update(quantizer_type=None, quantizer_kwargs=dict(codebook_dim=32), upscaler_type=None)
    dlg = getters.get_dataloader_generator(config['dataset'], config['training_method'],
                                           dict(config['dataloader_generator_kwargs'], seed=1234, device='cuda'))
    enc_dlg = getters.get_dataloader_generator(enc_cfg['dataset'], enc_cfg['training_method'],
                                               dict(enc_cfg['dataloader_generator_kwargs'], seed=1234, device='cuda'))
    encoder = getters.get_encoder(f'/tmp/vqcpc_bench_{kind}', enc_dlg, enc_cfg)
    dp = getters.get_data_processor(dlg, config['data_processor_type'], config['data_processor_kwargs'])
    dec = getters.get_decoder(f'/tmp/vqcpc_bench_{kind}', dlg, dp, encoder, DECODER_TYPE, config['decoder_kwargs'])
    dec.to('cuda')
    assert dec.continuous_source == (kind == 'continuous')
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


def source_of(dec, B, nb, seed):
    g = torch.Generator().manual_seed(seed)
    if dec.continuous_source:
        return torch.randn(B, nb, dec.source_dim, generator=g).cuda()
    return torch.randint(0, dec.source_embeddings.weight.shape[0], (B, nb), generator=g).cuda()


def capture(fn):
    fn()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode='thread_local'):
        fn()
    return graph


def replay_window(graph, n, before=None):
    if before is not None:
        before()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        graph.replay()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / n


class GenRun:
    """Captured step, captured slide and the isolated source launch of `dec` at batch B."""

    def __init__(self, dec, B, launches):
        from vqcpc_bach_amd import hip, ops
        from vqcpc_bach_amd.decoders.generation import IncrementalDecoder
        S, U = dec.num_tokens_source, dec.total_upscaling
        nb = S + 8
        self.inc = inc = IncrementalDecoder(dec, B)
        self.long = long = IncrementalDecoder(dec, B)
        with torch.no_grad():
            inc.prefill(source_of(dec, B, S, B))
            inc.start(seeds=1, temperature=1.0)
            self.step = capture(inc.step)
            chorale = torch.zeros(B, nb * U, dtype=torch.int64, device='cuda')
            long.start_long(source_of(dec, B, nb, B + 100), chorale, seeds=1, temperature=1.0)
            long.slide(4, S // 2)
            self.slide = capture(lambda: long.slide(None, S // 2, advance=0))     # the window index stays: every replay is the same move
            d = dec.d_model
            if dec.continuous_source:
                lin = dec.source_embeddings

                def source():
                    for _ in range(launches):
                        hip.call('vqcpc_decode_source_rows', long.z_full, long.z_nb, long.dz, long.win, lin.weight, lin.bias,
                                 long.src, d, B, S, d)
            else:
                def source():
                    for _ in range(launches):
                        ops.EmbeddingFn.apply(dec.source_embeddings.weight, long.codes_win.reshape(-1))
            self.source = capture(source)
        self.launches = launches


def stats(t):
    return dict(median=statistics.median(t), min=min(t), max=max(t))


def show(what, kind, s, unit):
    print(f'{what:22s} {kind:11s} median {s["median"]:9.2f}  min {s["min"]:9.2f}  max {s["max"]:9.2f} {unit}', flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=0)
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--windows', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=8)
    ap.add_argument('--slides', type=int, default=20)
    ap.add_argument('--launches', type=int, default=50)
    ap.add_argument('--gen-batches', default='1,8,32')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'this measurement needs the GPU'
    from vqcpc_bach_amd import hip
    hip.load()
    runs = {k: build(k, args.batch) for k in KINDS}
    for dec, loader in runs.values():
        for _ in range(args.warmup):
            dec.train_step(next(loader), train=True)
    line = dict(steps=args.steps, windows=args.windows, slides=args.slides, launches=args.launches,
                device=torch.cuda.get_device_name(0),
                graph_replay={k: bool(d._graph is not None and d._graph.replays > 0) for k, (d, _) in runs.items()},
                params={k: int(d.flat.numel) for k, (d, _) in runs.items()}, train_ms_per_step={}, gen_us_per_step={},
                slide_us={}, source_us_per_launch={}, source_share_of_slide={})
    times = {k: [] for k in runs}
    for _ in range(args.windows):
        for k, (dec, loader) in runs.items():
            times[k].append(train_window(dec, loader, args.steps))
    for k, v in times.items():
        line['train_ms_per_step'][k] = s = stats(v)
        show('train B=32', k, s, 'ms/step')
    for dec, _ in runs.values():
        dec.enable_step_graph(False)
        dec.eval()
    for B in (int(b) for b in args.gen_batches.split(',')):
        gens = {k: GenRun(dec, B, args.launches) for k, (dec, _) in runs.items()}
        res = {q: {k: [] for k in gens} for q in ('step', 'slide', 'source')}
        for w in range(args.windows + 1):                                # window 0 is the warm-up
            for k, g in gens.items():
                t = dict(step=replay_window(g.step, g.inc.T, before=g.inc.reset), slide=replay_window(g.slide, args.slides),
                         source=replay_window(g.source, 10) / g.launches)
                if w:
                    for q, v in t.items():
                        res[q][k].append(v)
        for q, key, unit in (('step', 'gen_us_per_step', 'us/step'), ('slide', 'slide_us', 'us/slide'),
                             ('source', 'source_us_per_launch', 'us/launch')):
            line[key][B] = {k: stats(v) for k, v in res[q].items()}
            for k in gens:
                show(f'{q} B={B}', k, line[key][B][k], unit)
        line['source_share_of_slide'][B] = {k: line['source_us_per_launch'][B][k]['median'] / line['slide_us'][B][k]['median']
                                            for k in gens}
        print(f'source / slide B={B}: ' + ', '.join(f'{k} {v:.4f}' for k, v in line['source_share_of_slide'][B].items()), flush=True)
        del gens
    print(json.dumps(line))


if __name__ == '__main__':
    main()
