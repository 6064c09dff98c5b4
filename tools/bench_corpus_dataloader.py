"""The device-resident corpus sampler against the synthetic data path at the flagship shape (profiles/corpus_dataloader_perf_log.md).

    python tools/bench_corpus_dataloader.py                      # C1: B = 256, Kl = Kr = 8, N = 15, random negatives
    python tools/bench_corpus_dataloader.py --pieces 40 --transpositions 2 --batch 8 --config C0 --steps 4 --windows 2   # a rehearsal

A seeded synthetic corpus of --pieces x --transpositions pieces (40 .. 80 beats each, vocab 56) is written to a temporary file and
loaded through `getters.get_dataloader_generator('corpus', ...)`.  Measured, all in ONE process, in alternating windows (a window is
--steps items between two device synchronisations; printed per window, then median / min / max -- the spread is the noise a
difference has to exceed):

  batch    ms per batch of CorpusCPCDataloaderGenerator (3 permute + 3 gather launches, nothing crosses PCIe) against
           SyntheticCPCDataloaderGenerator.batch() (host randint + 4 host-to-device copies), the data path of every earlier
           measurement of this repository;
  step     ms per replayed training step (`use_training_defaults()`: bf16x6 GEMMs, f16x3 gradient products, step-graph replay) on ONE
           fixed batch, fed from the corpus loader, and fed from the synthetic loader; the corpus batch time as a share of the
           fixed-batch step.

An epoch of the corpus loader is finite (min over the positive and the two negative streams, as the reference's zip of its
loaders); the feeder below starts the next epoch when one ends, which includes the loader's lazy id check (one device
synchronisation per epoch).  One JSON line at the end.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

VOCAB = (56, 56, 56, 56)


def write_corpus(path, pieces, transpositions, seed):
    from vqcpc_bach_amd.dataloaders.corpus import save_corpus
    rng = np.random.RandomState(seed)
    out = []
    for _ in range(pieces):
        beats = int(rng.randint(40, 81))
        base = rng.randint(12, 40, size=(beats * 4, 4))
        out += [base + t - transpositions // 2 for t in range(transpositions)]       # a transposition shifts every token
    v = np.asarray(VOCAB)
    save_corpus(path, out, VOCAB, v - 3, v - 2, v - 1)
    return len(out), sum(p.shape[0] for p in out)


def endless(gen, batch, counter):
    while True:
        loader = gen.dataloaders(batch_size=batch)[0]
        counter['epochs'] += 1
        counter['steps_per_epoch'] = len(loader)
        yield from loader


def timed(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--config', default='C1')
    ap.add_argument('--batch', type=int, default=0)
    ap.add_argument('--pieces', type=int, default=400)
    ap.add_argument('--transpositions', type=int, default=12)
    ap.add_argument('--steps', type=int, default=40)
    ap.add_argument('--windows', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=8)
    ap.add_argument('--seed', type=int, default=1234)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'this measurement needs the GPU'
    from vqcpc_bach_amd import configs, getters, hip
    hip.load()
    torch.manual_seed(0)
    config = configs.make_config(args.config)
    B = args.batch or config['batch_size']
    kw = dict(config['dataloader_generator_kwargs'], device='cuda', seed=args.seed)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, 'corpus.npz')
        n_pieces, n_ticks = write_corpus(path, args.pieces, args.transpositions, args.seed)
        cor = getters.get_dataloader_generator('corpus', 'vqcpc', dict(kw, corpus_path=path))
    syn = getters.get_dataloader_generator('bach', 'vqcpc', dict(kw, vocab=VOCAB))
    counter = dict(epochs=0, steps_per_epoch=0)
    cor_it = endless(cor, B, counter)
    syn_gen = torch.Generator().manual_seed(args.seed)
    feeds = {'corpus': lambda: next(cor_it), 'synthetic': lambda: syn.batch(B, syn_gen)}

    enc = getters.get_encoder('/tmp/vqcpc_bench_corpus', cor, config)
    tr = getters.get_encoder_trainer('/tmp/vqcpc_bench_corpus', cor, 'vqcpc', enc, config['auxiliary_networks_kwargs'])
    tr.to('cuda')
    tr.use_training_defaults()
    tr.init_optimizers(lr=config['lr'], schedule_lr=config['schedule_lr'])
    tr.train()
    fixed = feeds['corpus']()
    for feed in feeds.values():                                      # warm-up: the loaders' kernels, eager steps, the capture, replays
        for _ in range(args.warmup):
            tr.train_step(feed(), train=True)
    replayed = bool(tr._graph is not None and tr._graph.replays > 0)

    runs = {f'batch_{k}': f for k, f in feeds.items()}
    runs['step_fixed_batch'] = lambda: tr.train_step(fixed, train=True)
    runs['step_fed_corpus'] = lambda: tr.train_step(feeds['corpus'](), train=True)
    runs['step_fed_synthetic'] = lambda: tr.train_step(feeds['synthetic'](), train=True)
    times = {k: [] for k in runs}
    for w in range(args.windows):
        for k, fn in runs.items():
            ms = timed(fn, args.steps)
            times[k].append(ms)
            print(f'window {w} {k:20s} {ms:9.4f} ms', flush=True)
    tr.enable_step_graph(False)
    cor.device_corpus.raise_if_bad_ids()
    line = dict(config=args.config, batch=B, steps=args.steps, windows=args.windows, graph_replay=replayed, pieces=n_pieces,
                corpus_ticks=n_ticks, corpus_device_bytes=int(cor.device_corpus.tokens.numel() * 4),
                steps_per_epoch=counter['steps_per_epoch'], epochs_started=counter['epochs'],
                batch_bytes=int(sum(v.numel() * 8 for v in fixed.values())))
    for k, t in times.items():
        line[k] = dict(median_ms=statistics.median(t), min_ms=min(t), max_ms=max(t))
        print(f'{k:20s} median {line[k]["median_ms"]:.4f}  min {min(t):.4f}  max {max(t):.4f} ms over {len(t)} windows')
    line['corpus_over_synthetic_batch'] = line['batch_corpus']['median_ms'] / line['batch_synthetic']['median_ms']
    line['corpus_batch_share_of_step'] = line['batch_corpus']['median_ms'] / line['step_fixed_batch']['median_ms']
    print(json.dumps(line))


if __name__ == '__main__':
    main()
