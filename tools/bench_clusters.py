"""The cluster census (`clusters.cluster_census`, csrc/clusters.hip) on a synthetic corpus of about the Bach set's size with the C1
encoder, its parts timed separately, against a host loop that restates the reference's grouping (profiles/cluster_census_perf_log.md).

THE CORPUS.  `--pieces` 4096 pieces of 32 .. 96 beats (uniform, 64 on average: ~262 k one-beat blocks, ~223 k of them in the train
split), vocab 56 per voice, a voice holds its note with probability 0.6 per tick, as tools/bench_duplicates.py draws it.
THE ENCODER.  configs C1 (d_model 256, 2 + 2 layers, 2 codebooks of 512 words of 16 dimensions: the merged code has 2^18 values), random
weights; its codebooks are set to the latents of 512 blocks of the corpus, so that the codes in use are many, as after training.
Per part, in one process, device-synchronised host clocks, one warm-up, medians of `--reps` >= 5 runs over the WHOLE train split in
chunks of `--chunk` blocks (the same chunks everywhere):
  census_ms         one `cluster_census` call (E = 50): gather, encode, count, count merged, select, the copy back and the host statistics;
  encode_ms         gather + `encode_indices` of every chunk alone (the codes are kept on the device for the parts below);
  count_ms          vqcpc_cluster_count on the (n, 2) codes of every chunk (LDS form, 2 x 512 words);
  count_merged_ms   `merge_codes` + vqcpc_cluster_count with K = 2^18 (global-atomic form);
  select_ms         vqcpc_cluster_select (E = 50) of every chunk into freshly emptied slots;
  knn_ms            vqcpc_codebook_knn of the two codebooks, k = 3 (show_nn_clusters);
  host_loop_ms      the reference's grouping (VQCPCB/encoder.py:147-171) restated on the same codes of codebook 0, already on the host:
                    `.item()` per block, dict of lists, random.shuffle and a cap of 50 per code (the reference needs one codebook).
`kernels_share_of_census` = (count + count_merged + select) / census.

    python tools/bench_clusters.py [--reps 5] [--json profiles/cluster_census_bench.json]
    python tools/bench_clusters.py --pieces 64 --config C0 --chunk 512        # a rehearsal
"""
import argparse
import json
import os
import random
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VOCAB = 56


def _median_ms(fn, reps):
    fn()                                               # warm-up
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out), min(out), max(out)


def _music(rng, ticks):
    notes = rng.randint(1, VOCAB - 3, size=(ticks, 4))
    return np.where(rng.random_sample((ticks, 4)) < 0.6, 0, notes).astype(np.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--config', default='C1')
    ap.add_argument('--pieces', type=int, default=4096)
    ap.add_argument('--chunk', type=int, default=4096)
    ap.add_argument('--examples', type=int, default=50)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--json', default=None)
    args = ap.parse_args()
    assert args.reps >= 5, 'medians of at least 5 runs'
    assert torch.cuda.is_available(), 'bench_clusters needs the GPU'
    from vqcpc_bach_amd import clusters, configs, getters, hip
    from vqcpc_bach_amd.dataloaders.corpus import Corpus, CorpusCPCDataloaderGenerator, split_bounds
    hip.load()
    hip.use_training_default_gemm_mode()               # the arithmetic a trained encoder ran in
    torch.manual_seed(0)
    rng = np.random.RandomState(0)
    pieces = [_music(rng, 4 * int(b)) for b in rng.randint(32, 97, size=args.pieces)]
    piece_start = np.concatenate([[0], np.cumsum([len(p) for p in pieces])])
    v = [VOCAB] * 4
    corpus = Corpus(np.concatenate(pieces).astype(np.int16), piece_start, 4, v, [VOCAB - 3] * 4, [VOCAB - 2] * 4, [VOCAB - 1] * 4)
    config = configs.make_config(args.config)
    gen = CorpusCPCDataloaderGenerator(corpus, **dict(config['dataloader_generator_kwargs'], device='cuda', seed=1))
    dc = gen.device_corpus
    enc = getters.get_encoder('/tmp/vqcpc_bench_clusters', gen, config).to('cuda')
    q = enc.quantizer
    ncb, K, E, chunk = int(q.num_codebooks), int(q.codebook_size), args.examples, args.chunk
    n_all = dc.table(1)[1]
    lo, hi = split_bounds(n_all)['train']
    n = hi - lo
    ids = torch.arange(0, n_all, max(1, n_all // K), dtype=torch.int64, device='cuda')[:K]
    x = torch.empty(K, 4, 4, dtype=torch.int64, device='cuda')
    dc.gather(ids, 1, x)
    z = enc.encode_latents(x).reshape(K, ncb, -1)
    with torch.no_grad():
        for c, p in enumerate(q.embeddings):
            p.copy_(z[:, c])
    q.initialize = False
    enc.eval()
    head = {'config': args.config, 'pieces': args.pieces, 'blocks': n_all, 'train_blocks': n, 'chunk': chunk, 'examples': E,
            'num_codebooks': ncb, 'codebook_size': K, 'merged_codes': K ** ncb, 'gemm_mode': hip.get_gemm_mode(), 'reps': args.reps}
    print(json.dumps(head), flush=True)
    res = dict(head)

    census = clusters.cluster_census(enc, dc, split='train', examples=E, chunk=chunk)
    res.update(used=census.used.tolist(), perplexity=[round(float(p), 2) for p in census.perplexity], joint_used=census.joint_used,
               joint_perplexity=round(census.joint_perplexity, 2), max_count=int(census.counts.max()))
    res['census_ms'] = _median_ms(lambda: clusters.cluster_census(enc, dc, split='train', examples=E, chunk=chunk), args.reps)

    chunks = []

    def encode():
        chunks.clear()
        for s in range(0, n, chunk):
            m = min(chunk, n - s)
            i = torch.arange(lo + s, lo + s + m, dtype=torch.int64, device='cuda')
            xb = torch.empty(m, 4, 4, dtype=torch.int64, device='cuda')
            dc.gather(i, 1, xb)
            chunks.append((s, enc.encode_indices(xb).reshape(m, ncb)))
    res['encode_ms'] = _median_ms(encode, args.reps)
    counts = torch.zeros(ncb, K, dtype=torch.int32, device='cuda')
    joint = torch.zeros(1, K ** ncb, dtype=torch.int32, device='cuda')
    slots = torch.empty(ncb, K, E, dtype=torch.int64, device='cuda')
    flag = torch.zeros(1, dtype=torch.int32, device='cuda')
    key = clusters.census_key(0, 'train')

    def count():
        counts.zero_()
        for _, codes in chunks:
            clusters.count_codes(codes, K, counts, flag)

    def count_merged():
        joint.zero_()
        for _, codes in chunks:
            clusters.count_codes(enc.merge_codes(codes).reshape(-1, 1), K ** ncb, joint, flag)

    def select():
        slots.fill_(-1)
        for s, codes in chunks:
            clusters.select_examples(codes, K, key, slots, flag, id0=s)
    res['count_ms'] = _median_ms(count, args.reps)
    res['count_merged_ms'] = _median_ms(count_merged, args.reps)
    res['select_ms'] = _median_ms(select, args.reps)
    assert int(flag.item()) == 0
    assert np.array_equal(counts.cpu().numpy(), census.counts), 'the parts count what the census counted'
    books = torch.stack([e.detach() for e in q.embeddings], dim=0)
    res['knn_ms'] = _median_ms(lambda: clusters.codebook_knn(books, 3), args.reps)

    host_codes = torch.cat([codes[:, 0] for _, codes in chunks]).cpu()
    t0 = time.perf_counter()
    d = {}
    for block, code in enumerate(host_codes):          # encoder.py:147-156: one .item() per block, dict of lists
        k = code.item()
        if k not in d:
            d[k] = []
        d[k].append(block)
    for k, members in d.items():                       # :165-171
        random.shuffle(members)
        d[k] = members[:50]
    res['host_loop_ms'] = (time.perf_counter() - t0) * 1e3
    assert sorted(d) == [int(k) for k in np.nonzero(census.counts[0])[0]]

    med = {k: res[k][0] for k in ('census_ms', 'encode_ms', 'count_ms', 'count_merged_ms', 'select_ms', 'knn_ms')}
    kernels = med['count_ms'] + med['count_merged_ms'] + med['select_ms']
    res.update(kernels_ms=kernels, kernels_share_of_census=kernels / med['census_ms'], kernels_over_encode=kernels / med['encode_ms'],
               host_loop_over_kernels=res['host_loop_ms'] / kernels,
               blocks_per_s_census=n / (med['census_ms'] * 1e-3))
    for k in list(med):
        res[k] = dict(median=res[k][0], min=res[k][1], max=res[k][2])
    print(json.dumps({k: val for k, val in res.items() if k not in head}), flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, 'w') as fh:
            json.dump(res, fh, indent=1)
            fh.write('\n')


if __name__ == '__main__':
    main()
