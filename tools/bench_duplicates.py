"""The duplicate check (`DeviceCorpus.longest_common_run`, csrc/duplicates.hip) on a synthetic corpus of about the Bach set's size,
against the host loop it replaces and against the generation whose output it checks.

THE CORPUS.  The reference's chorale set is about 350 chorales in up to a dozen transpositions of some 60 beats each: of the
order of 4000 pieces and 10^6 ticks.  Here: `--pieces` 4096 pieces of 32 .. 96 beats (uniform, 64 on average: ~1.05 M ticks, ~8 MB
framed), vocab 56 per voice; a voice holds its note with probability 0.6 per tick (token 0, as the '__' symbol of the chorale
encoding does), so chance runs of held notes are common and the scan's partial-tick path is taken as often as on music.
QUERIES.  G = 1 / 8 / 32 rows of 96 and 384 ticks, drawn like the corpus, each with a 40-tick copy of a corpus stretch.
Per (G, ticks), in one process:
  check_ms           one `longest_common_run` call, host tokens in -> host dict out (pack, scan, copy back, unframe);
  kernel_ms          vqcpc_dup_longest_run alone, the keys zeroed on the device;
  comparisons_per_s  tick comparisons of the scan, G * ticks * framed ticks / kernel time;
  difflib_ms         the reference's loop, `difflib.SequenceMatcher(None, a, b, autojunk=False).find_longest_match` per piece, on the
                     first `--difflib-pieces` pieces for ONE row, EXTRAPOLATED linearly to all pieces and G rows (so labelled).
For 32 rows of 384 ticks it also times `generate_from_code_long` of the same 32 x 384 ticks at DEC shape (96 codes, replayed
steps), the generation that such a check follows.  Device-synchronised host clocks, warm-up first, medians of `--reps` >= 5 runs.

    python tools/bench_duplicates.py [--reps 5] [--json profiles/duplicate_check_bench.json]
"""
import argparse
import difflib
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

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
    return statistics.median(out)


def _music(rng, ticks):
    notes = rng.randint(1, VOCAB - 3, size=(ticks, 4))
    return np.where(rng.random_sample((ticks, 4)) < 0.6, 0, notes).astype(np.int64)


def _pairs(x):
    return [(v, int(t)) for row in x for v, t in enumerate(row)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--pieces', type=int, default=4096)
    ap.add_argument('--difflib-pieces', type=int, default=32)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--no-generation', action='store_true')
    ap.add_argument('--json', default=None)
    args = ap.parse_args()
    assert args.reps >= 5, 'medians of at least 5 runs'
    assert torch.cuda.is_available(), 'bench_duplicates needs the GPU'
    from vqcpc_bach_amd import hip
    from vqcpc_bach_amd.dataloaders.corpus import Corpus, DeviceCorpus
    rng = np.random.RandomState(0)
    pieces = [_music(rng, 4 * int(b)) for b in rng.randint(32, 97, size=args.pieces)]
    piece_start = np.concatenate([[0], np.cumsum([len(p) for p in pieces])])
    v = [VOCAB] * 4
    corpus = Corpus(np.concatenate(pieces).astype(np.int16), piece_start, 4, v, [VOCAB - 3] * 4, [VOCAB - 2] * 4, [VOCAB - 1] * 4)
    dc = DeviceCorpus(corpus, 'cuda')
    t0 = time.perf_counter()
    framed = dc.framed()
    torch.cuda.synchronize()
    head = {'pieces': args.pieces, 'ticks': int(piece_start[-1]), 'framed_ticks': int(framed.numel()),
            'frame_first_call_ms': (time.perf_counter() - t0) * 1e3}
    print(json.dumps(head), flush=True)
    rows = [head]
    for ticks in (96, 384):
        for G in (1, 8, 32):
            x = np.stack([_music(rng, ticks) for _ in range(G)])
            for g in range(G):
                src = pieces[(37 * g + ticks) % len(pieces)]
                x[g, 20:60] = src[50:90]
            xt = torch.from_numpy(x)
            res = {'G': G, 'ticks': ticks}
            out = dc.longest_common_run(xt)
            res['min_length'], res['max_length'] = int(out['length'].min()), int(out['length'].max())
            assert res['min_length'] >= 160, 'the planted 40-tick copy must be found'
            res['check_ms'] = _median_ms(lambda: dc.longest_common_run(xt), args.reps)
            query = torch.empty(G, ticks, dtype=torch.int64, device='cuda')
            xd = xt.cuda()
            hip.call('vqcpc_dup_pack', xd, xd.stride(0), xd.stride(1), ticks, G, query, ticks)
            keys = torch.zeros(G, dtype=torch.int64, device='cuda')

            def kernel():
                keys.zero_()
                hip.call('vqcpc_dup_longest_run', framed, framed.numel(), query, ticks, ticks, G, keys)
            res['kernel_ms'] = _median_ms(kernel, args.reps)
            res['comparisons_per_s'] = G * ticks * framed.numel() / (res['kernel_ms'] * 1e-3)
            a = _pairs(x[0])
            t0 = time.perf_counter()
            for p in pieces[:args.difflib_pieces]:
                b = _pairs(p)
                difflib.SequenceMatcher(None, a, b, autojunk=False).find_longest_match(0, len(a), 0, len(b))
            per_piece = (time.perf_counter() - t0) / args.difflib_pieces
            res['difflib_measured_pieces'] = args.difflib_pieces
            res['difflib_ms_extrapolated'] = per_piece * args.pieces * G * 1e3
            res['speedup_vs_difflib_extrapolated'] = res['difflib_ms_extrapolated'] / res['check_ms']
            rows.append(res)
            print(json.dumps({k: (round(val, 3) if isinstance(val, float) else val) for k, val in res.items()}), flush=True)
    if not args.no_generation:
        from oracle import decoder_oracle as D
        from test_decoder_gpu import seeded_decoder
        dec, _ = seeded_decoder(D.make_cfg('DEC', B=8), 5)
        dec.eval()
        S, U, nc = dec.num_tokens_source, dec.total_upscaling, dec.num_channels
        nb = 384 * nc // U
        assert nb >= S
        vocab = [int(n) for n in dec.num_tokens_per_channel]
        codes = torch.randint(0, dec.source_embeddings.weight.shape[0], (32, nb), generator=torch.Generator().manual_seed(1)).cuda()
        gen_ms = _median_ms(lambda: dec.generate_from_code_long(codes, temperature=1.0, seed=1, pad=[n - 1 for n in vocab],
                                                                start=[n - 3 for n in vocab]), args.reps)
        check = next(r for r in rows[1:] if (r['G'], r['ticks']) == (32, 384))
        res = {'generate_from_code_long_32x384_ms': gen_ms, 'check_32x384_ms': check['check_ms'],
               'check_over_generation': check['check_ms'] / gen_ms}
        rows.append(res)
        print(json.dumps({k: round(val, 4) for k, val in res.items()}), flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, 'w') as fh:
            json.dump(rows, fh, indent=1)
            fh.write('\n')


if __name__ == '__main__':
    main()
