"""Decoder generation at DEC shape (d_model 512, 8 heads, 3 + 3 layers, T = 384 target tokens, S = 24 codes): tokens/s and
us per step of the KV-cached incremental decoder (one captured step replayed T times, and eager steps), against the
reference's method on this package (one full `Decoder.forward` per generated token, timed over a few tokens and
extrapolated to T).  Device-synchronised host clocks around whole generations.

    python tools/bench_generate.py [--batches 1,8,32] [--reforward-tokens 16] [--json out.json]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def _timed(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', default='1,8,32')
    ap.add_argument('--reforward-tokens', type=int, default=16)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--json', default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_generate needs the GPU'
    from oracle import decoder_oracle as D
    from test_decoder_gpu import seeded_decoder
    from vqcpc_bach_amd.decoders.generation import IncrementalDecoder
    from vqcpc_bach_amd.utils import STEP_LOCK
    dec, _ = seeded_decoder(D.make_cfg('DEC', B=8), 5)
    dec.eval()
    T, nc = dec.num_tokens_target, dec.num_channels
    rows = []
    for B in [int(b) for b in args.batches.split(',')]:
        g = torch.Generator().manual_seed(B)
        codes = torch.randint(0, dec.source_embeddings.weight.shape[0], (B, dec.num_tokens_source), generator=g).cuda()
        res = {'batch': B, 'T': T}
        for use_graph in (True, False):
            dec.generate_from_codes(codes, seed=1, use_graph=use_graph)                 # warm-up (capture, first launches)
            total = _timed(lambda: dec.generate_from_codes(codes, seed=1, use_graph=use_graph), args.reps)
            # the steps alone: prefill + capture outside the clock
            with STEP_LOCK, torch.no_grad():
                inc = IncrementalDecoder(dec, B)
                inc.prefill(codes)
                inc.start(seeds=1)
                if use_graph:
                    inc.step()
                    graph = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(graph, capture_error_mode='thread_local'):
                        inc.step()
                    inc.reset()
                    steps = _timed(lambda: [graph.replay() for _ in range(T)], 1) / T
                    del graph
                else:
                    steps = _timed(lambda: [inc.step() for _ in range(T)], 1) / T
            key = 'replayed' if use_graph else 'eager'
            res[f'{key}_us_per_step'] = steps * 1e6
            res[f'{key}_generation_ms'] = total * 1e3
            res[f'{key}_tokens_per_s'] = B * T / total
        # the reference's method: one full forward per token (the logits row of position t kept), host draw omitted
        x = torch.zeros(B, T // nc, nc, dtype=torch.int64, device='cuda')
        with torch.no_grad():
            dec.forward(codes, x)
            n = args.reforward_tokens
            per_token = _timed(lambda: dec.forward(codes, x)['weights_per_category'][0][:, 0].cpu(), n)
        res['reforward_ms_per_token'] = per_token * 1e3
        res['reforward_generation_ms_extrapolated'] = per_token * T * 1e3
        res['reforward_tokens_per_s'] = B / per_token
        res['speedup_replayed_vs_reforward'] = res['reforward_generation_ms_extrapolated'] / res['replayed_generation_ms']
        rows.append(res)
        print(json.dumps({k: (round(v, 3) if isinstance(v, float) else v) for k, v in res.items()}), flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, 'w') as f:
            json.dump(rows, f, indent=1)


if __name__ == '__main__':
    main()
