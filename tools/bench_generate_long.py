"""Long-form generation at DEC shape (d_model 512, 8 heads, 3 + 3 layers, T = 384, S = 24, U = 16), nb = 4 S = 96 codes:
per batch, in one run,
  f         ms of one full `Decoder.forward` on a window -- the reference's cost per generated token on this package;
  s         us per replayed fixed-window step;
  slide     ms of one slide (window kernel + memory + cross k | v + re-prefill of P = (S // 2) U rows), eager and replayed,
            and of the full-T fallback (the training path's decoder stack over all T rows, vqcpc_relattn_x_fwd, no heads);
  the whole generation's tokens/s, its speedup over one forward per token and the bound U f / (f + U s).
Device-synchronised host clocks, warm-up first, medians of `--reps` >= 5 runs.

    python tools/bench_generate_long.py [--batches 1,8,32] [--reps 5] [--json profiles/generate_long_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def _median_ms(fn, reps, inner=1):
    fn()                                               # warm-up
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(inner):
            fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) / inner * 1e3)
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', default='1,8,32')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--json', default=None)
    args = ap.parse_args()
    assert args.reps >= 5, 'medians of at least 5 runs'
    assert torch.cuda.is_available(), 'bench_generate_long needs the GPU'
    from oracle import decoder_oracle as D
    from test_decoder_gpu import seeded_decoder
    from vqcpc_bach_amd import ops
    from vqcpc_bach_amd.decoders.generation import IncrementalDecoder
    from vqcpc_bach_amd.transformer.transformer_custom import mask_code
    from vqcpc_bach_amd.utils import STEP_LOCK
    dec, _ = seeded_decoder(D.make_cfg('DEC', B=8), 5)
    dec.eval()
    T, S, U, nc = dec.num_tokens_target, dec.num_tokens_source, dec.total_upscaling, dec.num_channels
    nb = 4 * S
    vocab = [int(v) for v in dec.num_tokens_per_channel]
    pad, start = [v - 1 for v in vocab], [v - 3 for v in vocab]
    rows = []
    for B in [int(b) for b in args.batches.split(',')]:
        g = torch.Generator().manual_seed(B)
        codes = torch.randint(0, dec.source_embeddings.weight.shape[0], (B, nb), generator=g).cuda()
        x = torch.cat([torch.randint(0, v, (B, T // nc, 1), generator=g) for v in vocab], dim=2).cuda()
        res = {'batch': B, 'nb': nb, 'tokens': nb * U}
        with STEP_LOCK, torch.no_grad():
            res['forward_ms'] = f = _median_ms(lambda: dec.forward(codes[:, :S], x), args.reps, inner=4)
            src = ops.EmbeddingFn.apply(dec.source_embeddings.weight, codes[:, :S].reshape(-1))
            tgt = dec._target_rows(x)
            res['slide_fallback_full_T_ms'] = _median_ms(lambda: dec.transformer.forward_rows(
                src, tgt, B, mask_code(dec.encoder_attention_type), ops.MASK_CAUSAL, mask_code(dec.cross_attention_type)),
                args.reps, inner=4)
            inc = IncrementalDecoder(dec, B)
            chorale = dec.init_generation_chorale(nb * U // nc, 0, pad=pad, start=start).reshape(1, -1).expand(B, -1)
            inc.start_long(codes, chorale, seeds=1, temperature=1.0)
            inc.slide(0, S // 2)
            res['slide_eager_ms'] = _median_ms(lambda: inc.slide(5, S // 2), args.reps, inner=4)
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, capture_error_mode='thread_local'):
                inc.slide(None, S // 2, advance=0)
            res['slide_replayed_ms'] = _median_ms(graph.replay, args.reps, inner=4)
            del graph
            inc.step()
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, capture_error_mode='thread_local'):
                inc.step()

            def steps():
                inc.pos.zero_()
                for _ in range(T):
                    graph.replay()
            res['step_us'] = s_us = _median_ms(steps, args.reps) * 1e3 / T
            del graph, inc
        for key, kw in (('replayed', dict(use_graph=True)), ('eager', dict(use_graph=False))):
            gen = _median_ms(lambda: dec.generate_from_code_long(codes, temperature=1.0, seed=1, pad=pad, start=start, **kw),
                             args.reps)
            res[f'{key}_generation_ms'] = gen
            res[f'{key}_tokens_per_s'] = B * nb * U / (gen * 1e-3)
        res['slide_over_forward'] = min(res['slide_eager_ms'], res['slide_replayed_ms']) / f
        res['reforward_generation_ms'] = nb * U * f
        res['speedup_vs_reforward'] = res['reforward_generation_ms'] / res['replayed_generation_ms']
        res['speedup_bound'] = U * f / (f + U * s_us * 1e-3)
        rows.append(res)
        print(json.dumps({k: (round(v, 3) if isinstance(v, float) else v) for k, v in res.items()}), flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, 'w') as fh:
            json.dump(rows, fh, indent=1)


if __name__ == '__main__':
    main()
