"""The code prior at the PRI shape (configs.make_prior_config: d_model 512, 8 heads, 6 layers, ff 1024, N = 24 codes per
window, V = 32), num_tokens = 96: per batch B, in one run,
  f            ms of one full `PriorRelative.forward` on a window -- the reference's cost per generated code on this
               package (its generate loop runs one per code, priors/prior_relative.py:338);
  head         us per code in the head regime (e < N): the cached step, eager and replayed, and the forward form (eager);
  sliding      us per code in the sliding regime (e >= N): cached moves at window_stride 1 (window kernel + re-prefill of
               N - 1 rows + one step) and at --stride, eager and replayed; the forward form's move (eager, as it runs);
  generations  96 codes by the default path, the cached form alone, the forward-per-code loop actually run (eager forward form
               with the sampler: the reference's algorithm on this package) and the cached form at --stride: ms and codes/s.
Once: ms per training step at batch 32, eager and replayed from the step graph; one end-to-end `generate` (96 codes ->
1 536 tokens through `Decoder.generate_from_code_long` at the DEC shape).
The tool CHECKS the condition of the feature and exits non-zero when it fails: at every batch, the form the default path
uses in each regime costs no more per code than the forward-per-code loop's step there (forward + head row + sampler; where
the default uses that very form the two are one measurement), and the default generation is not slower than the loop run.
The default's cost relative to the bare f (no head row, no sampler) is reported next to it.
Device-synchronised host clocks, warm-up first, medians of `--reps` >= 5 samples of >= 64 codes each.

    python tools/bench_prior.py [--batches 1,8,32] [--reps 5] [--json profiles/generate_prior_bench.json]
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


def build_prior_and_decoder():
    """PRI prior on the decoder fixture builder's DEC model (its frozen encoder is the prior's)."""
    from oracle import decoder_oracle as D
    from test_decoder_gpu import seeded_decoder
    from vqcpc_bach_amd import configs
    from vqcpc_bach_amd.priors.prior_relative import PriorRelative
    dec, _ = seeded_decoder(D.make_cfg('DEC', B=8), 5)
    k = configs.make_prior_config()['prior_kwargs']
    torch.manual_seed(6)
    prior = PriorRelative('/tmp/vqcpc_bench_prior', None, dec.encoder, d_model=k['d_model'], num_layers=k['num_layers'],
                          n_head=k['n_head'], dim_feedforward=k['dim_feedforward'], embedding_size=k['embedding_size'],
                          num_channels=1, num_events=dec.num_tokens_source, dropout=k['dropout']).cuda()
    return prior, dec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', default='1,8,32')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--stride', type=int, default=4)
    ap.add_argument('--json', default=None)
    args = ap.parse_args()
    assert args.reps >= 5, 'medians of at least 5 runs'
    assert torch.cuda.is_available(), 'bench_prior needs the GPU'
    from vqcpc_bach_amd import hip
    from vqcpc_bach_amd.priors.generation import IncrementalPrior
    from vqcpc_bach_amd.utils import STEP_LOCK
    prior, dec = build_prior_and_decoder()
    prior.eval()
    dec.eval()
    N, V, nt, ks = prior.num_tokens, prior.num_tokens_per_channel[0], 96, args.stride
    out = {'shape': dict(d_model=prior.d_model, layers=len(prior.transformer.layers), N=N, V=V, num_tokens=nt), 'rows': []}
    for B in [int(b) for b in args.batches.split(',')]:
        g = torch.Generator().manual_seed(B)
        codes = torch.randint(0, V, (B, nt), generator=g).cuda()
        res = {'batch': B}
        with STEP_LOCK, torch.no_grad():
            res['forward_ms'] = f = _median_ms(lambda: prior.compute_loss(codes[:, :N]), args.reps, inner=32)
            inc = IncrementalPrior(prior, B)
            inc.start(nt, seeds=1)
            inc.seq.copy_(codes)
            R = 8                                      # passes over the window per timed sample: >= 192 codes, tens of ms

            def head_cached_eager():
                for _ in range(R):
                    inc.pos.zero_()
                    for _ in range(N):
                        inc.step()
            res['head_cached_eager_us_per_code'] = _median_ms(head_cached_eager, args.reps) * 1e3 / (R * N)
            torch.cuda.synchronize()
            step_graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(step_graph, capture_error_mode='thread_local'):
                inc.step()

            def head_cached_replayed():
                for _ in range(R):
                    inc.pos.zero_()
                    for _ in range(N):
                        step_graph.replay()
            res['head_cached_replayed_us_per_code'] = _median_ms(head_cached_replayed, args.reps) * 1e3 / (R * N)

            def head_forward():
                for _ in range(R):
                    inc.pos.zero_()
                    for p in range(N):
                        inc.step_forward(p)
            res['head_forward_us_per_code'] = _median_ms(head_forward, args.reps) * 1e3 / (R * N)
            moves = 64
            for k in (1, ks):
                def slide_eager():
                    for i in range(moves):
                        inc.slide(1 + i % 8, N - k, advance=k)
                        for _ in range(k):
                            inc.step()
                res[f'sliding_stride{k}_cached_eager_us_per_code'] = _median_ms(slide_eager, args.reps) * 1e3 / (moves * k)
                inc.slide(1, N - k, advance=0)
                torch.cuda.synchronize()
                slide_graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(slide_graph, capture_error_mode='thread_local'):
                    inc.slide(None, N - k, advance=0)

                def slide_replayed():
                    for i in range(moves):
                        slide_graph.replay()
                        for _ in range(k):
                            step_graph.replay()
                res[f'sliding_stride{k}_cached_replayed_us_per_code'] = _median_ms(slide_replayed, args.reps) * 1e3 / (moves * k)
                del slide_graph

            def move_forward_eager():
                for i in range(moves):
                    inc.win[0:1].fill_(1 + i % 8)
                    inc._move_forward()
            res['sliding_forward_eager_us_per_code'] = _median_ms(move_forward_eager, args.reps) * 1e3 / moves
            head_form, slide_form = inc._forms('auto', 1)
            del step_graph, inc
        runs = [('default', dict()), ('cached', dict(method='cached')), (f'cached_stride{ks}', dict(window_stride=ks))]
        default_is_loop = (head_form, slide_form) == ('forward', 'forward')
        if not default_is_loop:                        # otherwise the default generation IS that loop: one measurement
            runs.append(('forward_per_code_loop', dict(method='forward', use_graph=False)))
        for key, kw in runs:
            gen = _median_ms(lambda: prior.generate_codes(nt, num_generated_codes=B, seed=1, **kw), args.reps)
            res[f'{key}_generation_ms'] = gen
            res[f'{key}_codes_per_s'] = B * nt / (gen * 1e-3)
        if default_is_loop:
            res['forward_per_code_loop_generation_ms'] = res['default_generation_ms']
        res['default_forms'] = dict(head=head_form, sliding=slide_form, default_is_the_forward_per_code_loop=default_is_loop)
        res['bare_forward_us'] = f * 1e3
        # the forward-per-code loop, per regime: forward on the window + head row + sampler (+ window kernel when sliding)
        loop_head, loop_slide = res['head_forward_us_per_code'], res['sliding_forward_eager_us_per_code']
        head_us = loop_head if head_form == 'forward' else res['head_cached_replayed_us_per_code']
        slide_us = loop_slide if slide_form == 'forward' else res['sliding_stride1_cached_replayed_us_per_code']
        res['default_head_us_per_code'], res['default_sliding_us_per_code'] = head_us, slide_us
        res['speedup_vs_forward_per_code_loop'] = res['forward_per_code_loop_generation_ms'] / res['default_generation_ms']
        # the condition: per regime the default's form costs no more per code than the loop's step there (where the default
        # uses the loop's own form the two are one measurement), and the default generation is not slower than the loop run
        res['not_slower_than_reforward'] = dict(head=head_us <= loop_head, sliding=slide_us <= loop_slide,
                                                generation=res['default_generation_ms']
                                                <= res['forward_per_code_loop_generation_ms'])
        res['default_over_bare_forward'] = dict(head=head_us / (f * 1e3), sliding=slide_us / (f * 1e3))
        out['rows'].append(res)
        print(json.dumps({k: (round(v, 3) if isinstance(v, float) else v) for k, v in res.items()}), flush=True)

    # end to end: codes -> tokens (96 codes x 16 tokens = 1 536 tokens per row)
    vocab = [int(v) for v in dec.num_tokens_per_channel]
    kw = dict(pad=[v - 1 for v in vocab], start=[v - 3 for v in vocab])
    e2e = _median_ms(lambda: prior.generate(nt, dec, temperature=1.0, seed=1, **kw), args.reps)
    out['generate_end_to_end'] = dict(batch=1, codes=nt, tokens=nt * dec.total_upscaling, ms=e2e)
    print(json.dumps({'generate_end_to_end_ms': round(e2e, 3)}), flush=True)

    # the training step at batch 32, the arithmetic train_model() selects
    hip.set_gemm_mode(1)
    try:
        gen = torch.Generator().manual_seed(3)
        batch = {'x': torch.cat([torch.randint(0, v, (32, dec.num_tokens_target // dec.num_channels, 1), generator=gen)
                                 for v in vocab], dim=2).cuda()}
        prior.init_optimizers(lr=1e-4)
        prior.train()
        steps = {}
        for name, graph in (('eager', False), ('replayed', True)):
            prior.enable_step_graph(graph)
            for _ in range(4):
                prior.train_step(batch)
            steps[f'train_step_{name}_ms'] = _median_ms(lambda: prior.train_step(batch), args.reps, inner=5)
        prior.enable_step_graph(False)
    finally:
        hip.set_gemm_mode(0)
    out['train_step_batch32'] = steps
    print(json.dumps({k: round(v, 3) for k, v in steps.items()}), flush=True)
    failed = [(r['batch'], k) for r in out['rows'] for k, ok in r['not_slower_than_reforward'].items() if not ok]
    out['verdict'] = 'ok' if not failed else 'SLOWER than one forward per code at (batch, regime): ' + repr(failed)
    print('VERDICT: ' + out['verdict'], flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, 'w') as fh:
            json.dump(out, fh, indent=1)
    return 1 if failed else 0


if __name__ == '__main__':
    sys.exit(main())
