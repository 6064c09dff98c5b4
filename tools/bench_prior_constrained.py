"""What given codes and code scores cost at the prior (vqcpc_prior_sample_constrained against vqcpc_prior_sample), at the PRI
shape (tools/bench_prior.py: d_model 512, 8 heads, 6 layers, ff 1024, N = 24 codes per window, V = 32), per batch B, in ONE
process with the two arms in ALTERNATING timing windows (plain, constrained, plain, ...), so that drift of the box hits both,
and for the step and the move on the SAME buffers (one stack, the arm is the sampler it launches):
  step         us of the replayed cached step in the head regime, plain sampler against the constrained one with half of the
               columns forced and logp on;
  move         us of the stride-1 move in the forward form (window kernel + stack + head row + sampler, eager, as it runs),
               the same two arms;
  score        ms of `score_codes` on 96 codes against the same scores from one `forward` per window + log_softmax;
Once: `continue_tokens` end to end (an opening of 24 codes of tokens, 72 new codes; DEC-shape decoder) and the share of the
prior's part (`generate_codes` with the same constraint) in it.
Per arm the median of `--reps` >= 5 windows and their spread (min .. max) are reported; a difference inside the spread is no
difference.  Device-synchronised host clocks, warm-up first.

    python tools/bench_prior_constrained.py [--batches 1,8,32] [--reps 7] [--json profiles/generate_prior_constrained_perf_log.json]
"""
import argparse
import json
import os
import statistics
import sys
import time
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))


def _window_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def alternating(arms, reps):
    """arms: {name: fn}.  One warm-up of each, then `reps` rounds of one window per arm in turn -> {name: (median, min, max)} ms."""
    for fn in arms.values():
        fn()
    samples = {k: [] for k in arms}
    for _ in range(reps):
        for k, fn in arms.items():
            samples[k].append(_window_ms(fn))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in samples.items()}


def _per(stats, n, scale=1e3):
    return {k: dict(median=m / n * scale, min=lo / n * scale, max=hi / n * scale) for k, (m, lo, hi) in stats.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', default='1,8,32')
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--json', default=None)
    args = ap.parse_args()
    assert args.reps >= 5, 'medians of at least 5 windows'
    assert torch.cuda.is_available(), 'bench_prior_constrained needs the GPU'
    from bench_prior import build_prior_and_decoder
    from vqcpc_bach_amd.priors.generation import IncrementalPrior
    from vqcpc_bach_amd.utils import STEP_LOCK
    prior, dec = build_prior_and_decoder()
    prior.eval()
    dec.eval()
    N, V, nt = prior.num_tokens, prior.num_tokens_per_channel[0], 96
    out = {'shape': dict(d_model=prior.d_model, layers=len(prior.transformer.layers), N=N, V=V, num_tokens=nt), 'rows': []}
    for B in [int(b) for b in args.batches.split(',')]:
        g = torch.Generator().manual_seed(B)
        codes = torch.randint(0, V, (B, nt), generator=g)
        half = torch.where(torch.rand(B, nt, generator=g) < 0.5, codes, torch.full_like(codes, -1))
        res = {'batch': B}
        with STEP_LOCK, torch.no_grad():
            # ONE stack: both arms run on the same buffers (the placement of the K / V caches moves a step by more than the
            # sampler costs), the arm is the sampler `_sample` launches; each arm has its own captured step
            inc = IncrementalPrior(prior, B)
            inc.start(nt, seeds=1, constraint=half, want_logp=True)
            inc.seq.copy_(codes.cuda())
            arms = {'plain': False, 'constrained': True}
            graphs = {}
            for k, flag in arms.items():
                inc.constrained = flag
                inc.pos.zero_()
                inc.step()
                torch.cuda.synchronize()
                graphs[k] = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graphs[k], capture_error_mode='thread_local'):
                    inc.step()
            R = 8                                      # passes over the window per timing window: 192 steps, tens of ms

            def head(k):
                def fn():
                    for _ in range(R):
                        inc.pos.zero_()
                        for _ in range(N):
                            graphs[k].replay()
                return fn
            res['step_replayed_us'] = _per(alternating({k: head(k) for k in arms}, args.reps), R * N)
            moves = 64

            def move(k):
                def fn():
                    inc.constrained = arms[k]
                    for i in range(moves):
                        inc.win[0:1].fill_(1 + i % 8)
                        inc._move_forward()
                return fn
            res['move_forward_stride1_us'] = _per(alternating({k: move(k) for k in arms}, args.reps), moves)
            del graphs, inc
        dcodes = codes.cuda()

        def per_window():
            with torch.no_grad():
                cols = [torch.log_softmax(prior.forward(dcodes[:, :N])['weights_per_category'][0], dim=-1)
                        .gather(2, dcodes[:, :N].unsqueeze(2)).squeeze(2)]
                for e in range(N, nt):
                    w = dcodes[:, e - N + 1:e + 1]
                    lg = prior.forward(w)['weights_per_category'][0][:, N - 1]
                    cols.append(torch.log_softmax(lg, dim=-1).gather(1, w[:, N - 1:]))
                return torch.cat(cols, dim=1)
        stats = alternating({'score_codes': lambda: prior.score_codes(dcodes), 'forward_per_window': per_window}, args.reps)
        res['score_96_codes_ms'] = _per(stats, 1, scale=1.0)
        res['score_max_abs_difference'] = float((prior.score_codes(dcodes) - per_window()).abs().max())
        gens = alternating({'plain': lambda: prior.generate_codes(nt, num_generated_codes=B, seed=1),
                            'constrained': lambda: prior.generate_codes(nt, num_generated_codes=B, seed=1, constraint=half,
                                                                        return_logp=True)}, args.reps)
        res['generation_96_codes_ms'] = _per(gens, 1, scale=1.0)
        for key in ('step_replayed_us', 'move_forward_stride1_us', 'generation_96_codes_ms'):
            res[key]['added'] = res[key]['constrained']['median'] - res[key]['plain']['median']
        out['rows'].append(res)
        print(json.dumps(res), flush=True)

    # continue_tokens end to end: an opening of 24 codes of tokens, 72 new codes
    vocab = [int(v) for v in dec.num_tokens_per_channel]
    dec.dataloader_generator = types.SimpleNamespace(dataset=types.SimpleNamespace(
        note2index_dicts=[{'START': v - 3, 'END': v - 2, 'XX': v - 1} for v in vocab]))
    g = torch.Generator().manual_seed(4)
    x = torch.cat([torch.randint(0, v - 3, (1, 24 * dec.num_events_per_code, 1), generator=g) for v in vocab], dim=2)
    codes, tokens = prior.continue_tokens(x, 72, dec, seed=1)
    L = codes.shape[1] - 72
    cons = torch.full((1, codes.shape[1]), -1, dtype=torch.int64)
    cons[:, :L] = codes[:, :L].cpu()
    stats = alternating({'continue_tokens': lambda: prior.continue_tokens(x, 72, dec, seed=1),
                         'prior_part': lambda: prior.generate_codes(codes.shape[1], seed=1, constraint=cons)}, args.reps)
    e2e = _per(stats, 1, scale=1.0)
    out['continue_tokens'] = dict(opening_codes=24, framed_given_codes=L, new_codes=72, tokens=int(tokens.shape[1] * tokens.shape[2]),
                                  ms=e2e, prior_share=e2e['prior_part']['median'] / e2e['continue_tokens']['median'])
    print(json.dumps(out['continue_tokens']), flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
