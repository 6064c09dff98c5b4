"""`Decoder.score_tokens` against the forced generation it replaces, at the DEC shape (d_model 512, 8 heads, 3 + 3 layers, T = 384,
S = 24, U = 16), nb = 96 codes, per batch B in --batches, in ONE process with alternating legs (profiles/score_tokens_perf_log.md):

  score    ms per `score_tokens(x, codes)` call over the whole piece: nb - S + 1 = 73 windows per piece, `--window-rows` rows per forward
  forced   ms per `generate_from_code_long(codes, constraint=x, return_logp=True)` call over the same pieces: a captured step replayed
           nb * U = 1 536 times and 72 slides (the call captures its graphs itself, as every user's call does)
  Each leg runs TWICE per round as two identical legs (a, b); the legs alternate a-score, a-forced, b-score, b-forced.  The spread of
  a quantity is the larger |median(a) - median(b)| of the two forms: what a difference between the forms has to exceed.
  head     us per pass of the concatenated head over the scored rows of one chunk of `--window-rows` middle windows
           (vqcpc_decode_linear with `gather`, 64 rows per launch), timed alone between two device synchronisations
  kernel   us per vqcpc_decode_score launch on those rows with every output on, timed alone
  step     us per replayed default generation step (the captured step of a plain `IncrementalDecoder.start()`): the figure to
           compare with the same tool on the parent tree (`--step-only --root <tree>`), since this change touches no launch of it

    timeout -k 10 900 python tools/bench_score_tokens.py [--batches 1,8,32] [--rounds 5] [--window-rows 32]
                                                         [--json profiles/score_tokens_bench.json]
    timeout -k 10 300 python tools/bench_score_tokens.py --step-only [--root <another tree>]

Every invocation is one GPU step: run it under its own `timeout`, as above.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import torch


def stats(t):
    return dict(median=statistics.median(t), min=min(t), max=max(t))


def timed(fn, reps=1):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        out = fn()
    torch.cuda.synchronize()
    del out
    return (time.perf_counter() - t0) / reps


def step_us(dec, B, windows):
    """us per replayed default step: the captured plain step, T replays per window."""
    from vqcpc_bach_amd.decoders.generation import IncrementalDecoder
    from vqcpc_bach_amd.utils import STEP_LOCK
    T, S = dec.num_tokens_target, dec.num_tokens_source
    g = torch.Generator().manual_seed(B)
    codes = torch.randint(0, dec.source_embeddings.weight.shape[0], (B, S), generator=g).cuda()
    with STEP_LOCK, torch.no_grad():
        inc = IncrementalDecoder(dec, B)
        inc.prefill(codes)
        inc.start(seeds=1, temperature=1.0)
        inc.step()
        graph = inc.capture(inc.step)
        times = []
        for w in range(windows + 1):
            inc.reset()
            t = timed(graph.replay, T) * 1e6
            if w:
                times.append(t)
    return stats(times)


def launches_alone(dec, B, window_rows, reps=200):
    """The head pass and the score launch of one chunk of middle windows, each alone: (head us, kernel us, scored rows)."""
    from vqcpc_bach_amd import hip
    T, U, nc, d = dec.num_tokens_target, dec.total_upscaling, dec.num_channels, dec.d_model
    S = dec.num_tokens_source
    sizes = [int(v) for v in dec.num_tokens_per_channel]
    offs = [0]
    for v in sizes:
        offs.append(offs[-1] + v)
    offs_c = (ctypes.c_int32 * (nc + 1))(*offs)
    vtot = offs[-1]
    n = window_rows
    R = n * U
    g = torch.Generator().manual_seed(7)
    out = torch.randn(n * T, d, generator=g).cuda()
    head_w = torch.cat([m.weight for m in dec.pre_softmaxes], dim=0).contiguous()
    head_b = torch.cat([m.bias for m in dec.pre_softmaxes], dim=0).contiguous()
    gather = (torch.arange(n).repeat_interleave(U) * T + (S // 2) * U + torch.arange(U).repeat(n)).cuda()
    logits = torch.empty(R, vtot, device='cuda')
    pieces = max(1, min(B, n))
    row_b = (torch.arange(R, dtype=torch.int32) // U % pieces).cuda()
    row_col = (torch.arange(R, dtype=torch.int32) // (U * pieces) * U + torch.arange(R, dtype=torch.int32) % U).cuda()
    cols = int(row_col.max()) + 1
    chorale = torch.stack([torch.randint(0, sizes[c % nc], (pieces,), generator=g) for c in range(cols)], dim=1).cuda()
    res = [torch.empty(pieces, cols, dtype=dt, device='cuda') for dt in (torch.float32, torch.float32, torch.float32, torch.int32,
                                                                          torch.int64, torch.float32)]

    def head():
        for g0 in range(0, R, 64):
            m = min(64, R - g0)
            hip.call('vqcpc_decode_linear', out, d, gather[g0:], head_w, head_b, None, 0, logits[g0:], vtot, m, vtot, d, 0)
        return logits

    def kernel():
        hip.call('vqcpc_decode_score', logits, vtot, offs_c, nc, R, row_b, row_col, chorale, cols, None, 0, pieces, cols, cols, *res)
        return res[0]
    head(), kernel()
    return timed(head, reps) * 1e6, timed(kernel, reps) * 1e6, R


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', default='1,8,32')
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--codes', type=int, default=96)
    ap.add_argument('--window-rows', type=int, default=32)
    ap.add_argument('--json', default=None)
    ap.add_argument('--step-only', action='store_true', help='the default generation step alone (runs on a tree without score_tokens)')
    ap.add_argument('--root', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    args = ap.parse_args()
    sys.path.insert(0, args.root)
    sys.path.insert(0, os.path.join(args.root, 'tests'))
    assert torch.cuda.is_available(), 'bench_score_tokens needs the GPU'
    from oracle import decoder_oracle as D
    from test_decoder_gpu import seeded_decoder
    dec, _ = seeded_decoder(D.make_cfg('DEC', B=8), 5)
    dec.eval()
    nb, nc, epc = args.codes, dec.num_channels, dec.num_events_per_code
    vocab = [int(v) for v in dec.num_tokens_per_channel]
    pad, start = [v - 1 for v in vocab], [v - 3 for v in vocab]
    rows = []
    for B in [int(b) for b in args.batches.split(',')]:
        res = dict(batch=B, nb=nb, T=dec.num_tokens_target, U=dec.total_upscaling, rounds=args.rounds, window_rows=args.window_rows,
                   device=torch.cuda.get_device_name(0), root=os.path.abspath(args.root))
        res['step_us'] = step_us(dec, B, args.rounds)
        print(f'B={B:2d} default step {res["step_us"]["median"]:.1f} us', flush=True)
        if not args.step_only:
            g = torch.Generator().manual_seed(100 + B)
            codes = torch.randint(0, dec.source_embeddings.weight.shape[0], (B, nb), generator=g).cuda()
            x = torch.cat([torch.randint(0, v, (B, nb * epc, 1), generator=g) for v in vocab], dim=2).cuda()
            forms = dict(score=lambda: dec.score_tokens(x, codes, pad=pad, start=start, window_rows=args.window_rows),
                         forced=lambda: dec.generate_from_code_long(codes, temperature=1.0, constraint=x, return_logp=True, seed=1,
                                                                    pad=pad, start=start)[1])
            a, b = forms['score'](), forms['forced']()                          # warm-up, and the two must agree
            with torch.no_grad():
                full = dec.forward(codes[:1, :dec.num_tokens_source], x[:1, :dec.num_tokens_source * epc])['weights_per_category']
            rms = float(torch.cat([f.reshape(-1) for f in full]).pow(2).mean().sqrt())
            res['max_abs_difference_over_rms'] = float((a.double() - b.double()).abs().max()) / rms
            del a, b, full
            times = {f'{f}_{leg}': [] for leg in 'ab' for f in forms}
            for r in range(args.rounds):
                for leg in 'ab':
                    for f, fn in forms.items():
                        times[f'{f}_{leg}'].append(timed(fn) * 1e3)
                        print(f'B={B:2d} round {r} {f}_{leg:1s} {times[f"{f}_{leg}"][-1]:10.2f} ms', flush=True)
            res['ms'] = {k: stats(v) for k, v in times.items()}
            med = {f: statistics.median(times[f'{f}_a'] + times[f'{f}_b']) for f in forms}
            res['score_ms'], res['forced_ms'] = med['score'], med['forced']
            res['spread_ms'] = max(abs(res['ms'][f'{f}_a']['median'] - res['ms'][f'{f}_b']['median']) for f in forms)
            res['forced_over_score'] = med['forced'] / med['score']
            res['score_not_slower'] = bool(med['score'] - med['forced'] <= res['spread_ms'])
            tokens = B * nb * dec.total_upscaling
            res['us_per_token'] = dict(score=med['score'] * 1e3 / tokens, forced=med['forced'] * 1e3 / tokens)
            head, kernel, R = launches_alone(dec, B, args.window_rows)
            res['alone'] = dict(scored_rows=R, head_us=head, kernel_us=kernel)
        rows.append(res)
        print(json.dumps(res), flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, 'w') as fh:
            json.dump(rows, fh, indent=1)


if __name__ == '__main__':
    main()
