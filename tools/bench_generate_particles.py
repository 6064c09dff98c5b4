"""Particle resampling at the DEC shape (d_model 512, 8 heads, 3 + 3 layers, T = 384, S = 24, U = 16), in ONE process on the same
decoder with alternating windows (profiles/generate_particles_perf_log.md):

  launches   on a 64-row stack, per P in --particles and per pos in {U, T / 2, T - U}, us per call between two device
             synchronisations (--reps calls per window), with a cyclic shift inside every group as the ancestor map (every row
             moves: the most a resampling can cost):
               steps16, steps16_again   the 16 replayed steps of a code, twice: two identical legs, whose difference is the spread
               resample                 vqcpc_particle_resample alone
               permute_rows             the permute launches without the caches (tokens, logp, next input row)
               permute_all              the same plus the K and V caches of every layer, in place through LDS
               scratch_caches           the caches through a scratch image instead (gather into a copy, copy back; torch's
                                        index_select + copy_ stand in for the two kernels of that design)
             and the achieved bytes per second of the in-place cache move (rows x pos x d x 4 bytes, read and written once, K
             and V of every layer) against the 6.29 TB/s float4 copy rate of the part.
  long       generate_from_code_long over nb = 96 codes with half of the positions forced, 64 rows: `particles=P` over 64 / P
             user rows against `num_decodings=P` over the same rows, seconds per call.
  quality    (information only: the decoder is randomly initialised) per P in {1, 4, 16} over --seeds seeds: the mean summed
             logp at the forced positions of the returned row, and the standard deviation of log_evidence.

    python tools/bench_generate_particles.py [--particles 4,16,64] [--windows 5] [--json profiles/generate_particles_bench.json]
                                             [--log profiles/generate_particles_perf_log.md]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

COPY_RATE = 6.29e12            # bytes / s, float4 copy measured on the MI355X


def stats(t):
    return dict(median=statistics.median(t), min=min(t), max=max(t))


def timed(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / reps


def forced_half(dec, B, nb, seed):
    """(B, nb * events_per_code, channels) int64: a random token at a random half of the positions, -1 elsewhere."""
    g = torch.Generator().manual_seed(seed)
    nc, epc = dec.num_channels, dec.num_events_per_code
    given = torch.cat([torch.randint(0, int(v) - 3, (B, nb * epc, 1), generator=g) for v in dec.num_tokens_per_channel], dim=2)
    return torch.where(torch.rand(B, nb * epc, nc, generator=g) < 0.5, given, torch.full_like(given, -1)).cuda()


def launch_legs(dec, P, windows, reps):
    """The kernel-level legs on one 64-row stack with groups of P."""
    from vqcpc_bach_amd import hip
    from vqcpc_bach_amd.decoders.generation import IncrementalDecoder
    M = 64
    T, S, U, d = dec.num_tokens_target, dec.num_tokens_source, dec.total_upscaling, dec.d_model
    g = torch.Generator().manual_seed(P)
    codes = torch.randint(0, dec.source_embeddings.weight.shape[0], (M, S), generator=g).cuda()
    cons = forced_half(dec, M // P, S, seed=P).reshape(M // P, T).repeat_interleave(P, dim=0)
    inc = IncrementalDecoder(dec, M)
    inc.prefill(codes)
    inc.start(seeds=1, temperature=1.0, constraint=cons, particles=P, resample_threshold=1.0)
    inc.step()
    step_graph = inc.capture(inc.step)
    inc.reset()
    for _ in range(T):                                                  # a whole generation: live caches, tokens and scores
        step_graph.replay()
    layers = len(inc.layers)
    shift = (torch.arange(M).view(M // P, P).roll(-1, dims=1)).reshape(M).to(torch.int32).cuda()
    one = torch.ones(1, dtype=torch.int32, device='cuda')
    shift64 = shift.long()
    out = []
    for pos in (U, T // 2, T - U):
        def set_pos(p=pos):
            inc.pos.fill_(p)

        def steps16():
            set_pos(pos - U)
            for _ in range(U):
                step_graph.replay()

        def resample():
            hip.call('vqcpc_particle_resample', inc.p_lw, inc.p_evidence, inc.p_pending, inc.p_seeds, inc.constraint, T, inc.logp, T,
                     None, T, inc.pos, None, U, 1.0, 0, inc.p_anc, inc.p_wn, inc.p_ess, inc.p_flag, inc.p_hist_anc, inc.p_hist_wn,
                     inc.p_hist_ess, S, M, P)

        def permute_rows():
            hip.call('vqcpc_particle_permute_i64', inc.tokens, T, T, inc.pos, shift, one, M, P)
            hip.call('vqcpc_particle_permute_f32', inc.logp, T, T, None, shift, one, M, P)
            hip.call('vqcpc_particle_permute_f32', inc.x, d, d, None, shift, one, M, P)

        def permute_all():
            permute_rows()
            for cache in (inc.kcache, inc.vcache):
                hip.call('vqcpc_particle_permute_cache', cache, layers, T, d, inc.pos, shift, one, M, P)

        def scratch_caches(p=pos):
            for cache in (inc.kcache, inc.vcache):
                live = cache[:, :, :p]
                live.copy_(live.index_select(1, shift64))

        legs = dict(steps16=steps16, steps16_again=steps16, resample=resample, permute_rows=permute_rows, permute_all=permute_all,
                    scratch_caches=scratch_caches)
        set_pos()
        for fn in legs.values():
            timed(fn, 2)                                                # warm-up
        times = {k: [] for k in legs}
        for w in range(windows):
            for k, fn in legs.items():
                set_pos()
                times[k].append(timed(fn, reps if k not in ('steps16', 'steps16_again') else max(1, reps // 8)))
                print(f'P={P:2d} pos={pos:3d} window {w} {k:15s} {times[k][-1]:10.2f} us', flush=True)
        res = {k: stats(v) for k, v in times.items()}
        a, b = res['steps16'], res['steps16_again']
        moved = 2 * layers * M * pos * d * 4 * 2                        # K and V, every layer, every row, read + written
        cache_us = res['permute_all']['median'] - res['permute_rows']['median']
        res.update(P=P, pos=pos, spread=max(abs(a['median'] - b['median']), a['max'] - a['min'], b['max'] - b['min']),
                   cache_bytes=moved, cache_us=cache_us, cache_rate=moved / (cache_us * 1e-6),
                   cache_share_of_copy_rate=moved / (cache_us * 1e-6) / COPY_RATE,
                   per_code_share=(res['resample']['median'] + res['permute_all']['median']) / a['median'])
        out.append(res)
    del step_graph
    return out


def long_legs(dec, Ps, nb, windows, seeds):
    """Long form over nb codes, half of the positions forced, 64 rows: particles=P against num_decodings=P."""
    vocab = [int(v) for v in dec.num_tokens_per_channel]
    pad, start = [v - 1 for v in vocab], [v - 3 for v in vocab]
    g = torch.Generator().manual_seed(7)
    rows = []
    for P in Ps:
        B = max(1, 64 // P)
        codes = torch.randint(0, dec.source_embeddings.weight.shape[0], (B, nb), generator=g).cuda()
        cons = forced_half(dec, B, nb, seed=100 + P)
        kw = dict(temperature=1.0, pad=pad, start=start, constraint=cons, return_logp=True)
        legs = dict(num_decodings=lambda s: dec.generate_from_code_long(codes, num_decodings=P, seed=s, **kw),
                    num_decodings_again=lambda s: dec.generate_from_code_long(codes, num_decodings=P, seed=s, **kw),
                    particles=lambda s: dec.generate_from_code_long(codes, particles=P, seed=s, **kw))
        for fn in legs.values():
            fn(0)
        times = {k: [] for k in legs}
        for w in range(windows):
            for k, fn in legs.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn(w + 1)
                torch.cuda.synchronize()
                times[k].append(time.perf_counter() - t0)
                print(f'long P={P:2d} B={B:2d} window {w} {k:20s} {times[k][-1]:8.3f} s', flush=True)
        res = {k: stats(v) for k, v in times.items()}
        a, b = res['num_decodings'], res['num_decodings_again']
        res.update(P=P, B=B, nb=nb, spread=max(abs(a['median'] - b['median']), a['max'] - a['min'], b['max'] - b['min']),
                   particles_over_plain=res['particles']['median'] / a['median'])
        rows.append(res)
    # information only: how much the returned row's forced tokens are worth, and how steady the evidence estimate is
    quality = []
    codes = torch.randint(0, dec.source_embeddings.weight.shape[0], (1, nb), generator=g).cuda()
    cons = forced_half(dec, 1, nb, seed=99)
    kw = dict(temperature=1.0, pad=pad, start=start, constraint=cons, return_logp=True)
    for P in (1, 4, 16):
        score, evid = [], []
        for s in range(seeds):
            if P == 1:
                _, lp = dec.generate_from_code_long(codes, seed=s, **kw)
                total = float(lp[cons >= 0].double().sum())
                score.append(total), evid.append(total)
            else:
                _, lp = dec.generate_from_code_long(codes, particles=P, seed=s, **kw)
                score.append(float(lp[cons >= 0].double().sum()))
                *_, info = dec.generate_from_code_long(codes, particles=P, seed=s, return_particles=True, **kw)
                evid.append(float(info['log_evidence'][0]))
        quality.append(dict(P=P, seeds=seeds, mean_forced_logp=statistics.mean(score),
                            log_evidence_mean=statistics.mean(evid), log_evidence_std=statistics.pstdev(evid)))
        print(json.dumps(quality[-1]), flush=True)
    return rows, quality


def markdown(res):
    cell = lambda s: f'{s["median"]:.1f} ({s["min"]:.1f} .. {s["max"]:.1f})'
    out = ['# Particle resampling at the DEC shape', '',
           f'Measured by `tools/bench_generate_particles.py` on {res["device"]}: one process, one decoder, alternating windows, '
           f'{res["windows"]} windows per leg; median (minimum .. maximum).  steps16 and steps16_again are the same leg twice; spread '
           '= the larger of the difference of their medians and of either one\'s maximum - minimum.', '',
           '## The launches of one resampling against the 16 replayed steps of a code (64 rows, us)', '',
           'Ancestor map: a cyclic shift inside every group, so every row moves.  permute_rows = tokens, logp and the next input '
           'row; permute_all = the same plus the K and V caches of every layer, in place through LDS; scratch_caches = the caches '
           'alone through a scratch image (gather into a copy, copy back).  cache rate = the bytes of the live cache rows, read and '
           f'written once, over permute_all - permute_rows; share = that rate over the part\'s {COPY_RATE / 1e12:.2f} TB/s float4 copy '
           'rate.  (resample + permute_all) / steps16 is what a resampling after every code adds to the code\'s steps.', '',
           '| P | pos | steps16 | steps16_again | spread | resample | permute_rows | permute_all | scratch_caches | cache MB | '
           'cache rate TB/s | share | (resample + permute_all) / steps16 |', '|---|---|---|---|---|---|---|---|---|---|---|---|---|']
    for r in res['launches']:
        out.append(f'| {r["P"]} | {r["pos"]} | {cell(r["steps16"])} | {cell(r["steps16_again"])} | {r["spread"]:.1f} | '
                   f'{cell(r["resample"])} | {cell(r["permute_rows"])} | {cell(r["permute_all"])} | {cell(r["scratch_caches"])} | '
                   f'{r["cache_bytes"] / 1e6:.1f} | {r["cache_rate"] / 1e12:.2f} | {r["cache_share_of_copy_rate"]:.2f} | '
                   f'{r["per_code_share"]:.3f} |')
    if res.get('long'):
        cs = lambda s: f'{s["median"]:.3f} ({s["min"]:.3f} .. {s["max"]:.3f})'
        out += ['', f'## Long form, {res["long"][0]["nb"]} codes, half of the positions forced, B x P = 64 rows (s per call)', '',
                '| P | B | num_decodings=P | num_decodings=P again | spread | particles=P | particles / num_decodings |',
                '|---|---|---|---|---|---|---|']
        for r in res['long']:
            out.append(f'| {r["P"]} | {r["B"]} | {cs(r["num_decodings"])} | {cs(r["num_decodings_again"])} | {r["spread"]:.3f} | '
                       f'{cs(r["particles"])} | {r["particles_over_plain"]:.3f} |')
        out += ['', '## For information: the returned row and the evidence (randomly initialised decoder, one user row)', '',
                '| P | seeds | mean summed logp at the forced positions | mean log_evidence | std of log_evidence |',
                '|---|---|---|---|---|']
        for q in res['quality']:
            out.append(f'| {q["P"]} | {q["seeds"]} | {q["mean_forced_logp"]:.2f} | {q["log_evidence_mean"]:.2f} | '
                       f'{q["log_evidence_std"]:.2f} |')
    out.append('')
    return '\n'.join(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--particles', default='4,16,64')
    ap.add_argument('--windows', type=int, default=5)
    ap.add_argument('--reps', type=int, default=40)
    ap.add_argument('--nb', type=int, default=96)
    ap.add_argument('--seeds', type=int, default=6)
    ap.add_argument('--skip-long', action='store_true')
    ap.add_argument('--json', default=None)
    ap.add_argument('--log', default=None)
    args = ap.parse_args()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(root, 'tests'))
    assert torch.cuda.is_available(), 'bench_generate_particles needs the GPU'
    from oracle import decoder_oracle as D
    from test_decoder_gpu import seeded_decoder
    from vqcpc_bach_amd.utils import STEP_LOCK
    dec, _ = seeded_decoder(D.make_cfg('DEC', B=8), 5)
    dec.eval()
    Ps = [int(p) for p in args.particles.split(',')]
    res = dict(device=torch.cuda.get_device_name(0), windows=args.windows, reps=args.reps, launches=[])
    with STEP_LOCK, torch.no_grad():
        for P in Ps:
            res['launches'] += launch_legs(dec, P, args.windows, args.reps)
    if not args.skip_long:
        res['long'], res['quality'] = long_legs(dec, [p for p in Ps if p <= 16], args.nb, max(2, args.windows // 2), args.seeds)
    print(json.dumps(res), flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, 'w') as fh:
            json.dump(res, fh, indent=1)
    if args.log:
        with open(args.log, 'w') as fh:
            fh.write(markdown(res))


if __name__ == '__main__':
    main()
