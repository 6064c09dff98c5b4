"""Beam search at the DEC shape (d_model 512, 8 heads, 3 + 3 layers, T = 384, S = 24, U = 16), in ONE process on the same decoder
with alternating windows (profiles/generate_beam_perf_log.md):

  steps      per (rows, W) in --shapes, us per replayed step between two device synchronisations (--reps replays per window from
             position T / 2, live caches of a whole generation behind them):
               plain, plain_again       the default path's captured step at the same number of rows, twice: two identical legs,
                                        whose difference is the spread
               beam_in_step             the captured step with vqcpc_decode_beam_select and the moves inside it
               beam_between             the captured step with the select inside and the moves issued eagerly after every replay
               select                   vqcpc_decode_beam_select alone (eager launches)
               move_tokens, move_logp, move_caches   each permute alone, with a cyclic shift inside every group as the ancestor
                                        map (every row moves: the most a step's moves can cost)
  long       generate_from_code_long over --nb codes with half of the positions forced: `beam=W` over 64 / W user rows against
             `num_decodings=W` over the same rows, seconds per call.
  --plain-only measures the plain legs alone (the default path, for a comparison against another checkout of the package).

    python tools/bench_generate_beam.py [--shapes 64x4,64x16,64x64,8x8] [--windows 5] [--json profiles/generate_beam_bench.json]
                                        [--log profiles/generate_beam_perf_log.md]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch


def stats(t):
    return dict(median=statistics.median(t), min=min(t), max=max(t))


def timed(fn, reps, before=None):
    if before is not None:
        before()
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


def _stack(dec, M, codes, graph_moves=None, **start):
    """A stack after a whole generation, with its captured step."""
    from vqcpc_bach_amd.decoders.generation import IncrementalDecoder
    inc = IncrementalDecoder(dec, M)
    if graph_moves is not None:
        inc.beam_moves_in_step = graph_moves
    inc.prefill(codes)
    inc.start(**start)
    inc.step()
    graph = inc.capture(inc.step)
    inc.reset()
    for t in range(inc.T):
        graph.replay()
        inc._code_done(t + 1)
    return inc, graph


def step_legs(dec, M, W, windows, reps, plain_only=False):
    from vqcpc_bach_amd import hip
    T, S, d = dec.num_tokens_target, dec.num_tokens_source, dec.d_model
    g = torch.Generator().manual_seed(W)
    codes = torch.randint(0, dec.source_embeddings.weight.shape[0], (M, S), generator=g).cuda()
    plain, plain_graph = _stack(dec, M, codes, seeds=1, temperature=1.0)
    pos0 = T // 2
    legs = dict(plain=(plain_graph.replay, lambda: plain.pos.fill_(pos0)), plain_again=(plain_graph.replay, lambda: plain.pos.fill_(pos0)))
    keep = [plain, plain_graph]
    if not plain_only:
        cons = forced_half(dec, M // W, S, seed=W).reshape(M // W, T).repeat_interleave(W, dim=0)
        kw = dict(constraint=cons, want_logp=True, beam=W)
        a, ga = _stack(dec, M, codes, True, **kw)
        b, gb = _stack(dec, M, codes, False, **kw)
        keep += [a, ga, b, gb]
        layers = len(a.layers)
        shift = (torch.arange(M).view(M // W, W).roll(-1, dims=1)).reshape(M).to(torch.int32).cuda()
        one = torch.ones(1, dtype=torch.int32, device='cuda')
        bound = torch.tensor([pos0, pos0], dtype=torch.int32, device='cuda')

        def between():
            gb.replay()
            b._beam_moves()

        def select():
            hip.call('vqcpc_decode_beam_select', a.logits, a.logits.shape[1], a._offsets_c, a.nc, M, W, None, a.constraint, T, None, T,
                     a.logp, T, None, T, None, T, None, a.tokens, T, T, a.table, a.table.shape[0], d, a.U, a.x, d, a.b_score, a.b_anc,
                     a.b_flag, a.b_bound, a.b_hist, T, None, a.pos)
        legs.update(beam_in_step=(ga.replay, lambda: a.pos.fill_(pos0)), beam_between=(between, lambda: b.pos.fill_(pos0)),
                    select=(select, lambda: a.pos.fill_(pos0)))
        if W > 1:
            legs.update(
                move_tokens=(lambda: hip.call('vqcpc_particle_permute_i64', a.tokens, T, T, bound[0:1], shift, one, M, W), None),
                move_logp=(lambda: hip.call('vqcpc_particle_permute_f32', a.logp, T, T, bound[1:2], shift, one, M, W), None),
                move_caches=(lambda: [hip.call('vqcpc_particle_permute_cache', c, layers, T, d, bound[0:1], shift, one, M, W)
                                      for c in (a.kcache, a.vcache)], None))
    for fn, before in legs.values():
        timed(fn, 4, before)                                              # warm-up
    times = {k: [] for k in legs}
    for w in range(windows):
        for k, (fn, before) in legs.items():
            times[k].append(timed(fn, reps, before))
            print(f'M={M:2d} W={W:2d} window {w} {k:13s} {times[k][-1]:9.2f} us', flush=True)
    res = {k: stats(v) for k, v in times.items()}
    p, q = res['plain'], res['plain_again']
    res.update(M=M, W=W, pos=pos0, spread=max(abs(p['median'] - q['median']), p['max'] - p['min'], q['max'] - q['min']))
    if not plain_only:
        res.update(in_step_over_plain=res['beam_in_step']['median'] / p['median'],
                   between_over_plain=res['beam_between']['median'] / p['median'])
    del keep
    return res


def long_legs(dec, Ws, nb, windows):
    vocab = [int(v) for v in dec.num_tokens_per_channel]
    pad, start = [v - 1 for v in vocab], [v - 3 for v in vocab]
    g = torch.Generator().manual_seed(7)
    rows = []
    for W in Ws:
        B = max(1, 64 // W)
        codes = torch.randint(0, dec.source_embeddings.weight.shape[0], (B, nb), generator=g).cuda()
        cons = forced_half(dec, B, nb, seed=100 + W)
        kw = dict(temperature=1.0, pad=pad, start=start, constraint=cons, return_logp=True)
        legs = dict(num_decodings=lambda s: dec.generate_from_code_long(codes, num_decodings=W, seed=s, **kw),
                    num_decodings_again=lambda s: dec.generate_from_code_long(codes, num_decodings=W, seed=s, **kw),
                    beam=lambda s: dec.generate_from_code_long(codes, beam=W, **kw))
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
                print(f'long W={W:2d} B={B:2d} window {w} {k:20s} {times[k][-1]:8.3f} s', flush=True)
        res = {k: stats(v) for k, v in times.items()}
        p, q = res['num_decodings'], res['num_decodings_again']
        _, lp = legs['beam'](0)
        _, lq = legs['num_decodings'](0)
        res.update(W=W, B=B, nb=nb, spread=max(abs(p['median'] - q['median']), p['max'] - p['min'], q['max'] - q['min']),
                   beam_over_plain=res['beam']['median'] / p['median'],
                   beam_total_logp=float(lp.double().reshape(B, -1).sum(dim=1).mean()),
                   best_sampled_total_logp=float(lq.double().reshape(B, W, -1).sum(dim=2).max(dim=1)[0].mean()))
        rows.append(res)
    return rows


def markdown(res):
    cell = lambda s: f'{s["median"]:.1f} ({s["min"]:.1f} .. {s["max"]:.1f})'
    out = ['# Beam search at the DEC shape', '',
           f'Measured by `tools/bench_generate_beam.py` on {res["device"]}: one process, one decoder, alternating windows, '
           f'{res["windows"]} windows of {res["reps"]} calls per leg; median (minimum .. maximum).  plain and plain_again are the same '
           'leg twice; spread = the larger of the difference of their medians and of either one\'s maximum - minimum.', '',
           '## One replayed step (us): the default path against `beam=W` at the same number of rows', '',
           'beam_in_step: the select and the moves are launches of the captured step; beam_between: the select inside, the moves '
           'issued eagerly after every replay.  select and move_* are eager launches alone; the moves use a cyclic shift inside '
           'every group, so every row moves, at position T / 2.', '',
           '| rows | W | plain | plain_again | spread | beam_in_step | beam_between | in_step / plain | between / plain | select | '
           'move_tokens | move_logp | move_caches |', '|---|---|---|---|---|---|---|---|---|---|---|---|---|']
    for r in res['steps']:
        mv = [cell(r[k]) if k in r else '-' for k in ('move_tokens', 'move_logp', 'move_caches')]
        out.append(f'| {r["M"]} | {r["W"]} | {cell(r["plain"])} | {cell(r["plain_again"])} | {r["spread"]:.1f} | '
                   f'{cell(r["beam_in_step"])} | {cell(r["beam_between"])} | {r["in_step_over_plain"]:.3f} | '
                   f'{r["between_over_plain"]:.3f} | {cell(r["select"])} | {mv[0]} | {mv[1]} | {mv[2]} |')
    if res.get('long'):
        cs = lambda s: f'{s["median"]:.3f} ({s["min"]:.3f} .. {s["max"]:.3f})'
        out += ['', f'## Long form, {res["long"][0]["nb"]} codes, half of the positions forced, B x W = 64 rows (s per call)', '',
                'total logp: the mean over the user rows of the returned hypothesis\'s summed log-probability, against the best of the '
                'W sampled decodings (randomly initialised decoder: information only).', '',
                '| W | B | num_decodings=W | num_decodings=W again | spread | beam=W | beam / num_decodings | beam total logp | '
                'best sampled total logp |', '|---|---|---|---|---|---|---|---|---|']
        for r in res['long']:
            out.append(f'| {r["W"]} | {r["B"]} | {cs(r["num_decodings"])} | {cs(r["num_decodings_again"])} | {r["spread"]:.3f} | '
                       f'{cs(r["beam"])} | {r["beam_over_plain"]:.3f} | {r["beam_total_logp"]:.1f} | {r["best_sampled_total_logp"]:.1f} |')
    out.append('')
    return '\n'.join(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='64x4,64x16,64x64,8x8')
    ap.add_argument('--windows', type=int, default=5)
    ap.add_argument('--reps', type=int, default=32)
    ap.add_argument('--nb', type=int, default=96)
    ap.add_argument('--long', default='4,16')
    ap.add_argument('--skip-long', action='store_true')
    ap.add_argument('--plain-only', action='store_true')
    ap.add_argument('--json', default=None)
    ap.add_argument('--log', default=None)
    args = ap.parse_args()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(root, 'tests'))
    assert torch.cuda.is_available(), 'bench_generate_beam needs the GPU'
    from oracle import decoder_oracle as D
    from test_decoder_gpu import seeded_decoder
    from vqcpc_bach_amd.utils import STEP_LOCK
    dec, _ = seeded_decoder(D.make_cfg('DEC', B=8), 5)
    dec.eval()
    shapes = [tuple(int(v) for v in s.split('x')) for s in args.shapes.split(',')]
    res = dict(device=torch.cuda.get_device_name(0), windows=args.windows, reps=args.reps, steps=[])
    with STEP_LOCK, torch.no_grad():
        for M, W in shapes:
            res['steps'].append(step_legs(dec, M, W, args.windows, args.reps, args.plain_only))
    if not args.skip_long and not args.plain_only:
        res['long'] = long_legs(dec, [int(w) for w in args.long.split(',')], args.nb, max(2, args.windows // 2))
    print(json.dumps(res), flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, 'w') as fh:
            json.dump(res, fh, indent=1)
    if args.log and not args.plain_only:
        with open(args.log, 'w') as fh:
            fh.write(markdown(res))


if __name__ == '__main__':
    main()
