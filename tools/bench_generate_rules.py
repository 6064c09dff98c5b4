"""Voice-leading rules at the DEC shape (d_model 512, 8 heads, 3 + 3 layers, T = 384, S = 24, U = 16), in ONE process on the same
decoder with alternating windows (profiles/generate_rules_perf_log.md):

  step       per B in --batches: us per replayed step (the 16 steps of the code at T / 2, between two device synchronisations) of
               default, default_again     the plain sampler, twice: what a call without any keyword runs
               masked, masked_again       the masked sampler with logp and allowed_mass, twice: two identical legs, whose
                                          difference is the spread
               rules                      the same plus vqcpc_decode_rules in front of the sampler (all three rules on)
  long       per B: ms per generated code of generate_from_code_long over --nb codes (a slide and 16 steps each) in the three legs
             masked, masked_again, rules
  launch     vqcpc_decode_rules alone on 32 rows, us per launch inside a captured graph of 20 launches, with every voice holding
             for 1 tick and for 384 ticks (six look-back iterations per voice, all but the latest ticks read from the chorale),
             and `floor`, the same launch with pos = T, which returns at once: what a kernel node of the graph costs by itself
  --default-only runs the `default` legs alone and uses nothing that a tree without the rules lacks: run from such a tree, in
  turns with this one, it is the comparison of the default path against the parent commit.

    python tools/bench_generate_rules.py [--batches 1,8,32] [--windows 5] [--json profiles/generate_rules_bench.json]
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


def spread(a, b):
    return max(abs(a['median'] - b['median']), a['max'] - a['min'], b['max'] - b['min'])


def timed(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / reps


def synthetic_kinds(vocab):
    """Per voice: 0 HOLD, 1 REST, the last three ids META, consecutive semitones around a centre that descends with the voice."""
    kinds = torch.full((len(vocab), max(vocab)), -3, dtype=torch.int16)
    for c, V in enumerate(vocab):
        n = V - 5
        kinds[c, 0], kinds[c, 1] = -1, -2
        kinds[c, 2:2 + n] = torch.clamp(72 - 5 * c - n // 2 + torch.arange(n), 0, 127).to(torch.int16)
    return kinds


def alternate(legs, windows, reps, label):
    for fn in legs.values():
        timed(fn, 1)                                                    # warm-up
    times = {k: [] for k in legs}
    for w in range(windows):
        for k, fn in legs.items():
            times[k].append(timed(fn, reps))
            print(f'{label} window {w} {k:15s} {times[k][-1]:10.2f}', flush=True)
    return {k: stats(v) for k, v in times.items()}


def step_legs(dec, B, windows, reps, rules):
    """us per replayed step: the 16 steps of the code at T / 2, on one stack per leg (a captured step holds its buffers)."""
    from vqcpc_bach_amd.decoders.generation import IncrementalDecoder
    T, S, U = dec.num_tokens_target, dec.num_tokens_source, dec.total_upscaling
    codes = torch.randint(0, dec.source_embeddings.weight.shape[0], (B, S), generator=torch.Generator().manual_seed(B)).cuda()
    kinds = {'default': {}, 'default_again': {}}
    if rules is not None:
        masked = dict(want_logp=True, want_allowed_mass=True)
        kinds.update(masked=masked, masked_again=masked, rules=dict(masked, rules=rules))
    legs, keep = {}, []
    for name, kw in kinds.items():
        inc = IncrementalDecoder(dec, B)
        inc.prefill(codes)
        inc.start(seeds=1, temperature=1.0, **kw)
        inc.step()
        graph = inc.capture(inc.step)
        inc.reset()
        for _ in range(T // 2):
            graph.replay()
        keep.append((inc, graph))

        def steps16(inc=inc, graph=graph):
            inc.pos.fill_(T // 2 - U)
            for _ in range(U):
                graph.replay()
        legs[name] = steps16
    res = alternate(legs, windows, reps, f'step B={B:2d}')
    res = {k: {s: v / U for s, v in r.items()} for k, r in res.items()}           # per step
    res.update(B=B, default_spread=spread(res['default'], res['default_again']))
    if rules is not None:
        res.update(spread=spread(res['masked'], res['masked_again']),
                   rules_minus_masked=res['rules']['median'] - res['masked']['median'])
    del keep
    return res


def long_legs(dec, B, nb, windows, rules):
    """ms per generated code of the long form."""
    vocab = [int(v) for v in dec.num_tokens_per_channel]
    pad, start = [v - 1 for v in vocab], [v - 3 for v in vocab]
    codes = torch.randint(0, dec.source_embeddings.weight.shape[0], (B, nb), generator=torch.Generator().manual_seed(B)).cuda()
    kw = dict(temperature=1.0, pad=pad, start=start, code_index_start=1, seed=3, return_logp=True, return_allowed_mass=True)
    legs = dict(masked=lambda: dec.generate_from_code_long(codes, **kw), masked_again=lambda: dec.generate_from_code_long(codes, **kw),
                rules=lambda: dec.generate_from_code_long(codes, rules=rules, **kw))
    res = alternate(legs, windows, 1, f'long B={B:2d}')
    res = {k: {s: v / 1e3 / (nb - 1) for s, v in r.items()} for k, r in res.items()}          # ms per code
    res.update(B=B, nb=nb, spread=spread(res['masked'], res['masked_again']),
               rules_minus_masked=res['rules']['median'] - res['masked']['median'])
    return res


def launch_legs(dec, rules, windows, reps):
    """vqcpc_decode_rules alone: 32 rows, every voice holding for `chain` ticks before the position."""
    import ctypes

    from vqcpc_bach_amd import hip
    M, nc, U, T = 32, dec.num_channels, dec.total_upscaling, dec.num_tokens_target
    vocab = [int(v) for v in dec.num_tokens_per_channel]
    off = [0]
    for v in vocab:
        off.append(off[-1] + v)
    off = (ctypes.c_int32 * (nc + 1))(*off)
    e = 390                                                              # the position's tick
    w0 = (e - 8) * nc // U                                               # the window starts late: most of the chain is chorale
    width = w0 * U + T
    assert w0 * U <= e * nc < w0 * U + T
    kinds, leap = rules.kinds.cuda(), rules.max_leap.cuda()
    sets = torch.zeros(M, width, 8, dtype=torch.int32, device='cuda')
    report = torch.full((M, width), -1, dtype=torch.int32, device='cuda')
    win = torch.tensor([w0 + 1, w0], dtype=torch.int32, device='cuda')
    legs, keep = {}, []
    for chain in (0, 1, 384):                                            # 0: the floor, a launch that returns at once (pos = T)
        col = e * nc + 1
        chorale = torch.full((M, width), 2, dtype=torch.int64)           # a pitch everywhere ...
        chorale.view(M, -1, nc)[:, e - chain:e] = 0                      # ... and `chain` holds in every voice before tick e
        tokens = chorale[:, w0 * U:w0 * U + T].contiguous().cuda()
        chorale = chorale.cuda()
        pos = torch.tensor([col - w0 * U if chain else T], dtype=torch.int32, device='cuda')

        def launch(tokens=tokens, chorale=chorale, pos=pos):
            hip.call('vqcpc_decode_rules', tokens, T, T, chorale, width, None, 0, kinds, kinds.shape[1], off, nc, leap, rules.mask,
                     None, None, 0, sets, width, report, width, pos, win, U, M)
        launch()
        torch.cuda.synchronize()
        assert chain == 0 or int(report[0, col]) >= 0, 'the launch wrote nothing'
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            for _ in range(20):
                launch()
        keep.append(graph)
        legs[f'chain_{chain}' if chain else 'floor'] = graph.replay
    res = alternate(legs, windows, reps, 'launch')
    res = {k: {s: v / 20 for s, v in r.items()} for k, r in res.items()}
    res.update(M=M, note='us per launch: 20 launches in one captured graph, replayed between two synchronisations')
    del keep
    return res


def markdown(res):
    cell = lambda s, f='.1f': f'{s["median"]:{f}} ({s["min"]:{f}} .. {s["max"]:{f}})'
    out = ['# Voice-leading rules at the DEC shape', '',
           f'Measured by `tools/bench_generate_rules.py` on {res["device"]}: one process, one decoder, alternating windows, '
           f'{res["windows"]} windows per leg; median (minimum .. maximum).  The `_again` legs repeat their leg; spread = the larger of '
           'the difference of the two medians and of either one\'s maximum - minimum.', '',
           '## One replayed step (us; the 16 steps of the code at T / 2)', '',
           '| B | default | default again | masked + logp + mass | again | spread | + rules | rules - masked |',
           '|---|---|---|---|---|---|---|---|']
    for r in res['step']:
        out.append(f'| {r["B"]} | {cell(r["default"])} | {cell(r["default_again"])} | {cell(r["masked"])} | {cell(r["masked_again"])} | '
                   f'{r["spread"]:.1f} | {cell(r["rules"])} | {r["rules_minus_masked"]:.1f} |')
    out += ['', f'## One long-form code (ms; a slide and 16 steps, {res["long"][0]["nb"]} codes per call)', '',
            '| B | masked + logp + mass | again | spread | + rules | rules - masked |', '|---|---|---|---|---|---|']
    for r in res['long']:
        out.append(f'| {r["B"]} | {cell(r["masked"], ".3f")} | {cell(r["masked_again"], ".3f")} | {r["spread"]:.3f} | '
                   f'{cell(r["rules"], ".3f")} | {r["rules_minus_masked"]:.3f} |')
    la = res['launch']
    out += ['', f'## vqcpc_decode_rules alone ({la["M"]} rows, us per launch: a captured graph of 20 launches, replayed)', '',
            '| every voice holds for | us |', '|---|---|', f'| (floor: pos = T, the kernel returns at once) | {cell(la["floor"], ".2f")} |',
            f'| 1 tick | {cell(la["chain_1"], ".2f")} |', f'| 384 ticks | {cell(la["chain_384"], ".2f")} |', '']
    return '\n'.join(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', default='1,8,32')
    ap.add_argument('--windows', type=int, default=5)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--nb', type=int, default=32)
    ap.add_argument('--default-only', action='store_true')
    ap.add_argument('--launch-only', action='store_true')
    ap.add_argument('--json', default=None)
    ap.add_argument('--log', default=None)
    args = ap.parse_args()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(root, 'tests'))
    assert torch.cuda.is_available(), 'bench_generate_rules needs the GPU'
    from oracle import decoder_oracle as D
    from test_decoder_gpu import seeded_decoder
    from vqcpc_bach_amd.utils import STEP_LOCK
    dec, _ = seeded_decoder(D.make_cfg('DEC', B=8), 5)
    dec.eval()
    rules = None
    if not args.default_only:
        from vqcpc_bach_amd import templates
        rules = templates.VoiceLeadingRules(synthetic_kinds([int(v) for v in dec.num_tokens_per_channel]), no_crossing=True, max_leap=12,
                                            no_parallels=True)
    batches = [int(b) for b in args.batches.split(',')]
    res = dict(device=torch.cuda.get_device_name(0), windows=args.windows, reps=args.reps, step=[])
    with STEP_LOCK, torch.no_grad():
        for B in batches if not args.launch_only else []:
            res['step'].append(step_legs(dec, B, args.windows, args.reps, rules))
        if rules is not None:
            res['launch'] = launch_legs(dec, rules, args.windows, 2 * args.reps)
    if rules is not None and not args.launch_only:
        res['long'] = [long_legs(dec, B, args.nb, max(2, args.windows // 2), rules) for B in batches]
    print(json.dumps(res), flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, 'w') as fh:
            json.dump(res, fh, indent=1)
    if args.log and rules is not None and not args.launch_only:
        with open(args.log, 'w') as fh:
            fh.write(markdown(res))


if __name__ == '__main__':
    main()
