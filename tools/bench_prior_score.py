"""`PriorRelative.score_codes(method='windows')` against the two ways the same scores were had before, at the PRI shape
(tools/bench_prior.py: d_model 512, 8 heads, 6 layers, ff 1024, N = 24 codes per window, V = 32), 96 codes, per batch B in --batches,
in ONE process with alternating timing windows (profiles/prior_score_perf_log.md):

  score     ms per call of three arms over the same pieces: `windows` (96 - 24 + 1 = 73 windows per piece, rows of one batched forward),
            `default` (`score_codes` as it was: the forced generation, 24 cached steps and 72 moves) and `loop` (one bare `forward` per
            window + log_softmax, the loop of tools/bench_prior_constrained.py).  Each arm runs TWICE per round as two identical legs
            (a, b); the legs alternate a-windows, a-default, a-loop, b-windows, ...  The spread is the largest |median(a) - median(b)| of
            the arms: what a difference between arms has to exceed.  The largest difference between the arms' scores is reported.
  rows      the same `windows` call per `window_rows` in {32, 64, 128, 256, 512}, alternating: the table behind the default
  alone     us per vqcpc_prior_score launch at R = 2 336 rows (32 pieces x 73 windows), V = 4 096 and V = 32, logp alone and every
            output, with the achieved read rate R V 4 bytes / time; and us per pass of the head over R gathered rows in its two forms,
            vqcpc_decode_linear with `gather` in slices of 64 rows against index_select + the training path's GEMM
  product   PRI shape on a 2 x 64 encoder (tools/bench_product_codes.py): `windows` against `default` for code_model 'product' and for
            the merged prior of V = 4 096
  chorale   `score_chorale` end to end at the DEC shape: a piece of 72 codes of tokens, and the share of the prior's half

    timeout -k 10 900 python tools/bench_prior_score.py [--sections score,rows,alone,product,chorale] [--batches 1,8,32] [--rounds 5]
                                                        [--json profiles/prior_score_perf_log.json]

Every invocation is one GPU step: run it under its own `timeout`, as above.  Device-synchronised host clocks, warm-up first."""
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

WINDOW_ROWS = (32, 64, 128, 256, 512)


def timed(fn, reps=1):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        out = fn()
    torch.cuda.synchronize()
    del out
    return (time.perf_counter() - t0) / reps


def stats(t):
    return dict(median=statistics.median(t), min=min(t), max=max(t))


def two_legs(arms, rounds, label=''):
    """arms: {name: fn}.  One warm-up of each, then `rounds` rounds of a-arm..., b-arm... -> ({arm_leg: stats}, {arm: median over
    both legs}, spread), ms."""
    for fn in arms.values():
        fn()
    times = {f'{k}_{leg}': [] for leg in 'ab' for k in arms}
    for r in range(rounds):
        for leg in 'ab':
            for k, fn in arms.items():
                times[f'{k}_{leg}'].append(timed(fn) * 1e3)
    ms = {k: stats(v) for k, v in times.items()}
    med = {k: statistics.median(times[f'{k}_a'] + times[f'{k}_b']) for k in arms}
    spread = max(abs(ms[f'{k}_a']['median'] - ms[f'{k}_b']['median']) for k in arms)
    print(f'{label} ' + ', '.join(f'{k} {v:.2f} ms' for k, v in med.items()) + f', spread {spread:.2f} ms', flush=True)
    return ms, med, spread


def per_window_loop(prior, dcodes):
    """One bare forward per window + log_softmax (merged prior, stride 1): the loop of tools/bench_prior_constrained.py."""
    N, nt = prior.num_tokens, dcodes.shape[1]
    with torch.no_grad():
        cols = [torch.log_softmax(prior.forward(dcodes[:, :N])['weights_per_category'][0], dim=-1)
                .gather(2, dcodes[:, :N].unsqueeze(2)).squeeze(2)]
        for e in range(N, nt):
            w = dcodes[:, e - N + 1:e + 1]
            lg = prior.forward(w)['weights_per_category'][0][:, N - 1]
            cols.append(torch.log_softmax(lg, dim=-1).gather(1, w[:, N - 1:]))
        return torch.cat(cols, dim=1)


def section_score(prior, batches, rounds, nt):
    rows = []
    V = prior.num_tokens_per_channel[0]
    for B in batches:
        codes = torch.randint(0, V, (B, nt), generator=torch.Generator().manual_seed(B)).cuda()
        arms = dict(windows=lambda: prior.score_codes(codes, method='windows'), default=lambda: prior.score_codes(codes),
                    loop=lambda: per_window_loop(prior, codes))
        got = {k: fn() for k, fn in arms.items()}
        res = dict(batch=B, codes=nt, max_abs_difference={f'{a}-{b}': float((got[a].double() - got[b].double()).abs().max())
                                                          for a, b in (('windows', 'default'), ('windows', 'loop'), ('default', 'loop'))})
        del got
        res['ms'], med, res['spread_ms'] = two_legs(arms, rounds, f'score B={B:2d}')
        res.update({f'{k}_ms': v for k, v in med.items()})
        res['windows_faster_than_both_by_more_than_the_spread'] = bool(min(med['default'], med['loop']) - med['windows'] > res['spread_ms'])
        rows.append(res)
    return rows


def section_rows(prior, batches, rounds, nt):
    rows = []
    V = prior.num_tokens_per_channel[0]
    for B in batches:
        codes = torch.randint(0, V, (B, nt), generator=torch.Generator().manual_seed(B)).cuda()
        arms = {f'rows{w}': (lambda w=w: prior.score_codes(codes, method='windows', window_rows=w)) for w in WINDOW_ROWS}
        ms, med, spread = two_legs(arms, rounds, f'rows  B={B:2d}')
        rows.append(dict(batch=B, windows=B * (nt - prior.num_tokens + 1), ms=med, spread_ms=spread))
    return rows


def section_alone(R=2336, d=512, reps=200):
    from vqcpc_bach_amd import hip, ops
    out = []
    g = torch.Generator().manual_seed(7)
    pieces, cols = 32, 96
    for V in (4096, 32):
        logits = (torch.randn(R, V, generator=g) * 2).cuda()
        row_b = (torch.arange(R, dtype=torch.int32) % pieces).cuda()
        row_col = (torch.arange(R, dtype=torch.int32) // pieces).cuda()
        seq = torch.randint(0, V, (pieces, cols), generator=g).cuda()
        res = [torch.empty(pieces, cols, dtype=dt, device='cuda') for dt in (torch.float32, torch.float32, torch.int32, torch.int64,
                                                                             torch.float32)]

        def kernel(full):
            lp, ent, rk, bs, bl = res if full else (res[0], None, None, None, None)
            hip.call('vqcpc_prior_score', logits, V, V, 1, 0, R, row_b, row_col, seq, cols, pieces, cols, lp, cols, cols, ent, rk, bs, bl)
            return res[0]
        hidden = torch.randn(R + 512, d, generator=g).cuda()
        gather = torch.randperm(R + 512, generator=g)[:R].cuda()
        w, b = (torch.randn(V, d, generator=g) / d ** 0.5).cuda(), torch.randn(V, generator=g).cuda()
        lg = torch.empty(R, V, device='cuda')

        def head_linear():
            for g0 in range(0, R, 64):
                m = min(64, R - g0)
                hip.call('vqcpc_decode_linear', hidden, d, gather[g0:], w, b, None, 0, lg[g0:], V, m, V, d, 0)
            return lg

        def head_gemm():
            return ops.gemm_nt(hidden.index_select(0, gather), w, bias=b)
        for fn in (lambda: kernel(False), lambda: kernel(True), head_linear, head_gemm):
            fn()
        diff = float((head_linear() - head_gemm()).abs().max())
        us = dict(kernel_logp=timed(lambda: kernel(False), reps) * 1e6, kernel_all=timed(lambda: kernel(True), reps) * 1e6,
                  head_decode_linear=timed(head_linear, 20) * 1e6, head_gemm=timed(head_gemm, 20) * 1e6)
        row = dict(V=V, rows=R, d=d, us=us, head_forms_max_abs_difference=diff,
                   kernel_read_TB_per_s={k: R * V * 4 / (us[k] * 1e-6) / 1e12 for k in ('kernel_logp', 'kernel_all')})
        print(json.dumps(row), flush=True)
        out.append(row)
    return out


def section_product(batches, rounds, nt):
    from bench_product_codes import build_prior
    rows = []
    for code_model in ('product', 'merged'):
        prior, _ = build_prior(64, 2, code_model, seed=6)
        prior.eval()
        for B in batches:
            codes = torch.randint(0, 4096, (B, nt), generator=torch.Generator().manual_seed(B)).cuda()
            arms = dict(windows=lambda: prior.score_codes(codes, method='windows'), default=lambda: prior.score_codes(codes))
            a, b = arms['windows'](), arms['default']()
            diff = float((a.double() - b.double()).abs().max())
            ms, med, spread = two_legs(arms, rounds, f'{code_model} 2 x 64 B={B:2d}')
            rows.append(dict(code_model=code_model, K=64, ncb=2, batch=B, ms=med, spread_ms=spread, max_abs_difference=diff))
        del prior
    return rows


def section_chorale(prior, dec, rounds):
    vocab = [int(v) for v in dec.num_tokens_per_channel]
    dec.dataloader_generator = types.SimpleNamespace(dataset=types.SimpleNamespace(
        note2index_dicts=[{'START': v - 3, 'END': v - 2, 'XX': v - 1} for v in vocab]))
    g = torch.Generator().manual_seed(4)
    x = torch.cat([torch.randint(0, v - 3, (1, 72 * dec.num_events_per_code, 1), generator=g) for v in vocab], dim=2)
    res = prior.score_chorale(x, dec)
    n2i = dec.dataloader_generator.dataset.note2index_dicts
    chunks = dec._frame_and_encode(x, n2i)[3]
    framed = torch.cat([prior.encode(c.unsqueeze(0)) for c in chunks], dim=1)
    arms = dict(score_chorale=lambda: prior.score_chorale(x, dec), prior_half=lambda: prior.score_codes(framed, method='windows'),
                decoder_half=lambda: dec.score_chorale(x))
    ms, med, spread = two_legs(arms, rounds, 'chorale')
    return dict(codes_of_tokens=72, framed_codes=int(framed.shape[1]), tokens=int(x.shape[1] * x.shape[2]), ms=med, spread_ms=spread,
                prior_share=med['prior_half'] / med['score_chorale'], nats_per_token=res['nats_per_token'])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sections', default='score,rows,alone,product,chorale')
    ap.add_argument('--batches', default='1,8,32')
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--codes', type=int, default=96)
    ap.add_argument('--json', default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_prior_score needs the GPU'
    sections = args.sections.split(',')
    batches = [int(b) for b in args.batches.split(',')]
    from vqcpc_bach_amd.priors import scoring
    out = dict(device=torch.cuda.get_device_name(0), rounds=args.rounds, default_window_rows=scoring.WINDOW_ROWS)
    prior = dec = None
    if {'score', 'rows', 'chorale'} & set(sections):
        from bench_prior import build_prior_and_decoder
        prior, dec = build_prior_and_decoder()
        prior.eval(), dec.eval()
        out['shape'] = dict(d_model=prior.d_model, layers=len(prior.transformer.layers), N=prior.num_tokens,
                            V=prior.num_tokens_per_channel[0], num_tokens=args.codes)
    def done(name, result):                            # the file is rewritten after every section
        out[name] = result
        print(json.dumps({name: result}), flush=True)
        if args.json:
            os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
            with open(args.json, 'w') as fh:
                json.dump(out, fh, indent=1)
    if 'score' in sections:
        done('score', section_score(prior, batches, args.rounds, args.codes))
    if 'rows' in sections:
        done('rows', section_rows(prior, batches, args.rounds, args.codes))
    if 'alone' in sections:
        done('alone', section_alone())
    if 'chorale' in sections:
        done('chorale', section_chorale(prior, dec, args.rounds))
    if 'product' in sections:                          # last: the builder selects the training arithmetic for the process
        done('product', section_product(batches, args.rounds, args.codes))


if __name__ == '__main__':
    main()
