"""The masked sampler against the default and the constrained one at the DEC shape (d_model 512, 8 heads, 3 + 3 layers,
T = 384, S = 24, U = 16), per batch B in --batches, in ONE process on the same decoder with alternating windows
(profiles/generate_masked_perf_log.md):

  step    us per replayed fixed-window step: the captured step of `IncrementalDecoder.start(...)` replayed T times between two
          device synchronisations.
  code    us per generated code of a long-form generation (nb = 4 S codes): the captured middle slide and U replayed steps, for
          --codes consecutive middle windows between two synchronisations.

  forms   default, default_again   vqcpc_decode_sample, twice: two identical legs, whose difference is the spread
          constrained              vqcpc_decode_sample_constrained: half of the positions forced, `logp` on
          masked                   vqcpc_decode_sample_masked: the same constraint and `logp`, plus a half-density set at every
                                   position and `allowed_mass` on

Printed: every window; per form the median, minimum and maximum over the windows.

    python tools/bench_generate_masked.py [--batches 1,8,32] [--windows 7] [--json profiles/generate_masked_bench.json]
                                          [--log profiles/generate_masked_perf_log.md] [--parent-json <file>]
    --defaults-only   the two default legs alone: runs on a tree without the masked entry point (--root <tree>)
    --parent-json     the --defaults-only --json of the parent commit's tree, measured in the same session: the log then
                      compares the default legs of the two trees against the spread of the identical legs
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

FORMS = ('default', 'default_again', 'constrained', 'masked')
LEGS = (('step_us', 'replayed fixed-window step, us'), ('code_us', 'long form, us per code (slide + U steps)'))


def stats(t):
    return dict(median=statistics.median(t), min=min(t), max=max(t))


class Run:
    """The captured step of a fixed-window generation and the captured slide + step of a long one, for one form."""

    def __init__(self, dec, B, nb, form):
        from vqcpc_bach_amd.decoders.generation import IncrementalDecoder
        self.T, self.S, self.U = dec.num_tokens_target, dec.num_tokens_source, dec.total_upscaling
        T, S, U, nc = self.T, self.S, self.U, dec.num_channels
        vocab = [int(v) for v in dec.num_tokens_per_channel]
        g = torch.Generator().manual_seed(B)
        codes = torch.randint(0, dec.source_embeddings.weight.shape[0], (B, nb), generator=g).cuda()
        extra, extra_long = {}, {}
        if form in ('constrained', 'masked'):
            given = torch.stack([torch.randint(0, vocab[t % nc], (B,), generator=g) for t in range(nb * U)], dim=1)
            cons = torch.where(torch.rand(B, nb * U, generator=g) < 0.5, given, torch.full_like(given, -1)).cuda()
            extra = dict(constraint=cons[:, :T].contiguous(), want_logp=True)
            extra_long = dict(constraint=cons, want_logp=True)
        if form == 'masked':
            events, vmax = nb * U // nc, max(vocab)
            allowed = torch.rand(B, events, nc, vmax, generator=g) < 0.5
            allowed.scatter_(3, given.view(B, events, nc, 1), True)           # every set holds a token, the forced one included
            words = dec._allowed_words(allowed, B, events, constraint=cons)   # (B, nb * U, 8), validated
            extra.update(allowed=words[:, :T].contiguous(), want_allowed_mass=True)
            extra_long.update(allowed=words, want_allowed_mass=True)
        self.inc = inc = IncrementalDecoder(dec, B)
        inc.prefill(codes[:, :S])
        inc.start(seeds=1, temperature=1.0, **extra)
        inc.step()
        self.step_graph = inc.capture(inc.step)
        self.long = lng = IncrementalDecoder(dec, B)
        pad, start = [v - 1 for v in vocab], [v - 3 for v in vocab]
        chorale = dec.init_generation_chorale(nb * U // nc, 0, pad=pad, start=start).reshape(1, -1).expand(B, -1)
        lng.start_long(codes, chorale, seeds=1, temperature=1.0, **extra_long)
        lng.slide(0, S // 2)
        lng.step()
        self.long_step = lng.capture(lng.step)
        lng.slide(0, S // 2)
        self.long_slide = lng.capture(lambda: lng.slide(None, S // 2, advance=1))

    def step_window(self):
        self.inc.reset()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(self.T):
            self.step_graph.replay()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6 / self.T

    def code_window(self, codes):
        self.long.win.copy_(torch.tensor([0, -1], dtype=torch.int32))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(codes):
            self.long_slide.replay()
            for _ in range(self.U):
                self.long_step.replay()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6 / codes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', default='1,8,32')
    ap.add_argument('--windows', type=int, default=7)
    ap.add_argument('--codes', type=int, default=24, help='middle windows per long-form timing window')
    ap.add_argument('--json', default=None)
    ap.add_argument('--log', default=None)
    ap.add_argument('--parent-json', default=None)
    ap.add_argument('--root', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument('--defaults-only', action='store_true')
    args = ap.parse_args()
    sys.path.insert(0, args.root)
    sys.path.insert(0, os.path.join(args.root, 'tests'))
    assert torch.cuda.is_available(), 'bench_generate_masked needs the GPU'
    from oracle import decoder_oracle as D
    from test_decoder_gpu import seeded_decoder
    from vqcpc_bach_amd.utils import STEP_LOCK
    dec, _ = seeded_decoder(D.make_cfg('DEC', B=8), 5)
    dec.eval()
    S = dec.num_tokens_source
    nb = 4 * S
    assert args.codes <= nb - S, 'every slide of a window must find a whole model window'
    forms = FORMS[:2] if args.defaults_only else FORMS
    rows = []
    for B in [int(b) for b in args.batches.split(',')]:
        with STEP_LOCK, torch.no_grad():
            runs = {f: Run(dec, B, nb, f) for f in forms}
            res = dict(batch=B, nb=nb, T=dec.num_tokens_target, U=dec.total_upscaling, windows=args.windows,
                       codes_per_window=args.codes, device=torch.cuda.get_device_name(0))
            for key, fn, unit in (('step_us', lambda r: r.step_window(), 'us/step'),
                                  ('code_us', lambda r: r.code_window(args.codes), 'us/code')):
                for r in runs.values():
                    fn(r)                                           # warm-up
                times = {f: [] for f in runs}
                for w in range(args.windows):
                    for f, r in runs.items():
                        times[f].append(fn(r))
                        print(f'B={B:2d} {key:8s} window {w} {f:13s} {times[f][-1]:10.3f} {unit}', flush=True)
                res[key] = {f: stats(v) for f, v in times.items()}
                d0, d1 = res[key]['default'], res[key]['default_again']
                # what two identical legs differ by: between their medians, and from window to window inside either
                res[key]['spread'] = max(abs(d0['median'] - d1['median']), d0['max'] - d0['min'], d1['max'] - d1['min'])
                if not args.defaults_only:
                    res[key]['constrained_minus_default'] = res[key]['constrained']['median'] - d0['median']
                    res[key]['masked_minus_constrained'] = res[key]['masked']['median'] - res[key]['constrained']['median']
            del runs
        rows.append(res)
        print(json.dumps(res), flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, 'w') as fh:
            json.dump(rows, fh, indent=1)
    if args.log:
        parent = json.load(open(args.parent_json)) if args.parent_json else None
        with open(args.log, 'w') as fh:
            fh.write(markdown(rows, forms, parent))


def markdown(rows, forms, parent=None):
    cell = lambda s: f'{s["median"]:.3f} ({s["min"]:.3f} .. {s["max"]:.3f})'
    out = ['# Masked sampler: replayed step and long-form code at the DEC shape', '',
           f'Measured by `tools/bench_generate_masked.py` on {rows[0]["device"]}: one process, one decoder, alternating windows, '
           f'{rows[0]["windows"]} windows per form; median (minimum .. maximum).  default and default_again are the same leg twice; '
           'spread = the larger of the difference of their medians and of either one\'s maximum - minimum.  constrained = half of '
           'the positions forced, `logp` on; masked = the same plus a half-density set at every position and `allowed_mass` on.  '
           f'A long-form window is {rows[0]["codes_per_window"]} consecutive middle codes of nb = {rows[0]["nb"]}.', '']
    extra = len(forms) > 2
    for key, title in LEGS:
        out += [f'## {title}', '', '| B | ' + ' | '.join(forms) + ' | spread |' +
                (' constrained - default | masked - constrained |' if extra else ''),
                '|---|' + '---|' * (len(forms) + (3 if extra else 1))]
        for r in rows:
            cells = [cell(r[key][f]) for f in forms] + [f'{r[key]["spread"]:.3f}']
            if extra:
                cells += [f'{r[key]["constrained_minus_default"]:+.3f}', f'{r[key]["masked_minus_constrained"]:+.3f}']
            out.append(f'| {r["batch"]} | ' + ' | '.join(cells) + ' |')
        out.append('')
    if parent is not None:
        out += ['## The default legs against the parent commit', '',
                'The parent commit\'s tree (its own library) ran `--defaults-only` as a separate process in the same session.  '
                'Condition: this tree\'s default median is not above the parent\'s by more than the spread of the identical '
                'legs (the larger of the two processes\' spreads).', '',
                '| B | leg | parent default | parent default_again | this tree default | this tree default_again | '
                'this - parent | spread | within |', '|---|---|---|---|---|---|---|---|---|']
        for r, p in zip(rows, parent):
            assert r['batch'] == p['batch']
            for key, _ in LEGS:
                diff = r[key]['default']['median'] - p[key]['default']['median']
                spread = max(r[key]['spread'], p[key]['spread'])
                out.append(f'| {r["batch"]} | {key} | {cell(p[key]["default"])} | {cell(p[key]["default_again"])} | '
                           f'{cell(r[key]["default"])} | {cell(r[key]["default_again"])} | {diff:+.3f} | {spread:.3f} | '
                           f'{"yes" if diff <= spread else "NO"} |')
        out.append('')
    return '\n'.join(out)


if __name__ == '__main__':
    main()
