"""The constrained sampler against the plain one at the DEC shape (d_model 512, 8 heads, 3 + 3 layers, T = 384, S = 24,
U = 16), per batch B in --batches, in ONE process with alternating windows (profiles/generate_constrained_perf_log.md):

  step    us per replayed fixed-window step: the captured step of `IncrementalDecoder.start(...)` replayed T times between two
          device synchronisations.  plain: vqcpc_decode_sample; constrained: vqcpc_decode_sample_constrained with half of the
          positions forced and `logp` on.
  code    us per generated code of a long-form generation (nb = 4 S codes): the captured middle slide and U replayed steps, for
          --codes consecutive middle windows between two synchronisations, in both forms.  The constrained form reads its
          constraint and writes logp at chorale columns through the device window index.
  slide   ms per replayed middle slide alone.  The slide launches no sampler, so both forms replay the same kernels: the
          difference between the two columns is noise, and is printed as such.

Printed: every window; per form the median, minimum and maximum over the windows -- the spread a difference has to exceed.

    python tools/bench_generate_constrained.py [--batches 1,8,32] [--windows 7] [--json profiles/generate_constrained_bench.json]
                                               [--log profiles/generate_constrained_perf_log.md]
    --plain-only   measure the plain form alone (runs on a tree without the constrained entry point: --root <tree>)
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

FORMS = ('plain', 'constrained')


def stats(t):
    return dict(median=statistics.median(t), min=min(t), max=max(t))


class Run:
    """The captured step of a fixed-window generation and the captured slide + step of a long one, for one form."""

    def __init__(self, dec, B, nb, constrained):
        from vqcpc_bach_amd.decoders.generation import IncrementalDecoder
        self.T, self.S, self.U = dec.num_tokens_target, dec.num_tokens_source, dec.total_upscaling
        T, S, U, nc = self.T, self.S, self.U, dec.num_channels
        vocab = [int(v) for v in dec.num_tokens_per_channel]
        g = torch.Generator().manual_seed(B)
        codes = torch.randint(0, dec.source_embeddings.weight.shape[0], (B, nb), generator=g).cuda()
        extra, extra_long = {}, {}
        if constrained:
            given = torch.stack([torch.randint(0, vocab[t % nc], (B,), generator=g) for t in range(nb * U)], dim=1)
            cons = torch.where(torch.rand(B, nb * U, generator=g) < 0.5, given, torch.full_like(given, -1)).cuda()
            extra = dict(constraint=cons[:, :T].contiguous(), want_logp=True)
            extra_long = dict(constraint=cons, want_logp=True)
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

    def _rewind(self):
        self.long.win.copy_(torch.tensor([0, -1], dtype=torch.int32))
        torch.cuda.synchronize()

    def code_window(self, codes):
        self._rewind()
        t0 = time.perf_counter()
        for _ in range(codes):
            self.long_slide.replay()
            for _ in range(self.U):
                self.long_step.replay()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6 / codes

    def slide_window(self, codes):
        self._rewind()
        t0 = time.perf_counter()
        for _ in range(codes):
            self.long_slide.replay()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / codes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', default='1,8,32')
    ap.add_argument('--windows', type=int, default=7)
    ap.add_argument('--codes', type=int, default=24, help='middle windows per long-form timing window')
    ap.add_argument('--json', default=None)
    ap.add_argument('--log', default=None)
    ap.add_argument('--root', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument('--plain-only', action='store_true')
    args = ap.parse_args()
    sys.path.insert(0, args.root)
    sys.path.insert(0, os.path.join(args.root, 'tests'))
    assert torch.cuda.is_available(), 'bench_generate_constrained needs the GPU'
    from oracle import decoder_oracle as D
    from test_decoder_gpu import seeded_decoder
    from vqcpc_bach_amd.utils import STEP_LOCK
    dec, _ = seeded_decoder(D.make_cfg('DEC', B=8), 5)
    dec.eval()
    S = dec.num_tokens_source
    nb = 4 * S
    assert args.codes <= nb - S, 'every slide of a window must find a whole model window'
    forms = FORMS[:1] if args.plain_only else FORMS
    rows = []
    for B in [int(b) for b in args.batches.split(',')]:
        with STEP_LOCK, torch.no_grad():
            runs = {f: Run(dec, B, nb, f == 'constrained') for f in forms}
            res = dict(batch=B, nb=nb, T=dec.num_tokens_target, U=dec.total_upscaling, windows=args.windows,
                       codes_per_window=args.codes, device=torch.cuda.get_device_name(0))
            for key, fn, unit in (('step_us', lambda r: r.step_window(), 'us/step'),
                                  ('code_us', lambda r: r.code_window(args.codes), 'us/code'),
                                  ('slide_ms', lambda r: r.slide_window(args.codes), 'ms/slide')):
                for r in runs.values():
                    fn(r)                                           # warm-up
                times = {f: [] for f in runs}
                for w in range(args.windows):
                    for f, r in runs.items():
                        times[f].append(fn(r))
                        print(f'B={B:2d} {key:8s} window {w} {f:11s} {times[f][-1]:10.3f} {unit}', flush=True)
                res[key] = {f: stats(v) for f, v in times.items()}
            if not args.plain_only:
                for key in ('step_us', 'code_us', 'slide_ms'):
                    p, c = res[key]['plain'], res[key]['constrained']
                    res[key]['constrained_minus_plain'] = c['median'] - p['median']
                    res[key]['spread'] = max(p['max'] - p['min'], c['max'] - c['min'])
            del runs
        rows.append(res)
        print(json.dumps(res), flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, 'w') as fh:
            json.dump(rows, fh, indent=1)
    if args.log:
        with open(args.log, 'w') as fh:
            fh.write(markdown(rows, forms))


def markdown(rows, forms):
    out = ['# Constrained sampler: replayed step, long-form code and slide at the DEC shape', '',
           f'Measured by `tools/bench_generate_constrained.py` on {rows[0]["device"]}: one process, alternating windows, '
           f'{rows[0]["windows"]} windows per form; median (minimum .. maximum).  constrained = half of the positions forced, '
           '`logp` on.  A long-form window is ' f'{rows[0]["codes_per_window"]} consecutive middle codes of nb = {rows[0]["nb"]}.', '']
    for key, title in (('step_us', 'replayed fixed-window step, us'), ('code_us', 'long form, us per code (slide + U steps)'),
                       ('slide_ms', 'replayed middle slide alone, ms (no sampler in it: the two columns replay the same kernels)')):
        out += [f'## {title}', '', '| B | ' + ' | '.join(forms) + (' | constrained - plain | largest spread |' if len(forms) > 1 else ' |'),
                '|---|' + '---|' * (len(forms) + (2 if len(forms) > 1 else 0))]
        for r in rows:
            cells = [f'{r[key][f]["median"]:.3f} ({r[key][f]["min"]:.3f} .. {r[key][f]["max"]:.3f})' for f in forms]
            if len(forms) > 1:
                cells += [f'{r[key]["constrained_minus_plain"]:+.3f}', f'{r[key]["spread"]:.3f}']
            out.append(f'| {r["batch"]} | ' + ' | '.join(cells) + ' |')
        out.append('')
    return '\n'.join(out)


if __name__ == '__main__':
    main()
