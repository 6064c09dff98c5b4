"""What recording the attention maps costs at the DEC shape (d_model 512, 8 heads, 3 + 3 layers, T = 384, S = 24, U = 16), per
batch B in --batches, in ONE process with alternating windows (profiles/generate_attentions_perf_log.md):

  step    us per replayed fixed-window step: the captured step of `IncrementalDecoder.start(want_attentions=...)` replayed T
          times between two device synchronisations.  off: every attention launch is vqcpc_decode_attn (today's step);
          one: decoder layer min(2, layers - 1) calls vqcpc_decode_attn_probs for its self- and cross-attention; all: every layer.
  long    ms per `Decoder.generate_from_code_long` call (B = --long-batch, nb = 2 S codes, every code generated, captures
          included) with return_attentions off and on (every layer).

  --parent-root TREE   the default path against the parent commit: TREE is a checkout of the parent commit with its library
          built in place.  Fresh child processes alternate, parent then this tree, --rounds times; each measures the `off` step
          alone (`--off-only`, which runs on a tree without the new entry point).  Printed per B: the median of each tree's
          windows, the difference, and the spread (maximum - minimum) of the PARENT's own windows -- the margin a difference
          has to exceed.

Printed: every window; per form the median, minimum and maximum over the windows.

    python tools/bench_generate_attentions.py [--batches 1,8,32] [--windows 7] [--json profiles/generate_attentions_bench.json]
                                              [--parent-root TREE --rounds 3]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import torch

FORMS = ('off', 'one', 'all')


def stats(t):
    return dict(median=statistics.median(t), min=min(t), max=max(t))


class Run:
    """The captured step of a fixed-window generation for one form."""

    def __init__(self, dec, B, form):
        from vqcpc_bach_amd.decoders.generation import IncrementalDecoder
        self.T = dec.num_tokens_target
        nl = len(dec.transformer.decoder.layers)
        g = torch.Generator().manual_seed(B)
        codes = torch.randint(0, dec.source_embeddings.weight.shape[0], (B, dec.num_tokens_source), generator=g).cuda()
        extra = {} if form == 'off' else dict(want_attentions=(min(2, nl - 1),) if form == 'one' else tuple(range(nl)))
        self.inc = inc = IncrementalDecoder(dec, B)
        inc.prefill(codes)
        inc.start(seeds=1, temperature=1.0, **extra)
        inc.step()
        self.graph = inc.capture(inc.step)

    def step_window(self):
        self.inc.reset()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(self.T):
            self.graph.replay()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6 / self.T


def long_window(dec, codes, pad, start, on):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    dec.generate_from_code_long(codes, temperature=1.0, seed=1, pad=pad, start=start, return_attentions=on)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def measure(args, forms):
    sys.path.insert(0, args.root)
    sys.path.insert(0, os.path.join(args.root, 'tests'))
    assert torch.cuda.is_available(), 'bench_generate_attentions needs the GPU'
    from oracle import decoder_oracle as D
    from test_decoder_gpu import seeded_decoder
    from vqcpc_bach_amd.utils import STEP_LOCK
    dec, _ = seeded_decoder(D.make_cfg('DEC', B=8), 5)
    dec.eval()
    rows = []
    for B in [int(b) for b in args.batches.split(',')]:
        with STEP_LOCK, torch.no_grad():
            runs = {f: Run(dec, B, f) for f in forms}
            res = dict(batch=B, T=dec.num_tokens_target, S=dec.num_tokens_source, windows=args.windows,
                       device=torch.cuda.get_device_name(0))
            for r in runs.values():
                r.step_window()                                     # warm-up
            times = {f: [] for f in runs}
            for w in range(args.windows):
                for f, r in runs.items():
                    times[f].append(r.step_window())
                    print(f'B={B:2d} step window {w} {f:4s} {times[f][-1]:10.3f} us/step', flush=True)
            res['step_us'] = {f: stats(v) for f, v in times.items()}
            res['step_us_windows'] = times
            for f in forms[1:]:
                res['step_us'][f + '_minus_off'] = res['step_us'][f]['median'] - res['step_us']['off']['median']
            del runs
        rows.append(res)
        print(json.dumps(res), flush=True)
    long = None
    if len(forms) > 1 and args.long_batch > 0:
        S = dec.num_tokens_source
        vocab = [int(v) for v in dec.num_tokens_per_channel]
        pad, start = [v - 1 for v in vocab], [v - 3 for v in vocab]
        g = torch.Generator().manual_seed(99)
        codes = torch.randint(0, dec.source_embeddings.weight.shape[0], (args.long_batch, 2 * S), generator=g).cuda()
        for on in (False, True):
            long_window(dec, codes, pad, start, on)                 # warm-up
        times = {'off': [], 'all': []}
        for w in range(args.long_windows):
            for f, on in (('off', False), ('all', True)):
                times[f].append(long_window(dec, codes, pad, start, on))
                print(f'long B={args.long_batch} nb={2 * S} window {w} {f:4s} {times[f][-1]:10.2f} ms', flush=True)
        long = dict(batch=args.long_batch, nb=2 * S, **{f: stats(v) for f, v in times.items()})
        print(json.dumps(long), flush=True)
    return dict(step=rows, long=long)


def against_parent(args):
    """Alternating fresh processes: the `off` step of the parent tree and of this one."""
    here = os.path.abspath(__file__)
    trees = (('parent', os.path.abspath(args.parent_root)), ('this', args.root))
    windows = {name: {} for name, _ in trees}
    for rnd in range(args.rounds):
        for name, root in trees:
            with tempfile.TemporaryDirectory() as tmp:
                out = os.path.join(tmp, 'off.json')
                subprocess.run([sys.executable, here, '--off-only', '--root', root, '--batches', args.batches, '--windows',
                                str(args.windows), '--json', out], check=True, timeout=600, stdout=subprocess.DEVNULL)
                for r in json.load(open(out))['step']:
                    windows[name].setdefault(r['batch'], []).extend(r['step_us_windows']['off'])
            print(f'round {rnd} {name}: ' + ' '.join(f'B={b} {statistics.median(v):.3f}' for b, v in windows[name].items()), flush=True)
    rows = []
    for b in windows['parent']:
        p, t = stats(windows['parent'][b]), stats(windows['this'][b])
        rows.append(dict(batch=b, parent=p, this=t, this_minus_parent=t['median'] - p['median'], parent_spread=p['max'] - p['min'],
                         windows_per_tree=len(windows['parent'][b])))
        print(json.dumps(rows[-1]), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', default='1,8,32')
    ap.add_argument('--windows', type=int, default=7)
    ap.add_argument('--long-batch', type=int, default=8)
    ap.add_argument('--long-windows', type=int, default=3)
    ap.add_argument('--json', default=None)
    ap.add_argument('--root', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument('--off-only', action='store_true')
    ap.add_argument('--parent-root', default=None)
    ap.add_argument('--rounds', type=int, default=3)
    args = ap.parse_args()
    if args.parent_root:
        result = dict(default_path_against_parent=against_parent(args))
    else:
        result = measure(args, FORMS[:1] if args.off_only else FORMS)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, 'w') as fh:
            json.dump(result, fh, indent=1)


if __name__ == '__main__':
    main()
