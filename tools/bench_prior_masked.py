"""What allowed code sets and particle resampling cost in the prior's generation, at the PRI shape (tools/bench_prior.py: d_model
512, 8 heads, 6 layers, ff 1024, N = 24 codes per window, V = 32), per batch B in --batches, in ONE process with alternating timing
windows and two identical legs (a, b) per arm for the spread (profiles/generate_prior_masked_perf_log.md):

  step      us per code of the replayed cached step with the plain / constrained / masked-with-mass sampler
  move      us per code of the forward-form move (window kernel + stack over the window + head row + sampler), the same three
  product   both of the above on a 2 x 64 product prior (tools/bench_product_codes.py): per stage one head and one sampler launch
  plan      96 codes with the last 8 forced: `particles=8` over 64 rows (8 groups; and 64 groups of 8 = 512 rows) against
            `num_generated_codes=64` ranked by logp; the log-probability of the forced close given the plan before it
  defaults  ms of the default `generate_codes` (96 codes), two identical legs, in a process of its own: --defaults-only.
            --root TREE imports the package from another checkout (the parent commit's, with its library built in place): fresh
            processes of the two trees alternate (parent, this tree, parent), --parent-json A,B and --this-json put their figures
            into the log.  --render writes the log from an existing --json without measuring.

    timeout -k 10 900 python tools/bench_prior_masked.py [--sections step,move,product,plan] [--batches 1,8,32] [--rounds 5]
                                  [--json FILE] [--log profiles/generate_prior_masked_perf_log.md]
                                  [--defaults-only [--root TREE]] [--parent-json A,B --this-json FILE] [--render]

Every invocation is one GPU step: run it under its own `timeout`, as above.  Device-synchronised host clocks, warm-up first."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def two_legs(arms, rounds, per=1.0, label=''):
    """arms: {name: fn}.  One warm-up of each, then `rounds` rounds of a-arm..., b-arm... -> ({arm: median over both legs},
    {arm: (median a, median b)}, spread = the largest |median(a) - median(b)|), in the unit ms / per."""
    for fn in arms.values():
        fn()
    times = {(k, leg): [] for leg in 'ab' for k in arms}
    for _ in range(rounds):
        for leg in 'ab':
            for k, fn in arms.items():
                times[k, leg].append(timed(fn) * 1e3 / per)
    legs = {k: (statistics.median(times[k, 'a']), statistics.median(times[k, 'b'])) for k in arms}
    med = {k: statistics.median(times[k, 'a'] + times[k, 'b']) for k in arms}
    spread = max(abs(a - b) for a, b in legs.values())
    print(f'{label} ' + ', '.join(f'{k} {v:.4g}' for k, v in med.items()) + f', spread {spread:.3g}', flush=True)
    return med, legs, spread


def sampler_stacks(prior, B, nt, product):
    """Three started stacks of B rows that differ in the sampler alone: plain, constrained (nothing forced, logp kept), masked
    (random sets of half the codes, logp and mass kept)."""
    from vqcpc_bach_amd.priors.code_sets import pack_sets
    from vqcpc_bach_amd.priors.generation import IncrementalPrior, IncrementalProductPrior
    cls = IncrementalProductPrior if product else IncrementalPrior
    g = torch.Generator().manual_seed(B)
    shape = (B, nt, prior.num_codebooks, prior.codebook_size) if product else (B, nt, prior.num_tokens_per_channel[0])
    allowed = torch.rand(shape, generator=g) < 0.5
    allowed[..., 0] = True
    free = torch.full((B, nt), -1, dtype=torch.int64)
    stacks = {}
    for name, kw in (('plain', dict()), ('constrained', dict(constraint=free, want_logp=True)),
                     ('masked', dict(constraint=free, want_logp=True, allowed=pack_sets(allowed.cuda()), want_allowed_mass=True))):
        inc = cls(prior, B)
        inc.start(nt, seeds=1, **kw)
        stacks[name] = inc
    return stacks


def section_step_move(prior, batches, rounds, nt, product=False):
    from vqcpc_bach_amd.utils import STEP_LOCK
    N = prior.num_tokens
    rows = []
    for B in batches:
        with STEP_LOCK, torch.no_grad():
            stacks = sampler_stacks(prior, B, nt, product)
            graphs = {}
            for name, inc in stacks.items():
                inc.step()
                graphs[name] = inc.capture(inc.step)
            passes = 8

            def head(name):
                inc, graph = stacks[name], graphs[name]
                for _ in range(passes):
                    inc.pos.zero_()
                    for _ in range(N):
                        graph.replay()

            def move(name):
                inc = stacks[name]
                for i in range(64):
                    inc.win[0:1].fill_(1 + i % 8)
                    inc._move_forward()
            step, step_legs, step_spread = two_legs({k: (lambda k=k: head(k)) for k in stacks}, rounds, passes * N / 1e3,
                                                    f'step us/code B={B:2d}')
            mv, mv_legs, mv_spread = two_legs({k: (lambda k=k: move(k)) for k in stacks}, rounds, 64 / 1e3, f'move us/code B={B:2d}')
            rows.append(dict(batch=B, step_us=step, step_legs_us=step_legs, step_spread_us=step_spread, move_us=mv,
                             move_legs_us=mv_legs, move_spread_us=mv_spread))
            del graphs, stacks
    return rows


def section_plan(prior, rounds, nt, forced=8, P=8):
    V = prior.num_tokens_per_channel[0]
    g = torch.Generator().manual_seed(11)
    cons = torch.full((1, nt), -1, dtype=torch.int64)
    cons[0, nt - forced:] = torch.randint(0, V, (forced,), generator=g)
    arms = dict(ranked64=lambda: prior.generate_codes(nt, num_generated_codes=64, seed=3, constraint=cons, return_logp=True),
                particles8_rows64=lambda: prior.generate_codes(nt, num_generated_codes=64 // P, seed=3, constraint=cons, particles=P,
                                                               return_logp=True),
                particles8_groups64=lambda: prior.generate_codes(nt, num_generated_codes=64, seed=3, constraint=cons, particles=P,
                                                                 return_logp=True))
    med, legs, spread = two_legs(arms, rounds, 1.0, 'plan ms')
    close = slice(nt - forced, nt)
    quality = {}
    for k, fn in arms.items():                              # what the forced close costs: its log-probability given the plan before it
        lp = fn()[1][:, close].double().sum(dim=1)
        quality[k] = dict(rows=int(lp.numel()), mean_close_logp=float(lp.mean()), best_close_logp=float(lp.max()))
    return dict(codes=nt, forced_last=forced, particles=P, ms=med, legs_ms=legs, spread_ms=spread, close=quality)


def section_defaults(prior, batches, rounds, nt):
    rows = []
    for B in batches:
        arm = lambda: prior.generate_codes(nt, num_generated_codes=B, seed=1)          # noqa: E731
        med, legs, spread = two_legs(dict(default=arm), rounds, 1.0, f'default generate_codes ms B={B:2d}')
        rows.append(dict(batch=B, ms=med['default'], legs_ms=legs['default'], spread_ms=spread))
    return rows


def markdown(out, parents=(), this=None):
    L = ['# Allowed code sets and particle resampling in the prior: what they cost', '',
         f"Device {out['device']}; tools/bench_prior_masked.py, {out['rounds']} rounds, two identical legs per arm, alternating windows; "
         'the spread is the largest |median(a) - median(b)| over the arms of a row.', '']

    def table(title, rows, key, unit):
        L.extend([f'## {title}', '', f'| B | plain {unit} | constrained {unit} | masked + mass {unit} | masked - constrained | spread |',
                  '|---|---|---|---|---|---|'])
        for r in rows:
            v = r[f'{key}_us']
            L.append(f"| {r['batch']} | {v['plain']:.1f} | {v['constrained']:.1f} | {v['masked']:.1f} | "
                     f"{v['masked'] - v['constrained']:+.1f} | {r[f'{key}_spread_us']:.1f} |")
        L.append('')
    for name, tag in (('pri', 'PRI shape, V = 32'), ('product', '2 x 64 product prior')):
        if name in out:
            table(f'The replayed cached step, {tag}', out[name], 'step', 'us/code')
            table(f'The forward-form move, {tag}', out[name], 'move', 'us/code')
    if 'plan' in out:
        p = out['plan']
        L.extend([f"## {p['codes']} codes with the last {p['forced_last']} forced", '',
                  '| arm | ms | rows returned | mean logp of the forced close | best |', '|---|---|---|---|---|'])
        for k, v in p['ms'].items():
            q = p['close'][k]
            L.append(f"| {k} | {v:.1f} | {q['rows']} | {q['mean_close_logp']:.2f} | {q['best_close_logp']:.2f} |")
        L.extend(['', f"Spread {p['spread_ms']:.2f} ms.  `ranked64`: 64 plain rows, the caller ranks them by logp; `particles8_rows64`: "
                  '8 groups of 8 particles (64 rows of the stack, 8 plans returned); `particles8_groups64`: 64 groups (512 rows, 64 plans).', ''])
    if parents and this is not None:
        L.extend(['## The default `generate_codes` (no new keyword) against the parent commit', '',
                  'Fresh processes of `--defaults-only`, in the order parent, this tree, parent; the parent commit\'s tree has its own '
                  'library.  Two identical legs per process.  Condition: this tree\'s legs lie inside the range of the parent\'s legs, '
                  'or below it.', '',
                  '| B | parent legs ms (process 1; process 2) | this tree\'s legs ms | parent range | inside or below |', '|---|---|---|---|---|'])
        for i, r in enumerate(this['defaults']):
            legs = [t for q in parents for t in q['defaults'][i]['legs_ms']]
            ok = all(t <= max(legs) for t in r['legs_ms'])
            L.append(f"| {r['batch']} | " + '; '.join(', '.join(f'{t:.2f}' for t in q['defaults'][i]['legs_ms']) for q in parents) +
                     f" | {r['legs_ms'][0]:.2f}, {r['legs_ms'][1]:.2f} | {min(legs):.2f} .. {max(legs):.2f} | {'yes' if ok else 'NO'} |")
        L.append('')
    return '\n'.join(L)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sections', default='step,move,product,plan')
    ap.add_argument('--batches', default='1,8,32')
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--codes', type=int, default=96)
    ap.add_argument('--defaults-only', action='store_true')
    ap.add_argument('--root', default=HERE)
    ap.add_argument('--json', default=None)
    ap.add_argument('--log', default=None)
    ap.add_argument('--parent-json', default=None)
    ap.add_argument('--this-json', default=None)
    ap.add_argument('--render', action='store_true')
    args = ap.parse_args()
    if args.render:
        write_log(args, json.load(open(args.json)))
        return
    root = os.path.abspath(args.root)
    for p in (os.path.join(root, 'tools'), os.path.join(root, 'tests'), root):
        sys.path.insert(0, p)
    assert torch.cuda.is_available(), 'bench_prior_masked needs the GPU'
    sections = ['defaults'] if args.defaults_only else args.sections.split(',')
    batches = [int(b) for b in args.batches.split(',')]
    out = dict(device=torch.cuda.get_device_name(0), rounds=args.rounds, root=os.path.basename(root))
    from bench_prior import build_prior_and_decoder
    prior, _ = build_prior_and_decoder()
    prior.eval()
    if 'step' in sections or 'move' in sections:
        out['pri'] = section_step_move(prior, batches, args.rounds, args.codes)
    if 'plan' in sections:
        out['plan'] = section_plan(prior, args.rounds, args.codes)
    if 'defaults' in sections:
        out['defaults'] = section_defaults(prior, batches, args.rounds, args.codes)
    if 'product' in sections:                              # last: the builder selects the training arithmetic for the process
        from bench_product_codes import build_prior
        prod, _ = build_prior(64, 2, 'product', seed=6)
        prod.eval()
        out['product'] = section_step_move(prod, batches, args.rounds, args.codes, product=True)
    print(json.dumps(out), flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, 'w') as fh:
            json.dump(out, fh, indent=1)
    write_log(args, out)


def write_log(args, out):
    if args.log:
        parents = [json.load(open(f)) for f in args.parent_json.split(',')] if args.parent_json else ()
        this = json.load(open(args.this_json)) if args.this_json else None
        with open(args.log, 'w') as fh:
            fh.write(markdown(out, parents, this))


if __name__ == '__main__':
    main()
