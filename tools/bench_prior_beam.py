"""What beam search over code plans costs in the prior's generation, at the PRI shape (tools/bench_prior.py: d_model 512, 8 heads,
6 layers, ff 1024, N = 24 codes per window, V = 32) on 64 rows of the stack, in ONE process with alternating timing windows and two
identical legs (a, b) per arm for the spread (profiles/generate_prior_beam_perf_log.md):

  step      us per code of the replayed cached step: 64 plain (sampled) rows against beam = 4 / 16 / 64 over the same 64 rows
  move      us per code of the forward-form move (window kernel + stack over the window + head row + tail), the same arms
  parts     us per launch of the beam's own launches, each alone in a replayed graph of N of them: the expansion, the select,
            the two K/V cache moves (every row of a group moved: a rotation of the group)
  plan      ms for 96 codes with beam = 4 / 16 against `num_generated_codes = W` sampled rows
  product   step and move on a 2 x 512 product prior (tools/bench_product_codes.py): a pair of launches per digit stage
  defaults  ms of the default `generate_codes` (96 codes), two identical legs, in a process of its own: --defaults-only.
            --root TREE imports the package from another checkout (the parent commit's, with its library built in place): fresh
            processes of the two trees alternate (parent, this tree, parent), --parent-json A,B and --this-json put their figures
            into the log.  --render writes the log from an existing --json without measuring.

    timeout -k 10 900 python tools/bench_prior_beam.py [--sections step,move,parts,plan,product] [--rounds 5] [--json FILE]
                                  [--log profiles/generate_prior_beam_perf_log.md] [--notes FILE]
                                  [--defaults-only [--root TREE]] [--parent-json A,B --this-json FILE] [--render]

Every invocation is one GPU step: run it under its own `timeout`, as above.  Device-synchronised host clocks, warm-up first.
--notes FILE: markdown appended to the log as it is (what was not measured by this tool: code-object sizes, mutations, tests)."""
import argparse
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(HERE, 'tools'))
from bench_prior_masked import two_legs  # noqa: E402

ROWS = 64
WIDTHS = (4, 16, 64)


def stacks_of(prior, nt, product):
    """Started stacks of 64 rows: plain sampling, and a beam of every width."""
    from vqcpc_bach_amd.priors.generation import IncrementalPrior, IncrementalProductPrior
    cls = IncrementalProductPrior if product else IncrementalPrior
    stacks = {}
    for name, kw in [('plain', dict())] + [(f'beam{W}', dict(beam=W)) for W in WIDTHS]:
        inc = cls(prior, ROWS)
        inc.start(nt, seeds=1, **kw)
        stacks[name] = inc
    return stacks


def section_step_move(prior, rounds, nt, product=False):
    from vqcpc_bach_amd.utils import STEP_LOCK
    N = prior.num_tokens
    with STEP_LOCK, torch.no_grad():
        stacks = stacks_of(prior, nt, product)
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
        step, step_legs, step_spread = two_legs({k: (lambda k=k: head(k)) for k in stacks}, rounds, passes * N / 1e3, 'step us/code')
        mv, mv_legs, mv_spread = two_legs({k: (lambda k=k: move(k)) for k in stacks}, rounds, 64 / 1e3, 'move us/code')
        out = dict(rows=ROWS, step_us=step, step_legs_us=step_legs, step_spread_us=step_spread, move_us=mv, move_legs_us=mv_legs,
                   move_spread_us=mv_spread)
        if not product:
            out['parts'] = section_parts(stacks, rounds)
        del graphs, stacks
    return out


def section_parts(stacks, rounds):
    """The beam's launches alone, N of each in one replayed graph."""
    from vqcpc_bach_amd import hip
    rows = {}
    for W in WIDTHS:
        inc = stacks[f'beam{W}']
        N, nt, M, V = inc.N, inc.nt, inc.M, inc.V
        scratch = (inc.b_cand, inc.b_code, inc.b_lp, inc.b_mass, inc.b_low, inc.b_lowlp)
        inc.logits.normal_()
        inc.b_score.zero_()

        def expand():
            hip.call('vqcpc_prior_beam_expand', inc.logits, V, V, M, W, inc.constraint, nt, inc.allowed, nt, inc.win, inc.b_score, N,
                     inc.pos, *scratch, None)

        def select():
            hip.call('vqcpc_prior_beam_select', *scratch, V, M, W, inc.logp, nt, inc.logmass, nt, inc.win, inc.codes_win, N, N,
                     inc.table, inc.table.shape[0], inc.d, inc.x, inc.d, inc.b_score, inc.b_anc, inc.b_flag, inc.b_bound, inc.b_hist,
                     nt, inc.pos)

        def caches():
            for cache in (inc.kcache, inc.vcache):
                hip.call('vqcpc_particle_permute_cache', cache, len(inc.layers), inc.W, inc.d, inc.pos, inc.b_anc, inc.b_flag, M, W)

        def n_expands():
            inc.pos.zero_()
            for _ in range(N):
                expand()

        def n_selects():                                      # every select advances pos: N of them walk the window
            inc.pos.zero_()
            for _ in range(N):
                select()

        def n_cache_moves():
            inc.pos.fill_(N // 2)                             # half a window of cache rows
            for _ in range(N):
                caches()
        inc.pos.zero_()
        expand()
        arms = {}
        for name, fn in (('expand', n_expands), ('select', n_selects), ('cache_moves', n_cache_moves)):
            if name == 'cache_moves':
                if W == 1:
                    continue
                rot = torch.arange(M, dtype=torch.int32).view(M // W, W).roll(1, dims=1).reshape(-1).cuda()
                setup = lambda rot=rot: (inc.b_anc.copy_(rot), inc.b_flag.fill_(1))         # noqa: E731
            else:
                setup = lambda: None                                                        # noqa: E731
            setup()
            fn()
            setup()
            graph = inc.capture(fn)
            arms[name] = (lambda graph=graph, setup=setup: (setup(), graph.replay()))
        med, legs, spread = two_legs(arms, rounds, N / 1e3, f'parts W={W} us/launch')
        rows[str(W)] = dict(us=med, legs_us=legs, spread_us=spread)
        inc.reset()
    return rows


def section_plan(prior, rounds, nt):
    arms = {}
    for W in (4, 16):
        arms[f'beam{W}'] = lambda W=W: prior.generate_codes(nt, beam=W, return_beams=True, return_logp=True)
        arms[f'sampled{W}'] = lambda W=W: prior.generate_codes(nt, num_generated_codes=W, seed=3, return_logp=True)
    med, legs, spread = two_legs(arms, rounds, 1.0, 'plan ms')
    quality = {}
    for k, fn in arms.items():                              # the total log-probability of the best plan each arm returns
        lp = fn()[1].double().sum(dim=1)
        quality[k] = dict(rows=int(lp.numel()), best_total_logp=float(lp.max()), mean_total_logp=float(lp.mean()))
    return dict(codes=nt, ms=med, legs_ms=legs, spread_ms=spread, totals=quality)


def section_defaults(prior, rounds, nt):
    rows = []
    for B in (1, 8, 32):
        arm = lambda: prior.generate_codes(nt, num_generated_codes=B, seed=1)          # noqa: E731
        med, legs, spread = two_legs(dict(default=arm), rounds, 1.0, f'default generate_codes ms B={B:2d}')
        rows.append(dict(batch=B, ms=med['default'], legs_ms=legs['default'], spread_ms=spread))
    return rows


def markdown(out, parents=(), this=None, notes=''):
    L = ['# Beam search over code plans in the prior: what it costs', '',
         f"Device {out['device']}; tools/bench_prior_beam.py, {out['rounds']} rounds, two identical legs per arm, alternating windows; "
         'the spread is the largest |median(a) - median(b)| over the arms of a row.  64 rows of the stack in every arm: 64 sampled '
         'rows, or 64 / W groups of W hypotheses.', '']

    def table(title, sec, key):
        v = sec[f'{key}_us']
        L.extend([f'## {title}', '', '| arm | us/code | over the plain rows | share of the step it rides on |', '|---|---|---|---|'])
        for k, t in v.items():
            L.append(f"| {k} | {t:.1f} | {t - v['plain']:+.1f} | {100 * (t - v['plain']) / v['plain']:+.1f} % |")
        L.extend(['', f"Spread {sec[f'{key}_spread_us']:.2f} us.", ''])
    for name, tag in (('pri', 'PRI shape, V = 32'), ('product', '2 x 512 product prior (two stages: two pairs of launches per code)')):
        if name in out:
            table(f'The replayed cached step, {tag}', out[name], 'step')
            table(f'The forward-form move, {tag}', out[name], 'move')
    parts = out.get('pri', {}).get('parts')
    if parts:
        L.extend(['## The beam\'s launches alone (PRI shape, V = 32, 64 rows; N = 24 of each in one replayed graph)', '',
                  '| W | expand us | select us | both cache moves us (12 of 24 cache rows, every row moved) | spread |', '|---|---|---|---|---|'])
        for W, r in parts.items():
            u = r['us']
            L.append(f"| {W} | {u['expand']:.1f} | {u['select']:.1f} | {u.get('cache_moves', float('nan')):.1f} | {r['spread_us']:.2f} |")
        L.append('')
    if 'plan' in out:
        p = out['plan']
        L.extend([f"## {p['codes']} codes: a beam against as many sampled rows", '',
                  '| arm | ms | rows | best total logp | mean total logp |', '|---|---|---|---|---|'])
        for k, v in p['ms'].items():
            q = p['totals'][k]
            L.append(f"| {k} | {v:.1f} | {q['rows']} | {q['best_total_logp']:.2f} | {q['mean_total_logp']:.2f} |")
        L.extend(['', f"Spread {p['spread_ms']:.2f} ms.  `beamW`: one group of W hypotheses, all W returned; `sampledW`: "
                  '`num_generated_codes=W` at temperature 1.', ''])
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
    if notes:
        L.append(notes.rstrip('\n'))
        L.append('')
    return '\n'.join(L)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sections', default='step,move,parts,plan,product')
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--codes', type=int, default=96)
    ap.add_argument('--defaults-only', action='store_true')
    ap.add_argument('--root', default=HERE)
    ap.add_argument('--json', default=None)
    ap.add_argument('--log', default=None)
    ap.add_argument('--notes', default=None)
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
    assert torch.cuda.is_available(), 'bench_prior_beam needs the GPU'
    sections = ['defaults'] if args.defaults_only else args.sections.split(',')
    out = dict(device=torch.cuda.get_device_name(0), rounds=args.rounds, root=os.path.basename(root))
    from bench_prior import build_prior_and_decoder
    prior, _ = build_prior_and_decoder()
    prior.eval()
    if 'step' in sections or 'move' in sections or 'parts' in sections:
        out['pri'] = section_step_move(prior, args.rounds, args.codes)
    if 'plan' in sections:
        out['plan'] = section_plan(prior, args.rounds, args.codes)
    if 'defaults' in sections:
        out['defaults'] = section_defaults(prior, args.rounds, args.codes)
    if 'product' in sections:                              # last: the builder selects the training arithmetic for the process
        from bench_product_codes import build_prior
        prod, _ = build_prior(512, 2, 'product', seed=6)
        prod.eval()
        out['product'] = section_step_move(prod, args.rounds, args.codes, product=True)
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
        notes = open(args.notes).read() if args.notes else ''
        with open(args.log, 'w') as fh:
            fh.write(markdown(out, parents, this, notes))


if __name__ == '__main__':
    main()
