"""Launch trace of the decoder's and the prior's generation with the kernel library replaced by a recorder (the technique of
test_encoder_layer_routes_cpu.py): for every generation option, both cross blocks, the fixed window and the sliding one, eager
and with the graph capture replaced by a replaying stub, `generate_from_codes`, `generate_from_code_long` and
`PriorRelative.generate_codes` make exactly the launches recorded in tests/golden/generation_launches.json -- entry points in
order, every scalar, the contents of every ctypes array, and of every tensor its dtype, shape, strides AND which buffer it is:
the first public attribute of the live incremental stack (sorted by name; `name[i]` inside a list) whose storage holds its
address, else the model parameter, else `tmp`, with the byte offset into that storage.  Raw addresses (`kv.data_ptr() + 4 * d`)
are resolved the same way, so nothing depends on where the allocator put things.  No GPU, no library.

The expected traces are data:  python tests/test_generation_launches_cpu.py --record  writes them from the checked-out package.
It was run at the commit BEFORE the generation options were set up in one place (one coordinate frame, `_configure`, one clearing
method, one body for the two public generators); that refactoring had to leave every trace as it was recorded.

The file keeps a table of distinct calls, a table of distinct segments (the calls up to and including a sampler launch: a step
repeats verbatim) and per case the run-length coded list of segments."""
import contextlib
import ctypes
import json
import os

import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'generation_launches.json')
KINDS = ('AC-AC', 'AC-D')
ROWS = 2
OPTION_LAUNCHES = ('_constrained', '_masked', 'vqcpc_decode_rules', 'vqcpc_particle_', 'vqcpc_decode_attn_probs')


# ---- the recorder -------------------------------------------------------------------------------------------------------
def _spans(value, name, out):
    if isinstance(value, torch.Tensor):
        if value.numel():
            st = value.untyped_storage()
            out.append((st.data_ptr(), st.data_ptr() + st.nbytes(), name))
    elif isinstance(value, list):
        for i, v in enumerate(value):
            if isinstance(v, torch.Tensor):
                _spans(v, f'{name}[{i}]', out)


class _Namer:
    """Addresses -> `buffer+byte offset`: the live stack's public attributes first, then the models' parameters."""

    def __init__(self):
        self.stack, self.params = None, []

    def add_model(self, model):
        for name, p in sorted(model.named_parameters()):
            _spans(p, name, self.params)

    def spans(self, args):
        """What an address of one launch can lie in: the stack's buffers, the parameters, then the launch's own tensors."""
        spans = []
        if self.stack is not None:
            for key, value in sorted(vars(self.stack).items()):
                if not key.startswith('_'):
                    _spans(value, key, spans)
        spans += self.params
        for i, t in enumerate(args):
            _spans(t, f'arg{i}', spans)
        return spans

    @staticmethod
    def name(ptr, spans, own):
        for lo, hi, name in spans:
            if lo <= ptr < hi and (own or not name.startswith('arg')):
                return f'{name}+{ptr - lo}'
        return 'tmp'

    def enc(self, a, spans):
        if isinstance(a, torch.Tensor):
            where = self.name(a.data_ptr(), spans, False) if a.numel() else 'tmp'
            return f'{where}:{str(a.dtype)[6:]}{list(a.shape)}{list(a.stride())}'
        if isinstance(a, ctypes.Array):
            return f'c{list(a)}'
        if isinstance(a, int) and not isinstance(a, bool) and a >= 1 << 32:          # a raw address
            return '@' + self.name(a, spans, True)
        return repr(a)


class _Replay:
    def __init__(self, fn):
        self.replay = fn


class _Stream:
    def synchronize(self):
        pass


@contextlib.contextmanager
def _recorder(*models):
    """hip / ops / the graph capture replaced; yields (calls, namer) and restores everything on exit."""
    from vqcpc_bach_amd import hip, ops
    from vqcpc_bach_amd.decoders.generation import IncrementalDecoder
    from vqcpc_bach_amd.priors.generation import IncrementalPrior
    from vqcpc_bach_amd.transformer.incremental import IncrementalStack
    calls, namer, real_stream = [], _Namer(), torch.cuda.current_stream
    for m in models:
        namer.add_model(m)

    def noting(init):
        def __init__(self, *a, **k):
            namer.stack = self
            init(self, *a, **k)
        return __init__

    def current_stream(device=None):          # the host models' stream: nothing to wait for; any other call is not ours
        return _Stream() if isinstance(device, torch.device) and device.type == 'cpu' else real_stream(device)

    def call(name, *args):
        spans = namer.spans(args)
        calls.append(f"{name}({', '.join(namer.enc(a, spans) for a in args)})")
        return 0
    new = {hip: {'call': call, 'query': lambda name, *args: 1, 'get_gemm_mode': lambda: 1,
                 'workspace': lambda n, dev: torch.empty(16, dtype=torch.uint8)},
           ops: {'_f32': lambda t: t, '_splitk_ws': {}, '_rowcut': {}, '_masked_ok_cache': {}, '_NAN1': {}},
           torch.cuda: {'current_stream': current_stream},
           IncrementalStack: {'capture': lambda self, fn: _Replay(fn)},
           IncrementalDecoder: {'__init__': noting(IncrementalDecoder.__init__)},
           IncrementalPrior: {'__init__': noting(IncrementalPrior.__init__)}}
    old = {m: {k: m.__dict__[k] if isinstance(m, type) else getattr(m, k) for k in kv} for m, kv in new.items()}
    try:
        for m, kv in new.items():
            for k, val in kv.items():
                setattr(m, k, val)
        yield calls, namer
    finally:
        for m, kv in old.items():
            for k, val in kv.items():
                setattr(m, k, val)


# ---- the models and the options ---------------------------------------------------------------------------------------------
_MODELS = {}


def _decoder(kind):
    from product_codes_helpers import build_decoder, tiny_cfg
    if kind not in _MODELS:
        _MODELS[kind] = build_decoder(tiny_cfg(4, 1), kind=kind, device=None, seed=11).eval()
    return _MODELS[kind]


def _prior():
    from product_codes_helpers import prior_cfg
    from test_prior_cpu import build_prior
    if 'prior' not in _MODELS:
        torch.manual_seed(12)
        _MODELS['prior'] = build_prior(prior_cfg(32, 1)).eval()
    return _MODELS['prior']


def _options(name, dec, events):
    """The keywords of one option case for a generation over `events` events (16 per window; the chorale's in long mode)."""
    from vqcpc_bach_amd.templates import VoiceLeadingRules
    nc, vmax = dec.num_channels, max(dec.num_tokens_per_channel)
    g = torch.Generator().manual_seed(5)
    constraint = torch.full((ROWS, events, nc), -1, dtype=torch.int64)
    constraint[:, ::3, 0] = torch.randint(0, 6, (ROWS, len(range(0, events, 3))), generator=g)
    allowed = torch.rand(events, nc, vmax, generator=g) < 0.7
    allowed[:, :, :6] = True
    rules = VoiceLeadingRules(50 + torch.arange(vmax).repeat(nc, 1) - 3 * torch.arange(nc).view(-1, 1), no_crossing=True,
                              max_leap=7, no_parallels=True)
    return {'plain': {},
            'constraint_logp': dict(constraint=constraint, return_logp=True),
            'allowed_mass': dict(allowed=allowed, return_allowed_mass=True),
            'rules': dict(rules=rules, return_rule_report=True),
            'rules_allowed': dict(rules=rules, return_rule_report=True, allowed=allowed),
            'attentions': dict(return_attentions=(0,)),
            'particles': dict(particles=2, constraint=constraint),
            'particles_returned': dict(particles=2, constraint=constraint, return_particles=True),
            'exclude': None,                                             # spelt differently by the two generators
            'decodings2': dict(num_decodings=2)}[name]


OPTIONS = ('plain', 'constraint_logp', 'allowed_mass', 'rules', 'rules_allowed', 'attentions', 'particles', 'particles_returned',
           'exclude', 'decodings2')
FORMS = ('fixed', 'long', 'long_sub')


def _cases():
    cases = {}
    for kind in KINDS:
        for graph in (False, True):
            tail = f'{kind}-{"graph" if graph else "eager"}'
            for form in FORMS:
                for opt in OPTIONS:
                    cases[f'{form}-{opt}-{tail}'] = dict(what='generate', kind=kind, graph=graph, form=form, opt=opt)
            cases[f'stack-plain-{tail}'] = dict(what='stack', kind=kind, graph=graph, again=False)
            cases[f'stack-again-{tail}'] = dict(what='stack', kind=kind, graph=graph, again=True)
    for graph in (False, True):
        for opt in ('plain', 'constraint_logp'):
            cases[f'prior-{opt}-{"graph" if graph else "eager"}'] = dict(what='prior', graph=graph, opt=opt)
    return cases


CASES = _cases()


def _run_generate(spec):
    dec = _decoder(spec['kind'])
    S, epc = dec.num_tokens_source, dec.num_events_per_code
    g = torch.Generator().manual_seed(3)
    with _recorder(dec) as (calls, _):
        if spec['form'] == 'fixed':
            kw = _options(spec['opt'], dec, S * epc)
            if kw is None:
                kw = dict(exclude_tokens=[[0, 7], [], [33 % 12], [1]])
            dec.generate_from_codes(torch.randint(0, 4, (ROWS, S), generator=g), temperature=0.9, top_k=5, top_p=0.8, seed=7,
                                    use_graph=spec['graph'], **kw)
        else:
            nb = S + 2
            kw = _options(spec['opt'], dec, nb * epc)
            if kw is None:
                kw = dict(exclude_meta_symbols=True)
            if spec['form'] == 'long_sub':
                kw.update(code_index_start=1, code_index_end=nb - 1)
            dec.generate_from_code_long(torch.randint(0, 4, (ROWS, nb), generator=g), temperature=0.9, top_k=5, top_p=0.8,
                                        seed=7, use_graph=spec['graph'], **kw)
        return list(calls)


def _run_stack(spec):
    """`start` + `run` on one IncrementalDecoder; again: after runs with every option on, fixed-window and sliding."""
    from vqcpc_bach_amd.decoders.generation import IncrementalDecoder
    from vqcpc_bach_amd.utils import STEP_LOCK
    dec = _decoder(spec['kind'])
    S, U, epc, nc = dec.num_tokens_source, dec.total_upscaling, dec.num_events_per_code, dec.num_channels
    g = torch.Generator().manual_seed(3)
    codes = torch.randint(0, 4, (ROWS, S + 2), generator=g)
    with _recorder(dec) as (calls, _), STEP_LOCK, torch.no_grad():
        inc = IncrementalDecoder(dec, ROWS)
        inc.prefill(codes[:, :S])
        if spec['again']:
            on = _options('rules_allowed', dec, S * epc)
            con = _options('constraint_logp', dec, S * epc)['constraint'].reshape(ROWS, -1)
            words = dec._allowed_words(on['allowed'], ROWS, S * epc).expand(ROWS, -1, -1)
            every = dict(constraint=con, want_logp=True, allowed=words, want_allowed_mass=True, rules=on['rules'],
                         exclude=[[0, 7], [], [9], [1]], want_probs=True)
            inc.start(seeds=5, temperature=0.7, top_k=3, top_p=0.9, want_attentions=(0, 1), **every)
            inc.run(use_graph=spec['graph'])
            inc.start(seeds=5, temperature=0.7, top_k=3, top_p=0.9, particles=2, **every)
            inc.run(use_graph=spec['graph'])
            nb = S + 2
            on = _options('rules_allowed', dec, nb * epc)
            con = _options('constraint_logp', dec, nb * epc)['constraint'].reshape(ROWS, -1)
            words = dec._allowed_words(on['allowed'], ROWS, nb * epc).expand(ROWS, -1, -1)
            every.update(constraint=con, allowed=words)
            chorale = torch.zeros(ROWS, nb * U, dtype=torch.int64)
            inc.start_long(codes, chorale, seeds=5, temperature=0.7, top_k=3, top_p=0.9, want_attentions=(1,), **every)
            inc.run_long(0, nb, use_graph=spec['graph'])
            inc.start_long(codes, chorale, seeds=5, temperature=0.7, top_k=3, top_p=0.9, particles=2, **every)
            inc.run_long(1, nb - 1, use_graph=spec['graph'])
            inc.prefill(codes[:, :S])
        del calls[:]
        inc.start(seeds=7, temperature=0.9, top_k=5, top_p=0.8)
        inc.run(use_graph=spec['graph'])
        return list(calls)


def _run_prior(spec):
    prior = _prior()
    N = prior.num_tokens
    kw = {}
    if spec['opt'] == 'constraint_logp':
        constraint = torch.full((ROWS, N + 3), -1, dtype=torch.int64)
        constraint[:, ::2] = 4
        kw = dict(constraint=constraint, return_logp=True)
    with _recorder(prior) as (calls, _):
        prior.generate_codes(N + 3, temperature=0.9, num_generated_codes=ROWS, top_k=5, seed=7, use_graph=spec['graph'], **kw)
        return list(calls)


def run_case(spec):
    return {'generate': _run_generate, 'stack': _run_stack, 'prior': _run_prior}[spec['what']](spec)


# ---- the fixture -------------------------------------------------------------------------------------------------------------
def _segments(trace):
    """The trace cut after every sampler launch."""
    seg = []
    for c in trace:
        seg.append(c)
        if '_sample' in c.split('(', 1)[0]:
            yield seg
            seg = []
    if seg:
        yield seg


def _golden():
    with open(GOLDEN) as fh:
        g = json.load(fh)
    segs = [[g['calls'][i] for i in idx] for idx in g['segments']]
    return {cid: [c for s, n in runs for _ in range(n) for c in segs[s]] for cid, runs in g['cases'].items()}


@pytest.fixture(scope='module')
def golden():
    return _golden()


def test_the_grid_is_the_recorded_one(golden):
    assert sorted(golden) == sorted(CASES)


@pytest.mark.parametrize('cid', sorted(CASES))
def test_generation_makes_the_recorded_launches(cid, golden):
    got, want = run_case(CASES[cid]), golden[cid]
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f'{cid}: launch {i}'
    assert len(got) == len(want), (cid, got[len(want):], want[len(got):])


@pytest.mark.parametrize('cid', sorted(c for c in CASES if '-again-' in c))
def test_a_second_start_leaves_every_option_off(cid, golden):
    """`start` with every option off on a stack that ran with every option on: the launches of a fresh stack."""
    assert golden[cid] == golden[cid.replace('-again-', '-plain-')]
    assert run_case(CASES[cid]) == golden[cid.replace('-again-', '-plain-')]


@pytest.mark.parametrize('cid', sorted(c for c in CASES if '-plain-' in c or '-again-' in c))
def test_plain_cases_launch_no_option_kernel(cid, golden):
    names = [c.split('(', 1)[0] for c in golden[cid]]
    assert names and not [n for n in names if any(o in n for o in OPTION_LAUNCHES)]


def test_known_launch_counts(golden):
    """A plain fixed-window run makes about 1 500 launches, a long one over S + 2 codes about 2 400."""
    assert 1400 <= len(golden['fixed-plain-AC-AC-eager']) <= 1600
    assert 2200 <= len(golden['long-plain-AC-AC-eager']) <= 2600


def record():
    calls, segs, cases = {}, {}, {}
    for cid in sorted(CASES):
        runs = []
        for seg in _segments(run_case(CASES[cid])):
            s = segs.setdefault(tuple(calls.setdefault(c, len(calls)) for c in seg), len(segs))
            if runs and runs[-1][0] == s:
                runs[-1][1] += 1
            else:
                runs.append([s, 1])
        cases[cid] = runs
    pack = lambda v: json.dumps(v, separators=(',', ':'))
    with open(GOLDEN, 'w') as fh:          # one launch / one segment / one case per line
        fh.write('{"calls": [\n' + ',\n'.join(json.dumps(c) for c in calls) + '\n],\n"segments": [\n')
        fh.write(',\n'.join(pack(list(s)) for s in segs) + '\n],\n"cases": {\n')
        fh.write(',\n'.join(f'{json.dumps(cid)}: {pack(runs)}' for cid, runs in cases.items()) + '\n}}\n')
    print(f'{len(cases)} cases, {len(segs)} distinct segments, {len(calls)} distinct launches -> {GOLDEN}')


if __name__ == '__main__':
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [os.path.dirname(here), here]
    if sys.argv[1:] == ['--record']:
        record()
    else:
        sys.exit('usage: test_generation_launches_cpu.py --record')
