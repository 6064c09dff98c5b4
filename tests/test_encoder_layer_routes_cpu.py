"""Launch trace of ops.EncoderLayerFn, forward and backward, with the kernel library replaced by a recorder (the technique of
test_arith_scopes_cpu.py): for every input form, GEMM mode, switch setting and `..._supported` answer the layer makes exactly the
launches recorded in tests/golden/encoder_layer_routes.json -- entry points in order, every scalar argument, and dtype / shape /
strides of every tensor argument, then the gradients handed back to autograd.  No GPU, no library.

The expected traces are data:  python tests/test_encoder_layer_routes_cpu.py --record  writes them from the checked-out ops.py
(it was run at the commit before the layer's route became one record, ops._LayerRoute)."""
import contextlib
import json
import os

import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'encoder_layer_routes.json')
H, D, FFD, NBLK, P = 8, 256, 1024, 64, 0.1
SWITCHES = ('ATT_B16_IN', 'ATT_B16_OUT', 'BF16_RESIDUAL', 'BF16_SUMS', 'BF16_GRAD_SUMS', 'BF16_GRAD_STREAM', 'BF16_ACT_STREAM',
            'BF16_TAB_GRAD')
SUPPORTED = ('vqcpc_gemm_nt_bf16_supported', 'vqcpc_gemm_tn_bf16_supported', 'vqcpc_relattn16_b16_supported',
             'vqcpc_relattn_b16_supported', 'vqcpc_relattn_sub_b16_supported', 'vqcpc_gemm_gatebits_supported')
FORMS = ('own', 'ext', 'tab', 'qs4')       # own projection | per-token qkv_in | block table + qkv_tokens | qstride = 4


def _variants(mode):
    """name -> settings, each varied alone from the base case (L = 16, p = 0.1, x requires grad, default switches, every query 1)."""
    v = {'base': {}, 'L4': {'L': 4}, 'p0': {'p': 0.0}, 'x_no_grad': {'x_grad': False},
         'sform_everywhere': {'ops': {'SFORM_MIN_TILES': 0}},          # the epilogue forms of the residual sums at this small size
         'gate_bits': {'ops': {'GATEBITS_MIN_TILES': 0}},              # ... and the bit-mask gate of the feed-forward backward
         'ATT_B16_OUT_off_L4': {'L': 4, 'ops': {'ATT_B16_OUT': False}},
         'tab_grad_b16_96_tokens': {'ops': {'BF16_TAB_GRAD': True}, 'vmax': 96}}      # past the bf16 segment sum's 80-token table
    for name in SWITCHES:
        v[name + '_flipped'] = {'ops': {name: None}}                   # None: the opposite of the module's default
    for name in SUPPORTED:
        v[name + '_0'] = {'no': (name,)}
    v['relattn_b16_supported_0_L4'] = {'L': 4, 'no': ('vqcpc_relattn_b16_supported',)}
    if mode == 2:
        v['not_native'] = {'not_native': True}
        v['chain_first'] = {'chain': 'first'}          # this form's layer with out_b16_only, feeding an own-projection layer
        v['chain_second'] = {'chain': 'second'}        # an own-projection layer with out_b16_only feeding this form's layer
        v['chain_second_not_native'] = {'chain': 'second', 'second_not_native': True}      # the carrier reaches a layer off the bf16 path
        v['chain_second_BF16_SUMS_off'] = {'chain': 'second', 'second_ops': {'BF16_SUMS': False}}
    return v


CASES = {f'{form}-mode{mode}-{name}': dict(spec, form=form, mode=mode)
         for form in FORMS for mode in (1, 2) for name, spec in _variants(mode).items()}
FLIPS_AFTER_FORWARD = ('ATT_B16_OUT', 'BF16_GRAD_SUMS')


def _enc(a):
    if isinstance(a, torch.Tensor):
        return f'{str(a.dtype)[6:]}{list(a.shape)}{list(a.stride())}'
    return repr(a)


@contextlib.contextmanager
def _recorder(mode, no=()):
    """hip / ops with the library replaced: yields the list the launches are appended to, restores everything on exit."""
    from vqcpc_bach_amd import hip, ops
    calls = []
    new = {hip: {'call': lambda name, *args: calls.append(f"{name}({', '.join(_enc(a) for a in args)})") or 0,
                 'query': lambda name, *args: 0 if name in no else 1,
                 'get_gemm_mode': lambda: mode,
                 'workspace': lambda n, dev: torch.empty(16, dtype=torch.uint8)},
           ops: {'_f32': lambda t: t, '_splitk_ws': {}, '_rowcut': {}, '_masked_ok_cache': {}, '_NAN1': {}}}
    old = {m: {k: getattr(m, k) for k in kv} for m, kv in new.items()}
    old[ops].update({k: getattr(ops, k) for k in SWITCHES + ('bf16_native', 'SFORM_MIN_TILES', 'GATEBITS_MIN_TILES')})
    try:
        for m, kv in new.items():
            for k, val in kv.items():
                setattr(m, k, val)
        yield calls
    finally:
        for m, kv in old.items():
            for k, val in kv.items():
                setattr(m, k, val)


def _set(ops, settings):
    for k, val in settings.items():
        setattr(ops, k, (not getattr(ops, k)) if val is None else val)


def _leaf(*shape, grad=True, dtype=torch.float32):
    return torch.empty(*shape, dtype=dtype, device='meta', requires_grad=grad)


def _params(L):
    hd = D // H
    shapes = [(3 * D, D), (3 * D,), (D, D), (D,), (H * L, hd), (H * L, hd), (FFD, D), (FFD,), (D, FFD), (D,), (D,), (D,), (D,), (D,)]
    return [_leaf(*s) for s in shapes]


def _layer(ops, x, form, L, p, out_b16_only, vmax):
    """One EncoderLayerFn.apply in the given input form; returns (y, the leaves whose gradients are recorded)."""
    M = x.shape[0]
    qkv_in = tokens = None
    if form == 'ext':
        qkv_in = _leaf(M, 3 * D)
    elif form == 'tab':
        qkv_in = _leaf(vmax * L, 3 * D)
        tokens = torch.empty(M, dtype=torch.int64, device='meta')
    params = _params(L)
    y, _ = ops.EncoderLayerFn.apply(x, L, H, p, 1234 if p > 0 else 0, 4 if form == 'qs4' else 1, qkv_in, tokens, out_b16_only, *params)
    return y, [qkv_in] + params


def run_case(spec, flip_after_forward=None):
    """The trace of one case: the forward launches, '--- backward', the backward launches, then the gradients autograd received."""
    from vqcpc_bach_amd import ops
    L, p, vmax = spec.get('L', 16), spec.get('p', P), spec.get('vmax', 40)
    chain = spec.get('chain')
    with _recorder(spec['mode'], spec.get('no', ())) as calls:
        _set(ops, spec.get('ops', {}))
        if spec.get('not_native'):
            ops.bf16_native = lambda *shapes: False
        x = _leaf(NBLK * L, D, grad=spec.get('x_grad', True))
        first, second = (spec['form'], 'own') if chain == 'first' else ('own', spec['form'])
        y, leaves = _layer(ops, x, first if chain else spec['form'], L, p, bool(chain), vmax)
        if chain:
            calls.append('--- second layer')
            _set(ops, spec.get('second_ops', {}))
            if spec.get('second_not_native'):
                ops.bf16_native = lambda *shapes: False
            y, more = _layer(ops, y, second, L, p, False, vmax)
            leaves = leaves + more
        if flip_after_forward:
            _set(ops, {flip_after_forward: None})
        calls.append('--- backward')
        y.backward(torch.empty(y.shape, device='meta'))
        calls.append('grads(' + ', '.join(_enc(None if t is None else t.grad) for t in [x] + leaves) + ')')
        return list(calls)


def _golden():
    with open(GOLDEN) as fh:
        g = json.load(fh)
    return {cid: [g['calls'][i] for i in idx] for cid, idx in g['cases'].items()}


@pytest.fixture(scope='module')
def golden():
    return _golden()


def test_the_grid_is_the_recorded_one(golden):
    assert sorted(golden) == sorted(CASES)


@pytest.mark.parametrize('cid', sorted(CASES))
def test_layer_makes_the_recorded_launches(cid, golden):
    got, want = run_case(CASES[cid]), golden[cid]
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f'{cid}: launch {i}'
    assert len(got) == len(want), (cid, got[len(want):], want[len(got):])


@pytest.mark.parametrize('form,mode,rows', [('own', 1, 22), ('own', 2, 31), ('ext', 1, 18), ('ext', 2, 24), ('tab', 1, 19),
                                            ('tab', 2, 25), ('qs4', 1, 25), ('qs4', 2, 36)])
def test_base_cases_have_the_known_launch_counts(form, mode, rows, golden):
    assert sum(1 for c in golden[f'{form}-mode{mode}-base'] if c.startswith('vqcpc_')) == rows


@pytest.mark.parametrize('switch', FLIPS_AFTER_FORWARD)
@pytest.mark.parametrize('cid', [f'{form}-mode{mode}-{name}' for form in FORMS for mode in (1, 2)
                                 for name in (('base', 'L4') if mode == 1 else ('base', 'L4', 'chain_first', 'chain_second'))])
def test_backward_follows_the_route_forward_chose(cid, switch, golden):
    """A switch assigned between a node's forward and its backward changes nothing: backward obeys the route forward stored."""
    assert run_case(CASES[cid], flip_after_forward=switch) == golden[cid]


def record():
    calls, cases = {}, {}
    for cid in sorted(CASES):
        cases[cid] = [calls.setdefault(c, len(calls)) for c in run_case(CASES[cid])]
    with open(GOLDEN, 'w') as fh:          # one launch / one case per line
        fh.write('{"calls": [\n' + ',\n'.join(json.dumps(c) for c in calls) + '\n],\n"cases": {\n')
        fh.write(',\n'.join(f'{json.dumps(cid)}: {json.dumps(idx, separators=(",", ":"))}' for cid, idx in cases.items()) + '\n}}\n')
    print(f'{len(cases)} cases, {len(calls)} distinct launches -> {GOLDEN}')


if __name__ == '__main__':
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    if sys.argv[1:] == ['--record']:
        record()
    else:
        sys.exit('usage: test_encoder_layer_routes_cpu.py --record')
