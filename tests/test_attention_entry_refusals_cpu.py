"""What the self-attention entry points (vqcpc_relattn_*, vqcpc_relattn16_*, vqcpc_relattn_tab_*) and the three vqcpc_decode_sample
forms refuse, with which code and under whose name.  Host-only: dummy 16-byte-aligned addresses that are never dereferenced, every
call wrong in exactly one respect, so each must come back with VQCPC_EINVAL (VQCPC_EWORKSPACE for a short workspace) and a message
that starts with the entry point's own name before anything is launched."""
import ctypes
import os
import shutil
import subprocess

import pytest
import torch

from conftest import ROOT

EINVAL, EWORKSPACE = -1, -3
N, L, H, HD = 3, 16, 2, 16
D = H * HD


@pytest.fixture(scope='module')
def lib():
    if torch.cuda.is_available():
        pytest.skip('host-only: a missing refusal must not become a launch on dummy addresses')
    from vqcpc_bach_amd import build, hip
    if not os.path.exists(hip.LIB_PATH):
        build.build(verbose=False)
    return hip.load()


def _addr(i):
    return 0x10000 * (i + 1)          # 16-byte aligned, distinct


def _fwd(name, src='qkv', tokens=None, has_L=True, in16=False):
    """(name, [(argument, good value)], facts) of a forward entry point, in the order of include/vqcpc.h."""
    a = [(src, _addr(0)), ('ldq', 3 * D)]
    if tokens is not None:
        a.append(('tokens', _addr(1) if tokens == 'required' else None))
    a += [('e1', _addr(2)), ('e2', _addr(3)), ('ctx', _addr(4)), ('ldo', D), ('probs', _addr(5)), ('n_blocks', N)]
    if has_L:
        a.append(('L', L))
    a += [('H', H), ('hd', HD), ('drop_p', 0.1), ('seed', 7)]
    return name, a, dict(fwd=True, src=src, tokens=tokens, has_L=has_L, in16=in16)


def _bwd(name, src='qkv', tokens=None, has_L=True, in16=False):
    a = [('d_ctx', _addr(6)), ('ldo', D), (src, _addr(0)), ('ldq', 3 * D)]
    if tokens is not None:
        a.append(('tokens', _addr(1) if tokens == 'required' else None))
    a += [('probs', _addr(5)), ('e1', _addr(2)), ('e2', _addr(3)), ('d_qkv', _addr(7)), ('ldg', 3 * D), ('d_e1', _addr(8)),
          ('d_e2', _addr(9)), ('n_blocks', N)]
    if has_L:
        a.append(('L', L))
    a += [('H', H), ('hd', HD), ('drop_p', 0.1), ('seed', 7), ('workspace', _addr(10)), ('workspace_bytes', None)]
    return name, a, dict(fwd=False, src=src, tokens=tokens, has_L=has_L, in16=in16)


# pointers whose misalignment is refused (not: sends the call to another kernel), per entry point
ENTRIES = [
    (_fwd('vqcpc_relattn_fwd'), ()),
    (_bwd('vqcpc_relattn_bwd'), ()),
    (_fwd('vqcpc_relattn_fwd_b16'), ('qkv', 'ctx')),
    (_bwd('vqcpc_relattn_bwd_b16'), ('qkv', 'd_ctx', 'd_qkv')),
    (_fwd('vqcpc_relattn16_fwd_b16', tokens='optional', has_L=False), ('qkv', 'e1', 'e2', 'ctx')),
    (_bwd('vqcpc_relattn16_bwd_b16', tokens='optional', has_L=False), ('qkv', 'd_ctx', 'e1', 'e2', 'd_qkv')),
    (_fwd('vqcpc_relattn16_fwd_b16io', has_L=False, in16=True), ('qkv', 'e1', 'e2', 'ctx')),
    (_bwd('vqcpc_relattn16_bwd_b16io', has_L=False, in16=True), ('qkv', 'd_ctx', 'e1', 'e2', 'd_qkv')),
    (_fwd('vqcpc_relattn_tab_fwd', src='table', tokens='required'), ()),
    (_bwd('vqcpc_relattn_tab_bwd', src='table', tokens='required'), ()),
]
# at any other L vqcpc_relattn_fwd / _bwd hand over to the strip kernels, and these must be aligned for them
STRIP_ALIGNED = {'vqcpc_relattn_fwd': ('qkv', 'e1', 'e2'), 'vqcpc_relattn_bwd': ('qkv', 'd_ctx', 'workspace')}


def _refused(lib, name, args, change, code=EINVAL):
    """Calls `name` with the good arguments and `change` applied; it must be refused with `code` under its own name."""
    vals = dict(args)
    vals.update(change)
    if 'workspace_bytes' in vals and vals['workspace_bytes'] is None:
        vals['workspace_bytes'] = lib.vqcpc_relattn_bwd_workspace(max(vals['n_blocks'], 1), vals.get('L', 16), vals['H'], vals['hd'])
    short = vals.pop('_short', 0)
    if short:
        vals['workspace_bytes'] -= short
    rc = getattr(lib, name)(*[vals[k] for k, _ in args], None)
    err = lib.vqcpc_last_error().decode()
    assert rc == code and err.startswith(name[len('vqcpc_'):] + ':'), (name, change, rc, err)


@pytest.mark.parametrize('entry,must_align', ENTRIES, ids=[e[0][0] for e in ENTRIES])
def test_self_attention_entry_refuses(lib, entry, must_align):
    name, args, f = entry
    src = f['src']
    pointers = [k for k, v in args if isinstance(v, int) and v >= 0x10000]
    for k in pointers:                                                     # a null pointer
        _refused(lib, name, args, {k: None})
    if f['tokens'] == 'required':                                          # (the table forms: `tokens` is one of them)
        assert 'tokens' in pointers
    # an unsupported (L, H, hd)
    _refused(lib, name, args, {'hd': 8})
    _refused(lib, name, args, {'H': 0})
    if f['has_L']:
        _refused(lib, name, args, {'L': 2000 if name in STRIP_ALIGNED else 24})
    # leading dimensions: not a multiple of 4 (of 8: bf16 q | k | v and d ctx), and too small
    in_step = 8 if f['in16'] else 4
    lds = [('ldq', 3 * D, in_step), ('ldo', D, 4 if f['fwd'] else in_step)] + ([] if f['fwd'] else [('ldg', 3 * D, 4)])
    for k, least, step in lds:
        _refused(lib, name, args, {k: least + step // 2})
        _refused(lib, name, args, {k: least - step})
    if f['fwd']:
        _refused(lib, name, args, {'drop_p': 1.0})
    else:
        _refused(lib, name, args, {'n_blocks': 0})
        _refused(lib, name, args, {'_short': 1}, code=EWORKSPACE)          # a workspace one byte short
    for k in must_align:                                                   # a pointer 4 bytes off
        k = src if k == 'qkv' else k
        _refused(lib, name, args, {k: dict(args)[k] + 4})
    for k in STRIP_ALIGNED.get(name, ()):
        _refused(lib, name, args, {'L': 24, k: dict(args)[k] + 4})


def test_route_table_against_the_documented_rule(tmp_path):
    """tests/relattn_forms_check.cpp: every descriptor of csrc/relattn_forms.h over block lengths, heads, head sizes, the force_general switch,
    tokens given or not and every alignment mask, against the documented rule; the 6 + 9 kernel instantiations are reached and no
    other (host program with its own main, under the address and undefined-behaviour sanitizers)."""
    cxx = shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    assert cxx, 'no host C++ compiler'
    exe = str(tmp_path / 'relattn_forms_check')
    subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-o', exe,
                    os.path.join(ROOT, 'tests', 'relattn_forms_check.cpp')], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert '307200 calls' in run.stdout and '6 + 9 forms reached, 0 failures' in run.stdout, run.stdout


T, NC, M, DM, U = 8, 2, 4, 16, 1


def _sample(form):
    a = [('logits', _addr(0)), ('ldl', 300), ('voice_offsets', None), ('nc', NC), ('M', M), ('temperature', 1.0), ('top_k', 0),
         ('top_p', 1.0), ('exclude', None), ('seeds', _addr(1))]
    if form == 'plain':
        a += [('teacher', None), ('ldteach', 0)]
    else:
        a += [('constraint', None), ('ldcons', 0), ('logp', None), ('ldlogp', 0), ('win', None)]
    if form == 'masked':
        a += [('allowed', None), ('ldallow', 0), ('logmass', None), ('ldmass', 0)]
    a += [('tokens', _addr(2)), ('ldtok', T), ('T', T), ('table', _addr(3)), ('table_rows', 290), ('d', DM), ('U', U),
          ('next_in', _addr(4)), ('ldn', DM), ('probs', None), ('ldp', 0), ('pos', _addr(5))]
    return a


SAMPLERS = [('vqcpc_decode_sample', 'plain'), ('vqcpc_decode_sample_constrained', 'constrained'), ('vqcpc_decode_sample_masked', 'masked')]


@pytest.mark.parametrize('name,form', SAMPLERS, ids=[s[1] for s in SAMPLERS])
def test_decode_sample_entry_refuses(lib, name, form):
    args = _sample(form)

    def refused(change, offsets=(0, 10, 30)):
        vo = (ctypes.c_int32 * 18)(*offsets, *([offsets[-1]] * (18 - len(offsets))))          # read on the host
        _refused(lib, name, args, dict(change, voice_offsets=ctypes.cast(vo, ctypes.c_void_p)))

    refused({}, offsets=(0, 290, 300))                                     # a voice of 290 tokens
    refused({'M': 65})
    refused({'nc': 17})
    refused({'temperature': 0.0})
    refused({'seeds': None})                                               # (plain form: no teacher either)
    refused({'ldtok': T - 1})
    refused({'table_rows': 19})                                            # 20 tokens x U rows needed
    refused({'ldl': 29})
    refused({'ldn': DM - 1})
    refused({'probs': _addr(6), 'ldp': 19})
    for k in ('logits', 'tokens', 'table', 'next_in', 'pos'):
        refused({k: None})
    if form == 'plain':
        refused({'teacher': _addr(7), 'seeds': None, 'ldteach': T - 1})    # teacher without seeds is accepted, a short ldteach not
    else:
        refused({'constraint': _addr(7), 'ldcons': T - 1})
        refused({'logp': _addr(8), 'ldlogp': T - 1})
    if form == 'masked':
        refused({'allowed': _addr(9), 'ldallow': T - 1})
        refused({'logmass': _addr(10), 'ldmass': T - 1})
