"""CPU-side checks of the generation attention maps: the new entry point is declared, exported and bound, rejects bad
arguments before any HIP call, and the host's `window_start` schedule of long-form generation equals a restatement of the
reference's window rule (decoder.py:831-854)."""
import os

import numpy as np
import pytest
import torch

ARGS_OK = dict(q=16, ldq=16, kc=16, vc=16, ldc=16, knew=None, vnew=None, ldn=0, e1=16, e2=16, ctx=16, ldo=16, pos=16, M=1, Lk=4,
               ratio=1, H=1, hd=16, mask=0, probs=16, ldp=4, rows=1, win=None, win_stride=0, stream=None)


@pytest.fixture(scope='module')
def lib():
    from vqcpc_bach_amd import build, hip
    if not os.path.exists(hip.LIB_PATH):
        build.build(verbose=False)
    return hip.load()


def _call(lib, **changed):
    """vqcpc_decode_attn_probs on fake (non-NULL, 16-byte aligned) addresses: only calls the host checks reject are made."""
    return lib.vqcpc_decode_attn_probs(*dict(ARGS_OK, **changed).values())


def test_entry_point_is_exported_and_bound(lib):
    from vqcpc_bach_amd import hip
    assert hasattr(lib, 'vqcpc_decode_attn_probs')
    res, args = hip.SIGNATURES['vqcpc_decode_attn_probs']
    plain = hip.SIGNATURES['vqcpc_decode_attn'][1]
    # every argument of vqcpc_decode_attn, then probs, ldp, rows, win, win_stride, and the stream
    assert res is hip.c_int and args == plain[:-1] + [hip.c_ptr, hip.c_i64, hip.c_i64, hip.c_ptr, hip.c_int, hip.c_ptr]
    assert lib.vqcpc_decode_attn_probs.argtypes == args
    assert lib.vqcpc_abi_version() == 2


@pytest.mark.parametrize('changed', [dict(probs=None), dict(ldp=3), dict(rows=0), dict(win=16, win_stride=0), dict(hd=24),
                                     dict(Lk=1025, ldp=1025), dict(q=None)])
def test_bad_arguments_are_refused_before_any_hip_call(lib, changed):
    assert _call(lib, **changed) == -1
    assert b'decode_attn_probs' in lib.vqcpc_last_error(), lib.vqcpc_last_error()


def test_the_plain_entry_keeps_its_name_in_errors(lib):
    a = dict(ARGS_OK, q=None)
    for k in ('probs', 'ldp', 'rows', 'win', 'win_stride'):
        del a[k]
    assert lib.vqcpc_decode_attn(*a.values()) == -1
    err = lib.vqcpc_last_error()
    assert b'decode_attn:' in err and b'decode_attn_probs' not in err


def _restated(t, nb, S):
    """The three branches of decoder.py:831-854: the first code of the window that generates code t."""
    h = S // 2
    return min(max(0, t - h), nb - S)


@pytest.mark.parametrize('nb,S', [(3, 3), (4, 3), (9, 4), (96, 24)])
def test_window_start_schedule(nb, S):
    from vqcpc_bach_amd.decoders.decoder import Decoder
    U = 16
    for start, end in {(0, nb), (1, nb), (0, nb - 1), (nb // 2, nb // 2), (1, max(1, nb - 1)), (nb // 3, 2 * nb // 3 + 1)}:
        ws = Decoder.attention_window_starts(nb, S, U, start, end)
        assert ws.dtype == torch.int64 and tuple(ws.shape) == (nb * U,) and not ws.is_cuda
        want = np.full(nb * U, -1, dtype=np.int64)
        for t in range(start, end):
            want[t * U:(t + 1) * U] = _restated(t, nb, S)
        assert np.array_equal(ws.numpy(), want), (start, end)
        # every emitted position lies inside its window: its row of the window is c - w * U in [0, S * U)
        c = np.nonzero(want >= 0)[0]
        assert ((c - want[c] * U >= 0) & (c - want[c] * U < S * U)).all()
        assert (want[c] + S <= nb).all()


def test_layer_choice_and_size_guard_on_the_host():
    """`_attention_layers` and `_check_attention_bytes` read a few attributes only: a namespace stands in for the module."""
    import types
    from vqcpc_bach_amd.decoders.decoder import Decoder
    layers = [None] * 3
    h = types.SimpleNamespace(transformer=types.SimpleNamespace(decoder=types.SimpleNamespace(layers=layers), nhead=8,
                                                                encoder=types.SimpleNamespace(layers=layers)),
                              num_tokens_target=384, num_tokens_source=24, cross_attention_type='anticausal')
    pick = types.MethodType(Decoder._attention_layers, h)
    assert pick(False) is None and pick(True) == (0, 1, 2) and pick([2, 0, 2]) == (0, 2) and pick(True, default=(2,)) == (2,)
    for bad in ([3], [-1], [], 1):
        with pytest.raises(ValueError):
            pick(bad)
    size = types.MethodType(Decoder._check_attention_bytes, h)
    # the DEC shape, B = 32, every layer: 32 * 3 * 8 * 384 * (384 + 24) * 4 + the encoder's 32 * 3 * 8 * 24 * 24 * 4: under 1 GiB
    n = size(32, (0, 1, 2), 384, True, 4 << 30)
    assert n == 4 * 32 * 3 * 8 * (384 * 408 + 24 * 24) and n < 1 << 30
    with pytest.raises(ValueError, match='fewer layers'):
        size(32, (0, 1, 2), 384, True, n - 1)
    h.cross_attention_type = 'diagonal'
    assert size(1, (1,), 384, False, 4 << 30) == 4 * 8 * 384 * 384
