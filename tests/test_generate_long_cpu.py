"""CPU-side checks of long-form generation: the window arithmetic and the initial chorale of `Decoder` against the
fixtures of the reference's own `generate_from_code_long` (tests/golden/generate_long_tiny_S*.npz), and the declaration
of the new entry points."""
import json
import os
import re
import types

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden

FIXTURES = ['generate_long_tiny_S4', 'generate_long_tiny_S3']


def _decoder_class():
    from vqcpc_bach_amd.decoders.decoder import Decoder
    return Decoder


def _host_decoder(vocab, n2i):
    """The two host-only methods need num_channels, the dataset and a device: a namespace stands in for the module."""
    Decoder = _decoder_class()
    ds = types.SimpleNamespace(note2index_dicts=n2i) if n2i is not None else types.SimpleNamespace()
    h = types.SimpleNamespace(num_channels=len(vocab), dataloader_generator=types.SimpleNamespace(dataset=ds),
                              sos=torch.zeros(1))
    h._meta_symbol = types.MethodType(Decoder._meta_symbol, h)
    h.init_generation_chorale = types.MethodType(Decoder.init_generation_chorale, h)
    return h


def _restated(t, nb, S):
    """The three branches of decoder.py:831-854 in four lines."""
    h = S // 2
    rel = h if h <= t < nb - h else (t if t < h else S - (nb - t))
    b = min(max(0, t - h), nb - S)
    return b, b + S, rel


@pytest.mark.parametrize('name', FIXTURES)
def test_window_arithmetic_equals_the_fixture(name):
    Decoder = _decoder_class()
    g = load_golden(name)
    cfg = json.loads(str(g['cfg_json']))
    nb = g['codes'].shape[1]
    S = cfg['events'] * len(cfg['vocab']) // 16
    start, end = int(g['code_index_start']), int(g['code_index_end'])
    assert g['windows'].shape == (end - start, 3)
    for k, t in enumerate(range(start, end)):
        assert tuple(Decoder.compute_start_end_times(t, nb, S)) == tuple(int(v) for v in g['windows'][k]), t
    assert g['gaps'].shape == (g['tokens'].shape[0], (end - start) * 16) and g['gaps'].min() > 1e-3
    assert g['tokens'].shape == (cfg['B'] * int(g['num_decodings']), (end - start) * 16 // len(cfg['vocab']), len(cfg['vocab']))


def test_window_arithmetic_exhaustive():
    Decoder = _decoder_class()
    for S in (2, 3, 4, 24):
        for nb in range(S, 3 * S + 2):
            for t in range(nb):
                b, e, rel = Decoder.compute_start_end_times(t, nb, S)
                assert (b, e, rel) == _restated(t, nb, S), (S, nb, t)
                assert 0 <= b and e <= nb and e - b == S and 0 <= rel < S and b + rel == t, (S, nb, t)


@pytest.mark.parametrize('name', FIXTURES)
def test_initial_chorale_equals_the_fixture(name):
    g = load_golden(name)
    cfg = json.loads(str(g['cfg_json']))
    vocab = cfg['vocab']
    n2i = [{'START': int(s), 'END': int(e), 'XX': int(p)} for s, e, p in zip(g['start'], g['end'], g['pad'])]
    epc = 16 // len(vocab)
    nb, start = g['codes'].shape[1], int(g['code_index_start'])
    ref = torch.from_numpy(g['init_chorale'])
    out = _host_decoder(vocab, n2i).init_generation_chorale(num_events=nb * epc, start_index=start * epc)
    assert out.dtype == torch.int64 and torch.equal(out, ref)
    # explicit per-voice ids, for datasets without meta symbols
    bare = _host_decoder(vocab, None)
    out = bare.init_generation_chorale(nb * epc, start * epc, pad=g['pad'].tolist(), start=g['start'].tolist())
    assert torch.equal(out, ref)
    with pytest.raises(ValueError, match='pad=.*start='):
        bare.init_generation_chorale(nb * epc, start * epc)
    with pytest.raises(ValueError, match='pad=.*start='):
        bare.init_generation_chorale(nb * epc, start * epc, pad=g['pad'].tolist())
    # start_index 0: no START anywhere
    out = bare.init_generation_chorale(8, 0, pad=g['pad'].tolist())
    assert torch.equal(out, torch.from_numpy(g['pad']).view(1, 1, -1).expand(1, 8, -1))


def test_new_entry_points_are_declared():
    from vqcpc_bach_amd import hip
    text = open(os.path.join(ROOT, 'include', 'vqcpc.h')).read()
    for name in ('vqcpc_decode_prefill_attn', 'vqcpc_decode_window'):
        assert name in hip.SIGNATURES
        m = re.search(r'^int ' + name + r'\((.*?)\);', text, flags=re.S | re.M)
        assert m, name
        assert len(m.group(1).split(',')) == len(hip.SIGNATURES[name][1]), name
