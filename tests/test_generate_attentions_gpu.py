"""Attention maps of generation (`Decoder.generate*(return_attentions=...)`, decoders/generation.py, vqcpc_decode_attn_probs)
on the tiny decoders of the greedy and long fixtures, against
  (1) the same calls without the keyword (tokens and logp bit-identical), eager against graph, subsets against all layers,
  (2) the rows the reference's own generate loop keeps (tests/golden/generate_attentions_tiny*.npz,
      tools/gen_golden_generate_attentions.py: decoder.py:647-667 taken at every layer),
  (3) the full forward of this package, row by row (fixed window and every window of a long-form generation).

Tolerance of (2) and (3).  E_FWD is the largest absolute difference between the maps of the EXISTING `Decoder.forward` on the
fixture's tokens and the fixture (three maps, every layer, both fixtures): what this package's training-path attention
kernels differ from the reference's CPU softmax by.  The step kernel adds the same two sums in the same order but reduces and
exponentiates differently (`__expf`, a 256-thread tree), so the generation maps get TOL = 4 x E_FWD.
Measured on the MI355X: E_FWD = 2.384e-7 = 2^-22 (re-measured and printed by test_e_fwd).  The generation maps differ from the fixture by at most 1.19e-7 (self), 2.09e-7 (cross),
1.79e-7 (encoder) and 2.38e-7 (diagonal decoder, self), and from `Decoder.forward` by at most 1.19e-7 (fixed window) and
1.79e-7 (long form, cross; self 3.7e-8), against TOL = 9.54e-7."""
import glob
import json
import os
import types

import numpy as np
import pytest
import torch

from conftest import load_golden, sub_state
from oracle import decoder_oracle as D
from test_decoder_gpu import build_decoder
from test_generate_gpu import _api_decoder

pytestmark = pytest.mark.gpu
T = torch.from_numpy

E_FWD = 2.385e-7             # measured (2.384e-7 = 2^-22, rounded up), see the module docstring
TOL = 4 * E_FWD


def _greedy(name):
    g = load_golden(name)
    cfg = D.make_cfg(**json.loads(str(g['cfg_json'])))
    return build_decoder(cfg, sub_state(g, 'sd')), g


@pytest.fixture(scope='module')
def tiny():
    """The model of generate_greedy_tiny, its reference maps and ONE greedy generation with every layer's maps."""
    dec, g = _greedy('generate_greedy_tiny')
    codes = T(g['codes']).cuda()
    tokens, att = dec.generate_from_codes(codes, top_k=1, seed=0, return_attentions=True)
    return types.SimpleNamespace(dec=dec, g=g, a=load_golden('generate_attentions_tiny'), codes=codes, tokens=tokens, att=att)


@pytest.fixture(scope='module')
def diagonal():
    dec, g = _greedy('generate_greedy_tiny_diagonal')
    codes = T(g['codes']).cuda()
    tokens, att = dec.generate_from_codes(codes, top_k=1, seed=0, return_attentions=True)
    return types.SimpleNamespace(dec=dec, g=g, a=load_golden('generate_attentions_tiny_diagonal'), codes=codes, tokens=tokens,
                                 att=att)


def _forward_maps(dec, codes, x):
    """`Decoder.forward` -> (self (B, nl, H, T, T), cross (B, nl, H, T, S) or None, encoder (B, L_enc, H, S, S))"""
    dec.eval()
    with torch.no_grad():
        out = dec.forward(codes, x)
    ad, ae = out['attentions_decoder'], out['attentions_encoder']
    cross = None if ad[0]['a_cross'] is None else torch.stack([a['a_cross'] for a in ad], dim=1)
    return torch.stack([a['a_self_decoder'] for a in ad], dim=1), cross, torch.stack([a['a_self_encoder'] for a in ae], dim=1)


def _enc_rows(dec):
    t = torch.arange(dec.num_tokens_target)
    return (t // dec.num_channels * dec.num_channels) // dec.total_upscaling


def _maxdiff(a, b):
    return float((torch.as_tensor(a).double().cpu() - torch.as_tensor(b).double().cpu()).abs().max())


def _same_maps(a, b):
    assert a['layers'] == b['layers']
    for k in ('self_attns_decoder', 'attns_cross', 'self_attns_encoder'):
        if k in a or k in b:
            assert (a[k] is None) == (b[k] is None), k
            if a[k] is not None:                              # bit for bit, NaN rows included
                assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k


# ---- the tolerance's yardstick: code that exists without this feature --------------------------------------------------
def test_e_fwd(tiny, diagonal):
    worst = 0.0
    for fx in (tiny, diagonal):
        s, c, e = _forward_maps(fx.dec, fx.codes, T(fx.a['tokens']).cuda())
        worst = max(worst, _maxdiff(s, fx.a['self_attns_decoder']), _maxdiff(e[:, :, :, _enc_rows(fx.dec)], fx.a['self_attns_encoder']))
        if c is not None:
            worst = max(worst, _maxdiff(c, fx.a['attns_cross']))
    print(f'E_FWD measured {worst:.3e} (constant {E_FWD:.3e}, TOL {TOL:.3e})')
    assert worst <= E_FWD * 1.0001, worst                     # the constant is the measurement, not a guess below it


# ---- tokens and logp do not notice the maps ------------------------------------------------------------------------------
@pytest.mark.parametrize('sampling', [dict(top_k=1), dict(temperature=0.9, top_p=0.9)])
@pytest.mark.parametrize('use_graph', [True, False])
def test_tokens_and_logp_are_bit_identical(tiny, sampling, use_graph):
    dec, codes = tiny.dec, tiny.codes
    kw = dict(seed=5, use_graph=use_graph, **sampling)
    plain = dec.generate_from_codes(codes, **kw)
    tok, att = dec.generate_from_codes(codes, return_attentions=True, **kw)
    assert torch.equal(tok, plain) and att['layers'] == (0, 1)
    tok_l, logp = dec.generate_from_codes(codes, return_logp=True, **kw)
    tok2, logp2, att2 = dec.generate_from_codes(codes, return_logp=True, return_attentions=[1], **kw)
    assert torch.equal(tok_l, plain) and torch.equal(tok2, plain) and torch.equal(logp.view(torch.int32), logp2.view(torch.int32))
    assert att2['layers'] == (1,)
    assert torch.equal(att2['self_attns_decoder'][:, 0], att['self_attns_decoder'][:, 1])


def test_eager_equals_graph_and_subsets_equal_slices(tiny):
    dec, codes = tiny.dec, tiny.codes
    assert torch.equal(tiny.tokens.cpu(), T(tiny.g['tokens']))
    tok, eager = dec.generate_from_codes(codes, top_k=1, seed=0, use_graph=False, return_attentions=True)
    assert torch.equal(tok, tiny.tokens)
    _same_maps(eager, tiny.att)
    for sub in ((0,), (1,), (0, 1)):
        _, part = dec.generate_from_codes(codes, top_k=1, seed=0, return_attentions=list(sub))
        assert part['layers'] == sub
        for k in ('self_attns_decoder', 'attns_cross'):
            assert torch.equal(part[k], tiny.att[k][:, list(sub)]), (k, sub)
        assert torch.equal(part['self_attns_encoder'], tiny.att['self_attns_encoder'])
    for bad in ([2], [-1], []):
        with pytest.raises(ValueError):
            dec.generate_from_codes(codes, return_attentions=bad)


def test_shapes_zeros_and_no_nan(tiny):
    dec, att = tiny.dec, tiny.att
    B, nl, H = 3, len(dec.transformer.decoder.layers), dec.transformer.nhead
    Tt, S, U = dec.num_tokens_target, dec.num_tokens_source, dec.total_upscaling
    L_enc = len(dec.transformer.encoder.layers)
    s, c, e = att['self_attns_decoder'], att['attns_cross'], att['self_attns_encoder']
    assert tuple(s.shape) == (B, nl, H, Tt, Tt) and tuple(c.shape) == (B, nl, H, Tt, S) and tuple(e.shape) == (B, L_enc, H, S, S)
    assert all(m.dtype == torch.float32 and m.is_cuda for m in (s, c, e))
    assert not any(bool(torch.isnan(m).any()) for m in (s, c, e))
    above = torch.triu(torch.ones(Tt, Tt, dtype=torch.bool, device=s.device), diagonal=1)
    assert bool((s[..., above].view(torch.int32) == 0).all())                      # exactly +0.0 above the diagonal
    assert dec.cross_attention_type == 'anticausal'
    p = (torch.arange(Tt, device=s.device) // U).view(Tt, 1)
    forbidden = torch.arange(S, device=s.device).view(1, S) < p                     # anticausal keeps j >= p
    assert bool((c[..., forbidden].view(torch.int32) == 0).all())
    for m in (s, c):
        assert float((m.double().sum(-1) - 1).abs().max()) < 1e-5


# ---- against the reference's rows and against the full forward ---------------------------------------------------------
def test_maps_equal_the_reference(tiny):
    a, att = tiny.a, tiny.att
    errs = {'self_attns_decoder': _maxdiff(att['self_attns_decoder'], a['self_attns_decoder']),
            'attns_cross': _maxdiff(att['attns_cross'], a['attns_cross']),
            'self_attns_encoder': _maxdiff(att['self_attns_encoder'][:, :, :, _enc_rows(tiny.dec)], a['self_attns_encoder'])}
    print('generation maps against the reference fixture:', {k: f'{v:.3e}' for k, v in errs.items()}, f'TOL {TOL:.3e}')
    assert max(errs.values()) <= TOL, errs


def test_maps_equal_the_full_forward(tiny):
    s, c, e = _forward_maps(tiny.dec, tiny.codes, tiny.tokens)
    errs = (_maxdiff(tiny.att['self_attns_decoder'], s), _maxdiff(tiny.att['attns_cross'], c),
            _maxdiff(tiny.att['self_attns_encoder'], e))
    print('generation maps against Decoder.forward (self, cross, encoder):', [f'{v:.3e}' for v in errs], f'TOL {TOL:.3e}')
    assert max(errs) <= TOL, errs
    assert errs[2] == 0.0                                     # the encoder's maps come from the very same launches


def test_diagonal_decoder(diagonal):
    dec, att, a = diagonal.dec, diagonal.att, diagonal.a
    assert torch.equal(diagonal.tokens.cpu(), T(diagonal.g['tokens']))
    assert att['attns_cross'] is None and 'attns_cross' not in a
    assert not bool(torch.isnan(att['self_attns_decoder']).any())
    errs = (_maxdiff(att['self_attns_decoder'], a['self_attns_decoder']),
            _maxdiff(att['self_attns_encoder'][:, :, :, _enc_rows(dec)], a['self_attns_encoder']),
            _maxdiff(att['self_attns_decoder'], _forward_maps(dec, diagonal.codes, diagonal.tokens)[0]))
    print('diagonal: self / encoder against the fixture, self against Decoder.forward:', [f'{v:.3e}' for v in errs])
    assert max(errs) <= TOL, errs
    _, eager = dec.generate_from_codes(diagonal.codes, top_k=1, seed=0, use_graph=False, return_attentions=True)
    _same_maps(eager, att)


def test_num_decodings_and_chunks_of_64_rows(tiny):
    dec = tiny.dec
    g = torch.Generator().manual_seed(3)
    codes = torch.randint(0, dec.source_embeddings.weight.shape[0], (35, dec.num_tokens_source), generator=g).cuda()
    seeds = torch.arange(70, dtype=torch.int64) * 31 + 5
    tok, att = dec.generate_from_codes(codes, num_decodings=2, seed=seeds, return_attentions=[1])        # 70 rows: 64 + 6
    rep = codes.repeat_interleave(2, dim=0)
    assert torch.equal(tok, dec.generate_from_codes(codes, num_decodings=2, seed=seeds))
    assert att['self_attns_decoder'].shape[0] == 70 and not bool(torch.isnan(att['self_attns_decoder']).any())
    for rows in (slice(0, 64), slice(64, 70)):
        t2, a2 = dec.generate_from_codes(rep[rows], seed=seeds[rows], return_attentions=[1])
        assert torch.equal(t2, tok[rows])
        for k in ('self_attns_decoder', 'attns_cross', 'self_attns_encoder'):
            assert torch.equal(a2[k], att[k][rows]), k


# ---- Decoder.generate ---------------------------------------------------------------------------------------------------
def test_generate_api(tmp_path):
    dec, cfg = _api_decoder(tmp_path)
    nc, E = len(cfg['vocab']), cfg['events']
    Tt, S, H = dec.num_tokens_target, dec.num_tokens_source, dec.transformer.nhead
    nl = len(dec.transformer.decoder.layers)
    plain = dec.generate(temperature=1.0, batch_size=2, seed_set='val', seed=3)
    assert set(plain) == {'original', 'generation', 'codes', 'recoding'}
    assert not glob.glob(os.path.join(str(tmp_path), 'generations', '*.npz'))
    for f in glob.glob(os.path.join(str(tmp_path), 'generations', '*')):
        os.remove(f)
    out = dec.generate(temperature=1.0, batch_size=2, seed_set='val', seed=3, return_attentions=True)
    assert set(out) == {'original', 'generation', 'codes', 'recoding', 'attentions'}
    att = out['attentions']
    layer = min(2, nl - 1)
    assert att['layers'] == (layer,) and tuple(att['self_attns_decoder'].shape) == (2, 1, H, Tt, Tt)
    files = glob.glob(os.path.join(str(tmp_path), 'generations', '*'))
    npz = [f for f in files if f.endswith('_attentions.npz')]
    assert len(npz) == 1 and len(files) == 2 and npz[0][:-len('_attentions.npz')] + '.txt' in files
    z = np.load(npz[0])
    assert set(z.files) == {'attns_cross', 'self_attns_decoder', 'self_attns_encoder', 'layers'}
    assert z['attns_cross'].shape == (2, H, Tt, S) and z['self_attns_decoder'].shape == (2, H, Tt, Tt)
    assert z['self_attns_encoder'].shape == (2, H, Tt, S) and z['layers'].tolist() == [layer]
    assert np.array_equal(z['self_attns_decoder'], att['self_attns_decoder'][:, 0].cpu().numpy())
    assert np.array_equal(z['attns_cross'], att['attns_cross'][:, 0].cpu().numpy())
    enc = att['self_attns_encoder'][:, min(layer, att['self_attns_encoder'].shape[1] - 1)].cpu().numpy()
    U = dec.total_upscaling
    for t in range(Tt):
        assert np.array_equal(z['self_attns_encoder'][:, :, t], enc[:, :, (t // nc * nc) // U]), t
    both = dec.generate(temperature=1.0, batch_size=1, seed_set='val', seed=3, return_attentions=[0, 1])
    assert both['attentions']['layers'] == (0, 1)
    with pytest.raises(NotImplementedError, match='return_attentions'):
        dec.generate(temperature=1.0, seed_set='val', plot_attentions=True)
    with pytest.raises(ValueError):
        dec.generate(temperature=1.0, seed_set='val', return_attentions=[nl])


# ---- long form -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['generate_long_tiny_S3', 'generate_long_tiny_S4'])
def test_long_form(name):
    g = load_golden(name)
    cfg = D.make_cfg(**json.loads(str(g['cfg_json'])))
    dec = build_decoder(cfg, sub_state(g, 'sd'))
    dec.dataloader_generator = types.SimpleNamespace(dataset=types.SimpleNamespace(
        note2index_dicts=[{'START': int(s), 'END': int(e), 'XX': int(p)} for s, e, p in zip(g['start'], g['end'], g['pad'])]))
    codes = T(g['codes']).cuda()
    start, end, nd = int(g['code_index_start']), int(g['code_index_end']), int(g['num_decodings'])
    kw = dict(temperature=1.0, top_k=1, num_decodings=nd, code_index_start=start, code_index_end=end, seed=0)
    S, U, nc, Tt = dec.num_tokens_source, dec.total_upscaling, dec.num_channels, dec.num_tokens_target
    nb, epc, B = codes.shape[1], dec.num_events_per_code, codes.shape[0] * nd
    nl, H = len(dec.transformer.decoder.layers), dec.transformer.nhead
    tokens, att = dec.generate_from_code_long(codes, return_attentions=True, **kw)
    assert torch.equal(tokens.cpu(), T(g['tokens'])) and torch.equal(tokens, dec.generate_from_code_long(codes, **kw))
    s, c, ws = att['self_attns_decoder'], att['attns_cross'], att['window_start']
    assert set(att) == {'layers', 'self_attns_decoder', 'attns_cross', 'window_start'} and att['layers'] == tuple(range(nl))
    assert tuple(s.shape) == (B, nl, H, nb * U, Tt) and tuple(c.shape) == (B, nl, H, nb * U, S)
    assert torch.equal(ws, dec.attention_window_starts(nb, S, U, start, end)) and ws.dtype == torch.int64
    emitted = torch.zeros(nb * U, dtype=torch.bool)
    emitted[start * U:end * U] = True
    assert torch.equal(ws >= 0, emitted)
    assert bool(torch.isnan(s[:, :, :, ~emitted]).all()) and bool(torch.isnan(c[:, :, :, ~emitted]).all())
    assert not bool(torch.isnan(s[:, :, :, emitted]).any()) and not bool(torch.isnan(c[:, :, :, emitted]).any())
    for use_graph, graph_slides in ((True, False), (False, True), (False, False)):
        t2, a2 = dec.generate_from_code_long(codes, return_attentions=True, use_graph=use_graph, graph_slides=graph_slides, **kw)
        assert torch.equal(t2, tokens), (use_graph, graph_slides)
        _same_maps(a2, att)
        assert torch.equal(a2['window_start'], ws)
    tl, logp, a3 = dec.generate_from_code_long(codes, return_logp=True, return_attentions=[nl - 1], **kw)
    assert torch.equal(tl, tokens) and a3['layers'] == (nl - 1,)
    assert torch.equal(a3['attns_cross'].view(torch.int32), c[:, nl - 1:].view(torch.int32))
    # every emitted row against the full forward on the window it was emitted in
    chorale = dec.init_generation_chorale(nb * epc, start * epc).repeat(B, 1, 1)
    chorale[:, start * epc:end * epc] = tokens
    codes_rep = codes.repeat_interleave(nd, dim=0)
    worst = [0.0, 0.0]
    for w in sorted(set(ws[emitted].tolist())):
        fs, fc, _ = _forward_maps(dec, codes_rep[:, w:w + S], chorale[:, w * epc:w * epc + Tt // nc])
        pos = torch.nonzero(ws == w).reshape(-1)
        worst[0] = max(worst[0], _maxdiff(s[:, :, :, pos], fs[:, :, :, pos - w * U]))
        worst[1] = max(worst[1], _maxdiff(c[:, :, :, pos], fc[:, :, :, pos - w * U]))
    print(f'{name}: long-form maps against Decoder.forward on their windows (self, cross):', [f'{v:.3e}' for v in worst],
          f'TOL {TOL:.3e}')
    assert max(worst) <= TOL, worst


def test_size_guard(tiny):
    dec, codes = tiny.dec, tiny.codes
    with pytest.raises(ValueError, match='fewer layers'):
        dec.generate_from_codes(codes, return_attentions=True, max_attention_bytes=1)
    with pytest.raises(ValueError, match='fewer layers'):
        dec.generate_from_code_long(torch.zeros(1, 7, dtype=torch.int64), temperature=1.0, pad=[0] * 4, start=[0] * 4,
                                    return_attentions=True, max_attention_bytes=1)
    assert dec._check_attention_bytes(3, (0, 1), 48, True, 4 << 30) == 4 * 3 * 2 * (2 * 48 * 51 + 2 * 3 * 3)
