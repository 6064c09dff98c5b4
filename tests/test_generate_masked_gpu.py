"""Generation under per-position allowed-token sets (Decoder.generate_from_codes / generate_from_code_long /
reharmonise_tokens with `allowed`, `return_allowed_mass`; decoders/generation.py; vqcpc_decode_sample_masked) on the tiny
decoders of the generation fixtures (S = 3 or 4, U = 16), both cross blocks, captured and eager:
  (1) greedy parity with one full forward per token and the argmax over the allowed tokens (tests/masked_reference.py),
  (2) an all-true mask == no mask, a one-hot mask == the constraint,
  (3) allowed_mass == log of the allowed share of softmax(forward) on the produced tokens,
  (4) long form: chorale-coordinate masks at every window, allowed_mass written for exactly the generated range,
  (5) repeated rows and chunks, rhythm templates, validation, and the unchanged launch sequence of the default path."""
import numpy as np
import pytest
import torch

import constrained_reference as C
import masked_reference as MR
from test_generate_gpu import _golden_decoder, _random_inputs
from test_generate_long_gpu import _meta_dataset, _meta_ids, _random_codes

pytestmark = pytest.mark.gpu

NAMES = ['generate_greedy_tiny', 'generate_greedy_tiny_diagonal']
LONG = ['generate_long_tiny_S3', 'generate_long_tiny_S4']


def _decoder(name):
    dec = _golden_decoder(name)[0]
    dec.eval()
    return dec


def _vocab(dec):
    return [int(v) for v in dec.num_tokens_per_channel]


def _random_mask(dec, B, events, seed, density=0.5, vmax=None, reserve=0):
    """bool (B, events, channels, vmax): random everywhere (also past the vocabularies), at least one token of every voice's
    vocabulary (below V - reserve) allowed at every place."""
    g = torch.Generator().manual_seed(seed)
    vocab = _vocab(dec)
    vmax = max(vocab) if vmax is None else vmax
    m = torch.rand(B, events, len(vocab), vmax, generator=g) < density
    for c, v in enumerate(vocab):
        keep = torch.randint(0, v - reserve, (B, events), generator=g)
        m[:, :, c].scatter_(2, keep.unsqueeze(2), True)
    return m


def _one_hot(tokens, vmax):
    return torch.zeros(tokens.shape + (vmax,), dtype=torch.bool).scatter_(tokens.dim(), tokens.cpu().unsqueeze(-1), True)


def _inside(tokens, allowed):
    """Every token lies in its set."""
    return bool(allowed.to(tokens.device).gather(3, tokens.unsqueeze(3)).all())


def _random_tokens(dec, B, events, seed, reserve=0):
    g = torch.Generator().manual_seed(seed)
    return torch.cat([torch.randint(0, v - reserve, (B, events, 1), generator=g) for v in _vocab(dec)], dim=2).cuda()


# ---- 1. greedy parity with the slow loop ---------------------------------------------------------------------------
@pytest.mark.parametrize('name', NAMES)
def test_greedy_parity_with_the_forward_per_token_loop(name):
    """top_k = 1 under a seeded half-density mask, a quarter of the places forced to a token of their set: the tokens equal
    those of one full forward per token with the argmax over the allowed tokens.  The loop's smallest top-1 / top-2 gap over
    the allowed tokens must exceed twice the teacher-forced logits tolerance (each of the two logits may move by it)."""
    dec = _decoder(name)
    B, E = 2, dec.num_tokens_target // dec.num_channels
    codes, given = _random_inputs(dec, B, seed=161)
    allowed = _random_mask(dec, B, E, seed=162, vmax=max(_vocab(dec)) + 3)
    force = torch.rand(given.shape, generator=torch.Generator().manual_seed(163)) < 0.25
    cons = torch.where(force.cuda(), given, torch.full_like(given, -1))
    allowed |= _one_hot(given, allowed.shape[-1]) & force.unsqueeze(-1)                 # a forced token belongs to its set
    want, gap, rms, mass = MR.masked_greedy_loop(dec, codes, cons, allowed)
    print(f'{name}: smallest top-2 gap over the allowed tokens {gap:.3e}, 2 x tolerance {2 * C.TEACHER_FORCED_TOL * rms:.3e}')
    assert gap > 2 * C.TEACHER_FORCED_TOL * rms, (gap, rms)
    assert torch.equal(want[cons >= 0], cons[cons >= 0]) and _inside(want, allowed)
    for use_graph in (True, False):
        got, am = dec.generate_from_codes(codes, top_k=1, seed=0, constraint=cons, allowed=allowed, return_allowed_mass=True,
                                          use_graph=use_graph)
        assert torch.equal(got, want), use_graph
        worst = float((am.double().cpu() - mass).abs().max())
        print(f'{name} (graph {use_graph}): max |allowed_mass - loop| / rms = {worst / rms:.2e}')
        assert worst / rms < C.TEACHER_FORCED_TOL, (worst, rms)


# ---- 2. all-true, one-hot ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', NAMES)
def test_an_all_true_mask_changes_nothing_and_a_one_hot_mask_is_the_constraint(name):
    dec = _decoder(name)
    B, E, nc = 3, dec.num_tokens_target // dec.num_channels, dec.num_channels
    codes, given = _random_inputs(dec, B, seed=164)
    vmax = max(_vocab(dec))
    kw = dict(temperature=1.1, top_p=0.9, seed=7)
    hot = _one_hot(given, vmax)
    for use_graph in (True, False):
        a, lp = dec.generate_from_codes(codes, use_graph=use_graph, return_logp=True, **kw)
        for full in (torch.ones(B, E, nc, vmax, dtype=torch.bool), torch.ones(E, nc, 256, dtype=torch.bool)):
            b, lpb, am = dec.generate_from_codes(codes, use_graph=use_graph, return_logp=True, allowed=full,
                                                 return_allowed_mass=True, **kw)
            assert torch.equal(b, a) and torch.equal(lpb.view(torch.int32), lp.view(torch.int32)), use_graph
            assert am.shape == a.shape and am.dtype == torch.float32 and bool((am == 0).all())
        only = dec.generate_from_codes(codes, use_graph=use_graph, return_allowed_mass=True, **kw)   # the mass alone: all 0
        assert torch.equal(only[0], a) and bool((only[1] == 0).all())
        f, lpf = dec.generate_from_codes(codes, use_graph=use_graph, constraint=given, return_logp=True, **kw)
        h, lph, am = dec.generate_from_codes(codes, use_graph=use_graph, allowed=hot, return_logp=True, return_allowed_mass=True,
                                             **kw)
        assert torch.equal(f, given) and torch.equal(h, given), use_graph
        assert torch.equal(lph.view(torch.int32), lpf.view(torch.int32)), use_graph
        assert torch.allclose(am, lph, rtol=0, atol=1e-5), use_graph                  # a one-token set's mass is its probability


# ---- 3. the mass is the model's ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', NAMES)
def test_allowed_mass_is_the_allowed_share_of_the_full_forward(name):
    """Sampled under temperature / top-k inside a half-density mask: allowed_mass equals log(sum of softmax(forward(codes,
    tokens)) over the set) within the teacher-forced logits tolerance (same statistic: max |difference| / rms of the logits)."""
    dec = _decoder(name)
    B, E = 3, dec.num_tokens_target // dec.num_channels
    codes, _ = _random_inputs(dec, B, seed=165)
    allowed = _random_mask(dec, B, E, seed=166)
    for use_graph in (True, False):
        tokens, lp, am = dec.generate_from_codes(codes, temperature=1.3, top_k=4, seed=3, allowed=allowed, return_logp=True,
                                                 return_allowed_mass=True, use_graph=use_graph)
        assert _inside(tokens, allowed)
        assert bool(torch.isfinite(am).all()) and bool((am <= 0).all()) and bool((lp <= am + 1e-6).all())
        with torch.no_grad():
            full = dec.forward(codes, tokens)['weights_per_category']
        rms = float(torch.cat([f.reshape(-1) for f in full]).pow(2).mean().sqrt())
        worst = 0.0
        for c, f in enumerate(full):
            f = f.double()
            a = allowed[:, :, c, :f.shape[-1]].cuda()
            ref = torch.logsumexp(f.masked_fill(~a, -float('inf')), dim=-1) - torch.logsumexp(f, dim=-1)
            worst = max(worst, float((am[:, :, c].double() - ref).abs().max()))
        print(f'{name} (graph {use_graph}): max |allowed_mass - log share(forward)| / rms = {worst / rms:.2e}')
        assert worst / rms < C.TEACHER_FORCED_TOL, (worst, rms)


# ---- 4. long form --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', LONG)
def test_long_form_masks_in_chorale_coordinates(name):
    """nb = S + 4 codes, codes [1, nb) generated: the head window, middle windows on one captured slide, the tail."""
    dec = _decoder(name)
    pad, start = _meta_ids(dec)
    S, nc, epc = dec.num_tokens_source, dec.num_channels, dec.num_events_per_code
    nb, B = S + 4, 2
    codes = _random_codes(dec, B, nb, seed=167)
    vmax = max(_vocab(dec))
    kw = dict(temperature=1.0, code_index_start=1, seed=7, pad=pad, start=start)
    a = dec.generate_from_code_long(codes, **kw)
    assert a.shape == (B, (nb - 1) * epc, nc)
    # (a) an all-true mask: nothing changes, the mass is 0 over the returned range
    for use_graph in (True, False):
        b, am = dec.generate_from_code_long(codes, allowed=torch.ones(nb * epc, nc, vmax, dtype=torch.bool),
                                            return_allowed_mass=True, use_graph=use_graph, **kw)
        assert torch.equal(b, a) and am.shape == a.shape and bool((am == 0).all()), use_graph
    # (b) voice 1 pinned by one-hot sets over the whole sequence, a random mask elsewhere; an impossible set before the
    # generated range is ignored
    given = _random_tokens(dec, B, nb * epc, seed=168)
    allowed = _random_mask(dec, B, nb * epc, seed=169)
    allowed[:, :, 1] = _one_hot(given[:, :, 1], vmax)
    allowed[:, :epc] = False
    for use_graph in (True, False):
        out, lp, am = dec.generate_from_code_long(codes, allowed=allowed, return_logp=True, return_allowed_mass=True,
                                                  use_graph=use_graph, **kw)
        assert torch.equal(out[:, :, 1], given[:, epc:, 1]), use_graph
        assert _inside(out, allowed[:, epc:]), use_graph
        assert bool(torch.isfinite(am).all()) and bool((lp <= am + 1e-6).all())
        assert torch.allclose(am[:, :, 1], lp[:, :, 1], rtol=0, atol=1e-5)
    # repeated rows
    two = dec.generate_from_code_long(codes[:1], allowed=allowed[:1], num_decodings=2, **kw)
    assert torch.equal(two[:, :, 1], given[:1, epc:, 1].expand(2, -1)) and _inside(two, allowed[:1, epc:].expand(2, -1, -1, -1))


@pytest.mark.parametrize('name', LONG)
def test_long_form_allowed_mass_covers_exactly_the_generated_range(name):
    from vqcpc_bach_amd.decoders.generation import IncrementalDecoder
    from vqcpc_bach_amd.utils import STEP_LOCK
    dec = _decoder(name)
    pad, start = _meta_ids(dec)
    S, U, epc, nc = dec.num_tokens_source, dec.total_upscaling, dec.num_events_per_code, dec.num_channels
    nb, B = S + 4, 2
    codes = _random_codes(dec, B, nb, seed=170)
    c0, c1 = 2, nb - 1
    chorale = dec.init_generation_chorale(nb * epc, c0 * epc, pad=pad, start=start).reshape(1, -1).expand(B, -1)
    allowed = _random_mask(dec, B, nb * epc, seed=171)
    words = dec._allowed_words(allowed, B, nb * epc, c0 * epc, c1 * epc)
    assert words.shape == (B, nb * U, 8) and words.dtype == torch.int32
    for use_graph in (True, False):
        with STEP_LOCK, torch.no_grad():
            inc = IncrementalDecoder(dec, B)
            inc.start_long(codes, chorale, seeds=5, temperature=1.0, allowed=words, want_allowed_mass=True)
            assert inc.allowed.data_ptr() != words.data_ptr()                    # the stack's own copy
            out = inc.run_long(c0, c1, use_graph=use_graph).clone()
            lm = inc.logmass.clone()
        assert lm.shape == (B, nb * U)
        assert bool(torch.isnan(lm[:, :c0 * U]).all()) and bool(torch.isnan(lm[:, c1 * U:]).all())
        assert bool(torch.isfinite(lm[:, c0 * U:c1 * U]).all())
        assert _inside(out.view(B, nb * epc, nc)[:, c0 * epc:c1 * epc], allowed[:, c0 * epc:c1 * epc])
        assert torch.equal(out[:, :c0 * U], chorale[:, :c0 * U])


# ---- 5. rows, templates -------------------------------------------------------------------------------------------------
def test_repeated_rows_and_chunks_above_sixty_four_rows():
    dec = _decoder(NAMES[0])
    B, E = 33, dec.num_tokens_target // dec.num_channels
    codes, given = _random_inputs(dec, B, seed=172)
    allowed = _random_mask(dec, B, E, seed=173)
    allowed[:, :, 0] = _one_hot(given[:, :, 0], allowed.shape[-1])
    out, am = dec.generate_from_codes(codes, temperature=1.0, seed=9, num_decodings=2, allowed=allowed, return_allowed_mass=True)
    assert out.shape == (66, E, dec.num_channels) and am.shape == out.shape          # 64 + 2 rows: two chunks
    rep = allowed.repeat_interleave(2, dim=0)
    assert _inside(out, rep) and torch.equal(out[:, :, 0], given[:, :, 0].repeat_interleave(2, dim=0))
    assert bool(torch.isfinite(am).all()) and bool((am <= 0).all())
    shared = dec.generate_from_codes(codes, temperature=1.0, seed=9, num_decodings=2, allowed=allowed[0])
    assert _inside(shared, allowed[:1].expand(66, -1, -1, -1))


def _named_dataset(vocab):
    """The stub dataset of the long tests (START / END / XX last) with a names table: '__', 'rest', then a chromatic scale."""
    steps = ['C', 'C#', 'D', 'E-', 'E', 'F', 'F#', 'G', 'A-', 'A', 'B-', 'B']
    names = np.full((len(vocab), max(vocab)), '', dtype=object)
    for c, v in enumerate(vocab):
        pitched = [f'{steps[i % 12]}{3 + i // 12}' for i in range(v - 5)]
        names[c, :v] = ['__', 'rest'] + pitched + ['START', 'END', 'XX']
    return _meta_dataset(vocab), names.astype(str)


def test_reharmonise_tokens_keeps_the_rhythm_of_the_template():
    from vqcpc_bach_amd import templates as T
    dec, cfg, _ = _golden_decoder(NAMES[0])
    dec.eval()
    vocab, E = cfg['vocab'], cfg['events']
    dec.dataloader_generator, names = _named_dataset(vocab)
    kinds = T.token_kinds(names, vocab)
    events = 2 * E + E // 2 - 1                                                # not a multiple of the window, nor of a code
    x = _random_tokens(dec, 1, events, seed=174, reserve=3).cpu()
    x[0, ::3, 2] = 0                                                           # some more holds and rests
    x[0, 1::4, 3] = 1
    kw = dict(num_reharmonisations=2, temperature=1.0, top_p=0.9, seed=5)
    plain = dec.reharmonise_tokens(x, **kw)
    mask = T.rhythm_mask(x[0], kinds)
    out, am = dec.reharmonise_tokens(x, allowed=mask, return_allowed_mass=True, **kw)
    assert out.shape == plain.shape and am.shape == out.shape and bool(torch.isfinite(am).all())
    kx = kinds.long()[torch.arange(len(vocab)), x[0]]                          # (events, voices)
    for r in range(2):
        ko = kinds.long()[torch.arange(len(vocab)), out[r, :events].cpu()]
        assert torch.equal(ko == T.HOLD, kx == T.HOLD) and torch.equal(ko == T.REST, kx == T.REST), r
        assert torch.equal(ko >= 0, kx >= 0), r
        kp = kinds.long()[torch.arange(len(vocab)), plain[r, :events].cpu()]
        assert not torch.equal(kp == T.HOLD, kx == T.HOLD), r                   # without the mask the rhythm comes out changed
    # with a range on top: voice 0 (pitches 48 .. 53) stays inside three semitones
    both = mask & T.range_mask(kinds, [50, 0, 0, 0], [52, 127, 127, 127])
    out = dec.reharmonise_tokens(x, allowed=both, **kw)
    k0 = kinds.long()[0, out[:, :events, 0].cpu()]
    assert bool(((k0 < 0) | ((k0 >= 50) & (k0 <= 52))).all()) and bool((k0 >= 50).any())


# ---- 6. validation ---------------------------------------------------------------------------------------------------------
def test_bad_masks_raise_value_errors():
    dec = _decoder(NAMES[0])
    vocab = _vocab(dec)
    nc, E, S, epc = len(vocab), dec.num_tokens_target // dec.num_channels, dec.num_tokens_source, dec.num_events_per_code
    vmax = max(vocab)
    codes, _ = _random_inputs(dec, 2, seed=175)
    good = torch.ones(2, E, nc, vmax, dtype=torch.bool)
    bad = [good[:1], good[:, :-1], good[:, :, :-1], good[..., :-1], good.reshape(2, E, -1), good.long(), good.float(),
           torch.ones(2, E, nc, 257, dtype=torch.bool)]
    for mask in bad:
        with pytest.raises(ValueError, match='allowed'):
            dec.generate_from_codes(codes, allowed=mask, seed=1)
    empty = good.clone()
    empty[1, 3, 2] = False
    empty[1, 3, 2, vocab[2]:] = True                                            # only entries past voice 2's vocabulary
    with pytest.raises(ValueError, match=r'allowed: \(row 1, event 3, voice 2\) has no allowed token inside'):
        dec.generate_from_codes(codes, allowed=empty, seed=1)
    drained = good.clone()
    drained[0, 5, 1] = False
    drained[0, 5, 1, [2, 4]] = True
    with pytest.raises(ValueError, match=r'allowed: \(row 0, event 5, voice 1\) has no allowed token left after exclude_tokens'):
        dec.generate_from_codes(codes, allowed=drained, exclude_tokens=[[], [2, 4], [], []], seed=1)
    dec.generate_from_codes(codes, allowed=drained, exclude_tokens=[[], [2], [], []], seed=1)
    cons = torch.full((2, E, nc), -1, dtype=torch.int64)
    cons[1, 7, 3] = 6
    forbids = good.clone()
    forbids[1, 7, 3, 6] = False
    with pytest.raises(ValueError, match=r'allowed: \(row 1, event 7, voice 3\) is forced to token 6'):
        dec.generate_from_codes(codes, allowed=forbids, constraint=cons, seed=1)
    with pytest.raises(ValueError, match=r'allowed: \(row 0, event 7, voice 3\) is forced to token 6'):
        dec.generate_from_codes(codes[:1], allowed=forbids[1], constraint=cons[1:], seed=1)     # a shared mask
    # the long form: the same checks inside the generated range only
    pad, start = _meta_ids(dec)
    long_codes = _random_codes(dec, 2, 2 * S, seed=176)
    long_good = torch.ones(2, 2 * S * epc, nc, vmax, dtype=torch.bool)
    lkw = dict(temperature=1.0, pad=pad, start=start, seed=1)
    for mask in (good, long_good.long()):
        with pytest.raises(ValueError, match='allowed'):
            dec.generate_from_code_long(long_codes, allowed=mask, **lkw)
    inside = long_good.clone()
    inside[0, epc, 0] = False
    with pytest.raises(ValueError, match=rf'allowed: \(row 0, event {epc}, voice 0\) has no allowed token inside'):
        dec.generate_from_code_long(long_codes, allowed=inside, **lkw)
    outside = long_good.clone()
    outside[0, 0, 0] = False                                                    # outside [code_index_start, code_index_end): ignored
    dec.generate_from_code_long(long_codes, allowed=outside, code_index_start=1, **lkw)
    dec.dataloader_generator = _meta_dataset(vocab)
    x = _random_tokens(dec, 1, E + 2, seed=177, reserve=3)
    with pytest.raises(ValueError, match='allowed'):
        dec.reharmonise_tokens(x, 1, 1.0, allowed=torch.ones(E + 1, nc, vmax, dtype=torch.bool), seed=1)


# ---- 7. the default path's launches ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', NAMES)
def test_without_the_keywords_only_the_existing_samplers_are_launched(monkeypatch, name):
    from vqcpc_bach_amd import hip
    dec = _decoder(name)
    codes, _ = _random_inputs(dec, 2, seed=178)
    pad, start = _meta_ids(dec)
    names, real = [], hip.call

    def recorder(entry, *args):
        names.append(entry)
        return real(entry, *args)

    def launches(fn):
        del names[:]
        with monkeypatch.context() as m:
            m.setattr(hip, 'call', recorder)
            fn()
        torch.cuda.synchronize()
        return set(n for n in names if n.startswith('vqcpc_decode_sample'))
    long_codes = _random_codes(dec, 2, 5, seed=179)
    E, nc = dec.num_tokens_target // dec.num_channels, dec.num_channels
    free = torch.full((2, E, nc), -1, dtype=torch.int64)
    lkw = dict(temperature=1.0, seed=1, pad=pad, start=start)
    assert launches(lambda: dec.generate_from_codes(codes, seed=1, use_graph=False)) == {'vqcpc_decode_sample'}
    assert launches(lambda: dec.generate_from_codes(codes, seed=1)) == {'vqcpc_decode_sample'}
    assert launches(lambda: dec.generate_from_code_long(long_codes, use_graph=False, **lkw)) == {'vqcpc_decode_sample'}
    assert launches(lambda: dec.generate_from_codes(codes, seed=1, use_graph=False, constraint=free, return_logp=True)) == \
        {'vqcpc_decode_sample_constrained'}
    assert launches(lambda: dec.generate_from_code_long(long_codes, return_logp=True, **lkw)) == {'vqcpc_decode_sample_constrained'}
    full = torch.ones(E, nc, max(_vocab(dec)), dtype=torch.bool)
    assert launches(lambda: dec.generate_from_codes(codes, seed=1, use_graph=False, allowed=full)) == {'vqcpc_decode_sample_masked'}
    assert launches(lambda: dec.generate_from_codes(codes, seed=1, return_allowed_mass=True)) == {'vqcpc_decode_sample_masked'}
    assert launches(lambda: dec.generate_from_code_long(long_codes, return_allowed_mass=True, **lkw)) == \
        {'vqcpc_decode_sample_masked'}
