"""Generation with fixed tokens and token scores (Decoder.generate_from_codes / generate_from_code_long / reharmonise_tokens /
generate with `constraint`, `keep_voices`, `return_logp`; decoders/generation.py; vqcpc_decode_sample_constrained) on the tiny
decoders of the generation tests (S = 3, U = 16, T = 48), both cross blocks, captured and eager:
  (1) greedy parity with one full forward per token and the same forcing (tests/constrained_reference.py),
  (2) all-free == unconstrained, idempotence under forcing the run's own tokens,
  (3) logp == log_softmax of the full forward on the produced tokens (so forced tokens reach the K/V caches),
  (4) long form: chorale-coordinate constraints at every window, logp written for exactly the generated range,
  (5) kept voices, validation, and the unchanged launch sequence of the default path."""
import pytest
import torch

import constrained_reference as C
from test_generate_gpu import _api_decoder, _golden_decoder, _random_inputs
from test_generate_long_gpu import _meta_dataset, _meta_ids, _random_codes

pytestmark = pytest.mark.gpu

NAMES = ['decoder_tiny', 'decoder_tiny_diagonal']           # 'transformer_relative', 'transformer_relative_diagonal'


def _decoder(name):
    dec = _golden_decoder(name)[0]
    dec.eval()
    return dec


def _random_tokens(dec, B, events, seed, reserve=0):
    g = torch.Generator().manual_seed(seed)
    return torch.cat([torch.randint(0, int(v) - reserve, (B, events, 1), generator=g) for v in dec.num_tokens_per_channel],
                     dim=2).cuda()


def _free_like(x):
    return torch.full_like(x, -1)


# ---- 1. greedy parity with the slow loop ---------------------------------------------------------------------------
@pytest.mark.parametrize('name', NAMES)
def test_greedy_parity_with_the_forward_per_token_loop(name):
    """top_k = 1 and (a) voice 0 fixed, (b) a span of events fixed: the tokens equal those of one full forward per token
    with the same forcing.  The loop's smallest top-1 / top-2 gap must exceed twice the teacher-forced logits tolerance
    (each of the two logits may move by it), so a near tie can neither hide nor cause a failure."""
    dec = _decoder(name)
    B, E = 2, dec.num_tokens_target // dec.num_channels
    codes, given = _random_inputs(dec, B, seed=61)
    voice0, span = _free_like(given), _free_like(given)
    voice0[:, :, 0] = given[:, :, 0]
    span[:, 3:7] = given[:, 3:7]
    for label, cons in (('voice 0', voice0), ('events 3..6', span)):
        want, gap, rms = C.forced_greedy_loop(dec, codes, cons)
        print(f'{name}, {label}: smallest top-2 gap {gap:.3e}, 2 x tolerance {2 * C.TEACHER_FORCED_TOL * rms:.3e}')
        assert gap > 2 * C.TEACHER_FORCED_TOL * rms, (label, gap, rms)
        assert torch.equal(want[cons >= 0], cons[cons >= 0])
        for use_graph in (True, False):
            got = dec.generate_from_codes(codes, top_k=1, seed=0, constraint=cons, use_graph=use_graph)
            assert torch.equal(got, want), (label, use_graph)


# ---- 2. all-free, idempotence ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', NAMES)
def test_all_free_equals_the_unconstrained_run_and_forcing_its_own_tokens_changes_nothing(name):
    dec = _decoder(name)
    B = 3
    codes, _ = _random_inputs(dec, B, seed=62)
    kw = dict(temperature=1.1, top_p=0.9, seed=7)
    for use_graph in (True, False):
        a = dec.generate_from_codes(codes, use_graph=use_graph, **kw)
        free, lp = dec.generate_from_codes(codes, use_graph=use_graph, constraint=_free_like(a), return_logp=True, **kw)
        assert torch.equal(free, a), use_graph
        assert lp.shape == a.shape and lp.dtype == torch.float32 and bool(torch.isfinite(lp).all()) and bool((lp <= 0).all())
        half = torch.rand(a.shape, generator=torch.Generator().manual_seed(63)).cuda() < 0.5
        again = dec.generate_from_codes(codes, use_graph=use_graph, constraint=torch.where(half, a, _free_like(a)), **kw)
        assert torch.equal(again, a), use_graph
    two = dec.generate_from_codes(codes[:1], num_decodings=2, constraint=torch.where(half, a, _free_like(a))[:1], **kw)
    assert torch.equal(two[0][half[0]], a[0][half[0]]) and torch.equal(two[1][half[0]], a[0][half[0]])     # rows repeated


# ---- 3. the scores are the model's ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', NAMES)
def test_logp_is_the_log_softmax_of_the_full_forward(name):
    """Half of the positions forced to arbitrary tokens, the rest sampled under temperature / top-k: logp equals
    log_softmax(forward(codes, tokens)) at the tokens within the teacher-forced logits tolerance (same statistic: max
    |difference| / rms of the forward logits).  A forced token that did not reach the caches would move every later logit."""
    dec = _decoder(name)
    B = 3
    codes, given = _random_inputs(dec, B, seed=64)
    half = torch.rand(given.shape, generator=torch.Generator().manual_seed(65)).cuda() < 0.5
    cons = torch.where(half, given, _free_like(given))
    for use_graph in (True, False):
        tokens, lp = dec.generate_from_codes(codes, temperature=1.3, top_k=4, seed=3, constraint=cons, return_logp=True,
                                             use_graph=use_graph)
        assert torch.equal(tokens[half], given[half])
        with torch.no_grad():
            full = dec.forward(codes, tokens)['weights_per_category']
        rms = float(torch.cat([f.reshape(-1) for f in full]).pow(2).mean().sqrt())
        worst = 0.0
        for c, f in enumerate(full):
            ref = torch.log_softmax(f.double(), dim=-1).gather(2, tokens[:, :, c:c + 1]).squeeze(2)
            worst = max(worst, float((lp[:, :, c].double() - ref).abs().max()))
        print(f'{name} (graph {use_graph}): max |logp - log_softmax(forward)| / rms = {worst / rms:.2e}')
        assert worst / rms < C.TEACHER_FORCED_TOL, (worst, rms)


# ---- 4. long form --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', NAMES)
def test_long_form_constraints_in_chorale_coordinates(name):
    """nb = 7 codes of an S = 3 model, codes [1, 7) generated: a head window (code 1 is the first middle code of window 0),
    five middle windows on one captured slide, the tail."""
    dec = _decoder(name)
    pad, start = _meta_ids(dec)
    nb, B, nc, epc = 7, 2, dec.num_channels, dec.num_events_per_code
    codes = _random_codes(dec, B, nb, seed=66)
    kw = dict(temperature=1.0, code_index_start=1, seed=7, pad=pad, start=start)
    a = dec.generate_from_code_long(codes, **kw)
    assert a.shape == (B, (nb - 1) * epc, nc)
    chorale_a = torch.cat([torch.zeros(B, epc, nc, dtype=torch.int64).cuda(), a], dim=1)
    # (a) the run's own voice 0 forced over the whole range, other tokens forced outside it (ignored): nothing changes
    own = torch.full((B, nb * epc, nc), -1, dtype=torch.int64).cuda()
    own[:, :, 0] = chorale_a[:, :, 0]
    own[:, :epc] = 2
    for use_graph in (True, False):
        b, lp = dec.generate_from_code_long(codes, constraint=own, return_logp=True, use_graph=use_graph, **kw)
        assert torch.equal(b, a), use_graph
        assert lp.shape == a.shape and lp.dtype == torch.float32 and bool(torch.isfinite(lp).all())
    # (b) arbitrary tokens for voice 1 in every window; one changed token: everything before it is the unconstrained run's
    given = _random_tokens(dec, B, nb * epc, seed=67)
    fixed = torch.full_like(own, -1)
    fixed[:, :, 1] = given[:, :, 1]
    out = dec.generate_from_code_long(codes, constraint=fixed, **kw)
    assert torch.equal(out[:, :, 1], given[:, epc:, 1])
    e0, v0 = 4 * epc + 1, 2                                                    # a middle window's event, chorale coordinates
    one = torch.full_like(own, -1)
    one[:, e0, v0] = (chorale_a[:, e0, v0] + 1) % int(dec.num_tokens_per_channel[v0])
    out = dec.generate_from_code_long(codes, constraint=one, **kw)
    flat_a, flat = a.reshape(B, -1), out.reshape(B, -1)
    p0 = (e0 - epc) * nc + v0
    assert torch.equal(flat[:, :p0], flat_a[:, :p0]) and torch.equal(flat[:, p0], one[:, e0, v0])
    # repeated rows
    two = dec.generate_from_code_long(codes[:1], constraint=fixed[:1], num_decodings=2, **kw)
    assert torch.equal(two[:, :, 1], given[:1, epc:, 1].expand(2, -1))


@pytest.mark.parametrize('name', NAMES)
def test_long_form_logp_covers_exactly_the_generated_range(name):
    from vqcpc_bach_amd.decoders.generation import IncrementalDecoder
    from vqcpc_bach_amd.utils import STEP_LOCK
    dec = _decoder(name)
    pad, start = _meta_ids(dec)
    nb, B, U, epc = 7, 2, dec.total_upscaling, dec.num_events_per_code
    codes = _random_codes(dec, B, nb, seed=68)
    c0, c1 = 2, 6
    chorale = dec.init_generation_chorale(nb * epc, c0 * epc, pad=pad, start=start).reshape(1, -1).expand(B, -1)
    given = _random_tokens(dec, B, nb * epc, seed=69).reshape(B, -1)
    cons = torch.where(torch.rand(given.shape, generator=torch.Generator().manual_seed(70)).cuda() < 0.5, given,
                       torch.full_like(given, -1))
    for use_graph in (True, False):
        with STEP_LOCK, torch.no_grad():
            inc = IncrementalDecoder(dec, B)
            inc.start_long(codes, chorale, seeds=5, temperature=1.0, constraint=cons, want_logp=True)
            out = inc.run_long(c0, c1, use_graph=use_graph).clone()
            lp = inc.logp.clone()
        assert lp.shape == (B, nb * U)
        assert bool(torch.isnan(lp[:, :c0 * U]).all()) and bool(torch.isnan(lp[:, c1 * U:]).all())
        assert bool(torch.isfinite(lp[:, c0 * U:c1 * U]).all())
        gen_range = slice(c0 * U, c1 * U)
        forced = cons[:, gen_range] >= 0
        assert torch.equal(out[:, gen_range][forced], cons[:, gen_range][forced])
        assert torch.equal(out[:, :c0 * U], chorale[:, :c0 * U])                # the constraint outside the range is not applied


# ---- 5. kept voices --------------------------------------------------------------------------------------------------------
def test_reharmonise_tokens_keeps_the_given_voices():
    dec, cfg, _ = _golden_decoder('decoder_tiny')
    dec.eval()
    vocab, E = cfg['vocab'], cfg['events']
    nc = len(vocab)
    dec.dataloader_generator = _meta_dataset(vocab)
    events = 2 * E + E // 2 - 1                                                # not a multiple of the window, nor of a code
    x = _random_tokens(dec, 1, events, seed=71, reserve=3).cpu()
    kw = dict(num_reharmonisations=2, temperature=1.0, top_p=0.9, seed=5)
    plain = dec.reharmonise_tokens(x, **kw)
    kept = dec.reharmonise_tokens(x, keep_voices=(0,), **kw)
    assert kept.shape == plain.shape and kept.shape[1] >= events
    for r in range(2):
        assert torch.equal(kept[r, :events, 0].cpu(), x[0, :, 0]), r
        assert not torch.equal(plain[r, :events, 0].cpu(), x[0, :, 0]), r         # without it the soprano comes out changed
        assert not torch.equal(kept[r, :events, 1:].cpu(), x[0, :, 1:]), r
    both = dec.reharmonise_tokens(x, keep_voices=[3, 0], exclude_meta_symbols=True, **kw)
    assert torch.equal(both[:, :events, [0, 3]].cpu(), x[:, :, [0, 3]].expand(2, -1, -1))
    (tokens, lp), c0, c1, n = dec.reharmonise_tokens(x, keep_voices=(0,), return_logp=True, return_bounds=True, **kw)
    assert torch.equal(tokens, kept) and lp.shape == kept.shape and bool(torch.isfinite(lp).all())
    assert tokens.shape[1] == (c1 - c0) * dec.num_events_per_code and n == 5 * dec.num_tokens_source


def test_generate_keeps_the_given_voices(tmp_path):
    dec, cfg = _api_decoder(tmp_path)
    out = dec.generate(temperature=1.0, batch_size=2, seed_set='val', seed=3, keep_voices=(0, 2))
    assert torch.equal(out['generation'][:, :, [0, 2]], out['original'][:, :, [0, 2]])
    assert not torch.equal(out['generation'][:, :, [1, 3]], out['original'][:, :, [1, 3]])


# ---- 6. validation ---------------------------------------------------------------------------------------------------------
def test_bad_constraints_raise_value_errors(tmp_path):
    dec, cfg = _api_decoder(tmp_path)
    dec.eval()
    vocab = cfg['vocab']
    nc, E, S, epc = len(vocab), cfg['events'], dec.num_tokens_source, dec.num_events_per_code
    codes, _ = _random_inputs(dec, 2, seed=72)
    good = torch.full((2, E, nc), -1, dtype=torch.int64)
    pad, start = _meta_ids(dec)
    long_codes = _random_codes(dec, 2, 2 * S, seed=73)
    bad = [good[:1], good[:, :-1], good[:, :, :-1], good.reshape(2, -1), good.to(torch.int32), good.float()]
    over = good.clone()
    over[1, 3, 2] = vocab[2]                                                    # one past voice 2's vocabulary
    for cons in bad + [over]:
        with pytest.raises(ValueError, match='constraint'):
            dec.generate_from_codes(codes, constraint=cons, seed=1)
    long_good = torch.full((2, 2 * S * epc, nc), -1, dtype=torch.int64)
    long_over = long_good.clone()
    long_over[0, epc, 0] = vocab[0]
    for cons in (good, long_good.to(torch.int32), long_over):
        with pytest.raises(ValueError, match='constraint'):
            dec.generate_from_code_long(long_codes, temperature=1.0, constraint=cons, pad=pad, start=start, seed=1)
    outside = long_good.clone()
    outside[0, 0, 0] = vocab[0]                                                 # outside [code_index_start, code_index_end): ignored
    dec.generate_from_code_long(long_codes, temperature=1.0, constraint=outside, code_index_start=1, pad=pad, start=start, seed=1)
    for voices in ((nc,), (-1,), (0, 7)):
        with pytest.raises(ValueError, match='keep_voices'):
            dec.generate(temperature=1.0, seed_set='val', seed=1, keep_voices=voices)
    dec.dataloader_generator = _meta_dataset(vocab)
    x = _random_tokens(dec, 1, E + 2, seed=74, reserve=3)
    with pytest.raises(ValueError, match='keep_voices'):
        dec.reharmonise_tokens(x, 1, 1.0, keep_voices=(nc,))
    with pytest.raises(ValueError, match='keep_voices'):
        dec.reharmonise_tokens(x, 1, 1.0, keep_voices=(0,), constraint=torch.zeros(1))
    x_over = x.clone()
    x_over[0, 1, 1] = vocab[1]
    with pytest.raises(ValueError, match='constraint'):
        dec.reharmonise_tokens(x_over, 1, 1.0, keep_voices=(1,), seed=1)


# ---- 7. the default path's launches ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', NAMES)
def test_the_default_path_launches_the_plain_sampler(monkeypatch, name):
    from vqcpc_bach_amd import hip
    dec = _decoder(name)
    codes, _ = _random_inputs(dec, 2, seed=75)
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
    long_codes = _random_codes(dec, 2, 5, seed=76)
    free = torch.full((2, dec.num_tokens_target // dec.num_channels, dec.num_channels), -1, dtype=torch.int64)
    assert launches(lambda: dec.generate_from_codes(codes, seed=1, use_graph=False)) == {'vqcpc_decode_sample'}
    assert launches(lambda: dec.generate_from_codes(codes, seed=1)) == {'vqcpc_decode_sample'}
    assert launches(lambda: dec.generate_from_code_long(long_codes, temperature=1.0, seed=1, pad=pad, start=start,
                                                        use_graph=False)) == {'vqcpc_decode_sample'}
    assert launches(lambda: dec.generate_from_codes(codes, seed=1, use_graph=False, constraint=free)) == \
        {'vqcpc_decode_sample_constrained'}
    assert launches(lambda: dec.generate_from_codes(codes, seed=1, use_graph=False, return_logp=True)) == \
        {'vqcpc_decode_sample_constrained'}
    assert launches(lambda: dec.generate_from_code_long(long_codes, temperature=1.0, seed=1, pad=pad, start=start,
                                                        return_logp=True)) == {'vqcpc_decode_sample_constrained'}
