"""Particle resampling in generation (Decoder.generate_from_codes / generate_from_code_long / reharmonise_tokens with
`particles`, `resample_threshold`, `return_particles`; decoders/generation.py `_resample`; csrc/particles.hip) on the tiny decoders
of the generation tests (S = 3, U = 16, T = 48; long form nb = 5: head, head -> middle without a slide, middle slides, tail),
captured and eager:
  (1) resample_threshold = 0 is the plain run with num_decodings * P rows, bit for bit, and its weights are the softmax of the
      summed scores; no constraint: nothing moves, evidence 0; everything forced: the evidence is the sum of logp;
  (2) resample_threshold = 1: forced tokens kept, every row's logp bit-equal to a plain run forcing the row's own tokens (the
      moved caches are the ancestor's bits), the recorded ancestors are the reference's function of the recorded weights,
      captured == eager;
  (3) chunks of whole groups, reharmonise_tokens, the refusals, and the default path's unchanged launches."""
import numpy as np
import pytest
import torch

import particles_reference as R
from test_generate_gpu import _golden_decoder, _random_inputs
from test_generate_long_gpu import _meta_dataset, _meta_ids, _random_codes
from test_generate_masked_gpu import _random_mask, _random_tokens

pytestmark = pytest.mark.gpu

NAMES = ['decoder_tiny', 'decoder_tiny_diagonal']
NB = 5


def _decoder(name):
    dec = _golden_decoder(name)[0]
    dec.eval()
    return dec


def _voice0(given):
    cons = torch.full_like(given, -1)
    cons[:, :, 0] = given[:, :, 0]
    return cons


def _span(given, e0, e1):
    cons = torch.full_like(given, -1)
    cons[:, e0:e1] = given[:, e0:e1]
    return cons


def _seeds(seed, rows):
    from vqcpc_bach_amd.transformer.incremental import row_seeds
    return row_seeds(seed, rows).numpy()


def _check_history(info, seeds, P, threshold, codes_generated, final_forced):
    """The recorded ancestors are the reference's function of the recorded wn / ess and of u, code by code; codes outside
    `codes_generated` keep their filler.  -> the number of rows that moved."""
    anc, wn, ess = (info[k].cpu().numpy() for k in ('ancestors', 'wn', 'ess'))
    rows = anc.shape[1]
    moved = 0
    for c in range(anc.shape[0]):
        if c not in codes_generated:
            assert (anc[c] == -1).all() and np.isnan(wn[c]).all() and np.isnan(ess[c]).all(), c
            continue
        last = c == codes_generated[-1]
        for g in range(rows // P):
            sl = slice(g * P, (g + 1) * P)
            assert np.isfinite(wn[c, sl]).all() and abs(float(wn[c, sl].sum()) - 1.0) < 1e-5
            assert ess[c, g] == R.ess_of(wn[c, sl])
            thr, force = (threshold, False) if not last else ((0.0, False) if not final_forced else (threshold, True))
            want = np.arange(g * P, (g + 1) * P)
            if R.decide(ess[c, g], thr, P, force, False):
                want = g * P + R.systematic_ancestors(wn[c, sl], R.uniform(seeds[g * P], c))
            assert np.array_equal(anc[c, sl], want), (c, g, anc[c, sl], want)
            moved += int((anc[c, sl] != np.arange(g * P, (g + 1) * P)).sum())
    return moved


# ---- 1. threshold 0, nothing to weigh, everything forced ------------------------------------------------------------------
@pytest.mark.parametrize('name', NAMES)
def test_threshold_zero_is_the_plain_run_with_P_times_the_rows(name):
    dec = _decoder(name)
    B, nd, P = 2, 2, 3
    E, nc = dec.num_tokens_target // dec.num_channels, dec.num_channels
    codes, given = _random_inputs(dec, B, seed=301)
    cons = _voice0(given)
    allowed = _random_mask(dec, B, E, seed=302)
    allowed.scatter_(3, given.cpu().unsqueeze(3), True)                       # a forced token lies in its set
    kw = dict(temperature=1.0, seed=9, constraint=cons, allowed=allowed, return_logp=True, return_allowed_mass=True)
    for use_graph in (True, False):
        tok, lp, mass = dec.generate_from_codes(codes, num_decodings=nd * P, use_graph=use_graph, **kw)
        ptok, plp, pmass, info = dec.generate_from_codes(codes, num_decodings=nd, particles=P, resample_threshold=0.0,
                                                         return_particles=True, use_graph=use_graph, **kw)
        assert torch.equal(ptok, tok) and torch.equal(plp.view(torch.int32), lp.view(torch.int32))
        assert torch.equal(pmass.view(torch.int32), mass.view(torch.int32))
        rows = B * nd * P
        assert info['weights'].shape == (B * nd, P) and info['log_evidence'].shape == (B * nd,)
        assert info['ancestors'].shape == (dec.num_tokens_source, rows) and info['ancestors'].dtype == torch.int32
        assert torch.equal(info['ancestors'].cpu(), torch.arange(rows, dtype=torch.int32).expand(dec.num_tokens_source, -1))
        # the weights: softmax over the group of the summed forced logp and free logmass (float64 sums of the fp32 scores)
        forced = cons.repeat_interleave(nd * P, dim=0) >= 0
        score = torch.where(forced, lp, mass).double().reshape(rows, -1).cpu().numpy()
        total, mag = score.sum(axis=1), np.abs(score).sum(axis=1)
        worst = 0.0
        for g in range(B * nd):
            sl = slice(g * P, (g + 1) * P)
            wn64, _, inc64, dmax = R.group_weights64(total[sl])
            sum_err = score.shape[1] * R.EPS * mag[sl].max()                     # the fp32 running sum of a row's scores
            bound = R.wn_bound(wn64, dmax, P) + 2.0 * sum_err * wn64
            worst = max(worst, float((np.abs(info['weights'][g].cpu().numpy() - wn64) / bound).max()))
            b_ev = R.inc_bound(float(total[sl].max()), inc64, dmax, P) + sum_err
            worst = max(worst, abs(float(info['log_evidence'][g]) - inc64) / b_ev)
        print(f'{name} (graph {use_graph}): weights and evidence, worst error / bound {worst:.3f}')
        assert worst <= 1.0
        # without return_particles the survivors come back in the shapes of a call without particles
        stok, slp, smass = dec.generate_from_codes(codes, num_decodings=nd, particles=P, resample_threshold=0.0,
                                                   use_graph=use_graph, **kw)
        assert stok.shape == (B * nd, E, nc) and slp.shape == smass.shape == stok.shape
        assert torch.equal(stok[:, :, 0], given.repeat_interleave(nd, dim=0)[:, :, 0])


def test_without_constraint_nothing_moves_and_the_evidence_is_zero():
    dec = _decoder(NAMES[0])
    pad, start = _meta_ids(dec)
    codes, _ = _random_inputs(dec, 2, seed=303)
    plain = dec.generate_from_codes(codes, num_decodings=4, seed=4)
    tok, info = dec.generate_from_codes(codes, particles=4, resample_threshold=1.0, return_particles=True, seed=4)
    assert torch.equal(tok, plain)
    assert bool((info['log_evidence'] == 0).all()) and bool((info['weights'] == 0.25).all())
    assert torch.equal(info['ancestors'].cpu(), torch.arange(8, dtype=torch.int32).expand(dec.num_tokens_source, -1))
    first = dec.generate_from_codes(codes, particles=4, resample_threshold=1.0, seed=4)
    assert torch.equal(first, plain[::4])
    long_codes = _random_codes(dec, 2, NB, seed=304)
    kw = dict(temperature=1.0, seed=4, pad=pad, start=start, code_index_start=1)
    plain = dec.generate_from_code_long(long_codes, num_decodings=2, **kw)
    tok, info = dec.generate_from_code_long(long_codes, particles=2, resample_threshold=1.0, return_particles=True, **kw)
    assert torch.equal(tok, plain) and bool((info['log_evidence'] == 0).all())
    assert bool((info['ancestors'][0] == -1).all()) and bool((info['ancestors'][1:] >= 0).all())


@pytest.mark.parametrize('name', NAMES)
def test_with_everything_forced_the_evidence_is_the_sum_of_logp(name):
    dec = _decoder(name)
    B, P = 2, 2
    codes, given = _random_inputs(dec, B, seed=305)
    tok, lp, info = dec.generate_from_codes(codes, constraint=given, particles=P, resample_threshold=1.0, return_logp=True,
                                            return_particles=True, seed=1)
    assert torch.equal(tok, given.repeat_interleave(P, dim=0))
    total = lp.double().reshape(B * P, -1).sum(dim=1).cpu().numpy()
    mag = float(lp.double().abs().reshape(B * P, -1).sum(dim=1).max())
    assert np.array_equal(total[0::2], total[1::2])                           # the particles of a group are the same row
    # the running fp32 sum of T scores, and per code one increment (equal weights: wn = 1 / 2 exactly, ess = 2, no resampling
    # below the strict threshold, so the last code's increment carries everything)
    bound = lp[0].numel() * R.EPS * mag + R.inc_bound(float(np.abs(total).max()), float(np.abs(total).max()), 0.0, P)
    err = np.abs(info['log_evidence'].double().cpu().numpy() - total[0::2]).max()
    print(f'{name}: |log_evidence - sum logp| = {err:.3e}, bound {bound:.3e}')
    assert err <= bound
    assert bool((info['weights'] == 0.5).all())


# ---- 2. threshold 1: rows really move ---------------------------------------------------------------------------------------
def _own_tokens_logp(dec, codes_rows, tokens, long_kw=None):
    """return_logp of a plain run (no particles, as many rows) that forces every row's own tokens."""
    if long_kw is None:
        out, lp = dec.generate_from_codes(codes_rows, constraint=tokens, return_logp=True, seed=0)
    else:
        c0, c1, nb = long_kw['code_index_start'], long_kw['code_index_end'], codes_rows.shape[1]
        epc = dec.num_events_per_code
        whole = torch.full((tokens.shape[0], nb * epc, tokens.shape[2]), -1, dtype=torch.int64, device=tokens.device)
        whole[:, c0 * epc:c1 * epc] = tokens
        out, lp = dec.generate_from_code_long(codes_rows, constraint=whole, return_logp=True, seed=0, **long_kw)
    assert torch.equal(out, tokens)
    return lp


@pytest.mark.parametrize('shape', ['voice0', 'span'])
@pytest.mark.parametrize('name', NAMES)
def test_resampled_rows_carry_their_ancestors_bits_fixed_window(name, shape):
    dec = _decoder(name)
    B, P, S = 2, 16, dec.num_tokens_source
    E = dec.num_tokens_target // dec.num_channels
    codes, given = _random_inputs(dec, B, seed=311)
    cons = _voice0(given) if shape == 'voice0' else _span(given, E // 2, E // 2 + 3)       # events of the second code
    kw = dict(temperature=1.0, seed=21, constraint=cons, particles=P, resample_threshold=1.0, return_logp=True)
    seeds = _seeds(21, B * P)
    runs = {}
    for use_graph in (True, False):
        tok, lp, info = dec.generate_from_codes(codes, return_particles=True, use_graph=use_graph, **kw)
        stok, slp = dec.generate_from_codes(codes, use_graph=use_graph, **kw)
        runs[use_graph] = (tok, lp, info['ancestors'], info['wn'], stok, slp)
        forced = cons.repeat_interleave(P, dim=0) >= 0
        assert torch.equal(tok[forced], cons.repeat_interleave(P, dim=0)[forced])
        assert torch.equal(stok[cons >= 0], cons[cons >= 0])
        moved = _check_history(info, seeds, P, 1.0, list(range(S)), final_forced=False)
        print(f'{name}, {shape} (graph {use_graph}): {moved} rows moved in {S - 1} resamplings')
        assert moved > 0
        own = _own_tokens_logp(dec, codes.repeat_interleave(P, dim=0), tok)
        assert torch.equal(lp.view(torch.int32), own.view(torch.int32))
        own = _own_tokens_logp(dec, codes.repeat_interleave(P, dim=0), stok.repeat_interleave(P, dim=0))[::P]
        assert torch.equal(slp.view(torch.int32), own.view(torch.int32))
    for a, b in zip(runs[True], runs[False]):
        assert torch.equal(torch.nan_to_num(a.float(), nan=-7.0), torch.nan_to_num(b.float(), nan=-7.0))


@pytest.mark.parametrize('shape', ['voice0', 'span'])
@pytest.mark.parametrize('name', NAMES)
def test_resampled_rows_carry_their_ancestors_bits_long_form(name, shape):
    dec = _decoder(name)
    pad, start = _meta_ids(dec)
    B, P, epc = 2, 16, dec.num_events_per_code
    codes = _random_codes(dec, B, NB, seed=312)
    given = _random_tokens(dec, B, NB * epc, seed=313, reserve=3)
    cons = _voice0(given) if shape == 'voice0' else _span(given, 3 * epc, 4 * epc)          # the fixed bars after a free span
    long_kw = dict(temperature=1.0, pad=pad, start=start, code_index_start=1, code_index_end=NB)
    kw = dict(seed=22, constraint=cons, particles=P, resample_threshold=1.0, return_logp=True, **long_kw)
    seeds = _seeds(22, B * P)
    gen = slice(epc, NB * epc)
    runs = {}
    for use_graph in (True, False):
        tok, lp, info = dec.generate_from_code_long(codes, return_particles=True, use_graph=use_graph, **kw)
        stok, slp = dec.generate_from_code_long(codes, use_graph=use_graph, **kw)
        runs[use_graph] = (tok, lp, info['ancestors'], info['wn'], stok, slp)
        want = cons[:, gen].repeat_interleave(P, dim=0)
        assert torch.equal(tok[want >= 0], want[want >= 0])
        assert torch.equal(stok[cons[:, gen] >= 0], cons[:, gen][cons[:, gen] >= 0])
        assert info['ancestors'].shape == (NB, B * P)
        moved = _check_history(info, seeds, P, 1.0, list(range(1, NB)), final_forced=False)
        print(f'{name}, {shape} (graph {use_graph}): {moved} rows moved in {NB - 2} resamplings')
        assert moved > 0
        own = _own_tokens_logp(dec, codes.repeat_interleave(P, dim=0), tok, long_kw)
        assert torch.equal(lp.view(torch.int32), own.view(torch.int32))
        own = _own_tokens_logp(dec, codes.repeat_interleave(P, dim=0), stok.repeat_interleave(P, dim=0), long_kw)[::P]
        assert torch.equal(slp.view(torch.int32), own.view(torch.int32))
    for a, b in zip(runs[True], runs[False]):
        assert torch.equal(torch.nan_to_num(a.float(), nan=-7.0), torch.nan_to_num(b.float(), nan=-7.0))


def test_the_final_forced_resampling_returns_a_draw_from_the_final_weights():
    """The stack itself, so that the forced launch's history is visible: its ancestors are the reference's function of its
    weights, and row 0 of every group ends as the ancestor's tokens and scores."""
    from vqcpc_bach_amd.decoders.generation import IncrementalDecoder
    from vqcpc_bach_amd.utils import STEP_LOCK
    dec = _decoder(NAMES[0])
    B, P, S = 2, 8, dec.num_tokens_source
    codes, given = _random_inputs(dec, B, seed=314)
    cons = _voice0(given).reshape(B, -1).repeat_interleave(P, dim=0)
    seeds = _seeds(23, B * P)
    outs = {}
    for final in (False, True):
        with STEP_LOCK, torch.no_grad():
            inc = IncrementalDecoder(dec, B * P)
            inc.prefill(codes.repeat_interleave(P, dim=0))
            inc.start(seeds=torch.from_numpy(seeds), constraint=cons, particles=P, resample_threshold=0.5, final_resample=final)
            tokens = inc.run(use_graph=False).clone()
            outs[final] = (tokens, inc.logp.clone(), inc.particle_results())
        _check_history(outs[final][2], seeds, P, 0.5, list(range(S)), final_forced=final)
    tok0, lp0, info0 = outs[False]
    tok1, lp1, info1 = outs[True]
    last = info1['ancestors'][S - 1].cpu().long()
    assert torch.equal(tok1.cpu(), tok0.cpu()[last]) and torch.equal(lp1.cpu().view(torch.int32), lp0.cpu()[last].view(torch.int32))
    assert torch.equal(info1['wn'][:S - 1].view(torch.int32), info0['wn'][:S - 1].view(torch.int32))
    ev0, ev1 = info0['log_evidence'].cpu(), info1['log_evidence'].cpu()
    assert torch.equal(ev0.view(torch.int32), ev1.view(torch.int32))              # pending added on the host or by the launch


# ---- 3. chunks, the other entry points, refusals, the default path ----------------------------------------------------------
def test_chunks_hold_whole_groups():
    """B * P = 72 > 64 rows with P = 24: chunks of 48 and 24 rows; equal to every group run alone with its own seeds."""
    dec = _decoder(NAMES[0])
    B, P = 3, 24
    codes, given = _random_inputs(dec, B, seed=315)
    cons = _voice0(given)
    seeds = torch.from_numpy(_seeds(31, B * P))
    kw = dict(temperature=1.0, particles=P, resample_threshold=1.0, return_particles=True, return_logp=True)
    tok, lp, info = dec.generate_from_codes(codes, constraint=cons, seed=seeds, **kw)
    assert tok.shape[0] == B * P and info['ancestors'].shape[1] == B * P and info['weights'].shape == (B, P)
    for g in range(B):
        sl = slice(g * P, (g + 1) * P)
        t1, l1, i1 = dec.generate_from_codes(codes[g:g + 1], constraint=cons[g:g + 1], seed=seeds[sl], **kw)
        assert torch.equal(tok[sl], t1) and torch.equal(lp[sl].view(torch.int32), l1.view(torch.int32)), g
        assert torch.equal(info['ancestors'][:, sl], i1['ancestors'] + g * P), g
        assert torch.equal(info['weights'][g].view(torch.int32), i1['weights'][0].view(torch.int32))
        assert torch.equal(info['log_evidence'][g:g + 1].view(torch.int32), i1['log_evidence'].view(torch.int32))
    first = dec.generate_from_codes(codes, constraint=cons, seed=seeds, temperature=1.0, particles=P, resample_threshold=1.0)
    assert first.shape[0] == B and torch.equal(first[:, :, 0], given[:, :, 0])


def test_reharmonise_tokens_with_particles_keeps_the_given_voice():
    dec, cfg, _ = _golden_decoder(NAMES[0])
    dec.eval()
    vocab, E = cfg['vocab'], cfg['events']
    dec.dataloader_generator = _meta_dataset(vocab)
    events = E + E // 2 - 1
    x = _random_tokens(dec, 1, events, seed=316, reserve=3).cpu()
    out = dec.reharmonise_tokens(x, num_reharmonisations=2, temperature=1.0, seed=5, keep_voices=(0,), particles=4)
    assert out.shape[0] == 2 and out.shape[1] >= events
    assert torch.equal(out[:, :events, 0].cpu(), x[:, :, 0].expand(2, -1))
    (tok, lp, info), c0, c1, n = dec.reharmonise_tokens(x, 2, 1.0, seed=5, keep_voices=(0,), particles=4, return_logp=True,
                                                        return_particles=True, return_bounds=True)
    assert tok.shape[0] == 8 and lp.shape == tok.shape and info['weights'].shape == (2, 4)
    assert info['ancestors'].shape == (n, 8) and bool(torch.isfinite(info['log_evidence']).all())
    assert bool((info['ancestors'][c0:c1] >= 0).all()) and bool((info['ancestors'][:c0] == -1).all())


def test_refusals():
    dec = _decoder(NAMES[0])
    pad, start = _meta_ids(dec)
    codes, given = _random_inputs(dec, 2, seed=317)
    long_codes = _random_codes(dec, 2, NB, seed=318)
    calls = (lambda **k: dec.generate_from_codes(codes, seed=1, **k),
             lambda **k: dec.generate_from_code_long(long_codes, temperature=1.0, seed=1, pad=pad, start=start, **k))
    for fn in calls:
        for P in (1, 65, 0, -2, 2.5, True):
            with pytest.raises(ValueError, match='particles'):
                fn(particles=P)
        for thr in (-0.1, 1.5, float('nan')):
            with pytest.raises(ValueError, match='resample_threshold'):
                fn(particles=2, resample_threshold=thr)
        with pytest.raises(ValueError, match='return_attentions'):
            fn(particles=2, return_attentions=True)
        with pytest.raises(ValueError, match='return_particles'):
            fn(return_particles=True)
        assert fn(particles=2).shape[0] == 2                                   # neither constraint nor sets: accepted


@pytest.mark.parametrize('name', NAMES)
def test_the_default_path_launches_nothing_new_and_the_step_launches_stay(monkeypatch, name):
    from vqcpc_bach_amd import hip
    dec = _decoder(name)
    codes, given = _random_inputs(dec, 2, seed=319)
    pad, start = _meta_ids(dec)
    long_codes = _random_codes(dec, 2, NB, seed=320)
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
        return list(names)
    cons = _voice0(given)
    long_kw = dict(temperature=1.0, seed=1, pad=pad, start=start)
    for use_graph in (True, False):
        for plain, filtered in ((lambda **k: dec.generate_from_codes(codes, seed=1, use_graph=use_graph, **k),
                                 dict(constraint=cons)),
                                (lambda **k: dec.generate_from_code_long(long_codes, use_graph=use_graph, **long_kw, **k), {})):
            default = launches(plain)
            assert not [n for n in default if n.startswith('vqcpc_particle')]
            assert {n for n in default if n.startswith('vqcpc_decode_sample')} == {'vqcpc_decode_sample'}
            # with particles: the same launches as the plain call over the same rows, plus the particle kernels
            same_rows = launches(lambda: plain(num_decodings=3, **filtered))
            with_p = launches(lambda: plain(particles=3, **filtered))
            assert [n for n in with_p if not n.startswith('vqcpc_particle')] == same_rows
            assert 'vqcpc_particle_resample' in with_p
    import inspect
    for fn in (dec.generate_from_codes, dec.generate_from_code_long):
        sig = inspect.signature(fn).parameters
        assert sig['particles'].default is None and sig['resample_threshold'].default == 0.5
        assert sig['return_particles'].default is False and sig['num_decodings'].default == 1
