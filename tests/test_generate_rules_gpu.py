"""Voice-leading rules in generation (`rules=`, `return_rule_report=` of Decoder.generate_from_codes / generate_from_code_long /
reharmonise_tokens, `Decoder.audit_voice_leading`; decoders/generation.py `_rule_sets`; csrc/rules.hip) on the tiny decoders of the
generation tests (vocabularies 11..14, S = 3, U = 16, T = 48; long form nb = 5) with a synthetic table of token names:
  (1) the returned rule_report is the reference's (tests/rules_reference.py), recomputed from the returned tokens, the
      constraint, the static sets and the exclusion, and every drawn token lies in the reference's final set -- on a case where
      the rules bite: a quarter of the free positions lose tokens and the same seed without rules breaks them;
      and on sets so tight that the rules give way inside the generation (the lower half of the report);
  (2) per tick, what the audit finds is a subset of what the report says was dropped or broken there;
  (3) an all-META table restricts nothing: tokens, logp and allowed_mass are the masked path's bits, the report is 0;
  (4) captured == eager, chunks == whole, a row == the row alone;
  (5) the long form through head, middle slides and tail, with a held soprano note that outlives its window;
  (6) particles: threshold 0 is the plain run, at threshold 1 the report moves with its row;
  (7) the refusals."""
import numpy as np
import pytest
import torch

import rules_reference as R
from test_generate_gpu import _golden_decoder, _random_inputs
from test_generate_long_gpu import _meta_dataset, _meta_ids, _random_codes
from test_generate_masked_gpu import _random_mask, _random_tokens

pytestmark = pytest.mark.gpu

NAMES = ['decoder_tiny', 'decoder_tiny_diagonal']
NB = 5
STEPS = ['C', 'C#', 'D', 'E-', 'E', 'F', 'F#', 'G', 'A-', 'A', 'B-', 'B']
CENTRES = (72, 67, 62, 57)


def _decoder(name):
    dec = _golden_decoder(name)[0]
    dec.eval()
    return dec


def _vocab(dec):
    return [int(v) for v in dec.num_tokens_per_channel]


def _names(dec):
    """Per voice: 0 '__', 1 'rest', then consecutive semitones around the voice's centre, and START / END / XX as the last three
    ids (the stub dataset of the long-form tests)."""
    vocab = _vocab(dec)
    names = np.full((len(vocab), max(vocab)), '', dtype=object)
    for c, V in enumerate(vocab):
        names[c, 0], names[c, 1] = '__', 'rest'
        n = V - 5
        for i in range(n):
            midi = CENTRES[c] - n // 2 + i
            names[c, 2 + i] = f'{STEPS[midi % 12]}{midi // 12 - 1}'
        names[c, V - 3:V] = ['START', 'END', 'XX']
    return names


def _rules(dec, **kw):
    from vqcpc_bach_amd import templates
    kinds = templates.token_kinds(_names(dec), _vocab(dec))
    kw = dict(dict(no_crossing=True, max_leap=4, no_parallels=True), **kw)
    return templates.VoiceLeadingRules(kinds, **kw), kinds.numpy().astype(np.int32)


def _exclude(dec):
    return [[v - 3, v - 2, v - 1] for v in _vocab(dec)]                 # the meta symbols are never drawn


def _exclude_bits(dec):
    bits = np.zeros((dec.num_channels, 256), dtype=bool)
    for c, toks in enumerate(_exclude(dec)):
        bits[c, toks] = True
    return bits


def _bass_constraint(dec, B, E, seed, share=0.5):
    """The bass forced on `share` of the events: pitches, and holds of them."""
    g = torch.Generator().manual_seed(seed)
    nc, V = dec.num_channels, _vocab(dec)[-1]
    cons = torch.full((B, E, nc), -1, dtype=torch.int64)
    forced = torch.rand(B, E, generator=g) < share
    tok = torch.randint(0, V - 3, (B, E), generator=g)                  # HOLD, REST or a pitch
    cons[:, :, nc - 1] = torch.where(forced, tok, torch.full_like(tok, -1))
    return cons.cuda()


def _static(allowed, rows, width):
    """The public mask (rows, events, channels, vmax) -> bool (rows, width, 256)."""
    out = np.zeros((rows, width, 256), dtype=bool)
    a = allowed.cpu().numpy().reshape(rows, width, -1)
    out[:, :, :a.shape[2]] = a
    return out


def _recompute(dec, kinds, rules, tokens, cons, static, exclude, first=0):
    """The reference over every row -> (sets (rows, width, 256), report (rows, width), -1 before column `first`)."""
    rows, nc, vocab = tokens.shape[0], dec.num_channels, _vocab(dec)
    tok = tokens.reshape(rows, -1).cpu().numpy()
    con = None if cons is None else cons.reshape(rows, -1).cpu().numpy()
    sets, report = [], []
    for b in range(rows):
        s, r = R.row_report(tok[b], nc, kinds, vocab, rules.max_leap.tolist(), rules.mask, None if con is None else con[b],
                            None if static is None else static[b], exclude, first=first)
        sets.append(s), report.append(r)
    return np.stack(sets), np.stack(report)


def _assert_case_one(dec, kinds, rules, tokens, report, cons, static, exclude, first=0):
    """Case (1): the report is the reference's and every free token lies in the final set.  -> (sets, the share of the free
    positions whose final set is strictly smaller than the static one)."""
    rows, vocab, nc = tokens.shape[0], _vocab(dec), dec.num_channels
    sets, want = _recompute(dec, kinds, rules, tokens, cons, static, exclude, first)
    got = report.reshape(rows, -1).cpu().numpy()
    assert got.dtype == np.int32 and np.array_equal(got[:, first:], want[:, first:]), np.argwhere(got != want)[:5]
    tok = tokens.reshape(rows, -1).cpu().numpy()
    free = np.ones_like(tok, dtype=bool) if cons is None else cons.reshape(rows, -1).cpu().numpy() < 0
    free[:, :first] = False
    smaller = total = 0
    for b, col in np.argwhere(free):
        V = vocab[col % nc]
        assert sets[b, col, tok[b, col]], (b, col)
        assert exclude is None or not exclude[col % nc, tok[b, col]]
        before = np.ones(V, dtype=bool) if static is None else static[b, col, :V]
        smaller += int(sets[b, col, :V].sum() < before.sum())
        total += 1
    return sets, smaller / max(total, 1)


def _broken(dec, kinds, rules, tokens):
    """The reference's audit of every row, >> 4."""
    tok = tokens.reshape(tokens.shape[0], -1).cpu().numpy()
    return np.stack([R.audit(t, dec.num_channels, kinds, _vocab(dec), rules.max_leap.tolist(), rules.mask) for t in tok]) >> 4


# ---- 1, 2. the report is the reference's; the audit ------------------------------------------------------------------------
@pytest.mark.parametrize('name', NAMES)
def test_report_and_tokens_follow_the_reference_where_the_rules_bite(name):
    dec = _decoder(name)
    rules, kinds = _rules(dec)
    B, nc = 3, dec.num_channels
    E = dec.num_tokens_target // nc
    codes, _ = _random_inputs(dec, B, seed=411)
    cons = _bass_constraint(dec, B, E, seed=412)
    allowed = _random_mask(dec, B, E, seed=413, density=0.7, reserve=3)
    allowed.scatter_(3, cons.clamp(min=0).cpu().unsqueeze(3), True)     # a forced token lies in its set (token 0 elsewhere)
    kw = dict(temperature=1.0, seed=21, constraint=cons, allowed=allowed, exclude_tokens=_exclude(dec))
    tokens, mass, report = dec.generate_from_codes(codes, rules=rules, return_allowed_mass=True, return_rule_report=True, **kw)
    assert report.shape == tokens.shape and report.dtype == torch.int32 and mass.shape == tokens.shape
    assert torch.equal(tokens[cons >= 0], cons[cons >= 0])
    static = _static(allowed, B, E * nc)
    sets, share = _assert_case_one(dec, kinds, rules, tokens, report, cons, static, _exclude_bits(dec))
    plain = dec.generate_from_codes(codes, **kw)
    broken = _broken(dec, kinds, rules, plain)
    print(f'{name}: {share:.2f} of the free positions lost tokens to the rules; without rules the same seed breaks '
          f'{int((broken != 0).sum())} places; dropped at {int(((report.cpu().numpy() & 7) != 0).sum())}')
    assert share >= 0.25 and bool((broken != 0).any())
    assert bool((mass <= 0).all()) and bool(torch.isfinite(mass).all())
    # (2) per tick, the audit's bits are among the tick's dropped and forced-broken bits
    audit = dec.audit_voice_leading(tokens, rules)
    assert audit.shape == tokens.shape and audit.dtype == torch.int32
    assert np.array_equal(audit.reshape(B, -1).cpu().numpy() >> 4, _broken(dec, kinds, rules, tokens))
    rep = report.cpu().numpy()
    said = np.bitwise_or.reduce((rep & 7) | (rep >> 4), axis=2)          # (B, E)
    found = np.bitwise_or.reduce(audit.cpu().numpy() >> 4, axis=2)
    assert bool(((found & ~said) == 0).all()), np.argwhere(found & ~said)[:5]
    # where nothing was dropped and nothing forced is broken, the piece keeps the rules
    assert bool((found[said == 0] == 0).all())


def test_tight_sets_make_the_rules_give_way_and_the_report_says_where():
    """Sets of two or three tokens: often none of them is clean, so the rules are relaxed inside a generation -- the lower
    half of the report -- and the sampler still never meets an empty set."""
    dec = _decoder(NAMES[0])
    rules, kinds = _rules(dec, max_leap=2)
    B, nc = 4, dec.num_channels
    E = dec.num_tokens_target // nc
    codes, _ = _random_inputs(dec, B, seed=415)
    allowed = _random_mask(dec, B, E, seed=416, density=0.2, reserve=3)
    kw = dict(temperature=1.0, seed=22, allowed=allowed, exclude_tokens=_exclude(dec), rules=rules, return_rule_report=True)
    tokens, report = dec.generate_from_codes(codes, **kw)
    _assert_case_one(dec, kinds, rules, tokens, report, None, _static(allowed, B, E * nc), _exclude_bits(dec))
    rep = report.cpu().numpy()
    print(f'reports seen: {sorted(int(r) for r in np.unique(rep))}, relaxed at {int((rep != 0).sum())} of {rep.size} positions')
    assert bool((rep >= 0).all()) and bool((rep <= 7).all()) and bool((rep != 0).any())      # the case reaches the relaxation
    found = np.bitwise_or.reduce(dec.audit_voice_leading(tokens, rules).cpu().numpy() >> 4, axis=2)
    assert bool(((found & ~np.bitwise_or.reduce(rep, axis=2)) == 0).all()) and bool((found != 0).any())
    eager = dec.generate_from_codes(codes, use_graph=False, **kw)
    assert torch.equal(eager[0], tokens) and torch.equal(eager[1], report)


# ---- 3. a table that names no pitch ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', NAMES)
def test_an_all_meta_table_is_the_masked_path(name):
    from vqcpc_bach_amd import templates
    dec = _decoder(name)
    B, nc = 2, dec.num_channels
    E = dec.num_tokens_target // nc
    rules = templates.VoiceLeadingRules(torch.full((nc, max(_vocab(dec))), templates.META, dtype=torch.int16), max_leap=3,
                                        no_parallels=True)
    codes, given = _random_inputs(dec, B, seed=421)
    cons = torch.full_like(given, -1)
    cons[:, ::3, 1] = given[:, ::3, 1]
    allowed = _random_mask(dec, B, E, seed=422, vmax=max(_vocab(dec)) + 2)
    allowed.scatter_(3, given.cpu().unsqueeze(3), True)
    for extra in (dict(allowed=allowed), dict()):
        kw = dict(temperature=0.9, top_p=0.95, seed=5, constraint=cons, return_logp=True, return_allowed_mass=True, **extra)
        tok, lp, mass = dec.generate_from_codes(codes, **kw)
        rtok, rlp, rmass, report = dec.generate_from_codes(codes, rules=rules, return_rule_report=True, **kw)
        assert torch.equal(rtok, tok) and torch.equal(rlp.view(torch.int32), lp.view(torch.int32))
        assert torch.equal(rmass.view(torch.int32), mass.view(torch.int32))
        assert bool((report == 0).all())
        if not extra:
            assert bool((mass == 0).all())


# ---- 4. captured, chunks, rows ------------------------------------------------------------------------------------------
def test_captured_equals_eager_chunks_equal_whole_and_a_row_equals_the_row_alone():
    from vqcpc_bach_amd.transformer.incremental import row_seeds
    dec = _decoder(NAMES[0])
    rules, kinds = _rules(dec)
    B, nc = 33, dec.num_channels
    E = dec.num_tokens_target // nc
    codes, _ = _random_inputs(dec, B, seed=431)
    cons = _bass_constraint(dec, B, E, seed=432, share=0.3)
    seeds = row_seeds(17, 2 * B)
    kw = dict(temperature=1.0, exclude_tokens=_exclude(dec), rules=rules, return_logp=True, return_allowed_mass=True,
              return_rule_report=True)
    whole = dec.generate_from_codes(codes, num_decodings=2, seed=seeds, constraint=cons, **kw)        # 66 rows: two chunks
    assert whole[0].shape == (2 * B, E, nc) and bool((whole[3] >= 0).all())
    same = lambda a, b: all(torch.equal(x.view(torch.int32) if x.is_floating_point() else x, y.view(torch.int32)
                                        if y.is_floating_point() else y) for x, y in zip(a, b))
    # the rows of the second chunk, and one row of the first, each in a call of their own
    tail = dec.generate_from_codes(codes[31:], num_decodings=2, seed=seeds[62:], constraint=cons[31:], **kw)
    assert same(tail, [w[62:] for w in whole])
    one = dec.generate_from_codes(codes[7:8], seed=seeds[15:16], constraint=cons[7:8], **kw)
    assert same(one, [w[15:16] for w in whole])
    eager = dec.generate_from_codes(codes[:4], num_decodings=2, seed=seeds[:8], constraint=cons[:4], use_graph=False, **kw)
    assert same(eager, [w[:8] for w in whole])
    _assert_case_one(dec, kinds, rules, whole[0][60:], whole[3][60:], cons.repeat_interleave(2, dim=0)[60:], None, _exclude_bits(dec))


# ---- 5. long form -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', NAMES)
def test_long_form_with_a_held_note_that_outlives_its_window(name):
    from vqcpc_bach_amd.decoders.decoder import Decoder
    dec = _decoder(name)
    dec.dataloader_generator = _meta_dataset(_vocab(dec))
    rules, kinds = _rules(dec, max_leap=5)
    pad, start = _meta_ids(dec)
    B, nc, S, U = 2, dec.num_channels, dec.num_tokens_source, dec.total_upscaling
    epc = U // nc
    E = NB * epc
    codes = _random_codes(dec, B, NB, seed=441)
    cs, ce = 1, NB
    # the soprano: one of its lowest pitches at the first generated event, then held to the end -- 15 ticks, the window has
    # 12 -- so the alto's upper tokens cross it for as long as the held pitch is found
    cons = torch.full((B, E, nc), -1, dtype=torch.int64)
    cons[:, cs * epc, 0] = torch.tensor([2, 3])
    cons[:, cs * epc + 1:, 0] = 0
    cons = cons.cuda()
    allowed = _random_mask(dec, B, E, seed=442, density=0.8, reserve=3)
    allowed.scatter_(3, cons.clamp(min=0).cpu().unsqueeze(3), True)
    kw = dict(temperature=1.0, seed=23, pad=pad, start=start, code_index_start=cs, code_index_end=ce, constraint=cons,
              allowed=allowed, exclude_meta_symbols=True, rules=rules, return_allowed_mass=True, return_rule_report=True)
    tokens, mass, report = dec.generate_from_code_long(codes, **kw)
    assert tokens.shape == (B, (ce - cs) * epc, nc) and report.shape == tokens.shape
    # the reference on the whole chorale: the frame before the first generated code is PAD / START, which have no pitch
    frame = torch.tensor(pad, dtype=torch.int64).view(1, 1, nc).expand(B, cs * epc, nc).cuda()
    full = torch.cat([frame, tokens], dim=1)
    full_report = torch.cat([torch.full_like(frame, -1, dtype=torch.int32), report], dim=1)
    static = _static(allowed, B, E * nc)
    excl = _exclude_bits(dec)
    sets, share = _assert_case_one(dec, kinds, rules, full, full_report, cons, static, excl, first=cs * U)
    assert share >= 0.25
    for graph in (dict(use_graph=False), dict(use_graph=True, graph_slides=False)):
        again = dec.generate_from_code_long(codes, **kw, **graph)
        assert torch.equal(again[0], tokens) and torch.equal(again[2], report)
        assert torch.equal(again[1].view(torch.int32), mass.view(torch.int32))
    # the held soprano is what the late positions were judged against: with a history cut at the window's start the reference
    # gives other sets somewhere in the windows that no longer hold the soprano's pitch
    starts = Decoder.attention_window_starts(NB, S, U, cs, ce).numpy()
    late = np.nonzero(starts * U > cs * U)[0]
    assert len(late) >= U
    tok = full.reshape(B, -1).cpu().numpy()
    con = cons.reshape(B, -1).cpu().numpy()
    differs = 0
    for b in range(B):
        for col in late:
            cut = tok[b].copy()
            for u in range(nc):
                cut[u:starts[col] * U:nc] = pad[u]                        # XX: no pitch
            s, _ = R.position(cut, int(col), nc, kinds, _vocab(dec), rules.max_leap.tolist(), rules.mask, con[b], static[b, col],
                              excl[col % nc])
            differs += int(not np.array_equal(s, sets[b, col]))
    print(f'{name}: {differs} of {B * len(late)} late positions depend on history before their window')
    assert differs >= 1


def test_reharmonise_tokens_takes_the_rules_and_reports_in_its_own_events():
    """A given soprano and bass, the inner voices written between them without crossing or leaping."""
    dec, cfg, _ = _golden_decoder(NAMES[0])
    dec.eval()
    dec.dataloader_generator = _meta_dataset(cfg['vocab'])
    rules, kinds = _rules(dec, no_parallels=False)
    events = cfg['events'] + cfg['events'] // 2 - 1
    x = _random_tokens(dec, 1, events, seed=471, reserve=3).cpu()
    out, report = dec.reharmonise_tokens(x, 2, temperature=1.0, seed=5, keep_voices=(0, 3), rules=rules, return_rule_report=True,
                                         exclude_meta_symbols=True)
    assert out.shape == report.shape and out.shape[0] == 2 and out.shape[1] >= events and report.dtype == torch.int32
    assert torch.equal(out[:, :events, 0].cpu(), x[:, :, 0].expand(2, -1)) and torch.equal(out[:, :events, 3].cpu(), x[:, :, 3].expand(2, -1))
    assert bool((report >= 0).all())
    audit = dec.audit_voice_leading(out, rules).cpu().numpy() >> 4
    rep = report.cpu().numpy()
    said = np.bitwise_or.reduce((rep & 7) | (rep >> 4), axis=2)
    assert bool(((np.bitwise_or.reduce(audit, axis=2) & ~said) == 0).all())
    # with particles the same call returns one survivor per reharmonisation, report included
    out4, report4 = dec.reharmonise_tokens(x, 2, temperature=1.0, seed=5, keep_voices=(0, 3), rules=rules, return_rule_report=True,
                                           exclude_meta_symbols=True, particles=4)
    assert out4.shape == out.shape and report4.shape == out.shape


def test_generate_takes_the_rules_and_returns_the_report(tmp_path):
    from test_generate_gpu import _api_decoder
    dec, cfg = _api_decoder(tmp_path)
    rules, kinds = _rules(dec)
    plain = dec.generate(temperature=1.0, batch_size=2, seed_set='val', seed=3, keep_voices=(0,))
    assert 'rule_report' not in plain
    out = dec.generate(temperature=1.0, batch_size=2, seed_set='val', seed=3, keep_voices=(0,), rules=rules, return_rule_report=True,
                       return_attentions=True)
    assert set(out) == set(plain) | {'rule_report', 'attentions'}
    tokens, report = out['generation'], out['rule_report']
    assert report.shape == tokens.shape and torch.equal(tokens[:, :, 0], out['original'][:, :, 0])
    cons = torch.full_like(tokens, -1)
    cons[:, :, 0] = tokens[:, :, 0]
    _assert_case_one(dec, kinds, rules, tokens, report, cons, None, None)
    quiet = dec.generate(temperature=1.0, batch_size=2, seed_set='val', seed=3, keep_voices=(0,), rules=rules)
    assert torch.equal(quiet['generation'], tokens) and 'rule_report' not in quiet


# ---- 6. particles ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', NAMES)
def test_particles_see_the_rules_and_the_report_moves_with_its_row(name):
    dec = _decoder(name)
    rules, kinds = _rules(dec)
    B, P, nc = 2, 4, dec.num_channels
    E = dec.num_tokens_target // nc
    codes, _ = _random_inputs(dec, B, seed=451)
    cons = _bass_constraint(dec, B, E, seed=452)
    kw = dict(temperature=1.0, seed=29, constraint=cons, exclude_tokens=_exclude(dec), rules=rules, return_logp=True,
              return_allowed_mass=True, return_rule_report=True)
    plain = dec.generate_from_codes(codes, num_decodings=P, **kw)
    still = dec.generate_from_codes(codes, particles=P, resample_threshold=0.0, return_particles=True, **kw)
    for a, b in zip(plain, still[:4]):
        assert torch.equal(a.view(torch.int32) if a.is_floating_point() else a, b.view(torch.int32) if b.is_floating_point() else b)
    assert bool((plain[2] < 0).any())                                   # the rules cost mass: the weights see them
    excl = _exclude_bits(dec)
    for use_graph in (True, False):
        tok, lp, mass, report, info = dec.generate_from_codes(codes, particles=P, resample_threshold=1.0, return_particles=True,
                                                              use_graph=use_graph, **kw)
        moved = int((info['ancestors'].cpu() != torch.arange(B * P, dtype=torch.int32)).sum())
        print(f'{name} (graph {use_graph}): {moved} row moves')
        assert moved > 0
        _assert_case_one(dec, kinds, rules, tok, report, cons.repeat_interleave(P, dim=0), None, excl)
    first = dec.generate_from_codes(codes, particles=P, resample_threshold=1.0, **kw)
    assert first[0].shape == (B, E, nc) and first[3].shape == (B, E, nc)
    _assert_case_one(dec, kinds, rules, first[0], first[3], cons, None, excl)
    # long form: the chorale rows and the report rows move together
    dec.dataloader_generator = _meta_dataset(_vocab(dec))
    pad, start = _meta_ids(dec)
    epc = dec.total_upscaling // nc
    long_codes = _random_codes(dec, 1, NB, seed=453)
    lcons = _bass_constraint(dec, 1, NB * epc, seed=454)
    tok, report, info = dec.generate_from_code_long(long_codes, temperature=1.0, seed=31, pad=pad, start=start, code_index_start=1,
                                                    constraint=lcons, exclude_meta_symbols=True, rules=rules, particles=P,
                                                    resample_threshold=1.0, return_particles=True, return_rule_report=True)
    frame = torch.tensor(pad, dtype=torch.int64).view(1, 1, nc).expand(P, epc, nc).cuda()
    _assert_case_one(dec, kinds, rules, torch.cat([frame, tok], dim=1),
                     torch.cat([torch.full_like(frame, -1, dtype=torch.int32), report], dim=1), lcons.repeat_interleave(P, dim=0),
                     None, excl, first=dec.total_upscaling)


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------
def test_the_refusals():
    from vqcpc_bach_amd import templates
    from vqcpc_bach_amd.decoders.generation import IncrementalDecoder
    dec = _decoder(NAMES[0])
    rules, _ = _rules(dec)
    codes, given = _random_inputs(dec, 2, seed=461)
    with pytest.raises(ValueError, match='return_rule_report'):
        dec.generate_from_codes(codes, return_rule_report=True)
    with pytest.raises(ValueError, match='rules'):
        dec.generate_from_codes(codes, rules='no crossing')
    with pytest.raises(ValueError, match='kinds'):
        dec.generate_from_codes(codes, rules=templates.VoiceLeadingRules(rules.kinds[:3]))
    with pytest.raises(ValueError, match='kinds'):
        dec.generate_from_codes(codes, rules=templates.VoiceLeadingRules(rules.kinds[:, :5]))
    with pytest.raises(ValueError, match='kinds'):
        dec.audit_voice_leading(given, templates.VoiceLeadingRules(rules.kinds[:3]))
    with pytest.raises(ValueError):
        dec.audit_voice_leading(given[0], rules)
    with pytest.raises(ValueError):
        dec.audit_voice_leading(given, None)
    with pytest.raises(ValueError, match='return_attentions'):
        dec.generate_from_codes(codes, rules=rules, particles=2, return_attentions=True)
    long_codes = _random_codes(dec, 1, NB, seed=462)
    with pytest.raises(ValueError, match='return_rule_report'):
        dec.generate_from_code_long(long_codes, temperature=1.0, pad=[0] * 4, start=[0] * 4, return_rule_report=True)
    inc = IncrementalDecoder(dec, 2)
    inc.prefill(codes)
    with pytest.raises(ValueError, match='teacher'):
        inc.start(seeds=1, teacher=given.reshape(2, -1), rules=rules)
    with pytest.raises(ValueError, match='teacher'):
        inc.start(seeds=1, teacher=given.reshape(2, -1), allowed=torch.zeros(2, dec.num_tokens_target, 8, dtype=torch.int32))
    # without the keywords the step's launches are what they were: no rule buffer, the plain sampler
    inc.start(seeds=1)
    assert inc.rules is None and inc.rule_report is None and inc.rule_static is None and not inc.masked
