"""The numpy statement of the voice-leading rules (tests/rules_reference.py) on hand-worked cases, every relaxation level
reached by construction, `templates.VoiceLeadingRules`'s checks, and the coverage of the case tables the GPU tests import
(tests/rules_cases.py).  No GPU."""
import numpy as np
import pytest
import torch

import rules_cases as C
import rules_reference as R

NC, V = 4, 60
HOLD_T, REST_T, META_T = 0, 1, 2
KINDS = np.array([[R.HOLD, R.REST, R.META] + list(range(40, 97))] * NC, dtype=np.int32)          # token p - 37 is pitch p
VOCAB = [V] * NC
NO_LEAP = [-1] * NC


def P(p):
    return p - 37


def piece(*ticks):
    """ticks: tuples of NC tokens -> one row, position-major."""
    return np.array([t for tick in ticks for t in tick], dtype=np.int64)


def viol(row, col, ck_token, constraint=None, max_leap=NO_LEAP):
    prev, now = R.voices_now(row, constraint, KINDS, VOCAB, NC, col)
    return R.violations(R.kind(KINDS, VOCAB, col % NC, ck_token), col % NC, prev, now, max_leap)


def test_crossing_against_an_emitted_upper_voice():
    row = piece((P(72), P(65), P(60), P(50)), (P(70), 0, 0, 0))
    col = 1 * NC + 1                                                    # the alto of tick 1: the soprano has drawn 70
    assert viol(row, col, P(72)) & R.CROSSING
    assert not viol(row, col, P(70)) & R.CROSSING                      # a unison is no crossing
    assert not viol(row, col, P(65)) & R.CROSSING
    assert not viol(row, col, REST_T) and not viol(row, col, META_T)
    # holding the alto's 65 under a soprano that fell to 64 crosses: the candidate's pitch is the held one
    row2 = piece((P(72), P(65), P(60), P(50)), (P(64), 0, 0, 0))
    assert viol(row2, col, HOLD_T) & R.CROSSING


def test_crossing_against_a_forced_lower_voice():
    row = piece((P(72), P(65), P(60), P(50)), (P(70), 0, 0, 0))
    cons = np.full(2 * NC, -1, dtype=np.int64)
    cons[1 * NC + 3] = P(60)                                            # the bass of tick 1 is given, not yet emitted
    col = 1 * NC + 1
    assert viol(row, col, P(58), cons) & R.CROSSING
    assert not viol(row, col, P(60), cons) & R.CROSSING
    assert not viol(row, col, P(58)) & R.CROSSING                      # without the constraint the bass is unknown
    cons[1 * NC + 2] = P(59)                                            # a voice BETWEEN: 58 is below the tenor too
    assert viol(row, col, P(59), cons) & R.CROSSING                    # 59 < the bass's 60
    # a free tenor says nothing, whatever lies in the row at its column
    cons[1 * NC + 2] = -1
    row[1 * NC + 2] = P(90)
    assert not viol(row, col, P(62), cons) & R.CROSSING


def test_a_forced_hold_is_resolved_through_its_chain():
    row = piece((P(72), P(65), P(60), P(62)), (P(72), P(65), P(60), HOLD_T), (P(72), P(65), P(60), HOLD_T), (P(70), 0, 0, 0))
    cons = np.full(4 * NC, -1, dtype=np.int64)
    cons[3 * NC + 3] = HOLD_T                                           # the bass holds the 62 of tick 0
    col = 3 * NC + 1
    prev, now = R.voices_now(row, cons, KINDS, VOCAB, NC, col)
    assert prev == [72, 65, 60, 62] and now == [70, R.NONE, R.NONE, 62]
    assert viol(row, col, P(61), cons) & R.CROSSING and not viol(row, col, P(62), cons) & R.CROSSING
    # a chain that runs into column 0, and one that ends on a rest, give no pitch
    row0 = piece((0, 0, 0, HOLD_T), (0, 0, 0, HOLD_T), (P(70), 0, 0, 0))
    assert R.pitch_at(row0, KINDS, VOCAB, NC, 3, 1) is R.NONE and R.pitch_at(row0, KINDS, VOCAB, NC, 3, -1) is R.NONE
    row1 = piece((0, 0, 0, REST_T), (0, 0, 0, HOLD_T), (P(70), 0, 0, 0))
    assert R.pitch_at(row1, KINDS, VOCAB, NC, 3, 1) is R.NONE


def test_leap_is_measured_from_the_sounding_pitch_and_a_rest_forgets_it():
    leaps = [5, 5, 5, 5]
    row = piece((P(72), P(60), 0, 0), (P(72), HOLD_T, 0, 0), (P(72), HOLD_T, 0, 0), (P(72), 0, 0, 0))
    col = 3 * NC + 1
    assert viol(row, col, P(66), max_leap=leaps) & R.LEAP and viol(row, col, P(54), max_leap=leaps) & R.LEAP
    assert not viol(row, col, P(65), max_leap=leaps) & R.LEAP and not viol(row, col, P(55), max_leap=leaps) & R.LEAP
    assert not viol(row, col, HOLD_T, max_leap=leaps) and not viol(row, col, REST_T, max_leap=leaps)
    assert not viol(row, col, P(66), max_leap=[5, -1, 5, 5]) & R.LEAP                  # off for this voice
    assert viol(row, col, P(61), max_leap=[0] * NC) & R.LEAP and not viol(row, col, P(60), max_leap=[0] * NC) & R.LEAP
    rest = piece((P(72), P(60), 0, 0), (P(72), REST_T, 0, 0), (P(72), 0, 0, 0))
    assert not viol(rest, 2 * NC + 1, P(90), max_leap=leaps) & R.LEAP                  # after a rest: unrestricted
    first = piece((P(72), 0, 0, 0))
    assert not viol(first, 1, P(40), max_leap=leaps) & R.LEAP                          # the first tick


def test_parallel_fifths_octaves_and_unison_to_octave():
    col = 1 * NC + 1
    fifth = piece((P(72), P(65), 0, 0), (P(74), 0, 0, 0))
    assert viol(fifth, col, P(67)) == R.PARALLEL
    assert not viol(fifth, col, P(66)) and not viol(fifth, col, P(65)) and not viol(fifth, col, HOLD_T)
    octave = piece((P(72), P(60), 0, 0), (P(74), 0, 0, 0))
    assert viol(octave, col, P(62)) == R.PARALLEL
    twelfth = piece((P(84), P(65), 0, 0), (P(86), 0, 0, 0))               # a compound fifth is a fifth
    assert viol(twelfth, col, P(67)) == R.PARALLEL
    unison = piece((P(60), P(60), 0, 0), (P(74), 0, 0, 0))
    assert viol(unison, col, P(62)) == R.PARALLEL                        # unison -> octave, both upwards
    # against a forced lower voice, through its held pitch of the previous tick
    cons = np.full(3 * NC, -1, dtype=np.int64)
    low = piece((0, P(72), 0, P(65)), (0, P(72), 0, HOLD_T), (0, 0, 0, 0))
    cons[2 * NC + 3] = P(63)
    assert viol(low, 2 * NC + 1, P(70), cons) == R.PARALLEL
    # a voice that stays, or an upper voice that stays, moves in no direction
    stay = piece((P(72), P(65), 0, 0), (P(72), 0, 0, 0))
    assert not viol(stay, col, P(60))
    # no previous pitch on either side: nothing to be parallel to
    assert not viol(piece((P(72), REST_T, 0, 0), (P(74), 0, 0, 0)), col, P(67))
    assert not viol(piece((REST_T, P(65), 0, 0), (P(74), 0, 0, 0)), col, P(67))


def test_contrary_motion_to_a_fifth_and_parallel_fourths_are_allowed():
    col = 1 * NC + 1
    contrary = piece((P(72), P(65), 0, 0), (P(79), 0, 0, 0))               # fifth -> twelfth, the voices part
    assert not viol(contrary, col, P(60))
    assert viol(contrary, col, P(72)) == R.PARALLEL                      # the same fifth reached in similar motion
    fourths = piece((P(72), P(67), 0, 0), (P(74), 0, 0, 0))
    assert not viol(fourths, col, P(69))
    into = piece((P(72), P(66), 0, 0), (P(74), 0, 0, 0))                   # a tritone that becomes a fifth in similar motion:
    assert not viol(into, col, P(67))                                    # a direct fifth, not a parallel one


def _set(*tokens):
    s = np.zeros(256, dtype=bool)
    s[list(tokens)] = True
    return s


def test_every_relaxation_level_by_construction():
    row = piece((P(72), P(65), 0, 0), (P(74), 0, 0, 0))
    col, leaps = 1 * NC + 1, [4] * NC
    pos = lambda static, exclude=None, enabled=7: R.position(row, col, NC, KINDS, VOCAB, leaps, enabled, None, static, exclude)
    # level 0: a clean token in the set; the set loses the offenders and everything past the vocabulary
    static = _set(P(66), P(67), P(80), P(50), 200)
    s, r = pos(static)
    assert r == 0 and np.array_equal(np.nonzero(s)[0], [P(66)])
    # no static set: the whole vocabulary minus the offenders
    s, r = pos(None)
    want = [k for k in range(V) if KINDS[1][k] < 0 or (KINDS[1][k] <= 74 and abs(KINDS[1][k] - 65) <= 4 and KINDS[1][k] != 67)]
    assert r == 0 and np.array_equal(np.nonzero(s)[0], want)
    # level 1: only the parallel fifth is in reach -> PARALLEL gives way, LEAP and CROSSING still hold
    s, r = pos(_set(P(67), P(80), P(50)))
    assert r == R.PARALLEL and np.array_equal(np.nonzero(s)[0], [P(67)])
    # level 2: every token leaps (one also crosses) -> LEAP gives way too, CROSSING holds
    s, r = pos(_set(P(80), P(50)))
    assert r == (R.PARALLEL | R.LEAP) and np.array_equal(np.nonzero(s)[0], [P(50)])
    # level 3: the only token crosses
    s, r = pos(_set(P(80)))
    assert r == 7 and np.array_equal(np.nonzero(s)[0], [P(80)])
    # exclude drains E & D: the clean token is excluded, so the rules give way -- but the written set is static & D_final,
    # the excluded token included (the sampler applies exclude)
    excl = _set(P(66))
    s, r = pos(static, excl)
    assert r == R.PARALLEL and np.array_equal(np.nonzero(s)[0], [P(66), P(67)])
    # a disabled rule neither restricts nor is reported
    s, r = pos(_set(P(67), P(80)), enabled=R.CROSSING | R.LEAP)
    assert r == 0 and np.array_equal(np.nonzero(s)[0], [P(67)])
    s, r = pos(_set(P(80)), enabled=R.CROSSING | R.PARALLEL)
    assert r == (R.CROSSING | R.PARALLEL)
    # a static set without a token of the vocabulary restricts nothing in the sampler: the whole vocabulary is written
    s, r = pos(_set(100, 255))
    assert r == 7 and np.array_equal(np.nonzero(s)[0], np.arange(V))
    # a forced position: the static set unchanged, the broken rules in the upper half
    cons = np.full(2 * NC, -1, dtype=np.int64)
    cons[col] = P(80)
    s, r = R.position(row, col, NC, KINDS, VOCAB, leaps, 7, cons, static, None)
    assert np.array_equal(s, static) and r == (R.CROSSING | R.LEAP) << 4
    cons[col] = P(67)
    s, r = R.position(row, col, NC, KINDS, VOCAB, leaps, 7, cons, None, None)
    assert np.array_equal(np.nonzero(s)[0], np.arange(V)) and r == R.PARALLEL << 4


def test_what_lies_at_and_past_the_column_cannot_matter():
    rng = np.random.default_rng(5)
    for c in C.CASES[:40:3]:
        for b in range(min(c['M'], 2)):
            row = c['rows'][b].copy()
            stat = None if c['static'] is None else R.unpack(c['static'][b, c['col']])
            excl = None if c['exclude'] is None else c['exclude'][c['v']]
            a = R.position(row, c['col'], c['nc'], c['kinds'], c['vocab'], c['max_leap'], c['enabled'], c['constraint'][b], stat, excl)
            row[c['col']:] = rng.integers(0, 256, size=len(row) - c['col'])
            z = R.position(row, c['col'], c['nc'], c['kinds'], c['vocab'], c['max_leap'], c['enabled'], c['constraint'][b], stat, excl)
            assert np.array_equal(a[0], z[0]) and a[1] == z[1]


def test_row_report_and_audit_agree_with_position():
    x, kinds, vocab, leaps = C.audit_piece(3, 2, 17)
    for b in range(2):
        aud = R.audit(x[b], 4, kinds, vocab, leaps, 7)
        sets, rep = R.row_report(x[b], 4, kinds, vocab, leaps, 7, constraint=x[b])
        assert np.array_equal(aud, rep) and bool(((aud & 15) == 0).all())
    words = R.pack(np.random.default_rng(0).random((3, 5, 256)) < 0.5)
    assert words.shape == (3, 5, 8) and words.dtype == np.int32 and np.array_equal(R.pack(R.unpack(words)), words)


def test_the_case_tables_cover_what_the_gpu_tests_claim():
    levels = {0: 0, R.PARALLEL: 0, R.PARALLEL | R.LEAP: 0, 7: 0}
    restricts, broken = {R.CROSSING: 0, R.LEAP: 0, R.PARALLEL: 0}, {R.CROSSING: 0, R.LEAP: 0, R.PARALLEL: 0}
    free_half = forced_half = 0
    seen = dict(M=set(), nc=set(), V=set(), chain=set(), static=set(), win=set())
    for c in C.CASES:
        M, nc, vocab, col, v = c['M'], c['nc'], c['vocab'], c['col'], c['v']
        # every id is in range
        assert len(vocab) == nc and all(1 <= n <= 256 for n in vocab) and c['kinds'].shape == (nc, max(vocab))
        assert 0 <= c['pos'] < c['T'] and col == c['w0'] * c['U'] + c['pos'] and col % nc == v and col < c['width']
        for u in range(nc):
            assert c['rows'][:, u::nc].min() >= 0 and c['rows'][:, u::nc].max() < vocab[u]
            assert c['constraint'][:, u::nc].min() >= -1 and c['constraint'][:, u::nc].max() < vocab[u]
        assert c['kinds'].min() >= R.META and c['kinds'].max() <= 127
        sets, report = C.expected(c['id'])
        hit_levels, hit_restricts, hit_broken = set(), set(), set()
        for b in range(M):
            assert sets[b, :vocab[v]].any() or c['constraint'][b, col] >= 0        # never an empty set inside the vocabulary
            if c['constraint'][b, col] >= 0:
                hit_broken |= {rule for rule in broken if (int(report[b]) >> 4) & rule}
                assert int(report[b]) & 15 == 0
                continue
            assert 0 <= int(report[b]) <= 7 and not sets[b, vocab[v]:].any()
            if c['enabled'] == 7:
                hit_levels.add(int(report[b]))
            # which rules restrict here: candidates of E that a rule alone removes
            prev, now = R.voices_now(c['rows'][b], c['constraint'][b], c['kinds'], vocab, nc, col)
            for k in range(vocab[v]):
                bits = R.violations(int(c['kinds'][v][k]), v, prev, now, c['max_leap']) & c['enabled'] & ~int(report[b])
                hit_restricts |= {rule for rule in restricts if bits & rule}
        for lv in hit_levels:
            levels[lv] += 1
        for rule in hit_restricts:
            restricts[rule] += 1
        for rule in hit_broken:
            broken[rule] += 1
        free_half += any(c['constraint'][b, col] < 0 and report[b] > 0 for b in range(M))
        forced_half += any(c['constraint'][b, col] >= 0 and report[b] > 0 for b in range(M))
        seen['M'].add(M), seen['nc'].add(nc), seen['V'].add(vocab[v]), seen['static'].add(c['static'] is None)
        seen['chain'].add(c['chain']), seen['win'].add(c['mode'])
    print('relaxation levels', levels, 'restricting', restricts, 'broken by a forced token', broken, 'report halves', free_half,
          forced_half)
    assert all(n >= 5 for n in levels.values()), levels
    assert all(n >= 5 for n in restricts.values()) and all(n >= 5 for n in broken.values()), (restricts, broken)
    assert free_half >= 5 and forced_half >= 5
    assert seen['M'] == set(C.SHAPES_M) and seen['nc'] == set(C.SHAPES_NC) and seen['V'] >= set(C.SHAPES_V)
    assert seen['chain'] >= set(C.CHAINS) and seen['static'] == {True, False} and seen['win'] == {'fixed', 'long'}
    assert sum(c['to_zero'] for c in C.CASES) >= 5 and sum(c['exclude'] is not None for c in C.CASES) >= 5
    # chains that cross from the live window into the chorale
    assert sum(c['mode'] == 'long' and c['chain'] * c['nc'] > c['pos'] for c in C.CASES) >= 5


def test_voice_leading_rules_checks_its_arguments():
    from vqcpc_bach_amd.templates import HOLD, META, REST, VoiceLeadingRules
    assert (HOLD, REST, META) == (R.HOLD, R.REST, R.META)
    kinds = torch.tensor(KINDS, dtype=torch.int16)
    r = VoiceLeadingRules(kinds)
    assert r.mask == 1 and r.kinds.dtype == torch.int32 and r.max_leap.tolist() == [-1] * NC
    assert VoiceLeadingRules(kinds, max_leap=12, no_parallels=True).mask == 7
    assert VoiceLeadingRules(kinds, no_crossing=False, max_leap=[None, 7, -1, 0]).max_leap.tolist() == [-1, 7, -1, 0]
    assert VoiceLeadingRules(kinds, no_crossing=False, max_leap=[None, 7, -1, 0]).mask == 2
    assert (VoiceLeadingRules.CROSSING, VoiceLeadingRules.LEAP, VoiceLeadingRules.PARALLEL) == (R.CROSSING, R.LEAP, R.PARALLEL)
    for bad in (kinds.float(), kinds[0], kinds.unsqueeze(0), kinds > 0, torch.zeros(17, 8, dtype=torch.int16),
                torch.zeros(4, 257, dtype=torch.int16), torch.full((4, 8), 128), torch.full((4, 8), -4)):
        with pytest.raises(ValueError):
            VoiceLeadingRules(bad)
    with pytest.raises(ValueError, match='no rule'):
        VoiceLeadingRules(kinds, no_crossing=False)
    with pytest.raises(ValueError, match='no rule'):
        VoiceLeadingRules(kinds, no_crossing=False, max_leap=[None, -1, None, None])
    with pytest.raises(ValueError):
        VoiceLeadingRules(kinds, max_leap=-1)
    with pytest.raises(ValueError):
        VoiceLeadingRules(kinds, max_leap=[1, 2, 3])
    with pytest.raises(ValueError):
        VoiceLeadingRules(kinds, max_leap=1.5)
