"""The float64 reference of the masked sampler (tests/masked_reference.py) against plain definitions, the mask builders of
vqcpc_bach_amd/templates.py position by position on a synthetic names table, and the new entry point's host-side argument
checks (no GPU: the checks fail before any HIP call)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import constrained_reference as C
import masked_reference as MR

SETTINGS = [(1.0, 0, 1.0, ()), (0.7, 5, 1.0, (1,)), (1.5, 0, 0.9, ()), (0.7, 4, 0.8, (0, 2))]


def _rows(M, V, seed):
    return torch.randn(M, V, generator=torch.Generator().manual_seed(seed)) * 2.0


@pytest.mark.parametrize('V', [1, 2, 13, 256])
def test_all_allowed_is_the_constrained_reference(V):
    M = 5
    lg = _rows(M, V, 400 + V)
    seeds = torch.arange(M, dtype=torch.int64) * 1000003 + 17
    cons = torch.tensor([-1, 0, -1, V - 1, -1], dtype=torch.int64)
    high = torch.zeros(M, 256, dtype=torch.bool)
    high[:, V:] = True                                                           # bits at or past V only: no restriction
    for temperature, top_k, top_p, exclude in SETTINGS:
        exclude = tuple(t for t in exclude if t < V and V > 3)
        want = C.constrained_step_ref(lg, temperature, top_k, top_p, exclude, seeds, 3, cons)
        sets = [None, torch.ones(M, V, dtype=torch.bool), torch.ones(M, 256, dtype=torch.bool)] + ([high] if V < 256 else [])
        for allowed in sets:
            tok, pr, lp, lm = MR.masked_step_ref(lg, temperature, top_k, top_p, exclude, seeds, 3, cons, allowed)
            assert torch.equal(tok, want[0]) and torch.equal(pr, want[1]) and torch.equal(lp, want[2])
            assert lm.tolist() == [0.0] * M


@pytest.mark.parametrize('V', [2, 13, 256])
def test_a_one_hot_set_is_forcing(V):
    M = 6
    lg = _rows(M, V, 500 + V)
    seeds = torch.arange(M, dtype=torch.int64) + 3
    g = torch.Generator().manual_seed(V)
    pick = torch.randint(0, V, (M,), generator=g)
    one_hot = torch.zeros(M, V, dtype=torch.bool)
    one_hot[torch.arange(M), pick] = True
    for temperature, top_k, top_p, _ in SETTINGS:
        tok, pr, lp, lm = MR.masked_step_ref(lg, temperature, top_k, top_p, (), seeds, 5, None, one_hot)
        forced = C.constrained_step_ref(lg, temperature, top_k, top_p, (), seeds, 5, pick)
        assert torch.equal(tok, pick) and torch.equal(tok, forced[0]) and torch.equal(lp, forced[2])
        assert torch.equal(pr, one_hot.double())                                 # all of the filtered mass on the one token
        assert torch.allclose(lm, lp, rtol=0, atol=1e-12)                        # the set's mass is its token's probability
    # a forced token outside its set is still emitted
    other = (pick + 1) % V
    tok = MR.masked_step_ref(lg, 1.0, 0, 1.0, (), seeds, 5, other, one_hot)[0]
    assert torch.equal(tok, other)


def test_the_set_acts_before_the_filters_and_joins_the_exclusion():
    lg = torch.tensor([[5.0, 4.0, 3.0, 2.0, 1.0, 0.0]])
    allowed = torch.tensor([[False, True, False, True, True, True]])
    seeds = torch.tensor([11], dtype=torch.int64)
    _, pr, _, lm = MR.masked_step_ref(lg, 1.0, 2, 1.0, (3,), seeds, 0, None, allowed)
    want = torch.zeros(6, dtype=torch.float64)
    want[[1, 4]] = torch.softmax(torch.tensor([4.0, 1.0], dtype=torch.float64), dim=0)   # top-2 of the allowed, not excluded
    assert torch.allclose(pr[0], want, rtol=0, atol=1e-15)
    p = torch.softmax(lg[0].double(), dim=0)
    assert abs(float(lm[0]) - float(torch.log(p[[1, 3, 4, 5]].sum()))) < 1e-12          # the exclusion does not enter the mass


@pytest.mark.parametrize('V', [2, 13, 256])
def test_logmass_against_logsumexp(V):
    g = torch.Generator().manual_seed(600 + V)
    rows = [_rows(1, V, 601 + V)[0], torch.linspace(-80.0, 80.0, V)[torch.randperm(V, generator=g)], _rows(1, V, 602 + V)[0]]
    rows[2][::2] = -float('inf')
    for row in rows:
        for density in (0.1, 0.5, 0.9):
            a = torch.rand(V, generator=g) < density
            a[int(torch.randint(0, V, (1,), generator=g))] = True
            r = row.double()
            want = float(torch.logsumexp(r[a], dim=0) - torch.logsumexp(r, dim=0))
            got = MR.logmass_ref(row, a)
            if want == -float('inf'):
                assert got == want
            else:
                assert abs(got - want) < 1e-12 * max(1.0, abs(want)), (V, density, got, want)
                assert got <= 1e-15
    assert MR.logmass_ref(rows[0], torch.ones(V, dtype=torch.bool)) == 0.0
    assert MR.logmass_ref(rows[0], torch.zeros(V, dtype=torch.bool)) == 0.0      # an empty set restricts nothing
    inf_only = torch.zeros(V, dtype=torch.bool)
    inf_only[0] = True
    assert MR.logmass_ref(rows[2], inf_only) == -float('inf')


def test_logmass_bound_covers_plain_fp32():
    """The bound holds for the same chain in fp32 numpy on the CPU (sequential sums: checked against gamma_V as the logp bound's
    test does), is 0 where the kernel is exact and is not vacuous."""
    g = torch.Generator().manual_seed(19)
    for V, scale in ((13, 2.0), (256, 2.0), (256, 40.0)):
        row = (torch.randn(V, generator=g) * scale).float()
        a = torch.rand(V, generator=g) < 0.5
        a[0] = True
        r = row.numpy()

        def chain(x):
            m = x.max()
            s = np.float32(0)
            for v in np.exp((x - m).astype(np.float32)).astype(np.float32):
                s = np.float32(s + v)
            return m, np.log(s, dtype=np.float32)
        (m, L), (ma, La) = chain(r), chain(r[a.numpy()])
        got = float(np.float32(np.float32(np.float32(ma - m) + La) - L))
        b = MR.logmass_bound(row, a)
        assert 0 < b < 1e-4, b
        assert abs(got - MR.logmass_ref(row, a)) <= b + 2 * V * C.U_FP32, (V, scale)
        assert MR.logmass_bound(row, torch.ones(V, dtype=torch.bool)) == 0.0


# ---- templates.py ---------------------------------------------------------------------------------------------------------
NAMES = [['C4', 'C#4', 'D-4', 'B-3', 'B--3', '__', 'rest', 'START', 'END', 'XX', ''],
         ['F##2', 'G2', 'a3', '__', 'rest', 'H4', 'C', '4C', 'rest ', 'E-5', 'C4'],
         ['__', 'rest', 'C-1', 'G9', 'C10', 'E4', '', '', '', '', '']]
VOCAB = [10, 10, 6]                        # voice 0: '' past the vocabulary; voice 1: its last name is past the vocabulary too


def _kinds():
    from vqcpc_bach_amd import templates as T
    return T, T.token_kinds(np.array(NAMES), VOCAB)


def test_token_kinds_reads_music21_names():
    T, kinds = _kinds()
    H, R, X = T.HOLD, T.REST, T.META
    assert (H, R, X) == (-1, -2, -3)
    assert kinds.dtype == torch.int16 and kinds.shape == (3, 11)
    assert kinds[0].tolist() == [60, 61, 61, 58, 57, H, R, X, X, X, X]
    assert kinds[1].tolist() == [43, 43, 57, H, R, X, X, X, X, 75, X]           # 'C4' at index 10 is past voice 1's vocabulary
    assert kinds[2].tolist() == [H, R, 23, 127, X, 64, X, X, X, X, X]           # 'C-1': C flat 1; 'C10' is past MIDI 127
    with pytest.raises(ValueError, match='token_kinds'):
        T.token_kinds(np.array(NAMES), [10, 10])
    with pytest.raises(ValueError, match='token_kinds'):
        T.token_kinds(np.array(NAMES), [10, 12, 6])


def test_rhythm_mask_position_by_position():
    T, kinds = _kinds()
    template = torch.tensor([[0, 3, 0], [5, 0, 5], [6, 4, 1], [7, 5, 3], [4, 9, 2]])        # (events, voices)
    m = T.rhythm_mask(template, kinds)
    assert m.shape == (5, 3, 11) and m.dtype == torch.bool
    for e in range(5):
        for c in range(3):
            k = int(kinds[c, template[e, c]])
            for i in range(11):
                ki = int(kinds[c, i])
                want = ki == T.HOLD if k == T.HOLD else ki == T.REST if k == T.REST else True if k == T.META else ki >= 0
                assert bool(m[e, c, i]) == want, (e, c, i)
    assert m[1, 0].tolist() == [False] * 5 + [True] + [False] * 5               # a hold admits the hold alone
    assert m[0, 0].tolist() == [True] * 5 + [False] * 6                         # a note start admits every pitch
    batched = T.rhythm_mask(template.unsqueeze(0).repeat(2, 1, 1), kinds)
    assert batched.shape == (2, 5, 3, 11) and torch.equal(batched[1], m)
    with pytest.raises(ValueError, match='rhythm_mask'):
        T.rhythm_mask(torch.full((5, 3), 11), kinds)


def test_pitch_class_mask_position_by_position():
    T, kinds = _kinds()
    pcs = torch.zeros(3, 12, dtype=torch.bool)
    pcs[0, [0, 4, 7]] = True                                                     # C major triad
    pcs[1, [1, 10]] = True                                                       # C# / D-, B-
    m = T.pitch_class_mask(kinds, pcs)                                           # event 2: no pitch class at all
    assert m.shape == (3, 3, 11)
    for e in range(3):
        for c in range(3):
            for i in range(11):
                k = int(kinds[c, i])
                want = bool(pcs[e, k % 12]) if k >= 0 else k in (T.HOLD, T.REST)
                assert bool(m[e, c, i]) == want, (e, c, i)
    assert m[0, 0].tolist() == [True, False, False, False, False, True, True, False, False, False, False]
    assert m[1, 0].tolist() == [False, True, True, True, False, True, True, False, False, False, False]
    assert m[2, 1].tolist() == [False, False, False, True, True] + [False] * 6
    with pytest.raises(ValueError, match='pitch_class_mask'):
        T.pitch_class_mask(kinds, pcs.long())


def test_range_mask_and_combination():
    T, kinds = _kinds()
    m = T.range_mask(kinds, [58, 43, 0], [60, 57, 64])
    assert m.shape == (1, 3, 11)
    for c, (lo, hi) in enumerate(((58, 60), (43, 57), (0, 64))):
        for i in range(11):
            k = int(kinds[c, i])
            want = lo <= k <= hi if k >= 0 else k in (T.HOLD, T.REST)
            assert bool(m[0, c, i]) == want, (c, i)
    assert m[0, 0].tolist() == [True, False, False, True, False, True, True, False, False, False, False]
    with pytest.raises(ValueError, match='range_mask'):
        T.range_mask(kinds, [0, 0], [127, 127])
    template = torch.tensor([[0, 0, 5], [5, 3, 0]])
    pcs = torch.zeros(2, 12, dtype=torch.bool)
    pcs[:, [0, 10]] = True
    both = T.rhythm_mask(template, kinds) & T.pitch_class_mask(kinds, pcs) & m
    assert both.shape == (2, 3, 11)
    assert both[0, 0].tolist() == [True, False, False, True] + [False] * 7      # a note start, C or B-, inside [58, 60]
    assert both[1, 0].tolist() == [False] * 5 + [True] + [False] * 5
    assert not bool(both[0, 2].any())                                            # E4 alone is pitched and in range, but not C or B-


# ---- the entry point's checks ---------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def lib():
    import torch  # noqa: F401  (loads the process-wide libamdhip64.so.7 first)
    from vqcpc_bach_amd import build, hip
    if not os.path.exists(hip.LIB_PATH):
        build.build(verbose=False)
    return hip.load()


def test_masked_entry_point_rejects_bad_arguments(lib):
    P, Q = 4096, 8192                     # stand-ins: nothing is dereferenced before the checks fail
    f = lib.vqcpc_decode_sample_masked
    offs = (ctypes.c_int32 * 2)(0, 40)

    def call(M=4, temperature=1.0, seeds=Q, cons=Q, ldcons=8, logp=P, ldlogp=8, allowed=Q, ldallow=8, logmass=P, ldmass=8,
             offsets=offs, nc=1, ldl=40, rows=40 * 16 + 1):
        return f(P, ldl, offsets, nc, M, temperature, 0, 1.0, None, seeds, cons, ldcons, logp, ldlogp, None, allowed, ldallow,
                 logmass, ldmass, P, 8, 8, Q, rows, 32, 16, P, 32, None, 0, P, None)
    for kw in (dict(M=65), dict(M=0), dict(seeds=None), dict(temperature=0.0), dict(ldcons=7), dict(ldlogp=7), dict(ldallow=7),
               dict(ldmass=7), dict(ldl=39), dict(rows=40 * 16 - 1),
               dict(offsets=(ctypes.c_int32 * 3)(0, 40, 297), nc=2, ldl=297, rows=257 * 16 + 1)):
        assert call(**kw) == -1, kw
        assert b'decode_sample_masked' in lib.vqcpc_last_error(), (kw, lib.vqcpc_last_error())
