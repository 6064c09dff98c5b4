"""Pins tests/particles_reference.py, the numpy statement of the particle filter that csrc/particles.hip follows, and checks that
the inputs of the GPU kernel cases (tests/particles_cases.py) are what their names claim.  No GPU."""
import math

import numpy as np
import pytest

import particles_cases as K
import particles_reference as R

F = np.float32


def _random_wn(rng, P, spread):
    lw = (-rng.random(P) * spread).astype(F)
    return R.group_weights(lw)[0]


@pytest.mark.parametrize('P', [2, 3, 5, 8, 64])
def test_systematic_resampling_copies_each_member_floor_or_ceil_times(P):
    rng = np.random.default_rng(P)
    for trial in range(40):
        wn = _random_wn(rng, P, spread=[0.0, 1.0, 8.0, 40.0][trial % 4])
        u = F(rng.integers(0, 1 << 24) * 2.0 ** -24)
        anc = R.systematic_ancestors(wn, u)
        assert anc.dtype == np.int32 and anc.min() >= 0 and anc.max() < P
        assert (np.diff(anc) >= 0).all()
        n = R.copies(anc, P)
        expect = P * wn.astype(np.float64)
        slack = 4 * P * R.EPS * P                       # the running fp32 sum against the exact one, in copies
        assert (n >= np.floor(expect - slack)).all() and (n <= np.ceil(expect + slack)).all(), (wn, u, n)
        assert n.sum() == P


def test_mean_copy_count_over_a_grid_of_u_is_P_wn():
    P, steps = 5, 512
    wn = _random_wn(np.random.default_rng(3), P, spread=3.0)
    total = np.zeros(P)
    for i in range(steps):
        total += R.copies(R.systematic_ancestors(wn, F(i / steps)), P)
    assert np.abs(total / steps - P * wn.astype(np.float64)).max() <= 1.0 / steps + 1e-5


def test_uniform_is_the_python_splitmix_restatement_bit_for_bit():
    def mix(z):
        z = (z + 0x9E3779B97F4A7C15) % 2 ** 64
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) % 2 ** 64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) % 2 ** 64
        return z ^ (z >> 31)
    assert R.SEED_MUL % 2 == 1 and R.SEED_MUL.bit_length() == 64
    assert R.splitmix64(0) == 0xE220A8397B1DCDAF                     # the published first output of splitmix64 seeded with 0
    for seed in (0, 1, -1, 2 ** 63 - 1, -2 ** 63, 123456789012345):
        for c in (0, 1, 7, 95):
            z = mix((seed % 2 ** 64) ^ ((c + 1) * R.SEED_MUL % 2 ** 64))
            want = (z >> 40) / 2.0 ** 24
            u = R.uniform(seed, c)
            assert u.dtype == F and float(u) == want and 0.0 <= want < 1.0
    assert R.uniform(5, 0) != R.uniform(5, 1) and R.uniform(5, 0) != R.uniform(6, 0)


def test_update_lw_adds_logp_where_forced_else_the_mass_in_column_order():
    U, c = 4, 1
    cons = np.array([[9, 9, 9, 9, 3, -1, 5, -1, 9]], dtype=np.int64)
    logp = np.array([[np.nan] * 4 + [-1.0, np.nan, -2.0, np.nan, np.nan]], dtype=F)
    mass = np.array([[np.nan] * 4 + [np.nan, -0.25, np.nan, -0.5, np.nan]], dtype=F)
    assert R.update_lw(np.zeros(1, F), c, U, cons, logp, mass)[0] == F(-3.75)
    assert R.update_lw(np.zeros(1, F), c, U, cons, logp, None)[0] == F(-3.0)
    assert R.update_lw(np.ones(1, F), c, U, None, logp, None)[0] == F(1.0)            # nothing forced, no sets: weights stay
    every = np.array([[np.nan] * 4 + [-0.25, -0.5, -1.0, -2.0]], dtype=F)
    assert R.update_lw(np.zeros(1, F), c, U, None, None, every)[0] == F(-3.75)        # no constraint: every position's mass
    assert R.update_lw(np.zeros(1, F), c, U, None, None, every[:, :6])[0] == F(-0.75)  # columns past the width add nothing
    logp[0, 4] = np.nan
    assert R.update_lw(np.zeros(1, F), c, U, cons, logp, mass)[0] == -np.inf          # NaN counts as -inf


def test_evidence_identities():
    rng = np.random.default_rng(11)
    for P in (2, 5, 64):
        lw = (-rng.random(P) * 9).astype(F)
        wn, ess, inc, dead = R.group_weights(lw)
        wn64, ess64, inc64, dmax = R.group_weights64(lw)
        assert not dead and abs(float(wn.sum()) - 1.0) < 4 * P * R.EPS
        assert inc64 == pytest.approx(math.log(np.exp(lw.astype(np.float64)).mean()), abs=1e-12)    # log of the mean weight
        assert (np.abs(wn - wn64) <= R.wn_bound(wn64, dmax, P)).all()
        assert abs(float(ess) - ess64) <= R.ess_bound(ess64, dmax, P)
        assert abs(float(inc) - inc64) <= R.inc_bound(float(lw.max()), inc64, dmax, P)
        assert 1.0 <= ess64 <= P
        # equal weights: ess = P and the increment is the common log-weight; a shift of every lw shifts the increment only
        same = np.full(P, F(-2.5))
        wn_s, ess_s, inc_s, _ = R.group_weights(same)
        assert (wn_s == F(1.0) / F(P)).all() and abs(float(ess_s) - P) <= 4 * P * R.EPS * P and abs(float(inc_s) + 2.5) < 1e-5
        assert np.abs(R.group_weights64(lw - F(3.0))[0] - wn64).max() < 1e-6
        assert R.group_weights64(lw - F(3.0))[2] == pytest.approx(inc64 - 3.0, abs=1e-5)
    # one survivor: weight one, ess one, the increment is its log-weight minus log P
    wn, ess, inc, dead = R.group_weights(np.array([-np.inf, -4.0, -np.inf], dtype=F))
    assert list(wn) == [0.0, 1.0, 0.0] and ess == 1.0 and not dead and abs(float(inc) - (-4.0 - math.log(3))) < 1e-6
    # nobody: uniform weights, evidence -inf, never resampled -- not even when forced
    wn, ess, inc, dead = R.group_weights(np.full(4, -np.inf, dtype=F))
    assert dead and (wn == 0.25).all() and inc == -np.inf
    assert not R.decide(ess, 1.0, 4, True, dead)
    out = R.resample(np.full(4, -np.inf, dtype=F), np.zeros(1, F), np.arange(4), 0, 1, 4, 1.0, force=True)
    assert out['evidence'][0] == -np.inf and out['flag'] == 0 and not out['resampled'][0]


def test_resampling_adds_the_increment_and_resets_the_weights_and_the_threshold_is_strict():
    lw = np.array([0.0, -1.0, -2.0, -3.0, -5.0, -5.0, -5.0, -5.0], dtype=F)
    seeds = np.arange(8, dtype=np.int64) * 77
    out = R.resample(lw, np.array([1.0, 2.0], F), seeds, 0, 2, 4, 0.75)
    assert list(out['resampled']) == [True, False]                   # group 1 is uniform: ess = 4, not below 3
    assert (out['lw'][:4] == 0).all() and (out['lw'][4:] == lw[4:]).all()
    assert out['evidence'][0] == F(F(1.0) + out['pending'][0]) and out['evidence'][1] == 2.0
    assert (out['ancestors'][4:] == np.arange(4, 8)).all()
    assert (out['ancestors'][:4] == R.systematic_ancestors(out['wn'][:4], R.uniform(seeds[0], 0))).all()
    never = R.resample(lw, np.zeros(2, F), seeds, 0, 2, 4, 0.0)
    assert not never['resampled'].any() and never['flag'] == 0 and (never['lw'] == lw).all()
    assert R.decide(F(4.0), 1.0, 4, False, False) is False and R.decide(F(3.9999998), 1.0, 4, False, False) is True


@pytest.mark.parametrize('name', sorted(K.RESAMPLE_CASES))
def test_resample_cases_are_what_they_claim(name):
    x = K.resample_inputs(name)
    P, G, M, U, c = x['P'], x['G'], x['M'], x['U'], x['c']
    assert 2 <= P <= 64 and M == G * P <= 64 and x['constraint'].shape == x['logp'].shape == (M, x['ld'])
    assert c == (x['pos'] // U - 1 if x['win'] is None else int(x['win'][1]) + x['pos'] // U - 1) and (c + 1) * U <= x['ld']
    cols = slice(c * U, (c + 1) * U)
    forced = x['constraint'][:, cols] >= 0
    assert forced.any(axis=1).all() and (~forced).any(axis=1).all()
    # NaN wherever the kernel must not read: other codes, logp at free positions, logmass at forced ones
    outside = np.ones(x['ld'], dtype=bool)
    outside[cols] = False
    assert np.isnan(x['logp'][:, outside]).all() and np.isnan(x['logp'][:, cols][~forced]).all()
    if x['logmass'] is not None:
        assert np.isnan(x['logmass'][:, outside]).all() and np.isnan(x['logmass'][:, cols][forced]).all()
        assert np.isfinite(x['logmass'][:, cols][~forced]).all()
    ref = R.resample(x['lw'], x['evidence'], x['seeds'], c, U, P, x['threshold'], x['force'], x['constraint'], x['logp'],
                     x['logmass'])
    for g, kind in enumerate(x['kinds']):
        rows = slice(g * P, (g + 1) * P)
        lw, wn, anc = ref['lw_updated'][rows], ref['wn'][rows], ref['ancestors'][rows] - g * P
        if kind == 'uniform':
            assert (lw == lw[0]).all() and np.isfinite(lw).all() and (wn == F(1.0) / F(P)).all()
            assert (anc == np.arange(P)).all()
            if x['threshold'] < 1.0:                                 # at 1 the rounding of ess decides; nothing moves either way
                assert ref['resampled'][g] == bool(x['force'])
        elif kind == 'dominant':
            j = x['dominant'][g]
            assert wn[j] == 1.0 and wn.sum() == 1.0
            if x['force'] or x['threshold'] > 0:
                assert ref['resampled'][g] and (anc == j).all()
        elif kind == 'inf':
            assert np.isinf(lw).any() and np.isfinite(lw).any() and (wn[np.isinf(lw)] == 0).all()
            assert not np.isin(anc[anc != np.arange(P)], np.nonzero(np.isinf(lw))[0]).any()
        elif kind == 'dead':
            assert np.isinf(lw).all() and not ref['resampled'][g] and ref['evidence'][g] == -np.inf
        elif kind == 'nan':
            assert np.isnan(x['logp'][rows, cols][forced[rows]]).sum() == 1 and np.isinf(lw).sum() == 1
        else:
            assert np.isfinite(lw).all() and len(set(lw.tolist())) == P
    if x['threshold'] == 0.0 and not x['force']:
        assert not ref['resampled'].any() and ref['flag'] == 0
    if x['force']:
        assert ref['resampled'].sum() == sum(k != 'dead' for k in x['kinds'])
    if name in ('p8_threshold1', 'p64_random', 'p5_mixed_half', 'p8_forced', 'p2_full_stack'):
        assert ref['flag'] == 1


@pytest.mark.parametrize('name', sorted(K.PERMUTE_CASES))
def test_permute_cases_are_what_they_claim(name):
    x = K.permute_inputs(name)
    P, M, anc = x['P'], x['M'], x['ancestors']
    assert M <= 64 and anc.dtype == np.int32 and ((anc // P) == (np.arange(M) // P)).all()       # nobody leaves its group
    assert 0 <= x['pos'] <= x['W'] and x['d'] % 4 == 0
    moved = bool((anc != np.arange(M)).any())
    assert moved == (x['map'] != 'identity')
    if x['map'] in ('shift', 'swap'):
        assert K.has_cycle(anc, P) and sorted(anc.tolist()) == list(range(M))                   # a permutation with cycles
    if x['map'] == 'all_to_one':
        assert all(len(set(anc[g * P:(g + 1) * P].tolist())) == 1 for g in range(x['G']))
    if name in ('random_p64', 'random_posW', 'wide'):
        assert K.has_cycle(anc, P)
    buf = np.arange(2 * M * 5, dtype=np.int64).reshape(2, M, 5)
    out = R.permute_rows(buf, anc, 3)
    assert (out[:, :, 3:] == buf[:, :, 3:]).all() and (out[1, :, :3] == buf[1, anc, :3]).all()
