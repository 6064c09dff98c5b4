"""The inputs of the direct kernel tests of csrc/particles.hip (tests/test_particle_kernels_gpu.py), built from seeds on the
host so that tests/test_particles_reference_cpu.py can check, without a GPU, that every case is what its name claims."""
import numpy as np

F = np.float32

# name: P, groups' kinds, U, threshold, force, windowed (w1, t_relative) or None, use_mass
#   kinds: 'random' (spread weights), 'uniform' (equal weights), 'dominant' (one member carries everything), 'inf' (some
#   members -inf), 'dead' (every member -inf), 'nan' (a NaN score at a used position)
RESAMPLE_CASES = {
    'p2_one_group': dict(P=2, kinds=['random'], U=4, threshold=1.0, force=0, window=None, mass=False),
    'p3_windowed': dict(P=3, kinds=['random', 'dominant', 'uniform'], U=5, threshold=1.0, force=0, window=(2, 1), mass=True),
    'p5_mixed_half': dict(P=5, kinds=['random', 'inf', 'dead', 'nan', 'uniform', 'dominant'], U=16, threshold=0.5, force=0,
                          window=None, mass=True),
    'p8_threshold0': dict(P=8, kinds=['random', 'dominant', 'inf', 'random'], U=16, threshold=0.0, force=0, window=(3, 0),
                          mass=False),
    'p8_threshold1': dict(P=8, kinds=['random'] * 6 + ['uniform', 'dead'], U=16, threshold=1.0, force=0, window=(0, 2),
                          mass=True),
    'p8_forced': dict(P=8, kinds=['uniform', 'random', 'dead', 'inf', 'dominant', 'nan', 'random', 'random'], U=3, threshold=0.0,
                      force=1, window=None, mass=True),
    'p8_uniform_below1': dict(P=8, kinds=['uniform'] * 3, U=16, threshold=0.99, force=0, window=None, mass=False),
    'p64_random': dict(P=64, kinds=['random'], U=16, threshold=1.0, force=0, window=(1, 1), mass=True),
    'p64_dominant_forced': dict(P=64, kinds=['dominant'], U=2, threshold=0.0, force=1, window=None, mass=False),
    'p2_full_stack': dict(P=2, kinds=['random', 'uniform', 'dominant', 'inf'] * 8, U=4, threshold=1.0, force=0, window=None,
                          mass=True),
}


def resample_inputs(name):
    """-> dict of numpy inputs: lw, evidence, seeds, constraint, logp, logmass (None without sets), pos, win (None: fixed window),
    c, U, P, M, G, threshold, force, ld, dominant (the dominant member of each 'dominant' group)."""
    case = RESAMPLE_CASES[name]
    P, kinds, U = case['P'], case['kinds'], case['U']
    G = len(kinds)
    M = G * P
    rng = np.random.default_rng(sum(name.encode()) * 7919 + P)
    if case['window'] is None:
        c = int(rng.integers(0, 3))
        pos, win = (c + 1) * U, None
    else:
        w1, tr = case['window']
        c, pos, win = w1 + tr, (tr + 1) * U, np.array([w1 + 1, w1], dtype=np.int32)
    ld = (c + 1) * U + 3                                         # columns past the code: never read
    constraint = np.full((M, ld), -1, dtype=np.int64)
    logp = np.full((M, ld), np.nan, dtype=F)                     # NaN wherever the kernel must not look
    logmass = np.full((M, ld), np.nan, dtype=F) if case['mass'] else None
    lw = np.zeros(M, dtype=F)
    dominant = {}
    for g, kind in enumerate(kinds):
        rows = np.arange(g * P, (g + 1) * P)
        forced = rng.random(U) < 0.5
        forced[0], forced[U - 1] = True, U == 1                  # a forced and (U > 1) a free position in every code
        cols = c * U + np.arange(U)
        constraint[np.ix_(rows, cols[forced])] = rng.integers(0, 50, size=(P, int(forced.sum())))
        constraint[rows, :c * U] = rng.integers(-1, 50, size=(P, c * U))          # other codes: forced or not, never read
        lp = -rng.random((P, int(forced.sum()))).astype(F) * 3
        if kind == 'uniform':
            lp[:] = lp[0]
        elif kind == 'dominant':
            j = int(rng.integers(0, P))
            dominant[g] = j
            lp[:, 0] = -200.0
            lp[j, 0] = -1.0
        elif kind == 'inf':
            lp[rng.permutation(P)[:max(1, P // 2)], 0] = -np.inf
        elif kind == 'dead':
            lp[:, 0] = -np.inf
        elif kind == 'nan':
            lp[int(rng.integers(0, P)), 0] = np.nan
        if kind in ('random', 'inf', 'nan'):
            lw[rows] = (-rng.random(P) * 6).astype(F)            # weights carried over from earlier codes
        logp[np.ix_(rows, cols[forced])] = lp
        if logmass is not None:
            lm = -rng.random((P, int((~forced).sum()))).astype(F)
            if kind in ('uniform', 'dominant'):
                lm[:] = lm[0]
            logmass[np.ix_(rows, cols[~forced])] = lm
    seeds = rng.integers(-2 ** 63, 2 ** 63 - 1, size=M, dtype=np.int64)
    evidence = (-rng.random(G) * 5).astype(F)
    return dict(lw=lw, evidence=evidence, seeds=seeds, constraint=constraint, logp=logp, logmass=logmass, pos=pos, win=win, c=c,
                U=U, P=P, M=M, G=G, threshold=case['threshold'], force=case['force'], ld=ld, dominant=dominant, kinds=kinds)


# name: P, G, map kind, rows x columns of the row buffers, pos, and the cache shape (layers, W, d)
PERMUTE_CASES = {
    'identity': dict(P=4, G=2, map='identity', pos=5),
    'all_to_one': dict(P=5, G=3, map='all_to_one', pos=8),
    'cyclic_shift': dict(P=8, G=2, map='shift', pos=7),
    'swap': dict(P=2, G=4, map='swap', pos=8),
    'random_p3': dict(P=3, G=7, map='random', pos=3),
    'random_p64': dict(P=64, G=1, map='random', pos=6, d=48),                   # 6 * 12 float4 columns: tiles of 32, the last partial
    'random_pos0': dict(P=8, G=8, map='random', pos=0),
    'random_pos1': dict(P=8, G=8, map='random', pos=1),
    'random_posW': dict(P=16, G=4, map='random', pos=8),
    'wide': dict(P=6, G=2, map='random', pos=37, layers=3, W=40, d=136),        # 37 * 34 float4 columns: tiles of 320, the last partial
}


def permute_inputs(name):
    """-> dict: ancestors (M,) int32 row indices, P, G, M, pos, layers, W, d."""
    case = dict(layers=2, W=8, d=16)
    case.update(PERMUTE_CASES[name])
    P, G = case['P'], case['G']
    M = G * P
    rng = np.random.default_rng(sum(name.encode()) * 104729 + P)
    anc = np.arange(M, dtype=np.int32)
    for g in range(G):
        base = g * P
        if case['map'] == 'all_to_one':
            anc[base:base + P] = base + int(rng.integers(0, P))
        elif case['map'] == 'shift':
            anc[base:base + P] = base + (np.arange(P) + 1 + g) % P
        elif case['map'] == 'swap':
            anc[base:base + P] = base + np.arange(P)[::-1]
        elif case['map'] == 'random':
            anc[base:base + P] = base + rng.integers(0, P, size=P)
    case.update(ancestors=anc, M=M)
    return case


def has_cycle(ancestors, P):
    """Whether some group's map sends a row k != a to a while a itself is overwritten -- the in-place hazard: a row that is
    read as an ancestor and written as a descendant."""
    anc = np.asarray(ancestors)
    rows = np.arange(anc.shape[0])
    written = anc != rows
    read = np.zeros_like(written)
    read[anc[written]] = True
    return bool((written & read).any())
