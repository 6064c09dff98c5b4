"""The case tables of the voice-leading kernel tests (tests/test_decode_rules_kernel_gpu.py imports them; tests/
test_rules_reference_cpu.py checks that they cover what they claim).  Everything is seeded numpy: a case is the complete input
of one vqcpc_decode_rules launch, and `expected(case)` the reference's sets and reports for it, computed once per process.

Token layout of a voice with V tokens: 0 HOLD, 1 REST, V - 1 META (V >= 5), every other id a pitch -- consecutive semitones
around the voice's centre, so that crossings, leaps and parallel fifths / octaves are all common; V = 1 is one pitch (even
seed) or HOLD (odd seed).  The centres descend with the voice index, a fifth or a fourth apart for four voices."""
import functools

import numpy as np

import rules_reference as R

SHAPES_M = (1, 3, 64)
SHAPES_NC = (1, 4, 16)
SHAPES_V = (1, 5, 31, 32, 33, 64, 65, 255, 256)
CHAINS = (0, 1, 63, 64, 65, 200)
TICKS_PER_CODE = 4


def make_kinds(rng, nc, vocab, seed):
    vmax = max(vocab)
    kinds = np.full((nc, vmax), R.META, dtype=np.int32)
    for u, V in enumerate(vocab):
        centre = 66 if nc == 1 else (76, 69, 64, 57)[u] if nc <= 4 else 80 - 3 * u
        if V == 1:
            kinds[u, 0] = centre if seed % 2 == 0 else R.HOLD
            continue
        special = [R.HOLD, R.REST][:min(V - 1, 2)]
        n = V - len(special) - (1 if V >= 5 else 0)
        kinds[u, :len(special)] = special
        kinds[u, len(special):len(special) + n] = np.clip(centre - n // 2 + np.arange(n), 0, 127)
    return kinds


def _ids(kinds, vocab, u, want):
    """token ids of voice u: want 'pitch' / 'hold' / 'any'."""
    k = kinds[u, :vocab[u]]
    if want == 'pitch':
        return np.nonzero(k >= 0)[0]
    if want == 'hold':
        return np.nonzero(k == R.HOLD)[0]
    return np.arange(vocab[u])


def _pick(rng, ids, fallback):
    return int(ids[rng.integers(len(ids))]) if len(ids) else int(fallback)


def make_case(cid, M, nc, V, chain, mode='fixed', static='none', exclude='none', enabled=7, forced=0.25, leap=4, to_zero=False,
              win_off=False, small_ld=False, past_T=False, other_V=None, parallel_only=False):
    """mode 'fixed': win NULL, col = pos; 'long': window index given, the history crosses from `tokens` into `chorale`.
    parallel_only (nc = 4, V = 31, static 'tight'): voice 0 moves by a step from a fifth or an octave above voice 1, whose set
    holds the one token that follows it in parallel -- within the leap, below voice 0: only PARALLEL can give way."""
    rng = np.random.default_rng(1000 + cid)
    U = TICKS_PER_CODE * nc
    v = 1 if parallel_only else int(rng.integers(nc))
    vocab = [int(V if u == v or other_V is None else other_V[(u + cid) % len(other_V)]) for u in range(nc)]
    kinds = make_kinds(rng, nc, vocab, cid)
    if mode == 'fixed':
        e = chain + 1 + int(rng.integers(3)) if not to_zero else chain
        S = e // TICKS_PER_CODE + 1
        T, w0, nb = S * U, 0, 0
        pos = e * nc + v
    else:
        S = 3
        T = S * U
        e_in = int(rng.integers(1, S * TICKS_PER_CODE))              # tick inside the window: shorter than every chain >= 63
        need = max(0, chain + 1 - e_in)
        w0 = (need + TICKS_PER_CODE - 1) // TICKS_PER_CODE + (0 if to_zero else int(rng.integers(1, 3)))
        if to_zero:
            chain = w0 * TICKS_PER_CODE + e_in
        e = w0 * TICKS_PER_CODE + e_in
        nb = w0 + S
        pos = e_in * nc + v
    col = e * nc + v
    width = max(nb * U, T)
    rows = np.zeros((M, width), dtype=np.int64)                       # chorale coordinates
    for b in range(M):
        for u in range(nc):
            rows[b, u::nc] = rng.integers(0, vocab[u], size=len(rows[b, u::nc]))
            L = chain if u == v or rng.random() < 0.5 else int(rng.integers(0, 3))
            hold = _ids(kinds, vocab, u, 'hold')
            if len(hold) and L > 0:
                for t in range(max(0, e - L), e):
                    rows[b, t * nc + u] = hold[0]
            if e - 1 - L >= 0 and (L > 0 or rng.random() < 0.8):
                rows[b, (e - 1 - L) * nc + u] = _pick(rng, _ids(kinds, vocab, u, 'pitch'), rows[b, (e - 1 - L) * nc + u])
            if u < v and rng.random() < 0.8:                          # this tick's upper voices: mostly pitched or held
                want = 'pitch' if rng.random() < 0.7 else 'hold'
                rows[b, e * nc + u] = _pick(rng, _ids(kinds, vocab, u, want), rows[b, e * nc + u])
    constraint = np.full((M, width), -1, dtype=np.int64)
    for b in range(M):
        for u in range(v + 1, nc):
            if rng.random() < 0.6:
                want = 'pitch' if rng.random() < 0.7 else 'hold'
                constraint[b, e * nc + u] = _pick(rng, _ids(kinds, vocab, u, want), 0)
        if rng.random() < forced:
            constraint[b, col] = int(rng.integers(vocab[v]))
    only = None
    if parallel_only:
        tok = lambda u, p: int(np.nonzero(kinds[u, :vocab[u]] == p)[0][0])
        only = np.zeros(M, dtype=np.int64)
        for b in range(M):
            a, d, gap = int(rng.integers(72, 79)), int(rng.choice([-2, -1, 1, 2])), int(rng.choice([7, 12]))
            rows[b, (e - 1) * nc + 0], rows[b, (e - 1) * nc + 1] = tok(0, a), tok(1, a - gap)
            rows[b, e * nc + 0] = tok(0, a + d)
            only[b] = tok(1, a + d - gap)
            constraint[b, e * nc:(e + 1) * nc] = -1
    excl, keep = None, int(rng.integers(vocab[v]))
    if exclude != 'none':
        excl = rng.random((nc, 256)) < (0.15 if exclude == 'random' else 0.85)
        excl[v, keep] = False                                         # a token of the vocabulary survives ...
    stat = None
    if static != 'none':
        bits = rng.random((M, width, 256)) < (0.5 if static == 'random' else 0.0)
        for b in range(M):
            n = 1 if static == 'tight' else 2
            bits[b, col, rng.integers(0, vocab[v], size=n) if only is None else only[b]] = True     # a token of the vocabulary
            if excl is not None:
                bits[b, col, keep] = True                             # ... in every E
            if constraint[b, col] >= 0:
                bits[b, col, constraint[b, col]] = True
        stat = R.pack(bits)
    base = w0 * U
    tokens = np.zeros((M, T), dtype=np.int64)
    n_live = min(T, width - base)
    tokens[:, :n_live] = rows[:, base:base + n_live]
    chorale = rows.copy() if mode == 'long' else None
    if chorale is not None:
        chorale[:, base:] = 0                                         # the live window is not committed yet
    max_leap = np.array([leap if (u + cid) % 3 else -1 for u in range(nc)], dtype=np.int32)
    max_leap[v] = leap
    return dict(id=cid, M=M, nc=nc, vocab=vocab, kinds=kinds, max_leap=max_leap, enabled=enabled, mode=mode, T=T, U=U, pos=pos,
                w0=w0, col=col, v=v, e=e, width=width, rows=rows, tokens=tokens, chorale=chorale, constraint=constraint,
                static=stat, exclude=excl, chain=chain, to_zero=to_zero, win_off=win_off, small_ld=small_ld, past_T=past_T)


def _table():
    cases, cid = [], 0

    def add(**kw):
        nonlocal cid
        cases.append(make_case(cid, **kw))
        cid += 1
    others = (5, 31, 33, 64)
    # every vocabulary size with every voice count; M, the chain and the static / exclude kinds cycle through their values
    k = 0
    for V in SHAPES_V:
        for nc in SHAPES_NC:
            M = SHAPES_M[k % 3] if not (V >= 64 and nc == 16 and SHAPES_M[k % 3] == 64) else 3
            add(M=M, nc=nc, V=V, chain=CHAINS[k % 6] if V > 1 else k % 2, mode='long' if k % 2 else 'fixed',
                static=('none', 'random', 'tight')[k % 3], exclude=('none', 'random', 'heavy', 'none')[k % 4],
                enabled=(7, 7, 5, 3, 6, 7, 1, 2, 4)[k % 9], other_V=others, leap=(4, 2, 7)[k % 3])
            k += 1
    # every chain length in both modes, also chains that run into column 0
    for chain in CHAINS:
        for mode in ('fixed', 'long'):
            add(M=3, nc=4, V=31, chain=chain, mode=mode, static='tight' if chain % 2 else 'none', exclude='none')
            add(M=1, nc=4, V=33, chain=chain, mode=mode, to_zero=True, static='none', exclude='random')
    # sets so tight that the rules have to give way, level by level; an exclude that drains what the rules leave
    for i in range(18):
        add(M=3, nc=4, V=(5, 31, 64)[i % 3], chain=i % 3, mode='long' if i % 2 else 'fixed', static='tight',
            exclude=('none', 'heavy')[i % 2], leap=(0, 1, 2)[i % 3], forced=0.0)
    for i in range(6):
        add(M=64, nc=4, V=(5, 33, 65)[i % 3], chain=(1, 64)[i % 2], mode='long' if i % 2 else 'fixed', static=('random', 'none')[i % 2],
            exclude=('heavy', 'random')[i % 2], forced=0.4)
    for i in range(6):
        add(M=3, nc=4, V=31, chain=0, mode='long' if i % 2 else 'fixed', static='tight', leap=4, forced=0.0, parallel_only=True)
    # nothing may happen: no live window, columns at and past the leading dimensions, pos >= T
    add(M=3, nc=4, V=31, chain=1, mode='long', win_off=True)
    add(M=3, nc=4, V=31, chain=63, mode='long', small_ld=True, static='random')
    add(M=3, nc=4, V=31, chain=1, mode='fixed', past_T=True)
    return cases


CASES = _table()


@functools.lru_cache(maxsize=None)
def expected(cid):
    """-> (sets bool (M, 256), report int32 (M,)) at the case's column, by the reference."""
    c = CASES[cid]
    sets = np.zeros((c['M'], 256), dtype=bool)
    report = np.zeros(c['M'], dtype=np.int32)
    for b in range(c['M']):
        stat = None if c['static'] is None else R.unpack(c['static'][b, c['col']])
        excl = None if c['exclude'] is None else c['exclude'][c['v']]
        sets[b], report[b] = R.position(c['rows'][b], c['col'], c['nc'], c['kinds'], c['vocab'], c['max_leap'], c['enabled'],
                                        c['constraint'][b], stat, excl)
    return sets, report


def audit_piece(seed, rows, ticks, nc=4, V=31):
    """A random piece for the audit kernel: long holds, rests and pitches.  -> (x (rows, ticks * nc), kinds, vocab, max_leap)"""
    rng = np.random.default_rng(seed)
    vocab = [V + u for u in range(nc)]
    kinds = make_kinds(rng, nc, vocab, seed)
    x = np.zeros((rows, ticks * nc), dtype=np.int64)
    for u in range(nc):
        draw = rng.integers(0, vocab[u], size=(rows, ticks))
        draw[rng.random((rows, ticks)) < 0.6] = 0                     # HOLD: chains of every length, also from column 0
        x[:, u::nc] = draw
    return x, kinds, vocab, np.array([5, -1, 7, 3][:nc] + [4] * max(0, nc - 4), dtype=np.int32)
