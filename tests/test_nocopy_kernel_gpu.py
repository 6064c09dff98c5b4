"""The copy guard's kernels called directly (vqcpc_bach_amd/csrc/nocopy.hip; include/vqcpc.h, "Copy guard"): sets and reports bit
for bit against tests/nocopy_reference.py, which scans the pieces without an index.  Rows are built so that matches abound: a row
quotes a piece up to the column (mode 0), quotes it but for the token max_copy back (1), quotes a piece from its very first token (2),
quotes across a piece boundary (3: no ban), quotes the right tokens in the wrong voice (4), or is random (5)."""
import ctypes

import numpy as np
import pytest
import torch

import nocopy_reference as N

pytestmark = pytest.mark.gpu

FILL = 0x5A5A5A5A


def _corpus(pieces, V):
    from vqcpc_bach_amd.dataloaders.corpus import Corpus, DeviceCorpus
    tokens = np.concatenate(pieces, axis=0).astype(np.int32)
    start = np.concatenate([[0], np.cumsum([p.shape[0] for p in pieces])])
    zero = np.zeros(4, dtype=np.int64)
    return DeviceCorpus(Corpus(tokens, start, 1, [V] * 4, zero, zero, zero), 'cuda')


def _pieces(ticks, V, seed):
    rng = np.random.RandomState(seed)
    return [rng.randint(0, V, size=(t, 4)).astype(np.int64) for t in ticks]


def _rows(pieces, n, col, M, width, V, rng):
    """(rows (M, width) in chorale coordinates, the mode of every row)."""
    rows = rng.randint(0, V, size=(M, width)).astype(np.int64)
    modes = np.full(M, 5)
    long = [i for i, p in enumerate(pieces) if p.size > n + 1]
    if col < n or not long:
        return rows, modes
    for b in range(M):
        mode = b % 6
        p = long[rng.randint(len(long))]
        flat = pieces[p].reshape(-1)
        js = [j for j in range(n, flat.size - 1) if j % 4 == col % 4]
        j = js[rng.randint(len(js))]
        if mode == 2 and n % 4 == col % 4:
            j = n                                           # the context is the piece's first n tokens
        elif mode == 2:
            mode = 0
        if mode == 3:
            s = (n - col - 1) % 4 + 1                       # tokens taken from the end of the piece before
            if p == 0 or n <= s or pieces[p - 1].size < s:
                mode = 0
            else:
                rows[b, col - n:col] = np.concatenate([pieces[p - 1].reshape(-1)[-s:], flat[:n - s]])
        if mode == 4:
            j += 1                                          # the same tokens, one voice off
        if mode in (0, 1, 2, 4):
            L = min(col, j)
            rows[b, col - L:col] = flat[j - L:j]
        if mode == 1:
            rows[b, col - n] = (rows[b, col - n] + 1) % V
        modes[b] = mode
    return rows, modes


def _offsets(vocab):
    off = np.concatenate([[0], np.cumsum(vocab)])
    return (ctypes.c_int32 * 5)(*[int(o) for o in off])


def _i32(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def launch(ix, vocab, rows, col, T=None, U=None, w0=None, cons=None, static=None, exclude=None, in_place=False, extra=3, M=None):
    """One launch at chorale column `col` of rows (M, width).  Fixed window (w0 None): tokens = rows, pos = col.  Windowed: the live
    window is [w0 * U, w0 * U + T), the chorale holds garbage at and past it.  -> (sets (M, ld, 256) bool, report (M, ld), the raw
    buffers) with ld = width + extra guard columns."""
    from vqcpc_bach_amd import hip
    rows = np.asarray(rows)
    M = rows.shape[0] if M is None else M
    width = rows.shape[1]
    ld = width + extra
    if w0 is None:
        T = width if T is None else T
        tokens, chorale, win, U, pos = _i32(rows[:, :T]), None, None, 1, col
    else:
        base = w0 * U
        tokens = np.zeros((M, T), dtype=np.int64)
        live = rows[:, base:base + T]
        tokens[:, :live.shape[1]] = live
        tokens, ch = _i32(tokens), rows.copy()
        ch[:, base:] = 255
        chorale, win, pos = _i32(ch), torch.tensor([w0 + 1, w0], dtype=torch.int32).cuda(), col - base
    sets = torch.full((M, ld, 8), FILL, dtype=torch.int32).cuda()
    report = torch.full((M, ld), FILL, dtype=torch.int32).cuda()
    stat = None
    if static is not None:
        packed = np.full((M, ld, 8), FILL, dtype=np.int32)
        packed[:, :width] = N.pack(static)
        if in_place:
            sets = _i32(packed)
            stat = sets
        else:
            stat = _i32(packed)
    cons_t = None if cons is None else _i32(np.asarray(cons, dtype=np.int64))
    excl = None if exclude is None else _i32(N.pack(exclude))
    posd = torch.tensor([pos], dtype=torch.int32).cuda()
    before = sets.clone()
    hip.call('vqcpc_decode_nocopy', tokens, tokens.shape[1], tokens.shape[1], chorale, width if chorale is not None else 0,
             cons_t, width, *ix.args(), _offsets(vocab), 4, excl, stat, ld, sets, ld, report, ld, posd, win, U, M)
    torch.cuda.synchronize()
    return sets.cpu().numpy(), report.cpu().numpy(), before.cpu().numpy()


def want(pieces, n, vocab, rows, col, cons=None, static=None, exclude=None):
    out = [N.position(rows[b], col, n, pieces, vocab, None if cons is None else cons[b], None if static is None else static[b, col],
                      None if exclude is None else exclude[col % 4]) for b in range(rows.shape[0])]
    return np.stack([o[0] for o in out]), np.array([o[1] for o in out], dtype=np.int32)


def check(got, pieces, n, vocab, rows, col, **kw):
    sets, report, before = got
    ws, wr = want(pieces, n, vocab, rows, col, **kw)
    assert np.array_equal(report[:, col], wr), (col, report[:, col], wr)
    assert np.array_equal(N.unpack(sets[:, col]), ws), col
    # guard cells: nothing but the live column is written
    sets2, report2 = sets.copy(), report.copy()
    sets2[:, col], report2[:, col] = before[:, col], FILL
    assert np.array_equal(sets2, before) and bool((report2 == FILL).all())
    return wr


# ---- the grid of the issue: M x n x vocabulary, columns below, at and above n -------------------------------------------------
@pytest.mark.parametrize('n', [1, 2, 5, 63, 64, 65, 130, 512])
@pytest.mark.parametrize('M,V', [(1, 3), (3, 2), (64, 5), (64, 256)])
def test_sets_and_reports_equal_the_reference(M, V, n):
    rng = np.random.RandomState(1000 * M + 10 * V + n)
    pieces = _pieces([n // 4 + 40, 3, n // 4 + 2, 2 * (n // 4) + 9], V, seed=n + V)
    ix = _corpus(pieces, V).copy_index(n)
    assert ix.max_copy == n and ix.vocab == (V,) * 4 and ix.pieces == (0, 4) and 0 < ix.entries <= ix.entries_before
    assert bool((ix.keys[1:] >= ix.keys[:-1]).all()) and bool((ix.keys >= 0).all())
    width = n + 24
    seen = crossing = 0
    for col in (n - 1, n, n + 1, n + 6, width - 1):
        if col < 0:
            continue
        rows, modes = _rows(pieces, n, col, M, width, V, rng)
        wr = check(launch(ix, [V] * 4, rows, col), pieces, n, [V] * 4, rows, col)
        if col < n:
            assert bool((wr == 0).all())
        elif M == 64:
            assert bool((wr[modes == 0] > 0).all())         # a quotation bans its continuation
            seen += int((wr[modes == 2] > 0).sum())
            crossing += int((modes == 3).sum())
            if V == 256:                                    # no chance match elsewhere: across a piece boundary nothing is banned
                assert bool((wr[modes == 3] == 0).all())
    assert M < 64 or seen > 0                               # the context that fills a piece from its first token was met
    assert M < 64 or n < 5 or crossing > 0                  # and so was the one that would cross a piece boundary (n > 4 tokens)


def test_two_launches_give_equal_bits_and_a_row_alone_equals_the_row_among_64():
    n, V, M = 7, 4, 64
    rng = np.random.RandomState(5)
    pieces = _pieces([30, 12, 50], V, seed=6)
    ix = _corpus(pieces, V).copy_index(n)
    rows, _ = _rows(pieces, n, 20, M, 40, V, rng)
    a, b = launch(ix, [V] * 4, rows, 20), launch(ix, [V] * 4, rows, 20)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    check(a, pieces, n, [V] * 4, rows, 20)
    for r in (0, 7, 63):
        one = launch(ix, [V] * 4, rows[r:r + 1], 20)
        assert np.array_equal(one[0][0], a[0][r]) and np.array_equal(one[1][0], a[1][r])


# ---- forced tokens, static sets, exclusion, the relaxation ---------------------------------------------------------------------
def test_forced_copy_relaxed_with_and_without_exclude_and_the_set_in_place():
    n, V, M, col, width = 4, 6, 64, 21, 32
    vocab = [V, V - 1, V, V - 2]
    rng = np.random.RandomState(8)
    pieces = [np.minimum(p, np.array(vocab) - 1) for p in _pieces([25, 40, 9], V, seed=9)]
    from vqcpc_bach_amd.dataloaders.corpus import Corpus, DeviceCorpus
    tokens = np.concatenate(pieces, axis=0).astype(np.int32)
    start = np.concatenate([[0], np.cumsum([p.shape[0] for p in pieces])])
    zero = np.zeros(4, dtype=np.int64)
    ix = DeviceCorpus(Corpus(tokens, start, 1, vocab, zero, zero, zero), 'cuda').copy_index(n)
    rows, modes = _rows(pieces, n, col, M, width, V, rng)
    rows = np.minimum(rows, np.tile(np.array(vocab) - 1, width // 4)[None, :])
    bans = np.stack([N.banned(rows[b], col, n, pieces) for b in range(M)])
    assert bans.any(axis=1).sum() > 10
    # forced: the banned token where there is one (FORCED_COPY), an unbanned one elsewhere
    cons = np.full((M, width), -1, dtype=np.int64)
    for b in range(M):
        cons[b, col] = np.flatnonzero(bans[b])[0] if bans[b].any() and b % 2 == 0 else np.flatnonzero(~bans[b])[0]
    wr = check(launch(ix, vocab, rows, col, cons=cons), pieces, n, vocab, rows, col, cons=cons)
    assert (wr == N.FORCED_COPY).sum() > 3 and (wr == 0).sum() > 3 and set(np.unique(wr)) <= {0, N.FORCED_COPY}
    # a free column next to forced ones, static sets: all of them banned (RELAXED), a superset (narrowed), an empty one (whole vocabulary)
    cons[:, col] = -1
    static = rng.rand(M, width, 256) < 0.5
    static[:, :, vocab[col % 4]:] = rng.rand(M, width, 256 - vocab[col % 4]) < 0.1        # bits past the vocabulary are carried along
    for b in range(M):
        if b % 3 == 0 and bans[b].any():
            static[b, col, :V] = bans[b, :V]
        if b % 3 == 1:
            static[b, col, :V] = False
    for in_place in (False, True):
        wr = check(launch(ix, vocab, rows, col, cons=cons, static=static, in_place=in_place), pieces, n, vocab, rows, col, cons=cons,
                   static=static)
        assert (wr == N.RELAXED).sum() > 3 and ((wr > 0) & (wr < 256)).sum() > 3
    # exclusion: what the ban leaves is excluded -> RELAXED, where without the exclusion the set is narrowed
    exclude = np.zeros((4, 256), dtype=bool)
    exclude[col % 4, 1:V] = True                            # token 0 alone may be drawn: banned, nothing is left
    plain = check(launch(ix, vocab, rows, col), pieces, n, vocab, rows, col)
    wr = check(launch(ix, vocab, rows, col, exclude=exclude), pieces, n, vocab, rows, col, exclude=exclude)
    assert ((wr == N.RELAXED) & (plain != N.RELAXED)).sum() > 0


# ---- the live window, the chorale and the leading dimensions -------------------------------------------------------------------
def test_a_context_that_spans_the_window_start_and_reaches_chorale_column_zero():
    U, T, w0, V, M = 16, 48, 2, 3, 64
    rng = np.random.RandomState(11)
    pieces = _pieces([20, 30], V, seed=12)
    width = 5 * U
    for col, n in ((40, 40), (41, 40), (36, 9), (32, 4), (79, 64)):
        ix = _corpus(pieces, V).copy_index(n)
        rows, modes = _rows(pieces, n, col, M, width, V, rng)
        wr = check(launch(ix, [V] * 4, rows, col, T=T, U=U, w0=w0), pieces, n, [V] * 4, rows, col)
        assert bool((wr[modes == 0] > 0).all()) and (wr > 0).sum() >= 8
        if col == n:
            assert (wr[modes == 2] > 0).all() and (modes == 2).sum() > 0


def test_without_a_live_window_or_past_T_nothing_is_written_and_columns_past_a_leading_dimension_are_skipped():
    from vqcpc_bach_amd import hip
    n, V, M, U, T = 3, 3, 4, 16, 48
    pieces = _pieces([20], V, seed=13)
    ix = _corpus(pieces, V).copy_index(n)
    tokens = torch.zeros(M, T, dtype=torch.int64).cuda()
    chorale = torch.zeros(M, 5 * U, dtype=torch.int64).cuda()
    off = _offsets([V] * 4)

    def run(pos, win, ldsets, ldrep):
        sets = torch.full((M, 5 * U, 8), FILL, dtype=torch.int32).cuda()
        report = torch.full((M, 5 * U), FILL, dtype=torch.int32).cuda()
        hip.call('vqcpc_decode_nocopy', tokens, T, T, chorale, 5 * U, None, 0, *ix.args(), off, 4, None, None, 0, sets, ldsets, report,
                 ldrep, torch.tensor([pos], dtype=torch.int32).cuda(), torch.tensor(win, dtype=torch.int32).cuda(), U, M)
        torch.cuda.synchronize()
        return bool((sets == FILL).all()), bool((report == FILL).all())

    assert run(5, [0, -1], 5 * U, 5 * U) == (True, True)
    assert run(T, [1, 0], 5 * U, 5 * U) == (True, True) and run(-1, [1, 0], 5 * U, 5 * U) == (True, True)
    assert run(5, [1, 0], 5 * U, 5 * U) == (False, False)
    # the buffers are declared T wide, the live column is 2 U + 20 = 52: at and past both leading dimensions
    assert run(20, [3, 2], T, T) == (True, True)
    assert run(20, [3, 2], 5 * U, T) == (False, True)


# ---- the index: long key ranges, the duplicate removal, piece ranges -------------------------------------------------------------
@pytest.mark.parametrize('held_ticks,floor', [(100, 64), (2500, 256)])
def test_key_ranges_of_more_than_64_and_256_candidates(held_ticks, floor):
    """Without the duplicate removal a held chord's context has one entry per occurrence: every one of them is verified."""
    n, V, M = 5, 4, 3
    held = np.tile(np.array([[1, 2, 1, 3]]), (held_ticks, 1))
    held[held_ticks // 2, 0] = 0                            # two continuations of the soprano's held context
    pieces = [held] + _pieces([11], V, seed=14)
    ix = _corpus(pieces, V).copy_index(n, deduplicate=False)
    assert ix.entries == ix.entries_before == N.distinct_pairs(n, pieces)[1]
    keys = ix.keys.cpu().numpy()
    _, counts = np.unique(keys >> 8, return_counts=True)
    assert counts.max() > floor                             # whatever the hash is, one context holds that many candidates
    rows = np.tile(np.array([1, 2, 1, 3]), (M, 8))
    rows[1, 3] = 0
    for col in (28, 29, 31):
        wr = check(launch(ix, [V] * 4, rows, col), pieces, n, [V] * 4, rows, col)
        assert wr[0] == (2 if col == 28 else 1)


def test_a_very_common_context_keeps_one_entry_per_continuation():
    n, V = 6, 4
    rng = np.random.RandomState(15)
    held = np.tile(np.array([[1, 2, 1, 3]]), (3000, 1))
    held[rng.randint(0, 3000, size=40), rng.randint(0, 4, size=40)] = 0
    pieces = [held] + _pieces([25, 7], V, seed=16)
    dc = _corpus(pieces, V)
    ix, raw = dc.copy_index(n), dc.copy_index(n, deduplicate=False)
    distinct, total = N.distinct_pairs(n, pieces)
    print(f'held chord, 3000 ticks: {total} entries, {ix.entries} after the duplicate removal, {distinct} distinct (context, next)')
    assert raw.entries == total and ix.entries_before == total
    assert distinct <= ix.entries <= total and distinct < total // 4
    assert ix.entries < total                               # thousands of occurrences of one chord were dropped
    rows = np.tile(np.array([1, 2, 1, 3]), (2, 10))
    rows[1, 20] = 0
    for col in (24, 26, 39):
        a, b = launch(ix, [V] * 4, rows, col), launch(raw, [V] * 4, rows, col)
        check(a, pieces, n, [V] * 4, rows, col)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_piece_sub_ranges():
    n, V, M, col, width = 3, 3, 64, 13, 20
    rng = np.random.RandomState(17)
    pieces = _pieces([9, 14, 5, 21, 8], V, seed=18)
    dc = _corpus(pieces, V)
    differ = 0
    for lo, hi in ((0, 5), (1, 3), (4, 5), (2, 4)):
        ix = dc.copy_index(n, pieces=(lo, hi))
        assert ix.pieces == (lo, hi)
        rows, _ = _rows(pieces, n, col, M, width, V, rng)   # quotations of ALL pieces, also those outside the range
        wr = check(launch(ix, [V] * 4, rows, col), pieces[lo:hi], n, [V] * 4, rows, col)
        differ += int(not np.array_equal(wr, want(pieces, n, [V] * 4, rows, col)[1]))
    assert differ >= 2                                      # the range matters
    with pytest.raises(ValueError):
        dc.copy_index(n, pieces=(3, 3))


# ---- the audit -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('ticks', [1, 17, 400])
@pytest.mark.parametrize('n', [2, 9, 70])
def test_the_audit_equals_the_reference_on_whole_pieces(ticks, n):
    from vqcpc_bach_amd import hip
    V = 3
    rng = np.random.RandomState(ticks + n)
    pieces = _pieces([60, 33, 150], V, seed=19)
    ix = _corpus(pieces, V).copy_index(n)
    x = rng.randint(0, V, size=(3, ticks, 4)).astype(np.int64)
    if ticks > 40:
        x[0, 5:35], x[1, 100:220] = pieces[1][2:32], pieces[2][10:130]
        x[2, 300:390] = np.concatenate([pieces[0][30:], pieces[0]])        # the end of a piece, then all of it: no run across the seam
    elif ticks == 17:
        x[0, 3:15] = pieces[0][20:32]
    x[2, 0, 1] = -1                                         # no token: never flagged, never matched
    flat = torch.from_numpy(x.reshape(3, -1)).cuda()
    ld = ticks * 4 + 5
    report = torch.full((3, ld), FILL, dtype=torch.int32).cuda()
    hip.call('vqcpc_nocopy_audit', flat, ticks * 4, ticks * 4, *ix.args(), report, ld, 3)
    got = report.cpu().numpy()
    assert bool((got[:, ticks * 4:] == FILL).all())
    for b in range(3):
        assert np.array_equal(got[b, :ticks * 4], N.audit(x[b].reshape(-1), n, pieces)), b
    if ticks > 40:
        assert (got[:, :ticks * 4] == N.FORCED_COPY).sum() > 50


# ---- the refusals ------------------------------------------------------------------------------------------------------------
def test_the_host_entries_refuse_bad_arguments_before_any_launch():
    from vqcpc_bach_amd import hip
    n, V, M, T = 3, 3, 4, 16
    dc = _corpus(_pieces([20], V, seed=21), V)
    ix = dc.copy_index(n)
    tokens = torch.zeros(64, T, dtype=torch.int64).cuda()
    sets = torch.zeros(64, T, 8, dtype=torch.int32).cuda()
    report = torch.zeros(64, T, dtype=torch.int32).cuda()
    pos = torch.zeros(1, dtype=torch.int32).cuda()
    off = _offsets([V] * 4)

    def call(tokens=tokens, ldtok=T, cons=None, ldcons=0, index=ix.args(), off=off, nc=4, stat=None, ldstat=0, sets=sets, ldsets=T,
             report=report, ldrep=T, pos=pos, M=M, chorale=None, win=None):
        hip.call('vqcpc_decode_nocopy', tokens, ldtok, T, chorale, 0, cons, ldcons, *index, off, nc, None, stat, ldstat, sets, ldsets,
                 report, ldrep, pos, win, 1, M)

    call()
    k, w, e, f, nf, mc = ix.args()
    bad = [dict(tokens=None), dict(sets=None), dict(pos=None), dict(off=None), dict(M=0), dict(M=65), dict(nc=3), dict(nc=5),
           dict(off=_offsets([V, 257, V, V])), dict(off=_offsets([V, 0, V, V])), dict(ldtok=T - 1), dict(ldsets=T - 1),
           dict(ldrep=T - 1), dict(stat=sets, ldstat=T - 1), dict(cons=tokens, ldcons=T - 1), dict(index=(k, w, e, None, nf, mc)),
           dict(index=(None, w, e, f, nf, mc)), dict(index=(k, w, e, f, nf, 0)), dict(index=(k, w, e, f, nf, 513)),
           dict(index=(k, w, e, f, 0, mc)), dict(win=pos)]
    for kw in bad:
        with pytest.raises(hip.VqcpcHipError):
            call(**kw)
    with pytest.raises(hip.VqcpcHipError):
        hip.call('vqcpc_nocopy_audit', tokens, T, T, *ix.args(), report, T - 1, 4)
    with pytest.raises(hip.VqcpcHipError):
        hip.call('vqcpc_nocopy_audit', tokens, T, T - 1, *ix.args(), report, T, 4)
    with pytest.raises(hip.VqcpcHipError):
        hip.call('vqcpc_copy_index_keys', f, nf, 513, k)
    assert hip.clear_runtime_error() == 0
    for mc in (0, 513):
        with pytest.raises(ValueError, match='max_copy'):
            dc.copy_index(mc)
    with pytest.raises(ValueError, match='vocab'):
        _corpus(_pieces([20], 257, seed=22), 257).copy_index(3)
    # an index without any entry (every piece is shorter than the context) bans nothing
    empty = dc.copy_index(100)
    assert empty.entries == 0
    rows = np.zeros((2, 120), dtype=np.int64)
    got = launch(empty, [V] * 4, rows, 110)
    assert (got[1][:, 110] == 0).all()
