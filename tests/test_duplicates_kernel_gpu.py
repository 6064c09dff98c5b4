"""vqcpc_dup_frame, vqcpc_dup_pack and vqcpc_dup_longest_run (csrc/duplicates.hip) called directly on tables this file builds
itself, against the difflib reference of tests/duplicates_reference.py: exact integer equality, no tolerance."""
import functools

import numpy as np
import pytest
import torch

import duplicates_reference as R

pytestmark = pytest.mark.gpu

GUARD = 0x5A5A5A5A5A5A5A5A
THREADS = 256                      # diagonals per block of dup_longest_run_kernel; a wave has 64


def _call(name, *args):
    from vqcpc_bach_amd import hip
    hip.load()
    hip.call(name, *args)


def _u64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).cuda()


def _piece_start(pieces):
    return np.concatenate([[0], np.cumsum([p.shape[0] for p in pieces])]).astype(np.int64)


def _frame(pieces):
    """The framed corpus from vqcpc_dup_frame, checked against its host twin; two guard words behind it stay untouched."""
    from vqcpc_bach_amd.dataloaders import corpus as C
    ps = _piece_start(pieces)
    tokens = np.concatenate(pieces)
    n_framed = tokens.shape[0] + len(pieces) + 1
    framed = torch.full((n_framed + 2,), GUARD, dtype=torch.int64, device='cuda')
    _call('vqcpc_dup_frame', torch.from_numpy(tokens.astype(np.int32)).cuda(), torch.from_numpy(ps).cuda(), len(pieces),
          tokens.shape[0], framed)
    got = framed.cpu().numpy().view(np.uint64)
    assert np.array_equal(got[:n_framed], C.frame_words(tokens, ps)), 'framed corpus'
    assert (got[n_framed:] == np.uint64(GUARD)).all(), 'guard words after the framed array'
    return framed, ps


def _keys(framed, first, count, queries, pad=3):
    """Raw keys of the rows of `queries` (G, n, 4) against framed[first : first + count]; the query rows are `pad` words apart
    more than they need (the filler packs token 0 of every voice and must not be read), guard words behind `out`."""
    from vqcpc_bach_amd.dataloaders import corpus as C
    G, n = queries.shape[:2]
    words = np.zeros((G, n + pad), dtype=np.uint64)
    words[:, :n] = C.pack_words(queries)
    out = torch.zeros(G + 2, dtype=torch.int64, device='cuda')
    out[G:] = GUARD
    _call('vqcpc_dup_longest_run', framed[first:], count, _u64(words), n + pad, n, G, out)
    got = out.cpu().numpy().view(np.uint64)
    assert (got[G:] == np.uint64(GUARD)).all(), 'guard words after out'
    return [int(k) for k in got[:G]]


def _run(pieces, queries, lo=0, hi=None, **kw):
    """[(length, i, piece, k)] per row, as tests/duplicates_reference.py states a result."""
    from vqcpc_bach_amd.dataloaders import corpus as C
    framed, ps = _frame(pieces)
    first, count = C.framed_range(ps, lo, len(pieces) if hi is None else hi)
    res = []
    for key in _keys(framed, first, count, np.asarray(queries), **kw):
        length, i, j = C.unpack_key(key)
        if not length:
            res.append(R.NO_MATCH)
            continue
        piece, tick, voice = C.unframe(j, ps, first)
        res.append((length, i, piece, 4 * tick + voice))
    return res


# ---- random corpora: long chance runs and ties ---------------------------------------------------------------------------------
TICKS = (4, 8, 52, 8, 4, 52)


@functools.lru_cache(maxsize=None)
def _random_case(vocab, n, ticks=TICKS):
    """(pieces, queries (3, n, 4), reference results): row 1 carries a copy of a corpus stretch, so the rows differ."""
    pieces = R.random_pieces(ticks, vocab, seed=vocab + n)
    rng = np.random.RandomState(7 * vocab + n)
    queries = rng.randint(0, vocab, size=(3, n, 4)).astype(np.int64)
    src = pieces[-1]
    m = min(n, src.shape[0]) // 2
    if m:
        queries[1, n - m:] = src[1:1 + m]
    want = tuple(R.longest_run(q, pieces) for q in queries)
    return pieces, queries, want


@pytest.mark.parametrize('n', [1, 5, 64, 96])
@pytest.mark.parametrize('vocab', [3, 60])
def test_random_corpora(vocab, n):
    pieces, queries, want = _random_case(vocab, n)
    assert _run(pieces, queries) == list(want)
    assert _run(pieces, queries[:1]) == list(want[:1]), 'G = 1'
    if n >= 64:
        assert len(set(want)) > 1, 'the rows have different answers'


@pytest.mark.parametrize('vocab', [3, 60])
def test_query_longer_than_the_whole_corpus(vocab):
    pieces, queries, want = _random_case(vocab, 64, ticks=(4, 8))
    assert _run(pieces, queries) == list(want)


@pytest.mark.parametrize('n', [257, 300, 600])
def test_random_corpus_and_a_query_of_more_than_one_pass(n):
    """The kernel stages the query in passes of 256 ticks: 257 (a last pass of one tick), 300 and 600 ticks (three passes).  Vocab 3;
    row 1 ends with a 100-tick copy of a corpus stretch, which crosses a pass boundary."""
    pieces, queries, want = _random_case(3, n, ticks=(8, 52, 200))
    assert _run(pieces, queries) == list(want)
    assert want[1][0] >= 400


def test_pieces_sub_range():
    pieces, queries, _ = _random_case(3, 64)
    for lo, hi in ((1, 3), (2, 3), (3, 6), (5, 6)):
        assert _run(pieces, queries, lo, hi) == [R.longest_run(q, pieces, lo, hi) for q in queries], (lo, hi)


def test_two_calls_give_identical_keys():
    from vqcpc_bach_amd.dataloaders import corpus as C
    pieces, queries, _ = _random_case(3, 96)
    framed, ps = _frame(pieces)
    first, count = C.framed_range(ps, 0, len(pieces))
    a, b = _keys(framed, first, count, queries), _keys(framed, first, count, queries)
    assert a == b and all(a)


# ---- planted runs ----------------------------------------------------------------------------------------------------------------
# corpus tokens are < 48, the filler of a query is >= 50: the only common tokens are the planted ones (48 and 49 are free for tokens
# that must occur once in the corpus)
N_TICKS = 96


@functools.lru_cache(maxsize=None)
def _corpus():
    pieces = R.random_pieces((52,) * 8, 48, seed=11)
    for p in pieces:
        p.setflags(write=False)
    return pieces


def _filler(n=N_TICKS, seed=0):
    return np.random.RandomState(seed).randint(50, 60, size=(n, 4)).astype(np.int64)


def _plant(query, i, piece, k, length):
    """Copies `length` tokens of `piece` from flattened position k to flattened position i of the query (same voice)."""
    assert i % 4 == k % 4
    query.reshape(-1)[i:i + length] = np.asarray(piece).reshape(-1)[k:k + length]


def _check(query, expected, pieces=None):
    pieces = _corpus() if pieces is None else pieces
    assert R.longest_run(query, pieces) == expected, 'the reference disagrees with the plan of the test'
    assert _run(pieces, query[None]) == [expected]


@pytest.mark.parametrize('voice,length', [(1, 6), (2, 5), (3, 2), (1, 11), (3, 9), (0, 3), (1, 1), (1, 2), (2, 1)])
def test_runs_that_start_and_end_inside_a_tick(voice, length):
    """Starts at voice 1, 2 and 3, ends mid-tick; the last three are 1 or 2 tokens strictly inside one tick, the only match."""
    q = _filler()
    i, k = 4 * 40 + voice, 4 * 17 + voice
    pieces = [p.copy() for p in _corpus()]
    pieces[3].reshape(-1)[k:k + 2] = [48, 49]          # a short run is the only one of its tokens
    _plant(q, i, pieces[3], k, length)
    _check(q, (length, i, 3, k), pieces=pieces)


def test_first_and_last_diagonal():
    """The query's last tick on the corpus's first tick and its first tick on the corpus's last: the outermost diagonals that
    hold a stored tick."""
    pieces = _corpus()
    q = _filler()
    _plant(q, 4 * (N_TICKS - 1), pieces[0], 0, 4)
    _check(q, (4, 4 * (N_TICKS - 1), 0, 0))
    q = _filler()
    _plant(q, 0, pieces[-1], 4 * 51, 4)
    _check(q, (4, 0, len(pieces) - 1, 4 * 51))
    q = _filler()
    _plant(q, 4 * (N_TICKS - 1) + 1, pieces[0], 1, 3)                       # both at once: equal lengths, the smaller i wins
    _plant(q, 1, pieces[-1], 4 * 51 + 1, 3)
    _check(q, (3, 1, len(pieces) - 1, 4 * 51 + 1))


def _on_diagonal(diagonal, query_tick):
    """(piece, tick of the piece) of the stored corpus tick that diagonal `diagonal` pairs with `query_tick`."""
    from vqcpc_bach_amd.dataloaders import corpus as C
    ps = _piece_start(_corpus())
    f = query_tick + diagonal - (N_TICKS - 1)
    piece, tick, _ = C.unframe(4 * f, ps, 0)
    return piece, tick


@pytest.mark.parametrize('boundary', [64, 128, THREADS, THREADS + 64])
def test_runs_on_both_sides_of_a_wave_and_a_chunk_boundary(boundary):
    """Diagonals boundary - 1 and boundary belong to two waves, or to two blocks: a run on either is found, and of two equal
    runs, one on each, the smaller i, then the smaller j wins whichever side holds it."""
    pieces = _corpus()
    for d in (boundary - 1, boundary):
        q = _filler()
        p, t = _on_diagonal(d, 80)
        _plant(q, 4 * 80 + 2, pieces[p], 4 * t + 2, 7)
        _check(q, (7, 4 * 80 + 2, p, 4 * t + 2))
    for d_first, d_second in ((boundary - 1, boundary), (boundary, boundary - 1)):
        q = _filler()
        (p1, t1), (p2, t2) = _on_diagonal(d_first, 70), _on_diagonal(d_second, 90)
        _plant(q, 4 * 70 + 1, pieces[p1], 4 * t1 + 1, 6)
        _plant(q, 4 * 90 + 1, pieces[p2], 4 * t2 + 1, 6)
        _check(q, (6, 4 * 70 + 1, p1, 4 * t1 + 1))
    # the same query stretch on both diagonals (the corpus holds it twice): equal length and i, the smaller j wins
    (p1, t1), (p2, t2) = _on_diagonal(boundary - 1, 80), _on_diagonal(boundary, 80)
    assert (p1, t1 + 1) == (p2, t2), 'both diagonals must fall inside one piece for this case'
    twice = [p.copy() for p in pieces]
    twice[p1][t1:t1 + 2] = [[1, 2, 3, 4], [1, 2, 3, 4]]
    q = _filler()
    q[80] = [1, 2, 3, 4]
    _check(q, (4, 320, p1, 4 * t1), pieces=twice)


PASS = 256                         # query ticks staged per pass of dup_longest_run_kernel


@pytest.mark.parametrize('n', [257, 300, 600])
def test_planted_runs_in_a_query_of_more_than_one_pass(n):
    """Four rows, one launch: (a) a run that begins mid-tick in the first pass and ends mid-tick in the second, (b) a run wholly in
    the last pass, (c) a run that ends with the last query tick of a last pass shorter than 256, (d) two equal runs, one per
    pass: the smaller i wins."""
    pieces = [p.copy() for p in _corpus()]
    pieces[5].reshape(-1)[4 * 20 + 1:4 * 20 + 3] = [48, 49]                 # (b) may have 2 tokens only: they occur once
    q = np.stack([_filler(n, seed=s) for s in range(4)])
    a = (14, 4 * (PASS - 3) + 1, 2, 4 * 10 + 1)                             # voice 1 of tick 253 to voice 2 of tick 256
    b_tick = max(PASS, n - 20)
    b = (min(14, 4 * (n - b_tick) - 2), 4 * b_tick + 1, 5, 4 * 20 + 1)
    c = (10, 4 * n - 10, 6, 4 * 30 + 2)
    d = (3, 4 * 100 + 1, 1, 4 * 5 + 1)
    for row, (length, i, piece, k) in enumerate((a, b, c, d)):
        _plant(q[row], i, pieces[piece], k, length)
    _plant(q[3], 4 * PASS + 1, pieces[4], 4 * 7 + 1, 3)                     # (d): the same length in the second pass
    assert a[1] + a[0] == 4 * PASS + 3 and b[1] >= 4 * PASS and c[1] + c[0] == 4 * n and n % PASS
    assert [R.longest_run(r, pieces) for r in q] == [a, b, c, d], 'the reference disagrees with the plan of the test'
    assert _run(pieces, q) == [a, b, c, d]
    q[3].reshape(-1)[4 * PASS] = pieces[4].reshape(-1)[4 * 7]               # (d) with the later run one token longer: it wins
    longer = (4, 4 * PASS, 4, 4 * 7)
    assert R.longest_run(q[3], pieces) == longer
    assert _run(pieces, q[3:]) == [longer]


def test_a_run_stops_at_the_piece_boundary():
    pieces = _corpus()
    q = _filler()
    q[8:11] = pieces[2][-3:]
    q[11:13] = pieces[3][:2]                                                # the query continues as the corpus does
    _check(q, (12, 32, 2, 4 * 49))
    q = _filler()
    q[8:10] = pieces[2][-2:]
    q[10:13] = pieces[3][:3]
    _check(q, (12, 40, 3, 0))


def test_equal_runs_smallest_query_position_then_smallest_corpus_position():
    pieces = [p.copy() for p in _corpus()]
    pieces[6][10:14] = pieces[1][30:34]                                     # the corpus holds one stretch twice
    q = _filler()
    _plant(q, 4 * 70 + 3, pieces[5], 4 * 5 + 3, 9)
    _plant(q, 4 * 20 + 3, pieces[6], 4 * 11 + 3, 9)                         # the same length earlier in the query, twice in the corpus
    _check(q, (9, 4 * 20 + 3, 1, 4 * 31 + 3), pieces=pieces)


def test_no_common_token():
    assert _run(_corpus(), np.stack([_filler(seed=1), _filler(seed=2)])) == [R.NO_MATCH, R.NO_MATCH]
    assert _run(_corpus(), _filler(n=1)[None]) == [R.NO_MATCH]


def test_pack_kernel_equals_its_host_twin():
    from vqcpc_bach_amd.dataloaders import corpus as C
    rng = np.random.RandomState(3)
    x = torch.from_numpy(rng.randint(0, 0xFFFF, size=(3, 7, 2, 4)).astype(np.int64)).cuda()
    view = x[:, :5, 1]                                                      # (3, 5, 4): rows 56 and ticks 8 words apart
    words = torch.full((3, 6), GUARD, dtype=torch.int64, device='cuda')
    _call('vqcpc_dup_pack', view, view.stride(0), view.stride(1), 5, 3, words, 6)
    got = words.cpu().numpy().view(np.uint64)
    assert np.array_equal(got[:, :5], C.pack_words(view.cpu().numpy())) and (got[:, 5] == np.uint64(GUARD)).all()


def test_refusals():
    from vqcpc_bach_amd import hip
    framed, ps = _frame(list(_corpus()[:1]))
    words = torch.zeros(8, dtype=torch.int64, device='cuda')
    out = torch.zeros(1, dtype=torch.int64, device='cuda')
    for n_ticks in (0, 16384):                                              # 4 * 16384 > 65535
        with pytest.raises(hip.VqcpcHipError, match='dup_longest_run'):
            _call('vqcpc_dup_longest_run', framed, 54, words, max(n_ticks, 8), n_ticks, 1, out)
    with pytest.raises(hip.VqcpcHipError, match='dup_longest_run'):
        _call('vqcpc_dup_longest_run', framed, 54, words, 8, 8, 0, out)
    assert int(out.item()) == 0
