"""The duplicate check without a GPU: the difflib reference (tests/duplicates_reference.py) against a brute-force table, tie
rule included, and the framing / unframing index arithmetic of vqcpc_bach_amd/dataloaders/corpus.py against that reference."""
import numpy as np
import pytest

import duplicates_reference as R


@pytest.mark.parametrize('seed', range(12))
def test_difflib_reference_equals_the_brute_force_table(seed):
    """Vocab 3: chance runs are long and ties abound, so the tie rule (smallest i, then smallest k) is exercised."""
    rng = np.random.RandomState(seed)
    query = rng.randint(0, 3, size=(int(rng.randint(1, 9)), 4))
    piece = rng.randint(0, 3, size=(int(rng.randint(1, 13)), 4))
    length, i, _, k = R.longest_run(query, [piece])
    assert (length, i, k) == R.brute_force(query, piece)
    assert length >= 1 and i % 4 == k % 4, 'a run pairs tokens of the same voice'


def test_reference_ties_and_piece_order():
    a = np.array([[0, 1, 2, 3], [4, 5, 6, 7]])
    far = np.array([[9, 9, 9, 9], [4, 5, 6, 7]])
    near = np.array([[0, 1, 2, 3], [9, 9, 9, 9]])
    assert R.longest_run(a, [far, near]) == (4, 0, 1, 0), 'equal lengths: the smallest query position wins over the earlier piece'
    assert R.longest_run(a, [far, far]) == (4, 4, 0, 4), 'equal length and query position: the earliest piece'
    assert R.longest_run(a, [far, near], lo=0, hi=1) == (4, 4, 0, 4)
    assert R.longest_run(a, [np.full((3, 4), 8)]) == R.NO_MATCH
    assert R.longest_run(np.array([[1, 2, 3, 4]]), [np.array([[2, 1, 4, 3]])]) == R.NO_MATCH, 'voices are never crossed'
    both = np.concatenate([a, a])
    assert R.longest_run(both, [a, a])[0] == 8, 'a run never crosses a piece boundary'
    assert R.as_dict((5, 6, 2, 10)) == dict(length=5, query_tick=1, query_voice=2, piece=2, piece_tick=2, voice=2)
    assert R.as_dict(R.NO_MATCH)['piece'] == -1


def _scan_framed(query_words, framed):
    """The longest run by a plain scan of every diagonal of the framed word array, token by token: (length, i, j) with the tie
    rule, j the token position inside `framed`."""
    n, N = len(query_words), len(framed)
    q = np.array([[(int(w) >> (16 * v)) & 0xFFFF for v in range(4)] for w in query_words]).reshape(-1)
    c = np.array([[(int(w) >> (16 * v)) & 0xFFFF for v in range(4)] for w in framed]).reshape(-1)
    best = (0, -1, -1)
    for delta in range(-(n - 1), N):
        run = 0
        for i in range(4 * n):
            j = i + 4 * delta
            run = run + 1 if 0 <= j < 4 * N and q[i] == c[j] else 0
            cand = (run, i - run + 1, j - run + 1)
            if run and (cand[0], -cand[1], -cand[2]) > (best[0], -best[1], -best[2]):
                best = cand
    return best


@pytest.mark.parametrize('seed', range(6))
def test_framing_and_unframing_against_the_reference(seed):
    from vqcpc_bach_amd.dataloaders import corpus as C
    rng = np.random.RandomState(100 + seed)
    ticks = [int(t) for t in rng.choice([4, 8, 12], size=4)]
    pieces = R.random_pieces(ticks, 3, seed)
    piece_start = np.concatenate([[0], np.cumsum(ticks)]).astype(np.int64)
    tokens = np.concatenate(pieces)
    framed = C.frame_words(tokens, piece_start)
    fs = C.framed_start(piece_start)
    assert len(framed) == tokens.shape[0] + len(pieces) + 1 == fs[-1] + 1
    assert (framed[fs] == np.uint64(0xFFFFFFFFFFFFFFFF)).all() and (np.delete(framed, fs) == C.pack_words(tokens)).all()
    query = rng.randint(0, 3, size=(int(rng.randint(1, 7)), 4))
    for lo, hi in ((0, 4), (1, 3), (3, 4), (0, 1)):
        first, count = C.framed_range(piece_start, lo, hi)
        assert (first, first + count - 1) == (fs[lo], fs[hi])
        length, i, j = _scan_framed(C.pack_words(query), framed[first:first + count])
        want = R.longest_run(query, pieces, lo, hi)
        got = R.NO_MATCH
        if length:
            piece, tick, voice = C.unframe(j, piece_start, first)
            got = (length, i, piece, 4 * tick + voice)
        assert got == want, (lo, hi)
        if length:
            assert voice == i % 4
            key = (length << 48) | ((0xFFFF - i) << 32) | (0xFFFFFFFF - j)
            assert C.unpack_key(key) == (length, i, j)
    assert C.unpack_key(0) == (0, -1, -1)
    for bad in ((2, 2), (3, 5), (-1, 2)):
        with pytest.raises(ValueError):
            C.framed_range(piece_start, *bad)


def test_window_at_follows_the_window_rule():
    from corpus_reference import extract_with_padding, specials
    from vqcpc_bach_amd.dataloaders.corpus import Corpus
    vocab = [9, 9, 9, 9]
    start, end, pad = specials(vocab)
    pieces = R.random_pieces([8, 4], 6, 3)
    c = Corpus(np.concatenate(pieces).astype(np.int16), [0, 8, 12], 4, vocab, start, end, pad)
    for piece, s, n in ((0, -3, 6), (0, 5, 7), (1, -1, 8), (1, 1, 2), (0, -1, 2)):
        assert np.array_equal(c.window_at(piece, s, n), extract_with_padding(pieces[piece], s, s + n, start, end, pad)), (piece, s, n)
    assert np.array_equal(c.window_at(0, 9, 3), np.tile(pad, (3, 1))) and np.array_equal(c.window_at(1, -6, 2), np.tile(pad, (2, 1)))
