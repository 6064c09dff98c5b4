"""Pins the copy guard's reference (tests/nocopy_reference.py) on the duplicate check's (tests/duplicates_reference.py, difflib):
  (1) on random sequences over 2-4 tokens per voice, k is banned at c exactly when placing k makes the run that ends at c at
      least n + 1 long;
  (2) a sequence built by always taking the lowest unbanned token has a longest run <= n;
  (3) the audit flags a position exactly when the run ending there is longer than n, and any position exactly when the longest
      run is."""
import difflib

import numpy as np
import pytest

import duplicates_reference as D
import nocopy_reference as N

CASES = [(2, 1, 11), (2, 3, 12), (3, 2, 13), (4, 5, 14), (3, 8, 15)]          # (tokens per voice, n, seed)


def _pieces(vocab, seed):
    return D.random_pieces([9, 1, 17, 6], vocab, seed)


def _run_ending_at(flat, c, pieces):
    """The length of the longest common run that ENDS at query position c, by difflib on (voice, token) pairs: the longest match
    of a[c - L + 1 .. c] that reaches c, for growing L."""
    a = D.pairs(np.asarray(flat).reshape(-1, 4))
    best = 0
    for piece in pieces:
        b = D.pairs(piece)
        sm = difflib.SequenceMatcher(None, a, b, autojunk=False)
        L = 1
        while L <= c + 1 and sm.find_longest_match(c - L + 1, c + 1, 0, len(b)).size == L:
            best = max(best, L)
            L += 1
    return best


@pytest.mark.parametrize('vocab,n,seed', CASES)
def test_banned_exactly_when_the_run_would_reach_n_plus_one(vocab, n, seed):
    pieces = _pieces(vocab, seed)
    query = D.random_pieces([12], vocab, seed + 100)[0].reshape(-1)
    query[8:28] = pieces[2].reshape(-1)[12:32]              # a quotation of 20 tokens, so that also a long context has matches
    seen = 0
    for c in range(len(query)):
        ban = N.banned(query, c, n, pieces)
        assert not ban[vocab:].any()
        for k in range(vocab):
            placed = query.copy()
            placed[c] = k
            want = _run_ending_at(placed, c, pieces) >= n + 1
            assert bool(ban[k]) == want, (c, k)
            seen += int(want)
    assert seen > 0                                         # the case has bans to get right


@pytest.mark.parametrize('vocab,n,seed', CASES)
def test_the_lowest_unbanned_token_never_copies_more_than_n(vocab, n, seed):
    pieces = _pieces(vocab, seed)
    row = np.zeros(4 * 16, dtype=np.int64)
    relaxed = []
    for c in range(len(row)):
        s, rep = N.position(row, c, n, pieces, [vocab] * 4)
        assert s[:vocab].any() and not s[vocab:].any()      # never an empty set
        relaxed.append(rep == N.RELAXED)
        row[c] = int(np.flatnonzero(s)[0])
    for c in range(len(row)):                               # position by position: an unflagged one ends no run longer than n
        assert relaxed[c] or _run_ending_at(row, c, pieces) <= n, c
    if not any(relaxed):                                    # the guarantee as the issue states it
        assert D.longest_run(row.reshape(-1, 4), pieces)[0] <= n


@pytest.mark.parametrize('vocab,n,seed', CASES)
def test_the_audit_flags_the_positions_that_complete_a_run_longer_than_n(vocab, n, seed):
    pieces = _pieces(vocab, seed)
    query = D.random_pieces([14], vocab, seed + 200)[0]
    query[3:9] = pieces[2][5:11]                            # a quotation of 24 tokens
    flat = query.reshape(-1)
    got = N.audit(flat, n, pieces)
    want = np.array([N.FORCED_COPY if _run_ending_at(flat, c, pieces) > n else 0 for c in range(len(flat))], dtype=np.int32)
    assert np.array_equal(got, want)
    assert bool(got.any()) == (D.longest_run(query, pieces)[0] > n)
    assert got.any()


def test_pack_and_unpack_are_inverse():
    rng = np.random.RandomState(3)
    sets = rng.rand(5, 7, 256) < 0.3
    words = N.pack(sets)
    assert words.shape == (5, 7, 8) and words.dtype == np.int32
    assert np.array_equal(N.unpack(words), sets)
    assert N.pack(np.arange(256)[None, :] == 33)[0].tolist() == [0, 2, 0, 0, 0, 0, 0, 0]
