"""The reference of the duplicate check (vqcpc_bach_amd/dataloaders/corpus.py, csrc/duplicates.hip): the standard library's
difflib on lists of (voice, token) pairs, per piece, combined by (longest, smallest query position, earliest piece); and a
brute-force O(n m) numpy table that pins difflib's tie rule.  Shares no code with the package."""
import difflib

import numpy as np

NO_MATCH = (0, -1, -1, -1)


def pairs(x):
    """(ticks, 4) tokens -> the flattened list of (voice, token), tick-major, voice-minor."""
    x = np.asarray(x)
    return [(v, int(x[t, v])) for t in range(x.shape[0]) for v in range(x.shape[1])]


def longest_run(query, pieces, lo=0, hi=None):
    """(length, i, piece, k): the longest common run of `query` (ticks, 4) with the pieces [lo, hi) of the list `pieces`; i is the
    query position 4 tick + voice, k the position inside the piece.  No common token: NO_MATCH."""
    a = pairs(query)
    best = NO_MATCH
    for p in range(lo, len(pieces) if hi is None else hi):
        b = pairs(pieces[p])
        m = difflib.SequenceMatcher(None, a, b, autojunk=False).find_longest_match(0, len(a), 0, len(b))
        if m.size and (m.size > best[0] or (m.size == best[0] and m.a < best[1])):       # an equal (size, a) keeps the earlier piece
            best = (m.size, m.a, p, m.b)
    return best


def brute_force(query, piece):
    """(length, i, k) by the full table of common-suffix lengths: longest, then smallest i, then smallest k."""
    a, b = pairs(query), pairs(piece)
    table = np.zeros((len(a) + 1, len(b) + 1), dtype=np.int64)
    for i in range(len(a)):
        for k in range(len(b)):
            if a[i] == b[k]:
                table[i + 1, k + 1] = table[i, k] + 1
    length = int(table.max())
    if length == 0:
        return 0, -1, -1
    ends = np.argwhere(table == length)                  # (i + 1, k + 1) of the last token of every longest run
    starts = sorted((int(e[0]) - length, int(e[1]) - length) for e in ends)
    return (length,) + starts[0]


def as_dict(result):
    """(length, i, piece, k) -> the dict DeviceCorpus.longest_common_run returns for one row."""
    length, i, piece, k = result
    if length == 0:
        return dict(length=0, query_tick=-1, query_voice=-1, piece=-1, piece_tick=-1, voice=-1)
    return dict(length=length, query_tick=i // 4, query_voice=i % 4, piece=piece, piece_tick=k // 4, voice=k % 4)


def random_pieces(ticks, vocab, seed):
    rng = np.random.RandomState(seed)
    return [rng.randint(0, vocab, size=(n, 4)).astype(np.int64) for n in ticks]
