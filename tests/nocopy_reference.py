"""The reference of the copy guard (include/vqcpc.h, "Copy guard"; vqcpc_bach_amd/csrc/nocopy.hip): the banned set, the report and
the audit by brute force over the pieces -- every stretch of n + 1 tokens of every piece is compared with the history, no hashing, no
index, no framing.  Shares no code with the package.  tests/test_nocopy_reference_cpu.py pins it on tests/duplicates_reference.py
and difflib.

Conventions: a row is a 1-D array of tokens flattened tick-major, voice-minor (column c: tick c // 4, voice c % 4); `pieces` is a
list of (ticks, 4) arrays; sets are bool (256,)."""
import numpy as np

RELAXED, FORCED_COPY = 1 << 16, 1 << 17
NC = 4


def banned(history, col, n, pieces):
    """bool (256,): token k is banned at column `col` given history[0 .. col): some piece position j of voice col % 4 holds k and
    the n tokens before j, all inside the piece, equal history[col - n .. col)."""
    ban = np.zeros(256, dtype=bool)
    if col < n:
        return ban
    ctx = np.asarray(history[col - n:col]).astype(np.int64)
    if (ctx < 0).any():
        return ban
    for piece in pieces:
        flat = np.asarray(piece).astype(np.int64).reshape(-1)
        if flat.size <= n:
            continue
        windows = np.lib.stride_tricks.sliding_window_view(flat, n + 1)        # windows[i] = flat[i .. i + n]; j = i + n
        j = np.arange(windows.shape[0]) + n
        hit = (j % NC == col % NC) & (windows[:, :n] == ctx[None, :]).all(axis=1)
        ban[windows[hit, n]] = True
    return ban


def position(tokens, col, n, pieces, vocab, constraint=None, static=None, exclude=None):
    """(set bool (256,), report): what vqcpc_decode_nocopy writes at column `col` of one row.  tokens: the row (only [0, col) is
    read); constraint: the row's forced tokens or None; static: the column's incoming set bool (256,) or None; exclude: the voice's
    excluded tokens bool (256,) or None."""
    V = int(vocab[col % NC])
    inside = np.arange(256) < V
    s = inside.copy() if static is None else np.asarray(static, dtype=bool).copy()
    if not (s & inside).any():
        s = inside.copy()
    ban = banned(tokens, col, n, pieces)
    forced = -1 if constraint is None else int(constraint[col])
    if forced >= 0:
        return s, FORCED_COPY if forced < 256 and ban[forced] else 0
    removed = int((s & ban).sum())
    left = s & ~ban & inside
    if exclude is not None:
        left = left & ~np.asarray(exclude, dtype=bool)
    if removed and not left.any():
        return s, RELAXED
    return s & ~ban, removed


def row_report(tokens, n, pieces, vocab, constraint=None, static=None, exclude=None, first=0):
    """(sets (width, 256), report (width,)) of a whole row, -1 / empty before column `first`.  static: (width, 256) or None;
    exclude: (4, 256) or None."""
    width = len(tokens)
    sets, report = np.zeros((width, 256), dtype=bool), np.full(width, -1, dtype=np.int32)
    for col in range(first, width):
        sets[col], report[col] = position(tokens, col, n, pieces, vocab, constraint, None if static is None else static[col],
                                          None if exclude is None else exclude[col % NC])
    return sets, report


def audit(tokens, n, pieces):
    """int32 (width,): FORCED_COPY where token c completes a shared run of n + 1 tokens, else 0."""
    tokens = np.asarray(tokens)
    out = np.zeros(len(tokens), dtype=np.int32)
    for col in range(n, len(tokens)):
        t = int(tokens[col])
        if 0 <= t < 256 and banned(tokens, col, n, pieces)[t]:
            out[col] = FORCED_COPY
    return out


def distinct_pairs(n, pieces):
    """(distinct (voice, context, next) triples, all entries): the bounds of the index's size after and before the duplicate
    removal."""
    seen, total = set(), 0
    for piece in pieces:
        flat = np.asarray(piece).astype(np.int64).reshape(-1)
        for j in range(n, flat.size):
            seen.add((j % NC, flat[j - n:j + 1].tobytes()))
            total += 1
    return len(seen), total


def pack(sets):
    """bool (..., 256) -> int32 (..., 8): bit i & 31 of word i >> 5."""
    bits = np.asarray(sets, dtype=bool).reshape(sets.shape[:-1] + (8, 32)).astype(np.uint64)
    words = (bits << np.arange(32, dtype=np.uint64)).sum(axis=-1).astype(np.uint32)
    return words.view(np.int32)


def unpack(words):
    """int32 (..., 8) -> bool (..., 256)."""
    w = np.asarray(words).view(np.uint32)
    return ((w[..., :, None] >> np.arange(32, dtype=np.uint32)) & 1).astype(bool).reshape(w.shape[:-1] + (256,))
