"""Numpy restatement of the reference's window dataset (VQCPCB/datasets/chorale_dataset.py:124-129, the loop over the start
offsets, and :418-470, _extract_score_tensor_with_padding) without music21, tick-major: it MATERIALISES every window of a corpus,
which is what the device sampler (vqcpc_bach_amd/dataloaders/corpus.py, csrc/corpus.hip) must never do and must agree with.
Shares no code with the package.  The per-window transposition ranges (:135-139) are not restated: one piece is one transposition.
"""
import numpy as np

SUB = 4


def extract_with_padding(piece, start_tick, end_tick, start, end, pad):
    """piece (ticks, 4); rows [start_tick, end_tick) with the padding of chorale_dataset.py:418-470 (there voice-major)."""
    assert start_tick < end_tick and end_tick > 0                    # :427-428
    length = piece.shape[0]
    parts = []
    if start_tick < 0:                                               # :432-446
        if start_tick == -1:
            parts.append(np.tile(start, (1, 1)))
        else:
            parts.append(np.tile(pad, (-start_tick - 1, 1)))
            parts.append(np.tile(start, (1, 1)))
    parts.append(piece[max(start_tick, 0):min(end_tick, length)])     # :448-451
    if end_tick > length:                                            # :453-467
        if end_tick - length == 1:
            parts.append(np.tile(end, (1, 1)))
        else:
            parts.append(np.tile(end, (1, 1)))
            parts.append(np.tile(pad, (end_tick - length - 1, 1)))
    return np.concatenate(parts, axis=0).astype(np.int64)


def materialise(pieces, W, start, end, pad, last_start_beat=None):
    """Every window of W beats, piece-major, start beats -(W - 1) .. last ascending (:124-129 with the stated upper bound):
    (n_windows, W * 4, 4) int64."""
    start, end, pad = (np.asarray(a, dtype=np.int64) for a in (start, end, pad))
    rows = []
    for p, piece in enumerate(pieces):
        piece = np.asarray(piece, dtype=np.int64)
        assert piece.shape[0] % SUB == 0
        last = piece.shape[0] // SUB - 1 if last_start_beat is None else int(last_start_beat[p])
        for o in range(-(W - 1), last + 1):
            w = extract_with_padding(piece, o * SUB, (o + W) * SUB, start, end, pad)
            assert w.shape == (W * SUB, 4)
            rows.append(w)
    return np.stack(rows)


def split_ranges(n):
    """(train, val, test) id ranges: the first int(0.85 n), the next int(0.10 n), the rest (:561-567, by id order)."""
    a = int(0.85 * n)
    b = int(0.10 * n)
    return (0, a), (a, a + b), (a + b, n)


def seeded_pieces(beats, vocab, seed):
    """Random pieces of the given beat counts over the first vocab - 3 tokens of each voice (the last three are START, END, PAD)."""
    rng = np.random.RandomState(seed)
    return [np.stack([rng.randint(0, v - 3, size=nb * SUB) for v in vocab], axis=1) for nb in beats]


def specials(vocab):
    v = np.asarray(vocab)
    return v - 3, v - 2, v - 1          # START, END, PAD
