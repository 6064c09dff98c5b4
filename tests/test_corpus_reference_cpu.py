"""The numpy restatement of the reference's window dataset (tests/corpus_reference.py) pinned on hand-written windows, and the
host side of vqcpc_bach_amd/dataloaders/corpus.py: file round trip, validation, window counts, split boundaries, keys.  No GPU."""
import numpy as np
import pytest

import corpus_reference as R

S, E, P = [40, 41, 42, 43], [44, 45, 46, 47], [48, 49, 48, 49]          # START, END, PAD per voice
VOCAB = [50, 50, 50, 50]


def _piece(beats):
    return np.array([[t, 10 + t, 20 + t, 30 + t] for t in range(4 * beats)])


def test_two_beat_piece_three_beat_windows_by_hand():
    """Start beats -2 .. 1: PAD...START then the piece; the piece then END, PAD..."""
    n = _piece(2).tolist()
    want = [
        [P] * 7 + [S] + n[0:4],
        [P] * 3 + [S] + n[0:8],
        n[0:8] + [E] + [P] * 3,
        n[4:8] + [E] + [P] * 7,
    ]
    got = R.materialise([_piece(2)], 3, S, E, P)
    assert got.dtype == np.int64 and got.shape == (4, 12, 4)
    assert np.array_equal(got, np.array(want))


def test_both_paddings_at_once_by_hand():
    """A 2-beat piece reaches the end of a 3-beat window exactly when it is padded in front (start beat -1 above), so the case
    with BOTH paddings is a 1-beat piece: start beats -2, -1, 0."""
    n = _piece(1).tolist()
    want = [
        [P] * 7 + [S] + n,
        [P] * 3 + [S] + n + [E] + [P] * 3,
        n + [E] + [P] * 7,
    ]
    assert np.array_equal(R.materialise([_piece(1)], 3, S, E, P), np.array(want))


def test_single_tick_paddings_and_upper_bound_by_hand():
    """:440-441 and :461-462: a padding of exactly one tick is START / END alone -- reached with W = 1 never (windows are whole
    beats), so it is pinned on the extraction itself; last_start_beat cuts the enumeration."""
    piece = _piece(2)
    assert np.array_equal(R.extract_with_padding(piece, -1, 3, *map(np.array, (S, E, P))), np.array([S] + piece[0:3].tolist()))
    assert np.array_equal(R.extract_with_padding(piece, 6, 9, *map(np.array, (S, E, P))), np.array(piece[6:8].tolist() + [E]))
    full = R.materialise([piece, _piece(1)], 2, S, E, P)
    cut = R.materialise([piece, _piece(1)], 2, S, E, P, last_start_beat=[0, 0])
    assert full.shape[0] == 3 + 2 and cut.shape[0] == 2 + 2
    assert np.array_equal(cut, full[[0, 1, 3, 4]])


def test_window_order_is_piece_major_then_start_beat():
    pieces = R.seeded_pieces([3, 1, 2], VOCAB, seed=1)
    all_ = R.materialise(pieces, 2, S, E, P)
    parts = [R.materialise([p], 2, S, E, P) for p in pieces]
    assert [len(p) for p in parts] == [4, 2, 3]
    assert np.array_equal(all_, np.concatenate(parts))
    assert np.array_equal(all_[1][:8], pieces[0][:8])                  # piece 0, start beat 0


@pytest.mark.parametrize('n, want', [(1, ((0, 0), (0, 0), (0, 1))), (7, ((0, 5), (5, 5), (5, 7))),
                                      (20, ((0, 17), (17, 19), (19, 20))), (1000, ((0, 850), (850, 950), (950, 1000)))])
def test_split_boundaries(n, want):
    from vqcpc_bach_amd.dataloaders import corpus as C
    assert R.split_ranges(n) == want
    b = C.split_bounds(n)
    assert (b['train'], b['val'], b['test']) == want


def _save(tmp_path, **over):
    from vqcpc_bach_amd.dataloaders import corpus as C
    pieces = R.seeded_pieces([1, 2, 5], VOCAB, seed=3)
    kw = dict(pieces=pieces, vocab=VOCAB, start=S, end=E, pad=P)
    kw.update(over)
    path = str(tmp_path / 'corpus.npz')
    C.save_corpus(path, **kw)
    return path, pieces


def test_round_trip(tmp_path):
    from vqcpc_bach_amd.dataloaders import corpus as C
    names = [[f'v{c}n{i}' for i in range(50)] for c in range(4)]
    path, pieces = _save(tmp_path, last_start_beat=[0, 1, 3], names=names)
    c = C.load_corpus(path)
    assert c.tokens.dtype == np.int16 and np.array_equal(c.tokens, np.concatenate(pieces))
    assert c.piece_start.tolist() == [0, 4, 12, 32] and c.piece_start.dtype == np.int64
    assert c.subdivision == 4 and c.num_pieces == 3 and c.num_beats.tolist() == [1, 2, 5]
    assert (c.vocab.tolist(), c.start.tolist(), c.end.tolist(), c.pad.tolist()) == (VOCAB, S, E, P)
    assert c.last_start_beat.tolist() == [0, 1, 3]
    assert c.index2note_dicts()[2] == {i: f'v2n{i}' for i in range(50)}
    for W in (1, 2, 16):
        assert c.window_counts(W).sum() == len(R.materialise(pieces, W, S, E, P, last_start_beat=[0, 1, 3]))
    path, pieces = _save(tmp_path, dtype=np.int32)
    c = C.load_corpus(path)
    assert c.tokens.dtype == np.int32 and c.last_start_beat is None and c.names is None
    assert c.index2note_dicts()[0] == {i: i for i in range(50)}
    assert c.window_counts(3).tolist() == [3, 4, 7]


def _arrays():
    pieces = R.seeded_pieces([1, 2], VOCAB, seed=4)
    return dict(tokens=np.concatenate(pieces).astype(np.int16), piece_start=np.array([0, 4, 12]), subdivision=np.int64(4),
                vocab=np.array(VOCAB), start=np.array(S), end=np.array(E), pad=np.array(P))


def _write(tmp_path, arrays):
    path = str(tmp_path / 'bad.npz')
    with open(path, 'wb') as f:
        np.savez(f, **arrays)
    return path


def test_load_corpus_refuses_bad_files(tmp_path):
    from vqcpc_bach_amd.dataloaders import corpus as C
    C.load_corpus(_write(tmp_path, _arrays()))                          # the unmodified arrays load
    a = _arrays()
    a['tokens'][5, 2] = 50
    with pytest.raises(ValueError, match='>= the vocab'):
        C.load_corpus(_write(tmp_path, a))
    a = _arrays()
    a['tokens'][0, 0] = -1
    with pytest.raises(ValueError, match='negative token'):
        C.load_corpus(_write(tmp_path, a))
    a = _arrays()
    a['piece_start'] = np.array([0, 6, 12])
    with pytest.raises(ValueError, match='not a multiple of the subdivision'):
        C.load_corpus(_write(tmp_path, a))
    a = _arrays()
    a['piece_start'] = np.array([0, 8, 4, 12])
    with pytest.raises(ValueError, match='not monotone'):
        C.load_corpus(_write(tmp_path, a))
    a = _arrays()
    a['tokens'] = a['tokens'][:, :3]
    with pytest.raises(ValueError, match='voice count is not 4'):
        C.load_corpus(_write(tmp_path, a))
    a = _arrays()
    a['vocab'] = np.array([50, 50, 50])
    with pytest.raises(ValueError, match='voice count is not 4'):
        C.load_corpus(_write(tmp_path, a))
    a = _arrays()
    a['last_start_beat'] = np.array([0, 2])
    with pytest.raises(ValueError, match='last_start_beat'):
        C.load_corpus(_write(tmp_path, a))
    with pytest.raises(ValueError, match='voice count is not 4'):
        C.save_corpus(str(tmp_path / 'x.npz'), [np.zeros((4, 3), dtype=int)], VOCAB, S, E, P)


def test_keys_differ_in_every_component():
    from vqcpc_bach_amd.dataloaders import corpus as C
    base = C.mix_key(7, 0, 0, 0)
    keys = {base, C.mix_key(8, 0, 0, 0), C.mix_key(7, 1, 0, 0), C.mix_key(7, 0, 1, 0), C.mix_key(7, 0, 0, 1)}
    assert len(keys) == 5 and all(0 <= k < 2 ** 64 for k in keys)
    assert C.mix_key(7, 0, 0, 0) == base
