"""The duplicate check through its public surface: DeviceCorpus.longest_common_run / split_pieces and Decoder.check_duplicate /
check_duplicate_all_corpus on a tiny decoder over a small saved corpus, against the difflib reference of
tests/duplicates_reference.py.  Exact integer equality."""
import functools
import json

import numpy as np
import pytest
import torch

import corpus_reference as CR
import duplicates_reference as R

pytestmark = pytest.mark.gpu

VOCAB = (11, 12, 13, 14)                                   # tests/golden/decoder_tiny.npz; 12 events = windows of 3 beats
BEATS = (12, 9, 16, 7, 20, 5, 3, 2, 2, 1, 1, 2)            # windows of 3 beats: pieces 0-7 begin in train, 8-10 in val, 11 in test
W = 3
KEYS = ('length', 'query_tick', 'query_voice', 'piece', 'piece_tick', 'voice')


@functools.lru_cache(maxsize=None)
def _pieces():
    pieces = CR.seeded_pieces(BEATS, VOCAB, seed=21)        # tokens < vocab - 3: START / END / PAD never occur in a piece
    for p in pieces:
        p.setflags(write=False)
    return pieces


@pytest.fixture(scope='module')
def dec(tmp_path_factory):
    from conftest import load_golden, sub_state
    from oracle import decoder_oracle as D
    from test_decoder_gpu import build_decoder
    from vqcpc_bach_amd.dataloaders.corpus import CorpusDataloaderGenerator, save_corpus
    g = load_golden('decoder_tiny')
    cfg = D.make_cfg(**json.loads(str(g['cfg_json'])))
    assert tuple(cfg['vocab']) == VOCAB and cfg['events'] == 4 * W
    path = str(tmp_path_factory.mktemp('dup') / 'corpus.npz')
    save_corpus(path, _pieces(), VOCAB, *CR.specials(VOCAB))
    d = build_decoder(cfg, sub_state(g, 'sd0'))
    d.dataloader_generator = CorpusDataloaderGenerator(path, sequences_size=W, seed=1, device='cuda')
    return d


def _pad_rows(n):
    return np.tile(CR.specials(VOCAB)[2], (n, 1)).astype(np.int64)


def _row(out, g=None):
    return {k: int(out[k] if g is None else out[k][g]) for k in KEYS}


def test_split_pieces_partition_the_pieces_by_their_first_window(dec):
    dc = dec.dataloader_generator.device_corpus
    firsts = np.concatenate([[0], np.cumsum([b + W - 1 for b in BEATS])])
    ranges = CR.split_ranges(int(firsts[-1]))
    want = [[p for p in range(len(BEATS)) if lo <= firsts[p] < hi] for lo, hi in ranges]
    assert want == [list(range(0, 8)), [8, 9, 10], [11]], 'the plan of this file'
    got = [dc.split_pieces(s, W) for s in ('train', 'val', 'test')]
    assert got == [(w[0], w[-1] + 1) for w in want]


def test_an_edited_corpus_window_returns_the_planted_run(dec, capsys):
    pieces = _pieces()
    original = pieces[4][30:42]                                             # 12 ticks of a train piece
    gen = original.copy().reshape(-1)
    gen[[5, 38, 39]] = [VOCAB[1] - 1, VOCAB[2] - 1, VOCAB[3] - 1]           # PAD ids: in no piece
    gen = gen.reshape(12, 4)
    want = R.longest_run(gen, pieces, 0, 8)
    assert want == (32, 6, 4, 4 * 30 + 6), 'tokens 6 .. 37 of the window survive the edits'
    out = dec.check_duplicate_all_corpus(torch.from_numpy(gen))
    assert _row(out) == R.as_dict(want) == dict(length=32, query_tick=1, query_voice=2, piece=4, piece_tick=31, voice=2)
    assert out['best_x'].shape == (12, 4) and np.array_equal(out['best_x'], original)
    printed = capsys.readouterr().out
    assert 'Num tokens plagiarisms: 32' in printed and 'Num beats plagiarisms: 2.0' in printed
    on_device = dec.check_duplicate_all_corpus(torch.from_numpy(gen).cuda(), split=None)
    assert _row(on_device) == _row(out)


def test_a_batch_of_three_rows(dec):
    pieces = _pieces()
    rows = np.stack([np.concatenate([_pad_rows(5), pieces[1][:7]]),         # the piece's first 7 ticks after padding
                     _pad_rows(12),                                         # nothing but padding: never counted as copied
                     np.concatenate([pieces[6][-4:], _pad_rows(8)])])
    rows[2, 3, 3] = VOCAB[3] - 1
    out = dec.check_duplicate_all_corpus(torch.from_numpy(rows).cuda())
    want = [R.longest_run(r, pieces, 0, 8) for r in rows]
    assert want == [(28, 20, 1, 0), R.NO_MATCH, (15, 0, 6, 4 * 8)]
    assert [_row(out, g) for g in range(3)] == [R.as_dict(w) for w in want]
    start, end, pad = CR.specials(VOCAB)
    assert out['best_x'].shape == (3, 12, 4)
    assert np.array_equal(out['best_x'][0], CR.extract_with_padding(pieces[1], -5, 7, start, end, pad))
    assert np.array_equal(out['best_x'][1], _pad_rows(12))
    assert np.array_equal(out['best_x'][2], CR.extract_with_padding(pieces[6], 8, 20, start, end, pad))


def test_the_split_excludes_a_run_of_a_val_only_piece(dec):
    pieces = _pieces()
    gen = np.concatenate([_pad_rows(2), pieces[8], _pad_rows(2)])           # all 8 ticks of a piece that begins in val
    val = dec.check_duplicate_all_corpus(torch.from_numpy(gen), split='val')
    assert _row(val) == R.as_dict((32, 8, 8, 0))
    everything = dec.check_duplicate_all_corpus(torch.from_numpy(gen), split=None)
    assert _row(everything) == _row(val)
    train = dec.check_duplicate_all_corpus(torch.from_numpy(gen), split='train')
    want = R.longest_run(gen, pieces, 0, 8)
    assert _row(train) == R.as_dict(want) and 0 <= train['piece'] < 8 and train['length'] < 32
    dc = dec.dataloader_generator.device_corpus
    assert _row(dc.longest_common_run(torch.from_numpy(gen), pieces=(8, 9))) == _row(val)
    assert _row(dc.longest_common_run(torch.from_numpy(gen), pieces=(9, 12))) == R.as_dict(R.longest_run(gen, pieces, 9, 12))


def test_pairwise_check_agrees_with_the_corpus_form_on_a_one_piece_corpus(dec, tmp_path):
    from vqcpc_bach_amd.dataloaders.corpus import CorpusDataloaderGenerator, save_corpus
    piece = _pieces()[2]
    rng = np.random.RandomState(4)
    gen = np.stack([rng.randint(0, v - 3, size=12) for v in VOCAB], axis=1)
    gen[3:8] = piece[40:45]
    gen[5, 2] = VOCAB[2] - 1
    path = str(tmp_path / 'one.npz')
    save_corpus(path, [piece], VOCAB, *CR.specials(VOCAB))
    keep = dec.dataloader_generator
    try:
        dec.dataloader_generator = CorpusDataloaderGenerator(path, sequences_size=W, seed=1, device='cuda')
        corpus_form = dec.check_duplicate_all_corpus(torch.from_numpy(gen), split=None)
    finally:
        dec.dataloader_generator = keep
    pairwise = dec.check_duplicate(torch.from_numpy(gen), torch.from_numpy(piece.copy()))
    assert _row(pairwise) == _row(corpus_form) == R.as_dict(R.longest_run(gen, [piece]))
    assert pairwise['length'] >= 10
    assert _row(dec.check_duplicate(torch.from_numpy(gen).cuda(), torch.from_numpy(piece.copy()).cuda())) == _row(pairwise)


def test_refusals(dec):
    from vqcpc_bach_amd.dataloaders.synthetic_student_dataloader import SyntheticStudentDataloaderGenerator
    gen = torch.from_numpy(_pieces()[0][:12].copy())
    with pytest.raises(NotImplementedError):
        dec.check_duplicate()
    for bad in (-1, VOCAB[1]):
        x = gen.clone()
        x[4, 1] = bad
        with pytest.raises(ValueError):
            dec.check_duplicate_all_corpus(x)
        with pytest.raises(ValueError):
            dec.check_duplicate(x, gen)
        with pytest.raises(ValueError):
            dec.check_duplicate(gen, x)
    with pytest.raises(ValueError):
        dec.dataloader_generator.device_corpus.longest_common_run(gen, pieces=(3, 3))
    keep = dec.dataloader_generator
    try:
        dec.dataloader_generator = SyntheticStudentDataloaderGenerator(sequences_size=W, vocab=VOCAB, seed=1, device='cuda')
        with pytest.raises(ValueError, match='corpus'):
            dec.check_duplicate_all_corpus(gen)
    finally:
        dec.dataloader_generator = keep
