"""vqcpc_corpus_permute and vqcpc_corpus_gather (csrc/corpus.hip) called directly, on device tables this file builds itself: the
permutation is a bijection of every n, the gathered windows equal the materialised dataset of tests/corpus_reference.py (exact
integer equality throughout)."""
import functools

import numpy as np
import pytest
import torch

import corpus_reference as R

pytestmark = pytest.mark.gpu

VOCAB = [50, 41, 33, 60]
START, END, PAD = R.specials(VOCAB)
SENTINEL = -7


def _call(name, *args):
    from vqcpc_bach_amd import hip
    hip.load()
    hip.call(name, *args)


def _permute(lo, n, key, q0, count):
    ids = torch.full((count,), SENTINEL, dtype=torch.int64, device='cuda')
    _call('vqcpc_corpus_permute', ids, lo, n, key, q0, count)
    return ids.cpu().numpy()


@pytest.mark.parametrize('n', [1, 2, 3, 5, 16, 17, 1000, 4099])
def test_permute_is_a_bijection_and_repeats_with_period_n(n):
    lo = 37
    ids = _permute(lo, n, 0x1234ABCD5678, 0, 2 * n)
    assert np.array_equal(np.sort(ids[:n]), np.arange(lo, lo + n)), 'positions 0 .. n - 1 must give every id exactly once'
    assert np.array_equal(ids[n:], ids[:n])


def test_permute_keys_and_split_calls():
    a, b = _permute(0, 1000, 1, 0, 1000), _permute(0, 1000, 2, 0, 1000)
    assert not np.array_equal(a, b) and (a == b).mean() < 0.05
    assert not np.array_equal(a, np.arange(1000))
    whole = _permute(5, 1000, 99, 123, 1001)                              # wraps past n inside the call
    halves = np.concatenate([_permute(5, 1000, 99, 123, 500), _permute(5, 1000, 99, 623, 501)])
    assert np.array_equal(whole, halves)
    assert np.array_equal(whole[:877], _permute(5, 1000, 99, 0, 1000)[123:])
    with pytest.raises(Exception, match='corpus_permute'):
        _permute(0, 0, 1, 0, 4)


# ---- gather ----------------------------------------------------------------------------------------------------------------
def _beats(W, P):
    return [1, 2, max(W - 1, 1), W, W + 1, 40] if P == 6 else [W + 1]


@functools.lru_cache(maxsize=None)
def _corpus(W, P):
    """(reference windows (n, 4 W, 4), device tables) of the seeded corpus for window length W; computed once."""
    pieces = R.seeded_pieces(_beats(W, P), VOCAB, seed=10 * W + P)
    ref = R.materialise(pieces, W, START, END, PAD)
    ref.setflags(write=False)
    counts = [p.shape[0] // 4 - 1 + W for p in pieces]
    assert sum(counts) == len(ref)
    dev = dict(
        tokens=torch.from_numpy(np.concatenate(pieces).astype(np.int32)).cuda(),
        piece_start=torch.from_numpy(np.concatenate([[0], np.cumsum([p.shape[0] for p in pieces])]).astype(np.int64)).cuda(),
        win_cum=torch.from_numpy(np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)).cuda(),
        special=torch.from_numpy(np.concatenate([START, END, PAD]).astype(np.int32)).cuda(),
        flag=torch.zeros(1, dtype=torch.int32, device='cuda'), P=P, W=W)
    return ref, dev


def _gather(dev, ids, out, ld_row, ld_tick, split=None, out2=None, ld_row2=0, ld_tick2=0):
    ticks = dev['W'] * 4
    _call('vqcpc_corpus_gather', dev['tokens'], dev['piece_start'], dev['win_cum'], dev['special'], dev['P'], dev['W'], 4, ids,
          ids.numel(), out, ld_row, ld_tick, ticks if split is None else split, out2, ld_row2, ld_tick2, dev['flag'])


@pytest.mark.parametrize('B', [1, 64])
@pytest.mark.parametrize('P', [1, 6])
@pytest.mark.parametrize('W', [1, 2, 16])
def test_gather_every_window_against_the_materialised_dataset(W, P, B):
    ref, dev = _corpus(W, P)
    n, T = len(ref), 4 * W
    order = np.random.RandomState(W + P + B).permutation(n)
    order = np.resize(order, -(-n // B) * B)                              # every id at least once, whole batches (repeats the order)
    for batch in order.reshape(-1, B):
        ids = torch.from_numpy(batch).cuda()
        out = torch.full((B, T, 4), SENTINEL, dtype=torch.int64, device='cuda')
        _gather(dev, ids, out, T * 4, 4)
        assert np.array_equal(out.cpu().numpy(), ref[batch]), batch
    assert int(dev['flag'].item()) == 0


def test_gather_negative_layout():
    ref, dev = _corpus(1, 6)
    B, N, Kr = 5, 3, 2
    ids = torch.from_numpy(np.random.RandomState(3).randint(0, len(ref), size=(B, N, Kr))).cuda()
    out = torch.full((B, N, Kr, 4, 4), SENTINEL, dtype=torch.int64, device='cuda')
    _gather(dev, ids, out, 16, 4)
    assert np.array_equal(out.cpu().numpy(), ref[ids.cpu().numpy()])


@pytest.mark.parametrize('col', [1, 2], ids=['unaligned_scalar_stores', 'aligned_vector_stores'])
def test_gather_strided_outputs_leave_the_guards_untouched(col):
    """Output rows inside a larger int64 buffer: guard rows, guard ticks and guard columns keep their sentinel.  Column offset 1
    is 8-byte aligned only (the scalar-store path), column offset 2 is 16-byte aligned (two 16-byte stores per tick)."""
    W = 2
    ref, dev = _corpus(W, 6)
    B, T = 7, 4 * W
    ids_np = np.random.RandomState(col).randint(0, len(ref), size=B)
    ids = torch.from_numpy(ids_np).cuda()
    big = torch.full((B + 2, T + 3, 8), SENTINEL, dtype=torch.int64, device='cuda')
    view = big[1:1 + B, 2:2 + T, col:col + 4]
    _gather(dev, ids, view, big.stride(0), big.stride(1))
    want = np.full(tuple(big.shape), SENTINEL, dtype=np.int64)
    want[1:1 + B, 2:2 + T, col:col + 4] = ref[ids_np]
    assert np.array_equal(big.cpu().numpy(), want)
    # the same windows split at tick 3 over two guarded buffers (x_left / x_right in one launch)
    left = torch.full((B, 3 + 1, 8), SENTINEL, dtype=torch.int64, device='cuda')
    right = torch.full((B + 1, T - 3 + 2, 6), SENTINEL, dtype=torch.int64, device='cuda')
    _gather(dev, ids, left[:, :3, col:col + 4], left.stride(0), left.stride(1), split=3, out2=right[:B, 1:1 + T - 3, col:col + 4],
            ld_row2=right.stride(0), ld_tick2=right.stride(1))
    wl = np.full(tuple(left.shape), SENTINEL, dtype=np.int64)
    wl[:, :3, col:col + 4] = ref[ids_np][:, :3]
    wr = np.full(tuple(right.shape), SENTINEL, dtype=np.int64)
    wr[:B, 1:1 + T - 3, col:col + 4] = ref[ids_np][:, 3:]
    assert np.array_equal(left.cpu().numpy(), wl) and np.array_equal(right.cpu().numpy(), wr)


def test_out_of_range_id_sets_the_flag_and_writes_nothing():
    ref, dev = _corpus(2, 6)
    n, T = len(ref), 8
    dev['flag'].zero_()
    ids_np = np.array([0, n, -1, n - 1, 2 ** 40])
    out = torch.full((5, T, 4), SENTINEL, dtype=torch.int64, device='cuda')
    _gather(dev, torch.from_numpy(ids_np).cuda(), out, T * 4, 4)
    got = out.cpu().numpy()
    assert int(dev['flag'].item()) == 1
    assert np.array_equal(got[[0, 3]], ref[[0, n - 1]])
    assert (got[[1, 2, 4]] == SENTINEL).all()
    dev['flag'].zero_()


def test_gather_rejects_bad_arguments():
    ref, dev = _corpus(2, 6)
    ids = torch.zeros(2, dtype=torch.int64, device='cuda')
    out = torch.zeros(2, 8, 4, dtype=torch.int64, device='cuda')
    with pytest.raises(Exception, match='corpus_gather'):
        _gather(dev, ids, out, 32, 3)                                     # a tick is 4 words
    with pytest.raises(Exception, match='corpus_gather'):
        _gather(dev, ids, out, 32, 4, split=3)                            # ticks past the split need out2
    with pytest.raises(Exception, match='corpus_gather'):
        _gather(dev, ids, out, 32, 4, split=9)
