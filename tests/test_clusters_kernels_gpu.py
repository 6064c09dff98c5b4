"""vqcpc_cluster_count, vqcpc_cluster_select and vqcpc_codebook_knn (csrc/clusters.hip) called directly on inputs this file builds
itself, against tests/clusters_reference.py.  Exact integer equality (and bit equality of the float32 distances); guard words
behind every output stay untouched; the padding of strided inputs is poisoned with values that would raise the flag if read."""
import functools

import numpy as np
import pytest
import torch

import clusters_reference as R

pytestmark = pytest.mark.gpu

GUARD32 = 0x5A5A5A5A
GUARD64 = 0x5A5A5A5A5A5A5A5A
POISON = 1 << 40                       # no code and no id: it raises the flag if it is ever read
LDS_WORDS = 8192                       # ncb * K up to this is counted in LDS, above it with global atomics
KEY = 0x0123456789ABCDEF


def _call(name, *args):
    from vqcpc_bach_amd import hip
    hip.load()
    hip.call(name, *args)


def _strided(codes, extra=2):
    """(n, ncb) codes as a device view of rows ncb + extra words apart; the padding is poison."""
    codes = np.asarray(codes, dtype=np.int64).reshape(len(codes), -1)
    buf = np.full((codes.shape[0], codes.shape[1] + extra), POISON, dtype=np.int64)
    buf[:, :codes.shape[1]] = codes
    return torch.from_numpy(buf).cuda()[:, :codes.shape[1]]


def _flag():
    return torch.tensor([GUARD32, 0, GUARD32], dtype=torch.int32, device='cuda')


def _read_flag(flag):
    f = flag.cpu().numpy()
    assert f[0] == GUARD32 and f[2] == GUARD32, 'guard words around the flag'
    return int(f[1])


# ---- vqcpc_cluster_count ----------------------------------------------------------------------------------------------------------
def _new_counts(ncb, K):
    counts = torch.zeros(ncb * K + 2, dtype=torch.int32, device='cuda')
    counts[ncb * K:] = GUARD32
    return counts


def _count(codes, K, counts=None, extra=2):
    """One call; returns (counts tensor with its guard words, flag value)."""
    codes = np.asarray(codes).reshape(len(codes), -1)
    n, ncb = codes.shape
    counts = _new_counts(ncb, K) if counts is None else counts
    flag = _flag()
    view = _strided(codes, extra)
    _call('vqcpc_cluster_count', view, ncb + extra, n, ncb, K, counts, flag[1:])
    return counts, _read_flag(flag)


def _counts_of(counts, ncb, K):
    got = counts.cpu().numpy()
    assert (got[ncb * K:] == GUARD32).all(), 'guard words after counts'
    return got[:ncb * K].reshape(ncb, K).astype(np.int64)


@pytest.mark.parametrize('n', [1, 63, 64, 65, 257, 5000])
@pytest.mark.parametrize('ncb,K', [(1, 1), (1, 2), (2, 2), (1, 512), (2, 512), (3, 512), (1, LDS_WORDS), (2, LDS_WORDS // 2),
                                   (1, LDS_WORDS + 1), (3, LDS_WORDS // 3 + 1), (1, 1 << 18)])
def test_counts_equal_bincount(n, ncb, K):
    """ncb * K = 8192 is the last LDS shape, 8193 (one codebook, and three of 2731) the first with global atomics; 2^18 is a merged
    code of 512 x 512.  Half of the rows fall on 7 codes, so counts above 1 occur at every K."""
    rng = np.random.RandomState(n + K + ncb)
    codes = rng.randint(0, K, size=(n, ncb))
    few = rng.randint(0, K, size=7)
    codes = np.where(rng.random_sample((n, ncb)) < 0.5, few[rng.randint(0, 7, size=(n, ncb))], codes)
    counts, flag = _count(codes, K)
    assert np.array_equal(_counts_of(counts, ncb, K), R.counts(codes, K)) and flag == 0


@pytest.mark.parametrize('K', [512, LDS_WORDS + 1])
def test_all_rows_in_one_code(K):
    codes = np.full((5000, 2), K - 1)
    codes[:, 1] = 0
    counts, flag = _count(codes, K)
    want = np.zeros((2, K), dtype=np.int64)
    want[0, K - 1] = want[1, 0] = 5000
    assert np.array_equal(_counts_of(counts, 2, K), want) and flag == 0


@pytest.mark.parametrize('K', [2, 512, LDS_WORDS + 1])
@pytest.mark.parametrize('bad', [-1, 'K'])
def test_a_code_outside_the_codebook_raises_the_flag_and_is_not_counted(K, bad):
    rng = np.random.RandomState(K)
    codes = rng.randint(0, K, size=(300, 2))
    assert _count(codes, K)[1] == 0
    codes[177, 1] = K if bad == 'K' else bad
    counts, flag = _count(codes, K)
    assert flag == 1 and R.has_bad_code(codes, K)
    got = _counts_of(counts, 2, K)
    assert np.array_equal(got, R.counts(codes, K)) and got[1].sum() == 299 and got[0].sum() == 300


@pytest.mark.parametrize('K', [512, LDS_WORDS + 1])
def test_two_calls_over_halves_equal_one_call_over_the_whole(K):
    rng = np.random.RandomState(K)
    codes = rng.randint(0, min(K, 40), size=(5000, 3))
    whole, _ = _count(codes, K)
    halves, _ = _count(codes[:2333], K)
    halves, _ = _count(codes[2333:], K, counts=halves, extra=0)
    assert np.array_equal(_counts_of(halves, 3, K), _counts_of(whole, 3, K))
    assert np.array_equal(_counts_of(whole, 3, K), R.counts(codes, K))


# ---- vqcpc_cluster_select ---------------------------------------------------------------------------------------------------------
def _new_slots(ncb, K, E):
    slots = torch.full((ncb * K * E + 2,), -1, dtype=torch.int64, device='cuda')
    slots[ncb * K * E:] = GUARD64
    return slots


def _select(codes, K, E, ids=None, id0=0, slots=None, key=KEY):
    """One call over codes (n, ncb) with an id array (padded with poison behind it) or id0 + row."""
    codes = np.asarray(codes).reshape(len(codes), -1)
    n, ncb = codes.shape
    slots = _new_slots(ncb, K, E) if slots is None else slots
    flag = _flag()
    view = _strided(codes)
    ids_t = None
    if ids is not None:
        ids_t = torch.from_numpy(np.concatenate([np.asarray(ids, dtype=np.int64), [POISON, POISON]])).cuda()
    _call('vqcpc_cluster_select', view, ncb + 2, n, ncb, K, ids_t, id0, key, E, slots[:ncb * K * E].view(ncb, K, E), flag[1:])
    assert _read_flag(flag) == 0
    return slots


def _slots_of(slots, ncb, K, E):
    got = slots.cpu().numpy().view(np.uint64)
    assert (got[ncb * K * E:] == np.uint64(GUARD64)).all(), 'guard words after slots'
    return got[:ncb * K * E].reshape(ncb, K, E)


def _orders(codes, ids, K, E, want):
    """The same rows as one call, reversed, in a random order, and in three calls: identical slots every time."""
    ncb = codes.shape[1]
    n = len(codes)
    perm = np.random.RandomState(n + E).permutation(n)
    for name, order in (('as given', np.arange(n)), ('reversed', np.arange(n)[::-1]), ('random', perm)):
        got = _slots_of(_select(codes[order], K, E, ids=ids[order]), ncb, K, E)
        assert np.array_equal(got, want), name
    a, b = n // 3, n - n // 4
    slots = None
    for part in (perm[:a], perm[a:b], perm[b:]):
        if len(part):
            slots = _select(codes[part], K, E, ids=ids[part], slots=slots)
    assert np.array_equal(_slots_of(slots, ncb, K, E), want), 'three chunks'
    again = _slots_of(_select(codes, K, E, ids=ids), ncb, K, E)
    assert np.array_equal(again, want), 'a second run'


@pytest.mark.parametrize('E', [1, 2, 50, 64])
def test_codes_with_zero_one_and_about_e_members(E):
    """Codebook 0: codes 0 .. 4 have 0, 1, E - 1, E and E + 1 members (code 5 none); codebook 1 holds the same sizes in reverse."""
    sizes = [0, 1, E - 1, E, E + 1]
    col = np.concatenate([np.full(s, k) for k, s in enumerate(sizes)])
    rng = np.random.RandomState(E)
    col = col[rng.permutation(len(col))]
    codes = np.stack([col, 4 - col], axis=1)
    ids = rng.permutation(100000)[:len(col)].astype(np.int64)
    ids[0] = (1 << 32) - 2                                                    # the largest id
    want = R.select(codes, ids, KEY, 6, E)
    assert [(want[0, k] != R.EMPTY).sum() for k in range(6)] == [min(s, E) for s in sizes] + [0]
    assert (want[:, 5] == R.EMPTY).all() and (want[0, 0] == R.EMPTY).all()
    _orders(codes, ids, 6, E, want)


@pytest.mark.parametrize('E', [1, 2, 50, 64])
def test_five_thousand_rows_in_one_code(E):
    codes = np.full((5000, 1), 3)
    ids = np.arange(5000, dtype=np.int64)
    want = R.select(codes, ids, KEY, 5, E)
    assert np.array_equal(want[0, 3], np.sort(R.packed(KEY, ids))[:E])
    _orders(codes, ids, 5, E, want)


@pytest.mark.parametrize('E', [2, 50])
def test_ids_as_id0_plus_row_equal_ids_as_an_array(E):
    rng = np.random.RandomState(E)
    codes = rng.randint(0, 7, size=(5000, 2))
    id0 = 123456
    ids = id0 + np.arange(5000, dtype=np.int64)
    want = R.select(codes, ids, KEY, 7, E)
    assert np.array_equal(_slots_of(_select(codes, 7, E, ids=ids), 2, 7, E), want)
    assert np.array_equal(_slots_of(_select(codes, 7, E, id0=id0), 2, 7, E), want)
    slots = _select(codes[:1700], 7, E, id0=id0)                               # three chunks of consecutive ids
    slots = _select(codes[1700:1701], 7, E, id0=id0 + 1700, slots=slots)
    slots = _select(codes[1701:], 7, E, id0=id0 + 1701, slots=slots)
    assert np.array_equal(_slots_of(slots, 2, 7, E), want)
    other = _slots_of(_select(codes, 7, E, id0=id0, key=KEY + 1), 2, 7, E)
    assert not np.array_equal(other, want) and np.array_equal(other, R.select(codes, ids, KEY + 1, 7, E)), 'the key enters'


def test_a_bad_code_or_id_raises_the_flag_and_takes_no_part():
    codes = np.array([[0], [1], [9], [1], [-1]])
    ids = np.array([5, 6, 7, (1 << 32) - 1, 8], dtype=np.int64)
    slots = _new_slots(1, 3, 2)
    flag = _flag()
    _call('vqcpc_cluster_select', _strided(codes), 3, 5, 1, 3, torch.from_numpy(ids).cuda(), 0, KEY, 2, slots[:6].view(1, 3, 2),
          flag[1:])
    assert _read_flag(flag) == 1
    assert np.array_equal(_slots_of(slots, 1, 3, 2), R.select(codes[:2], ids[:2], KEY, 3, 2))


# ---- vqcpc_codebook_knn -----------------------------------------------------------------------------------------------------------
TILE_FLOATS = 8192                     # a codebook of more floats than this is streamed through LDS in tiles


@functools.lru_cache(maxsize=None)
def _codebooks(ncb, K, d):
    """Random codebooks with two coinciding codewords (2 and 5, where K allows) and three (1, 7 and 9), and their float32 / float64
    distance tables."""
    e = (np.random.RandomState(1000 * K + d).standard_normal((ncb, K, d)) * 4).astype(np.float32)
    if K > 9:
        e[:, 5] = e[:, 2]
        e[:, 7] = e[:, 1]
        e[:, 9] = e[:, 1]
    elif K == 3:
        e[:, 2] = e[:, 0]
    e.setflags(write=False)
    d32 = [R.dist2_f32(b) for b in e]
    d64 = [R.dist2_f64(b) for b in e]
    return e, d32, d64


def _knn(e, k):
    ncb, K, d = e.shape
    nn = torch.full((ncb * K * k + 2,), GUARD32, dtype=torch.int32, device='cuda')
    dist = torch.full((ncb * K * k + 2,), float('nan'), dtype=torch.float32, device='cuda')
    _call('vqcpc_codebook_knn', torch.from_numpy(np.array(e)).cuda(), ncb, K, d, k, nn, dist)
    nn, dist = nn.cpu().numpy(), dist.cpu().numpy()
    assert (nn[ncb * K * k:] == GUARD32).all() and np.isnan(dist[ncb * K * k:]).all(), 'guard words after nn and dist2'
    return nn[:ncb * K * k].reshape(ncb, K, k).astype(np.int64), dist[:ncb * K * k].reshape(ncb, K, k)


def _check_knn(ncb, K, d, k):
    """Indices and distances bit-equal to the numpy float32 chain; the distances within gamma_{d + 3} of float64 (the bound is
    derived at clusters_reference.dist2_bound: one rounding for the difference, counted twice through the square, one for the
    product, d additions of non-negative terms; plus the float64 value's own gamma at its unit roundoff)."""
    e, d32, d64 = _codebooks(ncb, K, d)
    nn, dist = _knn(e, k)
    for c in range(ncb):
        want_nn, want_dist = R.knn_from(d32[c], k)
        assert np.array_equal(nn[c], want_nn), c
        assert np.array_equal(dist[c].view(np.uint32), want_dist.view(np.uint32)), c
        exact = np.take_along_axis(d64[c], nn[c], axis=1)
        assert (np.abs(dist[c].astype(np.float64) - exact) <= R.dist2_bound(d) * exact).all(), c
        assert (nn[c] != np.arange(K)[:, None]).all(), 'self is left out'
    return nn, dist


@pytest.mark.parametrize('d', [1, 3, 16, 32])
@pytest.mark.parametrize('K', [2, 3, 65, 512])
def test_neighbours_equal_the_float32_chain(K, d):
    """K = 512 with d = 32 is 16384 floats: past the resident limit, two tiles of 256 codewords (d = 16 is exactly resident)."""
    for k in sorted({1, min(3, K - 1), min(16, K - 1)}):
        _check_knn(2 if K <= 65 else 1, K, d, k)


@pytest.mark.parametrize('K,d', [(70, 130), (200, 100)])
def test_a_codebook_streamed_in_tiles_that_are_no_multiple_of_the_group(K, d):
    """d = 130: tiles of 63 codewords (63 + 7); d = 100: tiles of 81 (81 + 81 + 38); candidates go in groups of 8."""
    assert K * d > TILE_FLOATS and (TILE_FLOATS // d) % 8
    _check_knn(2, K, d, 16)


def test_coinciding_codewords_tie_to_the_smaller_index_and_self_is_left_out_by_index():
    nn, dist = _check_knn(2, 65, 16, 3)
    for c in range(2):
        assert nn[c, 2, 0] == 5 and nn[c, 5, 0] == 2 and dist[c, 2, 0] == 0 and dist[c, 5, 0] == 0
        assert nn[c, 1, :2].tolist() == [7, 9] and nn[c, 7, :2].tolist() == [1, 9] and nn[c, 9, :2].tolist() == [1, 7]
        assert (dist[c, [1, 7, 9], :2] == 0).all() and (dist[c, [1, 7, 9], 2] > 0).all()
    nn, dist = _check_knn(2, 3, 3, 2)
    assert nn[0].tolist() == [[2, 1], [0, 2], [0, 1]] and dist[0, 0, 0] == 0 and dist[0, 2, 0] == 0


def test_refusals():
    from vqcpc_bach_amd import hip
    e = torch.zeros(1, 8, 4, device='cuda')
    nn = torch.zeros(8 * 8, dtype=torch.int32, device='cuda')
    dist = torch.zeros(8 * 8, device='cuda')
    for k in (0, 8, 17):
        with pytest.raises(hip.VqcpcHipError, match='codebook_knn'):
            _call('vqcpc_codebook_knn', e, 1, 8, 4, k, nn, dist)
    codes = torch.zeros(4, 1, dtype=torch.int64, device='cuda')
    flag = torch.zeros(1, dtype=torch.int32, device='cuda')
    counts = torch.zeros(8, dtype=torch.int32, device='cuda')
    with pytest.raises(hip.VqcpcHipError, match='cluster_count'):
        _call('vqcpc_cluster_count', codes, 1, 4, 1, (1 << 24) + 1, counts, flag)
    slots = torch.full((8, 2), -1, dtype=torch.int64, device='cuda')
    for E, id0 in ((0, 0), (65, 0), (2, (1 << 32) - 4)):
        with pytest.raises(hip.VqcpcHipError, match='cluster_select'):
            _call('vqcpc_cluster_select', codes, 1, 4, 1, 8, None, id0, KEY, E, slots, flag)
    assert int(counts.sum()) == 0 and int(flag.item()) == 0 and bool((slots == -1).all())
