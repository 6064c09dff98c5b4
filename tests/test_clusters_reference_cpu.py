"""The reference of the cluster census (tests/clusters_reference.py) against itself and against the host twins in
vqcpc_bach_amd/clusters.py: no GPU."""
import numpy as np
import pytest

import clusters_reference as R


def test_host_twin_of_the_hash_equals_an_independent_restatement():
    from vqcpc_bach_amd import clusters as C
    rng = np.random.RandomState(0)
    ids = np.concatenate([[0, 1, 2, (1 << 31) - 1, 1 << 31, (1 << 32) - 2], rng.randint(0, 1 << 32, size=500, dtype=np.int64)])
    for key in (0, 1, 0x9E3779B97F4A7C15, (1 << 64) - 1, int(rng.randint(0, 1 << 62))):
        want = np.array([R.hash32(key, i) for i in ids], dtype=np.uint64)
        got = C.select_hash(key, ids)
        assert got.dtype == np.uint64 and np.array_equal(got, want)
        assert C.select_hash(key, int(ids[7])) == int(want[7])
        assert np.array_equal(C.packed_keys(key, ids), R.packed(key, ids))
    assert len(set(C.select_hash(5, np.arange(4096)).tolist())) > 4000, 'a mix, not a constant'
    assert not np.array_equal(C.select_hash(5, np.arange(64)), C.select_hash(6, np.arange(64))), 'the key enters'


def test_census_key_is_a_function_of_seed_and_split():
    from vqcpc_bach_amd import clusters as C
    keys = {C.census_key(seed, split) for seed in (0, 1) for split in ('train', 'val', 'test')}
    assert len(keys) == 6 and all(0 <= k < 1 << 64 for k in keys)


def test_packed_keys_are_unique_and_never_the_empty_value():
    ids = np.concatenate([np.arange(5000), [(1 << 32) - 2]])
    keys = R.packed(77, ids)
    assert len(np.unique(keys)) == len(ids)
    assert (keys != R.EMPTY).all()
    assert np.array_equal(keys & np.uint64(0xFFFFFFFF), ids.astype(np.uint64))


@pytest.mark.parametrize('E', [1, 2, 5])
def test_selection_equals_a_brute_force_top_e(E):
    rng = np.random.RandomState(E)
    codes = rng.randint(0, 6, size=(200, 2))
    codes[:, 1] = np.where(rng.random_sample(200) < 0.7, 3, codes[:, 1])                # one crowded code
    ids = rng.permutation(1000)[:200]
    got, want = R.select(codes, ids, 9, 7, E), R.select_brute(codes, ids, 9, 7, E)
    assert np.array_equal(got, want)
    assert (got[:, 6] == R.EMPTY).all(), 'code 6 has no member'
    perm = rng.permutation(200)
    assert np.array_equal(R.select(codes[perm], ids[perm], 9, 7, E), got), 'a function of the set of rows'
    n = R.counts(codes, 7)
    filled = (got != R.EMPTY).sum(axis=2)
    assert np.array_equal(filled, np.minimum(n, E))


def test_counts_and_perplexity():
    from vqcpc_bach_amd import clusters as C
    codes = np.array([[0, 2], [1, 2], [1, 2], [3, -1], [4, 1]])
    assert R.counts(codes, 4).tolist() == [[1, 2, 0, 1], [0, 1, 3, 0]] and R.has_bad_code(codes, 4)
    assert not R.has_bad_code(codes[:3], 4)
    assert np.allclose(C.perplexity(np.array([[5, 5, 0, 0], [7, 0, 0, 0], [1, 1, 1, 1]])), [2.0, 1.0, 4.0], rtol=1e-15)
    p = np.array([3, 1]) / 4
    assert np.isclose(C.perplexity([3, 1]), np.exp(-(p * np.log(p)).sum()), rtol=1e-15)


@pytest.mark.parametrize('K,d', [(40, 1), (65, 3), (64, 16), (48, 32)])
def test_float32_neighbour_order_equals_the_float64_order_where_the_gap_exceeds_the_bound(K, d):
    """Two distances a < b (float64) keep their float32 order when b (1 - g) > a (1 + g), g = dist2_bound(d): wherever consecutive
    float64 distances of a row are that far apart the two orders agree position by position."""
    rng = np.random.RandomState(K + d)
    e = (rng.standard_normal((K, d)) * 4).astype(np.float32)
    e[5] = e[2]
    d32, d64 = R.dist2_f32(e), R.dist2_f64(e)
    g = R.dist2_bound(d)
    assert (np.abs(d32.astype(np.float64) - d64) <= g * d64).all()
    assert d32[2, 5] == 0 and d32[5, 2] == 0
    k = K - 1
    nn32, _ = R.knn_from(d32, k)
    nn64, s64 = R.knn_from(d64, k)
    checked = 0
    for i in range(K):
        clear_before = np.concatenate([[True], s64[i, 1:] * (1 - g) > s64[i, :-1] * (1 + g)])
        clear = clear_before & np.concatenate([clear_before[1:], [True]])            # separated from both neighbours
        assert np.array_equal(nn32[i][clear], nn64[i][clear])
        checked += int(clear.sum())
    assert checked > K * k // 2
    assert nn32[2, 0] == 5 and nn32[5, 0] == 2, 'coinciding codewords are each other\'s nearest; self is left out by index'
    assert (nn32 != np.arange(K)[:, None]).all()


def test_equal_distances_go_to_the_smaller_index():
    e = np.zeros((5, 2), dtype=np.float32)
    e[:, 0] = [0, 1, -1, 2, 0]
    nn, dist = R.knn(e[None], 3)
    assert nn[0].tolist() == [[4, 1, 2], [0, 3, 4], [0, 4, 1], [1, 0, 4], [0, 1, 2]]
    assert dist[0, 0].tolist() == [0, 1, 1]


def test_bad_arguments_are_refused_before_any_device_call():
    """Each entry point validates on the host: -1 and a message that names it (no GPU needed to be refused)."""
    import os

    import torch  # noqa: F401  (loads the process-wide HIP runtime first)
    from vqcpc_bach_amd import build, hip
    if not os.path.exists(hip.LIB_PATH):
        build.build(verbose=False)
    lib = hip.load()
    for args in ((None, 1, 4, 0, 8, None, None, None), (None, 1, 4, 65, 8, None, None, None), (None, 1, 4, 1, 0, None, None, None),
                 (None, 1, 4, 1, (1 << 24) + 1, None, None, None), (None, 1, 4, 2, 8, None, None, None),
                 (None, 1, -1, 1, 8, None, None, None), (None, 1, 4, 1, 8, None, None, None)):
        assert lib.vqcpc_cluster_count(*args) == -1 and b'cluster_count' in lib.vqcpc_last_error(), args
    for args in ((None, 1, 4, 1, 8, None, 0, 0, 0, None, None, None), (None, 1, 4, 1, 8, None, 0, 0, 65, None, None, None),
                 (None, 1, 4, 1, 8, None, -1, 0, 4, None, None, None), (None, 1, 4, 1, 8, None, (1 << 32) - 4, 0, 4, None, None, None),
                 (None, 1, 4, 1, 8, None, 0, 0, 4, None, None, None)):
        assert lib.vqcpc_cluster_select(*args) == -1 and b'cluster_select' in lib.vqcpc_last_error(), args
    for args in ((None, 1, 1, 4, 1, None, None, None), (None, 1, 8, 0, 1, None, None, None), (None, 1, 8, 1025, 1, None, None, None),
                 (None, 1, 8, 4, 0, None, None, None), (None, 1, 8, 4, 8, None, None, None), (None, 1, 32, 4, 17, None, None, None),
                 (None, 0, 8, 4, 1, None, None, None), (None, 1, 8, 4, 1, None, None, None)):
        assert lib.vqcpc_codebook_knn(*args) == -1 and b'codebook_knn' in lib.vqcpc_last_error(), args
    assert lib.vqcpc_cluster_count(None, 1, 0, 1, 8, None, None, None) == 0, 'no rows: nothing to do'
