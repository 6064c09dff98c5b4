"""Numpy restatement of the cluster census (include/vqcpc.h, "Cluster census"; csrc/clusters.hip, vqcpc_bach_amd/clusters.py): counts
by bincount, example selection by sorting packed keys, codeword neighbours by the canonical float32 chain in explicit float32
operations and a lexsort.  Shares no code with the package (the hash is restated here on Python integers)."""
import numpy as np

M64 = (1 << 64) - 1
EMPTY = np.uint64(M64)
U = 2.0 ** -24                         # unit roundoff of float32
U64 = 2.0 ** -53


def hash32(key, i):
    """h(key, id) on Python integers: the low 32 bits of the splitmix64 finaliser of key + id * 0x9E3779B97F4A7C15."""
    z = (int(key) + int(i) * 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return (z ^ (z >> 31)) & 0xFFFFFFFF


def packed(key, ids):
    return np.array([(hash32(key, i) << 32) | int(i) for i in np.asarray(ids).reshape(-1)], dtype=np.uint64)


def counts(codes, K):
    """codes (n, ncb) -> (ncb, K) int64; codes outside [0, K) are not counted."""
    codes = np.asarray(codes).reshape(len(codes), -1)
    return np.stack([np.bincount(col[(col >= 0) & (col < K)], minlength=K) for col in codes.T]).astype(np.int64)


def has_bad_code(codes, K):
    codes = np.asarray(codes)
    return bool(((codes < 0) | (codes >= K)).any())


def select(codes, ids, key, K, E):
    """(ncb, K, E) uint64: per (codebook, code) the E smallest packed keys of its members, ascending; all ones where fewer."""
    codes = np.asarray(codes).reshape(len(codes), -1)
    keys = packed(key, ids)
    out = np.full((codes.shape[1], K, E), EMPTY, dtype=np.uint64)
    for c, col in enumerate(codes.T):
        for k in np.unique(col[(col >= 0) & (col < K)]):
            mine = np.sort(keys[col == k])[:E]
            out[c, k, :len(mine)] = mine
    return out


def select_brute(codes, ids, key, K, E):
    """The same by repeated extraction of the minimum on Python integers (no sort)."""
    codes = np.asarray(codes).reshape(len(codes), -1)
    keys = [(hash32(key, i) << 32) | int(i) for i in ids]
    out = np.full((codes.shape[1], K, E), EMPTY, dtype=np.uint64)
    for c in range(codes.shape[1]):
        for k in range(K):
            mine = [v for v, code in zip(keys, codes[:, c]) if code == k]
            for e in range(min(E, len(mine))):
                out[c, k, e] = min(mine)
                mine.remove(min(mine))
    return out


def dist2_f32(e):
    """e (K, d) float32 -> (K, K) float32: acc = 0; t ascending: df = e[i][t] - e[j][t]; acc = acc + df * df, every operation a
    float32 numpy operation (rounded on its own, no FMA)."""
    e = np.asarray(e, dtype=np.float32)
    acc = np.zeros((e.shape[0], e.shape[0]), dtype=np.float32)
    for t in range(e.shape[1]):
        df = (e[:, None, t] - e[None, :, t]).astype(np.float32)
        acc = (acc + (df * df).astype(np.float32)).astype(np.float32)
    return acc


def dist2_f64(e):
    e = np.asarray(e, dtype=np.float64)
    return ((e[:, None, :] - e[None, :, :]) ** 2).sum(axis=2)


def knn_from(dist, k):
    """(K, K) distances -> (nn (K, k), dist (K, k)): per row the k smallest (distance, index) with the row's own index left out."""
    K = dist.shape[0]
    nn = np.empty((K, k), dtype=np.int64)
    for i in range(K):
        order = np.lexsort((np.arange(K), dist[i]))
        nn[i] = order[order != i][:k]
    return nn, np.take_along_axis(dist, nn, axis=1)


def knn(e, k):
    """e (ncb, K, d) -> (nn (ncb, K, k) int64, dist2 (ncb, K, k) float32) by the float32 chain."""
    res = [knn_from(dist2_f32(book), k) for book in e]
    return np.stack([r[0] for r in res]), np.stack([r[1] for r in res])


def gamma(n, u=U):
    return n * u / (1 - n * u)


def dist2_bound(d):
    """|fl(dist2) - dist2| <= dist2_bound(d) * dist2 for the float32 chain over d features, against the float64 value: per term one
    rounding of the difference, which the square counts twice, and one of the product -- (1 + delta)^3; then at most d additions of
    non-negative terms -- (1 + delta)^d on the earliest term, fewer on the others: gamma_{d + 3}.  The float64 value carries
    gamma_{d + 3} of ITS unit roundoff by the same count.  (Codewords of ordinary size: nothing underflows.)"""
    return gamma(d + 3) + gamma(d + 3, U64)
