"""Dead-code restarts of the EMA codebooks in numpy (include/vqcpc.h: vqcpc_vq_restart_candidates, vqcpc_vq_ema_restart): the
keyed hash in uint64, the candidate rows of one step on every rank, and the restart rule.  Everything the feature does is a copy
of a row or a constant, so every comparison against this file is exact."""
import numpy as np

M64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15


def mix(x):
    """The splitmix64 finaliser on a uint64 array (or a Python int), mod 2^64."""
    if isinstance(x, int):
        x &= M64
        x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
        x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
        return x ^ (x >> 31)
    x = np.asarray(x, dtype=np.uint64)
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def draws(seed, step, ncb, K):
    """r [ncb][K] uint64: key = mix(seed + (step + 1) G), r = mix(key + (c K + k + 1) G)."""
    key = mix((int(seed) + (int(step) + 1) * GOLDEN) & M64)
    ids = np.arange(1, ncb * K + 1, dtype=np.uint64)
    return mix(np.uint64(key) + ids * np.uint64(GOLDEN)).reshape(ncb, K)


def rows(seed, step, ncb, K, total):
    """The row each code draws among `total` rows (all ranks laid end to end): int64 [ncb][K]."""
    return (draws(seed, step, ncb, K) % np.uint64(total)).astype(np.int64)


def candidates(z_per_rank, seed, step, ncb, K):
    """z_per_rank: one float32 [R][ncb * dsub] array per rank, the same R everywhere.  Returns one [ncb][K][dsub] float32 array
    per rank: sub-vector c of the drawn row on the rank that owns it (r_glob // R), +0.0 on every other rank."""
    zs = [np.ascontiguousarray(z, dtype=np.float32) for z in z_per_rank]
    world, (R, D) = len(zs), zs[0].shape
    assert all(z.shape == (R, D) for z in zs) and D % ncb == 0
    dsub = D // ncb
    r = rows(seed, step, ncb, K, R * world)
    owner, local = r // R, r % R
    out = []
    for rank, z in enumerate(zs):
        cand = np.zeros((ncb, K, dsub), dtype=np.float32)
        for c in range(ncb):
            mine = owner[c] == rank
            cand[c, mine] = z[local[c, mine], c * dsub:(c + 1) * dsub]
        out.append(cand)
    return out


def restart(cand, N, m, e, thr):
    """(N, m, e, restarts [ncb] int64) after the rule: N[c][k] < thr (strict, fp32) -> e = m = cand, N = 1."""
    cand, N, m, e = (np.array(a, dtype=np.float32) for a in (cand, N, m, e))
    dead = N < np.float32(thr)
    e[dead] = cand[dead]
    m[dead] = cand[dead]
    N[dead] = np.float32(1.0)
    return N, m, e, dead.sum(axis=1).astype(np.int64)
