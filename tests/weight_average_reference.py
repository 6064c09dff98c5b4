"""The weight-averaging rule of vqcpc_weight_average (include/vqcpc.h) restated twice: in numpy float32, operation by operation
as the kernel rounds them (the kernel tests compare BITS against it), and as a float64 closed form (what the float32 chain is
itself checked against, tests/test_weight_average_reference_cpu.py).

    d_u = min(decay, float(1 + u) / float(10 + u)) ;  w = 1 - d_u ;  avg = avg + w * (p - avg)        u = 1, 2, ...
"""
import numpy as np

F32 = np.float32


def decay_f32(decay, u):
    """d_u as the kernel computes it: the two integers are formed exactly, each converted to float32 (round to nearest even,
    which matters from 2**24 on), one float32 division, one minimum."""
    assert u >= 1
    num = F32(np.uint64(1 + int(u)))
    den = F32(np.uint64(10 + int(u)))
    return np.minimum(F32(decay), F32(num / den))


def update_f32(avg, p, decay, u):
    """One update, float32, every operation rounded on its own.  Returns a new array."""
    avg = np.asarray(avg, dtype=F32)
    p = np.asarray(p, dtype=F32)
    w = F32(F32(1.0) - decay_f32(decay, u))
    diff = (p - avg).astype(F32)
    return (avg + (w * diff).astype(F32)).astype(F32)


def average_f32(avg0, trajectory, decay, u0=1):
    """The float32 chain over a recorded parameter trajectory: update u0 sees trajectory[0], u0 + 1 sees trajectory[1], ..."""
    avg = np.asarray(avg0, dtype=F32).copy()
    for k, p in enumerate(trajectory):
        avg = update_f32(avg, p, decay, u0 + k)
    return avg


def decay_f64(decay, u):
    """d_u of the rule itself: `decay` is the float32 the kernel receives, everything else exact in float64."""
    return min(float(F32(decay)), (1.0 + u) / (10.0 + u))


def average_f64(avg0, trajectory, decay, u0=1):
    """Closed form in float64: avg_n = avg0 * prod_k d_k + sum_k (1 - d_k) p_k prod_{j > k} d_j."""
    avg0 = np.asarray(avg0, dtype=np.float64)
    ds = [decay_f64(decay, u0 + k) for k in range(len(trajectory))]
    out = avg0 * np.prod(ds) if ds else avg0.copy()
    for k, p in enumerate(trajectory):
        out = out + (1.0 - ds[k]) * np.prod(ds[k + 1:]) * np.asarray(p, dtype=np.float64)
    return out


def crossover(decay):
    """The first update at which `decay` alone acts: u >= (10 decay - 1) / (1 - decay)."""
    d = float(F32(decay))
    return int(np.ceil((10.0 * d - 1.0) / (1.0 - d)))
