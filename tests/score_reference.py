"""Float64 reference of vqcpc_decode_score (csrc/score.hip) and of the window plan of `Decoder.score_tokens`.  TEST
INFRASTRUCTURE: nothing here imports the package under test.  Anchored on the CPU by tests/test_score_reference_cpu.py; used by
tests/test_decode_score_kernel_gpu.py and tests/test_score_tokens_gpu.py.

  score_ref            the six outputs of one row in numpy float64
  rank_best_fp32       rank and best restated on the fp32 row itself: exact integer functions of its comparisons
  entropy_bound        the fp32 error bound of the kernel's entropy chain (logp / best_logp: constrained_reference.logp_bound,
                       logmass: masked_reference.logmass_bound -- the kernel restates the samplers' lines)
  start_end_times_ref  the window rule of `Decoder.compute_start_end_times`, restated
  window_plan_ref      the distinct windows of a code range and the codes scored in each
"""
import numpy as np

from constrained_reference import ULP_EXP, ULP_LOG
from decode_reference import U_FP32

# fp32 division of the device library within the OpenCL full-profile accuracy (x / y <= 2.5 ulp; hipcc's default is the correctly
# rounded one, 0.5 ulp); an ulp is at most 2 u relative
ULP_DIV = 2.5


def effective_set(allowed, V):
    """allowed (>= V,) bool or None -> (V,) bool: only entries [0, V) count, a set without any (or None) restricts nothing."""
    if allowed is None:
        return np.ones(V, dtype=bool)
    a = np.asarray(allowed, dtype=bool)[:V].copy()
    return a if a.any() else np.ones(V, dtype=bool)


def score_ref(row, tok, allowed=None):
    """row (V,) logits of the position's voice (-inf allowed, not all of them), tok its target in [0, V), allowed (>= V,) bool
    or None -> dict of the six outputs in float64 / int:
      logp       log_softmax(row)[tok]
      logmass    log sum_{i allowed} softmax(row)_i, each log-sum-exp with its own maximum subtracted (-inf: no mass)
      entropy    -sum_i p_i log p_i in nats, 0 log 0 = 0
      rank       #{i : row_i > row_tok or (row_i == row_tok and i < tok)}
      best       argmax, the lowest index among equals
      best_logp  log_softmax(row)[best]"""
    r = np.asarray(row, dtype=np.float64)
    V, tok = r.size, int(tok)
    assert 0 <= tok < V
    d = r - r.max()
    e = np.exp(d)
    L = np.log(e.sum())
    lsm = d - L
    p = e / e.sum()
    live = p > 0
    a = effective_set(allowed, V)
    ra = r[a]
    if ra.max() == -np.inf:
        logmass = -np.inf
    else:
        logmass = float((ra.max() - r.max()) + np.log(np.exp(ra - ra.max()).sum()) - L)
    idx = np.arange(V)
    best = int(np.flatnonzero(r == r.max())[0])
    return dict(logp=float(lsm[tok]), logmass=logmass, entropy=float(-(p[live] * lsm[live]).sum()),
                rank=int(((r > r[tok]) | ((r == r[tok]) & (idx < tok))).sum()), best=best, best_logp=float(lsm[best]))


def rank_best_fp32(row, tok):
    """(rank, best) from the fp32 row's own comparisons: what the kernel must give exactly."""
    r = np.asarray(row, dtype=np.float32)
    tok = int(tok)
    idx = np.arange(r.size)
    rank = int(((r > r[tok]) | ((r == r[tok]) & (idx < tok))).sum())
    return rank, int(np.flatnonzero(r == r.max())[0])


def entropy_bound(row):
    """Bound on |entropy_fp32 - entropy_64| for the kernel's chain on the fp32 row `row` (V <= 256 entries, -inf allowed), in the
    manner of constrained_reference.logp_bound (u = 2^-24, gamma_9 = 9u / (1 - 9u) for the nine additions on the path of any term of
    a lane-serial sum of four and a six-level butterfly, expf and logf within 3 ulp).  The kernel forms the entropy as

      H = L + A / s,   s = sum_i e_i,  A = sum_i e_i d_i,  L = log s,  d_i = m - row_i >= 0,  e_i = exp(-d_i)

    in which every term is >= 0, so no sum cancels:

      m      = max_i row_i                       exact
      d_i    = fl(m - row_i)                     relative error <= u (the same rounding as the sampler's fl(row_i - m))
      e_i    = expf(-d_i)                        relative error ee_i <= u d_i e^{u d_i} + 2 u ULP_EXP, plus an absolute 2^-126 where
                                                 the result is subnormal or flushed to zero
      a_i    = fl(e_i d_i)                       one more rounding (none when it is fused into the sum): relative (1 + ee_i)(1 + u)^2 - 1,
                                                 plus an absolute 2^-126 (1 + d_i) for the underflows of e_i and of the product
      A, s   = the two sums                      relative gamma_9 each, all terms >= 0
      q      = fl(A / s)                         q <= (A + dA) / (s (1 - ds)) (1 + 2 u ULP_DIV); the other side deviates by less
      L      = logf(s)                           |error| <= ds (1 + ds) + 2 u ULP_LOG |L|   (logp_bound's; s >= 1 as e_max = 1)
      H      = fl(L + q)                         + u |H|

    with ds the relative error of s, logp_bound's `ds`, and dA the absolute error of A.  V = 1 gives H = 0 exactly in the kernel;
    the bound stays at its constant terms."""
    r = np.asarray(row, dtype=np.float64)
    V = r.size
    u = U_FP32
    g9 = 9 * u / (1.0 - 9 * u)
    d = r.max() - r
    live = np.isfinite(d)
    dl = d[live]
    e = np.exp(-dl)
    s = e.sum()
    p = e / s
    ee = u * dl * np.exp(u * dl) + 2 * u * ULP_EXP
    ds = float((p * ee).sum()) * (1.0 + g9) + g9 + V * 2.0 ** -126
    a = e * dl
    A = a.sum()
    dA = float((a * ((1.0 + ee) * (1.0 + u) ** 2 * (1.0 + g9) - 1.0)).sum()) + float((2.0 ** -126 * (1.0 + dl)).sum()) * (1.0 + g9)
    q = A / s
    dq = (A + dA) / (s * (1.0 - ds)) * (1.0 + 2 * u * ULP_DIV) - q
    L = float(np.log(s))
    H = L + q
    return ds * (1.0 + ds) + 2 * u * ULP_LOG * abs(L) + dq + u * abs(H)


def start_end_times_ref(t, num_blocks, num_blocks_model):
    """The model window [begin, end) of codes in which code t of `num_blocks` codes is generated, and t's index in it
    (the rule of the reference's decoder.py:831-854): the first window while t < S // 2, the last one from num_blocks - S // 2 on,
    and between them a window that holds t at index S // 2."""
    half = num_blocks_model // 2
    if t < half:
        begin = 0
    elif t >= num_blocks - half:
        begin = num_blocks - num_blocks_model
    else:
        begin = t - half
    begin = min(max(begin, 0), num_blocks - num_blocks_model)
    return begin, begin + num_blocks_model, t - begin


def window_plan_ref(num_blocks, num_blocks_model, code_index_start, code_index_end):
    """[(window's first code, first scored code, one past the last scored code)], ascending, from `start_end_times_ref`."""
    by_window = {}
    for t in range(code_index_start, code_index_end):
        by_window.setdefault(start_end_times_ref(t, num_blocks, num_blocks_model)[0], []).append(t)
    plan = []
    for w in sorted(by_window):
        ts = by_window[w]
        assert ts == list(range(ts[0], ts[-1] + 1))
        plan.append((w, ts[0], ts[-1] + 1))
    return plan
