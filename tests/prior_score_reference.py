"""Float64 reference of vqcpc_prior_score (csrc/prior_score.hip) and of the window plan of
`PriorRelative.score_codes(method='windows')`.  TEST INFRASTRUCTURE: nothing here imports the package under test.  Anchored on the
CPU by tests/test_prior_score_reference_cpu.py; used by tests/test_prior_score_kernel_gpu.py and tests/test_prior_score_windows_gpu.py.

  target_digit         the target of a row: the code clamped to the V^ncb codes, and its digit `stage`
  prior_score_ref      the five outputs of one row in numpy float64
  rank_best_fp32       rank and best restated on the fp32 row itself: exact integer functions of its comparisons
  entropy_bound        the fp32 error bound of the kernel's entropy chain (logp / best_logp: prior_constrained_reference.logp_bound --
                       the kernel restates the sampler's lines)
  run_columns_ref      the columns `IncrementalPrior.run` scores, move by move, restated from its loop
  window_plan_ref      the distinct windows of a sequence and the columns scored in each, from a column -> window rule
"""
import numpy as np

from constrained_reference import ULP_EXP, ULP_LOG
from decode_reference import U_FP32
from prior_constrained_reference import SUM_CHAIN
from score_reference import ULP_DIV


def target_digit(code, V, ncb=1, stage=0):
    """The row's target: `code` clamped to [0, V^ncb) as the samplers clamp a forced code, then (code // V^stage) % V."""
    c = min(max(int(code), 0), V ** ncb - 1)
    return (c // V ** stage) % V


def prior_score_ref(row, tok):
    """row (V,) logits (-inf allowed, not all of them), tok the row's target in [0, V) -> dict of the five outputs in float64 / int:
      logp       log_softmax(row)[tok]  (-inf for a -inf target)
      entropy    -sum_i p_i log p_i in nats, 0 log 0 = 0
      rank       #{i : row_i > row_tok or (row_i == row_tok and i < tok)}
      best       argmax, the lowest index among equals
      best_logp  log_softmax(row)[best]"""
    r = np.asarray(row, dtype=np.float64)
    V, tok = r.size, int(tok)
    assert 0 <= tok < V
    d = r - r.max()
    e = np.exp(d)
    lsm = d - np.log(e.sum())
    p = e / e.sum()
    live = p > 0
    idx = np.arange(V)
    best = int(np.flatnonzero(r == r.max())[0])
    return dict(logp=float(lsm[tok]), entropy=float(-(p[live] * lsm[live]).sum()),
                rank=int(((r > r[tok]) | ((r == r[tok]) & (idx < tok))).sum()), best=best, best_logp=float(lsm[best]))


def rank_best_fp32(row, tok):
    """(rank, best) from the fp32 row's own comparisons: what the kernel must give exactly."""
    r = np.asarray(row, dtype=np.float32)
    tok = int(tok)
    idx = np.arange(r.size)
    return int(((r > r[tok]) | ((r == r[tok]) & (idx < tok))).sum()), int(np.flatnonzero(r == r.max())[0])


def entropy_bound(row):
    """Bound on |entropy_fp32 - entropy_64| for the kernel's chain on the fp32 row `row` (V <= 4096 entries, -inf allowed): the
    derivation of score_reference.entropy_bound with the prior kernels' summation tree -- thread t adds its 16 codes in ascending
    order to 0.0f (15 roundings), six butterfly levels, two levels over the four waves: gamma_23 = 23u / (1 - 23u) in place of
    gamma_9 (prior_constrained_reference.SUM_CHAIN; the single-wave form of V <= 1024 has two additions fewer).  The kernel forms

      H = L + A / s,   s = sum_i e_i,  A = sum_i e_i d_i,  L = log s,  d_i = m - row_i >= 0,  e_i = exp(-d_i)

    in which every term is >= 0, so no sum cancels:

      d_i    = fl(m - row_i)                     relative error <= u
      e_i    = expf(-d_i)                        relative error ee_i <= u d_i e^{u d_i} + 2 u ULP_EXP, plus an absolute 2^-126 where
                                                 the result is subnormal or flushed to zero
      a_i    = fl(e_i d_i)                       relative (1 + ee_i)(1 + u)^2 - 1 (one rounding fewer when the product is fused into
                                                 the sum), plus an absolute 2^-126 (1 + d_i) for the underflows
      A, s   = the two sums                      relative gamma_23 each, all terms >= 0
      q      = fl(A / s)                         q <= (A + dA) / (s (1 - ds)) (1 + 2 u ULP_DIV)
      L      = logf(s)                           |error| <= ds (1 + ds) + 2 u ULP_LOG |L|   (s >= 1 as e_max = 1)
      H      = fl(L + q)                         + u |H|

    with ds the relative error of s and dA the absolute error of A."""
    r = np.asarray(row, dtype=np.float64)
    V = r.size
    u = U_FP32
    g = SUM_CHAIN * u / (1.0 - SUM_CHAIN * u)
    d = r.max() - r
    dl = d[np.isfinite(d)]
    e = np.exp(-dl)
    s = e.sum()
    p = e / s
    ee = u * dl * np.exp(u * dl) + 2 * u * ULP_EXP
    ds = float((p * ee).sum()) * (1.0 + g) + g + V * 2.0 ** -126
    a = e * dl
    A = a.sum()
    dA = float((a * ((1.0 + ee) * (1.0 + u) ** 2 * (1.0 + g) - 1.0)).sum()) + float((2.0 ** -126 * (1.0 + dl)).sum()) * (1.0 + g)
    q = A / s
    dq = (A + dA) / (s * (1.0 - ds)) * (1.0 + 2 * u * ULP_DIV) - q
    L = float(np.log(s))
    return ds * (1.0 + ds) + 2 * u * ULP_LOG * abs(L) + dq + u * abs(L + q)


def run_columns_ref(L, N, k):
    """[(window's first code, [the sequence columns scored in it])] in the order `IncrementalPrior.run` visits them: N steps in
    window 0; per full move i the window (i + 1) k re-prefilled to position N - k and k steps; a last move to L - N re-prefilled to
    N - rem with rem steps.  A step at window position p of window w writes column w + p."""
    moves = [(0, list(range(N)))]
    n_full, rem = divmod(L - N, k)
    for i in range(n_full):
        w, P = (i + 1) * k, N - k
        moves.append((w, [w + p for p in range(P, N)]))
    if rem:
        w, P = L - N, N - rem
        moves.append((w, [w + p for p in range(P, N)]))
    return moves


def window_of_column(e, L, N, k):
    """The first code of the window in which column e is scored: window 0 for e < N; afterwards the j-th later column (j = e - N)
    belongs to full move j // k, at window (j // k + 1) k, or -- past the last full move -- to the last window L - N."""
    if e < N:
        return 0
    j = e - N
    return (j // k + 1) * k if j // k < (L - N) // k else L - N


def window_plan_ref(L, N, k):
    """[(window's first code, first scored column, one past the last scored column)], ascending, from `window_of_column`."""
    by_window = {}
    for e in range(L):
        by_window.setdefault(window_of_column(e, L, N, k), []).append(e)
    plan = []
    for w in sorted(by_window):
        es = by_window[w]
        assert es == list(range(es[0], es[-1] + 1))
        plan.append((w, es[0], es[-1] + 1))
    return plan
