"""Beam search over the prior's code plans, stated once in numpy (kernels: csrc/prior_beam.hip vqcpc_prior_beam_expand /
vqcpc_prior_beam_select; host: priors/generation.py `beam=W`).  TEST INFRASTRUCTURE: nothing here imports the package under test.
Anchored on the CPU by tests/test_prior_beam_reference_cpu.py; used by tests/test_prior_beam_kernel_gpu.py and
tests/test_prior_beam_gpu.py.

It is the decoder beam's rule (tests/beam_reference.py, whose start scores and ancestor walk are reused) on a
vocabulary of up to 4 096 merged codes, without an exclusion list.  Rows come in groups of W consecutive rows (slots).  At a column:

  lp(b, v)     the row's log-softmax at code v over the V logits (the kernel forms it in fp32 as the constrained sampler forms logp;
               here float64, compared within `cand_bound`)
  candidates   forced column (constraint >= 0): the one code, clamped to [0, V), the set ignored; free column: the codes of [0, V)
               in the row's set; no set, or a set with no code inside the vocabulary: the whole vocabulary   (`candidate_codes`)
  cand(b, v)   = score[b] + lp(b, v), ONE fp32 add; NaN counts as -inf; live means cand > -inf
  selection    per group the live candidates in the order cand descending, then row ascending, then code ascending (total);
               slot k < n (n = live candidates, at most W) gets the k-th: ancestor = its row, its code, score = cand;
               slots k >= n are dead: slot 0's ancestor and code, score -inf;
               n == 0: the identity, every row emits its own lowest candidate code (0 without one), score -inf      (`select`)
  row lists    what the expansion hands to the selection: a row's min(W, live) best, cand descending, then code ascending
                                                                                                               (`row_best`)

`select` is an exact function of the fp32 candidate scores: the kernel tests feed it the kernel's own `cand_out`, so ancestors,
codes and scores are pinned with no near-tie exemption."""
import numpy as np

from beam_reference import NINF, U_FP32, F, follow_ancestors, lp64, start_scores  # noqa: F401  (re-exported)

MAXV = 4096


def candidate_codes(V, forced=-1, allowed=None):
    """-> the sorted candidate codes of one row.  forced: the constraint's entry; allowed: None or an iterable of code ids (ids
    >= V are ignored, none below V: no restriction)."""
    if forced >= 0:
        return [min(max(min(int(forced), MAXV), 0), V - 1)]
    inside = None if allowed is None else sorted({int(t) for t in allowed if 0 <= int(t) < V})
    return inside if inside else list(range(V))


def cand64(score, row, codes):
    """-> (MAXV,) float64: score + lp at the candidate codes, -inf elsewhere and where the sum is NaN."""
    out = np.full(MAXV, -np.inf)
    lp = lp64(row)
    idx = np.asarray(codes, dtype=np.int64)
    with np.errstate(invalid='ignore'):
        v = float(score) + lp[idx]
    out[idx] = np.where(np.isnan(v), -np.inf, v)
    return out


def row_best(cand_row, W):
    """One row's list: [(cand, code)] of its min(W, live) best, cand descending, then code ascending."""
    c = np.asarray(cand_row, dtype=F)
    live = np.nonzero(c > NINF)[0]
    order = sorted(live.tolist(), key=lambda v: (-float(c[v]), v))
    return [(c[v], v) for v in order[:W]]


def select(cand, low, W):
    """cand (M, MAXV) float32, -inf for a non-candidate (and for a dead one); low (M,) the rows' lowest candidate codes; groups of
    W rows -> (ancestors (M,) int32 stack row indices, codes (M,) int64, score (M,) float32, n (G,) live slots, flag).  Only a
    row's W best can be among its group's W best, so the group's order is taken over the rows' lists."""
    cand = np.asarray(cand, dtype=F)
    M = cand.shape[0]
    assert M % W == 0 and cand.shape[1] == MAXV
    anc, code, sc, ns = np.arange(M, dtype=np.int32), np.zeros(M, dtype=np.int64), np.full(M, NINF, dtype=F), []
    for base in range(0, M, W):
        live = [(s, r, v) for r in range(base, base + W) for s, v in row_best(cand[r], W)]
        live.sort(key=lambda x: (-float(x[0]), x[1], x[2]))       # fp32 -> float64 is exact and order-preserving; -0 == +0
        n = min(len(live), W)
        ns.append(n)
        for k in range(W):
            r = base + k
            if n == 0:
                code[r] = int(low[r])
            else:
                s, a, v = live[k if k < n else 0]
                anc[r], code[r] = a, v
                if k < n:
                    sc[r] = s
    return anc, code, sc, np.asarray(ns), int((anc != np.arange(M)).any())


def logp_bounds(row, logp_bound):
    """tests/prior_constrained_reference.py `logp_bound` (passed in) at EVERY code of the fp32 row at once.  That bound is a part
    common to the row, ds (1 + ds) + 2 u ULP_LOG |L|, plus u |d_code| + u |lp_code|; at the arg-max d = 0 and lp = -L, so the common
    part is logp_bound(row, argmax) - u |L|.  A code of logit -inf has bound 0, as there."""
    r = np.asarray(row, dtype=np.float64)
    top = int(np.argmax(r))
    d = r - r[top]
    L = float(np.log(np.exp(d).sum()))
    common = logp_bound(r, top) - U_FP32 * abs(L)
    with np.errstate(invalid='ignore'):
        out = common + U_FP32 * np.abs(d) + U_FP32 * np.abs(d - L)
    return np.where(np.isneginf(r), 0.0, out)


def cand_bound(logp_bound, cand):
    """|cand_fp32 - cand_64| <= the logp chain's bound (tests/prior_constrained_reference.py `logp_bound`; the score is an exact
    fp32 input) + one rounding of the add, u |cand|."""
    return logp_bound + U_FP32 * abs(float(cand))


def beam_search(model, T, W, constraint=None, allowed=None, fp32=True):
    """One group's search over T columns.  model(prefix tuple) -> (V,) logits of the next column; constraint (T,) ints (< 0 free)
    or None; allowed: per column None or code ids.  -> (codes (W, T), scores (W,) float32, ancestors (T, W)), slot order, best
    first.  fp32: cand is rounded to float32 per step as the kernel does (lp stays float64: the toy models of the CPU tests have
    exactly representable log-probabilities or well separated sequences)."""
    rows = [() for _ in range(W)]
    score = start_scores(W, W)
    hist = np.zeros((T, W), dtype=np.int32)
    for t in range(T):
        cand, low = np.full((W, MAXV), NINF, dtype=F), np.zeros(W, dtype=np.int64)
        for b in range(W):
            logits = np.asarray(model(rows[b]), dtype=np.float64)
            codes = candidate_codes(len(logits), -1 if constraint is None else int(constraint[t]),
                                    None if allowed is None else allowed[t])
            low[b] = codes[0] if codes else 0
            c = cand64(score[b], logits, codes)
            cand[b] = c.astype(F) if fp32 else c
        anc, code, score, _, _ = select(cand, low, W)
        rows = [rows[anc[k]] + (int(code[k]),) for k in range(W)]
        hist[t] = anc
    return np.asarray(rows, dtype=np.int64).reshape(W, T), score, hist


# ---- the digit stages of a product prior ---------------------------------------------------------------------------------------
# A code is ncb digits, digit j in [0, K), code = sum_j digit_j K^j.  Stage j expands every row into the stage's candidate digits on
# the base the stage adds to (the hypotheses' scores at stage 0, the previous stage's scores afterwards) and `select` -- the same
# rule, V = K -- prunes to the group's W best (row, digit) pairs: the search is a beam over the DIGIT sequence.  After a stage the
# rows are in slot order, so a row's constraint and sets are those of the stack row it descends from (`anc_total`).
def forced_digit(forced, K, ncb, j):
    """Digit j of a forced code clamped to the K^ncb codes (< 0: free)."""
    if forced < 0:
        return -1
    return (min(int(forced), K ** ncb - 1) // K ** j) % K


def stage_state(M, ncb):
    """The stage state before stage 0 of a position (stage 0 overwrites everything it reads)."""
    return {'digits': np.zeros((M, ncb), dtype=np.int64), 'logp_acc': np.zeros(M, dtype=F), 'mass_acc': np.zeros(M, dtype=F),
            'anc_total': np.arange(M, dtype=np.int32)}


def stage_update(j, anc, digit, lp_sel, mass_rows, state):
    """What a stage's select writes per slot k, from the stage's selection (anc, digit -- `select`'s, rows in the CURRENT slot
    order), lp_sel (M,) float32 = lp(anc[k], digit[k]) and mass_rows (M,) float32, the rows' log-masses of this stage: the ancestor's
    digits with digit j appended; the accumulators, stage 0 stores, later stages add with ONE fp32 add in ascending stage order (the
    sampler's chain); the ancestor composed over the stages.  -> the new state."""
    anc = np.asarray(anc, dtype=np.int64)
    lp_sel, mass_sel = np.asarray(lp_sel, dtype=F), np.asarray(mass_rows, dtype=F)[anc]
    digits = state['digits'][anc].copy()
    digits[:, j] = digit
    if j == 0:
        return {'digits': digits, 'logp_acc': lp_sel.copy(), 'mass_acc': mass_sel.copy(), 'anc_total': anc.astype(np.int32)}
    with np.errstate(invalid='ignore'):
        return {'digits': digits, 'logp_acc': (state['logp_acc'][anc] + lp_sel).astype(F),
                'mass_acc': (state['mass_acc'][anc] + mass_sel).astype(F), 'anc_total': state['anc_total'][anc].copy()}


def merged_codes(digits, K):
    d = np.asarray(digits, dtype=np.int64)
    return (d * K ** np.arange(d.shape[1], dtype=np.int64)).sum(axis=1)


def product_beam_search(stage_model, T, W, K, ncb, constraint=None, allowed=None, fp32=True):
    """One group's search over T columns of ncb digit stages.  stage_model(prefix codes tuple, digits-so-far tuple) -> (K,) logits
    of the next digit; constraint (T,) merged codes (< 0 free) or None; allowed: per column None or a list of ncb digit-id lists
    (None: free).  -> (codes (W, T), scores (W,) float32, ancestors (T, W) composed over the stages, stage_ancestors (T, ncb, W))."""
    rows = [() for _ in range(W)]
    score = start_scores(W, W)
    hist, stage_hist = np.zeros((T, W), dtype=np.int32), np.zeros((T, ncb, W), dtype=np.int32)
    for t in range(T):
        state, base = stage_state(W, ncb), score
        for j in range(ncb):
            cand, low, lps = np.full((W, MAXV), NINF, dtype=F), np.zeros(W, dtype=np.int64), []
            for b in range(W):
                src = rows[int(state['anc_total'][b])] if j else rows[b]
                logits = np.asarray(stage_model(src, tuple(int(x) for x in state['digits'][b, :j])), dtype=np.float64)
                sets = None if allowed is None or allowed[t] is None else allowed[t][j]
                digs = candidate_codes(K, forced_digit(-1 if constraint is None else int(constraint[t]), K, ncb, j), sets)
                low[b] = digs[0] if digs else 0
                c = cand64(base[b], logits, digs)
                cand[b] = c.astype(F) if fp32 else c
                lps.append(lp64(logits))
            anc, dig, base, _, _ = select(cand, low, W)
            lp_sel = np.array([lps[anc[k]][dig[k]] for k in range(W)]).astype(F)
            state = stage_update(j, anc, dig, lp_sel, np.zeros(W, dtype=F), state)
            stage_hist[t, j] = anc
        score = base
        codes = merged_codes(state['digits'], K)
        rows = [rows[int(state['anc_total'][k])] + (int(codes[k]),) for k in range(W)]
        hist[t] = state['anc_total']
    return np.asarray(rows, dtype=np.int64).reshape(W, T), score, hist, stage_hist
