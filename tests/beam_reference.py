"""Beam search for decoder generation, stated once in numpy (kernel: csrc/beam.hip vqcpc_decode_beam_select; host:
decoders/generation.py `beam=W`).  TEST INFRASTRUCTURE: nothing here imports the package under test.  Anchored on the CPU by
tests/test_beam_reference_cpu.py; used by tests/test_beam_kernel_gpu.py and tests/test_generate_beam_gpu.py.

Rows come in groups of W consecutive rows (slots), the hypotheses of one user row.  At a position of voice c with V tokens:

  lp(b, v)     the row's log-softmax at token v over the voice's V logits (the kernel forms it in fp32 as the constrained sampler
               forms logp; here float64, compared within `cand_bound`)
  candidates   forced position (constraint >= 0): the one token, clamped to [0, V), exclusion and set ignored;
               free position: the tokens of [0, V) in the row's set that are not excluded; no set, or a set with no bit inside the
               vocabulary: the whole vocabulary                                                            (`candidate_tokens`)
  cand(b, v)   = score[b] + lp(b, v), ONE fp32 add; NaN counts as -inf; live means cand > -inf
  selection    per group the live candidates in the order cand descending, then row ascending, then token ascending (total);
               slot k < n (n = live candidates, at most W) gets the k-th: ancestor = its row, its token, score = cand;
               slots k >= n are dead: slot 0's ancestor and token, score -inf;
               n == 0: the identity, every row emits its own lowest candidate token (0 without one), score -inf      (`select`)
  start        score 0 for a group's first row, -inf for the others                                          (`start_scores`)

`select` is an exact function of the fp32 candidate scores: the kernel tests feed it the kernel's own `cand_out`, so ancestors,
tokens and scores are pinned with no near-tie exemption.  `beam_search` runs whole sequences on a caller-given model."""
import numpy as np

F = np.float32
U_FP32 = 2.0 ** -24
NINF = F(-np.inf)
MAXV = 256


def start_scores(M, W):
    s = np.full(M, NINF, dtype=F)
    s[0::W] = F(0.0)
    return s


def candidate_tokens(V, forced=-1, allowed=None, exclude=()):
    """-> the sorted candidate tokens of one row.  forced: the constraint's entry; allowed: None or an iterable of token ids (ids
    >= V are ignored, none below V: no restriction); exclude: token ids."""
    if forced >= 0:
        return [min(max(min(int(forced), MAXV), 0), V - 1)]
    inside = None if allowed is None else sorted({int(t) for t in allowed if 0 <= int(t) < V})
    if not inside:
        inside = list(range(V))
    ex = {int(t) for t in exclude}
    return [t for t in inside if t not in ex]


def lp64(row):
    """log-softmax of one voice's logits (V,) in float64 (NaN for a row of -inf, as the kernel's chain gives)."""
    r = np.asarray(row, dtype=np.float64)
    with np.errstate(invalid='ignore', divide='ignore'):
        d = r - r.max()
        return d - np.log(np.exp(d).sum())


def cand64(score, row, toks):
    """-> (MAXV,) float64: score + lp at the candidate tokens, -inf elsewhere and where the sum is NaN."""
    out = np.full(MAXV, -np.inf)
    lp = lp64(row)
    for t in toks:
        v = float(score) + lp[t]
        out[t] = -np.inf if np.isnan(v) else v
    return out


def select(cand, low, W):
    """cand (M, MAXV) float32, -inf for a non-candidate (and for a dead one); low (M,) the rows' lowest candidate tokens; groups of
    W rows -> (ancestors (M,) int32 stack row indices, tokens (M,) int64, score (M,) float32, n (G,) live slots, flag)."""
    cand = np.asarray(cand, dtype=F)
    M = cand.shape[0]
    assert M % W == 0 and cand.shape[1] == MAXV
    anc, tok, sc, ns = np.arange(M, dtype=np.int32), np.zeros(M, dtype=np.int64), np.full(M, NINF, dtype=F), []
    for base in range(0, M, W):
        live = [(cand[r, v], r, v) for r in range(base, base + W) for v in range(MAXV) if cand[r, v] > NINF]
        live.sort(key=lambda x: (-float(x[0]), x[1], x[2]))       # fp32 -> float64 is exact and order-preserving; -0 == +0
        n = min(len(live), W)
        ns.append(n)
        for k in range(W):
            r = base + k
            if n == 0:
                tok[r] = int(low[r])
            else:
                s, a, v = live[min(k, n - 1) if k < n else 0]
                anc[r], tok[r] = a, v
                if k < n:
                    sc[r] = s
    return anc, tok, sc, np.asarray(ns), int((anc != np.arange(M)).any())


def cand_bound(logp_bound, cand):
    """|cand_fp32 - cand_64| <= the logp chain's bound (tests/constrained_reference.py `logp_bound`; the score is an exact fp32
    input) + one rounding of the add, u |cand|."""
    return logp_bound + U_FP32 * abs(float(cand))


def beam_search(model, T, W, constraint=None, allowed=None, exclude=None, fp32=True):
    """One group's search over T positions.  model(prefix tuple) -> (V,) logits of the next position; constraint (T,) ints (< 0
    free) or None; allowed: per position None or token ids; exclude: per position token ids or None.  -> (tokens (W, T), scores (W,)
    float32, ancestors (T, W)), slot order, best first.  fp32: cand is rounded to float32 per step as the kernel does (lp stays
    float64: the toy models of the CPU tests have exactly representable log-probabilities or well separated sequences)."""
    rows = [() for _ in range(W)]
    score = start_scores(W, W)
    hist = np.zeros((T, W), dtype=np.int32)
    for t in range(T):
        cand, low = np.full((W, MAXV), NINF, dtype=F), np.zeros(W, dtype=np.int64)
        for b in range(W):
            logits = np.asarray(model(rows[b]), dtype=np.float64)
            toks = candidate_tokens(len(logits), -1 if constraint is None else int(constraint[t]),
                                    None if allowed is None else allowed[t], () if exclude is None or exclude[t] is None else exclude[t])
            low[b] = toks[0] if toks else 0
            c = cand64(score[b], logits, toks)
            cand[b] = c.astype(F) if fp32 else c
        anc, tok, score, _, _ = select(cand, low, W)
        rows = [rows[anc[k]] + (int(tok[k]),) for k in range(W)]
        hist[t] = anc
    return np.asarray(rows, dtype=np.int64).reshape(W, T), score, hist


def brute_force(model, T, constraint=None, allowed=None, exclude=None):
    """Every sequence the candidate rule admits with its float64 total log-probability, ranked: total descending, then the
    sequence ascending.  -> [(total, tokens tuple)]."""
    seqs = [(0.0, ())]
    for t in range(T):
        nxt = []
        for total, pre in seqs:
            logits = np.asarray(model(pre), dtype=np.float64)
            toks = candidate_tokens(len(logits), -1 if constraint is None else int(constraint[t]),
                                    None if allowed is None else allowed[t], () if exclude is None or exclude[t] is None else exclude[t])
            lp = lp64(logits)
            nxt += [(total + lp[v], pre + (v,)) for v in toks if lp[v] > -np.inf]
        seqs = nxt
    return sorted(seqs, key=lambda x: (-x[0], x[1]))


def follow_ancestors(tokens_by_pos, hist):
    """tokens_by_pos (T, M): the token slot k emitted at position t; hist (T, M) the recorded ancestors -> (M, T): every final row's
    sequence, read backwards from the last position (row r at position t descends from hist[t][r] at t - 1)."""
    T, M = hist.shape
    out = np.zeros((M, T), dtype=np.int64)
    for r in range(M):
        k = r
        for t in range(T - 1, -1, -1):
            out[r, t] = tokens_by_pos[t][k]
            k = int(hist[t][k])
    return out
