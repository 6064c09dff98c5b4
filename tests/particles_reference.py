"""The particle filter of constrained generation, stated once in numpy (kernels: csrc/particles.hip; host:
decoders/generation.py `_resample`).  Everything the kernels compute in fp32 is restated here with numpy float32 scalars, one
rounding per operation, members in ascending order -- sums of fp32 numbers done that way have the same bits on the device (the
kernel file is compiled without FMA contraction, fp32 division is correctly rounded) -- except exp and log, whose last bits
belong to the library: the weights are therefore compared within `wn_bound`, while the ANCESTORS are an exact function of the
weights the kernel itself stored (`systematic_ancestors`), with no near-tie exemption.

Rows come in groups of P consecutive rows.  After the U steps of a code with chorale index c:
  lw[b] += logp[b, q] where constraint[b, q] >= 0, else += logmass[b, q] where sets are in use, for q ascending over the code's
  columns [c * U, (c + 1) * U)  (U = the code's positions, events x voices);  NaN counts as -inf;
  per group: mx = max lw, w = exp(lw - mx), s = sum w, wn = w / s, ess = 1 / sum wn^2, inc = (mx + log s) - log P;
  all members -inf: wn uniform, never resampled, evidence -inf;
  resampled iff forced or ess < threshold * P:  u = uniform(seed of the group's first row, c); the ancestor of slot k is the first
  member whose running sum of wn exceeds (u + k) / P, clamped to the last; evidence += inc; lw = 0."""
import math

import numpy as np

F = np.float32
EPS = 2.0 ** -24                          # the unit roundoff of fp32
MASK64 = (1 << 64) - 1
SEED_MUL = 0x8CB92BA72F3D8DD7             # vqcpc_particle_resample's key constant (odd)


def splitmix64(z):
    z = (z + 0x9E3779B97F4A7C15) & MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    return z ^ (z >> 31)


def uniform(seed, c):
    """u in [0, 1), a multiple of 2^-24: (splitmix64(seed ^ (c + 1) * K) >> 40) * 2^-24, seed taken modulo 2^64."""
    key = (int(seed) & MASK64) ^ (((int(c) + 1) * SEED_MUL) & MASK64)
    return F((splitmix64(key) >> 40) * 2.0 ** -24)


def update_lw(lw, c, U, constraint=None, logp=None, logmass=None):
    """lw (M,) float32 -> the log-weights after code c, fp32, one add per addend in ascending column order.  constraint (M, w)
    int64, logp / logmass (M, w) float32, any of them None; columns past a buffer's width add nothing."""
    out = np.array(lw, dtype=F)
    for b in range(out.shape[0]):
        l = out[b]
        for q in range(c * U, (c + 1) * U):
            if constraint is not None and q < constraint.shape[1] and constraint[b, q] >= 0:
                if logp is not None and q < logp.shape[1]:
                    l = F(l + logp[b, q])
            elif logmass is not None and q < logmass.shape[1]:
                l = F(l + logmass[b, q])
        out[b] = F(-np.inf) if np.isnan(l) else l
    return out


def group_weights(lw):
    """One group's lw (P,) float32 -> (wn (P,) float32, ess, inc, dead) as the kernel's operation chain gives them (exp and log
    are numpy's float32 ones: equal to the device's within `wn_bound` / `inc_bound` only)."""
    lw = np.asarray(lw, dtype=F)
    P = lw.shape[0]
    mx = lw.max()
    if not mx > -np.inf:
        return np.full(P, F(1.0) / F(P), dtype=F), F(1.0) / sum_sq(np.full(P, F(1.0) / F(P), dtype=F)), F(-np.inf), True
    with np.errstate(under='ignore'):
        w = np.array([np.exp(F(l - mx)) if l > -np.inf else F(0.0) for l in lw], dtype=F)
    s = F(0.0)
    for v in w:
        s = F(s + v)
    wn = np.array([F(v / s) for v in w], dtype=F)
    inc = F(F(mx + np.log(s)) - np.log(F(P)))
    return wn, F(1.0) / sum_sq(wn), inc, False


def sum_sq(wn):
    ss = F(0.0)
    for v in wn:
        ss = F(ss + F(v * v))
    return ss


def ess_of(wn):
    """The effective sample size of STORED weights, exactly as the kernel computes it from them."""
    with np.errstate(under='ignore'):
        return F(F(1.0) / sum_sq(np.asarray(wn, dtype=F)))


def group_weights64(lw):
    """float64 values of the same quantities from the fp32 lw: (wn, ess, inc, dmax), dmax = the largest |lw - mx| of a member
    whose weight is not flushed (it sets the error that the subtraction's rounding leaves in the exponent)."""
    lw = np.asarray(lw, dtype=np.float64)
    P = lw.shape[0]
    mx = lw.max()
    if not mx > -np.inf:
        return np.full(P, 1.0 / P), float(P), -np.inf, 0.0
    d = lw - mx
    w = np.where(np.isfinite(d), np.exp(np.where(np.isfinite(d), d, 0.0)), 0.0)
    s = w.sum()
    wn = w / s
    live = np.isfinite(d) & (d > -104.0)
    return wn, 1.0 / (wn ** 2).sum(), mx + math.log(s) - math.log(P), float(np.abs(d[live]).max())


def rel_w(dmax):
    """Relative error of one weight: the subtraction leaves |d| * EPS in the exponent, exp is taken to be within 2 ulp."""
    return (dmax + 4.0) * EPS


def wn_bound(wn64, dmax, P):
    """|wn - wn64| <=: w's relative error, the sum's ((P - 1) sequential adds of non-negative terms, plus the terms' own error),
    the division; 2^-126 covers weights in the subnormal range, which may be flushed."""
    return wn64 * (2.0 * rel_w(dmax) + (P + 1) * EPS) + 2.0 ** -126


def ess_bound(ess64, dmax, P):
    """ess = 1 / sum wn^2: twice wn's relative error, the squares, the P - 1 adds and the division."""
    return ess64 * (2.0 * (2.0 * rel_w(dmax) + (P + 1) * EPS) + (P + 3) * EPS)


def inc_bound(mx, inc64, dmax, P):
    """inc = (mx + log s) - log P with 1 <= s <= P: the relative error of s enters log s absolutely; the two logs are within
    2 ulp of values of at most log P; two adds of results no larger than |mx| + 2 log P."""
    logp = math.log(P)
    return rel_w(dmax) + (P - 1) * EPS + 8.0 * EPS * logp + 2.0 * EPS * (abs(mx) + 2.0 * logp + abs(inc64))


def systematic_ancestors(wn, u):
    """Stored wn (P,) float32, u float32 -> ancestors (P,) of member indices: slot k gets the first member j whose running
    fp32 sum of wn (ascending, sequential adds) exceeds (u + k) / P, else the last member."""
    wn = np.asarray(wn, dtype=F)
    P = wn.shape[0]
    cum = np.empty(P, dtype=F)
    run = F(0.0)
    for j in range(P):
        run = F(run + wn[j])
        cum[j] = run
    out = np.empty(P, dtype=np.int32)
    for k in range(P):
        target = F(F(F(u) + F(k)) / F(P))
        hit = np.nonzero(cum > target)[0]
        out[k] = hit[0] if hit.size else P - 1
    return out


def decide(ess, threshold, P, force, dead):
    """Whether a group with the STORED fp32 ess resamples."""
    return (not dead) and (bool(force) or bool(F(ess) < F(F(threshold) * F(P))))


def resample(lw, evidence, seeds, c, U, P, threshold, force=False, constraint=None, logp=None, logmass=None, wn=None, ess=None):
    """One launch of vqcpc_particle_resample on M = G * P rows.  wn / ess: the kernel's own stored values (then the decision
    and the ancestors are functions of those, as the tests require); None: the reference's fp32 chain.
    -> dict(lw, evidence, pending, ancestors (row indices), wn, ess, flag, resampled (G,) bool, lw_updated)."""
    lw1 = update_lw(lw, c, U, constraint, logp, logmass)
    M = lw1.shape[0]
    G = M // P
    out = dict(lw=lw1.copy(), evidence=np.array(evidence, dtype=F), pending=np.empty(G, dtype=F),
               ancestors=np.arange(M, dtype=np.int32), wn=np.empty(M, dtype=F), ess=np.empty(G, dtype=F),
               resampled=np.zeros(G, dtype=bool), lw_updated=lw1)
    for g in range(G):
        rows = slice(g * P, (g + 1) * P)
        wn_g, ess_g, inc, dead = group_weights(lw1[rows])
        if wn is not None:
            wn_g, ess_g = np.asarray(wn[rows], dtype=F), F(ess[g])
        out['wn'][rows], out['ess'][g], out['pending'][g] = wn_g, ess_g, inc
        if dead:
            out['evidence'][g] = F(-np.inf)
        if decide(ess_g, threshold, P, force, dead):
            out['resampled'][g] = True
            out['ancestors'][rows] = g * P + systematic_ancestors(wn_g, uniform(seeds[g * P], c))
            out['evidence'][g] = F(out['evidence'][g] + inc)
            out['lw'][rows] = F(0.0)
    out['flag'] = int((out['ancestors'] != np.arange(M)).any())
    return out


def permute_rows(buf, ancestors, cols):
    """buf (..., M, ld): rows follow `ancestors` (M,) on columns [0, cols), everything else untouched -> a new array."""
    out = buf.copy()
    out[..., :, :cols] = buf[..., ancestors, :cols]
    return out


def copies(ancestors, P):
    """How often every member of one group appears among its ancestors (member indices)."""
    return np.bincount(np.asarray(ancestors), minlength=P)
