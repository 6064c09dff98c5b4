"""Float64 reference of the prior's masked sampler (vqcpc_prior_sample_masked, vqcpc_prior_sample_product_masked; csrc/prior.hip,
csrc/product_codes.hip) and the slow forward-per-code generation loop under per-column code sets.  TEST INFRASTRUCTURE: nothing
here imports the package under test (the slow loop takes the prior as an argument).  Anchored on the CPU by
tests/test_prior_masked_reference_cpu.py; used by tests/test_prior_sample_masked_gpu.py, tests/test_prior_masked_gpu.py and
tests/test_prior_particles_gpu.py.

  effective_set       only entries [0, V) count, a set without any of them restricts nothing
  pack_ref            bool (..., V) -> uint32 words, numpy.packbits with little bit order
  masked_step_ref     one step: the set -> temperature (multiplied) -> top-k -> top-p -> the draw, forced codes win; logp under
                      the unfiltered row, logmass of the set
  logmass_ref         log of the share of softmax(row) that lies on the allowed codes
  logmass_bound       the fp32 error bound of the kernel's chain (m_a - m) + log(s_a) - log(s), as a function of V
  product_chain_ref   the ncb stages of a product code: digit by digit, per-stage keys, summed logp and logmass
  masked_greedy_loop  one full `forward` per code on the reference's window, argmax over the allowed codes where free
"""
import numpy as np
import torch

from constrained_reference import ULP_EXP, ULP_LOG, draw_ref, logp_ref
from decode_reference import U_FP32, filter_ref, splitmix64
from prior_constrained_reference import SUM_CHAIN

STAGE_KEY = 0xA0761D6478BD642F          # the draw key of stage j >= 1: splitmix64(seed ^ j * STAGE_KEY) (include/vqcpc.h)


def effective_set(allowed, V):
    """allowed (>= V,) bool -> (V,) bool: only entries [0, V) count, and a set without any of them restricts nothing."""
    a = torch.as_tensor(np.asarray(allowed), dtype=torch.bool)[:V].clone()
    return a if bool(a.any()) else torch.ones(V, dtype=torch.bool)


def pack_ref(allowed):
    """bool (..., V) -> uint32 (..., ceil(V / 32)): bit i & 31 of word i >> 5 is entry i -- numpy.packbits in little bit order on
    the entries padded with False to a multiple of 32, four bytes per little-endian word."""
    a = np.asarray(allowed, dtype=bool)
    V = a.shape[-1]
    words = (V + 31) // 32
    pad = np.zeros(a.shape[:-1] + (words * 32,), dtype=bool)
    pad[..., :V] = a
    by = np.packbits(pad, axis=-1, bitorder='little')                      # (..., words * 4) bytes
    return np.ascontiguousarray(by).view('<u4').reshape(a.shape[:-1] + (words,))


def logmass_ref(row, allowed):
    """log(sum_{i allowed} softmax(row)_i) in float64, each log-sum-exp with its own maximum subtracted; -inf when every allowed
    logit is -inf.  `allowed` as `effective_set` reads it."""
    r = torch.as_tensor(row, dtype=torch.float64)
    a = effective_set(allowed, r.numel())
    m, ra = r.max(), r[a]
    ma = ra.max()
    if float(ma) == -float('inf'):
        return -float('inf')
    return float((ma - m) + torch.log(torch.exp(ra - ma).sum()) - torch.log(torch.exp(r - m).sum()))


def masked_step_ref(logits, temperature, top_k, top_p, seeds, pos, constraint, allowed):
    """logits (M, V); seeds (M,) int64; constraint (M,) int64 or None; allowed (M, >= V) bool or None, the sets of this column.
    The prior's temperature sense (multiplied).  -> (codes (M,) int64, probs (M, V) float64 -- the distribution filtered on the
    allowed set --, logp (M,) float64 under the UNFILTERED row, logmass (M,) float64).  A forced code wins over its set."""
    logits = torch.as_tensor(logits, dtype=torch.float64)
    M, V = logits.shape
    codes = torch.zeros(M, dtype=torch.int64)
    probs = torch.zeros(M, V, dtype=torch.float64)
    logp = torch.zeros(M, dtype=torch.float64)
    logmass = torch.zeros(M, dtype=torch.float64)
    for b in range(M):
        a = torch.ones(V, dtype=torch.bool) if allowed is None else effective_set(allowed[b], V)
        probs[b] = filter_ref(logits[b], temperature, top_k, top_p, torch.nonzero(~a).flatten().tolist(), multiply=True)
        f = -1 if constraint is None else int(constraint[b])
        codes[b] = min(max(f, 0), V - 1) if f >= 0 else draw_ref(probs[b].numpy(), int(seeds[b]), int(pos))
        logp[b] = logp_ref(logits[b], codes[b])
        logmass[b] = logmass_ref(logits[b], a)
    return codes, probs, logp, logmass


def _sum_error(d, p):
    """Relative error bound of the fp32 exp-sum of the differences d (<= 0, the maximum's is 0) whose float64 softmax is p: the
    `ds / s` of prior_constrained_reference.logp_bound (a thread's 16 codes ascending from 0.0f, six butterfly levels, the four
    waves' totals pairwise: gamma_23).  A masked code enters the kernel's sum as an exact 0 at its own place, so the chain of the
    allowed codes is the row's with fewer non-zero terms: the same bound."""
    u = U_FP32
    g = SUM_CHAIN * u / (1.0 - SUM_CHAIN * u)
    da = d.abs().masked_fill(p == 0, 0.0)                                  # -inf entries contribute exactly 0
    rel_terms = float((p * (u * da * torch.exp(u * da) + 2 * u * ULP_EXP)).sum())
    return rel_terms * (1.0 + g) + g + d.numel() * 2.0 ** -126


def logmass_bound(row, allowed):
    """Bound on |logmass_fp32 - logmass_64| for the kernel's chain on the fp32 row `row` (V <= 4096 entries, -inf allowed) and the
    set `allowed`, derived as prior_constrained_reference.logp_bound is (u = 2^-24, gamma_23 for the additions on the path of any
    term, exp and log within 3 ulp).  V enters through the number of terms of the two sums (their weights p_i sum to 1, so the
    bound grows with V only through the V 2^-126 underflow term and through |L| <= log V):

      m, m_a   = max over the row / over the allowed codes       exact
      s        = sum_i expf(fl(row_i - m))                       relative error ds   (logp_bound's ds / s; s >= 1)
      s_a      = sum_{i allowed} expf(fl(row_i - m_a))           relative error ds_a (the same bound on the allowed sub-row; s_a >= 1)
      L, L_a   = logf(s), logf(s_a)                              |error| <= ds (1 + ds) + 2 u ULP_LOG |L|, likewise for L_a
      t0       = fl(m_a - m)                                     |error| <= u |m_a - m|
      t1       = fl(t0 + L_a)                                    + u |t1|
      logmass  = fl(t1 - L)                                      + u |logmass|

    The full set has m_a = m and s_a = s bit for bit, so the kernel gives exactly 0 and so does float64: bound 0.  An allowed set
    of -inf logits gives -inf exactly: bound 0."""
    r = torch.as_tensor(row, dtype=torch.float64)
    a = effective_set(allowed, r.numel())
    if bool(a.all()) or float(r[a].max()) == -float('inf'):
        return 0.0
    u = U_FP32
    ra = r[a]
    d, da = r - r.max(), ra - ra.max()
    ds, dsa = _sum_error(d, torch.softmax(r, dim=-1)), _sum_error(da, torch.softmax(ra, dim=-1))
    L, La = float(torch.log(torch.exp(d).sum())), float(torch.log(torch.exp(da).sum()))
    t0 = float(ra.max() - r.max())
    t1 = t0 + La
    return (ds * (1.0 + ds) + 2 * u * ULP_LOG * abs(L)) + (dsa * (1.0 + dsa) + 2 * u * ULP_LOG * abs(La)) + \
        u * abs(t0) + u * abs(t1) + u * abs(t1 - L)


def _block_sum32(v):
    """The kernel's exp-sum of 4096 fp32 terms: thread t adds its 16 codes in ascending order to 0.0f, the xor butterfly over the
    64 lanes of a wave (offsets 32 .. 1), then (w0 + w1) + (w2 + w3)."""
    per = np.zeros(256, dtype=np.float32)
    for t in range(16):
        per = per + v.reshape(256, 16)[:, t]
    w = per.reshape(4, 64)
    for o in (32, 16, 8, 4, 2, 1):
        w = w + w[:, np.arange(64) ^ o]
    return np.float32(np.float32(w[0, 0] + w[1, 0]) + np.float32(w[2, 0] + w[3, 0]))


def logmass_chain32(row, allowed):
    """The kernel's chain in numpy fp32, summation order included (numpy's expf / logf stand in for the device's: the bits may
    differ in the last places, the error model is the same).  For the CPU anchor of `logmass_bound`."""
    r = np.full(4096, -np.inf, dtype=np.float32)
    V = len(row)
    r[:V] = np.asarray(row, dtype=np.float32)
    a = np.zeros(4096, dtype=bool)
    a[:V] = effective_set(allowed, V).numpy()
    ra = np.where(a, r, np.float32(-np.inf)).astype(np.float32)
    m, ma = r.max(), ra.max()
    if ma == -np.inf:
        return np.float32(-np.inf)
    with np.errstate(invalid='ignore'):
        s = _block_sum32(np.where(r > -np.inf, np.exp((r - m).astype(np.float32)), np.float32(0)).astype(np.float32))
        sa = _block_sum32(np.where(ra > -np.inf, np.exp((ra - ma).astype(np.float32)), np.float32(0)).astype(np.float32))
    return np.float32(np.float32(np.float32(ma - m) + np.log(sa)) - np.log(s))


def stage_seed(seed, stage):
    """The draw key of stage `stage` for the row's int64 seed, as a signed int64."""
    if stage == 0:
        return int(seed)
    z = splitmix64((int(seed) & ((1 << 64) - 1)) ^ ((stage * STAGE_KEY) & ((1 << 64) - 1)))
    return z - (1 << 64) if z >= 1 << 63 else z


def product_chain_ref(stage_logits, temperature, top_k, top_p, seeds, pos, constraint, allowed):
    """The ncb stages of one position.  stage_logits (ncb, M, K) -- here GIVEN per stage (in the model stage j's row depends on the
    digits before it; the kernel tests feed rows directly); seeds (M,) int64; constraint (M,) merged codes or None (>= 0 forces
    every digit, clamped to [0, K**ncb)); allowed (M, ncb, >= K) bool digit sets or None.
    -> (codes (M,) int64 merged, digits (ncb, M), logp (M,) float64 = the sum of the stages' log-probabilities, logmass (M,)
    float64 = the sum of the stages' conditional log-masses, both in ascending stage order)."""
    stage_logits = torch.as_tensor(stage_logits, dtype=torch.float64)
    ncb, M, K = stage_logits.shape
    dig = np.zeros((ncb, M), dtype=np.int64)
    logp, logmass = np.zeros(M), np.zeros(M)
    for j in range(ncb):
        forced = None
        if constraint is not None:
            c = torch.as_tensor(constraint, dtype=torch.int64)
            forced = torch.where(c >= 0, (c.clamp(max=K ** ncb - 1) // K ** j) % K, torch.full_like(c, -1))
        sj = torch.tensor([stage_seed(int(s), j) for s in seeds], dtype=torch.int64)
        codes, _, lp, lm = masked_step_ref(stage_logits[j], temperature, top_k, top_p, sj, pos, forced,
                                           None if allowed is None else torch.as_tensor(np.asarray(allowed))[:, j])
        dig[j] = codes.numpy()
        logp, logmass = logp + lp.numpy(), logmass + lm.numpy()
    codes = sum(dig[j] * K ** j for j in range(ncb))
    return torch.as_tensor(codes), dig, torch.as_tensor(logp), torch.as_tensor(logmass)


@torch.no_grad()
def masked_greedy_loop(prior, constraint, allowed):
    """The slow generation of a MERGED prior: ONE full `prior.forward` per code (the reference's loop, prior_relative.py:315-353)
    on the reference's window -- codes [0, N) for e < N, read at position e; codes [e - N + 1, e] afterwards, read at the last
    position --, the argmax over the ALLOWED codes of the position's logits where constraint (B, num_tokens) is < 0, its code
    elsewhere.  allowed: bool (B, num_tokens, V).
    -> (codes (B, num_tokens) int64, the smallest top-1 / top-2 logit gap over the allowed codes of the FREE columns that have at
    least two, the rms of every logit the loop read, mass (B, num_tokens) float64: the log of the allowed share of
    softmax(logits) at every column, given the codes before it, rows (B, num_tokens, V) float64: the logits each code was
    chosen from)."""
    prior.eval()
    N = prior.num_tokens
    B, nt = constraint.shape
    dev = prior.sos.device
    seq = torch.zeros(B, nt, dtype=torch.int64, device=dev)
    mass = torch.zeros(B, nt, dtype=torch.float64)
    gap, sq, n, rows = float('inf'), 0.0, 0, []
    for e in range(nt):
        w, p = (0, e) if e < N else (e - N + 1, N - 1)
        lg = prior.forward(seq[:, w:w + N].contiguous())['weights_per_category'][0][:, p].double()
        rows.append(lg.cpu())
        sq, n = sq + float(lg.pow(2).sum()), n + lg.numel()
        a = allowed[:, e].to(dev)
        open_lg = lg.masked_fill(~a, -float('inf'))
        mass[:, e] = (torch.logsumexp(open_lg, dim=-1) - torch.logsumexp(lg, dim=-1)).cpu()
        f = constraint[:, e].to(dev)
        two = (f < 0) & (a.sum(-1) >= 2)
        if bool(two.any()):
            top2 = torch.topk(open_lg[two], 2, dim=-1)[0]
            gap = min(gap, float((top2[:, 0] - top2[:, 1]).min()))
        seq[:, e] = torch.where(f < 0, open_lg.argmax(dim=-1), f)
    return seq, gap, (sq / max(n, 1)) ** 0.5, mass, torch.stack(rows, dim=1)
