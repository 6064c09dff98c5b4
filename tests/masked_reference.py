"""Float64 reference of the masked sampler (vqcpc_decode_sample_masked, csrc/decode.hip) and the slow forward-per-token
generation loop under per-position token sets.  TEST INFRASTRUCTURE: nothing here imports the package under test (the slow
loop takes the decoder as an argument).  Anchored on the CPU by tests/test_masked_reference_cpu.py; used by
tests/test_decode_sample_masked_gpu.py and tests/test_generate_masked_gpu.py.

  masked_step_ref     one step for one voice: `filter_ref` with exclusion = global exclusion U not-allowed, then the draw of
                      constrained_reference (forced tokens win), logp under the unfiltered row, logmass of the allowed set
  logmass_ref         log of the share of softmax(row) that lies on the allowed tokens
  logmass_bound       the fp32 error bound of the kernel's chain (m_a - m) + log(s_a) - log(s)
  masked_greedy_loop  one full `forward` per token, argmax over the allowed tokens, the constraint's token where forced
"""
import torch

from constrained_reference import ULP_EXP, ULP_LOG, draw_ref, logp_ref
from decode_reference import U_FP32, filter_ref


def effective_set(allowed, V):
    """allowed (>= V,) bool -> (V,) bool: only entries [0, V) count, and a set without any of them restricts nothing."""
    a = torch.as_tensor(allowed, dtype=torch.bool)[:V].clone()
    return a if bool(a.any()) else torch.ones(V, dtype=torch.bool)


def logmass_ref(row, allowed):
    """log(sum_{i allowed} softmax(row)_i) in float64, each log-sum-exp with its own maximum subtracted; -inf when every
    allowed logit is -inf.  `allowed` as `effective_set` reads it."""
    r = torch.as_tensor(row, dtype=torch.float64)
    a = effective_set(allowed, r.numel())
    m, ra = r.max(), r[a]
    ma = ra.max()
    if float(ma) == -float('inf'):
        return -float('inf')
    return float((ma - m) + torch.log(torch.exp(ra - ma).sum()) - torch.log(torch.exp(r - m).sum()))


def masked_step_ref(logits, temperature, top_k, top_p, exclude, seeds, pos, constraint, allowed):
    """logits (M, V) of the position's voice; seeds (M,) int64; constraint (M,) int64 or None; allowed (M, >= V) bool or None,
    the sets of this position.  -> (tokens (M,) int64, probs (M, V) float64 -- the distribution filtered on the allowed set --,
    logp (M,) float64 under the UNFILTERED row, logmass (M,) float64)."""
    logits = torch.as_tensor(logits, dtype=torch.float64)
    M, V = logits.shape
    tokens = torch.zeros(M, dtype=torch.int64)
    probs = torch.zeros(M, V, dtype=torch.float64)
    logp = torch.zeros(M, dtype=torch.float64)
    logmass = torch.zeros(M, dtype=torch.float64)
    for b in range(M):
        a = torch.ones(V, dtype=torch.bool) if allowed is None else effective_set(allowed[b], V)
        closed = sorted(set(int(t) for t in exclude if int(t) < V) | set(torch.nonzero(~a).flatten().tolist()))
        probs[b] = filter_ref(logits[b], temperature, top_k, top_p, closed)
        f = -1 if constraint is None else int(constraint[b])
        tokens[b] = min(max(f, 0), V - 1) if f >= 0 else draw_ref(probs[b].numpy(), int(seeds[b]), int(pos))
        logp[b] = logp_ref(logits[b], tokens[b])
        logmass[b] = logmass_ref(logits[b], a)
    return tokens, probs, logp, logmass


def _sum_error(d, p):
    """Relative error bound of the fp32 exp-sum of the differences d (<= 0, the maximum's is 0) whose float64 softmax is p: the
    `ds / s` of constrained_reference.logp_bound."""
    u = U_FP32
    g9 = 9 * u / (1.0 - 9 * u)
    da = d.abs().masked_fill(p == 0, 0.0)                                  # -inf entries contribute exactly 0
    rel_terms = float((p * (u * da * torch.exp(u * da) + 2 * u * ULP_EXP)).sum())
    return rel_terms * (1.0 + g9) + g9 + d.numel() * 2.0 ** -126


def logmass_bound(row, allowed):
    """Bound on |logmass_fp32 - logmass_64| for the kernel's chain on the fp32 row `row` (V <= 256 entries, -inf allowed) and
    the set `allowed`, derived as constrained_reference.logp_bound is (u = 2^-24, gamma_9 for the nine additions on the path
    of any term of a lane-serial sum of four and a six-level butterfly, exp and log within 3 ulp):

      m, m_a   = max over the row / over the allowed tokens      exact
      s        = sum_i expf(fl(row_i - m))                       relative error ds   (logp_bound's ds / s; s >= 1)
      s_a      = sum_{i allowed} expf(fl(row_i - m_a))           relative error ds_a (the same bound on the allowed sub-row; s_a >= 1)
      L, L_a   = logf(s), logf(s_a)                              |error| <= ds (1 + ds) + 2 u ULP_LOG |L|, likewise for L_a
      t0       = fl(m_a - m)                                     |error| <= u |m_a - m|
      t1       = fl(t0 + L_a)                                    + u |t1|
      logmass  = fl(t1 - L)                                      + u |logmass|

    three subtractions / additions of the final form, each rounding once.  The full set has m_a = m and s_a = s bit for bit, so
    the kernel gives exactly 0 and so does float64: bound 0.  An allowed set of -inf logits gives -inf exactly: bound 0."""
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


@torch.no_grad()
def masked_greedy_loop(dec, codes, constraint, allowed):
    """The slow generation: ONE full `dec.forward(codes, x)` per token, the argmax over the ALLOWED tokens of the position's
    logits where constraint (B, events, channels) is < 0, its token elsewhere.  allowed: bool (B, events, channels, vmax),
    read through `effective_set`'s rule (entries past the voice's vocabulary ignored).  -> (tokens (B, events, channels) int64,
    the smallest top-1 / top-2 logit gap over the allowed tokens of the FREE positions that have at least two, the rms of
    every logit the loop read, mass (B, events, channels) float64: the log of the allowed share of softmax(logits) at every
    position, given the tokens before it)."""
    dec.eval()
    B, events, nc = constraint.shape
    dev = codes.device
    x = torch.zeros(B, events, nc, dtype=torch.int64, device=dev)
    mass = torch.zeros(B, events, nc, dtype=torch.float64)
    gap, sq, n = float('inf'), 0.0, 0
    for t in range(events * nc):
        e, c = divmod(t, nc)
        lg = dec.forward(codes, x)['weights_per_category'][c][:, e].double()
        V = lg.shape[1]
        sq, n = sq + float(lg.pow(2).sum()), n + lg.numel()
        a = torch.stack([effective_set(allowed[b, e, c].cpu(), V) for b in range(B)]).to(dev)
        open_lg = lg.masked_fill(~a, -float('inf'))
        mass[:, e, c] = (torch.logsumexp(open_lg, dim=-1) - torch.logsumexp(lg, dim=-1)).cpu()
        f = constraint[:, e, c].to(dev)
        two = (f < 0) & (a.sum(-1) >= 2)
        if bool(two.any()):
            top2 = torch.topk(open_lg[two], 2, dim=-1)[0]
            gap = min(gap, float((top2[:, 0] - top2[:, 1]).min()))
        x[:, e, c] = torch.where(f < 0, open_lg.argmax(dim=-1), f)
    return x, gap, (sq / max(n, 1)) ** 0.5, mass
