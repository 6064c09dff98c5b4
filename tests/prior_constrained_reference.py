"""Float64 reference of the prior's constrained sampler (vqcpc_prior_sample_constrained, csrc/prior.hip) and the slow
forward-per-code generation loop with forcing.  TEST INFRASTRUCTURE: nothing here imports the package under test (the slow
loop takes the prior as an argument).  Anchored on the CPU by tests/test_prior_constrained_reference_cpu.py; used by
tests/test_prior_sample_constrained_gpu.py and tests/test_prior_constrained_gpu.py.

  prior_constrained_step_ref   one step: forced codes where the constraint holds one, the inverse-CDF draw of the filtered row
                               elsewhere, and the emitted code's log-probability under the UNFILTERED row
  logp_bound                   the fp32 error bound of the kernel's max / exp / sum / log chain
  forced_greedy_loop           one full `forward` per code on the reference's window, argmax where free, the constraint's code
                               where forced
"""
import torch

from constrained_reference import ULP_EXP, ULP_LOG, draw_ref, logp_ref
from decode_reference import U_FP32, filter_ref

# thread t sums its 16 codes in ascending order from 0.0f (the first addition is exact: 15 roundings), the wave butterfly has
# six levels, the four waves' totals are added pairwise (two levels)
SUM_CHAIN = 15 + 6 + 2


def prior_constrained_step_ref(logits, temperature, top_k, top_p, seeds, pos, constraint):
    """logits (M, V); seeds (M,) int64; constraint (M,) int64 or None, the constraint's column of this position.  The prior's
    temperature sense: the logits are MULTIPLIED by it.  -> (codes (M,) int64, probs (M, V) float64 -- the FILTERED
    distribution, whatever is forced --, logp (M,) float64 -- log_softmax of the UNFILTERED row (temperature 1) at the emitted
    code).  A forced code is clamped to [0, V); a free one is keyed by (seed, pos)."""
    logits = torch.as_tensor(logits, dtype=torch.float64)
    M, V = logits.shape
    codes = torch.zeros(M, dtype=torch.int64)
    probs = torch.zeros(M, V, dtype=torch.float64)
    logp = torch.zeros(M, dtype=torch.float64)
    for b in range(M):
        probs[b] = filter_ref(logits[b], temperature, top_k, top_p, multiply=True)
        f = -1 if constraint is None else int(constraint[b])
        codes[b] = min(max(f, 0), V - 1) if f >= 0 else draw_ref(probs[b].numpy(), int(seeds[b]), int(pos))
        logp[b] = logp_ref(logits[b], codes[b])
    return codes, probs, logp


def logp_bound(row, code):
    """Bound on |logp_fp32 - logp_64| for the kernel's chain on the fp32 row `row` (V <= 4096 entries, -inf allowed) at code
    `code`, u = 2^-24, gamma_n = n u / (1 - n u) (Higham, Accuracy and Stability of Numerical Algorithms, lemma 3.1):

      m      = max_i row_i                              exact (a maximum rounds nothing)
      d_i    = fl(row_i - m)                            |error| <= u |d_i|
      e_i    = expf(d_i)                                relative error <= u |d_i| e^{u |d_i|} (the argument's error) + 2 u ULP_EXP,
                                                        plus an absolute 2^-126 where the result is subnormal or flushed to zero
      s      = sum_i e_i                                thread t adds its codes 16 t .. 16 t + 15 in ascending order to 0.0f (the
                                                        first addition is exact: 15 roundings), six butterfly levels over the
                                                        wave's 64 lanes, then (w0 + w1) + (w2 + w3) over the four waves: at most
                                                        15 + 6 + 2 = 23 additions on the path of any term, all terms >= 0:
                                                        relative gamma_23
      L      = logf(s)                                  |error| <= |ds| / s (1 + |ds| / s) + 2 u ULP_LOG |L|;  s >= 1 as e_max = 1
      logp   = fl(d_code - L)                           + u |d_code| (d_code's own rounding) + u |logp| (the last subtraction)

    with ds / s <= sum_i p_i (u |d_i| e^{u |d_i|} + 2 u ULP_EXP) (1 + gamma_23) + gamma_23 + V 2^-126, p = softmax(row).  The
    result is stored as fp32: the last term covers that rounding.  A forced code of logit -inf has logp = -inf exactly: bound
    0."""
    r = torch.as_tensor(row, dtype=torch.float64)
    V = r.numel()
    if float(r[int(code)]) == -float('inf'):
        return 0.0
    u = U_FP32
    g = SUM_CHAIN * u / (1.0 - SUM_CHAIN * u)
    d = r - r.max()
    p = torch.softmax(r, dim=-1)
    da = d.abs().masked_fill(p == 0, 0.0)                                  # -inf entries contribute exactly 0
    rel_terms = float((p * (u * da * torch.exp(u * da) + 2 * u * ULP_EXP)).sum())
    ds = rel_terms * (1.0 + g) + g + V * 2.0 ** -126
    L = float(torch.log(torch.exp(d).sum()))
    lp = float(d[int(code)]) - L
    return ds * (1.0 + ds) + 2 * u * ULP_LOG * abs(L) + u * abs(float(d[int(code)])) + u * abs(lp)


@torch.no_grad()
def forced_greedy_loop(prior, constraint):
    """The slow generation: ONE full `prior.forward` per code (the reference's loop, prior_relative.py:315-353) on the
    reference's window -- codes [0, N) for e < N, read at position e; codes [e - N + 1, e] afterwards, read at the last
    position --, the argmax of the position's logits where constraint (B, num_tokens) is < 0, its code elsewhere.
    -> (codes (B, num_tokens) int64, the smallest top-1 / top-2 logit gap over the FREE positions, the rms of every logit the
    loop read, rows (B, num_tokens, V) float64: the logits each code was chosen from)."""
    prior.eval()
    N = prior.num_tokens
    B, nt = constraint.shape
    dev = prior.sos.device
    seq = torch.zeros(B, nt, dtype=torch.int64, device=dev)
    rows = []
    gap = float('inf')
    for e in range(nt):
        w, p = (0, e) if e < N else (e - N + 1, N - 1)
        lg = prior.forward(seq[:, w:w + N].contiguous())['weights_per_category'][0][:, p].double()
        rows.append(lg.cpu())
        f = constraint[:, e].to(dev)
        free = f < 0
        if lg.shape[1] >= 2 and bool(free.any()):
            top2 = torch.topk(lg[free], 2, dim=-1)[0]
            gap = min(gap, float((top2[:, 0] - top2[:, 1]).min()))
        seq[:, e] = torch.where(free, lg.argmax(dim=-1), f)
    rows = torch.stack(rows, dim=1)
    return seq, gap, float(rows.pow(2).mean().sqrt()), rows
