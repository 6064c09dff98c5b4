"""Float64 reference of the constrained sampler (vqcpc_decode_sample_constrained, csrc/decode.hip) and the slow
forward-per-token generation loop with forcing.  TEST INFRASTRUCTURE: nothing here imports the package under test (the slow
loop takes the decoder as an argument).  Anchored on the CPU by tests/test_constrained_reference_cpu.py; used by
tests/test_decode_sample_constrained_gpu.py and tests/test_generate_constrained_gpu.py.

  constrained_step_ref   one step for one voice: forced tokens where the constraint holds one, the inverse-CDF draw of the
                         filtered row elsewhere, and the emitted token's log-probability under the UNFILTERED row
  logp_bound             the fp32 error bound of the kernel's max / exp / sum / log chain
  forced_greedy_loop     one full `forward` per token, argmax where free, the constraint's token where forced
"""
import numpy as np
import torch

from decode_reference import U_FP32, filter_ref, rng_u24_ref

# The teacher-forced logits tolerance of tests/test_generate_gpu.py::test_incremental_step_equals_full_forward and
# tests/test_generate_long_gpu.py::test_reprefill_equals_full_forward: max |incremental - forward| / rms(forward logits) < 1e-5.
TEACHER_FORCED_TOL = 1e-5

# expf and logf of the device library follow the OpenCL full-profile accuracy (OpenCL C specification, "Relative error as
# ULPs": exp <= 3 ulp, log <= 3 ulp); an ulp is at most 2 u relative, u = 2^-24.
ULP_EXP = 3
ULP_LOG = 3


def draw_ref(probs, seed, pos):
    """The inverse-CDF draw on float64 probabilities (V,): u = (rng_u24(seed, pos) + 0.5) / 2^24, the first token of
    non-zero weight whose cumulative weight exceeds u; none (u rounded up to the total): the last token of non-zero weight."""
    p = np.asarray(probs, dtype=np.float64)
    u = (float(rng_u24_ref(seed, pos)) + 0.5) / 2.0 ** 24
    cum = np.cumsum(p)
    live = np.nonzero(p > 0)[0]
    hit = live[cum[live] > u * cum[-1]]
    return int(hit[0]) if hit.size else int(live[-1])


def logp_ref(row, tok):
    """log_softmax(row)[tok] in float64 with the maximum subtracted."""
    r = torch.as_tensor(row, dtype=torch.float64)
    d = r - r.max()
    return float(d[int(tok)] - torch.log(torch.exp(d).sum()))


def constrained_step_ref(logits, temperature, top_k, top_p, exclude, seeds, pos, constraint):
    """logits (M, V) of the position's voice; seeds (M,) int64; constraint (M,) int64 or None, the constraint's column of this
    position.  -> (tokens (M,) int64, probs (M, V) float64 -- the FILTERED distribution, whatever is forced --, logp (M,)
    float64 -- log_softmax of the UNFILTERED row at the emitted token).  A forced token is clamped to [0, V)."""
    logits = torch.as_tensor(logits, dtype=torch.float64)
    M, V = logits.shape
    tokens = torch.zeros(M, dtype=torch.int64)
    probs = torch.zeros(M, V, dtype=torch.float64)
    logp = torch.zeros(M, dtype=torch.float64)
    for b in range(M):
        probs[b] = filter_ref(logits[b], temperature, top_k, top_p, exclude)
        f = -1 if constraint is None else int(constraint[b])
        tokens[b] = min(max(f, 0), V - 1) if f >= 0 else draw_ref(probs[b].numpy(), int(seeds[b]), int(pos))
        logp[b] = logp_ref(logits[b], tokens[b])
    return tokens, probs, logp


def logp_bound(row, tok):
    """Bound on |logp_fp32 - logp_64| for the kernel's chain on the fp32 row `row` (V <= 256 entries, -inf allowed) at token
    `tok`, u = 2^-24, gamma_n = n u / (1 - n u) (Higham, Accuracy and Stability of Numerical Algorithms, lemma 3.1):

      m      = max_i row_i                              exact (a maximum rounds nothing)
      d_i    = fl(row_i - m)                            |error| <= u |d_i|
      e_i    = expf(d_i)                                relative error <= u |d_i| e^{u |d_i|} (the argument's error) + 2 u ULP_EXP,
                                                        plus an absolute 2^-126 where the result is subnormal or flushed to zero
      s      = sum_i e_i                                four lane-serial additions and six butterfly levels: at most nine
                                                        additions on the path of any term, all terms >= 0: relative gamma_9
      L      = logf(s)                                  |error| <= |ds| / s (1 + |ds| / s) + 2 u ULP_LOG |L|;  s >= 1 as e_max = 1
      logp   = fl(d_tok - L)                            + u |d_tok| (d_tok's own rounding) + u |logp| (the last subtraction)

    with ds / s <= sum_i p_i (u |d_i| e^{u |d_i|} + 2 u ULP_EXP) (1 + gamma_9) + gamma_9 + V 2^-126, p = softmax(row).  The result
    is stored as fp32: the last term covers that rounding.  A forced token of logit -inf has logp = -inf exactly: bound 0."""
    r = torch.as_tensor(row, dtype=torch.float64)
    V = r.numel()
    if float(r[int(tok)]) == -float('inf'):
        return 0.0
    u = U_FP32
    g9 = 9 * u / (1.0 - 9 * u)
    d = r - r.max()
    p = torch.softmax(r, dim=-1)
    da = d.abs().masked_fill(p == 0, 0.0)                                  # -inf entries contribute exactly 0
    rel_terms = float((p * (u * da * torch.exp(u * da) + 2 * u * ULP_EXP)).sum())
    ds = rel_terms * (1.0 + g9) + g9 + V * 2.0 ** -126
    L = float(torch.log(torch.exp(d).sum()))
    lp = float(d[int(tok)]) - L
    return ds * (1.0 + ds) + 2 * u * ULP_LOG * abs(L) + u * abs(float(d[int(tok)])) + u * abs(lp)


@torch.no_grad()
def forced_greedy_loop(dec, codes, constraint):
    """The slow generation: ONE full `dec.forward(codes, x)` per token (the reference's loop, decoder.py:552-723), the
    argmax of the position's logits where constraint (B, events, channels) is < 0, its token elsewhere.  -> (tokens (B,
    events, channels) int64, the smallest top-1 / top-2 logit gap over the FREE positions of vocabularies >= 2, the rms of
    every logit the loop read)."""
    dec.eval()
    B, events, nc = constraint.shape
    x = torch.zeros(B, events, nc, dtype=torch.int64, device=codes.device)
    gap, sq, n = float('inf'), 0.0, 0
    for t in range(events * nc):
        e, c = divmod(t, nc)
        lg = dec.forward(codes, x)['weights_per_category'][c][:, e].double()
        sq, n = sq + float(lg.pow(2).sum()), n + lg.numel()
        f = constraint[:, e, c].to(codes.device)
        free = f < 0
        if lg.shape[1] >= 2 and bool(free.any()):
            top2 = torch.topk(lg[free], 2, dim=-1)[0]
            gap = min(gap, float((top2[:, 0] - top2[:, 1]).min()))
        x[:, e, c] = torch.where(free, lg.argmax(dim=-1), f)
    return x, gap, (sq / max(n, 1)) ** 0.5

