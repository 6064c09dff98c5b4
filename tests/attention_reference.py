"""Float64 reference of the rectangular, masked attention with the learned relative bias (csrc/relattn_x.hip), written from the
closed form in that file's header comment and from include/vqcpc.h in plain torch.  TEST INFRASTRUCTURE: nothing here imports
the package under test or oracle/.  Anchored on the CPU by tests/test_attention_reference_cpu.py (the oracle's functions, the
reference project's recorded outputs, torch float64 autograd) and used by tests/test_relattn_x_kernels_gpu.py.

Every function takes `dtype` (default float64): the same formula in plain fp32 (`dtype=torch.float32`) is the yardstick of the
tolerances (see test_relattn_x_kernels_gpu.py).  Inputs are cast, never modified.

Layouts are the ABI's: q (n * Lq, H * hd), k / v (n * Lk, H * hd) with head h in columns [h * hd, (h + 1) * hd), q UNSCALED,
e1 / e2 (H * Lk, hd), ctx (n * Lq, H * hd), probs (n, H, Lq, Lk).  With r = Lq / Lk, qs = q / sqrt(hd) and p(i) = i // r:

    S[i][j]  = qs_i . k_j + qs_i . Erel[j - p(i) + Lk - 1]
    Erel[x]  = e1[h][x] for x < Lk, e2[h][x - Lk + 1] otherwise          (2 Lk - 1 rows; e2 row 0 is never read)
    keep     = all (mask 0) | j <= p(i) (mask 1, causal) | j >= p(i) (mask 2, anticausal)
    P        = softmax of S over the kept keys, exactly 0 elsewhere
    ctx      = (P * keep_scale) @ v,  keep_scale of element ((n * H + h) * Lq + i) * Lk + j = 0 or 1 / (1 - p_drop)

  erel / rel_index / keep_rule     the pieces above
  rel_bias                         qs_i . Erel[j - p(i) + Lk - 1]
  keep_scale                       train_reference.dropout_scale in the (n, H, Lq, Lk) layout
  attn_fwd                         ctx, probs
  attn_bwd                         explicit backward: d_q, d_k, d_v, d_e1, d_e2 and the 2-norm of the float64 summands of every
                                   d_e1 / d_e2 element (the scale of the column-sum statistic, as train_reference.col_err's)
  de_err                           |out - ref| / that norm, per element
"""
import math

import torch

import train_reference as T

F64 = torch.float64
NONE, CAUSAL, ANTICAUSAL = 0, 1, 2


def _t(x, dtype):
    return torch.as_tensor(x).to(dtype)


def heads(x, n, L, H):
    """(n * L, H * hd) -> (n, H, L, hd)"""
    return x.reshape(n, L, H, -1).transpose(1, 2)


def rows(x):
    """(n, H, L, hd) -> (n * L, H * hd)"""
    n, H, L, hd = x.shape
    return x.transpose(1, 2).reshape(n * L, H * hd)


def erel(e1, e2, H, Lk, dtype=F64):
    """(H, 2 Lk - 1, hd): rows 0 .. Lk - 1 are e1[h], rows Lk .. 2 Lk - 2 are e2[h][1 ..]."""
    e1, e2 = _t(e1, dtype).reshape(H, Lk, -1), _t(e2, dtype).reshape(H, Lk, -1)
    return torch.cat([e1, e2[:, 1:]], dim=1)


def rel_index(Lq, Lk):
    """(Lq, Lk) int64: x[i][j] = j - p(i) + Lk - 1 in [0, 2 Lk - 2]."""
    assert Lk >= 1 and Lq >= Lk and Lq % Lk == 0
    p = torch.arange(Lq) // (Lq // Lk)
    return torch.arange(Lk).view(1, Lk) - p.view(Lq, 1) + (Lk - 1)


def keep_rule(mask, Lq, Lk):
    """(Lq, Lk) bool"""
    x = rel_index(Lq, Lk)
    if mask == NONE:
        return torch.ones(Lq, Lk, dtype=torch.bool)
    assert mask in (CAUSAL, ANTICAUSAL)
    return x <= Lk - 1 if mask == CAUSAL else x >= Lk - 1


def rel_bias(qs, e1, e2, Lk, dtype=F64):
    """qs (n, H, Lq, hd), ALREADY scaled -> (n, H, Lq, Lk): qs_i . Erel[j - p(i) + Lk - 1]."""
    qs = _t(qs, dtype)
    n, H, Lq, _ = qs.shape
    band = qs @ erel(e1, e2, H, Lk, dtype).transpose(-1, -2)                      # (n, H, Lq, 2 Lk - 1)
    return band.gather(-1, rel_index(Lq, Lk).expand(n, H, Lq, Lk))


def keep_scale(seed, n, H, Lq, Lk, p):
    """(n, H, Lq, Lk) float64: 0 or 1 / (1 - p) by the library's counter-based generator; None when p == 0."""
    return None if p == 0 else T.dropout_scale(seed, (n, H, Lq, Lk), p)


def attn_fwd(q, k, v, e1, e2, n, Lq, Lk, H, mask, scale=None, dtype=F64):
    """-> ctx (n * Lq, H * hd), probs (n, H, Lq, Lk) (before dropout).  scale: keep_scale(..) or None."""
    q, k, v = _t(q, dtype), _t(k, dtype), _t(v, dtype)
    hd = q.shape[1] // H
    qs = heads(q, n, Lq, H) * (1.0 / math.sqrt(hd))
    s = qs @ heads(k, n, Lk, H).transpose(-1, -2) + rel_bias(qs, e1, e2, Lk, dtype)
    keep = keep_rule(mask, Lq, Lk)
    s = s.masked_fill(~keep, float('-inf'))
    e = torch.exp(s - s.max(-1, keepdim=True)[0])                                  # exp(-inf) = 0: masked entries exactly 0
    probs = e / e.sum(-1, keepdim=True)
    pd = probs if scale is None else probs * _t(scale, dtype)
    return rows(pd @ heads(v, n, Lk, H)), probs


def attn_bwd(d_ctx, q, k, v, probs, e1, e2, n, Lq, Lk, H, mask, scale=None, dtype=F64, dS=None):
    """Explicit backward.  `probs` is an INPUT, as it is of the kernel (the saved softmax before dropout); entries the mask
    removes are taken as 0 whatever they hold.  `dS` (n, H, Lq, Lk): use these softmax-input gradients instead of forming them
    (a replay of one kernel's dS through exact sums).
    -> d_q (n * Lq, H * hd), d_k, d_v (n * Lk, H * hd), d_e1, d_e2 (H * Lk, hd), n1, n2 (H * Lk, hd) = 2-norms of the summands of
    every d_e1 / d_e2 element (always float64-accurate enough: formed in `dtype` from the same terms)."""
    d_ctx, q, k, v, probs = (_t(a, dtype) for a in (d_ctx, q, k, v, probs))
    hd = q.shape[1] // H
    r = Lq // Lk
    sc = 1.0 / math.sqrt(hd)
    qs, kh, vh, do = heads(q, n, Lq, H) * sc, heads(k, n, Lk, H), heads(v, n, Lk, H), heads(d_ctx, n, Lq, H)
    keep = keep_rule(mask, Lq, Lk)
    P = torch.where(keep, probs, torch.zeros((), dtype=dtype))
    dP = do @ vh.transpose(-1, -2)
    Pd = P
    if scale is not None:
        dP = dP * _t(scale, dtype)
        Pd = P * _t(scale, dtype)
    dS = P * (dP - (dP * P).sum(-1, keepdim=True)) if dS is None else torch.where(keep, _t(dS, dtype), torch.zeros((), dtype=dtype))
    d_v = Pd.transpose(-1, -2) @ do
    d_k = dS.transpose(-1, -2) @ qs
    E = erel(e1, e2, H, Lk, dtype)
    x = rel_index(Lq, Lk)
    # d qs_i = sum_j dS[i][j] (k_j + Erel[x(i, j)]): the second term through the band, scattered to its relative rows
    band = torch.zeros(n, H, Lq, 2 * Lk - 1, dtype=dtype).scatter_(-1, x.expand(n, H, Lq, Lk), dS)
    d_q = (dS @ kh + band @ E) * sc
    # d Erel[x] = sum_n sum_i dS[i][x + p(i) - (Lk - 1)] qs_i.  The r queries of one memory position p meet relative rows
    # [Lk - 1 - p, 2 Lk - 2 - p] with keys 0 .. Lk - 1 in order: one (Lk, hd) block per p
    dE = torch.zeros(H, 2 * Lk - 1, hd, dtype=dtype)
    nE = torch.zeros(H, 2 * Lk - 1, hd, dtype=F64)
    dS5, qs5 = dS.reshape(n, H, Lk, r, Lk), qs.reshape(n, H, Lk, r, hd)
    dS5sq, qs5sq = dS5.double() ** 2, qs5.double() ** 2
    for p in range(Lk):
        dE[:, Lk - 1 - p:2 * Lk - 1 - p] += torch.einsum('nhuj,nhuc->hjc', dS5[:, :, p], qs5[:, :, p])
        nE[:, Lk - 1 - p:2 * Lk - 1 - p] += torch.einsum('nhuj,nhuc->hjc', dS5sq[:, :, p], qs5sq[:, :, p])
    nE = torch.sqrt(nE)

    def split(t):
        t1 = t[:, :Lk].reshape(H * Lk, hd)
        t2 = torch.cat([torch.zeros(H, 1, hd, dtype=t.dtype), t[:, Lk:]], dim=1).reshape(H * Lk, hd)
        return t1, t2

    d_e1, d_e2 = split(dE)
    n1, n2 = split(nE)
    return rows(d_q), rows(d_k), rows(d_v), d_e1, d_e2, n1, n2


def de_err(out, ref64, norm64):
    """Per element of d_e1 / d_e2: |out - ref| / ||summands||_2 -> float64, same shape.  An element with no non-zero summand
    (structurally zero under the mask; e2 row 0) has no scale: 0 when `out` is exactly zero there, inf otherwise."""
    out, ref, nrm = (torch.as_tensor(a).double() for a in (out, ref64, norm64))
    num = (out.reshape(ref.shape) - ref).abs()
    zero = nrm == 0
    res = num / torch.where(zero, torch.ones_like(nrm), nrm)
    return torch.where(zero, torch.where(num == 0, torch.zeros_like(num), torch.full_like(num, float('inf'))), res)
