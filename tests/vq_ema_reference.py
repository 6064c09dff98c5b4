"""Float64 restatements of the EMA quantiser (quantizer_type 'ema': vqcpc_vq_ema_stats, vqcpc_vq_commit_bwd,
vqcpc_vq_ema_update, EMAProductVectorQuantizer) and the DERIVED error bounds its GPU tests use.

Every function takes the fp32 inputs of the kernel (cast to float64 exactly) and the fp32-rounded constants g, h, eps, so the
only difference to the kernel is the kernel's own rounding.  tests/test_vq_ema_reference_cpu.py pins the loss and d_z on torch
float64 autograd and the update on a plain loop over k.

Error model: u = 2^-24; fl(a op b) = (a op b)(1 + d), |d| <= u, for + - * / (the kernels are compiled without FMA contraction
and with IEEE division); no underflow at the magnitudes of the tests.  The derivations sit next to each bound.
"""
import numpy as np
import torch

F64 = torch.float64
U = 2.0 ** -24
LOSS_EPS = float(np.float32(1e-5))            # the 1e-5f of the non-squared loss, as the kernels hold it


def f32(x):
    """A python float rounded to fp32, as a python float (what a c_float argument carries)."""
    return float(np.float32(x))


def constants(decay=0.99, epsilon=1e-5):
    """(g, h, eps) as the kernel receives them: g = float32(decay), h = float32(1 - decay) with the difference in double."""
    return f32(decay), f32(1.0 - float(decay)), f32(epsilon)


def _d(x):
    return torch.as_tensor(x).detach().cpu().to(F64)


# ---------------------------------------------------------------------------------------------------------------------
# statistics
def stats(z, idx, K):
    """z (R, D), idx (R, ncb) -> counts (ncb, K), sums (ncb, K, dsub), abs_sums (ncb, K, dsub) = sum |z| per cell (the scale of
    the summation bound).  Rows whose index is outside [0, K) are skipped, as the kernel skips them."""
    z, idx = _d(z), torch.as_tensor(idx).cpu().long()
    R, D = z.shape
    ncb = idx.shape[1]
    dsub = D // ncb
    n = torch.zeros(ncb, K, dtype=F64)
    s = torch.zeros(ncb, K, dsub, dtype=F64)
    a = torch.zeros(ncb, K, dsub, dtype=F64)
    for c in range(ncb):
        ok = (idx[:, c] >= 0) & (idx[:, c] < K)
        k = idx[ok, c]
        zc = z[ok, c * dsub:(c + 1) * dsub]
        n[c].index_add_(0, k, torch.ones(k.shape[0], dtype=F64))
        s[c].index_add_(0, k, zc)
        a[c].index_add_(0, k, zc.abs())
    return n, s, a


def sum_bound(counts, abs_sums):
    """|fp32 sum - exact sum| per cell.  A sum of n fp32 values in ANY order (here: 256-row chunks in row order, then the chunk
    partials in the order of the split reduction) has |err| <= gamma_(n-1) sum|z| with gamma_j = j u / (1 - j u): every summand
    passes through at most n - 1 rounded additions.  n u >= gamma_(n-1) for n u < 1/2 (n < 2^23), so the bound is n u sum|z|.
    Counts are sums of 1.0f below 2^24: exact."""
    return counts.unsqueeze(-1) * U * abs_sums


# ---------------------------------------------------------------------------------------------------------------------
# update
def update(N, m, n, s, g, h, eps):
    """One EMA update in float64: returns (N', m', e)."""
    N, m, n, s = _d(N), _d(m), _d(n), _d(s)
    K = N.shape[-1]
    N1 = g * N + h * n
    m1 = g * m + h * s
    T = N1.sum(-1, keepdim=True)
    Nt = (N1 + eps) / (T + K * eps) * T
    return N1, m1, m1 / Nt.unsqueeze(-1)


def update_loop(N, m, n, s, g, h, eps):
    """The same, one codebook and one code at a time (the pin of `update`)."""
    N, m, n, s = (_d(x).numpy() for x in (N, m, n, s))
    ncb, K = N.shape
    dsub = m.shape[2]
    N1, m1, e = np.zeros_like(N), np.zeros_like(m), np.zeros_like(m)
    for c in range(ncb):
        T = 0.0
        for k in range(K):
            N1[c, k] = g * N[c, k] + h * n[c, k]
            T += N1[c, k]
        for k in range(K):
            Nt = (N1[c, k] + eps) / (T + K * eps) * T
            for t in range(dsub):
                m1[c, k, t] = g * m[c, k, t] + h * s[c, k, t]
                e[c, k, t] = m1[c, k, t] / Nt
    return torch.from_numpy(N1), torch.from_numpy(m1), torch.from_numpy(e)


def ema_bounds(N, m, n, s, g, h, eps, s_err=None):
    """(bound N', bound m', bound e) for one fp32 update of exact fp32 inputs; s_err: an error the sums s already carry
    (sum_bound), propagated linearly.

    N' = fl(fl(g N) + fl(h n)).  The two products err by u |g N| and u |h n|; the addition by u |fl(gN) + fl(hn)|
        <= u (1 + u)(|g N| + |h n|).  Total <= (2 u + u^2)(|g N| + |h n|) <= 3 u (|g N| + |h n|).
    m': the same with (m, s): <= 3 u (|g m| + |h s|), plus h s_err.
    e = m' / Nt.  N, n >= 0 and g, h, eps > 0, so everything below the division by Nt is a sum / product / quotient of
      non-negative numbers and relative errors add (first order, counted in units of u):
        N'_k                                   2      (two roundings on its path: one product, the sum)
        a_k  = fl(N'_k + eps)                  3      (max of the operands' 2 and 0, + 1)
        T    = sum_k N'_k, K terms, any order  K + 1  (2 of the terms + at most K - 1 additions on a path; zero padding adds
                                                       exactly)
        Ke   = fl(float(K) eps)                1
        den  = fl(T + Ke)                      K + 2
        q_k  = fl(a_k / den)                   3 + (K + 2) + 1 = K + 6
        Nt_k = fl(q_k T)                       (K + 6) + (K + 1) + 1 = 2 K + 8
      and e = fl(m'_fl / Nt_fl): |e_fl - e| <= (|m'_fl - m'| + (2 K + 9) u |m'|) / Nt
                                            <= (2 K + 12) u (|g m| + |h s|) / Nt  (+ h s_err / Nt),
      since |m'| <= |g m| + |h s|.  When g m and h s have one sign this is c u |e| with c = 2 K + 12; when they cancel, |e| is
      no scale for the error of m' and the uncancelled magnitude takes its place.  Second-order terms: the factor
      1 / (1 - c u) <= 1.0002 at K = 1024 is covered by rounding c up by 1."""
    N, m, n, s = _d(N), _d(m), _d(n), _d(s)
    K = N.shape[-1]
    bN = 3.0 * U * ((g * N).abs() + (h * n).abs())
    mag = (g * m).abs() + (h * s).abs()
    extra = h * _d(s_err) if s_err is not None else torch.zeros_like(mag)
    bm = 3.0 * U * mag + extra
    N1 = g * N + h * n
    T = N1.sum(-1, keepdim=True)
    Nt = ((N1 + eps) / (T + K * eps) * T).unsqueeze(-1)
    be = (e_constant(K) * U * mag + extra) / Nt
    return bN, bm, be


def e_constant(K):
    """c of the codebook bound c u (|g m| + |h s|) / Nt: 2 K + 12 from the operation count above, + 1 for the second order."""
    return 2 * K + 13


# ---------------------------------------------------------------------------------------------------------------------
# forward, loss, d_z
def lookup(cb, idx):
    """cb (ncb, K, dsub), idx (R, ncb) -> q (R, D)."""
    cb, idx = _d(cb), torch.as_tensor(idx).cpu().long()
    return torch.cat([cb[c][idx[:, c]] for c in range(cb.shape[0])], dim=1)


def nearest(z, cb):
    """float64 nearest-code assignment (first index on ties) -- only for inputs without near ties."""
    z, cb = _d(z), _d(cb)
    ncb, K, dsub = cb.shape
    return torch.stack([((z[:, None, c * dsub:(c + 1) * dsub] - cb[c][None]) ** 2).sum(-1).argmin(1) for c in range(ncb)], dim=1)


def row_loss(z, q, squared, dtype=F64):
    """l per row: sum (q - z)^2, or ||(q - z) + 1e-5||."""
    z, q = torch.as_tensor(z).to(dtype), torch.as_tensor(q).to(dtype)
    if squared:
        return ((q - z) ** 2).sum(1)
    return torch.sqrt((((q - z) + LOSS_EPS) ** 2).sum(1))


def forward(z, cb, idx, beta, squared):
    """(straight-through output z + (q - z), loss beta * l) in float64."""
    z, q = _d(z), lookup(cb, idx)
    return z + (q - z), beta * row_loss(z, q, squared)


def d_z(z, cb, idx, g_zq, g_loss, beta, squared, dtype=F64):
    """d_z = g_zq + g_loss * beta * dl/dz, in closed form (q is a constant): dl/dz = -2 (q - z), or -((q - z) + 1e-5) / l.
    dtype=torch.float32 evaluates the same expressions in plain fp32 (the yardstick of the kernel's tolerance)."""
    z, g_zq, g_loss = (torch.as_tensor(x).detach().cpu().to(dtype) for x in (z, g_zq, g_loss))
    q = lookup(cb, idx).to(dtype)
    diff = q - z
    if squared:
        dq = 2.0 * diff
    else:
        v = diff + LOSS_EPS
        dq = v / torch.sqrt((v * v).sum(1, keepdim=True))
    return g_zq - g_loss.unsqueeze(1) * beta * dq
