"""Float64 references of the training step's pointwise and row kernels (csrc/embed_ln.hip, util.hip, gru.hip, nce.hip,
student.hip), written from the formulas of include/vqcpc.h in plain torch / numpy.  TEST INFRASTRUCTURE: nothing here imports
the package under test or oracle/.  Anchored on the CPU by tests/test_train_reference_cpu.py (torch float64 autograd and the
oracle's functions) and used by tests/test_train_kernels_gpu.py.

Every function takes `dtype` (default float64): the same formula in plain fp32 (`dtype=torch.float32`) is the yardstick of the
tolerances that are not derived (see test_train_kernels_gpu.py).  Inputs are cast, never modified.

  dropout_scale               the keep-mask of csrc/common.h times 1 / (1 - p), from decode_reference.rng_u24_ref
  ln_fwd / ln_bwd             y = LN(x + r * scale) * gamma + beta and its gradients (d_s, d_r, d_gamma, d_beta)
  selu / selu_grad            with expm1
  gru_cell_fwd / _bwd, gru_step_fwd / _bwd
  nce_fwd / nce_bwd           f_pos, f_neg, loss_b, hits; d_c, d_W, d_z_pos, d_z_neg
  softmax_ce                  hard or soft targets: loss and d loss / d logits
  upscale_fwd / upscale_bwd
  clip_coef / adam_step / adam_steps
  bf16_rne / bf16_to_f32      round to nearest even on the bit patterns
  row_err / col_err           the per-row / per-column error statistic
"""
import math

import numpy as np
import torch

from decode_reference import rng_u24_ref

F64 = torch.float64
SELU_ALPHA = 1.6732632423543772848170429916717
SELU_SCALE = 1.0507009873554804934193349852946


def _t(x, dtype):
    return None if x is None else torch.as_tensor(x).to(dtype)


# ---------------------------------------------------------------------------------------------------------------------
# dropout
def drop_threshold(p):
    """csrc/common.h: (uint32)(p * 2^24) with p and the product in fp32."""
    return int(np.float32(p) * np.float32(16777216.0))


def dropout_keep(seed, n, p, idx_base=0):
    """keep[i] (bool, numpy) for element indices idx_base + i, i < n: u24(seed, index) >= threshold; p == 0 keeps everything."""
    thr = drop_threshold(p)
    if thr == 0:
        return np.ones(int(n), dtype=bool)
    idx = (np.arange(int(n), dtype=np.uint64) + np.uint64(idx_base)).astype(np.int64)
    sd = np.array(seed, dtype=np.uint64).astype(np.int64)
    return rng_u24_ref(sd, idx) >= thr


def inv_keep(p):
    """1 / (1 - p) as the kernels form it: in fp32 (p is an fp32 argument of the ABI); returned as a Python float."""
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))


def dropout_scale(seed, shape, p, idx_base=0):
    """The mask value of every element of a row-major tensor: 0 or 1 / (1 - p) (1 when p == 0), float64."""
    n = int(np.prod(shape))
    k = dropout_keep(seed, n, p, idx_base)
    sc = 1.0 if drop_threshold(p) == 0 else inv_keep(p)
    return torch.from_numpy(k.astype(np.float64) * sc).reshape(shape)


# ---------------------------------------------------------------------------------------------------------------------
# LayerNorm
def ln_fwd(x, r, scale, gamma, beta, eps, dtype=F64):
    """s = x + r * scale (r None: s = x, the residual-sum form); mean, biased variance, rstd = 1 / sqrt(var + eps);
    y = (s - mean) * rstd * gamma + beta.  x (M, d) -> y (M, d), mean (M,), rstd (M,), s (M, d)."""
    x, r, scale, gamma, beta = (_t(a, dtype) for a in (x, r, scale, gamma, beta))
    s = x if r is None else x + r * scale
    mu = s.mean(-1, keepdim=True)
    xc = s - mu
    var = (xc * xc).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    y = xc * rstd * gamma + beta
    return y, mu.squeeze(-1), rstd.squeeze(-1), s


def ln_bwd(dy, s, gamma, mean, rstd, scale=None, dtype=F64):
    """Gradients of ln_fwd for the SAVED mean / rstd (inputs of the kernel): xh = (s - mean) rstd, g = dy gamma,
    d_s = rstd (g - mean_c(g) - xh mean_c(g xh)); d_r = d_s * scale; d_gamma = sum_m dy xh; d_beta = sum_m dy."""
    dy, s, gamma, mean, rstd, scale = (_t(a, dtype) for a in (dy, s, gamma, mean, rstd, scale))
    xh = (s - mean.unsqueeze(-1)) * rstd.unsqueeze(-1)
    g = dy * gamma
    m1 = g.mean(-1, keepdim=True)
    m2 = (g * xh).mean(-1, keepdim=True)
    d_s = rstd.unsqueeze(-1) * (g - m1 - xh * m2)
    d_r = d_s if scale is None else d_s * scale
    return d_s, d_r, (dy * xh).sum(0), dy.sum(0)


# ---------------------------------------------------------------------------------------------------------------------
# SELU
def selu(x, dtype=F64):
    x = _t(x, dtype)
    return SELU_SCALE * torch.where(x > 0, x, SELU_ALPHA * torch.expm1(x))


def selu_grad(x, dtype=F64):
    x = _t(x, dtype)
    return SELU_SCALE * torch.where(x > 0, torch.ones_like(x), SELU_ALPHA * torch.exp(x))


def dropout_selu_fwd(h, scale, dtype=F64):
    return selu(_t(h, dtype) * _t(scale, dtype), dtype)


def dropout_selu_bwd(h, g, scale, dtype=F64):
    h, g, scale = (_t(a, dtype) for a in (h, g, scale))
    return g * selu_grad(h * scale, dtype) * scale


# ---------------------------------------------------------------------------------------------------------------------
# GRU
def _gates(gi, gh, H):
    r = torch.sigmoid(gi[:, :H] + gh[:, :H])
    u = torch.sigmoid(gi[:, H:2 * H] + gh[:, H:2 * H])
    n = torch.tanh(gi[:, 2 * H:] + r * gh[:, 2 * H:])
    return r, u, n


def gru_cell_fwd(gi, gh, h_prev=None, scale=None, dtype=F64):
    """gi, gh (B, 3H) in gate order r | z | n -> h_out, y_out = h_out * scale (scale None: y_out = h_out)."""
    gi, gh, h_prev, scale = (_t(a, dtype) for a in (gi, gh, h_prev, scale))
    H = gi.shape[1] // 3
    r, u, n = _gates(gi, gh, H)
    hp = torch.zeros_like(n) if h_prev is None else h_prev
    h = (1 - u) * n + u * hp
    return h, (h if scale is None else h * scale)


def gru_cell_bwd(gi, gh, h_prev, d_y, d_h, scale=None, dtype=F64):
    """dh = d_y * scale + d_h (either may be None) -> d_gi, d_gh (B, 3H), d_hprev = dh * u."""
    gi, gh, h_prev, d_y, d_h, scale = (_t(a, dtype) for a in (gi, gh, h_prev, d_y, d_h, scale))
    H = gi.shape[1] // 3
    r, u, n = _gates(gi, gh, H)
    hp = torch.zeros_like(n) if h_prev is None else h_prev
    dh = torch.zeros_like(n)
    if d_h is not None:
        dh = dh + d_h
    if d_y is not None:
        dh = dh + (d_y if scale is None else d_y * scale)
    da_n = dh * (1 - u) * (1 - n * n)
    da_u = dh * (hp - n) * u * (1 - u)
    da_r = da_n * gh[:, 2 * H:] * r * (1 - r)
    return torch.cat([da_r, da_u, da_n], 1), torch.cat([da_r, da_u, da_n * r], 1), dh * u


def gru_step_fwd(gi, w_hh, b_hh, h_prev=None, scale=None, dtype=F64):
    """gh = h_prev W_hh^T + b_hh (h_prev None: gh = b_hh), then the cell -> gh, h_out, y_out."""
    gi, w_hh, b_hh, h_prev = (_t(a, dtype) for a in (gi, w_hh, b_hh, h_prev))
    gh = b_hh.expand(gi.shape[0], -1).clone() if h_prev is None else h_prev @ w_hh.t() + b_hh
    h, y = gru_cell_fwd(gi, gh, h_prev, scale, dtype)
    return gh, h, y


def gru_step_bwd(dgh_next, whh_t, dhp, gi, gh, h_prev, d_y, scale=None, dtype=F64):
    """dh = dgh_next (B, 3H) . whh_t (H, 3H)^T + dhp (+ d_y * scale), then the cell backward -> d_gi, d_gh, dhp' = dh * u."""
    dgh_next, whh_t, dhp = (_t(a, dtype) for a in (dgh_next, whh_t, dhp))
    d_h = dgh_next @ whh_t.t() + dhp
    return gru_cell_bwd(gi, gh, h_prev, d_y, d_h, scale, dtype)


# ---------------------------------------------------------------------------------------------------------------------
# InfoNCE
def nce_fwd(c, W, z_pos, z_neg, dtype=F64):
    """c (B, cdim), W (zdim, cdim, K), z_pos (B, K, zdim), z_neg (B, N, K, zdim) -> f_pos (B, K), f_neg (B, K, N),
    loss_b (B,) = -sum_k (pos - logsumexp([neg, pos])), hits (B, K) = pos > max_n neg."""
    c, W, z_pos, z_neg = (_t(a, dtype) for a in (c, W, z_pos, z_neg))
    wc = torch.einsum('bc,zck->bkz', c, W)
    f_pos = (wc * z_pos).sum(-1)
    f_neg = torch.einsum('bkz,bnkz->bkn', wc, z_neg)
    allf = torch.cat([f_neg, f_pos.unsqueeze(2)], 2)
    m = allf.max(2, keepdim=True)[0]
    lse = m.squeeze(2) + torch.log(torch.exp(allf - m).sum(2))
    loss_b = -(f_pos - lse).sum(1)
    hits = (f_pos > f_neg.max(2)[0]).to(dtype)
    return f_pos, f_neg, loss_b, hits


def nce_bwd(c, W, z_pos, z_neg, f_pos, f_neg, g, dtype=F64):
    """Gradients of sum_b g[b] loss_b from the SAVED scores: softmax p over [neg, pos]; d f_neg = g p_n, d f_pos = -g (1 - p_pos);
    d_z = d f * Wc; dWc = d f_pos z_pos + sum_n d f_neg z_neg; d_c[b, c] = sum_{k,z} dWc W; d_W[z, c, k] = sum_b dWc[b,k,z] c[b,c]."""
    c, W, z_pos, z_neg, f_pos, f_neg, g = (_t(a, dtype) for a in (c, W, z_pos, z_neg, f_pos, f_neg, g))
    wc = torch.einsum('bc,zck->bkz', c, W)
    allf = torch.cat([f_neg, f_pos.unsqueeze(2)], 2)
    m = allf.max(2, keepdim=True)[0]
    e = torch.exp(allf - m)
    p = e / e.sum(2, keepdim=True)
    gb = g.view(-1, 1)
    df_neg = gb.unsqueeze(2) * p[:, :, :-1]                        # (B, K, N)
    df_pos = -gb * (1 - p[:, :, -1])                               # (B, K)
    d_z_pos = df_pos.unsqueeze(2) * wc
    d_z_neg = df_neg.permute(0, 2, 1).unsqueeze(3) * wc.unsqueeze(1)
    dwc = df_pos.unsqueeze(2) * z_pos + torch.einsum('bkn,bnkz->bkz', df_neg, z_neg)
    d_c = torch.einsum('bkz,zck->bc', dwc, W)
    d_W = torch.einsum('bkz,bc->zck', dwc, c)
    return d_c, d_W, d_z_pos, d_z_neg


# ---------------------------------------------------------------------------------------------------------------------
# softmax cross-entropy
def softmax_ce(logits, target=None, target_logits=None, dtype=F64):
    """loss[r] = -sum_v t[v] log_softmax(logits[r])[v], grad = softmax(logits[r]) - t; t = onehot(target) or softmax(target_logits)."""
    x = _t(logits, dtype)
    lp = x - x.max(-1, keepdim=True)[0]
    lp = lp - torch.log(torch.exp(lp).sum(-1, keepdim=True))
    if target is not None:
        t = torch.zeros_like(x)
        t.scatter_(1, torch.as_tensor(target).long().view(-1, 1), 1.0)
    else:
        tl = _t(target_logits, dtype)
        te = torch.exp(tl - tl.max(-1, keepdim=True)[0])
        t = te / te.sum(-1, keepdim=True)
    return -(t * lp).sum(-1), torch.exp(lp) - t


# ---------------------------------------------------------------------------------------------------------------------
# upscale
def upscale_fwd(x, emb, dtype=F64):
    """x (rows, d), emb (f, d) -> out (rows * f, d): out[r f + u] = x[r] + emb[u]."""
    x, emb = _t(x, dtype), _t(emb, dtype)
    return (x.unsqueeze(1) + emb.unsqueeze(0)).reshape(-1, x.shape[1])


def upscale_bwd(g, f, dtype=F64):
    """g (rows * f, d) -> dx (rows, d) = sum_u, d_emb (f, d) = sum_r."""
    g = _t(g, dtype)
    g3 = g.reshape(-1, f, g.shape[1])
    return g3.sum(1), g3.sum(0)


# ---------------------------------------------------------------------------------------------------------------------
# optimiser
def sumsq(g, grad_scale=1.0):
    g = torch.as_tensor(g).double() * float(grad_scale)
    return float((g * g).sum())


def clip_coef(sumsq_value, max_norm, grad_scale=1.0):
    """grad_scale * min(1, max_norm / (sqrt(sumsq) + 1e-6)); sumsq None: no clipping."""
    if sumsq_value is None:
        return float(grad_scale)
    return float(grad_scale) * min(1.0, float(max_norm) / (math.sqrt(float(sumsq_value)) + 1e-6))


def adam_step(p, g, m, v, lr, beta1, beta2, eps, t, coef=1.0):
    """One step with step count t >= 1 in float64: g *= coef; m = b1 m + (1 - b1) g; v = b2 v + (1 - b2) g^2;
    p -= lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps).  -> p, g, m, v (new tensors)."""
    p, g, m, v = (torch.as_tensor(a).double() for a in (p, g, m, v))
    g = g * coef
    m = beta1 * m + (1.0 - beta1) * g
    v = beta2 * v + (1.0 - beta2) * g * g
    bc1, bc2 = 1.0 - beta1 ** t, 1.0 - beta2 ** t
    p = p - (lr / bc1) * (m / (torch.sqrt(v) / math.sqrt(bc2) + eps))
    return p, g, m, v


def adam_steps(p, grads, lr, beta1, beta2, eps, max_norm=None, grad_scale=1.0):
    """Clip + Adam for t = 1 .. len(grads) from zero moments (what clip_grad_norm_ + torch.optim.Adam.step do) -> p, m, v."""
    p = torch.as_tensor(p).double()
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    for t, g in enumerate(grads, 1):
        coef = clip_coef(None if max_norm is None else sumsq(g, grad_scale), max_norm, grad_scale)
        p, _, m, v = adam_step(p, g, m, v, lr, beta1, beta2, eps, t, coef)
    return p, m, v


# ---------------------------------------------------------------------------------------------------------------------
# bf16
def bf16_rne(x):
    """fp32 tensor -> int32 tensor of the bf16 bit patterns (0 .. 65535), round to nearest, ties to even (finite inputs)."""
    u = torch.as_tensor(x).float().contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    return (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF).to(torch.int32)


def bf16_to_f32(b):
    """bf16 bit patterns (any integer tensor) -> the fp32 values they stand for."""
    return ((torch.as_tensor(b).to(torch.int64) & 0xFFFF) << 16).to(torch.int32).view(torch.float32)


# ---------------------------------------------------------------------------------------------------------------------
# error statistics
def row_err(out, ref64):
    """Per row: max |out - ref| / rms(ref of that row) -> (rows,) float64.  A row whose reference is identically zero has no
    scale: its entry is 0 when `out` is exactly zero there and inf otherwise.  Never a tensor-wide denominator."""
    out, ref = torch.as_tensor(out).double(), torch.as_tensor(ref64).double()
    ref = ref.reshape(ref.shape[0], -1)                            # a vector is rows of one element: rms = |ref|
    out = out.reshape(ref.shape)
    num = (out - ref).abs().max(1)[0]
    rms = torch.sqrt((ref * ref).mean(1))
    zero = rms == 0
    res = num / torch.where(zero, torch.ones_like(rms), rms)
    return torch.where(zero, torch.where(num == 0, torch.zeros_like(num), torch.full_like(num, float('inf'))), res)


def col_err(out, ref64, terms64):
    """Per column of a column sum (d_gamma, d_beta): |out[c] - ref[c]| / ||terms[:, c]||_2, terms (rows, cols) = the float64
    summands of column c.  The sum itself may cancel to nothing, so the column's own scale is the norm of what is summed (the
    size a sum of that many rounded terms errs by is proportional to it).  A column of zero summands: 0 if out is 0, else inf."""
    out, ref, terms = (torch.as_tensor(a).double() for a in (out, ref64, terms64))
    num = (out.reshape(-1) - ref.reshape(-1)).abs()
    nrm = torch.sqrt((terms * terms).sum(0))
    zero = nrm == 0
    res = num / torch.where(zero, torch.ones_like(nrm), nrm)
    return torch.where(zero, torch.where(num == 0, torch.zeros_like(num), torch.full_like(num, float('inf'))), res)
