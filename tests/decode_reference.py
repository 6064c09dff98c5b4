"""Float64 references of the generation kernels (csrc/decode.hip, csrc/prior.hip), written from the definitions in plain
torch / numpy.  TEST INFRASTRUCTURE: nothing here imports the package under test.  Anchored on the CPU by
tests/test_decode_reference_cpu.py (the reference's own attention fixtures, its filter fixtures, the host seed rule) and
used by tests/test_decode_kernels_gpu.py.

  linear_ref / linear_bound   y = x W^T + b (ReLU) (+ residual) and the componentwise fp32 error bound of the kernel's chain
  attn_ref                    relative attention of some query rows against Lk keys (self: ratio 1, mask 1, Lk = T)
  filter_ref                  temperature, exclusion, top-k, top-p, softmax (the reference's top_k_top_p_filtering)
  decode_window_ref / prior_window_ref   the integer plumbing of a window move
  splitmix64 / window_seed / rng_u24_ref the seed rule of moving windows and the counter-based draw of csrc/common.h
"""
import math

import numpy as np
import torch

from oracle.decoder_oracle import relative_bias_cross

U_FP32 = 2.0 ** -24


# ---------------------------------------------------------------------------------------------------------------------
# decode_linear
def linear_ref(x, w, b=None, res=None, relu=False, gather=None):
    """x (rows, K) [rows >= M when gathered], w (N, K), b (N,), res (M, N), gather (M,) row indices into x -> (M, N) float64."""
    x = torch.as_tensor(x).double()
    if gather is not None:
        x = x[torch.as_tensor(gather).long()]
    y = x @ torch.as_tensor(w).double().t()
    if b is not None:
        y = y + torch.as_tensor(b).double()
    if relu:
        y = torch.relu(y)
    if res is not None:
        y = y + torch.as_tensor(res).double()
    return y


def linear_bound(x, w, b=None, res=None, gather=None):
    """Componentwise bound on |y_fp32 - y_64| for an fp32 evaluation that is, per output, a chain of 4 ceil(K / 256) FMAs,
    6 butterfly adds, a bias add and a residual add: gamma_n (sum_k |w_k x_k| + |b| + |res|), n = 4 ceil(K / 256) + 8,
    gamma_n = n u / (1 - n u), u = 2^-24 (Higham, Accuracy and Stability of Numerical Algorithms, lemma 3.1 / eq. 3.4), plus
    half an ulp of the float64 result for the final rounding to fp32.  ReLU is 1-Lipschitz and exact: it does not widen it."""
    x = torch.as_tensor(x).double().abs()
    if gather is not None:
        x = x[torch.as_tensor(gather).long()]
    w = torch.as_tensor(w).double().abs()
    K = w.shape[1]
    n = 4 * ((K + 255) // 256) + 8
    gamma = n * U_FP32 / (1.0 - n * U_FP32)
    mag = x @ w.t()
    if b is not None:
        mag = mag + torch.as_tensor(b).double().abs()
    if res is not None:
        mag = mag + torch.as_tensor(res).double().abs()
    return gamma * mag


def half_ulp_fp32(y64):
    """Half the spacing of fp32 at |y64| (the final rounding of a result stored as fp32)."""
    a = torch.as_tensor(y64).double().abs().float().numpy()
    return torch.from_numpy(0.5 * np.spacing(np.maximum(a, np.float32(2.0 ** -126))).astype(np.float64))


# ---------------------------------------------------------------------------------------------------------------------
# decode_attn / decode_prefill_attn
def attn_ref(q, k, v, e1, e2, Lk, ratio, mask, rows, dtype=torch.float64, return_weights=False):
    """q (n, R, H, hd) unscaled query rows at target positions `rows` (R ints in [0, ratio * Lk)); k, v (n, Lk, H, hd);
    e1, e2 (H * Lk, hd).  logits[i, j] = (q_i . k_j + q_i . E[j - p + Lk - 1]) / sqrt(hd), p = i // ratio, E = rows of e1
    for index < Lk, else e2[index - Lk + 1]; mask 0 none / 1 keeps j <= p / 2 keeps j >= p; softmax; P V.
    The relative term is oracle.decoder_oracle.relative_bias_cross (pinned to the reference's skewing by
    tests/test_decoder_oracle_golden.py) evaluated in `dtype`.  -> ctx (n, R, H, hd) [, weights (n, H, R, Lk)].
    `dtype=torch.float32` is the same formula in plain fp32 (the yardstick of the kernels' attention tolerance)."""
    q, k, v = (torch.as_tensor(t).to(dtype) for t in (q, k, v))
    e1, e2 = torch.as_tensor(e1).to(dtype), torch.as_tensor(e2).to(dtype)
    n, R, H, hd = q.shape
    rows = torch.as_tensor(list(rows), dtype=torch.long)
    assert rows.numel() == R and k.shape == (n, Lk, H, hd) and v.shape == (n, Lk, H, hd)
    assert e1.shape == (H * Lk, hd) and e2.shape == (H * Lk, hd)
    assert int(rows.min()) >= 0 and int(rows.max()) < ratio * Lk
    qs = (q * (float(hd) ** -0.5)).permute(0, 2, 1, 3)                       # (n, H, R, hd), scaled as the reference (:137)
    qfull = torch.zeros(n, H, ratio * Lk, hd, dtype=dtype)
    qfull[:, :, rows] = qs
    bias = relative_bias_cross(qfull, e1, e2, Lk)[:, :, rows]                # (n, H, R, Lk)
    scores = qs @ k.permute(0, 2, 3, 1) + bias
    p = (rows // ratio).view(R, 1)
    j = torch.arange(Lk).view(1, Lk)
    if mask == 1:
        scores = scores.masked_fill(~(j <= p), float('-inf'))
    elif mask == 2:
        scores = scores.masked_fill(~(j >= p), float('-inf'))
    else:
        assert mask == 0
    w = torch.softmax(scores, dim=-1)
    ctx = (w @ v.permute(0, 2, 1, 3)).permute(0, 2, 1, 3)
    return (ctx, w) if return_weights else ctx


def attn_logits_ref(q, k, e1, e2, Lk, ratio, rows):
    """The unmasked float64 logits of attn_ref (n, H, R, Lk): lets a test place a row's maximum where it wants it."""
    q, k = torch.as_tensor(q).double(), torch.as_tensor(k).double()
    n, R, H, hd = q.shape
    rows = torch.as_tensor(list(rows), dtype=torch.long)
    qs = (q * (float(hd) ** -0.5)).permute(0, 2, 1, 3)
    qfull = torch.zeros(n, H, ratio * Lk, hd, dtype=torch.float64)
    qfull[:, :, rows] = qs
    return qs @ k.permute(0, 2, 3, 1) + relative_bias_cross(qfull, torch.as_tensor(e1).double(), torch.as_tensor(e2).double(),
                                                            Lk)[:, :, rows]


# ---------------------------------------------------------------------------------------------------------------------
# the samplers' filter
def filter_ref(row, temperature, top_k, top_p, exclude=(), multiply=False):
    """The reference rule (utils.py:101-128, excluded tokens -inf first) in float64 -> probabilities (V,).
    `multiply`: the prior's sense of the temperature (prior_relative.py:346 multiplies the logits by it)."""
    lg = torch.as_tensor(row, dtype=torch.float64).clone()
    lg = lg * temperature if multiply else lg / temperature
    lg[list(exclude)] = -float('inf')
    top_k = min(int(top_k), lg.numel())
    if top_k > 0:
        lg[lg < torch.topk(lg, top_k)[0][-1]] = -float('inf')
    if 0 < top_p < 1:
        srt, idx = torch.sort(lg, descending=True)
        cum = torch.cumsum(torch.softmax(srt, dim=-1), dim=-1)
        rm = cum > top_p
        rm[1:] = rm[:-1].clone()
        rm[0] = False
        lg[idx[rm]] = -float('inf')
    return torch.softmax(lg, dim=-1)


# ---------------------------------------------------------------------------------------------------------------------
# seeds and the draw
_M64 = (1 << 64) - 1


def splitmix64(z):
    """Steele, Lea & Flood's splitmix64 finaliser on Python ints (mod 2^64)."""
    z = (z + 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def _as_i64(v):
    v &= _M64
    return v - (1 << 64) if v >= 1 << 63 else v


def window_seed(seed, window):
    """The effective seed of a row in window `window` (int64 in, int64 out): window 0 keeps the row's seed, window w > 0
    draws from splitmix64(seed ^ (w * 0xD1B54A32D192ED03))."""
    sd = int(seed) & _M64
    if window == 0:
        return _as_i64(sd)
    return _as_i64(splitmix64(sd ^ ((int(window) * 0xD1B54A32D192ED03) & _M64)))


def rng_u24_ref(seed, pos):
    """The samplers' 24-bit draw (csrc/common.h: rng_x0, rng_u24_from_x0) for int64 seeds and positions (broadcast), in
    numpy uint32 arithmetic: x0 = pos * 0x9E3779B1 + lo32(seed); x = x0 ^ hi32(seed); x ^= x >> 16; y = mul24(x, 0x6B43A9);
    y ^= y >> 15; y = mul24(y, 0x52DCE7) + x; y ^= y >> 14; y >> 8, mul24 = the low 32 bits of the product of the low 24."""
    sd = np.asarray(seed, dtype=np.int64).astype(np.uint64)
    pos = np.asarray(pos, dtype=np.int64).astype(np.uint64)
    lo = (sd & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    hi = (sd >> np.uint64(32)).astype(np.uint32)
    p32 = (pos & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    m24 = np.uint32(0xFFFFFF)
    with np.errstate(over='ignore'):
        x = p32 * np.uint32(0x9E3779B1) + lo
        x = x ^ hi
        x = x ^ (x >> np.uint32(16))
        y = (x & m24) * np.uint32(0x6B43A9)
        y = y ^ (y >> np.uint32(15))
        y = (y & m24) * np.uint32(0x52DCE7) + x
        y = y ^ (y >> np.uint32(14))
    return (y >> np.uint32(8)).astype(np.int64)


# ---------------------------------------------------------------------------------------------------------------------
# the window moves (numpy int64 / float32 arrays; every array is copied, the updated state is returned as a dict)
def _clamp(v, lo, hi):
    return min(max(int(v), lo), hi)


def decode_window_ref(codes_full, chorale, win, advance, codes_win, tokens, U, P, prefix_rows, table, x, seeds_in, seeds_out,
                      pos):
    """codes_full (M, nb); chorale (M, ldch >= nb * U); win [next, live]; codes_win (M, S); tokens (M, T = S * U);
    prefix_rows (M, P) or None; table (rows, d), its last row the start-of-sentence row; x (M, ldx >= d); seeds (M,); pos int.
      commit  live >= 0 and live + S <= nb: chorale[m, live * U + j] = tokens[m, j] for j < clamp(pos, 0, T)
      stop    next < 0 or next + S > nb: nothing else changes
      load    codes_win = codes_full[:, next : next + S]; tokens = chorale[:, next * U : next * U + T]  (after the commit)
              prefix_rows[m, 0] = sos; prefix_rows[m, j + 1] = clamp(tokens[m, j] * U + j % U, 0, sos - 1) for j + 1 < P
              x[m, :d] = table[sos if P == 0 else clamp(tokens[m, P - 1] * U + (P - 1) % U, 0, sos - 1)]
              seeds_out[m] = window_seed(seeds_in[m], next); pos = P; win = [next + advance, next]"""
    st = dict(chorale=np.array(chorale), win=np.array(win), codes_win=np.array(codes_win), tokens=np.array(tokens),
              prefix_rows=None if prefix_rows is None else np.array(prefix_rows), x=np.array(x), seeds_out=np.array(seeds_out),
              pos=int(pos))
    M, nb = codes_full.shape
    S, T = st['codes_win'].shape[1], st['tokens'].shape[1]
    assert T == S * U
    d = table.shape[1]
    nxt, live = int(win[0]), int(win[1])
    cur = _clamp(pos, 0, T)
    if live >= 0 and live + S <= nb:
        st['chorale'][:, live * U:live * U + cur] = st['tokens'][:, :cur]
    if nxt < 0 or nxt + S > nb:
        return st
    sos = table.shape[0] - 1
    st['codes_win'][:] = codes_full[:, nxt:nxt + S]
    st['tokens'][:] = st['chorale'][:, nxt * U:nxt * U + T]
    for m in range(M):
        if P > 0:
            st['prefix_rows'][m, 0] = sos
            for j in range(P - 1):
                st['prefix_rows'][m, j + 1] = _clamp(int(st['tokens'][m, j]) * U + j % U, 0, sos - 1)
        row = sos if P == 0 else _clamp(int(st['tokens'][m, P - 1]) * U + (P - 1) % U, 0, sos - 1)
        st['x'][m, :d] = table[row]
        st['seeds_out'][m] = window_seed(int(seeds_in[m]), nxt)
    st['pos'] = P
    st['win'][:] = (nxt + advance, nxt)
    return st


def prior_window_ref(seq, nt, win, advance, codes_win, P, prefix_rows, table, x, seeds_in, seeds_out, pos):
    """seq (M, ldseq >= nt); codes_win (M, N); otherwise as decode_window_ref with the codes themselves as table rows:
      commit  live >= 0 and live + N <= nt: seq[m, live + j] = codes_win[m, j] for j < clamp(pos, 0, N)
      stop    next < 0 or next + N > nt
      load    codes_win = seq[:, next : next + N]; prefix_rows[m, 0] = sos, [m, j + 1] = clamp(codes_win[m, j], 0, sos - 1);
              x[m, :d] = table[sos if P == 0 else clamp(codes_win[m, P - 1], 0, sos - 1)]; seeds, pos, win as above"""
    st = dict(seq=np.array(seq), win=np.array(win), codes_win=np.array(codes_win),
              prefix_rows=None if prefix_rows is None else np.array(prefix_rows), x=np.array(x), seeds_out=np.array(seeds_out),
              pos=int(pos))
    M, N = st['codes_win'].shape
    d = table.shape[1]
    nxt, live = int(win[0]), int(win[1])
    cur = _clamp(pos, 0, N)
    if live >= 0 and live + N <= nt:
        st['seq'][:, live:live + cur] = st['codes_win'][:, :cur]
    if nxt < 0 or nxt + N > nt:
        return st
    sos = table.shape[0] - 1
    st['codes_win'][:] = st['seq'][:, nxt:nxt + N]
    for m in range(M):
        if P > 0:
            st['prefix_rows'][m, 0] = sos
            for j in range(P - 1):
                st['prefix_rows'][m, j + 1] = _clamp(int(st['codes_win'][m, j]), 0, sos - 1)
        row = sos if P == 0 else _clamp(int(st['codes_win'][m, P - 1]), 0, sos - 1)
        st['x'][m, :d] = table[row]
        st['seeds_out'][m] = window_seed(int(seeds_in[m]), nxt)
    st['pos'] = P
    st['win'][:] = (nxt + advance, nxt)
    return st
