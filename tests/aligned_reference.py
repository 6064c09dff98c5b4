"""Float64 numpy references of the aligned ("diagonal") cross block's kernels (csrc/aligned.hip; reference:
TransformerAlignedDecoderLayerCustom, VQCPCB/transformer/transformer_custom.py:389-492).

  expand(C, n, S, P, U, nc)        C (n * S, nc * d), feature index j * nc + v  ->  (n * P, d), row b * P + i = C[b * S + i // U, v::nc]
                                   with v = i % nc
  reduce(G, n, S, U, nc)           its adjoint for P = S * U: (n * S * U, d) -> (n * S, nc * d), events summed in ascending order
  reduce_abs(G, n, S, U, nc)       the same sum over |terms| (the error bound's scale)
  elu / elu_grad                   alpha = 1, with expm1
  step_add(h, C, pos, S, U, nc)    the generation step's form at one position
All take and return float64 unless the input dtype is kept on purpose (expand and step_add of fp32 inputs are exact copies /
one fp32 add, see the `dtype` argument).
"""
import numpy as np


def expand(C, n, S, P, U, nc, dtype=np.float64):
    C = np.asarray(C, dtype=dtype)
    d = C.shape[1] // nc
    assert C.shape == (n * S, nc * d) and U % nc == 0 and 0 <= P <= S * U
    out = np.zeros((n * P, d), dtype=dtype)
    for b in range(n):
        for i in range(P):
            out[b * P + i] = C[b * S + i // U, (i % nc)::nc]
    return out


def _terms(G, n, S, U, nc):
    """(n, S, epc, nc, d): the summands of every (code, voice, feature), events on axis 2."""
    G = np.asarray(G, dtype=np.float64)
    d = G.shape[1]
    assert G.shape[0] == n * S * U and U % nc == 0
    return G.reshape(n, S, U // nc, nc, d)


def _to_c_layout(x, n, S, nc):
    """(n, S, nc, d) -> (n * S, d * nc) with feature index j * nc + v."""
    return np.ascontiguousarray(x.transpose(0, 1, 3, 2)).reshape(n * S, -1)


def reduce(G, n, S, U, nc):
    t = _terms(G, n, S, U, nc)
    acc = t[:, :, 0].copy()
    for e in range(1, t.shape[2]):
        acc += t[:, :, e]
    return _to_c_layout(acc, n, S, nc)


def reduce_abs(G, n, S, U, nc):
    return _to_c_layout(np.abs(_terms(G, n, S, U, nc)).sum(axis=2), n, S, nc)


def elu(x):
    x = np.asarray(x, dtype=np.float64)
    return np.where(x > 0, x, np.expm1(np.minimum(x, 0.0)))


def elu_grad(x, g):
    x, g = np.asarray(x, dtype=np.float64), np.asarray(g, dtype=np.float64)
    return np.where(x > 0, g, g * np.exp(np.minimum(x, 0.0)))


def step_add(h, C, pos, S, U, nc, dtype=np.float64):
    h, C = np.asarray(h, dtype=dtype), np.asarray(C, dtype=dtype)
    M, d = h.shape
    assert C.shape == (M * S, nc * d) and 0 <= pos < S * U
    rows = C[np.arange(M) * S + pos // U]
    return h + rows[:, (pos % nc)::nc]
