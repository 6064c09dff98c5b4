"""float64 numpy restatement of vqcpc_decode_source_rows (include/vqcpc.h): the source rows of a decoder on continuous latents,
src[(b * S + j), n] = bias[n] + sum_k z_full[b, w0 + j, k] * w[n, k] on the live window [w0, w0 + S) of every sequence."""
import numpy as np


def source_rows(z_full, w, bias, S, w0=0):
    """z_full (M, nb, dz), w (N, dz), bias (N,) or None -> (M * S, N) float64, or None when the window does not fit (the
    kernel then writes nothing)."""
    z_full, w = np.asarray(z_full, np.float64), np.asarray(w, np.float64)
    M, nb, dz = z_full.shape
    if w0 < 0 or w0 + S > nb:
        return None
    out = np.zeros((M * S, w.shape[0]), np.float64)
    for b in range(M):
        for j in range(S):
            for n in range(w.shape[0]):
                acc = 0.0
                for k in range(dz):
                    acc += z_full[b, w0 + j, k] * w[n, k]
                out[b * S + j, n] = acc + (0.0 if bias is None else float(bias[n]))
    return out


def source_rows_fast(z_full, w, bias, S, w0=0):
    """The same numbers by matrix product (float64; summation order differs at the 1e-16 level), for the large cases."""
    z_full, w = np.asarray(z_full, np.float64), np.asarray(w, np.float64)
    M, nb, dz = z_full.shape
    if w0 < 0 or w0 + S > nb:
        return None
    out = z_full[:, w0:w0 + S].reshape(M * S, dz) @ w.T
    return out if bias is None else out + np.asarray(bias, np.float64)[None, :]


def error_bound(z_full, w, bias, S, w0=0):
    """(dz + 2) * 2^-24 * (sum_k |z_k w_nk| + |bias_n|): a length-dz fp32 dot product by FMA plus one addition."""
    z_full, w = np.abs(np.asarray(z_full, np.float64)), np.abs(np.asarray(w, np.float64))
    M, nb, dz = z_full.shape
    mag = z_full[:, w0:w0 + S].reshape(M * S, dz) @ w.T
    if bias is not None:
        mag = mag + np.abs(np.asarray(bias, np.float64))[None, :]
    return (dz + 2) * 2.0 ** -24 * mag
