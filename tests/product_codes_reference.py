"""Restatements of the product-code kernels (csrc/product_codes.hip, ops.ProductEmbeddingFn, quantizer/product_embedding.py) in
numpy fp32 (the kernels' own order of operations: the expected BITS) and float64 (the exact value, for derived bounds).

A merged code of ncb codebooks of K codewords is ncb digits, digit j = (code // K**j) % K (Encoder.merge_codes); V = K**ncb;
indices V <= i < V + n_extra address the extra (start-of-sentence) rows.  tests/test_product_codes_reference_cpu.py pins the
float64 functions on torch float64 autograd over nn.Embedding sums.

Error model: u = 2^-24; fl(a + b) = (a + b)(1 + d), |d| <= u; no underflow at the magnitudes of the tests.
"""
import numpy as np

U = 2.0 ** -24


def digits(idx, ncb, K):
    """idx (M,) int64 merged codes -> (ncb, M) int64 digits, digit j = (idx // K**j) % K."""
    idx = np.asarray(idx, dtype=np.int64)
    return np.stack([(idx // K ** j) % K for j in range(ncb)])


def merge(dig, K):
    """(ncb, M) digits -> (M,) merged codes."""
    return sum(np.asarray(d, dtype=np.int64) * K ** j for j, d in enumerate(dig))


def gather(tables, idx, nj=None, res=None, extra=None, dtype=np.float32):
    """tables (ncb, K, C), idx (M,) -> (M, C): (res[m] +) tables[0][c_0] + ... + tables[nj-1][c_{nj-1}], left to right, one add of
    `dtype` each; without res the chain starts AT the first row; rows idx >= V are extra[idx - V].  dtype=np.float32 gives the
    kernel's bits (numpy adds fp32 arrays in fp32, one IEEE rounding per element), np.float64 the exact chain."""
    tables = np.asarray(tables, dtype=dtype)
    ncb, K, C = tables.shape
    nj = ncb if nj is None else nj
    idx = np.asarray(idx, dtype=np.int64)
    V = K ** ncb
    code = idx < V
    dig = digits(np.where(code, idx, 0), ncb, K)
    acc = tables[0][dig[0]]
    if res is not None:
        acc = np.asarray(res, dtype=dtype) + acc
    for j in range(1, nj):
        acc = acc + tables[j][dig[j]]
    if extra is not None:
        acc = acc.copy()
        acc[~code] = np.asarray(extra, dtype=dtype)[idx[~code] - V]
    return acc


def segment_sums(g, idx, ncb, K, nj=None, n_extra=0):
    """Float64 gradient of `gather` for the tables and the extra rows: g (M, C), idx (M,) ->
    d_tables (ncb, K, C), d_extra (n_extra, C), and per cell the number of summands n_tables (ncb, K), n_extra_rows (n_extra,)
    and the sums of |g| a_tables, a_extra (the scale of `sum_bound`).  Codebooks j >= nj stay 0."""
    g = np.asarray(g, dtype=np.float64)
    idx = np.asarray(idx, dtype=np.int64)
    M, C = g.shape
    nj = ncb if nj is None else nj
    V = K ** ncb
    d_t, a_t, n_t = np.zeros((ncb, K, C)), np.zeros((ncb, K, C)), np.zeros((ncb, K))
    d_e, a_e, n_e = np.zeros((n_extra, C)), np.zeros((n_extra, C)), np.zeros(n_extra)
    for m in range(M):
        if idx[m] >= V:
            e = idx[m] - V
            d_e[e] += g[m]
            a_e[e] += np.abs(g[m])
            n_e[e] += 1
            continue
        for j in range(nj):
            k = (idx[m] // K ** j) % K
            d_t[j, k] += g[m]
            a_t[j, k] += np.abs(g[m])
            n_t[j, k] += 1
    return d_t, d_e, (n_t, a_t), (n_e, a_e)


def sum_bound(counts, abs_sums):
    """|fp32 sum - exact sum| per element of a cell, the bound of tests/vq_ema_reference.sum_bound (the same structure: a sum of n
    fp32 values, here 0 + g[m_1] + g[m_2] + ... in ascending m, whose first add is exact): every summand passes through at most
    n - 1 rounded additions, so |err| <= gamma_(n-1) sum|g| <= n u sum|g| for n < 2^23."""
    return np.asarray(counts)[..., None] * U * np.asarray(abs_sums)


# ---------------------------------------------------------------------------------------------------------------------------
# the prior over product codes (priors/prior_relative.py, code_model = 'product'), in torch so that autograd gives the gradients
def prior_forward(P, codes, ncb, K, stack):
    """The factorised prior in the dtype of the tensors of P (float64 for a reference).  P: state-dict names -> tensors
    (embedding.weight (ncb, K, emb), linear.*, sos, pre_softmaxes.j.*, digit_embeddings.weight (ncb - 1, K, d)); codes (B, N)
    int64 merged codes; stack: (B, N, d) input rows -> (B, N, d) outputs of the causal stack.
    -> (loss, [logits_j (B, N, K)], logp (B, N)): input row of a code = linear(sum_j E_j[c_j]), shifted by one behind the
    start-of-sentence row; stage j's logits = head_j(h + sum_{i<j} D_i[c_i]) on the SAME position's digits; loss = sum_j mean
    CE_j; logp = sum_j log_softmax(logits_j)[c_j], the log-probability of each code given the codes before it."""
    import torch
    B, N = codes.shape
    dig = [(codes // K ** j) % K for j in range(ncb)]
    E = P['embedding.weight']
    emb = sum(E[j][dig[j]] for j in range(ncb))                                           # (B, N, emb)
    rows = emb @ P['linear.weight'].t() + P['linear.bias']
    x = torch.cat([P['sos'].reshape(1, 1, -1).expand(B, 1, -1), rows[:, :-1]], dim=1)
    h = stack(x)
    loss, logits, logp = 0.0, [], 0.0
    for j in range(ncb):
        hj = h if j == 0 else hj + P['digit_embeddings.weight'][j - 1][dig[j - 1]]
        lg = hj @ P[f'pre_softmaxes.{j}.weight'].t() + P[f'pre_softmaxes.{j}.bias']
        ls = torch.log_softmax(lg, dim=-1).gather(-1, dig[j].unsqueeze(-1)).squeeze(-1)    # (B, N)
        loss = loss - ls.mean()
        logp = logp + ls
        logits.append(lg)
    return loss, logits, logp
