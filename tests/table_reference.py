"""Plain references, in torch and numpy, for the kernels that index by token or code: the product quantiser (vqcpc_vq_fwd,
vqcpc_vq_bwd), the token tables (vqcpc_embed_pos_fwd / _bwd, vqcpc_block_table_gather / _segsum / _segsum_b16) and the plain
embedding gradient (vqcpc_embedding_bwd).  Every function takes `dtype`: torch.float64 is the reference, torch.float32 the SAME
formula in plain fp32 (sums by index_add_), the yardstick of tests/test_table_kernels_gpu.py.  Nothing here knows a launch
geometry: no chunk, no tile, no wave.

Every segment sum also returns, per output element, the 2-norm of its summands (`nrm`): the scale its rounding error is
proportional to, and exactly 0 where nothing is summed (the element must then be +0.0).

The second half builds the inputs of the GPU tests (case tables + builders).  tests/test_table_reference_cpu.py pins the
references against torch autograd, the oracle and the goldens, and verifies for EVERY case what the builders claim: ids in range,
planted unreferenced cells unreferenced, planted ties exact fp32 ties."""
import numpy as np
import torch

F64, F32 = torch.float64, torch.float32
VQ_EPS = 1e-5
U = 2.0 ** -24


def gamma(n):
    """n roundings of relative size u = 2^-24 each: (1 + u)^n - 1 <= n u / (1 - n u)."""
    return n * U / (1.0 - n * U)


def gen(seed):
    return torch.Generator().manual_seed(seed)


def seg_sum(vals, keys, n, dtype=F64):
    """out[k] = sum of vals[i] over keys[i] == k (vals (N, W), keys (N,)) -> (n, W) in dtype, and the 2-norm of each element's
    summands in float64."""
    vals = torch.as_tensor(vals)
    out = torch.zeros(n, vals.shape[1], dtype=dtype).index_add_(0, keys, vals.to(dtype))
    v64 = vals.double()
    return out, torch.sqrt(torch.zeros(n, vals.shape[1], dtype=F64).index_add_(0, keys, v64 * v64))


def seg_err(out, ref64, nrm):
    """Per element |out - ref| / nrm over the elements that have summands -> 1-d float64 tensor."""
    out, ref64 = torch.as_tensor(out).double().reshape(-1), torch.as_tensor(ref64).double().reshape(-1)
    live = nrm.reshape(-1) > 0
    return (out[live] - ref64[live]).abs() / nrm.reshape(-1)[live]


def is_pos_zero(t):
    """Every element is +0.0 (bit pattern 0)."""
    return bool((torch.as_tensor(t).float().contiguous().view(torch.int32) == 0).all())


# =====================================================================================================================
# product quantiser.  z (R, D), cb (ncb, K, dsub), idx (R, ncb)
def _eps(eps, dtype):
    """The kernels' constant is 1e-5f, the fp32 value; eps = 1e-5 (a double) is the oracle's expression evaluated in float64."""
    return torch.tensor(VQ_EPS, dtype=F32).to(dtype) if eps is None else torch.tensor(eps, dtype=dtype)


def vq_distances(z, cb, dtype=F64):
    """(R, ncb, K): sum_t (z_t - e_t)^2 per codebook."""
    ncb, K, dsub = cb.shape
    x = z.to(dtype).reshape(z.shape[0], ncb, 1, dsub)
    return ((x - cb.to(dtype).unsqueeze(0)) ** 2).sum(-1)


def vq_argmin(z, cb):
    """float64 argmin (first index) and the float64 minimum -> (R, ncb) int64, (R, ncb) float64."""
    d = vq_distances(z, cb)
    m, i = d.min(-1)
    return i, m


def vq_quantized(cb, idx, dtype=F64):
    """(R, D): the chosen codes side by side."""
    return torch.cat([cb[c].to(dtype)[idx[:, c]] for c in range(cb.shape[0])], 1)


def vq_fwd(z, cb, idx, beta, squared, dtype=F64, eps=None):
    """-> zq = z + (q - z), loss (R,).  squared: q_latent + beta * e_latent with both = sum (q - z)^2; else the norm of
    (q - z) + 1e-5."""
    zz, q = z.to(dtype), vq_quantized(cb, idx, dtype)
    diff = q - zz
    if squared:
        l = (diff * diff).sum(1)
    else:
        v = diff + _eps(eps, dtype)
        l = torch.sqrt((v * v).sum(1))
    return zz + diff, l + torch.tensor(beta, dtype=F32).to(dtype) * l


def vq_zq_bits(z, cb, idx):
    """fl(z + fl(q - z)) in fp32, as numpy computes it (one rounding per operation)."""
    zn, qn = z.numpy().astype(np.float32), vq_quantized(cb, idx, F32).numpy()
    return torch.from_numpy((zn + (qn - zn).astype(np.float32)).astype(np.float32))


def vq_bwd(z, cb, idx, g_zq, g_loss, beta, squared, dtype=F64, eps=None):
    """-> d_z (R, D), d_cb (ncb, K, dsub), nrm (ncb, K, dsub), T (R, D).
    dq = d loss_q / d q: 2 (q - z) or ((q - z) + eps) / ||(q - z) + eps||;  d_z = g_zq - g_loss beta dq;  d_cb[c][k] = sum over
    the rows with idx[r][c] == k of g_loss[r] dq[r][c].  T = g_loss beta dq, the term subtracted in d_z (for the derived bound)."""
    ncb, K, dsub = cb.shape
    zz, q = z.to(dtype), vq_quantized(cb, idx, dtype)
    diff = q - zz
    if squared:
        dq = 2.0 * diff
    else:
        v = diff + _eps(eps, dtype)
        dq = v / torch.sqrt((v * v).sum(1, keepdim=True))
    gl = g_loss.to(dtype).unsqueeze(1)
    T = gl * torch.tensor(beta, dtype=F32).to(dtype) * dq
    val = gl * dq
    d_cb, nrm = [], []
    for c in range(ncb):
        s, n = seg_sum(val[:, c * dsub:(c + 1) * dsub], idx[:, c], K, dtype)
        d_cb.append(s), nrm.append(n)
    return g_zq.to(dtype) - T, torch.stack(d_cb), torch.stack(nrm), T


# =====================================================================================================================
# token tables
def embed_pos_fwd(tokens, tpb, nv, table, chan, event):
    """out[r] = [table[v][tokens[r]] | chan[v] | event[e]], p = r % tpb, v = p % nv, e = p // nv; event None: no event part."""
    r = torch.arange(tokens.shape[0])
    p = r % tpb
    v, e = p % nv, p // nv
    parts = [table[v, tokens], chan[v]] + ([event[e]] if event is not None else [])
    return torch.cat(parts, 1)


def embed_pos_bwd(tokens, tpb, nv, vmax, dlin, pos, g, has_ev, dtype=F64):
    """-> dict d_table (nv, vmax, dlin), d_chan (nv, pos), d_event (tpb / nv, pos) or None, and n_table / n_chan / n_event, the
    norms of the summands."""
    r = torch.arange(tokens.shape[0])
    p = r % tpb
    v, e = p % nv, p // nv
    out = {}
    t, n = seg_sum(g[:, :dlin], v * vmax + tokens, nv * vmax, dtype)
    out['d_table'], out['n_table'] = t.reshape(nv, vmax, dlin), n.reshape(nv, vmax, dlin)
    out['d_chan'], out['n_chan'] = seg_sum(g[:, dlin:dlin + pos], v, nv, dtype)
    out['d_event'], out['n_event'] = seg_sum(g[:, dlin + pos:], e, tpb // nv, dtype) if has_ev else (None, None)
    return out


def block_gather(table, tokens, L):
    """out[r] = table[tokens[r] * L + r % L]."""
    return table[tokens * L + torch.arange(tokens.shape[0]) % L]


def block_segsum(g, tokens, L, vmax, dtype=F64):
    """d_table[t * L + p] = sum over r with tokens[r] == t and r % L == p of g[r] -> (vmax * L, C), nrm."""
    return seg_sum(g, tokens * L + torch.arange(tokens.shape[0]) % L, vmax * L, dtype)


def embedding_bwd(g, idx, V, dtype=F64):
    """d_table[v] = sum over m with idx[m] == v of g[m] -> (V, C), nrm."""
    return seg_sum(g, idx, V, dtype)


def embedding_bwd_replay(g, idx, V):
    """The order include/vqcpc.h fixes: a stable sort, and every row's sum taken in ascending m, one fp32 add at a time starting
    from +0.0 -> (V, C) float32."""
    gn = torch.as_tensor(g).numpy().astype(np.float32)
    out = np.zeros((V, gn.shape[1]), np.float32)
    sidx, perm = torch.sort(idx, stable=True)
    sidx, perm = sidx.numpy(), perm.numpy()
    start = np.flatnonzero(np.r_[True, sidx[1:] != sidx[:-1]]) if len(sidx) else np.zeros(0, np.int64)
    length = np.diff(np.r_[start, len(sidx)])
    for j in range(int(length.max()) if len(length) else 0):
        sel = length > j
        rows = perm[start[sel] + j]
        out[sidx[start[sel]]] = (out[sidx[start[sel]]] + gn[rows]).astype(np.float32)
    return torch.from_numpy(out)


def bf16_trunc_values(x):
    """Values exactly representable in bf16 (the low 16 bits cleared) -> fp32 tensor and its bf16 patterns as int16."""
    b = torch.as_tensor(x).float().contiguous().view(torch.int32) & ~0xFFFF
    return b.view(F32), (b >> 16).to(torch.int16)


# =====================================================================================================================
# inputs of the GPU tests
# ---- vq_fwd: (label, R, ncb, K, dsub).  dsub 3 4 8 16 32 64: the specialised instantiations (KU = 4 unrolled scan: 16 codes a
# step, so K around 16 and 32); every other dsub: the generic one.  K * dsub * 4 > 64 KiB: the hipFuncSetAttribute path; 36 864
# floats = 144 KiB is the largest codebook the host accepts.
VQ_FWD_DSUB = [(f'dsub{d}', (65, 257, 63, 64, 1)[i % 5], (2, 1, 4)[i % 3], 33, d)
               for i, d in enumerate([3, 4, 8, 16, 32, 64, 1, 5, 12, 128])]
VQ_FWD_K = [(f'K{K}', (1, 63, 64, 65, 257)[i % 5], (1, 2, 4)[i % 3], K, dsub)
            for i, K in enumerate([1, 2, 3, 4, 5, 15, 16, 17, 31, 33, 100]) for dsub in (4, 5)]
VQ_FWD_BIG = [('2048x16', 65, 2, 2048, 16), ('512x64', 63, 1, 512, 64), ('2304x16 (144 KiB)', 64, 1, 2304, 16),
              ('288x128 (144 KiB, generic)', 65, 2, 288, 128)]


def vq_fwd_inputs(case):
    """The inputs of one vq_fwd case of the tables above, for the CPU check and the GPU test alike (the seed is the case's place in
    VQ_FWD_DSUB + VQ_FWD_K + VQ_FWD_BIG) -> z, cb, plan, given: `given` (R, ncb) are the in-range indices of the assign = 0 launches."""
    seed = (VQ_FWD_DSUB + VQ_FWD_K + VQ_FWD_BIG).index(case)
    _, R, ncb, K, dsub = case
    z, cb, plan = vq_fwd_case(R, ncb, K, dsub, seed)
    return z, cb, plan, torch.randint(0, K, (R, ncb), generator=gen(7700 + seed))


def vq_fwd_case(R, ncb, K, dsub, seed):
    """-> z, cb, plan.  Planted, per codebook, as far as K and R allow:
      ties:      code `dup[1]` is a copy of code `dup[0]` (dup[0] < dup[1]); the rows `tie_rows` sit near it, so the two equal
                 distances are the row's minimum and the FIRST index must win;
      on a code: the rows `on_rows` ARE code on_k (distance exactly 0);
      near-ties: code `near[1]` is code `near[0]` with coordinate 0 moved by one ulp; the rows `near_rows` sit near both, so the
                 two are the two smallest distances of the row."""
    g = gen(seed)
    z = torch.randn(R, ncb * dsub, generator=g)
    cb = torch.randn(ncb, K, dsub, generator=g)
    plan = []
    for c in range(ncb):
        p = dict(dup=None, tie_rows=[], on_k=None, on_rows=[], near=None, near_rows=[])
        sl = slice(c * dsub, (c + 1) * dsub)
        if K >= 2:
            a, b = sorted(torch.randperm(K, generator=g)[:2].tolist())
            cb[c, b] = cb[c, a]
            p['dup'], p['tie_rows'] = (a, b), list(range(0, R, 5))
            for r in p['tie_rows']:
                z[r, sl] = cb[c, a] + 1e-4 * torch.randn(dsub, generator=g)
        if K >= 4:
            rest = [k for k in torch.randperm(K, generator=g).tolist() if k not in p['dup']]
            a, b = rest[0], rest[1]
            cb[c, b] = cb[c, a]
            cb[c, b, 0] = torch.from_numpy(np.nextafter(cb[c, a, 0:1].numpy(), np.float32(np.inf)))
            p['near'], p['near_rows'] = (a, b), list(range(1, R, 5))
            for r in p['near_rows']:
                z[r, sl] = cb[c, a] + 1e-4 * torch.randn(dsub, generator=g)
        p['on_k'], p['on_rows'] = int(torch.randint(0, K, (1,), generator=g)), list(range(2, R, 5))
        for r in p['on_rows']:
            z[r, sl] = cb[c, p['on_k']]
        plan.append(p)
    return z, cb, plan


# ---- vq_bwd: (label, R, ncb, K, dsub, pattern).  kgroups = 256 // dsub: 256, 85, 51, 21, 16, 4 and, above 128, 1.  The kernel
# stages 256 rows x dsub next to the K x dsub accumulator, so dsub (K + 256) + 256 floats must fit 160 KiB: dsub <= 158 at K = 1.
# dsub = 200 and 256 (and anything larger) can never fit: VQ_BWD_REFUSED.  150 and 158 take their place as the
# kgroups = 1 cases.
VQ_BWD_DSUBS = [1, 3, 5, 12, 16, 64, 150, 158]
VQ_BWD_REFUSED = [(200, 1), (256, 1), (159, 1), (158, 2), (300, 1)]                    # (dsub, K): over 160 KiB of LDS


def vq_bwd_cases(dsub):
    Rs, pats = (1, 255, 256, 257, 513), ('one', 'random', 'own')
    i = VQ_BWD_DSUBS.index(dsub)
    out = []
    for j, K in enumerate((1, 7, 128)):
        if (K * dsub + 256 * dsub + 256) * 4 > 160 * 1024:
            continue
        for s, R in enumerate(Rs):
            pat = pats[(i + j + s) % 3]
            if pat == 'own' and R > K:
                pat = 'one' if K == 1 else 'random'
            if pat == 'random' and K == 1:
                pat = 'one'
            out.append((f'dsub{dsub} K{K} R{R} {pat}', R, (1, 2, 4)[(i + j + s) % 3] if dsub <= 16 else 1, K, dsub, pat))
    K = 7 if (7 * dsub + 256 * dsub + 256) * 4 <= 160 * 1024 else 1
    out.append((f'dsub{dsub} K{K} R1 own', 1, 2 if dsub <= 16 else 1, K, dsub, 'own'))
    # every row on a code of its own with more than one row: the largest K of the three that fits, R just below it
    K = max(k for k in (1, 7, 128) if (k * dsub + 256 * dsub + 256) * 4 <= 160 * 1024)
    if K > 1:
        out.append((f'dsub{dsub} K{K} R{K - 2} own', K - 2, 2 if dsub <= 16 else 1, K, dsub, 'own'))
    return out


def vq_bwd_inputs(case):
    """The inputs of one vq_bwd case (vq_bwd_cases(dsub) or VQ_BWD_BIG), for the CPU check and the GPU test alike: the seed is a
    function of the case's own numbers -> z, cb, idx, g_zq, g_loss."""
    _, R, ncb, K, dsub, pattern = case
    return vq_bwd_case(R, ncb, K, dsub, pattern, 100000 * dsub + 100 * R + 10 * K + ncb + ('one', 'random', 'own').index(pattern) * 7)


VQ_BWD_BIG = [('2048x16 R513 own', 513, 1, 2048, 16, 'own'), ('2048x16 R257 random', 257, 2, 2048, 16, 'random')]


def vq_bwd_case(R, ncb, K, dsub, pattern, seed):
    """-> z, cb, idx, g_zq, g_loss (g_loss is 0 in the rows 1, 4, 7, ..: row 0 always counts, R = 1 included).  pattern 'one': every row on one code; 'own': every row on a code of
    its own (R <= K); 'random': random over three quarters of the codes, so at least a quarter is never chosen."""
    g = gen(seed)
    z = torch.randn(R, ncb * dsub, generator=g)
    cb = torch.randn(ncb, K, dsub, generator=g)
    idx = torch.empty(R, ncb, dtype=torch.int64)
    for c in range(ncb):
        if pattern == 'one':
            idx[:, c] = int(torch.randint(0, K, (1,), generator=g))
        elif pattern == 'own':
            idx[:, c] = torch.randperm(K, generator=g)[:R]
        else:
            allowed = torch.randperm(K, generator=g)[:K - (K + 3) // 4]
            idx[:, c] = allowed[torch.randint(0, len(allowed), (R,), generator=g)]
    g_zq = torch.randn(R, ncb * dsub, generator=g)
    g_loss = torch.randn(R, generator=g)
    g_loss[1::3] = 0.0
    return z, cb, idx, g_zq, g_loss


# ---- block table: (label, L, vmax, C, n_blocks, distribution).  fp32: 1 KiB of LDS per token (vmax > 64: over 64 KiB, 160: all
# 160 KiB of a CU); bf16: 2 KiB per token (80: all of it).  segsum_chunks = min(32, n_blocks // 256): 1 up to 511, 2 from 512 (256 +
# 256 blocks; 513: 257 + 256), 32 at 8193 (chunks of 257, the last of 226).  32 rows in flight: 31 / 32 / 33 blocks.
SEG_F32 = [(1, 1, 1, 1, 'one'), (4, 2, 5, 31, 'uniform'), (16, 57, 96, 32, 'unused'), (4, 57, 256, 33, 'uniform'),
           (1, 100, 260, 255, 'unused'), (4, 160, 5, 511, 'unused'), (1, 160, 768, 33, 'uniform'), (4, 2, 1, 512, 'one'),
           (16, 57, 5, 513, 'unused'), (1, 100, 96, 8193, 'uniform'), (4, 1, 260, 32, 'one'), (16, 2, 96, 255, 'uniform')]
SEG_B16 = [(1, 1, 2, 1, 'one'), (4, 57, 6, 513, 'unused'), (16, 80, 510, 31, 'uniform'), (4, 80, 2, 8193, 'unused'),
           (1, 57, 512, 511, 'uniform'), (4, 57, 514, 33, 'one'), (1, 80, 6, 512, 'uniform'), (16, 1, 514, 32, 'one'),
           (4, 57, 512, 255, 'unused')]


def seg_case(L, vmax, C, n_blocks, dist, seed):
    """-> tokens (n_blocks * L,), g (M, C), unused tokens, unused (token, position) cells.  'one': one token on every row;
    'unused': the tokens of `dead` never occur and the cells of `dead_cells` (token, position) never either."""
    g = gen(seed)
    M = n_blocks * L
    dead, dead_cells = [], []
    if dist == 'one':
        t0 = int(torch.randint(0, vmax, (1,), generator=g))
        tokens = torch.full((M,), t0, dtype=torch.int64)
        dead = [t for t in range(vmax) if t != t0]
    elif dist == 'uniform' or vmax < 4:
        tokens = torch.randint(0, vmax, (M,), generator=g)
    else:
        dead = sorted({0, vmax // 2, vmax - 1})
        allowed = torch.tensor([t for t in range(vmax) if t not in dead])
        tokens = allowed[torch.randint(0, len(allowed), (M,), generator=g)]
        dead_cells = [(int(allowed[1]), 0), (int(allowed[-1]), L - 1), (int(allowed[2]), L // 2)]
        pos = torch.arange(M) % L
        for t, p in dead_cells:
            tokens[(tokens == t) & (pos == p)] = int(allowed[0])           # allowed[0] is the token of no dead cell
    return tokens, torch.randn(M, C, generator=g), dead, dead_cells


# ---- embed_pos: (label, tpb, nv, pos, dlin, has_ev, n_rows); d = dlin + (2 or 1) pos.  d % 64 in [1, 15]: the PARTIAL
# instantiation.  Chunks: n_rows < 65 536: chunk = ceil(ceil(n_rows / 48) / tpb) tpb rows (47 and 48 blocks: one block a chunk; 49
# blocks: two, the last chunk ragged); from 65 536 on 2048 rows a chunk.
EMB_VMAX = 11
EMB_CASES = [('one block d32', 16, 4, 8, 16, True, 16),
             ('47 blocks d12 partial, one event', 4, 4, 4, 4, True, 4 * 47),
             ('48 blocks d12 partial, nv1, no event', 8, 1, 4, 8, False, 8 * 48),
             ('49 blocks d64', 64, 4, 8, 48, True, 64 * 49),
             ('one block of 2048, d40, no event', 2048, 4, 4, 36, False, 2048),
             ('47 blocks d68 partial, no event', 16, 4, 8, 60, False, 16 * 47),
             ('48 blocks d16', 16, 4, 4, 8, True, 16 * 48),
             ('65536-16 rows d32', 16, 4, 8, 16, True, 65536 - 16),
             ('65536 rows d32', 16, 4, 8, 16, True, 65536),
             ('65536+16 rows d32, ragged 2048-row chunk, no event', 16, 4, 8, 24, False, 65536 + 16),
             ('one block d260 partial, second column pass', 4, 4, 8, 244, True, 4),
             ('49 blocks d80, nv1', 8, 1, 8, 64, True, 8 * 49),
             ('one block d76 partial', 64, 4, 4, 68, True, 64),
             ('3 blocks of 2048, d64', 2048, 4, 8, 48, True, 3 * 2048),
             ('one block d64, no event', 16, 4, 8, 56, False, 16),
             ('2 blocks d16, no event', 16, 4, 4, 12, False, 32),
             ('one block d40', 16, 4, 8, 24, True, 16)]


def emb_case(tpb, nv, pos, dlin, has_ev, n_rows, seed):
    """-> tokens, table, chan, event (or None), g, dead: voice v never sees the ids dead[v] = {(v + 1) % vmax, vmax - 1}."""
    g = gen(seed)
    vmax = EMB_VMAX
    v = torch.arange(n_rows) % tpb % nv
    dead = [sorted({(u + 1) % vmax, vmax - 1}) for u in range(nv)]
    tokens = torch.randint(0, vmax, (n_rows,), generator=g)
    for u in range(nv):
        ok = torch.tensor([t for t in range(vmax) if t not in dead[u]])
        sel = v == u
        tokens[sel] = ok[torch.randint(0, len(ok), (int(sel.sum()),), generator=g)]
    d = dlin + (2 if has_ev else 1) * pos
    table, chan = torch.randn(nv, vmax, dlin, generator=g), torch.randn(nv, pos, generator=g)
    event = torch.randn(tpb // nv, pos, generator=g) if has_ev else None
    return tokens, table, chan, event, torch.randn(n_rows, d, generator=g), dead


# ---- embedding_bwd: (M, C, ldg - C, V, pattern).  U = 8 rows in flight: runs of 1, 8, 9, 17 and M; C > 256: a second column pass.
EMBG_CASES = [(0, 1, 0, 1, 'same'), (0, 257, 3, 5, 'same'), (1, 1, 0, 1, 'same'), (1, 600, 3, 5, 'same'), (7, 255, 3, 5, 'same'),
              (8, 256, 0, 5, 'same'), (9, 257, 3, 1, 'same'), (9, 600, 0, 5, 'mixed'), (1000, 1, 3, 100000, 'mixed'),
              (1000, 256, 0, 100000, 'mixed'), (1000, 600, 3, 5, 'mixed'), (1000, 255, 0, 5, 'mixed'), (1000, 257, 3, 1, 'same'),
              (1000, 257, 3, 5, 'same')]


def embg_case(M, C, gap, V, pattern, seed):
    """-> g (M, C), idx (M,), runs {value: length}.  'same': one value on every row (a run of M that ends at M).  'mixed': values
    with runs of exactly 1, 8, 9 and 17 (as far as M allows), the rest spread over a few more values; the largest value's run ends at
    M in sorted order; at least one row of the table stays unreferenced when V > 1."""
    g = gen(seed)
    if pattern == 'same' or V == 1:
        idx = torch.full((M,), int(torch.randint(0, V, (1,), generator=g)) if M else 0, dtype=torch.int64)
    else:
        vals = torch.randperm(V, generator=g)[:min(V - 1, 40)].tolist()           # V - 1 at most: one row stays unreferenced
        parts, nval = [], 0
        for n in (1, 8, 9, 17):
            if len(parts) + n <= M and nval < len(vals) - 1:
                parts += [vals[nval]] * n
                nval += 1
        rest = vals[nval:]
        parts += [rest[int(i)] for i in torch.randint(0, len(rest), (M - len(parts),), generator=g)]
        idx = torch.tensor(parts, dtype=torch.int64)[torch.randperm(M, generator=g)]
    runs = {int(v): int(n) for v, n in zip(*np.unique(idx.numpy(), return_counts=True))}
    return torch.randn(M, C, generator=g), idx, runs
