"""Pins tests/table_reference.py without a GPU: against torch float64 autograd (F.embedding, index_add_, the cat expression of
the fused embedding), against oracle.vqcpc_oracle (vq_forward / vq_assign) and the vq_* goldens -- agreement 1e-12, integers and
fp32 bit patterns exact -- and verifies, for EVERY parametrised case of tests/test_table_kernels_gpu.py, what the input builders
claim: every id in range, every planted unreferenced cell unreferenced, every planted tie an exact fp32 tie."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import table_reference as R
from conftest import load_golden
from oracle import vqcpc_oracle as O

TOL = 1e-12
F64 = torch.float64


def close(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return a.shape == b.shape and float((a - b).abs().max() if a.numel() else 0.0) <= TOL * max(1.0, float(b.abs().max() if b.numel() else 0.0))


# =====================================================================================================================
# quantiser
@pytest.mark.parametrize('squared', [True, False])
@pytest.mark.parametrize('ncb,K,dsub', [(1, 1, 3), (2, 7, 5), (4, 33, 16)])
def test_vq_reference_against_the_oracle_in_float64(ncb, K, dsub, squared):
    z, cb, idx, g_zq, g_loss = R.vq_bwd_case(37, ncb, K, dsub, 'random' if K > 1 else 'one', 5)
    zd = z.double().requires_grad_(True)
    cbs = [cb[c].double().requires_grad_(True) for c in range(ncb)]
    zq, _, loss = O.vq_forward(zd, cbs, beta=0.25, squared=squared, idx=idx)
    mine_zq, mine_loss = R.vq_fwd(z, cb, idx, 0.25, squared, eps=1e-5)
    assert close(mine_zq, zq.detach()) and close(mine_loss, loss.detach())
    ((zq * g_zq.double()).sum() + (loss * g_loss.double()).sum()).backward()
    d_z, d_cb, nrm, T = R.vq_bwd(z, cb, idx, g_zq, g_loss, 0.25, squared, eps=1e-5)
    assert close(d_z, zd.grad) and close(d_cb, torch.stack([c.grad for c in cbs]))
    assert close(d_z, g_zq.double() - T)
    # the summands: their squares add up to nrm^2, and a code no row chose has none
    chosen = torch.zeros(ncb, K, dtype=torch.bool)
    for c in range(ncb):
        chosen[c, idx[:, c]] = True
    assert bool((nrm[~chosen] == 0).all()) and bool((d_cb[~chosen] == 0).all())
    # the fp32 constant the kernels use moves the non-squared loss by less than 1e-10 and nothing else
    assert float((R.vq_fwd(z, cb, idx, 0.25, squared)[1] - mine_loss).abs().max()) < 1e-10


def test_vq_distances_and_argmin_against_the_oracle():
    z, cb, _ = R.vq_fwd_case(65, 2, 33, 16, 3)
    d64 = R.vq_distances(z, cb)
    for c in range(2):
        canon = O.vq_distances_canonical(z[:, c * 16:(c + 1) * 16].contiguous(), cb[c])
        assert float((canon.double() - d64[:, c]).abs().max() / d64[:, c].max()) < R.gamma(18)
        want = ((z[:, None, c * 16:(c + 1) * 16].double() - cb[c][None].double()) ** 2).sum(-1)
        assert close(d64[:, c], want)
    i64, m64 = R.vq_argmin(z, cb)
    assert torch.equal(m64, d64.min(-1)[0]) and torch.equal(torch.gather(d64, 2, i64.unsqueeze(-1)).squeeze(-1), m64)


@pytest.mark.parametrize('name', ['vq_ncb1', 'vq_ncb2', 'vq_ncb2_d32', 'vq_wide_d64', 'vq_ties', 'vq_l2norm'])
def test_vq_reference_against_the_goldens(name):
    g = load_golden(name)
    cb = torch.from_numpy(g['codebooks'].copy())
    ncb, K, dsub = cb.shape
    z = torch.from_numpy(g['z']).reshape(-1, ncb * dsub)
    idx = torch.from_numpy(g['idx']).reshape(-1, ncb)
    beta, squared = float(g['beta']), bool(g['squared'])
    assert torch.equal(O.vq_assign(z, list(cb)), idx)
    # the golden index is the float64 argmin wherever the two best distances are clearly apart, and never worse than the fp32
    # chain allows
    d64 = R.vq_distances(z, cb)
    i64, m64 = R.vq_argmin(z, cb)
    top2 = torch.sort(d64, -1)[0]
    clear = (top2[..., 1] - top2[..., 0]) > 4 * R.gamma(dsub + 2) * top2[..., 1] if K > 1 else torch.ones_like(m64, dtype=torch.bool)
    assert torch.equal(i64[clear], idx[clear])
    chosen = torch.gather(d64, 2, idx.unsqueeze(-1)).squeeze(-1)
    assert bool((chosen <= m64 * (1 + R.gamma(dsub + 2)) / (1 - R.gamma(dsub + 2)) + 1e-300).all())
    assert torch.equal(R.vq_zq_bits(z, cb, idx).view(torch.int32), torch.from_numpy(g['zq']).reshape(z.shape).view(torch.int32))
    zq64, loss64 = R.vq_fwd(z, cb, idx, beta, squared, eps=1e-5)
    ozq, _, oloss = O.vq_forward(z.double(), [c.double() for c in cb], beta=beta, squared=squared, idx=idx)
    assert close(zq64, ozq) and close(loss64, oloss)
    # the recorded fp32 results lie within fp32 rounding of the float64 reference
    assert float(((loss64 - torch.from_numpy(g['loss']).reshape(-1).double()).abs() / loss64.abs().clamp_min(1e-30)).max()) < R.gamma(ncb * dsub + 8)
    d_z, d_cb, _, _ = R.vq_bwd(z, cb, idx, torch.from_numpy(g['g_zq']).reshape(z.shape), torch.from_numpy(g['g_loss']).reshape(-1), beta,
                               squared, eps=1e-5)
    assert float((d_z - torch.from_numpy(g['dz']).reshape(z.shape).double()).abs().max()) < 2e-5 * float(d_z.abs().max())
    assert float((d_cb - torch.from_numpy(g['dE']).double()).abs().max()) < 2e-5 * float(d_cb.abs().max())


ALL_VQ_FWD = R.VQ_FWD_DSUB + R.VQ_FWD_K + R.VQ_FWD_BIG


@pytest.mark.parametrize('case', ALL_VQ_FWD, ids=[f'{c[0]}-d{c[4]}' for c in ALL_VQ_FWD])
def test_vq_fwd_cases_hold_what_they_plant(case):
    label, Rr, ncb, K, dsub = case
    assert K * dsub <= 36 * 1024
    z, cb, plan, given = R.vq_fwd_inputs(case)
    assert given.dtype == torch.int64 and given.shape == (Rr, ncb) and int(given.min()) >= 0 and int(given.max()) < K
    assert z.shape == (Rr, ncb * dsub) and cb.shape == (ncb, K, dsub) and bool(torch.isfinite(z).all() and torch.isfinite(cb).all())
    idx = O.vq_assign(z, list(cb))
    assert int(idx.min()) >= 0 and int(idx.max()) < K
    for c, p in enumerate(plan):
        canon = O.vq_distances_canonical(z[:, c * dsub:(c + 1) * dsub].contiguous(), cb[c])
        if p['dup'] is not None:
            a, b = p['dup']
            assert a < b and torch.equal(cb[c, a].view(torch.int32), cb[c, b].view(torch.int32))
            rows = torch.tensor(p['tie_rows'])
            assert len(rows) >= 1
            da, db = canon[rows, a], canon[rows, b]
            assert torch.equal(da.view(torch.int32), db.view(torch.int32)), 'a planted tie is not an exact fp32 tie'
            assert torch.equal(da, canon[rows].min(1)[0]), 'a planted tie is not the minimum of its row'
            assert bool((idx[rows, c] <= a).all()) and bool((idx[rows, c] != b).all())
        if p['near'] is not None:
            a, b = p['near']
            assert int((cb[c, a].view(torch.int32) != cb[c, b].view(torch.int32)).sum()) == 1
            assert abs(int(cb[c, a, 0].view(torch.int32)) - int(cb[c, b, 0].view(torch.int32))) == 1, 'not one ulp apart'
            rows = torch.tensor(p['near_rows'], dtype=torch.long)
            others = torch.ones(K, dtype=torch.bool)
            others[[a, b]] = False
            if len(rows) and bool(others.any()):                              # the two near codes are the row's two smallest distances
                assert bool((torch.maximum(canon[rows, a], canon[rows, b]) < canon[rows][:, others].min(1)[0]).all()), \
                    'a planted near-tie is not the pair of smallest distances of its row'
        for r in p['on_rows']:
            assert float(canon[r, p['on_k']]) == 0.0 and float(canon[r, idx[r, c]]) == 0.0
    if K >= 4:
        assert sum(len(p['near_rows']) for p in plan) >= (1 if Rr > 1 else 0)


ALL_VQ_BWD = [c for d in R.VQ_BWD_DSUBS for c in R.vq_bwd_cases(d)] + R.VQ_BWD_BIG


def test_vq_bwd_case_table_covers_what_it_says():
    assert {c[4] for c in ALL_VQ_BWD} == set(R.VQ_BWD_DSUBS)
    assert {c[3] for c in ALL_VQ_BWD} >= {1, 7, 128, 2048} and {c[1] for c in ALL_VQ_BWD} >= {1, 255, 256, 257, 513}
    assert {c[5] for c in ALL_VQ_BWD} == {'one', 'own', 'random'}
    for d in R.VQ_BWD_DSUBS:
        assert {c[5] for c in R.vq_bwd_cases(d)} >= {'one', 'own'}
        assert d == 158 or any(c[5] == 'own' and c[1] > 1 for c in R.vq_bwd_cases(d))      # own codes with more than one row
    kgroups = {256 // c[4] for c in ALL_VQ_BWD}
    assert kgroups >= {256, 85, 51, 21, 16, 4, 1}                                        # 85, 51, 21: the `%` path; 1: dsub > 128
    for _, _, _, K, dsub, _ in ALL_VQ_BWD:
        assert (K * dsub + 256 * dsub + 256) * 4 <= 160 * 1024
    assert any((K * dsub + 256 * dsub + 256) * 4 > 64 * 1024 for _, _, _, K, dsub, _ in ALL_VQ_BWD)
    for dsub, K in R.VQ_BWD_REFUSED:
        assert (K * dsub + 256 * dsub + 256) * 4 > 160 * 1024


@pytest.mark.parametrize('case', ALL_VQ_BWD, ids=[c[0] for c in ALL_VQ_BWD])
def test_vq_bwd_cases_hold_what_they_plant(case):
    label, Rr, ncb, K, dsub, pat = case
    z, cb, idx, g_zq, g_loss = R.vq_bwd_inputs(case)
    assert idx.dtype == torch.int64 and idx.shape == (Rr, ncb) and int(idx.min()) >= 0 and int(idx.max()) < K
    assert bool((g_loss[1::3] == 0).all()) and float(g_loss[0]) != 0.0 and (Rr < 2 or int((g_loss != 0).sum()) >= Rr // 2)
    _, d_cb, nrm, _ = R.vq_bwd(z, cb, idx, g_zq, g_loss, 0.25, True)
    for c in range(ncb):                          # every code chosen by a row that counts has summands, row 0's code among them
        counted = torch.unique(idx[g_loss != 0, c])
        assert len(counted) >= 1 and bool((nrm[c, counted] > 0).all()) and bool((nrm[c, idx[0, c]] > 0).all())
    for c in range(ncb):
        n = len(torch.unique(idx[:, c]))
        if pat == 'one':
            assert n == 1
        elif pat == 'own':
            assert n == Rr
        else:
            assert K - n >= K / 4.0, 'fewer than a quarter of the codes stay unchosen'


# =====================================================================================================================
# token tables
def test_embed_pos_reference_against_autograd():
    for label, tpb, nv, pos, dlin, has_ev, n_rows in R.EMB_CASES[:7]:
        tokens, table, chan, event, g, _ = R.emb_case(tpb, nv, pos, dlin, has_ev, n_rows, 11)
        t, c = table.double().requires_grad_(True), chan.double().requires_grad_(True)
        e = event.double().requires_grad_(True) if has_ev else None
        nb = n_rows // tpb
        emb = torch.stack([F.embedding(tokens.reshape(nb, tpb // nv, nv)[:, :, v], t[v]) for v in range(nv)], 2)   # (nb, ev, nv, dlin)
        parts = [emb, c.reshape(1, 1, nv, pos).expand(nb, tpb // nv, nv, pos)]
        if has_ev:
            parts.append(e.reshape(1, tpb // nv, 1, pos).expand(nb, tpb // nv, nv, pos))
        out = torch.cat(parts, -1).reshape(n_rows, -1)
        assert torch.equal(R.embed_pos_fwd(tokens, tpb, nv, table, chan, event).double(), out.detach()), label
        (out * g.double()).sum().backward()
        ref = R.embed_pos_bwd(tokens, tpb, nv, R.EMB_VMAX, dlin, pos, g, has_ev)
        assert close(ref['d_table'], t.grad) and close(ref['d_chan'], c.grad), label
        assert (ref['d_event'] is None) == (not has_ev) and (not has_ev or close(ref['d_event'], e.grad)), label
        sq = torch.zeros(nv, pos, dtype=F64)
        for v in range(nv):
            sq[v] = (g[torch.arange(n_rows) % tpb % nv == v][:, dlin:dlin + pos].double() ** 2).sum(0)
        assert close(ref['n_chan'] ** 2, sq), label


@pytest.mark.parametrize('case', R.EMB_CASES, ids=[c[0] for c in R.EMB_CASES])
def test_embed_pos_cases_hold_what_they_plant(case):
    label, tpb, nv, pos, dlin, has_ev, n_rows = case
    tokens, table, chan, event, g, dead = R.emb_case(tpb, nv, pos, dlin, has_ev, n_rows, R.EMB_CASES.index(case))
    assert tokens.dtype == torch.int64 and int(tokens.min()) >= 0 and int(tokens.max()) < R.EMB_VMAX
    assert n_rows % tpb == 0 and tpb % nv == 0 and 2048 % tpb == 0 and dlin % 4 == 0 and pos % 4 == 0 and pos in (4, 8)
    assert g.shape == (n_rows, dlin + (2 if has_ev else 1) * pos) and (event is None) == (not has_ev)
    v = torch.arange(n_rows) % tpb % nv
    ref = R.embed_pos_bwd(tokens, tpb, nv, R.EMB_VMAX, dlin, pos, g, has_ev)
    for u in range(nv):
        assert len(dead[u]) >= 1
        for t in dead[u]:
            assert not bool(((tokens == t) & (v == u)).any())
            assert bool((ref['n_table'][u, t] == 0).all()) and bool((ref['d_table'][u, t] == 0).all())


def test_embed_pos_case_table_covers_what_it_says():
    assert {(c[1], c[2]) for c in R.EMB_CASES} == {(16, 4), (4, 4), (8, 1), (64, 4), (2048, 4)}
    assert {c[3] for c in R.EMB_CASES} == {4, 8}
    ds = {((c[4] + (2 if c[5] else 1) * c[3]) % 64, c[5]) for c in R.EMB_CASES}
    assert ds >= {(m, e) for m in (0, 4, 12, 16, 40) for e in (True, False)}                # every width with and without the event part
    assert any(1 <= m <= 15 and not e for m, e in ds)                                    # d_event == NULL with a partial last wave
    rows = {(c[1], c[6]) for c in R.EMB_CASES}
    assert {(16, 65536 - 16), (16, 65536), (16, 65536 + 16)} <= rows and (65536 + 16) % 2048 != 0
    assert {c[6] // c[1] for c in R.EMB_CASES} >= {1, 2, 47, 48, 49}


def test_block_table_reference_against_autograd():
    for L, vmax, C, nb, dist in R.SEG_F32[:5] + R.SEG_B16[:3]:
        tokens, g, _, _ = R.seg_case(L, vmax, C, nb, dist, 3)
        table = torch.randn(vmax * L, C, generator=R.gen(4)).double().requires_grad_(True)
        out = F.embedding(tokens * L + torch.arange(nb * L) % L, table)
        assert torch.equal(R.block_gather(table.detach(), tokens, L), out.detach())
        (out * g.double()).sum().backward()
        ref, nrm = R.block_segsum(g, tokens, L, vmax)
        assert close(ref, table.grad)
        manual = torch.zeros(vmax * L, C, dtype=F64).index_add_(0, tokens * L + torch.arange(nb * L) % L, g.double() ** 2)
        assert close(nrm ** 2, manual)


SEG_ALL = [('f32',) + c for c in R.SEG_F32] + [('b16',) + c for c in R.SEG_B16]


@pytest.mark.parametrize('case', SEG_ALL, ids=['-'.join(str(x) for x in c) for c in SEG_ALL])
def test_block_table_cases_hold_what_they_plant(case):
    kind, L, vmax, C, nb, dist = case
    assert vmax * (1024 if kind == 'f32' else 2048) <= 160 * 1024 and (kind == 'f32' or C % 2 == 0)
    tokens, g, dead, dead_cells = R.seg_case(L, vmax, C, nb, dist, SEG_ALL.index(case))
    assert tokens.dtype == torch.int64 and tokens.shape == (nb * L,) and int(tokens.min()) >= 0 and int(tokens.max()) < vmax
    ref, nrm = R.block_segsum(g, tokens, L, vmax)
    pos = torch.arange(nb * L) % L
    if dist == 'one':
        assert len(torch.unique(tokens)) == 1 and len(dead) == vmax - 1
    if dist == 'unused':
        assert len(dead) == 3 and len(dead_cells) == 3
    for t in dead:
        assert not bool((tokens == t).any()) and bool((nrm[t * L:(t + 1) * L] == 0).all()) and bool((ref[t * L:(t + 1) * L] == 0).all())
    for t, p in dead_cells:
        assert t not in dead and not bool(((tokens == t) & (pos == p)).any()) and bool((nrm[t * L + p] == 0).all())


def test_block_table_case_table_covers_what_it_says():
    for cases, vm, cs in ((R.SEG_F32, {1, 2, 57, 100, 160}, {1, 5, 96, 256, 260, 768}), (R.SEG_B16, {1, 57, 80}, {2, 6, 510, 512, 514})):
        assert {c[0] for c in cases} == {1, 4, 16} and {c[1] for c in cases} == vm and {c[2] for c in cases} == cs
        assert {c[4] for c in cases} == {'one', 'uniform', 'unused'}
    assert {c[3] for c in R.SEG_F32 + R.SEG_B16} == {1, 31, 32, 33, 255, 511, 512, 513, 8193}
    assert {c[3] for c in R.SEG_F32} >= {1, 31, 32, 33, 511, 512, 513, 8193}
    gather = [c for c in R.SEG_F32 if c[2] % 4 == 0]
    assert {c[0] for c in gather} == {1, 4, 16} and {c[1] for c in gather} == {1, 2, 57, 100, 160}


def test_embedding_bwd_reference_against_autograd_and_replay():
    for M, C, gap, V, pat in R.EMBG_CASES:
        if V > 5 and C > 1:
            continue
        g, idx, _ = R.embg_case(M, C, gap, V, pat, 9)
        table = torch.zeros(V, C, dtype=F64, requires_grad=True)
        (F.embedding(idx, table) * g.double()).sum().backward()
        ref, nrm = R.embedding_bwd(g, idx, V)
        assert close(ref, table.grad)
        rep = R.embedding_bwd_replay(g, idx, V)
        # the replay against a plain loop over m in fp32
        loop = np.zeros((V, C), np.float32)
        for m in range(M):
            loop[int(idx[m])] = loop[int(idx[m])] + g[m].numpy()
        assert torch.equal(rep.view(torch.int32), torch.from_numpy(loop).view(torch.int32))
        assert bool((rep[nrm.sum(1) == 0] == 0).all())


@pytest.mark.parametrize('case', R.EMBG_CASES, ids=['-'.join(str(x) for x in c) for c in R.EMBG_CASES])
def test_embedding_bwd_cases_hold_what_they_plant(case):
    M, C, gap, V, pat = case
    g, idx, runs = R.embg_case(M, C, gap, V, pat, R.EMBG_CASES.index(case))
    assert idx.dtype == torch.int64 and idx.shape == (M,) and g.shape == (M, C)
    assert M == 0 or (int(idx.min()) >= 0 and int(idx.max()) < V)
    assert sum(runs.values()) == M
    if pat == 'same' and M:
        assert list(runs.values()) == [M]
    if pat == 'mixed' and M == 1000:
        assert {1, 8, 9} <= set(runs.values()) and (V == 5 or 17 in runs.values())
        assert len(runs) < V, 'no unreferenced row'
    if pat == 'mixed' and M == 9:
        assert sorted(runs.values()) == [1, 8]


def test_embedding_bwd_case_table_covers_what_it_says():
    assert {c[0] for c in R.EMBG_CASES} == {0, 1, 7, 8, 9, 1000} and {c[1] for c in R.EMBG_CASES} == {1, 255, 256, 257, 600}
    assert {c[2] for c in R.EMBG_CASES} == {0, 3} and {c[3] for c in R.EMBG_CASES} == {1, 5, 100000}
    assert all(c[3] * c[1] * 4 <= 128 << 20 for c in R.EMBG_CASES)


def test_seg_err_and_positive_zero():
    out = torch.tensor([1.0, 0.0, 3.0])
    assert torch.equal(R.seg_err(out, torch.tensor([1.5, 0.0, 3.0]), torch.tensor([2.0, 0.0, 1.0])), torch.tensor([0.25, 0.0], dtype=F64))
    assert R.is_pos_zero(torch.zeros(3)) and not R.is_pos_zero(torch.tensor([0.0, -0.0])) and not R.is_pos_zero(torch.tensor([1e-45]))
    v, b = R.bf16_trunc_values(torch.tensor([1.0 + 2.0 ** -10, -3.0]))
    assert v.tolist() == [1.0, -3.0] and b.tolist() == [0x3F80, 0xC040 - 65536]
