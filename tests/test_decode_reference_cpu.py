"""Anchors tests/decode_reference.py (the float64 references of the generation kernels) before any GPU is involved:
the reference's own attention fixtures, its top-k / top-p keep-masks, the host's seed rule.  CPU only."""
import numpy as np
import pytest
import torch

import decode_reference as R
from conftest import load_golden, rel_err

T = torch.from_numpy
TOL = 1e-6            # the fixtures are fp32: the bound tests/test_decoder_oracle_golden.py uses for the relative term


@pytest.mark.parametrize('name,mask', [('mha_self_causal_T24', 1), ('mha_self_full_T16', 0),
                                        ('mha_cross_anticausal_S6_T12', 2)])
def test_attn_ref_reproduces_the_reference_attention(name, mask):
    """in_proj and out_proj restated in float64 around attn_ref: the module's output and its per-head weights."""
    g = load_golden(name)
    H, S, Tq = int(g['H']), int(g['S']), int(g['T'])
    xq = T(g['q']).double().transpose(0, 1)                                  # fixtures are time-first
    xkv = T(g['mem']).double().transpose(0, 1) if 'mem' in g else xq
    n, _, d = xq.shape
    hd = d // H
    W, b = T(g['sd/in_proj_weight']).double(), T(g['sd/in_proj_bias']).double()
    q = xq @ W[:d].t() + b[:d]
    k, v = (xkv @ W[d:].t() + b[d:]).split(d, dim=-1)
    if 'attn_mask' in g:                                                     # the additive mask the fixture was made with
        keep = np.isfinite(g['attn_mask'])
        p = (np.arange(Tq) // (Tq // S))[:, None]
        j = np.arange(S)[None, :]
        assert np.array_equal(keep, (j <= p) if mask == 1 else (j >= p))
    else:
        assert mask == 0
    ctx, w = R.attn_ref(q.reshape(n, Tq, H, hd), k.reshape(n, S, H, hd), v.reshape(n, S, H, hd), g['sd/attn_bias.e1'],
                        g['sd/attn_bias.e2'], S, Tq // S, mask, range(Tq), return_weights=True)
    assert w.dtype == torch.float64 and ctx.shape == (n, Tq, H, hd)
    out = ctx.reshape(n, Tq, d) @ T(g['sd/out_proj.weight']).double().t() + T(g['sd/out_proj.bias']).double()
    assert rel_err(w, g['weights']) < TOL
    assert rel_err(out.transpose(0, 1), g['out']) < TOL
    # a subset of rows is the same rows of the whole
    rows = [Tq - 1, 0, Tq // 2]
    sub = R.attn_ref(q.reshape(n, Tq, H, hd)[:, rows], k.reshape(n, S, H, hd), v.reshape(n, S, H, hd), g['sd/attn_bias.e1'],
                     g['sd/attn_bias.e2'], S, Tq // S, mask, rows)
    assert float((sub - ctx[:, rows]).abs().max()) < 1e-14
    # and the fp32 evaluation of the same formula is an fp32-accurate copy of it
    c32 = R.attn_ref(q.reshape(n, Tq, H, hd), k.reshape(n, S, H, hd), v.reshape(n, S, H, hd), g['sd/attn_bias.e1'],
                     g['sd/attn_bias.e2'], S, Tq // S, mask, range(Tq), dtype=torch.float32)
    assert c32.dtype == torch.float32 and 0.0 < rel_err(c32, ctx) < 1e-5


def test_attn_logits_ref_are_the_logits_of_attn_ref():
    g = torch.Generator().manual_seed(0)
    n, H, hd, Lk, ratio = 2, 3, 16, 5, 4
    q, k, v = torch.randn(n, 2, H, hd, generator=g), torch.randn(n, Lk, H, hd, generator=g), torch.randn(n, Lk, H, hd, generator=g)
    e1, e2 = torch.randn(H * Lk, hd, generator=g), torch.randn(H * Lk, hd, generator=g)
    rows = [7, 19]
    s = R.attn_logits_ref(q, k, e1, e2, Lk, ratio, rows)
    _, w = R.attn_ref(q, k, v, e1, e2, Lk, ratio, 0, rows, return_weights=True)
    assert float((torch.softmax(s, dim=-1) - w).abs().max()) < 1e-15
    # written out for one entry: query row 19 -> p = 4, key 1 -> e1 row Lk - 1 - (p - j) = 1 of head 2
    want = (q[1, 1, 2].double() @ (k[1, 1, 2].double() + e1.view(H, Lk, hd)[2, 1].double())) / 4.0
    assert abs(float(s[1, 2, 1, 1]) - float(want)) < 1e-13
    # query row 7 -> p = 1, key 3 -> e2 row j - p = 2
    want = (q[0, 0, 0].double() @ (k[0, 3, 0].double() + e2.view(H, Lk, hd)[0, 2].double())) / 4.0
    assert abs(float(s[0, 0, 0, 3]) - float(want)) < 1e-13


def test_filter_ref_reproduces_the_reference_keep_masks():
    """Every keep-mask of generate_filter.npz (the reference's top_k_top_p_filtering in fp32), under the documented
    deviation: top_p >= 1 keeps all, where the reference can drop tail tokens whose fp32 cumulative sum rounds above 1.0."""
    g = load_golden('generate_filter')
    logits, widths, keep = g['logits'], g['widths'], g['keep']
    checked = 0
    for r in range(logits.shape[0]):
        V = int(widths[r])
        for a, k in enumerate(g['top_k']):
            for b, p in enumerate(g['top_p']):
                for c, temp in enumerate(g['temperature']):
                    pr = R.filter_ref(logits[r, :V], float(temp), int(k), float(p))
                    ref_keep = T(keep[r, a, b, c, :V].copy())
                    assert not bool(keep[r, a, b, c, V:].any())
                    if p >= 1.0:
                        extra = (pr > 0) & ~ref_keep
                        f = T(logits[r, :V].copy()).double() / float(temp)
                        assert float(torch.softmax(f, dim=-1)[extra].sum()) < 1e-7
                        ref_keep = ref_keep | extra
                    assert torch.equal(pr > 0, ref_keep), (r, V, int(k), float(p), float(temp))
                    assert abs(float(pr.sum()) - 1.0) < 1e-12
                    checked += 1
    assert checked == logits.shape[0] * 4 * 4 * 3


def test_filter_ref_edges():
    row = [0.0, -0.0, -1.0, 2.0, 2.0]
    # a logit equal to the k-th largest is kept (utils.py:113 drops `<` only); -0.0 == +0.0
    assert (R.filter_ref(row, 1.0, 1, 1.0) > 0).tolist() == [False, False, False, True, True]
    assert (R.filter_ref(row, 1.0, 3, 1.0) > 0).tolist() == [True, True, False, True, True]
    assert (R.filter_ref([0.0, -0.0, -1.0], 1.0, 1, 1.0) > 0).tolist() == [True, True, False]
    assert (R.filter_ref(row, 1.0, 99, 1.0) > 0).all()                       # top_k = min(top_k, V) (utils.py:110)
    assert (R.filter_ref(row, 1.0, 0, 1.0, exclude=(3,)) > 0).tolist() == [True, True, True, False, True]
    # the prior multiplies by its temperature
    a, b = R.filter_ref(row, 0.5, 0, 1.0, multiply=True), R.filter_ref(row, 2.0, 0, 1.0)
    assert float((a - b).abs().max()) < 1e-15
    # top-p: the first token above the threshold is kept too
    pr = R.filter_ref(np.log([0.5, 0.3, 0.15, 0.05]), 1.0, 0, 0.7)
    assert (pr > 0).tolist() == [True, True, False, False]


def test_window_seed_is_the_host_seed_rule():
    from vqcpc_bach_amd.decoders.generation import _splitmix64
    for z in (0, 1, 0x9E3779B97F4A7C15, (1 << 64) - 1, 1234567890123456789):
        assert R.splitmix64(z) == _splitmix64(z)
    assert R.splitmix64(0) == 0xE220A8397B1DCDAF                             # the published first output of seed 0
    for sd in (0, 5, -1, -(1 << 63), (1 << 63) - 1):
        assert R.window_seed(sd, 0) == sd
        for w in (1, 2, 1000):
            want = _splitmix64((sd & ((1 << 64) - 1)) ^ ((w * 0xD1B54A32D192ED03) & ((1 << 64) - 1)))
            assert R.window_seed(sd, w) & ((1 << 64) - 1) == want
            assert -(1 << 63) <= R.window_seed(sd, w) < (1 << 63)


def test_rng_u24_ref_against_python_ints():
    """The numpy uint32 restatement against the same recurrence on unbounded Python ints."""
    def slow(sd, pos):
        sd &= (1 << 64) - 1
        m = 0xFFFFFFFF
        x = ((pos & m) * 0x9E3779B1 + (sd & m)) & m
        x ^= sd >> 32
        x ^= x >> 16
        y = ((x & 0xFFFFFF) * 0x6B43A9) & m
        y ^= y >> 15
        y = (((y & 0xFFFFFF) * 0x52DCE7) + x) & m
        y ^= y >> 14
        return y >> 8
    seeds = np.array([0, 1, -1, 7919 * 1003, -(1 << 63), (1 << 63) - 1, 0x123456789ABCDEF], dtype=np.int64)
    pos = np.arange(0, 5000, 37, dtype=np.int64)
    got = R.rng_u24_ref(seeds[:, None], pos[None, :])
    assert got.shape == (len(seeds), len(pos)) and got.min() >= 0 and got.max() < 1 << 24
    for a, sd in enumerate(seeds):
        for b, p in enumerate(pos):
            assert int(got[a, b]) == slow(int(sd), int(p))


def test_window_refs_on_a_hand_made_case():
    U, S, nb, M, d = 2, 2, 4, 1, 3
    T_ = S * U
    table = np.arange(7 * d, dtype=np.float32).reshape(7, d)                  # sos = row 6
    chorale = np.array([[9, 9, 1, 0, 2, 1, 9, 9]], dtype=np.int64)
    tokens = np.array([[1, 2, 0, 1]], dtype=np.int64)
    st = R.decode_window_ref(np.array([[5, 6, 7, 8]]), chorale, [1, 0], 1, np.zeros((M, S), np.int64), tokens, U, 3,
                             np.zeros((M, 3), np.int64), table, np.zeros((M, d + 1), np.float32), [3], [0], pos=3)
    assert st['chorale'].tolist() == [[1, 2, 0, 0, 2, 1, 9, 9]]              # three tokens committed at window 0
    assert st['codes_win'].tolist() == [[6, 7]] and st['tokens'].tolist() == [[0, 0, 2, 1]]      # the load sees the commit
    assert st['prefix_rows'].tolist() == [[6, 0 * U + 0, 0 * U + 1]]
    assert st['x'][0, :d].tolist() == table[min(2 * U + 0, 5)].tolist() and st['x'][0, d] == 0.0
    assert st['pos'] == 3 and st['win'].tolist() == [2, 1] and st['seeds_out'][0] == R.window_seed(3, 1)
    # next + S > nb: commit only
    st = R.decode_window_ref(np.array([[5, 6, 7, 8]]), chorale, [3, 2], 1, np.zeros((M, S), np.int64), tokens, U, 0, None,
                             table, np.zeros((M, d), np.float32), [3], [0], pos=T_ + 5)
    assert st['chorale'].tolist() == [[9, 9, 1, 0, 1, 2, 0, 1]] and st['pos'] == T_ + 5 and st['win'].tolist() == [3, 2]
    # the prior's: codes are table rows
    st = R.prior_window_ref(np.array([[4, 4, 9, 1, 0]]), 5, [1, 0], 4, np.array([[2, 3, 5]]), 2, np.zeros((M, 2), np.int64),
                            table, np.zeros((M, d), np.float32), [8], [0], pos=2)
    assert st['seq'].tolist() == [[2, 3, 9, 1, 0]] and st['codes_win'].tolist() == [[3, 9, 1]]
    assert st['prefix_rows'].tolist() == [[6, 3]] and st['x'][0].tolist() == table[5].tolist()   # code 9 clamps to sos - 1
    assert st['pos'] == 2 and st['win'].tolist() == [5, 1]
