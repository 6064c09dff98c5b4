"""CPU anchors of tests/prior_masked_reference.py and of the host-only parts of the prior's allowed code sets
(vqcpc_bach_amd/priors/code_sets.py): the packers, the one check of a call, `code_sets` / `digit_sets`.  No GPU."""
import numpy as np
import pytest
import torch

import prior_constrained_reference as C
import prior_masked_reference as R
from vqcpc_bach_amd.priors import code_sets as S

VS = [1, 2, 15, 16, 17, 31, 32, 33, 65, 1000, 4095, 4096]


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _set(V, seed, share=0.4):
    a = torch.rand(V, generator=_gen(seed)) < share
    a[int(torch.randint(0, V, (1,), generator=_gen(seed + 1)))] = True
    return a


# ---- the reference itself ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('V', VS)
def test_logmass_is_the_allowed_share_of_the_softmax(V):
    row = torch.randn(V, generator=_gen(V)) * 3.0
    a = _set(V, 10 + V)
    want = float(torch.log(torch.softmax(row.double(), -1)[a].sum()))
    assert abs(R.logmass_ref(row, a) - want) < 1e-12
    assert R.logmass_ref(row, torch.ones(V, dtype=torch.bool)) == 0.0
    assert R.logmass_ref(row, torch.zeros(V, dtype=torch.bool)) == 0.0            # no bit inside the vocabulary: no restriction
    dead = row.clone()
    dead[a] = -float('inf')
    if not bool(a.all()):
        assert R.logmass_ref(dead, a) == -float('inf')


@pytest.mark.parametrize('V', VS)
def test_the_fp32_chain_in_the_kernels_order_stays_inside_the_derived_bound(V):
    worst = 0.0
    for k, scale in enumerate((2.0, 40.0)):
        row = (torch.randn(V, generator=_gen(100 + V + k)) * scale).float()
        if V >= 4 and k == 1:
            row[::3] = -float('inf')
        for share in (0.1, 0.5, 0.9):
            a = _set(V, 200 + V + k, share)
            got, ref, bound = float(R.logmass_chain32(row.numpy(), a)), R.logmass_ref(row, a), R.logmass_bound(row, a)
            if ref == -float('inf') or bound == 0.0:
                assert got == ref
                continue
            assert bound > 0.0 and abs(got - ref) <= bound, (V, scale, share, got, ref, bound)
            worst = max(worst, abs(got - ref) / bound)
    full = torch.ones(V, dtype=torch.bool)
    assert float(R.logmass_chain32(row.numpy(), full)) == 0.0 and R.logmass_bound(row, full) == 0.0
    print(f'V {V}: worst share of the bound {worst:.3f}')


def test_the_bound_grows_with_the_vocabulary_only_through_log_v_and_the_chain():
    """A flat row: s = V, s_a = V / 2, every d_i = 0, so the bound is 2 (g (1 + g) + ...) + 2 u ULP_LOG (log V + log V / 2) + the
    three roundings: between the smallest and the largest V it grows by the log terms alone."""
    u, g = 2.0 ** -24, C.SUM_CHAIN * 2.0 ** -24 / (1 - C.SUM_CHAIN * 2.0 ** -24)
    for V in (16, 4096):
        row, a = torch.zeros(V), torch.arange(V) % 2 == 0
        ds = 2 * u * R.ULP_EXP * (1 + g) + g + V * 2.0 ** -126
        dsa = 2 * u * R.ULP_EXP * (1 + g) + g + (V // 2) * 2.0 ** -126
        L, La = np.log(V), np.log(V // 2)
        want = ds * (1 + ds) + 2 * u * R.ULP_LOG * L + dsa * (1 + dsa) + 2 * u * R.ULP_LOG * La + u * La + u * abs(La - L)
        assert abs(R.logmass_bound(row, a) - want) <= 1e-12 * want


@pytest.mark.parametrize('V', [2, 17, 65])
def test_the_masked_step_is_the_constrained_step_on_a_row_closed_outside_the_set(V):
    M = 4
    lg = torch.randn(M, V, generator=_gen(V)) * 2.0
    seeds = torch.arange(M, dtype=torch.int64) * 7919 + 3
    allowed = torch.stack([_set(V, 300 + b) for b in range(M)])
    cons = torch.tensor([-1, 0, -1, V - 1])
    for top_k, top_p in ((0, 1.0), (3, 1.0), (0, 0.8), (3, 0.8)):
        codes, probs, logp, mass = R.masked_step_ref(lg, 1.3, top_k, top_p, seeds, 2, cons, allowed)
        closed = lg.double().masked_fill(~allowed, -float('inf'))
        c2, p2, _ = C.prior_constrained_step_ref(closed, 1.3, top_k, top_p, seeds, 2, cons)
        assert torch.equal(codes, c2) and torch.equal(probs, p2)
        free = cons < 0
        assert bool(allowed[free].gather(1, codes[free].unsqueeze(1)).all())                  # a drawn code lies in its set
        assert codes[1] == 0 and codes[3] == V - 1                                            # a forced code wins over the set
        c3, p3, l3 = C.prior_constrained_step_ref(lg, 1.3, top_k, top_p, seeds, 2, cons)
        full = R.masked_step_ref(lg, 1.3, top_k, top_p, seeds, 2, cons, torch.ones(M, V, dtype=torch.bool))
        assert torch.equal(full[0], c3) and torch.equal(full[1], p3) and torch.equal(full[2], l3) and bool((full[3] == 0).all())
        assert torch.equal(logp[free.logical_not()], l3[free.logical_not()])                   # logp: the unmodified row
        for b in range(M):
            assert abs(float(mass[b]) - R.logmass_ref(lg[b], allowed[b])) == 0.0
    one = torch.zeros(M, V, dtype=torch.bool)
    one[torch.arange(M), torch.tensor([0, 1, V - 1, V // 2])] = True
    codes = R.masked_step_ref(lg, 1.0, 0, 1.0, seeds, 0, None, one)[0]
    assert codes.tolist() == [0, 1, V - 1, V // 2]                                            # a one-hot set is forcing


def test_the_product_chain_of_one_codebook_is_the_masked_step_and_sums_the_stages():
    M, K = 3, 5
    lg = torch.randn(2, M, K, generator=_gen(5)) * 2.0
    seeds = torch.tensor([11, -5, 2 ** 40 + 1])
    sets = torch.rand(M, 2, K, generator=_gen(6)) < 0.6
    sets[:, :, 0] = True
    cons = torch.tensor([-1, 7, -1])
    one = R.product_chain_ref(lg[:1], 1.2, 0, 0.9, seeds, 3, cons.clamp(max=K - 1), sets[:, :1])
    ref = R.masked_step_ref(lg[0], 1.2, 0, 0.9, seeds, 3, cons.clamp(max=K - 1), sets[:, 0])
    assert torch.equal(one[0], ref[0]) and torch.equal(one[2], ref[2]) and torch.equal(one[3], ref[3])
    codes, dig, logp, mass = R.product_chain_ref(lg, 1.2, 0, 0.9, seeds, 3, cons, sets)
    assert torch.equal(codes, torch.as_tensor(dig[0] + K * dig[1])) and int(codes[1]) == 7
    for b in range(M):
        lp = sum(C.logp_ref(lg[j, b], dig[j][b]) for j in range(2))
        lm = sum(R.logmass_ref(lg[j, b], sets[b, j]) for j in range(2))
        assert abs(float(logp[b]) - lp) < 1e-12 and abs(float(mass[b]) - lm) < 1e-12
        if cons[b] < 0:
            assert bool(sets[b, 0, dig[0][b]]) and bool(sets[b, 1, dig[1][b]])
    assert R.stage_seed(11, 0) == 11 and R.stage_seed(11, 1) != R.stage_seed(11, 2) != 11


# ---- the packers ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('V', VS)
def test_pack_sets_is_packbits_in_little_bit_order(V):
    a = torch.rand(2, 3, V, generator=_gen(V)) < 0.5
    got = S.pack_sets(a)
    want = R.pack_ref(a.numpy())
    assert got.dtype == torch.int32 and tuple(got.shape) == (2, 3, (V + 31) // 32)
    assert np.array_equal(got.numpy().view(np.uint32), want)
    for i in (0, V // 2, V - 1):                                           # bit i & 31 of word i >> 5
        assert np.array_equal((want[..., i >> 5] >> np.uint32(i & 31)) & np.uint32(1), a[..., i].numpy().astype(np.uint32))
    d = torch.rand(2, 3, 2, V, generator=_gen(V + 1)) < 0.5                # product: one more axis before the words
    assert np.array_equal(S.pack_sets(d).numpy().view(np.uint32), R.pack_ref(d.numpy()))


# ---- the helpers and the one check of a call -------------------------------------------------------------------------------------
def test_code_sets_and_digit_sets_are_full_where_nothing_is_said_and_combine():
    a = S.code_sets(6, 11, {1: [2, 3], 5: [10]})
    assert a.dtype == torch.bool and tuple(a.shape) == (1, 6, 11)
    assert a[0, 1].nonzero().flatten().tolist() == [2, 3] and a[0, 5].nonzero().flatten().tolist() == [10]
    assert bool(a[0, [0, 2, 3, 4]].all())
    b = S.code_sets(6, 11, {1: [3, 4]})
    assert (a & b)[0, 1].nonzero().flatten().tolist() == [3] and torch.equal((a & b)[0, 5], a[0, 5])
    assert bool(S.code_sets(3, 4).all())
    d = S.digit_sets(4, 2, 5, {2: [[1, 4], None], 0: [None, [0]]})
    assert tuple(d.shape) == (1, 4, 2, 5) and d[0, 2, 0].nonzero().flatten().tolist() == [1, 4] and bool(d[0, 2, 1].all())
    assert d[0, 0, 1].nonzero().flatten().tolist() == [0] and bool(d[0, [1, 3]].all())
    for bad in (lambda: S.code_sets(6, 11, {6: [0]}), lambda: S.code_sets(6, 11, {0: [11]}), lambda: S.code_sets(6, 11, {0: [-1]}),
                lambda: S.digit_sets(4, 2, 5, {4: [None, None]}), lambda: S.digit_sets(4, 2, 5, {0: [None]}),
                lambda: S.digit_sets(4, 2, 5, {0: [[5], None]})):
        with pytest.raises(ValueError):
            bad()


def test_the_check_names_the_first_empty_set_and_the_first_forbidden_forced_code():
    a = S.code_sets(5, 7, {1: [2], 3: [0, 6]}).expand(2, 5, 7).clone()
    S.check_sets(a)
    S.check_sets(a, torch.tensor([[-1, 2, -1, 6, -1], [0, -1, 3, 0, 5]]))
    a[1, 4] = False
    with pytest.raises(ValueError, match=r'\(row 1, column 4\) has no allowed code'):
        S.check_sets(a)
    a[0, 2] = False
    with pytest.raises(ValueError, match=r'\(row 0, column 2\) has no allowed code'):
        S.check_sets(a)
    b = S.code_sets(5, 7, {1: [2], 3: [0, 6]})                                               # one row of sets for every row
    with pytest.raises(ValueError, match=r'\(row 1, column 3\) is forced to code 5'):
        S.check_sets(b, torch.tensor([[-1, 2, -1, 6, -1], [0, -1, 3, 5, 5]]))
    with pytest.raises(ValueError, match=r'\(row 0, column 1\) is forced to code 3'):
        S.check_sets(b, torch.tensor([[-1, 3, -1, 1, -1], [0, -1, 3, 5, 5]]))
    d = S.digit_sets(3, 2, 4, {1: [[1, 2], [0]]})
    S.check_sets(d, torch.tensor([[-1, 1, 15], [3, 2, -1]]))                                 # 1 = (1, 0), 2 = (2, 0)
    with pytest.raises(ValueError, match=r'\(row 1, column 1, codebook 1\) is forced to code 6'):
        S.check_sets(d, torch.tensor([[-1, 1, 15], [3, 6, -1]]))                             # 6 = (2, 1): digit 1 outside {0}
    with pytest.raises(ValueError, match=r'\(row 0, column 1, codebook 0\) is forced to code 0'):
        S.check_sets(d, torch.tensor([[-1, 0, 15], [3, 6, -1]]))
    d[0, 2, 1] = False
    with pytest.raises(ValueError, match=r'\(row 0, column 2, codebook 1\) has no allowed code'):
        S.check_sets(d)
