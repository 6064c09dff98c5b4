"""tests/prior_score_reference.py anchored on the CPU: its five outputs against torch float64 log_softmax / entropy / stable argsort,
the entropy bound's sanity, `PriorRelative.score_window_plan` against the two restatements of the columns `IncrementalPrior.run`
scores, and the C ABI of vqcpc_prior_score (declared, bound, every refusal before any HIP call)."""
import math

import numpy as np
import pytest
import torch

import prior_constrained_reference as C
import prior_score_reference as PS


def _rows():
    g = torch.Generator().manual_seed(911)
    for V in (1, 2, 15, 16, 17, 255, 256, 257, 1024, 1025, 4095, 4096):
        for spread in (0.0, 1e-3, 2.0, 80.0):
            row = (torch.randn(V, generator=g) * spread).float()
            if V >= 4:
                row[1] = row[V - 1] = row[V // 2]                     # ties below and above the middle code
            yield V, spread, row
    holes = torch.randn(37, generator=g).float()
    holes[::3] = -float('inf')
    yield 37, 'holes', holes


def test_reference_against_torch_float64():
    g = torch.Generator().manual_seed(912)
    for V, spread, row in _rows():
        r64 = row.double()
        lsm = torch.log_softmax(r64, dim=-1)
        p = torch.softmax(r64, dim=-1)
        ent = float(-(p[p > 0] * lsm[p > 0]).sum())
        order = torch.argsort(r64, descending=True, stable=True)     # equal logits keep their index order
        for tok in sorted({0, V // 2, V - 1, int(torch.randint(0, V, (1,), generator=g))}):
            ref = PS.prior_score_ref(row.numpy(), tok)
            label = (V, spread, tok)
            if float(lsm[tok]) == -float('inf'):
                assert ref['logp'] == -float('inf'), label
            else:
                assert abs(ref['logp'] - float(lsm[tok])) <= 1e-12 * max(1.0, abs(float(lsm[tok]))), label
            assert abs(ref['entropy'] - ent) <= 1e-12 * max(1.0, ent), label
            assert -1e-12 <= ref['entropy'] <= math.log(V) + 1e-12, label
            assert ref['rank'] == int((order == tok).nonzero()[0, 0]), label
            assert ref['best'] == int(order[0]) and ref['best_logp'] == pytest.approx(float(lsm.max()), abs=1e-12), label
            assert (ref['rank'] == 0) == (ref['best'] == tok), label
            assert ref['best_logp'] >= ref['logp'], label
            assert PS.rank_best_fp32(row.numpy(), tok) == (ref['rank'], ref['best']), label


def test_rank_best_tie_rules_and_the_digit_rule():
    row = np.array([1.0, 3.0, 3.0, 0.5, 3.0, 1.0], np.float32)
    assert [PS.prior_score_ref(row, t)['rank'] for t in range(6)] == [3, 0, 1, 5, 2, 4]
    assert PS.prior_score_ref(row, 4)['best'] == 1 and PS.rank_best_fp32(row, 2) == (1, 1)
    flat = np.zeros(7, np.float32)
    assert [PS.prior_score_ref(flat, t)['rank'] for t in range(7)] == list(range(7)) and PS.prior_score_ref(flat, 3)['best'] == 0
    assert [PS.target_digit(5 + 8 * 3 + 64 * 7, 8, 3, j) for j in range(3)] == [5, 3, 7]
    assert PS.target_digit(-4, 8, 3, 1) == 0 and PS.target_digit(10 ** 9, 8, 3, 2) == 7 and PS.target_digit(40, 32) == 31


def test_entropy_bound_is_small_and_covers_a_plain_fp32_evaluation():
    """The bound is of the order of u (H + 1), and an fp32 numpy evaluation of the kernel's formula (numpy's pairwise sums are
    another tree than the kernel's, so it is only checked against 30 x the bound) stays inside."""
    for V, spread, row in _rows():
        r = row.numpy()
        b = PS.entropy_bound(r)
        ref = PS.prior_score_ref(r, 0)['entropy']
        assert 0.0 < b < 4e-5 * (1.0 + ref), (V, spread, b)
        m = r.max()
        live = np.isfinite(r)
        d = (m - r[live]).astype(np.float32)
        e = np.exp(-d).astype(np.float32)
        s = np.float32(e.sum(dtype=np.float32))
        got = float(np.float32(np.log(s)) + np.float32((e * d).sum(dtype=np.float32)) / s)
        assert abs(got - ref) <= 30 * b, (V, spread, got, ref, b)
    assert PS.prior_score_ref(np.zeros(1, np.float32), 0)['entropy'] == 0.0
    uniform = PS.prior_score_ref(np.full(4096, 0.25, np.float32), 7)
    assert uniform['entropy'] == pytest.approx(math.log(4096), abs=1e-12) and uniform['rank'] == 7 and uniform['best'] == 0
    assert C.logp_bound(torch.zeros(4), 0) > 0


def test_score_window_plan():
    from vqcpc_bach_amd.priors.prior_relative import PriorRelative
    for N in (1, 2, 6):
        for L in range(N, 3 * N + 2):
            for k in range(1, max(N, 2)):
                plan = PriorRelative.score_window_plan(L, N, k)
                label = (N, L, k)
                assert plan == PS.window_plan_ref(L, N, k), label
                assert plan == [(w, cols[0], cols[-1] + 1) for w, cols in PS.run_columns_ref(L, N, k)], label
                assert [p[0] for p in plan] == sorted({p[0] for p in plan}), 'windows ascend and are distinct'
                seen = []
                for w, lo, hi in plan:
                    assert 0 <= w <= L - N and w <= lo < hi <= w + N, label       # scored columns inside their window
                    seen += list(range(lo, hi))
                assert seen == list(range(L)), label                             # every column exactly once, ascending
                assert plan[0] == (0, 0, N), label
                for w, lo, hi in plan[1:]:
                    assert hi == w + N and hi - lo in (k, (L - N) % k), label     # a later window scores its last columns
        assert PriorRelative.score_window_plan(N, N, 1) == [(0, 0, N)]           # L == N: one window
    assert PriorRelative.score_window_plan(96, 24, 1) == [(0, 0, 24)] + [(i, i + 23, i + 24) for i in range(1, 73)]
    assert PriorRelative.score_window_plan(15, 6, 4) == [(0, 0, 6), (4, 6, 10), (8, 10, 14), (9, 14, 15)]
    for bad in ((5, 6, 1), (6, 6, 0), (6, 6, 6), (12, 6, 7), (3, 1, 2), (0, 0, 1), (9, 6, 1.5), (9, 6, True)):
        with pytest.raises(ValueError):
            PriorRelative.score_window_plan(*bad)


def test_score_chorale_refuses_what_needs_no_device_to_refuse():
    import types
    from vqcpc_bach_amd.priors import scoring
    x = torch.zeros(1, 8, 4, dtype=torch.int64)
    with pytest.raises(NotImplementedError, match='continuous'):
        scoring.score_chorale(None, x, types.SimpleNamespace(continuous_source=True))
    with pytest.raises(ValueError, match='START'):
        scoring.score_chorale(None, x, types.SimpleNamespace(continuous_source=False, dataloader_generator=None))


def test_prior_score_is_declared_bound_and_refuses_bad_arguments_before_any_hip_call():
    import ctypes
    import torch  # noqa: F401,F811  (the process-wide HIP runtime first)
    from test_abi import header_symbols
    from vqcpc_bach_amd import hip
    assert 'vqcpc_prior_score' in header_symbols() and 'vqcpc_prior_score' in hip.SIGNATURES
    lib = hip.load()
    fn = lib.vqcpc_prior_score
    p = ctypes.c_void_p(64)                                           # never dereferenced: every call below is refused on the host
    good = dict(logits=p, ldl=40, V=32, ncb=1, stage=0, R=4, row_b=p, row_col=p, seq=p, ldseq=9, B=2, cols=9, logp=p, ldlogp=9,
                ld=9, entropy=p, rank=p, best=p, best_logp=p)
    bad = [dict(logits=None), dict(row_b=None), dict(row_col=None), dict(seq=None), dict(V=0), dict(V=4097), dict(ncb=0),
           dict(ncb=5), dict(stage=-1), dict(stage=1), dict(ncb=2, stage=2, ld=18), dict(V=4096, ldl=4096, ncb=3, ld=27), dict(R=0),
           dict(B=0), dict(cols=0), dict(ldl=31), dict(ldseq=8), dict(ldlogp=8), dict(ld=8), dict(ncb=2, ld=17)]
    for kw in bad:
        args = dict(good)
        args.update(kw)
        assert fn(*args.values(), None) == -1, kw
        assert b'prior_score' in lib.vqcpc_last_error(), kw
