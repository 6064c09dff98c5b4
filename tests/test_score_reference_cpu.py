"""tests/score_reference.py anchored on the CPU: its six outputs against torch float64 log_softmax / entropy / argsort, the bounds'
sanity, `Decoder.score_window_plan` against `compute_start_end_times`, `attention_window_starts` and the restated plan, and the
ValueErrors of `score_tokens` that need no device."""
import math

import numpy as np
import pytest
import torch

import constrained_reference as C
import masked_reference as MR
import score_reference as SR


def _rows():
    g = torch.Generator().manual_seed(901)
    for V in (1, 2, 3, 4, 5, 63, 64, 65, 255, 256):
        for spread in (0.0, 1e-3, 2.0, 80.0):
            row = (torch.randn(V, generator=g) * spread).float()
            if V >= 4:
                row[1] = row[V - 1] = row[V // 2]                     # ties below and above the middle token
            yield V, spread, row
    holes = torch.randn(37, generator=g).float()
    holes[::3] = -float('inf')
    yield 37, 'holes', holes


def test_reference_against_torch_float64():
    g = torch.Generator().manual_seed(902)
    for V, spread, row in _rows():
        r64 = row.double()
        lsm = torch.log_softmax(r64, dim=-1)
        p = torch.softmax(r64, dim=-1)
        ent = float(-(p[p > 0] * lsm[p > 0]).sum())
        order = torch.argsort(r64, descending=True, stable=True)     # equal logits keep their index order
        for tok in sorted({0, V // 2, V - 1, int(torch.randint(0, V, (1,), generator=g))}):
            allowed = torch.rand(256, generator=g) < 0.5
            allowed[tok] = True
            ref = SR.score_ref(row.numpy(), tok, allowed.numpy())
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
            assert SR.rank_best_fp32(row.numpy(), tok) == (ref['rank'], ref['best']), label
            want = MR.logmass_ref(row, allowed)
            assert ref['logmass'] == pytest.approx(want, abs=1e-12) or ref['logmass'] == want, label
            assert SR.score_ref(row.numpy(), tok, None)['logmass'] == 0.0, label
            assert SR.score_ref(row.numpy(), tok, np.zeros(256, bool))['logmass'] == 0.0, label      # an empty set: no restriction


def test_rank_and_best_tie_rules():
    row = np.array([1.0, 3.0, 3.0, 0.5, 3.0, 1.0], np.float32)
    assert [SR.score_ref(row, t)['rank'] for t in range(6)] == [3, 0, 1, 5, 2, 4]
    assert SR.score_ref(row, 4)['best'] == 1
    assert SR.rank_best_fp32(row, 2) == (1, 1)
    flat = np.zeros(7, np.float32)
    assert [SR.score_ref(flat, t)['rank'] for t in range(7)] == list(range(7)) and SR.score_ref(flat, 3)['best'] == 0


def test_entropy_bound_is_small_and_covers_a_plain_fp32_evaluation():
    """The bound is of the order of u (H + 1) -- far below any modelling difference -- and an fp32 numpy evaluation of the kernel's
    formula (sequential sums: at most V - 1 additions per term instead of nine, so it is only checked against 30 x the bound)
    stays inside."""
    for V, spread, row in _rows():
        r = row.numpy()
        b = SR.entropy_bound(r)
        ref = SR.score_ref(r, 0)['entropy']
        assert 0.0 < b < 2e-5 * (1.0 + ref), (V, spread, b)
        m = r.max()
        live = np.isfinite(r)
        d = (m - r[live]).astype(np.float32)
        e = np.exp(-d).astype(np.float32)
        s = np.float32(e.sum(dtype=np.float32))
        got = float(np.float32(np.log(s)) + np.float32((e * d).sum(dtype=np.float32)) / s)
        assert abs(got - ref) <= 30 * b, (V, spread, got, ref, b)
    assert SR.score_ref(np.zeros(1, np.float32), 0)['entropy'] == 0.0
    uniform = SR.score_ref(np.full(256, 0.25, np.float32), 7)
    assert uniform['entropy'] == pytest.approx(math.log(256), abs=1e-12) and uniform['rank'] == 7 and uniform['best'] == 0
    assert C.logp_bound(torch.zeros(4), 0) > 0


def _check_plan(dec_cls, nb, S, c0, c1):
    plan = dec_cls.score_window_plan(nb, S, c0, c1)
    assert plan == SR.window_plan_ref(nb, S, c0, c1), (nb, S, c0, c1)
    assert [p[0] for p in plan] == sorted({p[0] for p in plan}), 'windows ascend and are distinct'
    seen = {}
    for w, lo, hi in plan:
        assert 0 <= w <= nb - S and lo < hi, 'no window without a code'
        for t in range(lo, hi):
            assert t not in seen
            seen[t] = w
    assert sorted(seen) == list(range(c0, c1)), 'every code of the range in exactly one window'
    U = 2
    starts = dec_cls.attention_window_starts(nb, S, U, c0, c1)
    for t in range(nb):
        tb, te, tr = dec_cls.compute_start_end_times(t, nb, S)
        assert (tb, te, tr) == SR.start_end_times_ref(t, nb, S), (t, nb, S)
        if c0 <= t < c1:
            assert seen[t] == tb and tb <= t < te and tr == t - tb
            assert starts[t * U:(t + 1) * U].tolist() == [tb] * U
        else:
            assert starts[t * U:(t + 1) * U].tolist() == [-1] * U


def test_score_window_plan():
    from vqcpc_bach_amd.decoders.decoder import Decoder
    for S in (2, 3, 4, 24):
        for nb in list(range(S, S + 10)) + [96]:
            small = nb <= S + 9 and S <= 4
            ranges = [(a, b) for a in range(nb + 1) for b in range(a, nb + 1)] if small else \
                [(0, nb), (1, nb), (0, nb - 1), (S // 2, nb - S // 2), (nb // 2, nb // 2 + 1), (3, 3)]
            for c0, c1 in ranges:
                _check_plan(Decoder, nb, S, c0, c1)
        assert Decoder.score_window_plan(S, S, 0, S) == [(0, 0, S)]                  # nb == S: one window
        assert len(Decoder.score_window_plan(96, S, 0, 96)) == 96 - S + 1            # the nb - S + 1 distinct windows of a piece
    assert Decoder.score_window_plan(7, 3, 1, 7) == [(0, 1, 2), (1, 2, 3), (2, 3, 4), (3, 4, 5), (4, 5, 7)]
    assert Decoder.score_window_plan(7, 3, 4, 4) == []
    for bad in ((2, 3, 0, 2), (7, 3, -1, 4), (7, 3, 5, 4), (7, 3, 0, 8), (7, 0, 0, 7)):
        with pytest.raises(ValueError):
            Decoder.score_window_plan(*bad)


class _Stub:
    """What `score_tokens` touches before its first launch, without a device: S = 3, U = 8, two voices."""
    num_tokens_source, total_upscaling, num_events_per_code, num_channels, num_tokens_target = 3, 8, 4, 2, 24
    num_tokens_per_channel = [5, 7]
    d_model, continuous_source, source_dim = 8, False, None
    sos = torch.zeros(1)

    from vqcpc_bach_amd.decoders.decoder import Decoder as _D
    compute_start_end_times = staticmethod(_D.compute_start_end_times)
    _check_source, _source_on_device = _D._check_source, _D._source_on_device


def test_score_tokens_refuses_bad_arguments_without_a_device():
    from vqcpc_bach_amd.decoders import scoring
    dec = _Stub()
    nb = 5
    codes = torch.zeros(2, nb, dtype=torch.int64)
    x = torch.zeros(2, nb * 4, 2, dtype=torch.int64)
    for kw, match in ((dict(window_rows=0), 'window_rows'), (dict(window_rows=1.5), 'window_rows'),
                      (dict(codes=codes[:, :2]), 'at least 3 codes'), (dict(codes=codes.float()), 'merged codes'),
                      (dict(codes=codes[0]), 'merged codes'), (dict(code_index_start=4, code_index_end=3), 'code_index_start'),
                      (dict(code_index_end=6), 'code_index_start'), (dict(code_index_start=-1), 'code_index_start'),
                      (dict(x=x[:, :-1]), r'x: \(2, 20, 2\) int64'), (dict(x=x.int()), r'x: \(2, 20, 2\) int64'),
                      (dict(x=x[:1]), r'x: \(2, 20, 2\) int64')):
        args = dict(x=x, codes=codes)
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            scoring.score_tokens(dec, **args)
    bad = x.clone()
    bad[1, 9, 1] = 7                                                 # voice 1 holds 7 tokens: 7 is outside
    bad[1, 13, 0] = -1
    with pytest.raises(ValueError, match=r'row 1, event 9, voice 1\) holds token 7'):
        scoring.score_tokens(dec, bad, codes)
    with pytest.raises(ValueError, match=r'row 1, event 13, voice 0\) holds token -1'):
        scoring.score_tokens(dec, bad, codes, code_index_start=3)    # event 9 lies before the scored range: ignored
