"""tests/prior_beam_reference.py anchored without a GPU: on toy table-driven models whose beam is at least as wide as the number of
plans the search is exhaustive and must return exactly the brute-force ranking; the tie order, dead slots, forced columns and sets
of `select` / `candidate_codes` on columns past the decoder's 256; the rows' lists the expansion hands over; every refusal of the
public keywords that needs no GPU; and, with the kernel library replaced by the recorder of tests/test_generation_launches_cpu.py,
the launches a beam makes on the prior's host path."""
import itertools

import numpy as np
import pytest
import torch

import prior_beam_reference as R

F = np.float32
NINF = -np.inf


def table_model(seed, V, scale=2.0):
    """A model whose next logits are a fixed function of (column, the two previous codes)."""
    rng = np.random.default_rng(seed)
    tables = {}

    def model(prefix):
        key = (len(prefix),) + tuple(prefix[-2:])
        if key not in tables:
            tables[key] = rng.normal(size=V) * scale
        return tables[key]
    return model


def brute_force(model, T, constraint=None, allowed=None):
    """Every plan the candidate rule admits with its float64 total, ranked: total descending, then the plan ascending."""
    seqs = [(0.0, ())]
    for t in range(T):
        nxt = []
        for total, pre in seqs:
            logits = np.asarray(model(pre), dtype=np.float64)
            lp = R.lp64(logits)
            codes = R.candidate_codes(len(logits), -1 if constraint is None else int(constraint[t]),
                                      None if allowed is None else allowed[t])
            nxt += [(total + lp[v], pre + (v,)) for v in codes if lp[v] > -np.inf]
        seqs = nxt
    return sorted(seqs, key=lambda x: (-x[0], x[1]))


@pytest.mark.parametrize('seed,V,T,W', [(0, 3, 3, 64), (1, 2, 5, 32), (2, 7, 2, 49), (3, 5, 2, 25)])
def test_exhaustive_beam_equals_brute_force(seed, V, T, W):
    model = table_model(seed, V)
    ranking = brute_force(model, T)
    tot = np.array([t for t, _ in ranking])
    assert len(ranking) <= W and float(np.min(tot[:-1] - tot[1:])) > 1e-4     # fp32 rounding of the totals cannot reorder these
    codes, scores, hist = R.beam_search(model, T, W)
    n = len(ranking)
    assert [tuple(r) for r in codes[:n]] == [s for _, s in ranking]
    np.testing.assert_allclose(scores[:n], tot, rtol=0, atol=T * 4 * 2.0 ** -24 * 10)
    assert np.all(scores[n:] == NINF) and np.all(codes[n:] == codes[0])              # dead slots copy slot 0
    assert np.all(np.diff(scores[:n]) <= 0) and hist.min() >= 0 and hist.max() < W


def test_constraint_and_sets_follow_the_candidate_rule():
    model = table_model(4, 300)                                    # codes past the decoder's 256
    T, W = 3, 16
    constraint = [-1, 9999, -1]                                    # clamped to V - 1 = 299
    allowed = [[0, 257, 299, 300, 5000], [1], [7, 280]]            # 300 and 5000 are ignored; the forced column ignores [1]
    ranking = brute_force(model, T, constraint, allowed)
    assert {s[0] for _, s in ranking} == {0, 257, 299} and {s[1] for _, s in ranking} == {299}
    assert {s[2] for _, s in ranking} == {7, 280} and len(ranking) == 6
    codes, scores, _ = R.beam_search(model, T, W, constraint, allowed)
    assert [tuple(r) for r in codes[:6]] == [s for _, s in ranking] and np.all(scores[6:] == NINF)
    assert R.candidate_codes(5, forced=7) == [4] and R.candidate_codes(5, forced=9000) == [4] and R.candidate_codes(5, forced=0) == [0]
    assert R.candidate_codes(4, allowed=[1, 3, 9]) == [1, 3] and R.candidate_codes(4, allowed=[9]) == [0, 1, 2, 3]
    assert R.candidate_codes(4096, allowed=[4095, 4096]) == [4095]


def test_narrow_beam_keeps_the_greedy_prefixes_and_is_a_subset():
    model = table_model(5, 6)
    codes, _, _ = R.beam_search(model, 4, 1)
    greedy = ()
    for _ in range(4):
        greedy += (int(np.argmax(model(greedy))),)
    assert tuple(codes[0]) == greedy
    totals = dict((s, t) for t, s in brute_force(model, 4))
    codes, scores, _ = R.beam_search(model, 4, 5)
    for row, sc in zip(codes, scores):
        assert abs(totals[tuple(row)] - float(sc)) < 1e-5
    assert len({tuple(r) for r in codes}) == 5 and np.all(np.diff(scores) <= 0)


def test_exact_ties_come_out_by_row_then_code():
    flat = lambda prefix: np.zeros(2)                              # noqa: E731  every plan has total -T log 2: all tie, exactly
    codes, scores, hist = R.beam_search(flat, 3, 8)
    assert [tuple(r) for r in codes] == list(itertools.product((0, 1), repeat=3))        # lexicographic = row, then code
    assert len(set(scores.tolist())) == 1 and hist[2].tolist() == [0, 0, 1, 1, 2, 2, 3, 3]
    cand = np.full((4, R.MAXV), NINF, dtype=F)
    cand[1, 700] = cand[0, 4000] = cand[0, 300] = cand[3, 0] = F(-1.5)
    cand[2, 4095] = F(-1.25)
    anc, code, sc, n, flag = R.select(cand, np.zeros(4, dtype=np.int64), 4)
    assert anc.tolist() == [2, 0, 0, 1] and code.tolist() == [4095, 300, 4000, 700] and n.tolist() == [4] and flag == 1
    assert sc.tolist() == [-1.25, -1.5, -1.5, -1.5]
    cand = np.full((2, R.MAXV), NINF, dtype=F)                     # -0 and +0 tie
    cand[1, 0], cand[0, 1] = F(0.0), F(-0.0)
    anc, code, _, _, _ = R.select(cand, np.zeros(2, dtype=np.int64), 2)
    assert anc.tolist() == [0, 1] and code.tolist() == [1, 0]


def test_dead_slots_all_dead_group_row_lists_and_nan():
    cand = np.full((6, R.MAXV), NINF, dtype=F)
    cand[1, 400], cand[1, 2] = F(-0.5), F(-3.0)
    low = np.array([0, 2, 0, 5, 0, 4095])
    anc, code, sc, n, flag = R.select(cand, low, 3)
    assert n.tolist() == [2, 0] and flag == 1
    assert anc.tolist() == [1, 1, 1, 3, 4, 5] and code.tolist() == [400, 2, 400, 5, 0, 4095]
    assert sc.tolist() == [-0.5, -3.0, NINF, NINF, NINF, NINF]
    cand = np.full((2, R.MAXV), NINF, dtype=F)
    cand[0, 1] = cand[1, 1] = F(-1.0)
    assert R.select(cand, np.zeros(2, dtype=np.int64), 1)[4] == 0                     # the identity leaves the flag down
    # a row's list: its W best, equal scores by ascending code; a row with fewer live candidates hands over fewer
    row = np.full(R.MAXV, NINF, dtype=F)
    row[[5, 17, 1000, 4095]] = [-2.0, -1.0, -2.0, -2.0]
    assert [v for _, v in R.row_best(row, 3)] == [17, 5, 1000] and [v for _, v in R.row_best(row, 64)] == [17, 5, 1000, 4095]
    assert np.all(R.cand64(0.0, np.array([NINF, NINF, NINF]), [0, 1, 2]) == NINF)     # lp is NaN there: NaN counts as -inf
    c = R.cand64(-1.0, np.array([0.0, NINF]), [0, 1])
    assert c[0] == -1.0 and c[1] == NINF and c.shape == (R.MAXV,)
    assert R.cand_bound(1e-6, -10.0) == 1e-6 + 10.0 * 2.0 ** -24


# ---- the host path, recorded ------------------------------------------------------------------------------------------------
def _traced(graph, **kw):
    from test_generation_launches_cpu import ROWS, _prior, _recorder
    prior = _prior()
    kw.setdefault('num_generated_codes', ROWS)
    with _recorder(prior) as (calls, _):
        out = prior.generate_codes(prior.num_tokens + 3, seed=7, use_graph=graph, **kw)
    return [c.split('(', 1)[0] for c in calls], out, prior


@pytest.mark.parametrize('method,stride', [('cached', 1), ('cached', 2), ('forward', 1)])
@pytest.mark.parametrize('graph', [False, True])
def test_host_path_launches_expand_and_select_in_the_samplers_place(graph, method, stride):
    """Recorded launches, no GPU: one expand + select pair per code where the sampler was, followed by the moves of the window's
    codes, the sequence, the logp rows and -- in the cached step only -- both caches; W = 1 launches no move; the public shapes."""
    from test_generation_launches_cpu import ROWS
    form = dict(method=method, window_stride=stride)
    plain, out0, prior = _traced(graph, **form)
    nt = prior.num_tokens + 3
    n_steps = plain.count('vqcpc_prior_sample')
    names, out, _ = _traced(graph, beam=2, return_logp=True, **form)
    assert not [n for n in names if 'sample' in n]
    assert names.count('vqcpc_prior_beam_expand') == names.count('vqcpc_prior_beam_select') == n_steps
    moves = ['vqcpc_particle_permute_i64'] * 2 + ['vqcpc_particle_permute_f32']
    cached = moves + ['vqcpc_particle_permute_cache'] * 2
    tails = set()
    for i, n in enumerate(names):
        if n == 'vqcpc_prior_beam_expand':
            assert names[i + 1] == 'vqcpc_prior_beam_select' and names[i + 2:i + 2 + len(moves)] == moves
            tails.add('cached' if names[i + 2:i + 2 + len(cached)] == cached else 'forward')
    assert tails == {method}
    assert [n for n in names if 'permute' not in n and 'beam' not in n] == [n for n in plain if 'sample' not in n]
    assert out[0].shape == out0.shape == (ROWS, nt) and out[1].shape == out0.shape and out[1].dtype == torch.float32
    names1, _, _ = _traced(graph, beam=1, **form)
    assert not [n for n in names1 if 'permute' in n] and names1.count('vqcpc_prior_beam_select') == n_steps
    codes, beams = _traced(graph, beam=2, return_beams=True, **form)[1]
    assert codes.shape == (2 * ROWS, nt) and beams['scores'].shape == (ROWS, 2)
    assert beams['ancestors'].shape == (nt, 2 * ROWS) and beams['ancestors'].dtype == torch.int32


def test_without_the_keyword_no_launch_changes():
    plain, _, _ = _traced(False)
    assert not [n for n in plain if 'beam' in n or 'permute' in n]


def test_host_path_refuses_before_any_launch():
    for kw, word in ((dict(beam=2, particles=2), 'particles'), (dict(beam=2, temperature=0.5), 'temperature'),
                     (dict(beam=2, top_k=2), 'top_k'), (dict(beam=2, top_p=0.9), 'top_p'), (dict(beam=65), 'beam'),
                     (dict(beam=0), 'beam'), (dict(beam=True), 'beam'), (dict(beam=2.5), 'beam'),
                     (dict(return_beams=True), 'return_beams')):
        with pytest.raises(ValueError, match=word):
            _traced(False, **kw)
    # the stack's own checks
    from test_generation_launches_cpu import _prior, _recorder
    from vqcpc_bach_amd.priors.generation import IncrementalPrior
    prior = _prior()
    N = prior.num_tokens
    with _recorder(prior), torch.no_grad():
        inc = IncrementalPrior(prior, 6)
        with pytest.raises(ValueError, match='particles'):
            inc.start(N + 1, seeds=0, particles=2, beam=2)
        with pytest.raises(ValueError, match='teacher'):
            inc.start(N, seeds=0, teacher=torch.zeros(6, N, dtype=torch.int64), beam=2)
        with pytest.raises(ValueError, match='want_probs'):
            inc.start(N + 1, seeds=0, want_probs=True, beam=2)
        for bad in (4, 0, 65):                                     # not dividing the 6 rows, outside [1, 64]
            with pytest.raises(ValueError, match='beam'):
                inc.start(N + 1, seeds=0, beam=bad)
        inc.start(N + 1, seeds=0, beam=3)
        assert inc.b_score.tolist() == [0.0, NINF, NINF, 0.0, NINF, NINF] and inc.b_hist.shape == (N + 1, 6)
        assert inc.beam_results()['scores'].shape == (2, 3)


def test_the_vectorised_bound_is_the_constrained_references_bound():
    from prior_constrained_reference import logp_bound
    rng = np.random.default_rng(8)
    for V in (1, 17, 1000):
        row = (rng.normal(size=V) * 4).astype(F)
        if V > 2:
            row[1] = NINF
        all_codes = R.logp_bounds(row, logp_bound)
        for code in {0, 1 % V, V // 2, V - 1, int(np.argmax(row)), int(np.argmin(row))}:
            want = logp_bound(row, code)
            assert abs(all_codes[code] - want) <= 1e-12 * max(want, 1e-30), (V, code)


# ---- the digit stages ------------------------------------------------------------------------------------------------------------
def stage_table_model(seed, K, scale=2.0):
    """Next-digit logits as a fixed function of (column, the previous code, the digits of this code so far)."""
    rng = np.random.default_rng(seed)
    tables = {}

    def model(prefix, digits):
        key = (len(prefix),) + tuple(prefix[-1:]) + ('|',) + tuple(digits)
        if key not in tables:
            tables[key] = rng.normal(size=K) * scale
        return tables[key]
    return model


def test_one_codebook_is_the_merged_rule():
    K, T, W = 5, 4, 6
    stage = stage_table_model(11, K)
    merged = lambda prefix: stage(prefix, ())                     # noqa: E731
    constraint, allowed = [-1, 3, -1, -1], [None, None, [1, 4], None]
    want = R.beam_search(merged, T, W, constraint, allowed)
    got = R.product_beam_search(stage, T, W, K, 1, constraint, [None if a is None else [a] for a in allowed])
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.int32), want[1].view(np.int32))
    assert np.array_equal(got[2], want[2]) and np.array_equal(got[3][:, 0], want[2])


@pytest.mark.parametrize('K,ncb,T,W', [(2, 2, 3, 64), (3, 2, 1, 16), (2, 3, 2, 64)])
def test_an_exhaustive_digit_beam_equals_brute_force_over_the_merged_codes(K, ncb, T, W):
    stage = stage_table_model(12, K)

    def merged(prefix):                                           # the joint distribution over the K^ncb codes: the chain rule
        out = np.zeros(K ** ncb)
        for code in range(K ** ncb):
            digs = [(code // K ** j) % K for j in range(ncb)]
            out[code] = sum(R.lp64(stage(prefix, tuple(digs[:j])))[digs[j]] for j in range(ncb))
        return out
    ranking = brute_force(merged, T)
    tot = np.array([t for t, _ in ranking])
    assert len(ranking) <= W and float(np.min(tot[:-1] - tot[1:])) > 1e-4
    codes, scores, hist, _ = R.product_beam_search(stage, T, W, K, ncb)
    assert [tuple(r) for r in codes[:len(ranking)]] == [s for _, s in ranking]
    np.testing.assert_allclose(scores[:len(ranking)], tot, rtol=0, atol=T * ncb * 4 * 2.0 ** -24 * 10)
    assert np.all(scores[len(ranking):] == NINF)


def test_a_narrow_digit_beam_prunes_after_every_digit():
    """W = 1 is the greedy digit chain, which need not be the greedy merged code: digit 0 is fixed before digit 1 is looked at."""
    K, ncb = 3, 2
    stage = stage_table_model(13, K)
    codes, scores, _, _ = R.product_beam_search(stage, 3, 1, K, ncb)
    prefix = ()
    for _ in range(3):
        d0 = int(np.argmax(stage(prefix, ())))
        d1 = int(np.argmax(stage(prefix, (d0,))))
        prefix += (d0 + K * d1,)
    assert tuple(codes[0]) == prefix
    assert R.forced_digit(7, 3, 2, 0) == 1 and R.forced_digit(7, 3, 2, 1) == 2 and R.forced_digit(99, 3, 2, 1) == 2
    assert R.forced_digit(-1, 3, 2, 0) == -1 and R.merged_codes([[1, 2], [0, 0], [2, 2]], 3).tolist() == [7, 0, 8]


def test_ancestor_composition_equals_following_the_stages_one_by_one():
    K, ncb, T, W = 3, 3, 3, 5
    stage = stage_table_model(14, K, scale=3.0)
    codes, _, hist, stage_hist = R.product_beam_search(stage, T, W, K, ncb)
    assert (stage_hist != np.arange(W)).any()                     # rows really move between the stages
    for t in range(T):
        for k in range(W):
            r = k
            for j in range(ncb - 1, -1, -1):                      # slot k after the last stage, back through the stages
                r = int(stage_hist[t, j, r])
            assert hist[t, k] == r
    # and the rows are what the composed ancestors say: row k at column t continues row hist[t][k] of column t - 1
    lines = R.follow_ancestors([codes[:, t] for t in range(T)], hist)
    assert np.array_equal(lines[:, -1], codes[:, -1])
    # the accumulators: stage 0 stores, later stages add one fp32 add each
    st = R.stage_state(2, 2)
    st = R.stage_update(0, [1, 1], [2, 0], np.array([-0.5, -1.5], dtype=F), np.array([-9.0, -0.25], dtype=F), st)
    assert st['digits'].tolist() == [[2, 0], [0, 0]] and st['logp_acc'].tolist() == [-0.5, -1.5] and st['mass_acc'].tolist() == [-0.25, -0.25]
    st = R.stage_update(1, [1, 0], [1, 1], np.array([-1.0, -2.0], dtype=F), np.array([-0.5, 0.0], dtype=F), st)
    assert st['digits'].tolist() == [[0, 1], [2, 1]] and st['logp_acc'].tolist() == [-2.5, -2.5] and st['mass_acc'].tolist() == [-0.25, -0.75]
    assert st['anc_total'].tolist() == [1, 1]


@pytest.mark.parametrize('method,stride', [('cached', 1), ('cached', 2), ('forward', 1)])
def test_host_path_of_a_product_prior_launches_a_pair_per_digit_stage(method, stride):
    from product_codes_helpers import build_prior, prior_cfg
    from test_generation_launches_cpu import ROWS, _recorder
    torch.manual_seed(13)
    prior = build_prior(prior_cfg(4, 2), 'product').eval()
    nt = prior.num_tokens + 3

    def traced(**kw):
        with _recorder(prior) as (calls, _):
            out = prior.generate_codes(nt, seed=7, use_graph=False, num_generated_codes=ROWS, method=method, window_stride=stride, **kw)
        return [c.split('(', 1)[0] for c in calls], out
    plain, out0 = traced()
    stages = plain.count('vqcpc_prior_sample_product')
    assert stages % 2 == 0
    names, (codes, lp, beams) = traced(beam=2, return_logp=True, return_beams=True)
    assert not [n for n in names if 'sample' in n]
    assert names.count('vqcpc_prior_beam_expand_product') == names.count('vqcpc_prior_beam_select_product') == stages
    assert [n for n in names if 'permute' not in n and 'beam' not in n] == [n for n in plain if 'sample' not in n]
    # the moves follow the LAST stage's select only: one set per code
    moves = [i for i, n in enumerate(names) if n == 'vqcpc_particle_permute_i64']
    assert len(moves) == 2 * (stages // 2) and all(names[i - 1] == 'vqcpc_prior_beam_select_product' for i in moves[0::2])
    assert ('vqcpc_particle_permute_cache' in names) == (method == 'cached')
    assert codes.shape == (2 * ROWS, nt) and lp.shape == (2 * ROWS, nt) and beams['scores'].shape == (ROWS, 2)
    assert out0.shape == (ROWS, nt)
