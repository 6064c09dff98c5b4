"""Particle resampling for code plans (PriorRelative.generate_codes with `particles`, `resample_threshold`, `return_particles`;
priors/generation.py `_resample`; csrc/particles.hip with U = 1) on the tiny priors of tests/test_prior_masked_gpu.py (N = 6,
num_tokens 14: the head regime, the first move, the middle moves, a ragged tail), merged V = 11 and product 2 x 4, the step form
pinned to 'cached' and to 'forward' in turn, captured and eager:
  (1) resample_threshold = 0 is the plain run with rows * P rows, bit for bit; its weights are the softmax of the summed scores,
      log_evidence their log-mean; everything forced: the evidence is the ordered sum of logp, the weights are equal,
  (2) resample_threshold = 1 with the last 3 codes forced and sets on 2 columns: the recorded ancestors are
      tests/particles_reference.py's function of the recorded weights, and every returned row's logp and allowed_mass are bit-equal to
      a plain run that forces the row's own codes -- which fails when a cache move, the move of `seq` or of the next input row is
      skipped; groups alone == groups among others; chunks of whole groups,
  (3) the refusals."""
import numpy as np
import pytest
import torch

import particles_reference as R
from test_generate_particles_gpu import _check_history, _seeds
from test_prior_gpu import fp32_gemms  # noqa: F401  (fixture)
from test_prior_masked_gpu import NT, N, digits_of, open_for, same_bits, tiny_prior

pytestmark = pytest.mark.gpu

MODELS = [(11, 1, 'merged'), (4, 2, 'product')]
FORMS = [('cached', 1), ('cached', 3), ('forward', 1)]          # (method, window_stride); stride 3: a ragged last move of two
SET_COLUMNS = (2, 7)                                     # head regime; a middle move (stride 3: inside a move, a cached step follows)
FORCED = 3                                               # the last codes of the plan
GAIN = 8.0                                               # sharper heads: the particles of a group weigh differently


def _plan(K, ncb, rows, seed):
    """The last FORCED codes given, narrow sets on SET_COLUMNS, everything else free.  -> (constraint (rows, NT), allowed)."""
    g = torch.Generator().manual_seed(seed)
    V = K ** ncb
    cons = torch.full((rows, NT), -1, dtype=torch.int64)
    cons[:, NT - FORCED:] = torch.randint(0, V, (rows, FORCED), generator=g)
    if ncb == 1:
        allowed = torch.ones(rows, NT, V, dtype=torch.bool)
        for c in SET_COLUMNS:
            allowed[:, c] = torch.rand(rows, V, generator=g) < 0.3
            allowed[:, c].scatter_(1, torch.randint(0, V, (rows, 1), generator=g), True)
        return cons, allowed
    allowed = torch.ones(rows, NT, ncb, K, dtype=torch.bool)
    for c in SET_COLUMNS:
        allowed[:, c] = torch.rand(rows, ncb, K, generator=g) < 0.4
        allowed[:, c].scatter_(2, torch.randint(0, K, (rows, ncb, 1), generator=g), True)
    return cons, open_for(allowed, cons, K, ncb)


def _scores(cons_rows, lp, mass):
    """Per (row, column) what the filter adds to the log-weight: logp where forced, else the allowed mass."""
    return torch.where(cons_rows.to(lp.device) >= 0, lp, mass).double().cpu().numpy()


# ---- 1. threshold 0, everything forced ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('method,stride', FORMS)
@pytest.mark.parametrize('K,ncb,model', MODELS)
def test_threshold_zero_is_the_plain_run_with_P_times_the_rows(fp32_gemms, K, ncb, model, method, stride):  # noqa: F811
    prior = tiny_prior(K, ncb, model)
    rows, P = 2, 3
    cons, allowed = _plan(K, ncb, rows, 61)
    kw = dict(seed=9, method=method, window_stride=stride, temperature=1.1, return_logp=True, return_allowed_mass=True)
    rep = lambda t: t.repeat_interleave(P, dim=0)                                   # noqa: E731
    for use_graph in (True, False):
        codes, lp, mass = prior.generate_codes(NT, num_generated_codes=rows * P, constraint=rep(cons), allowed=rep(allowed),
                                               use_graph=use_graph, **kw)
        pc, plp, pmass, info = prior.generate_codes(NT, num_generated_codes=rows, constraint=cons, allowed=allowed, particles=P,
                                                    resample_threshold=0.0, return_particles=True, use_graph=use_graph, **kw)
        assert torch.equal(pc, codes) and same_bits(plp, lp) and same_bits(pmass, mass)
        assert info['weights'].shape == (rows, P) and info['log_evidence'].shape == (rows,)
        assert info['ancestors'].shape == (NT, rows * P) and info['ancestors'].dtype == torch.int32
        assert torch.equal(info['ancestors'].cpu(), torch.arange(rows * P, dtype=torch.int32).expand(NT, -1))
        # the weights: softmax over the group of the summed forced logp and free logmass (float64 sums of the fp32 scores); the
        # bounds of tests/particles_reference.py plus the fp32 running sum of a row's NT scores
        score = _scores(rep(cons), lp, mass)
        assert (score[:, list(SET_COLUMNS)] < 0).any() and (score[:, NT - FORCED:] < 0).all()
        total, mag = score.sum(axis=1), np.abs(score).sum(axis=1)
        worst = 0.0
        for g in range(rows):
            sl = slice(g * P, (g + 1) * P)
            wn64, _, inc64, dmax = R.group_weights64(total[sl])
            sum_err = NT * R.EPS * mag[sl].max()
            bound = R.wn_bound(wn64, dmax, P) + 2.0 * sum_err * wn64
            worst = max(worst, float((np.abs(info['weights'][g].cpu().numpy() - wn64) / bound).max()))
            b_ev = R.inc_bound(float(total[sl].max()), inc64, dmax, P) + sum_err
            worst = max(worst, abs(float(info['log_evidence'][g]) - inc64) / b_ev)
        print(f'{model} {method}/{stride} (graph {use_graph}): weights and evidence, worst error / bound {worst:.3f}')
        assert worst <= 1.0
        # without return_particles: the shapes of a call without the keyword, forced codes in place
        sc, slp, smass = prior.generate_codes(NT, num_generated_codes=rows, constraint=cons, allowed=allowed, particles=P,
                                              resample_threshold=0.0, use_graph=use_graph, **kw)
        assert sc.shape == (rows, NT) and slp.shape == smass.shape == (rows, NT)
        assert torch.equal(sc.cpu()[cons >= 0], cons[cons >= 0])


@pytest.mark.parametrize('K,ncb,model', MODELS)
def test_with_everything_forced_the_evidence_is_the_ordered_sum_of_logp(fp32_gemms, K, ncb, model):  # noqa: F811
    prior = tiny_prior(K, ncb, model)
    rows, P = 2, 2
    given = torch.randint(0, K ** ncb, (rows, NT), generator=torch.Generator().manual_seed(62))
    codes, lp, info = prior.generate_codes(NT, num_generated_codes=rows, constraint=given, particles=P, resample_threshold=1.0,
                                           return_logp=True, return_particles=True, seed=1, method='cached')
    assert torch.equal(codes.cpu(), given.repeat_interleave(P, dim=0))
    assert same_bits(lp[0::2], lp[1::2])                                          # the particles of a group are the same row
    assert bool((info['weights'] == 0.5).all())                                   # equal weights: wn = 1 / 2 exactly, ess = 2:
    assert torch.equal(info['ancestors'].cpu(), torch.arange(rows * P, dtype=torch.int32).expand(NT, -1))    # never below 1.0 * P
    # lw is the fp32 sum of logp in column order, one add each; the last code's increment (mx + log 2) - log 2 carries it
    lw = np.zeros(rows * P, dtype=np.float32)
    lpn = lp.cpu().numpy()
    for c in range(NT):
        lw = R.update_lw(lw, c, 1, given.repeat_interleave(P, dim=0).numpy(), lpn, None)
    for g in range(rows):
        ordered = float(lw[g * P])
        bound = R.inc_bound(ordered, ordered, 0.0, P)
        err = abs(float(info['log_evidence'][g]) - ordered)
        print(f'{model}: |log_evidence - ordered sum of logp| = {err:.3e}, bound {bound:.3e}')
        assert err <= bound


# ---- 2. threshold 1: rows really move -------------------------------------------------------------------------------------------
def _own_codes(prior, codes, allowed_rows, method, stride):
    """logp and allowed_mass of a plain run (no particles, as many rows) that forces every row's own codes."""
    out, lp, mass = prior.generate_codes(NT, num_generated_codes=codes.shape[0], constraint=codes.cpu(), allowed=allowed_rows,
                                         return_logp=True, return_allowed_mass=True, seed=0, method=method, window_stride=stride)
    assert torch.equal(out, codes)
    return lp, mass


@pytest.mark.parametrize('method,stride', FORMS)
@pytest.mark.parametrize('K,ncb,model', MODELS)
def test_resampled_rows_carry_their_ancestors_bits(fp32_gemms, K, ncb, model, method, stride):  # noqa: F811
    prior = tiny_prior(K, ncb, model, gain=GAIN)
    rows, P = 2, 16
    cons, allowed = _plan(K, ncb, rows, 63)
    rep = lambda t: t.repeat_interleave(P, dim=0)                                   # noqa: E731
    kw = dict(seed=21, constraint=cons, allowed=allowed, particles=P, resample_threshold=1.0, return_logp=True,
              return_allowed_mass=True, method=method, window_stride=stride, num_generated_codes=rows)
    seeds = _seeds(21, rows * P)
    runs = {}
    for use_graph in (True, False):
        codes, lp, mass, info = prior.generate_codes(NT, return_particles=True, use_graph=use_graph, **kw)
        sc, slp, smass = prior.generate_codes(NT, use_graph=use_graph, **kw)
        runs[use_graph] = (codes, lp, mass, info['ancestors'], info['wn'], sc, slp, smass)
        forced = rep(cons) >= 0
        assert torch.equal(codes.cpu()[forced], rep(cons)[forced]) and torch.equal(sc.cpu()[cons >= 0], cons[cons >= 0])
        digs = codes.cpu() if ncb == 1 else digits_of(codes.cpu(), K, ncb)
        assert bool(rep(allowed).gather(-1, digs.unsqueeze(-1)).all())
        # the ancestors: the reference's function of the stored weights, code by code
        moved = _check_history(info, seeds, P, 1.0, list(range(NT)), final_forced=False)
        anc = info['ancestors'].cpu().numpy()
        ident = np.arange(rows * P)
        assert all((anc[c] == ident).all() for c in range(SET_COLUMNS[0]))            # equal weights: ess = P exactly, no move
        per_code = [int((anc[c] != ident).sum()) for c in range(NT)]
        print(f'{model} {method}/{stride} (graph {use_graph}): {moved} rows moved, per code {per_code}')
        # a precondition on the inputs: rows move in the head regime, in a middle move and at the forced close
        assert per_code[SET_COLUMNS[0]] > 0 and per_code[SET_COLUMNS[1]] > 0 and per_code[NT - FORCED] > 0
        # the weights at the first restricted column are the softmax of that column's masses: nothing has moved before it, so
        # they are the threshold-0 run's column (same seeds)
        _, _, mass0 = prior.generate_codes(NT, use_graph=use_graph, **dict(kw, resample_threshold=0.0, return_particles=False,
                                                                           num_generated_codes=rows * P, particles=None,
                                                                           constraint=rep(cons), allowed=rep(allowed)))
        first = mass0[:, SET_COLUMNS[0]].double().cpu().numpy()
        for g in range(rows):
            sl = slice(g * P, (g + 1) * P)
            wn64, _, _, dmax = R.group_weights64(first[sl])
            got = info['wn'][SET_COLUMNS[0], sl].cpu().numpy()
            assert (np.abs(got - wn64) <= R.wn_bound(wn64, dmax, P)).all(), (g, got, wn64)
        # every returned row's scores are those of a plain run forcing the row's own codes: the moved caches, `seq` and next input
        # row are the ancestor's bits
        own_lp, own_mass = _own_codes(prior, codes, rep(allowed), method, stride)
        assert same_bits(lp, own_lp) and same_bits(mass, own_mass)
        own_lp, own_mass = _own_codes(prior, rep(sc), rep(allowed), method, stride)
        assert same_bits(slp, own_lp[::P]) and same_bits(smass, own_mass[::P])
    for a, b in zip(runs[True], runs[False]):                                        # captured == eager
        assert torch.equal(torch.nan_to_num(a.float(), nan=-7.0), torch.nan_to_num(b.float(), nan=-7.0))
    # a group alone is the group among others
    codes, lp, mass = runs[True][:3]
    s = torch.from_numpy(seeds)
    for g in range(rows):
        sl = slice(g * P, (g + 1) * P)
        c1, l1, m1, i1 = prior.generate_codes(NT, return_particles=True, **dict(kw, seed=s[sl], num_generated_codes=1,
                                                                                constraint=cons[g:g + 1], allowed=allowed[g:g + 1]))
        assert torch.equal(c1, codes[sl]) and same_bits(l1, lp[sl]) and same_bits(m1, mass[sl]), g
        assert torch.equal(i1['ancestors'] + g * P, runs[True][3][:, sl])


def test_chunks_hold_whole_groups(fp32_gemms):  # noqa: F811
    """24 rows of P = 5: 120 rows of the stack run as 60 + 60 (12 groups each), not 64 + 56."""
    prior = tiny_prior(11, 1, 'merged', gain=GAIN)
    rows, P = 24, 5
    cons, allowed = _plan(11, 1, rows, 64)
    kw = dict(seed=5, particles=P, resample_threshold=1.0, return_logp=True, return_particles=True, method='cached')
    codes, lp, info = prior.generate_codes(NT, num_generated_codes=rows, constraint=cons, allowed=allowed, **kw)
    assert codes.shape == (rows * P, NT) and info['weights'].shape == (rows, P) and info['ancestors'].shape == (NT, rows * P)
    anc = info['ancestors'].cpu()
    assert bool((anc // P == torch.arange(rows * P) // P).all())                      # ancestors are row indices of the whole call
    seeds = torch.from_numpy(_seeds(5, rows * P))
    for g in (0, 11, 12, 23):
        sl = slice(g * P, (g + 1) * P)
        c1, l1, i1 = prior.generate_codes(NT, num_generated_codes=1, constraint=cons[g:g + 1], allowed=allowed[g:g + 1],
                                          **dict(kw, seed=seeds[sl]))
        assert torch.equal(c1, codes[sl]) and same_bits(l1, lp[sl]) and torch.equal(i1['ancestors'].cpu() + g * P, anc[:, sl])


# ---- 3. refusals -------------------------------------------------------------------------------------------------------------------
def test_the_refusals_raise(fp32_gemms):  # noqa: F811
    from vqcpc_bach_amd.priors.generation import IncrementalPrior
    from vqcpc_bach_amd.utils import STEP_LOCK
    prior = tiny_prior(11, 1, 'merged')
    for bad in (1, 65, 2.5, True):
        with pytest.raises(ValueError, match='particles'):
            prior.generate_codes(NT, particles=bad)
    for bad in (-0.1, 1.5):
        with pytest.raises(ValueError, match='resample_threshold'):
            prior.generate_codes(NT, particles=2, resample_threshold=bad)
    with pytest.raises(ValueError, match='return_particles'):
        prior.generate_codes(NT, return_particles=True)
    with STEP_LOCK, torch.no_grad():
        inc = IncrementalPrior(prior, 6)
        with pytest.raises(ValueError, match='teacher'):
            inc.start(N, seeds=0, teacher=torch.zeros(6, N, dtype=torch.int64), particles=2)
        with pytest.raises(ValueError, match='want_probs'):
            inc.start(NT, seeds=0, want_probs=True, particles=2)
        for bad in (4, 1, 65):                                                       # not dividing the 6 rows, outside [2, 64]
            with pytest.raises(ValueError, match='particles'):
                inc.start(NT, seeds=0, particles=bad)
        with pytest.raises(ValueError, match='resample_threshold'):
            inc.start(NT, seeds=0, particles=2, resample_threshold=1.01)
