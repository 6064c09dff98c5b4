"""Beam search over code plans (PriorRelative.generate_codes / generate / continue_tokens with `beam`, `return_beams`, `code_beam`;
priors/generation.py `_beam_step`, `_beam_stages`, `_beam_moves`; csrc/prior_beam.hip) on the tiny priors of
tests/test_prior_masked_gpu.py (N = 6, num_tokens 14: the head regime, the first move, the middle moves, a ragged tail), merged
V = 11 and product 2 x 4, the step form pinned to 'cached', to 'cached' at stride 3 and to 'forward' in turn, captured and eager:
  (1) beam=1 is greedy decoding: the top_k = 1 run of the same form bit for bit, and at stride 1 the slow loop with one forward per
      code,
  (2) everything forced is the constrained run, and `scores` the ordered fp32 sum of its logp (a product prior: of its digits'
      log-probabilities, compared with the columns' sums within the rounding of the two chains),
  (3) three two-code columns among forced ones at W = 8: exactly the eight plans, ranked as `score_codes` ranks them,
  (4) every returned row's logp / allowed_mass is bit-equal to a plain run forcing the row's own codes -- which fails when a cache
      move, the move of `seq` or of a record is skipped --, its score is the ordered sum of its logp, and the recorded ancestors
      followed backwards are consistent with the returned rows,
  (5) chunks of whole groups equal groups alone, generate / continue_tokens pass `code_beam` on, and the refusals.
A product prior's search prunes after every digit: its greedy run is the greedy digit chain, and its two-code columns are two values
of digit 0 with the other digits fixed."""
import itertools

import numpy as np
import pytest
import torch

import prior_masked_reference as MR
from test_prior_gpu import fp32_gemms  # noqa: F401  (fixture)
from test_prior_masked_gpu import (NT, N, forced_columns, in_sets, open_for, product_masked_greedy_loop, random_sets, same_bits,
                                   tiny_prior)

pytestmark = pytest.mark.gpu

MODELS = [(11, 1, 'merged'), (4, 2, 'product')]
FORMS = [('cached', 1), ('cached', 3), ('forward', 1)]          # (method, window_stride); stride 3: a ragged last move of two
GAIN = 8.0                                                      # sharper heads: the plans of a group weigh differently
U = 2.0 ** -24


def _sets(rows, K, ncb, seed, cons, share=0.4):
    """Random sets in the model's public form, every forced code (digit) inside its own."""
    if ncb == 1:
        return open_for(random_sets((rows, NT, K), seed, share), cons)
    return open_for(random_sets((rows, NT, ncb, K), seed, max(share, 0.5)), cons, K, ncb)


def _inside(codes, allowed, K, ncb):
    return in_sets(codes, allowed) if ncb == 1 else in_sets(codes, allowed, K, ncb)


def ordered_sum(lp):
    """(rows, NT) float32 -> (rows,) float32: the column-ascending fp32 sum from 0, one add per column."""
    acc = np.zeros(lp.shape[0], dtype=np.float32)
    for c in range(lp.shape[1]):
        acc = (acc + lp[:, c]).astype(np.float32)
    return acc


def scores_are_the_ordered_sum(sc, lp, ncb):
    """sc (rows,) float32 against the rows' logp (rows, NT) float32.  A merged prior adds one logp per column to the score: the
    bits of `ordered_sum`.  A product prior adds one DIGIT's log-probability per stage, (score + lp_0) + lp_1 ..., while a column of
    logp is lp_0 + lp_1 ... rounded on its own: the same NT * ncb terms in another association, so the two agree within the
    rounding of both chains, each at most NT * ncb additions of partial sums no larger than sum |lp|."""
    if ncb == 1:
        return np.array_equal(sc.view(np.int32), ordered_sum(lp).view(np.int32))
    lp = lp.astype(np.float64)
    return bool(np.all(np.abs(sc - lp.sum(axis=1)) <= 2 * NT * ncb * U * np.abs(lp).sum(axis=1)))


# ---- 1. beam = 1 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('method,stride', FORMS)
@pytest.mark.parametrize('K,ncb,model', MODELS)
def test_beam_one_is_greedy_decoding(fp32_gemms, K, ncb, model, method, stride):  # noqa: F811
    prior = tiny_prior(K, ncb, model)
    B, V = 3, K ** ncb
    cons = forced_columns(B, NT, V, 41)
    allowed = _sets(B, K, ncb, 42, cons)
    kw = dict(num_generated_codes=B, method=method, window_stride=stride, constraint=cons, allowed=allowed, return_logp=True,
              return_allowed_mass=True)
    if stride == 1:
        want, gap = (MR.masked_greedy_loop if ncb == 1 else product_masked_greedy_loop)(prior, cons, allowed)[:2]
        assert gap > 2e-5, gap                                   # a precondition on the inputs: the arg-max is defined
    for use_graph in (True, False):
        greedy = prior.generate_codes(NT, top_k=1, seed=0, use_graph=use_graph, **kw)
        codes, lp, mass, beams = prior.generate_codes(NT, beam=1, return_beams=True, seed=123, use_graph=use_graph, **kw)
        assert torch.equal(codes, greedy[0]) and same_bits(lp, greedy[1]) and same_bits(mass, greedy[2])
        assert _inside(codes, allowed, K, ncb) and torch.equal(codes.cpu()[cons >= 0], cons[cons >= 0])
        if stride == 1:
            assert torch.equal(codes, want)
        assert beams['scores'].shape == (B, 1) and beams['ancestors'].shape == (NT, B)
        assert torch.equal(beams['ancestors'].cpu(), torch.arange(B, dtype=torch.int32).expand(NT, -1))
        assert scores_are_the_ordered_sum(beams['scores'].cpu().numpy()[:, 0], lp.cpu().numpy(), ncb)
        only = prior.generate_codes(NT, beam=1, **dict(kw, return_logp=False, return_allowed_mass=False))
        assert torch.equal(only, codes)


# ---- 2. everything forced ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('method,stride', FORMS)
@pytest.mark.parametrize('K,ncb,model', MODELS)
def test_everything_forced_is_the_constrained_run(fp32_gemms, K, ncb, model, method, stride):  # noqa: F811
    prior = tiny_prior(K, ncb, model)
    rows, W, V = 2, 4, K ** ncb
    given = torch.randint(0, V, (rows, NT), generator=torch.Generator().manual_seed(62))
    kw = dict(num_generated_codes=rows, constraint=given, return_logp=True, method=method, window_stride=stride)
    c0, l0 = prior.generate_codes(NT, seed=0, **kw)
    for use_graph in (True, False):
        codes, lp, beams = prior.generate_codes(NT, beam=W, return_beams=True, use_graph=use_graph, **kw)
        assert torch.equal(codes.cpu(), given.repeat_interleave(W, dim=0))         # dead slots copy slot 0
        assert same_bits(lp, l0.repeat_interleave(W, dim=0))
        sc = beams['scores'].cpu().numpy()
        assert scores_are_the_ordered_sum(np.ascontiguousarray(sc[:, 0]), l0.cpu().numpy(), ncb) and np.all(np.isneginf(sc[:, 1:]))
        best, blp = prior.generate_codes(NT, beam=W, use_graph=use_graph, **kw)
        assert torch.equal(best, c0) and same_bits(blp, l0)


# ---- 3. eight plans ------------------------------------------------------------------------------------------------------------
FREE = (2, 8, 13)                                               # the head regime, a middle move, the tail


def _eight_plans(prior, K, ncb, method, stride):
    """Two allowed codes on each column of FREE (a product prior: two values of digit 0, one of every other digit), everything else
    forced.  -> (constraint (1, NT), allowed in the model's public form, the eight plans (8, NT) ranked by their float64 totals
    under `score_codes` of the same form, the totals).  A seed whose totals lie closer than the fp32 running sums may differ is
    rejected here."""
    for seed in range(70, 90):
        g = torch.Generator().manual_seed(seed)
        V = K ** ncb
        cons = torch.randint(0, V, (1, NT), generator=g)
        allowed = torch.ones((1, NT, V) if ncb == 1 else (1, NT, ncb, K), dtype=torch.bool)
        pairs = []
        for c in FREE:
            two = torch.randperm(K, generator=g)[:2].sort()[0]
            allowed[0, c] = False
            cons[0, c] = -1
            if ncb == 1:
                allowed[0, c, two] = True
                pairs.append(two.tolist())
            else:
                rest = torch.randint(0, K, (ncb,), generator=g)
                allowed[0, c, 0, two] = True
                high = 0
                for j in range(1, ncb):
                    allowed[0, c, j, rest[j]] = True
                    high += int(rest[j]) * K ** j
                pairs.append([int(t) + high for t in two])
        plans = cons.repeat(8, 1)
        for i, choice in enumerate(itertools.product(*pairs)):
            plans[i, list(FREE)] = torch.tensor(choice)
        lp = prior.score_codes(plans, method=method, window_stride=stride).double().cpu().numpy()
        total = lp.sum(axis=1)
        order = np.argsort(-total, kind='stable')
        slack = 2 * NT * U * np.abs(lp).sum(axis=1).max()        # an fp32 running sum of NT terms against the float64 sum, twice
        if np.min(-np.diff(total[order])) > 10 * slack:
            return cons, allowed, plans[order], total[order]
    raise AssertionError('no seed separates the eight plans')


@pytest.mark.parametrize('method,stride', FORMS)
@pytest.mark.parametrize('K,ncb,model', MODELS)
def test_three_two_code_columns_give_exactly_the_eight_plans_in_order(fp32_gemms, K, ncb, model, method, stride):  # noqa: F811
    prior = tiny_prior(K, ncb, model, gain=GAIN)
    cons, allowed, plans, total = _eight_plans(prior, K, ncb, method, stride)
    kw = dict(constraint=cons, allowed=allowed, method=method, window_stride=stride, return_logp=True)
    for use_graph in (True, False):
        codes, lp, beams = prior.generate_codes(NT, beam=8, return_beams=True, use_graph=use_graph, **kw)
        assert torch.equal(codes.cpu(), plans), (codes.cpu(), plans)
        sc = beams['scores'].cpu().numpy()[0]
        assert np.all(np.diff(sc) < 0) and np.all(np.abs(sc - total) <= NT * U * np.abs(lp.double().cpu().numpy()).sum(axis=1) + U * np.abs(total))
        # a narrower beam prunes, and what it keeps are plans of the eight with their own totals
        c4, l4, b4 = prior.generate_codes(NT, beam=4, return_beams=True, use_graph=use_graph, **kw)
        index = {tuple(p.tolist()): i for i, p in enumerate(plans)}
        kept = [index[tuple(r.tolist())] for r in c4.cpu()]
        assert len(set(kept)) == 4 and kept == sorted(kept)
        assert same_bits(l4, lp[kept])
        # wider than the plans: dead slots
        c16, _, b16 = prior.generate_codes(NT, beam=16, return_beams=True, use_graph=use_graph, **kw)
        assert torch.equal(c16[:8].cpu(), plans) and torch.equal(c16[8:].cpu(), plans[:1].expand(8, -1))
        assert np.all(np.isneginf(b16['scores'].cpu().numpy()[0, 8:]))


# ---- 4. rows really move ---------------------------------------------------------------------------------------------------------
def _lines(anc):
    """anc (NT, M) -> (M, NT): the slot every final row sat in at each column (row r at column t descends from anc[t][r])."""
    nt, M = anc.shape
    out = np.zeros((M, nt), dtype=np.int64)
    for r in range(M):
        k = r
        for t in range(nt - 1, -1, -1):
            out[r, t] = k
            k = int(anc[t][k])
    return out


@pytest.mark.parametrize('W', [8, 64])
@pytest.mark.parametrize('method,stride', FORMS)
@pytest.mark.parametrize('K,ncb,model', MODELS)
def test_returned_rows_carry_their_ancestors_bits(fp32_gemms, K, ncb, model, method, stride, W):  # noqa: F811
    prior = tiny_prior(K, ncb, model, gain=GAIN)
    rows, V = (2 if W == 8 else 1), K ** ncb
    g = torch.Generator().manual_seed(63)
    cons = torch.full((rows, NT), -1, dtype=torch.int64)
    cons[:, [4, NT - 1]] = torch.randint(0, V, (rows, 2), generator=g)              # forced codes after free ones select prefixes
    allowed = _sets(rows, K, ncb, 64, cons, share=0.5)
    rep = lambda t: t.repeat_interleave(W, dim=0)                                   # noqa: E731
    kw = dict(num_generated_codes=rows, constraint=cons, allowed=allowed, return_logp=True, return_allowed_mass=True, method=method,
              window_stride=stride)
    runs = {}
    for use_graph in (True, False):
        codes, lp, mass, beams = prior.generate_codes(NT, beam=W, return_beams=True, use_graph=use_graph, **kw)
        runs[use_graph] = (codes, lp, mass, beams['scores'], beams['ancestors'])
        assert codes.shape == (rows * W, NT) and _inside(codes, rep(allowed), K, ncb)
        assert torch.equal(codes.cpu()[rep(cons) >= 0], rep(cons)[rep(cons) >= 0])
        sc = beams['scores'].cpu().numpy()
        assert np.isfinite(sc).all() and np.all(np.diff(sc, axis=1) <= 0)          # more than W plans exist: no dead slot
        assert len({tuple(r.tolist()) for r in codes[:W].cpu()}) == W              # W different plans
        anc = beams['ancestors'].cpu().numpy()
        ident = np.arange(rows * W)
        per_col = [int((anc[c] != ident).sum()) for c in range(NT)]
        print(f'{model} {method}/{stride} W={W} (graph {use_graph}): rows moved per column {per_col}')
        # a precondition on the inputs: rows move in the head regime, in the moves and at the tail
        assert sum(per_col[1:N]) > 0 and sum(per_col[N:NT - 2]) > 0 and sum(per_col[NT - 2:]) > 0
        assert bool((anc // W == ident // W).all())
        # every row's scores are those of a plain run forcing the row's own codes
        own, own_lp, own_mass = prior.generate_codes(NT, seed=0, **dict(kw, num_generated_codes=rows * W, constraint=codes.cpu(),
                                                                        allowed=rep(allowed)))
        assert torch.equal(own, codes)
        assert same_bits(lp, own_lp) and same_bits(mass, own_mass)
        assert scores_are_the_ordered_sum(sc.reshape(-1), lp.cpu().numpy(), ncb)
        # the ancestors, read backwards: two final rows that sat in the same slot at column t share everything up to t
        lines, cn = _lines(anc), codes.cpu().numpy()
        for t in range(NT):
            first = {}
            for r in range(rows * W):
                o = first.setdefault(int(lines[r, t]), r)
                assert np.array_equal(cn[r, :t + 1], cn[o, :t + 1]), (t, r, o)
        # slot 0 without return_beams
        best, blp, bmass = prior.generate_codes(NT, beam=W, use_graph=use_graph, **kw)
        assert torch.equal(best, codes[::W]) and same_bits(blp, lp[::W]) and same_bits(bmass, mass[::W])
    for a, b in zip(runs[True], runs[False]):                                        # captured == eager
        assert torch.equal(a, b) if a.dtype != torch.float32 else same_bits(a, b)
    # a group alone is the group among others
    codes, lp, mass, sc, anc = runs[True]
    for gi in range(rows):
        sl = slice(gi * W, (gi + 1) * W)
        c1, l1, m1, b1 = prior.generate_codes(NT, beam=W, return_beams=True, **dict(kw, num_generated_codes=1, constraint=cons[gi:gi + 1],
                                                                                 allowed=allowed[gi:gi + 1]))
        assert torch.equal(c1, codes[sl]) and same_bits(l1, lp[sl]) and same_bits(m1, mass[sl]) and same_bits(b1['scores'], sc[gi:gi + 1])
        assert torch.equal(b1['ancestors'] + gi * W, anc[:, sl])


# ---- 5. chunks, the pipeline, refusals -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('W,rows', [(64, 2), (5, 14)])
@pytest.mark.parametrize('K,ncb,model', MODELS)
def test_chunks_hold_whole_groups(fp32_gemms, K, ncb, model, W, rows):  # noqa: F811
    """W = 64: a chunk holds one group, two groups run as 64 + 64; W = 5: 70 rows run as 60 + 10, not 64 + 6."""
    prior = tiny_prior(K, ncb, model, gain=GAIN)
    cons = forced_columns(rows, NT, K ** ncb, 65, share=0.15)
    allowed = _sets(rows, K, ncb, 66, cons, share=0.5)
    kw = dict(beam=W, return_beams=True, return_logp=True, method='cached')
    codes, lp, beams = prior.generate_codes(NT, num_generated_codes=rows, constraint=cons, allowed=allowed, **kw)
    assert codes.shape == (rows * W, NT) and beams['scores'].shape == (rows, W) and beams['ancestors'].shape == (NT, rows * W)
    anc = beams['ancestors'].cpu()
    assert bool((anc // W == torch.arange(rows * W) // W).all())                      # ancestors are row indices of the whole call
    for gi in sorted({0, rows - 1, min(12, rows - 1)}):
        sl = slice(gi * W, (gi + 1) * W)
        c1, l1, b1 = prior.generate_codes(NT, num_generated_codes=1, constraint=cons[gi:gi + 1], allowed=allowed[gi:gi + 1], **kw)
        assert torch.equal(c1, codes[sl]) and same_bits(l1, lp[sl]) and torch.equal(b1['ancestors'].cpu() + gi * W, anc[:, sl])
        assert same_bits(b1['scores'], beams['scores'][gi:gi + 1])


def test_generate_and_continue_tokens_pass_the_beam_on(fp32_gemms):  # noqa: F811
    from test_generate_gpu import _golden_decoder
    from test_generate_long_gpu import _meta_dataset
    from test_prior_gpu import _golden_prior
    prior, _, _ = _golden_prior('v32')
    dec, _, _ = _golden_decoder('decoder_tiny')
    vocab = [int(v) for v in dec.num_tokens_per_channel]
    nc, epc, E = dec.num_channels, dec.num_events_per_code, dec.data_processor.num_events
    g = torch.Generator().manual_seed(3)
    x = torch.cat([torch.randint(0, v - 3, (1, 2 * epc, 1), generator=g) for v in vocab], dim=2)     # two codes of tokens
    dec.dataloader_generator = _meta_dataset(vocab)
    framed = torch.cat([torch.tensor([v - 1 for v in vocab]).view(1, 1, nc).repeat(1, E - 1, 1),
                        torch.tensor([v - 3 for v in vocab]).view(1, 1, nc), x], dim=1).cuda()
    prior.eval()
    prefix = torch.cat([prior.encode(c) for c in framed.split(E, 1)], dim=1)
    L, new = prefix.shape[1], 5
    total = L + new
    close = torch.full((1, total), -1, dtype=torch.int64)
    close[0, -1] = 19                                                        # the fixed close
    codes, tokens = prior.continue_tokens(x, new, dec, seed=1, code_constraint=close, code_beam=4)
    assert codes.shape == (1, total) and torch.equal(codes[:, :L], prefix) and int(codes[0, -1]) == 19
    assert tokens.shape == (1, x.shape[1] + new * epc, nc) and torch.equal(tokens[:, :x.shape[1]].cpu(), x)
    full = close.clone()
    full[:, :L] = prefix.cpu()
    assert torch.equal(codes, prior.generate_codes(total, constraint=full, beam=4))
    again, _ = prior.continue_tokens(x, new, dec, seed=99, code_constraint=close, code_beam=4)
    assert torch.equal(again, codes)                                         # the plan does not depend on the seed
    kw = dict(pad=[0, 0, 0, 0], start=[1, 1, 1, 1])
    gc, gt = prior.generate(8, dec, num_generated_codes=2, seed=5, code_beam=3, **kw)
    want = prior.generate_codes(8, num_generated_codes=2, beam=3)
    assert torch.equal(gc, want) and torch.equal(gc[0], gc[1]) and gt.shape[0] == 2
    # the whole chain deterministic: the decoder's own beam arrives through the decoder's keywords
    t1 = prior.generate(8, dec, seed=5, code_beam=3, beam=2, **kw)[1]
    t2 = prior.generate(8, dec, seed=6, code_beam=3, beam=2, **kw)[1]
    assert torch.equal(t1, t2)


def test_the_refusals_raise(fp32_gemms):  # noqa: F811
    from vqcpc_bach_amd.priors.generation import IncrementalPrior
    from vqcpc_bach_amd.utils import STEP_LOCK
    prior = tiny_prior(11, 1, 'merged')
    for bad in (0, 65, 2.5, True):
        with pytest.raises(ValueError, match='beam'):
            prior.generate_codes(NT, beam=bad)
    for kw, word in ((dict(particles=2), 'particles'), (dict(temperature=0.9), 'temperature'), (dict(top_k=2), 'top_k'),
                     (dict(top_p=0.5), 'top_p')):
        with pytest.raises(ValueError, match=word):
            prior.generate_codes(NT, beam=2, **kw)
    with pytest.raises(ValueError, match='return_beams'):
        prior.generate_codes(NT, return_beams=True)
    with STEP_LOCK, torch.no_grad():
        inc = IncrementalPrior(prior, 6)
        with pytest.raises(ValueError, match='teacher'):
            inc.start(N, seeds=0, teacher=torch.zeros(6, N, dtype=torch.int64), beam=2)
        with pytest.raises(ValueError, match='want_probs'):
            inc.start(NT, seeds=0, want_probs=True, beam=2)
        with pytest.raises(ValueError, match='particles'):
            inc.start(NT, seeds=0, particles=2, beam=2)
        for bad in (4, 0, 65):                                                       # not dividing the 6 rows, outside [1, 64]
            with pytest.raises(ValueError, match='beam'):
                inc.start(NT, seeds=0, beam=bad)
