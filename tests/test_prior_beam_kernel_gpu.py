"""vqcpc_prior_beam_expand + vqcpc_prior_beam_select (csrc/prior_beam.hip) called directly, against tests/prior_beam_reference.py:
  * `cand_out` against float64 within prior_constrained_reference.logp_bound + u |cand| at every candidate, -inf exactly elsewhere,
  * ancestors, codes, scores, the rows' scratch lists, flag and bound are EXACTLY the reference's function of the kernel's own
    `cand_out` -- no near-tie exemption,
  * logp is bit-equal to vqcpc_prior_sample_constrained forcing the slot's code on the ancestor's row, logmass and the next input row
    to vqcpc_prior_sample_masked's,
  * every output sits in guard cells, unused inputs are NaN / garbage, and a second launch gives the same bits.
V runs around a thread's 16 codes, a wave's 1 024 and the limit; W includes W > V; M is 1, 3 W and 64 (63 for W = 63).
The digit stages (vqcpc_prior_beam_expand_product / vqcpc_prior_beam_select_product), K in {1, 4, 64, 512} x ncb in {1, 2, 3}: every
stage's digits, accumulators, stage scores, composed ancestors and h_next against the reference's chain; the final logp / logmass /
next input row bit-equal to vqcpc_prior_sample_product_masked's chain forcing the emitted code; ncb = 1 bit-equal to the merged pair."""
import numpy as np
import pytest
import torch

import prior_beam_reference as R
from prior_constrained_reference import logp_bound

pytestmark = pytest.mark.gpu

F = np.float32
NINF = -np.inf
N, D = 6, 8                                                      # window and model width of the direct calls
VS = [1, 2, 15, 16, 17, 255, 256, 257, 1000, 4095, 4096]
GROUPS = [(1, 1), (1, 3), (1, 64), (2, 6), (2, 64), (3, 9), (8, 24), (8, 64), (63, 63), (64, 64)]       # (W, M)
GUARD = -12345.0


def _hip():
    from vqcpc_bach_amd import hip
    hip.load()
    return hip


def _pack(sets, V):
    """bool (M, V) -> int32 (M, words) of the kernel's packed sets."""
    M, words = sets.shape[0], (V + 31) // 32
    bits = np.zeros((M, words * 32), dtype=np.uint64)
    bits[:, :V] = sets
    w = (bits.reshape(M, words, 32) << np.arange(32, dtype=np.uint64)).sum(axis=2).astype(np.uint32)
    return w.view(np.int32)


class Case:
    """One column of a beam step on M rows: inputs on the device (leading dimensions wider than the widths, NaN / garbage outside
    what the kernels may read) and guarded outputs."""

    def __init__(self, M, V, W, seed, p=2, w1=3, logits=None, score=None, forced=None, sets=None, ld=N + 7, with_sets=True,
                 with_cons=True, with_win=True):
        rng = np.random.default_rng(seed)
        self.M, self.V, self.W, self.p, self.w1, self.ld = M, V, W, p, w1, ld
        self.col = (w1 + p if w1 >= 0 else -1) if with_win else p
        col = self.col
        self.ldl = V + 3
        lg = np.full((M, self.ldl), np.nan, dtype=F)
        if logits is None:
            logits = (rng.normal(size=(M, V)) * 3).astype(F)
            if V > 2:                                            # masked logits: candidates that are not live
                logits[:, 1:][rng.random((M, V - 1)) < 0.05] = NINF
        lg[:, :V] = logits
        self.logits = lg
        if score is None:                                        # about a third of the rows are dead, as in a young beam
            score = (-rng.random(M) * 20).astype(F)
            score[rng.random(M) < 0.3] = NINF
        self.score = np.asarray(score, dtype=F)
        self.forced = np.full(M, -1, dtype=np.int64) if forced is None else np.asarray(forced, dtype=np.int64)
        if forced is None and with_cons:
            pick = rng.random(M) < 0.25
            self.forced[pick] = rng.integers(0, V + 2, size=int(pick.sum()))       # V, V + 1: clamped
        if sets is None:
            sets = rng.random((M, V)) < 0.5
            sets[rng.random(M) < 0.2] = False                    # no code inside the vocabulary: no restriction
            sets[rng.random(M) < 0.2] = True
        self.sets = np.asarray(sets, dtype=bool)
        words = (V + 31) // 32
        allowed = rng.integers(-2 ** 31, 2 ** 31, size=(M, ld, words), dtype=np.int64).astype(np.int32)
        cons = rng.integers(-3, V, size=(M, ld)).astype(np.int64)
        self.live_col = 0 <= col < ld
        if self.live_col:
            pk = _pack(self.sets, V)
            tail = V % 32
            if tail:                                             # garbage in the bits at and past V: only [0, V) counts
                pk[:, -1] |= np.int32(-1) << np.int32(tail)
            allowed[:, col] = pk
            cons[:, col] = self.forced
        self.with_sets, self.with_cons, self.with_win = with_sets, with_cons, with_win
        dev = 'cuda'
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)             # noqa: E731
        self.d_logits, self.d_score0 = t(lg), t(self.score)
        self.d_allowed = t(allowed) if with_sets else None
        self.d_cons = t(cons) if with_cons else None
        self.d_win = torch.tensor([77, w1], dtype=torch.int32, device=dev) if with_win else None
        self.table = torch.from_numpy(rng.normal(size=(V + 1, D)).astype(F)).to(dev)

    # what the rule sees at this column
    def candidates(self, b):
        on = self.live_col
        forced = int(self.forced[b]) if on and self.with_cons else -1
        allowed = np.nonzero(self.sets[b])[0] if on and self.with_sets else None
        return R.candidate_codes(self.V, forced, allowed)

    def run(self):
        hip, M, V, W, ld, dev = _hip(), self.M, self.V, self.W, self.ld, 'cuda'
        f32, i32 = dict(dtype=torch.float32, device=dev), dict(dtype=torch.int32, device=dev)
        o = self.out = {
            'cand': torch.full((M, W), float('nan'), **f32), 'code': torch.full((M, W), -7, **i32),
            'lp': torch.full((M, W), float('nan'), **f32), 'mass': torch.full((M,), float('nan'), **f32),
            'low': torch.full((M,), -7, **i32), 'lowlp': torch.full((M,), float('nan'), **f32),
            'cand_out': torch.full((M, R.MAXV), float('nan'), **f32),
            'logp': torch.full((M, ld), GUARD, **f32), 'logmass': torch.full((M, ld), GUARD, **f32),
            'codes': torch.full((M, N + 2), -7, dtype=torch.int64, device=dev), 'next_in': torch.full((M, D + 2), GUARD, **f32),
            'score': self.d_score0.clone(), 'anc': torch.full((M + 2,), -7, **i32), 'flag': torch.full((3,), -7, **i32),
            'bound': torch.full((4,), -7, **i32), 'hist': torch.full((ld, M), -7, **i32),
            'pos': torch.tensor([self.p, -7], **i32)}
        hip.call('vqcpc_prior_beam_expand', self.d_logits, self.ldl, V, M, W, self.d_cons, ld, self.d_allowed, ld, self.d_win,
                 o['score'], N, o['pos'], o['cand'], o['code'], o['lp'], o['mass'], o['low'], o['lowlp'], o['cand_out'])
        hip.call('vqcpc_prior_beam_select', o['cand'], o['code'], o['lp'], o['mass'], o['low'], o['lowlp'], V, M, W, o['logp'], ld,
                 o['logmass'], ld, self.d_win, o['codes'], N + 2, N, self.table, V + 1, D, o['next_in'], D + 2, o['score'],
                 o['anc'][1:], o['flag'][1:], o['bound'][1:], o['hist'], ld, o['pos'])
        torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in o.items()}

    def sampler(self, anc, code):
        """vqcpc_prior_sample_constrained / _masked forcing slot k's code on its ancestor's row (and set): -> (logp bits of the
        constrained sampler, logp, logmass and next input row of the masked one)."""
        hip, M, V, ld, dev = _hip(), self.M, self.V, self.ld, 'cuda'
        col = self.col if self.live_col else self.p              # no live column: only the next input row is compared
        idx = torch.from_numpy(anc.astype(np.int64)).to(dev)
        logits = self.d_logits[idx].contiguous()
        cons = torch.full((M, ld), -1, dtype=torch.int64, device=dev)
        cons[:, col] = torch.from_numpy(code.astype(np.int64)).to(dev)
        allowed = None
        if self.with_sets and self.live_col:
            allowed = self.d_allowed[idx].contiguous()
        win = torch.tensor([0, col - self.p], dtype=torch.int32, device=dev)
        seeds = torch.zeros(M, dtype=torch.int64, device=dev)
        outs = []
        for masked in (False, True):
            lp = torch.full((M, ld), GUARD, dtype=torch.float32, device=dev)
            lm = torch.full((M, ld), GUARD, dtype=torch.float32, device=dev)
            codes = torch.zeros(M, N, dtype=torch.int64, device=dev)
            nxt = torch.zeros(M, D, dtype=torch.float32, device=dev)
            pos = torch.tensor([self.p], dtype=torch.int32, device=dev)
            ticket = torch.zeros(1, dtype=torch.int32, device=dev)
            if masked:
                hip.call('vqcpc_prior_sample_masked', logits, self.ldl, V, M, 1.0, 0, 1.0, seeds, cons, ld, lp, ld, win, allowed, ld,
                         lm, ld, codes, N, N, self.table, V + 1, D, nxt, D, None, V, pos, ticket)
            else:
                hip.call('vqcpc_prior_sample_constrained', logits, self.ldl, V, M, 1.0, 0, 1.0, seeds, cons, ld, lp, ld, win, codes,
                         N, N, self.table, V + 1, D, nxt, D, None, V, pos, ticket)
            torch.cuda.synchronize()
            assert codes[:, self.p].cpu().numpy().tolist() == code.tolist()
            outs += [lp[:, col].cpu().numpy(), lm[:, col].cpu().numpy(), nxt.cpu().numpy()]
        return outs[0], outs[3], outs[4], outs[5]


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.int32)


def check(case, label=''):
    """Every property of the module docstring on one case.  -> the kernels' outputs."""
    M, V, W, p, col, ld = case.M, case.V, case.W, case.p, case.col, case.ld
    got = case.run()
    cand = got['cand_out']
    # 1. cand_out: float64 within the bound at the candidates, -inf elsewhere
    worst, low = 0.0, np.zeros(M, dtype=np.int64)
    for b in range(M):
        codes = case.candidates(b)
        low[b] = codes[0] if codes else 0
        row = case.logits[b, :V]
        want = R.cand64(case.score[b], row, codes)
        other = np.ones(R.MAXV, dtype=bool)
        other[codes] = False
        assert np.all(cand[b, other] == NINF), (label, b)
        idx = np.asarray(codes)
        w, g = want[idx], cand[b, idx].astype(np.float64)
        dead = np.isneginf(w)
        assert np.all(g[dead] == NINF) and not np.isnan(g).any(), (label, b)
        bound = R.logp_bounds(row, logp_bound)[idx] + R.U_FP32 * np.abs(np.where(dead, 0.0, w))
        err = np.abs(np.where(dead, 0.0, g - np.where(dead, 0.0, w)))
        worst = max(worst, float((err[~dead] / bound[~dead]).max()) if (~dead).any() else 0.0)
    print(f'{label} V={V} W={W} M={M}: cand_out worst error / bound {worst:.3f}')
    assert worst <= 1.0
    # 2. the selection is the reference's function of the kernel's own cand_out, exactly
    anc, code, sc, n, flag = R.select(cand, low, W)
    assert got['low'].tolist() == low.tolist(), label
    for b in range(M):                                           # the rows' lists in the scratch
        best = R.row_best(cand[b], W)
        k = len(best)
        assert got['cand'][b, :k].tolist() == [float(s) for s, _ in best] and got['code'][b, :k].tolist() == [v for _, v in best]
        assert np.all(got['cand'][b, k:] == NINF), (label, b)
    assert got['anc'][1:1 + M].tolist() == anc.tolist() and got['codes'][:, p].tolist() == code.tolist(), label
    assert np.array_equal(bits(got['score']), bits(sc)), label
    assert got['flag'].tolist() == [-7, flag, -7] and got['bound'].tolist() == [-7, p, col, -7], label
    assert got['pos'].tolist() == [p + 1, -7] and got['anc'][[0, -1]].tolist() == [-7, -7], label
    # 3. logp / logmass / next input: the samplers' bits for the slot's code on the ancestor's row
    lp_c, lp_m, lm_m, nxt = case.sampler(anc, code)
    live = case.live_col
    if live:
        assert np.array_equal(bits(got['logp'][:, col]), bits(lp_c)) and np.array_equal(bits(lp_c), bits(lp_m)), label
        assert np.array_equal(bits(got['logmass'][:, col]), bits(lm_m)), label
        assert got['hist'][col].tolist() == anc.tolist(), label
    assert np.array_equal(bits(got['next_in'][:, :D]), bits(nxt)), label
    # 4. guard cells: nothing but the live column, the position's code and the d columns was written
    for key in ('logp', 'logmass'):
        rest = np.delete(got[key], col, axis=1) if live else got[key]
        assert np.all(rest == F(GUARD)), (label, key)
    assert np.all(np.delete(got['hist'], col, axis=0) == -7 if live else got['hist'] == -7), label
    assert np.all(np.delete(got['codes'], p, axis=1) == -7) and np.all(got['next_in'][:, D:] == F(GUARD)), label
    # 5. a second launch: the same bits
    again = case.run()
    for key in got:
        assert np.array_equal(got[key].view(np.int32) if got[key].dtype == F else got[key],
                              again[key].view(np.int32) if again[key].dtype == F else again[key]), (label, key)
    got['anc_ref'], got['code_ref'] = anc, code
    return got


# ---- the grid ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('W,M', GROUPS)
@pytest.mark.parametrize('V', VS)
def test_expand_and_select_on_random_rows(V, W, M):
    check(Case(M, V, W, seed=1000 * V + 64 * W + M), 'random')


@pytest.mark.parametrize('V,W,M', [(17, 8, 24), (257, 64, 64), (4096, 3, 9), (2, 8, 16), (1000, 63, 63)])
def test_planted_ties(V, W, M):
    """Duplicate integer logits inside a row (lp ties exactly) and identical rows with equal scores: the order is cand, then row,
    then code."""
    rng = np.random.default_rng(V + W)
    logits = rng.integers(-2, 3, size=(M, V)).astype(F)
    logits[1::2] = logits[0::2][:logits[1::2].shape[0]]           # pairs of identical rows
    score = np.repeat((-rng.integers(0, 3, size=(M + 1) // 2)).astype(F), 2)[:M]          # equal (integer) scores within a pair
    case = Case(M, V, W, seed=5, logits=logits, score=score, forced=np.full(M, -1), sets=np.ones((M, V), dtype=bool))
    got = check(case, 'ties')
    cand = got['cand_out'][:, :V]
    assert len(np.unique(cand[np.isfinite(cand)])) < np.isfinite(cand).sum() // 2          # ties really are there
    if M >= 2:
        assert np.array_equal(cand[0].view(np.int32), cand[1].view(np.int32))


@pytest.mark.parametrize('W,M', [(4, 12), (64, 64), (1, 5)])
def test_dead_slots_and_dead_groups(W, M):
    V = 37
    rng = np.random.default_rng(W)
    score = np.full(M, NINF, dtype=F)
    if M // W >= 2:
        score[W] = F(-1.0)                                        # group 1: one live row; the others: all dead
    sets = np.zeros((M, V), dtype=bool)
    sets[:, [5, 9]] = True                                        # two candidates per row: a live row fills two slots
    forced = np.full(M, -1)
    forced[0] = 11                                                # a dead row's lowest candidate is its forced code
    if M > 2 * W:
        score[M - 1] = np.nan                                     # NaN counts as -inf
    got = check(Case(M, V, W, seed=3, score=score, sets=sets, forced=forced), 'dead')
    anc, code = got['anc'][1:1 + M], got['codes'][:, 2]
    assert code[0] == 11 and anc[0] == 0 and np.all(np.isneginf(got['score'][:W]))
    if M // W >= 2 and W >= 2:
        assert anc[W:2 * W].tolist() == [W] * W and sorted(code[W:W + 2].tolist()) == [5, 9]
        assert np.isfinite(got['score'][W:W + 2]).all() and np.all(np.isneginf(got['score'][W + 2:2 * W]))
        assert code[W + 2:2 * W].tolist() == [code[W]] * (W - 2)
    del rng


@pytest.mark.parametrize('V', [16, 300])
def test_window_columns_and_leading_dimensions(V):
    W, M = 4, 8
    base = dict(seed=21)
    check(Case(M, V, W, w1=0, **base), 'win 0')
    got = check(Case(M, V, W, w1=-1, **base), 'no live window')                        # col -1: everything is free, no record written
    assert got['bound'][2] == -1
    got = check(Case(M, V, W, w1=N + 7 - 2, **base), 'column past the leading dimensions')   # col = ld
    assert got['bound'][2] == N + 7
    check(Case(M, V, W, with_win=False, **base), 'win NULL')                            # col = p
    check(Case(M, V, W, with_sets=False, **base), 'no sets')
    check(Case(M, V, W, with_cons=False, **base), 'no constraint')
    check(Case(M, V, W, p=0, **base), 'p 0')
    check(Case(M, V, W, p=N - 1, **base), 'p N - 1')


@pytest.mark.parametrize('p', [-1, N, N + 5])
def test_a_position_outside_the_window_touches_nothing_but_the_flag(p):
    case = Case(8, 40, 4, seed=22, p=p)
    got = case.run()
    assert got['flag'].tolist() == [-7, 0, -7] and got['pos'].tolist() == [p, -7]
    assert np.isnan(got['cand']).all() and np.isnan(got['cand_out']).all() and np.isnan(got['mass']).all()
    assert np.all(got['code'] == -7) and np.all(got['low'] == -7) and np.all(got['anc'] == -7) and np.all(got['bound'] == -7)
    assert np.all(got['logp'] == F(GUARD)) and np.all(got['logmass'] == F(GUARD)) and np.all(got['next_in'] == F(GUARD))
    assert np.all(got['codes'] == -7) and np.all(got['hist'] == -7)
    assert np.array_equal(bits(got['score']), bits(case.score))


@pytest.mark.parametrize('V,W', [(257, 8), (4096, 16)])
def test_a_group_alone_is_the_group_among_others(V, W):
    M = 4 * W
    whole = Case(M, V, W, seed=31)
    got = check(whole, 'among others')
    for g in (0, 3):
        sl = slice(g * W, (g + 1) * W)
        alone = Case(W, V, W, seed=0, logits=whole.logits[sl, :V], score=whole.score[sl], forced=whole.forced[sl], sets=whole.sets[sl])
        one = alone.run()
        assert (one['anc'][1:1 + W] + g * W).tolist() == got['anc'][1 + g * W:1 + (g + 1) * W].tolist()
        assert one['codes'][:, 2].tolist() == got['codes'][sl, 2].tolist()
        for key in ('score', 'cand_out', 'mass'):
            assert np.array_equal(bits(one[key]), bits(got[key][sl])), key
        col = whole.col
        assert np.array_equal(bits(one['logp'][:, col]), bits(got['logp'][sl, col]))
        assert np.array_equal(bits(one['logmass'][:, col]), bits(got['logmass'][sl, col]))


def test_the_launch_functions_refuse_bad_arguments():
    from vqcpc_bach_amd.hip import VqcpcHipError
    hip = _hip()
    case = Case(6, 20, 3, seed=41)
    case.run()
    o = case.out

    def expand(V=20, M=6, W=3, ldl=case.ldl, ld=case.ld, n=N):
        hip.call('vqcpc_prior_beam_expand', case.d_logits, ldl, V, M, W, case.d_cons, ld, case.d_allowed, ld, case.d_win, o['score'],
                 n, o['pos'], o['cand'], o['code'], o['lp'], o['mass'], o['low'], o['lowlp'], None)

    def select(V=20, M=6, W=3, ld=case.ld, d=D, rows=21):
        hip.call('vqcpc_prior_beam_select', o['cand'], o['code'], o['lp'], o['mass'], o['low'], o['lowlp'], V, M, W, o['logp'], ld,
                 o['logmass'], ld, case.d_win, o['codes'], N + 2, N, case.table, rows, d, o['next_in'], D + 2, o['score'],
                 o['anc'], o['flag'], o['bound'], o['hist'], case.ld, o['pos'])
    o['pos'].fill_(N)                                             # a launch that passes the checks does nothing
    for fn in (expand, select):
        for kw in (dict(V=0), dict(V=4097), dict(M=0), dict(M=65), dict(W=0), dict(W=4), dict(W=65, M=65), dict(ld=N - 1)):
            with pytest.raises(VqcpcHipError):
                fn(**kw)
    for kw in (dict(ldl=19), dict(n=0), dict(n=1025)):
        with pytest.raises(VqcpcHipError):
            expand(**kw)
    for kw in (dict(d=0), dict(d=4097), dict(d=D + 3), dict(rows=19)):
        with pytest.raises(VqcpcHipError):
            select(**kw)
    torch.cuda.synchronize()


# ---- the digit stages of a product prior ---------------------------------------------------------------------------------------
def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _sampler_lp_mass(logits, K, code, packed):
    """vqcpc_prior_sample_masked on one column forcing `code` (M,) on the rows of `logits` (M, K) with the packed sets (M, words) or
    None -> (logp, logmass) float32 (M,): lp(row, code) and the row's log-mass with the merged samplers' bits."""
    hip, M = _hip(), logits.shape[0]
    lg, cons = _dev(logits), _dev(np.asarray(code, dtype=np.int64).reshape(M, 1))
    sets = None if packed is None else _dev(packed.reshape(M, 1, -1))
    lp, lm = torch.zeros(M, 1, device='cuda'), torch.zeros(M, 1, device='cuda')
    codes, nxt = torch.zeros(M, 1, dtype=torch.int64, device='cuda'), torch.zeros(M, D, device='cuda')
    table = torch.zeros(K, D, device='cuda')
    pos, ticket = torch.zeros(1, dtype=torch.int32, device='cuda'), torch.zeros(1, dtype=torch.int32, device='cuda')
    hip.call('vqcpc_prior_sample_masked', lg, K, K, M, 1.0, 0, 1.0, torch.zeros(M, dtype=torch.int64, device='cuda'), cons, 1, lp, 1,
             None, sets, 1, lm, 1, codes, 1, 1, table, K, D, nxt, D, None, K, pos, ticket)
    torch.cuda.synchronize()
    return lp[:, 0].cpu().numpy(), lm[:, 0].cpu().numpy()


def _product_chain(K, ncb, W, M, seed, p=2, w1=3, ld=N + 7):
    """All ncb stages of one position through the kernels, every stage checked against the reference.  -> what the last stage
    wrote plus the inputs the caller needs."""
    hip, rng, col = _hip(), np.random.default_rng(seed), w1 + p
    words = (K + 31) // 32
    score = (-rng.random(M) * 20).astype(F)
    score[rng.random(M) < 0.3] = NINF
    stage_logits = [(rng.normal(size=(M, K)) * 3).astype(F) for _ in range(ncb)]
    cons = np.full((M, ld), -1, dtype=np.int64)
    forced = np.where(rng.random(M) < 0.25, rng.integers(0, K ** ncb + 2, size=M), -1)
    cons[:, col] = forced
    sets = rng.random((M, ncb, K)) < 0.6
    sets[rng.random((M, ncb)) < 0.2] = False                      # no digit inside: no restriction
    allowed = rng.integers(-2 ** 31, 2 ** 31, size=(M, ld, ncb, words), dtype=np.int64).astype(np.int32)
    for j in range(ncb):
        pk = _pack(sets[:, j], K)
        if K % 32:
            pk[:, -1] |= np.int32(-1) << np.int32(K % 32)
        allowed[:, col, j] = pk
    h = [(rng.normal(size=(M, D))).astype(F)] + [None] * (ncb - 1)
    dtab = rng.normal(size=(max(ncb - 1, 1), K, D)).astype(F)
    tables = rng.normal(size=(ncb, K, D)).astype(F)
    f32, i32 = dict(dtype=torch.float32, device='cuda'), dict(dtype=torch.int32, device='cuda')
    o = {'cand': torch.full((M, W), float('nan'), **f32), 'code': torch.full((M, W), -7, **i32), 'lp': torch.full((M, W), float('nan'), **f32),
         'mass': torch.full((M,), float('nan'), **f32), 'low': torch.full((M,), -7, **i32), 'lowlp': torch.full((M,), float('nan'), **f32),
         'cand_out': torch.full((M, R.MAXV), float('nan'), **f32),
         'digits': torch.full((M, ncb), -7, **i32), 'logp_acc': torch.full((M,), float('nan'), **f32),
         'mass_acc': torch.full((M,), float('nan'), **f32), 'stage_score': torch.full((M,), float('nan'), **f32),
         'anc_total': torch.full((M,), -7, **i32),
         'logp': torch.full((M, ld), GUARD, **f32), 'logmass': torch.full((M, ld), GUARD, **f32),
         'codes': torch.full((M, N + 2), -7, dtype=torch.int64, device='cuda'), 'next_in': torch.full((M, D + 2), GUARD, **f32),
         'score': _dev(score), 'anc': torch.full((M,), -7, **i32), 'flag': torch.full((1,), -7, **i32),
         'bound': torch.full((2,), -7, **i32), 'hist': torch.full((ld, M), -7, **i32), 'pos': torch.tensor([p], **i32)}
    d_cons, d_allowed, d_win = _dev(cons), _dev(allowed), torch.tensor([77, w1], **i32)
    d_dtab, d_tables = _dev(dtab), _dev(tables)
    d_h = [_dev(h[0])] + [torch.full((M, D + 1), GUARD, **f32) for _ in range(ncb - 1)]
    ldh = [D] + [D + 1] * (ncb - 1)
    state, base, stage_anc, worst = R.stage_state(M, ncb), score, [], 0.0
    for j in range(ncb):
        last = j == ncb - 1
        d_lg = _dev(stage_logits[j])
        hip.call('vqcpc_prior_beam_expand_product', d_lg, K, K, ncb, j, M, W, d_cons, ld, d_allowed, ld, d_win,
                 o['score'] if j == 0 else o['stage_score'], None if j == 0 else o['anc_total'], N, o['pos'], o['cand'], o['code'],
                 o['lp'], o['mass'], o['low'], o['lowlp'], o['cand_out'])
        hip.call('vqcpc_prior_beam_select_product', o['cand'], o['code'], o['lp'], o['mass'], o['low'], o['lowlp'], K, ncb, j, M, W,
                 o['digits'], o['logp_acc'], o['mass_acc'], o['stage_score'], o['anc_total'], None if last else d_h[j], ldh[j],
                 None if last else d_dtab, None if last else d_h[j + 1], D + 1, o['logp'], ld, o['logmass'], ld, d_win, o['codes'],
                 N + 2, N, d_tables, D, o['next_in'], D + 2, o['score'], o['anc'], o['flag'], o['bound'], o['hist'], ld, o['pos'])
        torch.cuda.synchronize()
        got = {k: v.cpu().numpy() for k, v in o.items()}
        # the stage's candidates: the digit of the forced code / the digit set of the stack row the slot descends from
        src = state['anc_total'] if j else np.arange(M)
        cand, low = got['cand_out'], np.zeros(M, dtype=np.int64)
        for b in range(M):
            digs = R.candidate_codes(K, R.forced_digit(int(forced[src[b]]), K, ncb, j), np.nonzero(sets[src[b], j])[0])
            low[b] = digs[0]
            want = R.cand64(base[b], stage_logits[j][b], digs)
            other = np.ones(R.MAXV, dtype=bool)
            other[digs] = False
            assert np.all(cand[b, other] == NINF), (j, b)
            idx = np.asarray(digs)
            w, g = want[idx], cand[b, idx].astype(np.float64)
            dead = np.isneginf(w)
            assert np.all(g[dead] == NINF) and not np.isnan(g).any(), (j, b)
            if (~dead).any():
                bound = R.logp_bounds(stage_logits[j][b], logp_bound)[idx] + R.U_FP32 * np.abs(np.where(dead, 0.0, w))
                worst = max(worst, float((np.abs(g - w)[~dead] / bound[~dead]).max()))
        anc, dig, sc, _, _ = R.select(cand, low, W)
        stage_anc.append(anc)
        # lp(anc, digit) and the rows' masses with the merged samplers' bits, then the reference's chain
        packed = np.stack([allowed[src[b], col, j] for b in range(M)])
        lp_sel, _ = _sampler_lp_mass(stage_logits[j][anc], K, dig, None)
        _, mass_rows = _sampler_lp_mass(stage_logits[j], K, low, packed)
        new = R.stage_update(j, anc, dig, lp_sel, mass_rows, state)
        if not last:
            assert got['digits'][:, :j + 1].tolist() == new['digits'][:, :j + 1].tolist() and np.all(got['digits'][:, j + 1:] == -7)
            assert np.array_equal(bits(got['logp_acc']), bits(new['logp_acc'])) and np.array_equal(bits(got['mass_acc']), bits(new['mass_acc']))
            assert got['anc_total'].tolist() == new['anc_total'].tolist() and np.array_equal(bits(got['stage_score']), bits(sc))
            h[j + 1] = (h[j][anc] + dtab[j][dig]).astype(F)
            hn = d_h[j + 1].cpu().numpy()
            assert np.array_equal(bits(hn[:, :D]), bits(h[j + 1])) and np.all(hn[:, D:] == F(GUARD))
            # an earlier stage leaves the position's outputs alone
            assert np.all(got['codes'] == -7) and np.all(got['next_in'] == F(GUARD)) and np.all(got['logp'] == F(GUARD))
            assert got['pos'].tolist() == [p] and got['flag'].tolist() == [-7] and np.all(got['anc'] == -7)
            assert np.array_equal(bits(got['score']), bits(score))
        state, base = new, sc
    print(f'product K={K} ncb={ncb} W={W} M={M}: cand_out worst error / bound {worst:.3f}')
    assert worst <= 1.0
    # the last stage: the merged select's outputs with the composed ancestors
    at = state['anc_total']
    assert got['codes'][:, p].tolist() == R.merged_codes(state['digits'], K).tolist() and got['anc'].tolist() == at.tolist()
    assert np.array_equal(bits(got['score']), bits(base)) and got['hist'][col].tolist() == at.tolist()
    assert np.array_equal(bits(got['logp'][:, col]), bits(state['logp_acc'])) and np.array_equal(bits(got['logmass'][:, col]), bits(state['mass_acc']))
    nxt = tables[0][state['digits'][:, 0]]
    for i in range(1, ncb):
        nxt = (nxt + tables[i][state['digits'][:, i]]).astype(F)
    assert np.array_equal(bits(got['next_in'][:, :D]), bits(nxt)) and np.all(got['next_in'][:, D:] == F(GUARD))
    assert got['flag'].tolist() == [int((at != np.arange(M)).any())] and got['bound'].tolist() == [p, col] and got['pos'].tolist() == [p + 1]
    assert np.all(np.delete(got['logp'], col, axis=1) == F(GUARD)) and np.all(np.delete(got['codes'], p, axis=1) == -7)
    assert np.all(np.delete(got['hist'], col, axis=0) == -7)
    # the composed ancestors are the stages' followed one by one
    rows_at = [None] * ncb
    r = np.arange(M)
    for j in range(ncb - 1, -1, -1):
        r = stage_anc[j][r]
        rows_at[j] = r
    assert r.tolist() == at.tolist()
    return dict(got=got, state=state, rows_at=rows_at, stage_logits=stage_logits, allowed=allowed, col=col, p=p, ld=ld, tables=tables,
                score=score, cons=cons, sets=sets, forced=forced)


@pytest.mark.parametrize('ncb', [1, 2, 3])
@pytest.mark.parametrize('K', [1, 4, 64, 512])
def test_product_stage_chain(K, ncb):
    """Every stage against the reference, and the final logp / logmass bit-equal to vqcpc_prior_sample_product_masked's chain forcing
    the emitted code on the logits rows the hypothesis read at each stage."""
    hip = _hip()
    for W, M in ((8, 24), (64, 64), (1, 3)):
        c = _product_chain(K, ncb, W, M, seed=100 * K + 10 * ncb + W)
        got, col, p, ld = c['got'], c['col'], c['p'], c['ld']
        at = c['state']['anc_total']
        cons = torch.full((M, ld), -1, dtype=torch.int64, device='cuda')
        cons[:, col] = _dev(got['codes'][:, p])
        allowed = _dev(c['allowed'][at])
        f32, i32 = dict(dtype=torch.float32, device='cuda'), dict(dtype=torch.int32, device='cuda')
        lp, lm = torch.full((M, ld), GUARD, **f32), torch.full((M, ld), GUARD, **f32)
        digits, lacc, macc = torch.zeros(M, ncb, **i32), torch.zeros(M, **f32), torch.zeros(M, **f32)
        codes, nxt = torch.zeros(M, N, dtype=torch.int64, device='cuda'), torch.zeros(M, D, **f32)
        hbuf, hnext, dtab = torch.zeros(M, D, **f32), torch.zeros(M, D, **f32), torch.zeros(max(ncb - 1, 1), K, D, **f32)
        pos, ticket, win = torch.tensor([p], **i32), torch.zeros(1, **i32), torch.tensor([0, col - p], **i32)
        for j in range(ncb):
            last = j == ncb - 1
            lg = _dev(c['stage_logits'][j][c['rows_at'][j]])
            hip.call('vqcpc_prior_sample_product_masked', lg, K, K, ncb, j, M, 1.0, 0, 1.0, torch.zeros(M, dtype=torch.int64, device='cuda'),
                     None, N, cons, ld, lp, ld, win, allowed, ld, lm, ld, digits, lacc, macc, None if last else hbuf, D,
                     None if last else dtab, None if last else hnext, D, codes, N, N, _dev(c['tables']), D, nxt, D, None, K, pos, ticket)
        torch.cuda.synchronize()
        assert codes[:, p].cpu().numpy().tolist() == got['codes'][:, p].tolist()
        assert np.array_equal(bits(lp[:, col].cpu().numpy()), bits(got['logp'][:, col])), (K, ncb, W)
        assert np.array_equal(bits(lm[:, col].cpu().numpy()), bits(got['logmass'][:, col])), (K, ncb, W)
        assert np.array_equal(bits(nxt.cpu().numpy()), bits(got['next_in'][:, :D])), (K, ncb, W)


@pytest.mark.parametrize('K', [1, 4, 64, 512])
def test_one_codebook_through_the_product_entry_points_is_the_merged_pair(K):
    for W, M in ((8, 24), (64, 64)):
        c = _product_chain(K, 1, W, M, seed=7 * K + W)
        sets = c['sets'][:, 0]
        case = Case(M, K, W, seed=0, p=c['p'], w1=c['col'] - c['p'], logits=c['stage_logits'][0], score=c['score'], forced=c['forced'],
                    sets=sets, ld=c['ld'])
        case.table = _dev(c['tables'][0])
        merged, got = case.run(), c['got']
        for key in ('cand', 'code', 'lp', 'mass', 'low', 'lowlp', 'cand_out', 'logp', 'logmass', 'score'):
            a, b = merged[key], got[key]
            assert np.array_equal(bits(a), bits(b)) if a.dtype == F else np.array_equal(a, b), (K, W, key)
        assert merged['codes'].tolist() == got['codes'].tolist() and merged['anc'][1:1 + M].tolist() == got['anc'].tolist()
        assert np.array_equal(bits(merged['next_in']), bits(got['next_in'])) and merged['hist'].tolist() == got['hist'].tolist()
        assert merged['flag'][1] == got['flag'][0] and merged['bound'][1:3].tolist() == got['bound'].tolist()
