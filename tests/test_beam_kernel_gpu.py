"""vqcpc_decode_beam_select (csrc/beam.hip) by direct calls.  Every launch of this file goes through `check`, which leaves no case
out of any comparison:

  * `cand_out`, every row's candidate scores as the selection used them, against float64 within the derived bound -- the logp bound
    of tests/constrained_reference.py plus one rounding of the add (`beam_reference.cand_bound`) -- and exactly -inf off the
    candidate set; the worst ratio is returned and recorded in the docstrings below;
  * ancestors / tokens / score / flag / bound / pos are EXACTLY `beam_reference.select` of the kernel's own cand_out;
  * logp of slot k has the bits vqcpc_decode_sample_constrained writes for the ancestor row forced to the slot's token (the same
    call pins the tokens and next_in rows), logmass the bits vqcpc_decode_sample_masked writes for the ancestor;
  * rule_report and the history row; every guard cell; and a second launch on the same inputs gives the same bits.

Conventions as in tests/test_decode_sample_constrained_gpu.py: outputs sit in sentinel-filled allocations with guard rows and wider
leading dimensions, logits are NaN outside the position's voice, the sets of every column the step must not read are garbage."""
import ctypes

import numpy as np
import pytest
import torch

import beam_reference as R
import constrained_reference as C
from test_decode_kernels_gpu import GR, NAN, Buf, _i32_words, call, gen, same_bits
from test_decode_sample_constrained_gpu import D_
from test_decode_sample_masked_gpu import mask_buf, put, random_sets

pytestmark = pytest.mark.gpu

NINF = float('-inf')
MW = [(1, 1), (2, 2), (3, 3), (63, 3), (64, 64), (64, 2)]
VS = [1, 2, 63, 64, 65, 255, 256]


@pytest.fixture(scope='module', autouse=True)
def _lib():
    from vqcpc_bach_amd import hip
    hip.load()
    return hip


def lp_bounds(row):
    """`constrained_reference.logp_bound(row, v)` for every token v of the fp32 row at once (the same terms, vectorised)."""
    r = torch.as_tensor(row, dtype=torch.float64)
    u = C.U_FP32
    g9 = 9 * u / (1.0 - 9 * u)
    d = r - r.max()
    p = torch.softmax(r, dim=-1)
    da = d.abs().masked_fill(p == 0, 0.0)
    ds = float((p * (u * da * torch.exp(u * da) + 2 * u * C.ULP_EXP)).sum()) * (1.0 + g9) + g9 + r.numel() * 2.0 ** -126
    L = float(torch.log(torch.exp(d).sum()))
    out = ds * (1.0 + ds) + 2 * u * C.ULP_LOG * abs(L) + u * d.abs() + u * (d - L).abs()
    return out.masked_fill(r == NINF, 0.0).numpy()


class Spec:
    """One launch: M rows in groups of W at position `pos` of nc = len(widths) voices.  forced: None, 'all', 'mixed' or an (M,)
    int64 tensor; sets: None or bool (M, 256); exclude: token ids of the position's voice; scores: 'start', 'random' or (M,) fp32;
    win: None or the live window index w0 (< 0: no live window); ld_*: the option buffers' leading dimensions (default: past the
    column); `rows` (M, V) are the voice's logits, to be edited before `launch`."""

    def __init__(self, M, W, widths, pos=0, T=4, U=1, win=None, seed=0, forced=None, sets=None, exclude=(), scores='random',
                 scale=2.0, ld_cons=None, ld_allow=None, ld_logp=None, ld_mass=None, ld_rep=None, hist_rows=None, report=True,
                 mass=True):
        self.M, self.W, self.widths, self.pos, self.T, self.U, self.win = M, W, tuple(widths), pos, T, U, win
        self.nc = nc = len(widths)
        g = gen(seed)
        self.live = 0 <= pos < T
        self.c = c = pos % nc if self.live else 0
        self.V = V = widths[c]
        self.col = (pos if win is None else win * U + pos if win >= 0 else -1) if self.live else -1
        self.width = width = max(self.col + 1, T) + 1
        self.off = np.concatenate([[0], np.cumsum(widths)]).astype(int)
        self.offs = (ctypes.c_int32 * (nc + 1))(*self.off.tolist())
        self.ldl = int(self.off[-1]) + 6
        self.rows = torch.randn(M, V, generator=g) * scale
        if isinstance(scores, str):
            s = -5.0 * torch.rand(M, generator=g)
            s[torch.rand(M, generator=g) < 0.15] = NINF
            scores = torch.from_numpy(R.start_scores(M, W)) if scores == 'start' else s
        self.scores = scores.float()
        if isinstance(forced, str):
            f = torch.randint(0, V, (M,), generator=g)
            f[torch.rand(M, generator=g) < 0.2] = 300                      # clamped to V - 1
            forced = f if forced == 'all' else torch.where(torch.rand(M, generator=g) < 0.5, f, torch.full_like(f, -1))
        self.forced, self.sets, self.exclude = forced, sets, tuple(exclude)
        self.ld = dict(cons=ld_cons or width + 1, allow=ld_allow or width + 1, logp=ld_logp or width + 2, mass=ld_mass or width + 3,
                       rep=ld_rep or width + 1)
        self.hist_rows = width if hist_rows is None else hist_rows
        self.want_report, self.want_mass = report, mass
        self.table_rows = max(widths) * U + 1
        self.table = (torch.arange(self.table_rows, dtype=torch.float32).view(-1, 1) * 4 + torch.arange(D_, dtype=torch.float32)).cuda()
        words = np.zeros(nc * 8, np.int64)
        for t in self.exclude:
            words[c * 8 + t // 32] |= 1 << (t % 32)
        self.excl = _i32_words(words) if self.exclude else None
        self.seed = seed

    def logits(self, idx=None):
        full = torch.full((self.M, self.ldl), NAN)
        full[:, self.off[self.c]:self.off[self.c + 1]] = self.rows
        return (full if idx is None else full[idx]).cuda().contiguous()

    def reads(self, name):
        """The kernel reads / writes the option buffer `name` at the live column."""
        return 0 <= self.col < self.ld[name]

    def candidates(self, b):
        f = -1 if self.forced is None or not self.reads('cons') else int(self.forced[b])
        a = None if self.sets is None or not self.reads('allow') else torch.nonzero(self.sets[b]).flatten().tolist()
        return R.candidate_tokens(self.V, f, a, self.exclude)


def launch(sp, group=None):
    """One vqcpc_decode_beam_select launch of sp (group: that group alone, an M' = W call on the same rows) -> its buffers."""
    idx = torch.arange(sp.M) if group is None else torch.arange(group * sp.W, (group + 1) * sp.W)
    M, T, width, ld, g = len(idx), sp.T, sp.width, sp.ld, gen(sp.seed + 77)
    o = dict(idx=idx, M=M)
    o['tokens'] = Buf(M, T, T + 3, dtype=torch.int64)
    o['next'] = Buf(M, D_, D_ + 3)
    o['logp'] = Buf(M, min(width, ld['logp']), ld['logp'], data=torch.full((M, min(width, ld['logp'])), NAN))
    o['mass'] = Buf(M, min(width, ld['mass']), ld['mass'], data=torch.full((M, min(width, ld['mass'])), NAN)) if sp.want_mass else None
    rep = torch.randint(0, 1 << 20, (sp.M, width), generator=g, dtype=torch.int32)[idx][:, :min(width, ld['rep'])]
    o['rep'] = Buf(M, rep.shape[1], ld['rep'], data=rep, dtype=torch.int32) if sp.want_report else None
    o['score'] = Buf(1, M, M + 3, data=sp.scores[idx])
    o['anc'] = Buf(1, M, M + 3, dtype=torch.int32)
    o['flag'], o['bound'] = Buf(1, 1, 4, dtype=torch.int32), Buf(1, 2, 5, dtype=torch.int32)
    o['hist'] = Buf(sp.hist_rows, M, M, dtype=torch.int32) if sp.hist_rows else None
    o['cand'] = Buf(M, 256, 256)
    o['pos'] = torch.full((1,), sp.pos, dtype=torch.int32, device='cuda')
    cons = None
    if sp.forced is not None:
        cons = torch.randint(-1, 5, (M, ld['cons']), generator=g)
        if sp.reads('cons'):
            cons[:, sp.col] = sp.forced[idx]
        cons = cons.cuda()
    al = None
    if sp.sets is not None:
        al = mask_buf(M, min(width, ld['allow']), ld['allow'], sp.seed + 5)
        if sp.reads('allow'):
            put(al, sp.col, sp.sets[idx])
    win = None if sp.win is None else torch.tensor([123, sp.win], dtype=torch.int32, device='cuda')
    o['args'] = lambda: (sp.logits(idx), sp.ldl, sp.offs, sp.nc, M, sp.W, sp.excl, cons, ld['cons'], None if al is None else al.view,
                         ld['allow'], o['logp'].view, ld['logp'], None if o['mass'] is None else o['mass'].view, ld['mass'],
                         None if o['rep'] is None else o['rep'].view, ld['rep'], win, o['tokens'].view, T + 3, T, sp.table,
                         sp.table_rows, D_, sp.U, o['next'].view, D_ + 3, o['score'].view, o['anc'].view, o['flag'].view,
                         o['bound'].view, None if o['hist'] is None else o['hist'].view, sp.hist_rows, o['cand'].view, o['pos'])
    call('vqcpc_decode_beam_select', *o['args']())
    torch.cuda.synchronize()
    if al is not None:
        al.assert_untouched()
    return o


def _expect(buf, col, values):
    """Nothing of `buf` but column `col` of its logical rows changed, and that column holds exactly `values`' bits."""
    exp = buf.before.clone()
    if col is not None:
        exp[GR:GR + buf.rows, col] = values.to(exp.device).to(exp.dtype)
    if not same_bits(exp, buf.full):
        at = torch.nonzero(exp.view(torch.int32 if exp.dtype == torch.float32 else exp.dtype) !=
                           buf.full.view(torch.int32 if exp.dtype == torch.float32 else exp.dtype))
        r, c = (int(v) for v in at[0])
        raise AssertionError(f'{len(at)} cells differ, the first at allocation row {r}, column {c}: expected {exp[r, c].item()!r}, '
                             f'got {buf.full[r, c].item()!r}')


def sampler_logp(sp, anc, tok):
    """What vqcpc_decode_sample_constrained writes for rows `anc` forced to `tok`: (logp column, next_in, tokens column)."""
    M, T = len(anc), sp.T
    cons = torch.full((M, T), -1, dtype=torch.int64)
    cons[:, sp.pos] = torch.as_tensor(tok)
    lp, tokens, nxt = Buf(M, T, T + 2, data=torch.full((M, T), NAN)), Buf(M, T, T + 3, dtype=torch.int64), Buf(M, D_, D_ + 3)
    pos = torch.full((1,), sp.pos, dtype=torch.int32, device='cuda')
    seeds = torch.arange(M, dtype=torch.int64, device='cuda')
    call('vqcpc_decode_sample_constrained', sp.logits(torch.as_tensor(anc, dtype=torch.int64)), sp.ldl, sp.offs, sp.nc, M, 1.0, 0, 1.0,
         None, seeds, cons.cuda(), T, lp.view, T + 2, None, tokens.view, T + 3, T, sp.table, sp.table_rows, D_, sp.U, nxt.view, D_ + 3,
         None, 0, pos)
    torch.cuda.synchronize()
    return lp.view[:, sp.pos].clone(), nxt.view.clone(), tokens.view[:, sp.pos].clone()


def sampler_mass(sp):
    """What vqcpc_decode_sample_masked writes into logmass for every row of sp with its set."""
    M, T = sp.M, sp.T
    al = None
    if sp.sets is not None and sp.reads('allow'):
        al = mask_buf(M, T, T, 3)
        put(al, sp.pos, sp.sets)
    lm, tokens, nxt = Buf(M, T, T, data=torch.full((M, T), NAN)), Buf(M, T, T, dtype=torch.int64), Buf(M, D_, D_)
    pos = torch.full((1,), sp.pos, dtype=torch.int32, device='cuda')
    seeds = torch.arange(M, dtype=torch.int64, device='cuda')
    call('vqcpc_decode_sample_masked', sp.logits(), sp.ldl, sp.offs, sp.nc, M, 1.0, 0, 1.0, None, seeds, None, 0, None, 0, None,
         None if al is None else al.view, T, lm.view, T, tokens.view, T, T, sp.table, sp.table_rows, D_, sp.U, nxt.view, D_, None, 0, pos)
    torch.cuda.synchronize()
    return lm.view[:, sp.pos].clone()


def check(sp, label, group=None, again=True):
    """Every comparison of the module docstring on one launch of sp -> (its buffers, the worst |cand - float64| / bound)."""
    o = launch(sp, group)
    M, idx, W = o['M'], o['idx'], sp.W
    base0 = int(idx[0])
    if not sp.live:                                            # nothing happens: flag 0 alone
        for key in ('tokens', 'next', 'logp', 'mass', 'rep', 'score', 'anc', 'bound', 'hist', 'cand'):
            if o[key] is not None:
                o[key].assert_untouched()
        _expect(o['flag'], 0, torch.zeros(1, dtype=torch.int32))
        assert int(o['pos'].item()) == sp.pos, label
        return o, 0.0
    # 1. cand_out against float64, exactly -inf off the candidate set
    cand = o['cand'].view.cpu().numpy()
    o['cand'].assert_only()
    low, worst = np.zeros(M, dtype=np.int64), 0.0
    for k in range(M):
        b = int(idx[k])
        toks = sp.candidates(b)
        low[k] = toks[0] if toks else 0
        want = R.cand64(float(sp.scores[b]), sp.rows[b].numpy(), toks)
        got = cand[k].astype(np.float64)
        dead = want == NINF
        assert np.all(got[dead] == NINF), (label, b, 'a non-candidate or dead candidate is not -inf')
        if (~dead).any():
            bound = lp_bounds(sp.rows[b])
            t = np.nonzero(~dead)[0]
            limit = bound[t] + C.U_FP32 * np.abs(want[t])
            err = np.abs(got[t] - want[t])
            assert np.all(err <= limit), (label, b, float((err / limit).max()))
            worst = max(worst, float((err / limit).max()))
    # 2. the selection is exactly the reference's function of cand_out
    anc, tok, sc, n, flag = R.select(cand, low, W)
    _expect(o['anc'], slice(0, M), torch.from_numpy(anc).view(1, -1))       # row indices of the launch's own stack
    _expect(o['score'], slice(0, M), torch.from_numpy(sc).view(1, -1))
    _expect(o['tokens'], sp.pos, torch.from_numpy(tok))
    _expect(o['flag'], 0, torch.tensor([flag], dtype=torch.int32))
    _expect(o['bound'], slice(0, 2), torch.tensor([[sp.pos, sp.col]], dtype=torch.int32))
    assert int(o['pos'].item()) == sp.pos + 1, label
    assert np.all(sc.reshape(-1, W)[:, :-1] >= sc.reshape(-1, W)[:, 1:]), label
    # 3. logp, tokens and next_in: the constrained sampler's bits for the ancestor row forced to the slot's token
    lp, nxt, stok = sampler_logp(sp, anc + base0, tok)
    assert torch.equal(stok.cpu(), torch.from_numpy(tok)), label
    _expect(o['next'], slice(0, D_), nxt)
    _expect(o['logp'], sp.col if sp.reads('logp') else None, lp)
    # logmass: the masked sampler's bits for the ancestor
    if o['mass'] is not None:
        _expect(o['mass'], sp.col if sp.reads('mass') else None, sampler_mass(sp)[torch.from_numpy(anc + base0)])
    # rule_report: the ancestor's value, read before any was written
    if o['rep'] is not None:
        before = o['rep'].before[GR:GR + M]
        _expect(o['rep'], sp.col if sp.reads('rep') else None,
                before[torch.from_numpy(anc.astype(np.int64)), sp.col] if sp.reads('rep') else None)
    if o['hist'] is not None:
        exp = o['hist'].before.clone()
        if 0 <= sp.col < sp.hist_rows:
            exp[GR + sp.col] = torch.from_numpy(anc).to(exp.device)
        assert same_bits(exp, o['hist'].full), label
    # a second launch on the same inputs: the same bits
    if again:
        o2 = launch(sp, group)
        for key in ('tokens', 'next', 'logp', 'mass', 'rep', 'score', 'anc', 'flag', 'bound', 'hist', 'cand'):
            if o[key] is not None:
                assert same_bits(o[key].full, o2[key].full), (label, key)
    o.update(anc_ref=anc + base0, tok_ref=tok, sc_ref=sc, n=n)
    return o, worst


def _modes(M, V, i, seed):
    """The i-th option mix of the grid: forced / free / mixed rows, sets with and without exclusion."""
    g = gen(seed)
    sets = random_sets(M, V, g)
    if M > 1:
        sets[1, :V] = False                                    # no bit inside the vocabulary: no restriction
    ex = tuple(sorted({0, V // 2, V - 1})) if V >= 4 else (V - 1,) if V >= 2 else ()
    return [dict(), dict(forced='all', sets=sets), dict(forced='mixed', exclude=ex), dict(sets=sets, exclude=ex),
            dict(forced='mixed', sets=sets, exclude=ex, scores='start')][i % 5]


@pytest.mark.parametrize('M,W', MW)
def test_select_against_float64_and_the_samplers(M, W):
    """The grid of group shapes and vocabularies, every option mix in turn.  Worst |cand - float64| / bound seen: 0.53."""
    worst = 0.0
    for i, V in enumerate(VS):
        for j in range(2):
            mode = _modes(M, V, i + 3 * j, 31 * M + V)
            sp = Spec(M, W, (V,), pos=1 + j, T=4, U=2, seed=1000 * M + 10 * V + j, **mode)
            _, w = check(sp, (M, W, V, sorted(mode)))
            worst = max(worst, w)
    print(f'worst cand ratio (M={M}, W={W}): {worst:.3f}')
    assert worst < 1.0


@pytest.mark.parametrize('M,W', [(3, 3), (64, 2), (64, 64)])
def test_several_voices_with_unequal_vocabularies(M, W):
    """nc = 4 with unequal vocabularies and NaN everywhere outside the position's voice; nc = 1 is the grid above."""
    widths = (5, 256, 1, 67)
    for pos in range(6):
        V = widths[pos % 4]
        mode = _modes(M, V, pos, 7 * M + pos)
        check(Spec(M, W, widths, pos=pos, T=8, U=4, seed=300 + 10 * M + pos, **mode), (M, W, pos), again=pos < 2)


def test_dead_slots_when_the_vocabulary_is_smaller_than_the_beam():
    for (M, W, V) in [(8, 4, 1), (8, 8, 2), (64, 64, 3), (6, 3, 2)]:
        sp = Spec(M, W, (V,), seed=40 + V, scores='start')      # one live row of V candidates: n = V < W
        o, _ = check(sp, (M, W, V))
        assert o['n'].tolist() == [min(V, W)] * (M // W)
        sc = o['sc_ref'].reshape(-1, W)
        assert np.all(sc[:, :min(V, W)] > NINF) and np.all(sc[:, min(V, W):] == NINF)
        assert np.all(o['anc_ref'].reshape(-1, W) == np.arange(0, M, W)[:, None])
        assert np.all(o['tok_ref'].reshape(-1, W)[:, min(V, W):] == o['tok_ref'].reshape(-1, W)[:, :1])


def test_infinite_rows_and_dead_groups():
    """A row of -inf logits has no live candidate (lp is NaN: -inf); a group of such rows, or of -inf scores, keeps the identity
    and every row emits its own lowest candidate token; -inf entries inside a live row are dead candidates."""
    M, W, V = 12, 4, 9
    sp = Spec(M, W, (V,), seed=5, exclude=(0, 1))
    sp.rows[1] = NINF                                           # one dead row in a live group
    sp.rows[4:8] = NINF                                         # a dead group: rows of -inf
    sp.scores[4:8] = torch.tensor([0.0, -1.0, NINF, -2.0])
    sp.scores[8:12] = NINF                                      # a dead group: scores of -inf
    sp.rows[2, 3:] = NINF
    sp.scores[0:4] = torch.tensor([-1.0, -0.5, -2.0, -3.0])
    o, _ = check(sp, 'dead')
    assert o['n'].tolist() == [4, 0, 0]
    assert o['anc_ref'][4:].tolist() == list(range(4, 12)) and o['tok_ref'][4:].tolist() == [2] * 8
    assert 1 not in o['anc_ref'][:4].tolist()
    # forced rows in a dead group emit their forced token
    sp = Spec(4, 4, (V,), seed=6, forced=torch.tensor([3, -1, 300, 0]), scores=torch.full((4,), NINF))
    o, _ = check(sp, 'dead forced')
    assert o['tok_ref'].tolist() == [3, 0, V - 1, 0] and o['n'].tolist() == [0]
    # every token excluded: no candidate at all, token 0
    sp = Spec(2, 2, (3,), seed=7, exclude=(0, 1, 2))
    o, _ = check(sp, 'all excluded')
    assert o['tok_ref'].tolist() == [0, 0] and o['n'].tolist() == [0]


def test_planted_exact_ties():
    """Identical rows with equal scores come out by row, equal logits inside a row by token."""
    M, W, V = 8, 4, 6
    sp = Spec(M, W, (V,), seed=8)
    sp.rows[0:4] = torch.tensor([1.0, 3.0, 3.0, -1.0, 3.0, 0.5])           # tokens 1, 2, 4 tie inside every row
    sp.scores[0:4] = torch.tensor([-1.0, -1.0, -2.0, -1.0])                # rows 0, 1, 3 tie
    sp.rows[4:8] = torch.zeros(V)
    sp.scores[4:8] = 0.0
    o, _ = check(sp, 'ties')
    assert o['anc_ref'].tolist() == [0, 0, 0, 1, 4, 4, 4, 4] and o['tok_ref'].tolist() == [1, 2, 4, 1, 0, 1, 2, 3]
    cand = o['cand'].view.cpu()
    assert len({float(cand[r, t]) for r in (0, 1, 3) for t in (1, 2, 4)}) == 1          # the ties are exact in cand_out
    # 64 identical rows, one group: the first row's tokens first
    sp = Spec(64, 64, (3,), seed=9, scores=torch.zeros(64))
    sp.rows[:] = torch.tensor([0.25, 0.25, 0.25])
    o, _ = check(sp, 'ties 64')
    assert o['anc_ref'].tolist() == [k // 3 for k in range(64)] and o['tok_ref'].tolist() == [k % 3 for k in range(64)]


@pytest.mark.parametrize('win', [None, 0, 3, -1])
def test_window_addressing_and_leading_dimensions(win):
    """win == NULL, win[1] >= 0 (the column is win[1] * U + pos) and win[1] < 0 (no live window: everything free, nothing recorded);
    then a column AT each leading dimension in turn: that buffer alone is free / unwritten."""
    M, W, V, U, pos = 6, 3, 7, 4, 2
    g = gen(3)
    base = dict(forced='mixed', sets=random_sets(M, V, g), exclude=(1,))
    sp = Spec(M, W, (V,), pos=pos, T=5, U=U, win=win, seed=60, **base)
    o, _ = check(sp, ('win', win))
    assert sp.col == {None: 2, 0: 2, 3: 14, -1: -1}[win]
    if win == -1:
        return
    for name in ('cons', 'allow', 'logp', 'mass', 'rep'):
        sp = Spec(M, W, (V,), pos=pos, T=5, U=U, win=win, seed=61, **{f'ld_{name}': max(sp.col, 5)}, **base)
        if win == 3:
            assert not sp.reads(name)
        check(sp, ('ld', win, name))
    check(Spec(M, W, (V,), pos=pos, T=5, U=U, win=win, seed=62, hist_rows=max(sp.col, 1), **base), ('hist', win))
    check(Spec(M, W, (V,), pos=pos, T=5, U=U, win=win, seed=63, hist_rows=0, report=False, mass=False, **base), ('none', win))


def test_nothing_happens_past_the_last_position():
    for pos in (4, 5, -1):
        check(Spec(4, 2, (5,), pos=pos, T=4, seed=70, forced='mixed'), ('past', pos))
    check(Spec(4, 2, (5,), pos=3, T=4, seed=71, forced='mixed'), 'last')


def test_a_group_alone_equals_the_group_among_twenty_one():
    M, W, V = 63, 3, 65
    g = gen(11)
    sp = Spec(M, W, (V,), pos=1, T=4, U=2, seed=80, forced='mixed', sets=random_sets(M, V, g), exclude=(2, 64))
    whole, _ = check(sp, 'whole')
    for grp in (0, 10, 20):
        one, _ = check(sp, ('alone', grp), group=grp, again=False)
        rows = slice(GR + grp * W, GR + (grp + 1) * W)
        for key in ('tokens', 'next', 'logp', 'mass', 'rep', 'cand'):
            assert same_bits(whole[key].full[rows], one[key].full[GR:GR + W]), (grp, key)
        assert same_bits(whole['score'].view[:, grp * W:(grp + 1) * W], one['score'].view), grp
        assert torch.equal(whole['anc'].view[:, grp * W:(grp + 1) * W] - grp * W, one['anc'].view), grp


def test_the_vectorised_bound_is_the_reference_bound():
    g = gen(12)
    for V in (1, 5, 256):
        row = torch.randn(V, generator=g) * 3
        if V > 2:
            row[1] = NINF
        b = lp_bounds(row)
        for v in range(0, V, max(1, V // 7)):
            assert abs(b[v] - C.logp_bound(row, v)) <= 1e-12 * max(1.0, C.logp_bound(row, v))


def test_bad_arguments_are_refused_before_any_launch():
    from vqcpc_bach_amd import hip
    sp = Spec(4, 2, (5,), seed=90)
    o = launch(sp)
    good = list(o['args']())

    def go(**kw):
        a = list(good)
        for i, v in kw.items():
            a[int(i[1:])] = v
        call('vqcpc_decode_beam_select', *a)
    for kw in (dict(a4=65), dict(a4=0), dict(a5=3), dict(a5=0), dict(a5=65), dict(a3=17), dict(a0=None), dict(a27=None),
               dict(a28=None), dict(a29=None), dict(a30=None), dict(a34=None), dict(a23=4097), dict(a19=3), dict(a12=3),
               dict(a22=4)):
        with pytest.raises(hip.VqcpcHipError, match='decode_beam_select'):
            go(**kw)
    offs = (ctypes.c_int32 * 2)(0, 257)
    with pytest.raises(hip.VqcpcHipError, match='1 <= V_c <= 256'):
        go(a2=offs, a1=300)
