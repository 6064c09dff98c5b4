"""vqcpc_decode_sample_constrained (csrc/decode.hip) by direct calls: bit-identity with vqcpc_decode_sample where the two
must agree (nothing forced / everything forced / the free positions of a mixed constraint), the log-probabilities against
float64 within the derived bound of tests/constrained_reference.py, the chorale-coordinate addressing through the device
window index, and the edges.  Conventions as in tests/test_decode_kernels_gpu.py: outputs sit in sentinel-filled allocations
with guard rows and a wider leading dimension, inputs the result must not depend on are NaN, seeds are fixed."""
import ctypes

import numpy as np
import pytest
import torch

import constrained_reference as C
from test_decode_kernels_gpu import GR, NAN, Buf, _i32_words, call, gen, same_bits

pytestmark = pytest.mark.gpu

D_ = 4                                       # width of the table rows
SAMPLING = dict(temperature=0.7, top_k=5, top_p=0.9)


@pytest.fixture(scope='module', autouse=True)
def _lib():
    from vqcpc_bach_amd import hip
    hip.load()
    return hip


class Case:
    """`steps` positions from pos0 of nc voices of the given widths: per step a logits matrix that is NaN outside the
    position's voice, one table, per-voice exclusion words, fixed seeds."""

    def __init__(self, M, widths, steps, U, T_, seed, pos0=0, exclude=None, scale=2.0):
        self.M, self.widths, self.steps, self.U, self.T, self.pos0 = M, tuple(widths), steps, U, T_, pos0
        self.nc = nc = len(widths)
        self.off = np.concatenate([[0], np.cumsum(widths)]).astype(int)
        self.offs = (ctypes.c_int32 * (nc + 1))(*self.off.tolist())
        self.ldl = int(self.off[-1]) + 6
        g = gen(seed)
        self.rows, self.lg = [], []
        for s in range(steps):
            c = (pos0 + s) % nc
            sl = torch.randn(M, widths[c], generator=g) * scale
            full = torch.full((M, self.ldl), NAN)
            full[:, self.off[c]:self.off[c + 1]] = sl
            self.rows.append(sl)
            self.lg.append(full.cuda())
        self.exclude_tokens = exclude or {}
        words = np.zeros(nc * 8, np.int64)
        for c, toks in self.exclude_tokens.items():
            for t in toks:
                words[c * 8 + t // 32] |= 1 << (t % 32)
        self.excl = _i32_words(words)
        self.table_rows = max(widths) * U + 1
        self.table = (torch.arange(self.table_rows, dtype=torch.float32).view(-1, 1) * 4
                      + torch.arange(D_, dtype=torch.float32)).cuda()
        self.seeds = (torch.arange(M, dtype=torch.int64) * 1000003 * 7919 + 17).cuda()

    def set_row(self, step, b, values):
        c = (self.pos0 + step) % self.nc
        self.rows[step][b] = values
        self.lg[step][b, self.off[c]:self.off[c + 1]] = values.cuda()

    def run(self, entry, teacher=None, constraint=None, ldcons=None, logp=None, ldlogp=None, win=None, sampling=SAMPLING,
            rows=None):
        """entry 'plain' (vqcpc_decode_sample, optional teacher (M, T)) or 'cons'.  rows: run these rows only (an M' = len(rows)
        call on the same logits, seeds and constraint rows).  -> dict of the outputs, guards included."""
        idx = torch.arange(self.M) if rows is None else torch.as_tensor(rows)
        M, T_ = len(idx), self.T
        pos = torch.full((1,), self.pos0, dtype=torch.int32, device='cuda')
        tokens = Buf(M, T_, T_ + 3, dtype=torch.int64)
        seeds = self.seeds[idx.cuda()].contiguous()
        nxt, prs = [], []
        for s in range(self.steps):
            n, p = Buf(M, D_, D_ + 3), Buf(M, 256, 256 + 4)
            lg = self.lg[s][idx.cuda()].contiguous()
            head = (lg, self.ldl, self.offs, self.nc, M, float(sampling['temperature']), int(sampling['top_k']),
                    float(sampling['top_p']), self.excl, seeds)
            tail = (tokens.view, T_ + 3, T_, self.table, self.table_rows, D_, self.U, n.view, D_ + 3, p.view, 256 + 4, pos)
            if entry == 'plain':
                call('vqcpc_decode_sample', *head, teacher, T_ if teacher is not None else 0, *tail)
            else:
                call('vqcpc_decode_sample_constrained', *head, constraint, ldcons or 0, logp, ldlogp or 0, win, *tail)
            torch.cuda.synchronize()
            n.assert_only(), p.assert_only()
            nxt.append(n.full.clone()), prs.append(p.full.clone())
        tokens.assert_only()
        return dict(tokens=tokens.full.clone(), tok=tokens.view.cpu().clone(), nxt=nxt, probs=prs, pos=int(pos.item()))


def assert_same_outputs(a, b, label):
    assert a['pos'] == b['pos'], label
    assert same_bits(a['tokens'], b['tokens']), label
    for s, (x, y) in enumerate(zip(a['nxt'], b['nxt'])):
        assert same_bits(x, y), (label, 'next_in', s)
    for s, (x, y) in enumerate(zip(a['probs'], b['probs'])):
        assert same_bits(x, y), (label, 'probs', s)


def _nan_logp(M, width, ld):
    return Buf(M, width, ld, data=torch.full((M, width), NAN))


def _check_logp(case, out, lp, cols, label):
    """logp column cols[s] of step s against float64 at the emitted token, within the derived bound."""
    worst = 0.0
    for s in range(case.steps):
        for b in range(case.M):
            tok = int(out['tok'][b, case.pos0 + s])
            row = case.rows[s][b]
            got, want, bound = float(lp[b, cols[s]]), C.logp_ref(row, tok), C.logp_bound(row, tok)
            if want == -float('inf'):
                assert got == want, (label, s, b)
                continue
            assert abs(got - want) <= bound, (label, s, b, got, want, bound)
            worst = max(worst, abs(got - want) / bound)
    return worst


VS = [1, 2, 13, 255, 256]


@pytest.mark.parametrize('M', [1, 16, 17, 64])
def test_constrained_sampler_against_the_plain_one(M):
    """Per V: nothing forced (all -1, and constraint == NULL) and everything forced are bit-identical to the plain sampler
    without / with `teacher`; in a mixed constraint the forced positions are exact and the free ones are the plain draws;
    logp is within the bound of float64 and row b's logp is bit-identical when the row runs alone."""
    steps = 4
    for V in VS:
        excl = {0: (1, 200) if V > 200 else (1,) if V >= 3 else (40,)}             # V < 3: a set bit past the vocabulary
        case = Case(M, (V,), steps, U=1, T_=steps + 2, seed=1000 * M + V, exclude=excl)
        T_ = case.T
        label = (M, V)
        plain = case.run('plain')
        assert plain['pos'] == steps
        g = gen(5 * M + V)
        forced = torch.randint(0, V, (M, T_), generator=g)
        taught = case.run('plain', teacher=forced.cuda())
        free = torch.full((M, T_), -1, dtype=torch.int64)

        lp = _nan_logp(M, T_, T_ + 2)
        out = case.run('cons', constraint=free.cuda(), ldcons=T_, logp=lp.view, ldlogp=T_ + 2)
        assert_same_outputs(out, plain, (label, 'all free'))
        assert_same_outputs(case.run('cons'), plain, (label, 'constraint NULL'))
        lp_free = lp.view.cpu().clone()
        exp = lp.before.clone()
        exp[GR:GR + M, :steps] = lp.view[:, :steps]
        assert same_bits(exp, lp.full) and bool(torch.isfinite(lp_free[:, :steps]).all()), label      # columns [0, steps) only
        _check_logp(case, out, lp_free, list(range(steps)), (label, 'free'))

        lp = _nan_logp(M, T_, T_ + 2)
        out = case.run('cons', constraint=forced.cuda(), ldcons=T_, logp=lp.view, ldlogp=T_ + 2)
        assert_same_outputs(out, taught, (label, 'all forced'))
        assert torch.equal(out['tok'][:, :steps], forced[:, :steps])
        _check_logp(case, out, lp.view.cpu(), list(range(steps)), (label, 'forced'))

        mask = torch.rand(M, T_, generator=g) < 0.5
        mixed = torch.where(mask, forced, torch.full_like(forced, -1 - V))
        lp = _nan_logp(M, T_, T_ + 2)
        out = case.run('cons', constraint=mixed.cuda(), ldcons=T_, logp=lp.view, ldlogp=T_ + 2)
        want = torch.where(mask, forced, plain['tok'])[:, :steps]                    # the logits do not depend on the prefix here
        assert torch.equal(out['tok'][:, :steps], want), label
        for s in range(steps):
            assert same_bits(out['probs'][s], plain['probs'][s]), (label, s)          # the filtered row, whatever is forced
            assert torch.equal(out['nxt'][s][GR:GR + M, :D_].cpu(), case.table.cpu()[want[:, s] * case.U + s % case.U])
        lp_mixed = lp.view.cpu().clone()
        _check_logp(case, out, lp_mixed, list(range(steps)), (label, 'mixed'))
        for b in sorted({0, M - 1}):                                                  # the row alone: M = 1
            lp1 = _nan_logp(1, T_, T_ + 2)
            alone = case.run('cons', constraint=mixed[b:b + 1].cuda(), ldcons=T_, logp=lp1.view, ldlogp=T_ + 2, rows=[b])
            assert torch.equal(alone['tok'][0], out['tok'][b]), (label, b)
            assert same_bits(lp1.view.cpu()[0, :steps], lp_mixed[b, :steps]), (label, b)


def test_constrained_sampler_with_several_voices():
    """nc = 4 voices of widths (1, 37, 256, 60), pos walked over two rounds and a step, per-voice exclusion words, a mixed
    constraint that forces some excluded tokens too: forced positions exact (an excluded token is still forced), free ones
    the plain draws, logp against float64 per voice."""
    widths, M, steps = (1, 37, 256, 60), 5, 9
    excl = {1: (0, 31, 32), 2: (0, 31, 32, 255), 3: (0, 31, 32)}
    case = Case(M, widths, steps, U=8, T_=12, seed=70, exclude=excl)
    plain = case.run('plain')
    g = gen(71)
    cons = torch.full((M, case.T), -1, dtype=torch.int64)
    for s in range(steps):
        V = widths[s % 4]
        pick = torch.rand(M, generator=g) < 0.5
        cons[:, s] = torch.where(pick, torch.randint(0, V, (M,), generator=g), cons[:, s])
    cons[0, 1], cons[1, 2], cons[2, 3] = 31, 255, 32                                  # excluded tokens, forced
    lp = _nan_logp(M, case.T, case.T + 5)
    out = case.run('cons', constraint=cons.cuda(), ldcons=case.T, logp=lp.view, ldlogp=case.T + 5)
    want = torch.where(cons >= 0, cons, plain['tok'])[:, :steps]
    assert out['pos'] == steps and torch.equal(out['tok'][:, :steps], want)
    for s in range(steps):
        assert same_bits(out['probs'][s], plain['probs'][s]), s
        assert torch.equal(out['nxt'][s][GR:GR + M, :D_].cpu(), case.table.cpu()[want[:, s] * case.U + s % case.U]), s
    _check_logp(case, out, lp.view.cpu(), list(range(steps)), 'voices')
    exp = lp.before.clone()
    exp[GR:GR + M, :steps] = lp.view[:, :steps]
    assert same_bits(exp, lp.full)
    assert_same_outputs(case.run('cons', constraint=torch.full_like(cons, -1).cuda(), ldcons=case.T), plain, 'voices, all free')


def test_logp_of_wide_and_infinite_rows():
    """V = 256: a row spanning +- 80 (most of its exponentials underflow in fp32), a row whose even entries are -inf, a row
    of one finite entry; forced onto the largest, the smallest and a -inf entry (logp = -inf exactly)."""
    V, M = 256, 6
    case = Case(M, (V,), 1, U=1, T_=2, seed=80, scale=3.0)
    wide = torch.linspace(-80.0, 80.0, V)[torch.randperm(V, generator=gen(81))]
    holes = torch.randn(V, generator=gen(82)) * 3.0
    holes[::2] = -float('inf')
    single = torch.full((V,), -float('inf'))
    single[77] = 0.3
    for b, row in enumerate((wide, wide, holes, holes, single, wide * 0.5)):
        case.set_row(0, b, row)
    cons = torch.full((M, 2), -1, dtype=torch.int64)
    cons[0, 0], cons[1, 0] = int(wide.argmax()), int(wide.argmin())
    cons[2, 0], cons[3, 0], cons[4, 0] = 1, 0, 77                                     # holes[0] = -inf
    lp = _nan_logp(M, 2, 5)
    out = case.run('cons', constraint=cons.cuda(), ldcons=2, logp=lp.view, ldlogp=5, sampling=dict(temperature=1.0, top_k=0,
                                                                                                    top_p=1.0))
    got = lp.view.cpu()
    assert out['tok'][:5, 0].tolist() == cons[:5, 0].tolist()
    worst = _check_logp(case, out, got, [0], 'wide')
    print(f'logp wide / -inf rows: worst |error| / bound = {worst:.3f}; logp = {got[:, 0].tolist()}')
    assert float(got[3, 0]) == -float('inf') and float(got[4, 0]) == 0.0
    assert float(got[1, 0]) < -150.0 and bool(torch.isfinite(got[[0, 1, 2, 4, 5], 0]).all())
    assert bool(torch.isnan(got[:, 1]).all())


@pytest.mark.parametrize('M', [3, 17])
def test_window_addressing(M):
    """win = {x, w0}: constraint and logp are read / written at column w0 * U + pos and nowhere else -- every other column
    of the constraint forces ANOTHER token, every other column of logp stays NaN.  win[1] = -1: nothing forced, nothing
    written.  A column at or past the leading dimension is free / not written."""
    V, U, S = 13, 4, 2
    T_, pos0, steps, w0, nbU = S * U, 5, 2, 3, 30
    case = Case(M, (V,), steps, U=U, T_=T_, seed=90 + M, pos0=pos0)
    plain = case.run('plain')
    assert plain['pos'] == pos0 + steps
    g = gen(91)
    decoy = torch.randint(0, V, (M, nbU), generator=g)
    cons = Buf(M, nbU, nbU + 3, data=decoy, dtype=torch.int64)
    cols = [w0 * U + pos0 + s for s in range(steps)]
    forced = (plain['tok'][:, pos0] + 1) % V                                           # differs from the free draw
    decoy[:, cols[0]], decoy[:, cols[1]] = forced, -1
    decoy[:, pos0] = (forced + 1) % V                                                  # what col = pos would read
    cons.view.copy_(decoy)
    cons.before = cons.full.clone()
    win = torch.tensor([99, w0], dtype=torch.int32).cuda()
    lp = _nan_logp(M, nbU, nbU + 2)
    out = case.run('cons', constraint=cons.view, ldcons=nbU + 3, logp=lp.view, ldlogp=nbU + 2, win=win)
    assert out['pos'] == pos0 + steps and win.tolist() == [99, w0]
    assert torch.equal(out['tok'][:, pos0], forced)
    assert torch.equal(out['tok'][:, pos0 + 1], plain['tok'][:, pos0 + 1])
    exp = lp.before.clone()
    exp[GR:GR + M, cols] = lp.view[:, cols]
    assert same_bits(exp, lp.full) and bool(torch.isfinite(lp.view[:, cols]).all())
    _check_logp(case, out, lp.view.cpu(), [c - 0 for c in cols], 'win')
    # col = pos without win: the decoy at column pos0 is what is forced
    assert torch.equal(case.run('cons', constraint=cons.view, ldcons=nbU + 3)['tok'][:, pos0], (forced + 1) % V)
    # no live window
    dead = torch.tensor([0, -1], dtype=torch.int32).cuda()
    lp2 = _nan_logp(M, nbU, nbU + 2)
    out = case.run('cons', constraint=cons.view, ldcons=nbU + 3, logp=lp2.view, ldlogp=nbU + 2, win=dead)
    assert_same_outputs(out, plain, 'win[1] = -1')
    lp2.assert_untouched()
    # a window whose columns lie past the leading dimensions: free, not written (never out of bounds)
    far = torch.tensor([0, 1000], dtype=torch.int32).cuda()
    out = case.run('cons', constraint=cons.view, ldcons=nbU + 3, logp=lp2.view, ldlogp=nbU + 2, win=far)
    assert_same_outputs(out, plain, 'window past ldcons')
    lp2.assert_untouched()
    cons.assert_untouched()


def test_nothing_happens_past_the_last_position():
    V, T_ = 13, 6
    case = Case(4, (V,), 1, U=1, T_=T_, seed=95, pos0=T_)
    cons = torch.zeros(4, T_ + 4, dtype=torch.int64).cuda()
    lp = _nan_logp(4, T_ + 4, T_ + 6)
    pos = torch.full((1,), T_, dtype=torch.int32, device='cuda')
    tokens, n, p = Buf(4, T_, T_ + 3, dtype=torch.int64), Buf(4, D_, D_ + 3), Buf(4, 256, 260)
    for value in (T_, T_ + 3, -1):
        pos.fill_(value)
        call('vqcpc_decode_sample_constrained', case.lg[0], case.ldl, case.offs, 1, 4, 1.0, 0, 1.0, None, case.seeds, cons, T_ + 4,
             lp.view, T_ + 6, None, tokens.view, T_ + 3, T_, case.table, case.table_rows, D_, 1, n.view, D_ + 3, p.view, 260, pos)
        torch.cuda.synchronize()
        assert int(pos.item()) == value
        for buf in (tokens, n, p, lp):
            buf.assert_untouched()


def test_bad_arguments_are_refused_before_any_launch():
    from vqcpc_bach_amd import hip
    case = Case(4, (13,), 1, U=1, T_=6, seed=96)
    T_ = case.T
    pos = torch.zeros(1, dtype=torch.int32, device='cuda')
    tokens, n = Buf(4, T_, T_, dtype=torch.int64), Buf(4, D_, D_)
    cons = torch.full((4, T_), -1, dtype=torch.int64).cuda()
    lp = _nan_logp(4, T_, T_)

    def go(M=4, seeds=case.seeds, ldcons=T_, ldlogp=T_, temperature=1.0, rows=case.table_rows):
        call('vqcpc_decode_sample_constrained', case.lg[0], case.ldl, case.offs, 1, M, temperature, 0, 1.0, None, seeds, cons,
             ldcons, lp.view, ldlogp, None, tokens.view, T_, T_, case.table, rows, D_, 1, n.view, D_, None, 0, pos)
    for kw in (dict(M=65), dict(seeds=None), dict(ldcons=T_ - 1), dict(ldlogp=T_ - 1), dict(temperature=0.0), dict(rows=12)):
        with pytest.raises(hip.VqcpcHipError, match='decode_sample_constrained'):
            go(**kw)
    torch.cuda.synchronize()
    assert int(pos.item()) == 0
    for buf in (tokens, n, lp):
        buf.assert_untouched()
    go()
    torch.cuda.synchronize()
    assert int(pos.item()) == 1
